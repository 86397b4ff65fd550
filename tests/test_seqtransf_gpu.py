"""sim_header 'seqTransf' on the GPU: the key-masked attention kernels, the head's forward (cc_seqtransf_forward_f32) inside
CLIP4Clip.get_similarity_logits and eval_epoch, and the head's training backward.  Every test here fails on a model that
refuses the head.

Kernel bounds (as tests/test_backward_gpu.py): the operands are fp16 values, computed from in float64; the result may
differ by the fp16 rounding of an fp16 output (2^-11 relative) plus 2^-24 x (the longest serial chain) x sum|terms|, with the
softmax's own error carried in: a score is a 64-term fp32 sum, its error moves P_ij by at most 2 x 64 x 2^-24 x
max_j sum_d |q_d k_jd| / 8 relative (plus a few units for exp and the division), and that factor joins the chain length.
Masked keys: their weights are exactly 0 by construction (their k / v rows are never read), so changing those rows leaves
every output bit-identical and their dk / dv rows are exactly 0 - no tolerance.

Module / eval: the project's parity contract (README), <= 1e-3 on L2-normalised pooled features and on cosine similarities
(logits / exp(logit_scale)), against the float64 restatement tests/seqtransf_ref.py (pinned to the reference's float64 run by
tests/test_seqtransf_host.py) on the same features."""
import os
import sys

import numpy as np
import pytest
import torch

import seqtransf_ref as ref
from centerclip_amd import torch_ops  # noqa: F401  (registers torch.ops.centerclip.*)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H = 2.0 ** -11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LS = [1, 3, 4, 12, 64, 77]
HEADS = 8


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


# ------------------------------------------------------------------------------------------------ kernels
def _att_case(L, seed, nseq=3):
    g = torch.Generator().manual_seed(seed)
    W = 64 * HEADS
    qkv = (torch.randn(nseq * L, 3 * W, generator=g) * 0.7).half()
    mask = (torch.rand(nseq, L, generator=g) < 0.6).long()
    mask[:, 0] = torch.randint(0, 2, (nseq,), generator=g)
    mask[0] = 1                                          # no padding
    if nseq > 2:
        mask[2] = 0                                      # every key masked: the unmasked softmax
        mask[1, int(torch.randint(0, L, (1,), generator=g))] = 1
    return qkv, mask


def _split(qkv, nseq, L):
    W = qkv.shape[1] // 3
    t = qkv.double().view(nseq, L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)       # [3, nseq, H, L, 64]
    return t[0], t[1], t[2]


def _ref_mask(mask):
    m = mask.clone()
    m[m.sum(1) == 0] = 1                                  # all masked: -1e6 on every score cancels (the exact value)
    return m


def _strided(mask):
    """The mask as a strided view (every other column of a wider tensor), as the segment mask after clustering is."""
    wide = torch.zeros(mask.shape[0], 2 * mask.shape[1], dtype=torch.long)
    wide[:, 1::2] = mask
    return wide.to(DEV)[:, 1::2]


@pytest.mark.parametrize("L", LS)
def test_key_masked_attention_forward_against_float64(L):
    nseq = 3
    qkv, mask = _att_case(L, 10 + L, nseq)
    m = _strided(mask)
    out = torch.ops.centerclip.key_masked_attention(qkv.to(DEV), m, nseq, L, HEADS).cpu().double()
    q, k, v = _split(qkv, nseq, L)
    live = _ref_mask(mask).bool()[:, None, None, :]
    s = q @ k.transpose(-1, -2) / 8
    p = torch.softmax(s.masked_fill(~live, -float("inf")), -1)
    o = (p @ v).transpose(1, 2).reshape(nseq * L, 64 * HEADS)
    smax = ((q.abs() @ k.abs().transpose(-1, -2)) / 8).masked_fill(~live, 0).amax(-1, keepdim=True)     # [n, H, L, 1]
    chain = L + 16 + 2 * 64 * smax                                                                      # (in units of U)
    pv = (p @ v.abs())
    bound = H * o.abs() + (U * chain * pv).transpose(1, 2).reshape(nseq * L, 64 * HEADS)
    err = (out - o).abs()
    print("L %2d  max|d| %.2e  max(|d| / bound) %.3f" % (L, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    # masked keys' k / v rows: any value, the same bits
    qkv2 = qkv.clone().view(nseq, L, 3, 64 * HEADS)
    dead = ~_ref_mask(mask).bool()
    qkv2[:, :, 1:][dead] = torch.randn(int(dead.sum()), 2, 64 * HEADS).half() * 100
    out2 = torch.ops.centerclip.key_masked_attention(qkv2.view(nseq * L, -1).to(DEV), m, nseq, L, HEADS).cpu().double()
    assert torch.equal(out, out2)


@pytest.mark.parametrize("L", LS)
def test_key_masked_attention_backward_against_float64(L):
    nseq = 3
    qkv, mask = _att_case(L, 20 + L, nseq)
    m = _strided(mask)
    g = torch.Generator().manual_seed(L)
    dout = torch.randn(nseq * L, 64 * HEADS, generator=g)
    amax = torch.zeros(1, device=DEV)
    d = torch.ops.centerclip.key_masked_attention_backward(qkv.to(DEV), m, dout.to(DEV), nseq, L, HEADS, amax).cpu().double()
    q, k, v = _split(qkv, nseq, L)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    live = _ref_mask(mask).bool()[:, None, None, :]
    s = q @ k.transpose(-1, -2) / 8
    p = torch.softmax(s.masked_fill(~live, -float("inf")), -1)
    o = p @ v
    dO = dout.double().view(nseq, L, HEADS, 64).transpose(1, 2)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), dO)
    with torch.no_grad():
        dP = dO @ v.transpose(-1, -2)
        D = (p * dP).sum(-1, keepdim=True)
        A = dO.abs() @ v.abs().transpose(-1, -2)
        Bi = (p * dP.abs()).sum(-1, keepdim=True)
        C = p * (A + Bi) + p * (dP - D).abs()
        smax = ((q.abs() @ k.abs().transpose(-1, -2)) / 8).masked_fill(~live, 0).amax(-1, keepdim=True)
        chain = L + 96 + 2 * 64 * smax
        b_dq = U * chain * (C @ k.abs()) / 8
        b_dk = U * (C * chain).transpose(-1, -2) @ q.abs() / 8
        b_dv = U * (p * chain).transpose(-1, -2) @ dO.abs()
    got = d.view(nseq, L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    for name, gg, rr, bb in (("dq", got[0], dq, b_dq), ("dk", got[1], dk, b_dk), ("dv", got[2], dv, b_dv)):
        err = (gg - rr).abs()
        print("L %2d %s max|d| %.2e  max(|d| / bound) %.3f" % (L, name, float(err.max()), float((err / bb.clamp_min(1e-300)).max())))
        assert bool((err <= bb).all()), name
    # masked keys: dk and dv rows exactly 0
    dead = ~_ref_mask(mask).bool()
    rows = d.view(nseq, L, 3, 64 * HEADS)[dead]
    assert bool((rows[:, 1:] == 0).all())
    assert float(amax) == float(d.abs().max())


def test_key_masked_attention_refusals():
    qkv = torch.zeros(81 * 2, 3 * 128, device=DEV, dtype=torch.float16)
    from centerclip_amd import _lib as L
    with pytest.raises(L.CenterClipHipError, match="cc_key_masked_attention_f16"):
        torch.ops.centerclip.key_masked_attention(qkv, torch.ones(2, 81, dtype=torch.long, device=DEV), 2, 81, 2)
    assert L.lib().cc_key_masked_attention_f16(L.ptr(qkv), L.ptr(qkv), 2, 81, 2, 128, L.ptr(qkv), 81, 1, None) == -2
    assert L.lib().cc_key_masked_attention_f16(L.ptr(qkv), L.ptr(qkv), 2, 80, 2, 96, L.ptr(qkv), 80, 1, None) == -1
    with pytest.raises(ValueError):
        torch.ops.centerclip.key_masked_attention(qkv[:8], torch.ones(2, 4, dtype=torch.int32, device=DEV), 2, 4, 2)


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model():
    from centerclip_amd.clip4clip import CLIP4Clip
    b = _bench()
    c = b.CFG2
    args = b.task_config(c)
    args.sim_header, args.cross_num_hidden_layers = "seqTransf", 4
    m = CLIP4Clip.from_state_dict(b.random_state_dict(c, seed=0), args).to(DEV).eval()
    with torch.no_grad():                                    # a head that is not just the text blocks: perturb every weight
        g = torch.Generator().manual_seed(3)
        for p in list(m.transformerClip.parameters()) + [m.frame_position_embeddings.weight]:
            p.add_((torch.randn(p.shape, generator=g) * 0.02).to(DEV))
    return m


def _ref_head(model, vis, mask):
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items() if not k.startswith("clip.")}
    blocks = ref.blocks_from_state(sd, model.transformerClip.layers)
    return ref.head(vis.double().cpu(), mask.cpu(), sd["frame_position_embeddings.weight"], blocks, model.transformerClip.heads)


@pytest.mark.parametrize("B,T", [(16, 3), (64, 12), (8, 64), (2, 77)])
def test_similarity_logits_against_float64(model, B, T):
    g = torch.Generator().manual_seed(B * 100 + T)
    vis = torch.randn(B, T, 512, generator=g)
    seq = torch.randn(B + 3, 1, 512, generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for b in range(1, B, 2):
        mask[b, int(torch.randint(1, T + 1, (1,), generator=g)):] = 0
    wide = torch.zeros(B, 4 * T, dtype=torch.long)                    # the strided segment mask of a clustered model
    wide[:, 3::4] = mask
    vm = wide.to(DEV)[:, 3::4]
    with torch.no_grad():
        lg, _ = model.get_similarity_logits(seq.to(DEV), vis.to(DEV), None, vm, shaped=True)
        h = model.seq_head(vis.to(DEV), vm).cpu().double()
    ls = float(model.clip.logit_scale)
    r = _ref_head(model, vis, mask)
    pooled = ref.pooled(h, mask)
    pooled_ref = ref.pooled(r, mask)
    t = seq.squeeze(1).double()
    cos_ref = (t / t.norm(dim=-1, keepdim=True)) @ pooled_ref.t()
    dp = float((pooled - pooled_ref).abs().max())
    dc = float((lg.cpu().double() / np.exp(ls) - cos_ref).abs().max())
    print("B %d T %d  pooled %.2e  cosine %.2e" % (B, T, dp, dc))
    assert dp <= 1e-3 and dc <= 1e-3


def test_masked_frames_and_masked_videos_do_not_leak(model):
    B, T = 8, 12
    g = torch.Generator().manual_seed(9)
    vis = torch.randn(B, T, 512, generator=g).to(DEV)
    seq = torch.randn(B, 1, 512, generator=g).to(DEV)
    mask = torch.ones(B, T, dtype=torch.long, device=DEV)
    mask[1, 5:] = 0
    mask[4, 2:] = 0
    with torch.no_grad():
        lg, _ = model.get_similarity_logits(seq, vis, None, mask, shaped=True)
        vis2 = vis.clone()
        vis2[mask == 0] = torch.randn(int((mask == 0).sum()), 512, generator=g).to(DEV) * 10
        lg2, _ = model.get_similarity_logits(seq, vis2, None, mask, shaped=True)
        assert torch.equal(lg, lg2)                               # masked frames' features: the same bits
        h = model.seq_head(vis, mask)
        m3 = mask.clone()
        m3[6] = 0                                                 # one video fully masked: no fault, the others unchanged
        h3 = model.seq_head(vis, m3)
        torch.cuda.synchronize()
        keep = torch.arange(B, device=DEV) != 6
        assert torch.equal(h[keep], h3[keep]) and bool(torch.isfinite(h3[6]).all())


def test_in_place_weight_change_is_seen(model):
    g = torch.Generator().manual_seed(4)
    vis = torch.randn(4, 3, 512, generator=g).to(DEV)
    mask = torch.ones(4, 3, dtype=torch.long, device=DEV)
    w = model.transformerClip.resblocks[1].mlp["c_proj"].weight
    with torch.no_grad():
        h0 = model.seq_head(vis, mask)
        w.mul_(1.5)
        h1 = model.seq_head(vis, mask)
        w.div_(1.5)
        p = model.frame_position_embeddings.weight
        p[1].add_(0.5)
        h2 = model.seq_head(vis, mask)
        p[1].sub_(0.5)
    assert not torch.equal(h0, h1) and not torch.equal(h0, h2)
    r = _ref_head(model, vis, mask)
    assert float((h0.cpu().double() - r).abs().max()) <= 1e-2 * float(r.abs().max())


def _loader(n, seed):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from eval_synthetic import SyntheticRetrieval
    ds = SyntheticRetrieval(n, seed=seed)
    ds.vmask[1, 0, 7:] = 0
    ds.vmask[5, 0, 4:] = 0                        # (segment 0 keeps its last frame: every video has a live segment)
    return torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False)


def _sim_matrix(model, loader, **kw):
    from centerclip_amd import eval as ceval
    seen = {}
    orig = ceval._sharded_metrics

    def grab(core, cache, *a):
        seen["video"] = torch.cat(cache.video).clone()
        seen["text"] = torch.cat(cache.text).clone()
        return orig(core, cache, *a)
    ceval._sharded_metrics = grab
    try:
        ceval.eval_epoch(model, loader, DEV, **kw)
    finally:
        ceval._sharded_metrics = orig
    return seen


def test_eval_epoch_modes_agree_and_apply_the_head(model):
    from centerclip_amd.eval import HipBackend
    loader = _loader(24, 1)
    base = _sim_matrix(model, loader, in_flight=1)
    for kw in (dict(), dict(in_flight=3), dict(in_flight=1, graphed=True), dict(in_flight=2, graphed=True),
               dict(in_flight=1, shard=True)):
        got = _sim_matrix(model, loader, **kw)
        dv = (got["video"].float() - base["video"].float()).abs()
        print(kw, "identical:", torch.equal(got["video"], base["video"]), "max|d| per batch:",
              [float(dv[i:i + 8].max()) for i in range(0, dv.shape[0], 8)], "text identical:", torch.equal(got["text"], base["text"]))
        assert torch.equal(got["video"], base["video"]) and torch.equal(got["text"], base["text"]), kw
    # the cached video rows are the head's output pooled (not meanP's)
    batch = next(iter(loader))
    ids, am, seg, video, vm = (t.to(DEV) for t in batch)
    with torch.no_grad():
        vis = model(ids, seg, am, video, vm)["visual_output"]
        vmask = model.get_video_mask_after_cluster(vm.view(-1, vm.shape[-1]))
        head_rows = HipBackend.video_operand(model.seq_head(vis, vmask).contiguous(), vmask.contiguous())
        meanp_rows = HipBackend.video_operand(vis.contiguous(), vmask.contiguous())
    assert torch.equal(base["video"][:8], head_rows) and not torch.equal(head_rows, meanp_rows)


# ------------------------------------------------------------------------------------------------ training
def test_training_head_gradients_and_exact_zeros(model):
    """seq_head_train: rows of the position table behind T and masked frames' features get exactly zero gradient; the
    head's gradients agree with float64 autograd of the restatement, each relative to its own largest entry.  Measured worst on
    an MI355X: 1.20e-3 (B = 16, T = 3, 4 blocks of width 512); the bound is twice that, under the 2.5e-2 cap of
    tests/test_train_full_gpu.py."""
    from centerclip_amd import train as cctrain
    model.train()
    try:
        B, T = 16, 3
        g = torch.Generator().manual_seed(12)
        vis = torch.randn(B, T, 512, generator=g).to(DEV).requires_grad_(True)
        mask = torch.ones(B, T, dtype=torch.long, device=DEV)
        mask[-1, 2:] = 0
        w = torch.randn(B, T, 512, generator=g).to(DEV)
        for p in model.parameters():
            p.grad = None
        out = cctrain.seq_head_train(model, vis, mask)
        ((out * w)[mask.bool()]).sum().backward()
        gpos = model.frame_position_embeddings.weight.grad
        assert gpos is not None and not gpos[T:].any()
        assert not vis.grad[-1, 2:].any()
        # float64 reference of the same scalar
        sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items() if not k.startswith("clip.")}
        blocks = ref.blocks_from_state(sd, model.transformerClip.layers)
        v64 = vis.detach().double().cpu().requires_grad_(True)
        r = ref.head(v64, mask.cpu(), sd["frame_position_embeddings.weight"], blocks, model.transformerClip.heads)
        ((r * w.double().cpu())[mask.cpu().bool()]).sum().backward()
        worst = 0.0
        named = dict(model.named_parameters())
        for k, t in list(sd.items()) + [("vis", v64)]:
            got = (vis.grad if k == "vis" else named[k].grad).double().cpu()
            e = float((got - t.grad).abs().max()) / max(float(t.grad.abs().max()), 1e-30)
            worst = max(worst, e)
            assert e <= 2.4e-3, (k, e)
        print("worst relative gradient error %.2e" % worst)
    finally:
        model.eval()
