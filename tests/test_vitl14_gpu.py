"""ViT-L/14 on the GPU (``-m gpu``): the patch gather for a patch size off the 8-wide grid, the streaming attention for
256 < L <= 640, the attention backward's fifth key tile (L <= 320), the encoders and the training towers at a tiny L/14
geometry (patch 14, 224 px: 257 tokens per frame) and one block stack at the real width (1024, 16 heads).

Bounds are the ones the project already states for the same quantities: test_clip_gpu.test_attention's 4e-3 of the largest
output entry, test_r4_gpu.test_attention_backward_on_the_matrix_cores' 2e-3 per q / k / v part, SURVEY.md 8c's 1e-3 on
L2-normalised embeddings, test_train_full_gpu's per-group gradient bounds of the ViT-B/16 step (the two-launch attention
backward, as here)."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import torch_ops  # noqa: F401  (registers torch.ops.centerclip)
from oracle import clip_oracle as clo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vitl14_attention_l256.npz")


# ------------------------------------------------------------------------------------------------ patch gather
def _gather(entry, data_ptr, fmt, F, res, p, cols):
    """cc_patch_gather_f16 / cc_patch_gather_any_f16 through ctypes into a buffer with a guard region -> (status, matrix, guard)."""
    from centerclip_amd import _lib as L
    from centerclip_amd._lib_clip import Frames
    fr = Frames()
    fr.data, fr.format = data_ptr, fmt
    fr.mean = (ctypes.c_float * 3)(*clo.PIXEL_MEAN)
    fr.std = (ctypes.c_float * 3)(*clo.PIXEL_STD)
    rows = F * (res // p) ** 2
    out = torch.full((rows * cols + 4096,), 7.0, dtype=torch.float16, device=DEV)
    rc = getattr(L.lib(), entry)(ctypes.byref(fr), F, res, p, L.ptr(out), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, out[:rows * cols].view(rows, cols).cpu(), out[rows * cols:].cpu()


def _patch_rows(x, p):
    """[F, 3, H, W] fp32 -> the patch matrix [F * g * g, 3 p^2], columns (c, kh, kw): the oracle's reshape."""
    F, g = x.shape[0], x.shape[-1] // p
    return x.view(F, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F * g * g, 3 * p * p)


@pytest.mark.parametrize("res,F", [(28, 2), (224, 3)])
@pytest.mark.parametrize("kind", ["f32", "f32+1", "u8_chw", "u8_chw+1", "u8_hwc"])
def test_patch_gather_p14(res, F, kind):
    """Patch 14: rows 28 / 56 bytes apart, with the base moved by one element so that rows start off every alignment.  The
    first 588 columns are the fp16 rounding of the loader's fp32 values, bit for bit (the comparison the p = 32 / 16 gather
    tests make); columns 588 .. 639 are exact zeros; nothing is written behind the matrix."""
    p, cols = 14, 640
    gen = torch.Generator().manual_seed(res + len(kind))
    off = 1 if kind.endswith("+1") else 0
    if kind.startswith("f32"):
        x = torch.randn(F, 3, res, res, generator=gen)
        ref, fmt = x, 0
        buf = torch.empty(x.numel() + off, device=DEV)
    else:
        hwc = kind == "u8_hwc"
        x = torch.randint(0, 256, (F, res, res, 3) if hwc else (F, 3, res, res), dtype=torch.uint8, generator=gen)
        ref, fmt = clo.loader_normalize(x, channels_last=hwc), 2 if hwc else 1
        buf = torch.empty(x.numel() + off, dtype=torch.uint8, device=DEV)
    buf[off:].copy_(x.reshape(-1))
    ptr = buf.data_ptr() + off * buf.element_size()
    assert ptr % (16 if fmt == 0 else 8) == (off * buf.element_size())          # the offset really breaks the vector alignment
    rc, a, guard = _gather("cc_patch_gather_any_f16", ptr, fmt, F, res, p, cols)
    assert rc == 0
    want = _patch_rows(ref, p).half()
    assert torch.equal(a[:, :588], want)
    assert not a[:, 588:].any() and bool((guard == 7.0).all())
    if off == 0:                                                                  # the op the training towers call
        op = torch.ops.centerclip.patch_gather(x.to(DEV), res, p).cpu()
        assert op.shape == (F * (res // p) ** 2, cols) and torch.equal(op, a)


@pytest.mark.parametrize("p", [32, 16])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_patch_gather_p32_p16_bits_are_those_of_the_old_entry(p, fmt):
    """p % 8 == 0: the dispatcher for any patch size gives the bits of cc_patch_gather_f16 (3 p^2 columns, no padding), and keeps
    its refusal of a base off the 8-wide loads' grid."""
    res, F = 64, 3
    gen = torch.Generator().manual_seed(p + fmt)
    if fmt == 0:
        x = torch.randn(F, 3, res, res, generator=gen).to(DEV)
    else:
        x = torch.randint(0, 256, (F, res, res, 3) if fmt == 2 else (F, 3, res, res), dtype=torch.uint8, generator=gen).to(DEV)
    cols = 3 * p * p
    rc0, old, g0 = _gather("cc_patch_gather_f16", x.data_ptr(), fmt, F, res, p, cols)
    rc1, new, g1 = _gather("cc_patch_gather_any_f16", x.data_ptr(), fmt, F, res, p, cols)
    assert rc0 == 0 and rc1 == 0 and torch.equal(old, new) and bool((g0 == 7.0).all()) and bool((g1 == 7.0).all())
    assert float(old.float().abs().max()) > 0
    assert torch.equal(torch.ops.centerclip.patch_gather(x, res, p).cpu(), old)
    assert _gather("cc_patch_gather_any_f16", x.data_ptr() + x.element_size(), fmt, F, res, p, cols)[0] == -1


# ------------------------------------------------------------------------------------------------ attention forward
def _attention_ref(qkv, nseq, L, heads, causal, lens=None):
    """float64 softmax attention on the same fp16 qkv, on the device -> [nseq * L, W] (rows behind a sequence's length: 0)."""
    W = heads * 64
    q, k, v = qkv.double().view(nseq, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-2, -1) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64, device=qkv.device).triu_(1)
    if lens is not None:
        for i, n in enumerate(lens):
            s[i, :, :, n:] = float("-inf")
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(nseq, L, W)
    if lens is not None:
        for i, n in enumerate(lens):
            ref[i, n:] = 0
    return ref.reshape(nseq * L, W)


def _qkv(nseq, L, heads, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(nseq * L, 3 * heads * 64, generator=gen) * 1.5).half().to(DEV)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [257, 289, 320, 321, 577, 640])
def test_attention_long(L, causal):
    """256 < L <= 640 (streamed key tiles, online softmax) against float64 on the same fp16 q, k, v: test_attention's measure
    and bound - max |delta| below 4e-3 of the largest output entry."""
    from centerclip_amd import ops
    nseq, heads = 2, 2
    qkv = _qkv(nseq, L, heads, L * 7 + heads)
    ref = _attention_ref(qkv, nseq, L, heads, causal)
    y = ops.attention_f16(qkv, nseq, L, heads, causal)
    err, top = float((y.double() - ref).abs().max()), float(ref.abs().max())
    print("L %d causal %d: max|d| %.3e = %.3e of the largest entry" % (L, causal, err, err / top))
    assert err < 4e-3 * top
    # the LND row order ResidualAttentionBlock.forward uses (seq_rows = 1, tok_rows = nseq): the same numbers, permuted
    lnd = qkv.view(nseq, L, -1).permute(1, 0, 2).contiguous().view(nseq * L, -1)
    y2 = ops.attention_f16(lnd, nseq, L, heads, causal, seq_rows=1, tok_rows=nseq)
    assert torch.equal(y2.view(L, nseq, -1).permute(1, 0, 2).reshape(nseq * L, -1), y)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_long_with_sequence_lengths(causal):
    """The seq_len / seq_off form of AttArgs (lengths 257 and 40, packed back to back) through the in_proj + attention block of
    the encoders is not reachable above 256 tokens from Python, so the lengths go through the C launcher's own entry: rows of
    two sequences of different length in one launch, sized by the upper bound 257."""
    from centerclip_amd import _lib as L_
    lens, heads, W = (257, 40), 2, 128
    qkv = _qkv(1, sum(lens), heads, 99)
    out = torch.zeros(sum(lens), W, dtype=torch.float16, device=DEV)
    off = torch.tensor([0, lens[0]], dtype=torch.int32, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    L_.check(L_.lib().cc_attention_varlen_f16(L_.ptr(qkv), L_.ptr(out), 2, max(lens), heads, W, int(causal), L_.ptr(off), L_.ptr(ln),
                                              L_.stream_ptr(torch.device(DEV))), "cc_attention_varlen_f16")
    torch.cuda.synchronize()
    row = 0
    for n in lens:
        part = qkv[row:row + n]
        ref = _attention_ref(part, 1, n, heads, causal)
        err = float((out[row:row + n].double() - ref).abs().max())
        assert err < 4e-3 * float(ref.abs().max()), (n, err)
        row += n


def test_attention_641_is_refused():
    from centerclip_amd import ops, _lib as L_
    with pytest.raises(L_.CenterClipHipError, match="(?i)unsupported"):
        ops.attention_f16(_qkv(1, 641, 1, 1), 1, 641, 1, False)


def test_attention_256_keeps_its_bits():
    """L = 256 runs the resident-K kernel it ran before: the output recorded from the commit before the streaming kernel
    (tests/golden/vitl14_attention_l256.npz: the fp16 output for this generator's input), bit for bit, both mask forms."""
    from centerclip_amd import ops
    g = np.load(GOLDEN)
    qkv = _qkv(2, 256, 2, 256)
    assert np.array_equal(qkv.cpu().numpy().view(np.uint16)[:4, :8], g["qkv_head"])           # the same input as recorded
    for causal in (False, True):
        y = ops.attention_f16(qkv, 2, 256, 2, causal).cpu().numpy().view(np.uint16)
        assert np.array_equal(y, g["out_causal" if causal else "out"])


# ------------------------------------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [257, 320])
def test_attention_backward_long(L, causal):
    """256 < L <= 320: the query-side / key-side pair with a fifth key tile against float64 autograd on the same fp16 q, k, v -
    test_attention_backward_on_the_matrix_cores' measure and bound (every part of d_qkv within 2e-3 of its largest entry,
    gradients of tiny magnitude included)."""
    from centerclip_amd import _lib as L_
    from centerclip_amd.torch_ops import _st
    nseq, heads = 2, 2
    W = heads * 64
    g = torch.Generator().manual_seed(nseq * 100 + L)
    qkv = torch.randn(nseq * L, 3 * W, generator=g).to(DEV).half()
    for mag in (1.0, 3e-7):
        d_out = (torch.randn(nseq * L, W, generator=g) * mag).to(DEV)
        d_out.view(nseq, L, W)[0] *= 64.0
        got = torch.empty(nseq * L, 3 * W, device=DEV)
        am = torch.zeros(2, device=DEV)
        nb = L_.lib().cc_attention_backward_workspace_bytes(nseq, L, heads)
        assert nb == nseq * L * heads * 8
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        L_.check(L_.lib().cc_attention_backward_f16(L_.ptr(qkv), L_.ptr(d_out), L_.ptr(got), nseq, L, heads, W, int(causal),
                                                    L_.ptr(am), L_.ptr(ws), nb, _st(got)), "cc_attention_backward_f16")
        x = qkv.double().view(nseq, L, 3, heads, 64).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)
        sc = x[0] @ x[1].transpose(-1, -2) / 8.0
        if causal:
            sc = sc + torch.full((L, L), float("-inf"), device=DEV, dtype=torch.float64).triu_(1)
        out = (sc.softmax(dim=-1) @ x[2]).permute(0, 2, 1, 3).reshape(nseq * L, W)
        (out * d_out.double()).sum().backward()
        want = x.grad.permute(1, 3, 0, 2, 4).reshape(nseq * L, 3 * W)
        torch.cuda.synchronize()
        for part in range(3):
            a, b = got[:, part * W:(part + 1) * W].double(), want[:, part * W:(part + 1) * W]
            err = float((a - b).abs().max()) / float(b.abs().max())
            print("L %d causal %d mag %g part %d: %.3e" % (L, causal, mag, part, err))
            assert err <= 2e-3, (part, mag)
            # the same measure per (sequence, head) against that head's own largest entry (the fp16 scales are per head)
            errh = (a - b).abs().view(nseq, L, heads, 64).amax(dim=(1, 3))
            toph = b.abs().view(nseq, L, heads, 64).amax(dim=(1, 3))
            assert bool((errh <= 2e-3 * toph).all()), (part, mag, (errh / toph).tolist())
        assert float(am[0]) == float(got.abs().max())


def test_attention_backward_321_is_refused():
    from centerclip_amd import _lib as L_
    from centerclip_amd.train import block as tb
    p = torch.zeros(16, device=DEV)
    rc = L_.lib().cc_attention_backward_f16(L_.ptr(p), L_.ptr(p), L_.ptr(p), 1, 321, 1, 64, 0, None, L_.ptr(p), 1 << 30, None)
    with pytest.raises(L_.CenterClipHipError, match="(?i)unsupported"):
        L_.check(rc, "cc_attention_backward_f16")
    from centerclip_amd.clip import ResidualAttentionBlock
    blk = ResidualAttentionBlock(64, 1).to(DEV)
    with pytest.raises(NotImplementedError, match="321 tokens"):
        tb.block_forward_train(blk, torch.zeros(321, 1, 64, device=DEV))


# ------------------------------------------------------------------------------------------------ towers, evaluation
def _tiny_sd(width=128, layers=3, embed=64, seed=0):
    """Random weights of a small CLIP with ViT-L/14's patch geometry (patch 14, 224 px: 257 tokens), rounded through fp16."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(seed)
    m = CLIP(embed, 224, layers, width, 14, 77, 512, 128, 2, 2, args=None)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _ids(B, seed=1):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, 32, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(4, 33, (1,), generator=gen))
        ids[b, 0], ids[b, n - 1] = 510, 511
        ids[b, 1:n - 1] = torch.randint(1, 500, (n - 2,), generator=gen)
    return ids


def _cluster_args(T):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T, 1, 1],
                     cluster_num_blocks=[256, 64, 64], cluster_distance='euclidean', cluster_threshold=1e-6,
                     cluster_iter_limit=100, minkowski_norm_p=2.0, pretrained_clip_name='ViT-L/14', aggregation=None,
                     pre_norm=False)


@pytest.fixture(scope="module")
def tiny_eval():
    """The tiny geometry, B = 1, T = 2: the oracle's embeddings without clustering and with a cluster module at block 2
    (2 -> 1 frames, K = 64 of N = 512 tokens), its medoids, the hidden states - computed once."""
    sd = _tiny_sd()
    video = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).half().float()
    ids = _ids(2)
    plain, plain_h = clo.visual_forward(sd, video, 2, return_hidden=True)
    clus, clus_h, med = clo.visual_forward(sd, video, 2, cluster_plan={1: (1, 64)}, return_hidden=True, return_medoids=True)
    return dict(sd=sd, video=video, ids=ids, plain=plain, plain_h=plain_h, clus=clus, clus_h=clus_h, med=med[1],
                text=clo.text_forward(sd, ids))


def _nrm(x):
    return x / x.norm(dim=-1, keepdim=True)


def _emb_err(a, b):
    return float((_nrm(a.detach().cpu().float()) - _nrm(b.float())).abs().max())


@pytest.mark.parametrize("clustered", [False, True])
def test_tiny_l14_encoders_against_the_oracle(tiny_eval, clustered):
    """encode_image, encode_pair, return_hidden, the prefix encoder and a replica at L = 257: without clustering every block is
    in_proj GEMM + streaming attention; with a cluster module at block 2 (medoids forced from the oracle) block 1 is the long
    path and blocks 2 - 3 (L = 65) the one-launch in_proj + attention.  L2-normalised embeddings within 1e-3 of the oracle."""
    from centerclip_amd.clip import build_clip_model
    t = tiny_eval
    model, cfg = build_clip_model(dict(t["sd"]), args=_cluster_args(2) if clustered else None)
    model = model.to(DEV)
    assert cfg["vision_patch_size"] == 14 and cfg["image_resolution"] == 224
    video, ids = t["video"].to(DEV), t["ids"].to(DEV)
    ref, ref_h = (t["clus"], t["clus_h"]) if clustered else (t["plain"], t["plain_h"])
    if clustered:
        model.visual.forced_medoids = t["med"]
        feats, hidden = model.visual.encode(video, 2, want_hidden=True, forced_medoids=t["med"])
    else:
        feats, _ = model.encode_image(video, video_frame=2)
        _, hidden = model.visual.encode(video, 2, want_hidden=True)
    e = _emb_err(feats, ref)
    print("tiny L/14 clustered=%d: encode_image %.2e" % (clustered, e))
    assert feats.shape == ref.shape and e <= 1e-3
    assert hidden.shape == ref_h.shape == ((1, 65, 128) if clustered else (2, 257, 128))
    scale = float(ref_h.abs().max())
    eh = float((hidden.cpu() - ref_h).abs().max()) / scale
    print("tiny L/14 clustered=%d: hidden state %.2e of its largest entry" % (clustered, eh))
    assert eh <= 1e-3                                          # (test_clip_gpu's bound for the hidden state)
    vpair, tpair = model.encode_pair(video, ids, video_frame=2)
    ev, et = _emb_err(vpair, ref), _emb_err(tpair, t["text"])
    print("tiny L/14 clustered=%d: encode_pair visual %.2e text %.2e" % (clustered, ev, et))
    assert ev <= 1e-3 and et <= 1e-3
    # return_hidden: ln_post + proj on every token, its CLS row is the feature
    if clustered:                                               # (encode_image clusters on its own: the forced form by hand)
        from centerclip_amd import ops
        vis = model.visual
        hid = ops.head_project(hidden, vis.ln_post.weight, vis.ln_post.bias, vis.proj).view(hidden.shape[0], hidden.shape[1], -1)
        x = hid[:, 0, :]
        own, _ = model.encode_image(video, return_hidden=True, video_frame=2)
        assert own.shape == x.shape and bool(torch.isfinite(own).all())
    else:
        x, hid = model.encode_image(video, return_hidden=True, video_frame=2)
    assert hid.shape[:2] == hidden.shape[:2] and _emb_err(x, ref) <= 1e-3
    # the prefix encoder: the residual stream behind 1 block (L = 257: the two-launch block) and behind all 3
    med = t["med"] if clustered else None
    h1 = model.visual.encode_prefix(video, 2, 1, forced_medoids=med)
    h3 = model.visual.encode_prefix(video, 2, 3, forced_medoids=med)
    assert h1.shape == (2, 257, 128) and bool(torch.isfinite(h1).all())
    assert float((h3.cpu() - ref_h).abs().max()) <= 1e-3 * scale
    # uint8 frames through the encoder: the loader's normalisation inside the p = 14 gather
    u8 = torch.randint(0, 256, (2, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    f_u8, _ = model.visual.encode(u8.to(DEV), 2, forced_medoids=med)
    f_fl, _ = model.visual.encode(clo.loader_normalize(u8, channels_last=True).to(DEV), 2, forced_medoids=med)
    assert torch.equal(f_u8, f_fl)


def test_tiny_l14_graphed_eval_and_replica(tiny_eval):
    """The encoders captured into a hipGraph (both towers in one enqueue, L = 257 blocks as two launches each) replay the
    eager bits; CLIP4Clip.replica() (what the eval lanes hold) gives the bits of the model it copies."""
    from centerclip_amd.clip import build_clip_model
    t = tiny_eval
    model, _ = build_clip_model(dict(t["sd"]), args=None)
    model = model.to(DEV)
    video, ids = t["video"].to(DEV), t["ids"].to(DEV)
    v0, t0 = model.encode_pair(video, ids, video_frame=2)
    out = (torch.empty_like(v0), torch.empty_like(t0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.encode_pair(video, ids, video_frame=2, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model.encode_pair(video, ids, video_frame=2, out=out)
    out[0].zero_()
    out[1].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], v0) and torch.equal(out[1], t0)
    make, (ids4, _, video4, _) = _tiny_model()
    m4 = make().eval()
    twin = m4.replica()
    frames = video4.reshape(-1, 3, 224, 224)
    va, ta = m4.clip.encode_pair(frames, ids4, video_frame=TINY_TRAIN["T"])
    vb, tb_ = twin.clip.encode_pair(frames, ids4, video_frame=TINY_TRAIN["T"])
    assert va.shape == (TINY_TRAIN["B"] * TINY_TRAIN["T_new"], 512) and bool(torch.isfinite(va).all())
    assert torch.equal(va, vb) and torch.equal(ta, tb_)


def test_full_width_l14_blocks_against_the_oracle():
    """Width 1024, 16 heads, 4 layers, one frame: the GEMM shapes N = 1024 / 3072 / 4096 at M = 257 and the 640-deep patch GEMM."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(11)
    m = CLIP(768, 224, 4, 1024, 14, 77, 512, 128, 2, 1, args=None)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    video = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(12)).half().float()
    ref = clo.visual_forward(sd, video, 1)
    feats, _ = m.to(DEV).eval().encode_image(video.to(DEV), video_frame=1)
    e = _emb_err(feats, ref)
    print("width 1024, 4 layers: normalised embedding max|delta| %.2e" % e)
    assert feats.shape == (1, 768) and e <= 1e-3


# ------------------------------------------------------------------------------------------------ towers, training
TINY_TRAIN = dict(name="tiny ViT-L/14 geometry: patch 14, 224 px, width 128, 3 layers, 4 frames -> 2 segments @block 3, K = 64",
                  B=2, T=4, T_new=2, K=64, cluster_block=3, words=32, patch=14, res=224, width=128, layers=3)


@pytest.fixture(scope="module")
def tiny_step():
    """One HIP training step of CLIP4Clip at the tiny L/14 geometry and its float64 autograd reference (the helper of
    tests/test_train_full_gpu.py: same weights, batch and block-3 selection) - computed once."""
    from test_train_full_gpu import _full_step
    return _full_step(TINY_TRAIN, seed_w=3, seed_batch=103)


def test_tiny_l14_training_step_against_float64(tiny_step):
    """Blocks 1 - 2 train at L = 257 (attention backward with five key tiles), block 3 behind the cluster module at L = 65.
    Every parameter gradient against float64 autograd with test_train_full_gpu's measure and its ViT-B/16 bounds; conv1 (the
    padded patch GEMM), the positional embedding and the first block are printed on their own."""
    from test_train_full_gpu import _rel, compare_grads, BOUNDS_CFG5, FEAT_BOUNDS_CFG5
    s = tiny_step
    out, c = s["out"], TINY_TRAIN
    e_seq, e_vis = _rel(out["sequence_output"].detach(), s["seq64"]), _rel(out["visual_output"].detach(), s["vis64"])
    # The loss in two steps.  FEAT_BOUNDS_*["loss"] are what the loss kernel adds at batches of 4 and 16; at B = 2 (a 2 x 2
    # logit matrix, a small loss) the features' fp16-level error, multiplied by exp(logit_scale), is the larger part.  So: the
    # features against the reference's within their bounds, and the loss against float64 on the step's OWN features within
    # the loss bound - the two errors that add up to the loss's.
    e_loss_total = abs(float(out["loss"].detach()) - float(s["loss64"])) / abs(float(s["loss64"]))
    print("\n[tiny L/14] loss %.2e (vs the reference's features)  sequence_output %.2e  visual_output %.2e" % (e_loss_total, e_seq, e_vis))
    assert e_seq <= FEAT_BOUNDS_CFG5["sequence_output"] and e_vis <= FEAT_BOUNDS_CFG5["visual_output"]
    named = dict(s["model"].clip.named_parameters())
    vmask = torch.ones(c["B"], c["T"], dtype=torch.long, device=DEV)
    vmask[-1, c["T"] - 2:] = 0                                                  # bench.synthetic_batch's mask
    _, _, own = clo.contrastive_loss_native(out["sequence_output"].detach().double(), out["visual_output"].detach().double(),
                                            clo.video_mask_after_cluster(vmask, c["T"], c["T_new"]),
                                            named["logit_scale"].detach().double())
    e_loss = abs(float(out["loss"].detach()) - float(own)) / abs(float(own))
    print("[tiny L/14] loss %.2e against float64 on the step's own features" % e_loss)
    assert e_loss <= FEAT_BOUNDS_CFG5["loss"]
    assert set(s["hip"]) == set(s["ref"]) and "logit_scale" in s["ref"]
    errs, bad = compare_grads(s["hip"], s["ref"], BOUNDS_CFG5)
    print("[tiny L/14] five worst tensors:", sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    watch = {k: e for k, e in errs.items() if k.startswith(("visual.conv1", "visual.positional_embedding",
                                                            "visual.transformer.resblocks.0."))}
    print("[tiny L/14] conv1 / positional embedding / block 1:", {k: "%.2e" % e for k, e in watch.items()})
    assert len(watch) == 2 + 16 and not bad
    assert s["hip"]["visual.conv1.weight"].shape == (128, 3, 14, 14)


def _tiny_model():
    import sys
    from test_train_full_gpu import ROOT
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = bench.random_state_dict(TINY_TRAIN, seed=3)
    ids, amask, video, vmask = bench.synthetic_batch(TINY_TRAIN, DEV, seed=103)
    return (lambda: CLIP4Clip.from_state_dict(dict(sd), bench.task_config(TINY_TRAIN)).float().to(DEV).train()), (ids, amask, video, vmask)


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.clip.named_parameters()}


def test_tiny_l14_training_from_uint8_frames():
    """uint8 frames (patch 14: this raised ValueError) give the loss and every gradient of the float frames the loader's
    transform makes of them, bit for bit."""
    make, (ids, amask, _, vmask) = _tiny_model()
    model = make()
    B, T = TINY_TRAIN["B"], TINY_TRAIN["T"]
    u8 = torch.randint(0, 256, (B * T, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    flt = clo.loader_normalize(u8, channels_last=True)
    runs = []
    for video in (u8.view(B, 1, T, 224, 224, 3), flt.view(B, 1, T, 3, 224, 224)):
        model.zero_grad(set_to_none=True)
        out = model(ids, torch.zeros_like(ids), amask, video.to(DEV), vmask)
        out["loss"].backward()
        torch.cuda.synchronize()
        runs.append((out["loss"].detach().clone(), _grads(model)))
    assert torch.isfinite(runs[0][0]) and torch.equal(runs[0][0], runs[1][0])
    for k, gq in runs[0][1].items():
        assert gq is not None and torch.equal(gq, runs[1][1][k]), k


def test_tiny_l14_training_with_a_frozen_first_block():
    """freeze_cip_layers(1): the front end and block 1 of both towers are frozen, so the visual prefix runs the L = 257 block on
    the fused forward (in_proj GEMM + streaming attention) and hands block 2 its residual stream.  The gradients of everything
    that still trains against float64 autograd on the same weights with this step's own block-3 selection, same bounds; the
    frozen tensors get none."""
    from test_train_full_gpu import compare_grads, BOUNDS_CFG5
    make, (ids, amask, video, vmask) = _tiny_model()
    model = make()
    model.freeze_cip_layers(1)
    video = video.half().float()
    out = model(ids, torch.zeros_like(ids), amask, video, vmask)
    out["loss"].backward()
    torch.cuda.synchronize()
    med = model.clip.visual.transformer.resblocks[2].tokencluster_inter.last_medoids.clone()
    grads = {k: g for k, g in _grads(model).items() if g is not None}
    frozen = [k for k, p in model.clip.named_parameters() if not p.requires_grad]
    assert "visual.conv1.weight" in frozen and "visual.transformer.resblocks.0.attn.in_proj_weight" in frozen
    assert not set(frozen) & set(grads) and "visual.transformer.resblocks.1.attn.in_proj_weight" in grads
    c = TINY_TRAIN
    p64 = {k: v.detach().to(torch.float64).requires_grad_(True) for k, v in model.clip.named_parameters()}
    loss64, _, _ = clo.clip4clip_train_loss_native(p64, ids, video.double(), vmask, c["T"], c["T_new"], {2: (c["T_new"], c["K"])},
                                                   forced_medoids={2: med})
    loss64.backward()
    assert np.isfinite(float(out["loss"].detach())) and abs(float(out["loss"].detach()) - float(loss64.detach())) <= 1e-3 * abs(float(loss64.detach()))
    ref = {k: p.grad for k, p in p64.items() if k in grads}
    assert set(ref) == set(grads) and all(v is not None for v in ref.values())
    errs, bad = compare_grads(grads, ref, BOUNDS_CFG5)
    print("[tiny L/14 frozen block 1] worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, [(k, errs[k]) for k in bad]


def test_tiny_l14_graphed_train_step_equals_eager_steps():
    """train.GraphedTrainStep at the tiny L/14 geometry: two calls (capture + replay, replay) leave the parameters two eager
    steps leave, bit for bit - as test_r4_gpu.test_graphed_train_step_equals_eager_steps compares them."""
    from centerclip_amd.train import BertAdam, prep_optim_params_groups, train_epoch, GraphedTrainStep
    make, (ids, amask, video, vmask) = _tiny_model()
    batch = (ids.cpu(), amask.cpu(), torch.zeros_like(ids).cpu(), video.cpu(), vmask.cpu())
    args = Namespace(lr=1e-3, wd=0.2, new_added_modules=["Cross"], gradient_accumulation_steps=1, clip_grad_norm=None)

    def build(capturable):
        m = make()
        o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                     e=1e-6, max_grad_norm=1.0, capturable=capturable)
        return m, o
    m0, o0 = build(False)
    train_epoch(0, args, m0, [batch] * 2, DEV, o0, 0)
    m1, o1 = build(True)
    stepper = GraphedTrainStep(m1, o1)
    for _ in range(2):
        loss = stepper(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and all(st["step"] == 2 for st in o1.state.values())
    for (k, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p0, p1), k
