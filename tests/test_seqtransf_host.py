"""sim_header 'seqTransf' without a GPU: the float64 restatement of the head (tests/seqtransf_ref.py) against the reference's
own float64 run (fixture tests/golden/seqtransf_golden.npz, tools/gen_golden_seqtransf.py), the initialisation trick, the
state-dict names, the parameter groups and the refusals.

Bound of the restatement check: 1e-9 of each tensor's largest entry.  Both sides are float64 and differ only in summation
order (the reference scales q before q k^T, takes LayerNorm from ATen): about 1e-16 x a chain of ~1e4 operations, with a
wide margin for the LayerNorm and softmax amplification.  Summarised gradients (first 256 entries, 2-norm, largest magnitude,
16 projections <r_i, g>) carry the same bound; a projection's error is at most sum_k |r_ik| x the entry-wise bound."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import seqtransf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REL = 1e-9
TS = (1, 3, 12, 64, 77)
HEADS, LAYERS = 2, 2


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "seqtransf_golden.npz"))


@pytest.fixture(scope="module")
def clip_sd():
    g = np.load(os.path.join(GOLD, "clip_golden.npz"))
    return {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
            if k.startswith("sd/")}


def _sketch(name, numel):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal((16, numel))


def _head_params(clip_sd, gold):
    from centerclip_amd.clip4clip import CLIP4Clip
    init = CLIP4Clip.seq_head_init(clip_sd, LAYERS)
    pos = torch.from_numpy(gold["pos"]).double().requires_grad_(True)
    blocks = ref.blocks_from_state({k: v.double().requires_grad_(True) for k, v in init.items()}, LAYERS)
    return pos, blocks


def _close(name, got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if scale is None else scale
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print("%-60s max|d| %.2e  (scale %.2e)" % (name, err, scale))
    assert err <= REL * scale, name


@pytest.mark.parametrize("T", TS)
def test_restatement_matches_the_reference_in_float64(gold, clip_sd, T):
    c = "c/%d/" % T
    pos, blocks = _head_params(clip_sd, gold)
    vis = torch.from_numpy(gold[c + "vis"]).double().requires_grad_(True)
    mask = torch.from_numpy(gold[c + "mask"])
    seq = torch.from_numpy(gold[c + "seq"]).double()
    ls = clip_sd["logit_scale"].double()
    h = ref.head(vis, mask, pos, blocks, HEADS)
    _close(c + "head64", h.detach().numpy(), gold[c + "head64"])
    lg = ref.logits(seq, vis, mask, pos, blocks, HEADS, ls)
    _close(c + "logits64", lg.detach().numpy(), gold[c + "logits64"])
    loss = ref.cross_en_symmetric(lg)
    _close(c + "loss64", loss.item(), gold[c + "loss64"])
    names = ["vis", "frame_position_embeddings.weight"] + ["transformerClip.resblocks.%d.%s" % (i, p) for i in range(LAYERS)
                                                           for p in ref.BLOCK_PARAMS]
    tensors = [vis, pos] + [b[p] for b in blocks for p in ref.BLOCK_PARAMS]
    grads = torch.autograd.grad(loss, tensors)
    for name, g in zip(names, grads):
        k = c + "g64/" + name
        f = g.numpy().reshape(-1)
        if k in gold.files:
            _close(k, f, gold[k].reshape(-1))
            continue
        amax = float(gold[k + "/amax"])
        _close(k + "/amax", np.abs(f).max(), amax, amax)
        _close(k + "/norm", np.linalg.norm(f), gold[k + "/norm"], float(gold[k + "/norm"]))
        _close(k + "/head", f[:256], gold[k + "/head"], amax)
        r = _sketch(name, f.size)
        got = r @ f
        err = float(np.abs(got - gold[k + "/sketch"]).max())
        bound = REL * amax * float(np.abs(r).sum(1).max())
        print("%-60s max|d| %.2e  (bound %.2e)" % (k + "/sketch", err, bound))
        assert err <= bound, k
    # rows of the position table behind T get exactly zero gradient
    assert not grads[1][T:].any()


def test_reference_fp32_logits_are_within_the_parity_contract(gold, clip_sd):
    """The reference's own fp32 logits against its float64 run: the rounding of the fp32 head (documents what the 1e-3 parity
    contract on cosines leaves to an implementation)."""
    ls = float(np.exp(clip_sd["logit_scale"].double().item()))
    for T in TS:
        c = "c/%d/" % T
        d = float(np.abs(gold[c + "logits32"].astype(np.float64) - gold[c + "logits64"]).max()) / ls
        print("T %2d  fp32 vs float64 cosine: %.2e" % (T, d))
        assert d <= 1e-3


def test_init_trick_matches_the_reference(gold, clip_sd):
    from centerclip_amd.clip4clip import CLIP4Clip
    init = CLIP4Clip.seq_head_init(clip_sd, LAYERS)
    assert sorted(init) == json.loads(str(gold["init/names"]))
    for k, v in init.items():
        f = v.double().numpy().reshape(-1)
        assert np.array_equal(f[:256], gold["init/" + k + "/head"]), k
        np.testing.assert_allclose(_sketch(k, f.size) @ f, gold["init/" + k + "/sketch"], rtol=1e-12, atol=1e-12)


def _task(**kw):
    a = Namespace(cluster_inter=0, cluster_algo=None, max_frames=4, target_frames_blocks=[4, 4, 4], cluster_num_blocks=[16] * 3,
                  loose_type=True, sim_header='seqTransf', linear_patch='2d', cross_num_hidden_layers=LAYERS,
                  pre_visual_pooling=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _square_sd(clip_sd):
    """The small model with embed_dim = transformer_width (128): the head runs on the visual features, so the two agree, as
    in every shipped CLIP (512 / 512)."""
    sd = dict(clip_sd)
    g = torch.Generator().manual_seed(5)
    sd["text_projection"] = torch.randn(128, 128, generator=g) * 0.05
    sd["visual.proj"] = torch.randn(sd["visual.proj"].shape[0], 128, generator=g) * 0.05
    return sd


def test_state_dict_names_shapes_and_reference_checkpoint(clip_sd, gold):
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = _square_sd(clip_sd)
    m = CLIP4Clip.from_state_dict(sd, _task())
    names = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("clip.")}
    want = {"frame_position_embeddings.weight": (16, 128)}
    for i in range(LAYERS):
        for p, shp in (("attn.in_proj_weight", (384, 128)), ("attn.in_proj_bias", (384,)), ("attn.out_proj.weight", (128, 128)),
                       ("attn.out_proj.bias", (128,)), ("ln_1.weight", (128,)), ("ln_1.bias", (128,)),
                       ("mlp.c_fc.weight", (512, 128)), ("mlp.c_fc.bias", (512,)), ("mlp.c_proj.weight", (128, 512)),
                       ("mlp.c_proj.bias", (128,)), ("ln_2.weight", (128,)), ("ln_2.bias", (128,))):
            want["transformerClip.resblocks.%d.%s" % (i, p)] = shp
    assert names == want
    assert all(v.dtype == torch.float32 for k, v in m.state_dict().items() if not k.startswith("clip."))
    # from_state_dict applied the initialisation trick
    assert torch.equal(m.frame_position_embeddings.weight, sd["positional_embedding"])
    assert torch.equal(m.transformerClip.resblocks[1].mlp.c_fc.weight, sd["transformer.resblocks.1.mlp.c_fc.weight"])
    # a reference-named checkpoint (clip.* + the head) loads with no missing and no unexpected key
    ck = {"clip." + k: v for k, v in m.clip.state_dict().items()}
    ck.update({k: torch.randn(v.shape) for k, v in m.state_dict().items() if not k.startswith("clip.")})
    res = m.load_state_dict(ck, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.transformerClip.resblocks[0].attn.in_proj_bias, ck["transformerClip.resblocks.0.attn.in_proj_bias"])


def test_from_pretrained_keeps_a_fine_tuned_head(clip_sd, tmp_path, monkeypatch):
    from centerclip_amd import clip4clip as c4c
    sd = _square_sd(clip_sd)
    monkeypatch.setattr(c4c, "load_clip_state_dict", lambda *a, **k: dict(sd))
    fine = {"frame_position_embeddings.weight": torch.full((16, 128), 0.25)}
    m = c4c.CLIP4Clip.from_pretrained(state_dict=fine, task_config=_task(pretrained_dir=str(tmp_path)))
    assert torch.equal(m.frame_position_embeddings.weight, fine["frame_position_embeddings.weight"])
    # no frame_position_embeddings in the fine-tuned dict: the trick
    m = c4c.CLIP4Clip.from_pretrained(state_dict={}, task_config=_task(pretrained_dir=str(tmp_path)))
    assert torch.equal(m.frame_position_embeddings.weight, sd["positional_embedding"])
    assert torch.equal(m.transformerClip.resblocks[0].attn.in_proj_weight, sd["transformer.resblocks.0.attn.in_proj_weight"])


def test_param_groups_put_the_head_at_full_lr(clip_sd):
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.train import prep_optim_params_groups
    m = CLIP4Clip.from_state_dict(_square_sd(clip_sd), _task())
    head_ids = {id(p) for n, p in m.named_parameters() if not n.startswith("clip.")}
    assert len(head_ids) == 1 + 12 * LAYERS
    for optim in ("BertAdam", "AdamW"):
        groups = prep_optim_params_groups(Namespace(lr=1e-2, wd=0.2, new_added_modules=["Cross"], optim=optim), m, coef_lr=1e-3)
        in_clip = {id(p) for g in groups[:2] for p in g['params']}
        in_new = {id(p) for g in groups[2:] for p in g['params']}
        assert head_ids <= in_new and not (head_ids & in_clip)
        if optim == "BertAdam":
            assert 'lr' not in groups[2] and 'lr' not in groups[3]        # the optimizer's own lr, not lr * coef_lr
        else:
            assert groups[2]['lr_mult'] == 1.0 and groups[3]['lr_mult'] == 1.0
        biases = {id(m.transformerClip.resblocks[0].attn.in_proj_bias), id(m.transformerClip.resblocks[0].ln_1.bias)}
        assert biases <= {id(p) for p in groups[3]['params']}


def test_refusals(clip_sd):
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = _square_sd(clip_sd)
    with pytest.raises(ValueError, match="pre_visual_pooling"):
        CLIP4Clip.from_state_dict(sd, _task(pre_visual_pooling=1))
    for header in ("seqLSTM", "tightTransf"):
        with pytest.raises(NotImplementedError):
            CLIP4Clip.from_state_dict(sd, _task(sim_header=header))
    with pytest.raises(NotImplementedError):
        CLIP4Clip.from_state_dict(sd, _task(loose_type=False))
    with pytest.raises(ValueError, match="embed_dim"):
        CLIP4Clip.from_state_dict(clip_sd, _task())                     # embed 64 != width 128
    m = CLIP4Clip.from_state_dict(sd, _task())
    with pytest.raises(ValueError, match="position table"):
        m.seq_head(torch.zeros(2, 17, 128), torch.ones(2, 17, dtype=torch.long))     # T = 17 > the 16-row table
    # (the shipped CLIPs have 77 rows: T > 77 is refused the same way)
    big = dict(sd, positional_embedding=torch.zeros(77, 128))
    m77 = CLIP4Clip.from_state_dict(big, _task())
    assert m77.frame_position_embeddings.num_embeddings == 77
    with pytest.raises(ValueError, match="position table"):
        m77.seq_head(torch.zeros(1, 78, 128), torch.ones(1, 78, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        m.encode_into(None, torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 1, 4, 3, 64, 64), torch.ones(1, 4, dtype=torch.long))


@pytest.mark.parametrize("L", (3, 12))
def test_attention_with_every_key_masked_against_the_reference(gold, clip_sd, L):
    """Block 0's attention (out_proj included) of two sequences, sequence 0 with every key masked, sequence 1 with half of
    them, against the reference's fp32 output: the restatement in float64 (key_masked_attention, for sequence 0 the unmasked
    softmax) is what the HIP kernels are held to.  Bound, per output entry: the reference's scores s - 1e6 are rounded to the
    fp32 spacing at 1e6 (2^-4, an error of at most 2^-5 per score) in sequence 0, and carry fp32 summation error (a 128-term
    in_proj and a 64-term score, 256 units of 2^-24 of sum |q_d k_d| / 8) in both; a score error e moves the output by at most
    2 e sum_j p_j |v_j|, then out_proj adds its own 128-term fp32 sum: |out - ref| <= (2 E |o|_p) |W_o|^T + 2^-24 (128 + 8)
    (|o| |W_o|^T + |b_o|)."""
    from centerclip_amd.clip4clip import CLIP4Clip
    a = "a/%d/" % L
    D = 128
    init = CLIP4Clip.seq_head_init(clip_sd, LAYERS)
    p = {k: init["transformerClip.resblocks.0." + k].double() for k in ("attn.out_proj.weight", "attn.out_proj.bias")}
    qkv = torch.from_numpy(gold[a + "qkv"]).double().view(2, L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    mask = torch.from_numpy(gold[a + "mask"])
    assert int(mask[0].sum()) == 0 and 0 < int(mask[1].sum()) < L
    live = mask.clone()
    live[live.sum(1) == 0] = 1
    q, k, v = qkv[0], qkv[1], qkv[2]
    o = ref.key_masked_attention(q, k, v, mask)                          # the restatement itself (its -1e6, float64)
    o = o.transpose(1, 2).reshape(2 * L, D)
    out = o @ p["attn.out_proj.weight"].t() + p["attn.out_proj.bias"]
    U = 2.0 ** -24
    s_abs = (q.abs() @ k.abs().transpose(-1, -2) / 8).amax(-1, keepdim=True)      # [2, H, L, 1]
    E = 256 * U * s_abs + torch.tensor([2.0 ** -5, 0.0], dtype=torch.float64).view(2, 1, 1, 1)
    pr = torch.softmax(q @ k.transpose(-1, -2) / 8 + ((1.0 - live.double()) * -1e6)[:, None, None, :], -1)
    dpv = (2 * E * (pr @ v.abs())).transpose(1, 2).reshape(2 * L, D)
    Wa = p["attn.out_proj.weight"].abs()
    bound = dpv @ Wa.t() + U * (D + 8) * (o.abs() @ Wa.t() + p["attn.out_proj.bias"].abs())
    err = (out - torch.from_numpy(gold[a + "out"]).double()).abs()
    print("L %2d  max|d| %.2e  max(|d| / bound) %.3f" % (L, float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    # sequence 0 is the unmasked softmax: the formula's exact value, up to the float64 rounding of s - 1e6 (spacing 2^-52 x
    # 2^20, at most 2^-33 per score, which moves the output by at most 2 x 2^-33 x max |v|; doubled for the other roundings)
    o_un = torch.softmax(q[0] @ k[0].transpose(-1, -2) / 8, -1) @ v[0]
    assert float((o_un.transpose(0, 1).reshape(L, D) - o[:L]).abs().max()) <= 4 * 2.0 ** -33 * float(v[0].abs().max())
