"""The training step at the shape the launchers train, against a float64 torch.autograd reference.

* the whole cfg-2 step (ViT-B/32, 12 + 12 layers, 12 frames -> 3 segments at block 7, K = 49, B = 16, one clip with padded
  frames): CLIP4Clip in .train(), loss.backward(), against oracle.clip_oracle.clip4clip_train_loss_native run in float64 on
  the device with the HIP path's own block-7 selection forced (pinned to the reference's autograd on the CPU in
  tests/test_oracle_train.py).  Every parameter gradient is compared relative to its own largest entry, in_proj_* per
  q / k / v third; the same helper must reject perturbed copies of the HIP gradients; a second step gives the same bits.
* a ViT-B/16 step (cfg-5 shapes: 197 tokens, K = 100, split 4) at B = 4.
* the kernels whose training shapes one GPU's step cannot reach: the contrastive loss at the all-gathered batch (n up to
  512), the token-cluster backward at W = 768 / 1024, train.LinearFunction at the patch-embedding and head shapes.  Sums are
  bounded by (the kernel's longest serial chain) * 2^-24 * sum|terms| (+ the fp16 rounding of the operands where the kernel
  multiplies fp16), as in tests/test_backward_gpu.py; gathers and single divisions are compared bit for bit.

Measured worst errors on an MI355X (relative to each tensor's largest entry, the loss to itself; the HIP path gives the same
bits run to run).  Each bound below (BOUNDS_* / FEAT_BOUNDS_*) is at most twice the measured worst and never above 2.5e-2.
                 patch    vis_embed vis_blocks vis_head txt_embed txt_blocks txt_head logit_scale | loss    seq     visual
  cfg 2, B = 16  1.43e-3  3.17e-3   6.70e-3    4.35e-3  2.97e-3   3.81e-3    2.54e-3  5.67e-4     | 1.07e-6 7.26e-4 3.70e-4
  cfg 5, B = 4   1.24e-3  3.82e-3   1.06e-2    4.53e-3  2.84e-3   6.36e-3    3.69e-3  1.04e-2     | 4.44e-6 7.72e-4 3.00e-4
The worst tensors are the late visual blocks' c_proj weights and in_proj v biases (fp16 operands of the MFMA GEMMs: ~2^-11
per operand, summed over the block).  cfg 5's logit_scale gradient (1.0e-2) is a sum over the 4 x 4 logits that nearly
cancels, so the features' ~7e-4 fp16-level error is amplified there; the loss kernel itself is at ~1e-6 relative (the
contrastive-loss tests below).  Of their running-error bounds the kernel-level checks use at most 3 % (contrastive loss)
and 32 % (LinearFunction, text_projection dW); the token-cluster grad_x is bit for bit.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import clip_oracle as clo

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                                                  # unit roundoff of fp32
H = 2.0 ** -11                                                  # of fp16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 2.5e-2


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


# ------------------------------------------------------------------------------------------------ comparison helper
GROUPS = ("patch", "vis_embed", "vis_blocks", "vis_head", "txt_embed", "txt_blocks", "txt_head", "logit_scale")


def _group(label):
    """The bound group of a parameter (or of a q / k / v third of one)."""
    name = label.split("[")[0]
    if name == "logit_scale":
        return "logit_scale"
    if name.startswith("visual.transformer.resblocks."):
        return "vis_blocks"
    if name.startswith("transformer.resblocks."):
        return "txt_blocks"
    if name == "visual.conv1.weight":
        return "patch"
    if name.startswith("visual.ln_post") or name == "visual.proj":
        return "vis_head"
    if name.startswith("visual."):
        return "vis_embed"
    if name.startswith("ln_final") or name == "text_projection":
        return "txt_head"
    return "txt_embed"


def _pieces(name, g):
    """[(label, tensor)]: in_proj_weight / in_proj_bias as their q, k and v thirds, anything else whole."""
    if name.endswith("attn.in_proj_weight") or name.endswith("attn.in_proj_bias"):
        w = g.shape[0] // 3
        return [("%s[%s]" % (name, part), g[i * w:(i + 1) * w]) for i, part in enumerate("qkv")]
    return [(name, g)]


def _rel(got, ref, scale=None):
    """max |got - ref| over the largest |entry| of scale (default: of ref)."""
    den = float((ref if scale is None else scale).double().abs().max())
    diff = float((got.double() - ref.double()).abs().max())
    return diff / den if den > 0 else (0.0 if diff == 0 else math.inf)


def compare_grads(hip, ref, bounds):
    """hip, ref {name: gradient}; bounds {group: bound} -> ({label: error}, [labels above their group's bound])."""
    errs = {}
    for name, r in ref.items():
        for (label, a), (_, b) in zip(_pieces(name, hip[name].reshape(r.shape)), _pieces(name, r)):
            # the k third of in_proj_bias has no gradient in exact arithmetic (a shift of all of a query's scores leaves its
            # softmax unchanged): it is measured against the whole tensor's largest entry
            errs[label] = _rel(a, b, r if label.endswith("in_proj_bias[k]") else None)
    bad = [k for k, e in errs.items() if not e <= bounds[_group(k)]]
    return errs, bad


def _worst(errs, k=5):
    return sorted(errs.items(), key=lambda kv: -kv[1])[:k]


# ------------------------------------------------------------------------------------------------ the whole step
def _full_step(cfg, seed_w, seed_batch):
    """One HIP training step and its float64 reference on the same weights, batch and block selection."""
    bench = _bench()
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = bench.random_state_dict(cfg, seed=seed_w)
    model = CLIP4Clip.from_state_dict(dict(sd), bench.task_config(cfg)).to(DEV).train()
    ids, amask, video, vmask = bench.synthetic_batch(cfg, DEV, seed=seed_batch)
    video = video.half().float()                              # the patch GEMM's input quantisation, for both sides
    assert int(vmask.sum()) < vmask.numel()                   # a clip with padded frames

    def step():
        out = model(ids, torch.zeros_like(ids), amask, video, vmask)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out

    out = step()
    tc = model.clip.visual.transformer.resblocks[cfg["cluster_block"] - 1].tokencluster_inter
    med = tc.last_medoids.clone()
    named = dict(model.clip.named_parameters())
    hip = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith("clip."))
    # the float64 reference, on the device, with the HIP path's selection forced
    p64 = {k: v.detach().to(torch.float64).requires_grad_(True) for k, v in named.items()}
    plan = {cfg["cluster_block"] - 1: (cfg["T_new"], cfg["K"])}
    loss64, seq64, vis64 = clo.clip4clip_train_loss_native(p64, ids, video.double(), vmask, cfg["T"], cfg["T_new"], plan,
                                                           forced_medoids={cfg["cluster_block"] - 1: med})
    loss64.backward()
    ref = {k: p.grad for k, p in p64.items() if p.grad is not None}
    return dict(model=model, step=step, out=out, med=med, hip=hip, ref=ref, loss64=loss64.detach(), seq64=seq64.detach(),
                vis64=vis64.detach(), cfg=cfg)


@pytest.fixture(scope="module")
def cfg2_step():
    return _full_step(_bench().CFG2, seed_w=0, seed_batch=100)


def _check_step(s, bounds, feat_bounds, tag):
    cfg, out, med = s["cfg"], s["out"], s["med"]
    B, Tn, K = cfg["B"], cfg["T_new"], cfg["K"]
    N = (cfg["T"] // Tn) * (cfg["res"] // cfg["patch"]) ** 2
    # the selection: [T_new * B, K], ascending ids of the segment's fd * n tokens
    assert tuple(med.shape) == (Tn * B, K) and med.dtype == torch.long
    assert bool((med[:, 1:] > med[:, :-1]).all()) and int(med.min()) >= 0 and int(med.max()) < N
    e_loss = abs(float(out["loss"].detach()) - float(s["loss64"])) / abs(float(s["loss64"]))
    e_seq = _rel(out["sequence_output"].detach(), s["seq64"])
    e_vis = _rel(out["visual_output"].detach(), s["vis64"])
    errs, bad = compare_grads(s["hip"], s["ref"], bounds)
    worst = {g: max(e for k, e in errs.items() if _group(k) == g) for g in GROUPS}
    print(f"\n[{tag}] loss {e_loss:.2e}  sequence_output {e_seq:.2e}  visual_output {e_vis:.2e}")
    print(f"[{tag}] worst per group:", {g: "%.2e" % e for g, e in worst.items()})
    print(f"[{tag}] five worst tensors:", [(k, "%.2e" % e) for k, e in _worst(errs)])
    fb = feat_bounds
    assert e_loss <= fb["loss"] and e_seq <= fb["sequence_output"] and e_vis <= fb["visual_output"], (e_loss, e_seq, e_vis)
    assert not bad, [(k, errs[k]) for k in bad]
    # exactly the parameters the float64 graph reaches receive a gradient (logit_scale included)
    assert set(s["hip"]) == set(s["ref"]) and "logit_scale" in s["ref"]


# per group: <= 2x the measured worst (module docstring), never above 2.5e-2
BOUNDS_CFG2 = dict(patch=2.5e-3, vis_embed=6e-3, vis_blocks=1.3e-2, vis_head=8e-3, txt_embed=5e-3, txt_blocks=7e-3,
                   txt_head=5e-3, logit_scale=1e-3)
BOUNDS_CFG5 = dict(patch=2.4e-3, vis_embed=7.5e-3, vis_blocks=2.1e-2, vis_head=9e-3, txt_embed=5.5e-3, txt_blocks=1.25e-2,
                   txt_head=7e-3, logit_scale=2e-2)
FEAT_BOUNDS_CFG2 = dict(loss=2e-6, sequence_output=1.4e-3, visual_output=7e-4)
FEAT_BOUNDS_CFG5 = dict(loss=8e-6, sequence_output=1.5e-3, visual_output=6e-4)
assert all(max(b.values()) <= CAP for b in (BOUNDS_CFG2, BOUNDS_CFG5, FEAT_BOUNDS_CFG2, FEAT_BOUNDS_CFG5))


def test_cfg2_training_step_against_float64(cfg2_step):
    """cfg 2 (B = 16): the selection, the loss, the features and every parameter gradient of the HIP step against float64
    autograd; the five worst tensors are printed."""
    _check_step(cfg2_step, BOUNDS_CFG2, FEAT_BOUNDS_CFG2, "cfg2")


def test_cfg2_training_step_is_deterministic(cfg2_step):
    """The same inputs after zeroing the gradients: the selection, the loss and every gradient bit for bit."""
    s = cfg2_step
    model = s["model"]
    model.zero_grad(set_to_none=False)
    out = s["step"]()
    assert torch.equal(out["loss"].detach(), s["out"]["loss"].detach())
    tc = model.clip.visual.transformer.resblocks[s["cfg"]["cluster_block"] - 1].tokencluster_inter
    assert torch.equal(tc.last_medoids, s["med"])
    for k, p in model.clip.named_parameters():
        if k in s["hip"]:
            assert torch.equal(p.grad, s["hip"][k]), k


def test_cfg2_comparison_rejects_perturbed_gradients(cfg2_step):
    """The helper the step test uses has teeth: one tensor scaled by 1 + 3 * bound, the gradients of blocks 3 and 4 swapped,
    one head's rows of one in_proj_weight's k part zeroed - each is rejected (the kernels are not touched)."""
    hip, ref = cfg2_step["hip"], cfg2_step["ref"]
    assert not compare_grads(hip, ref, BOUNDS_CFG2)[1]
    name = "visual.transformer.resblocks.9.mlp.c_fc.weight"
    scaled = dict(hip)
    scaled[name] = hip[name] * (1 + 3 * BOUNDS_CFG2[_group(name)])
    assert compare_grads(scaled, ref, BOUNDS_CFG2)[1] == [name]
    swapped = dict(hip)
    for k in hip:
        if k.startswith("visual.transformer.resblocks.3."):
            k4 = k.replace(".resblocks.3.", ".resblocks.4.")
            swapped[k], swapped[k4] = hip[k4], hip[k]
    bad = compare_grads(swapped, ref, BOUNDS_CFG2)[1]
    assert any(".resblocks.3." in k for k in bad) and any(".resblocks.4." in k for k in bad), bad
    name = "visual.transformer.resblocks.8.attn.in_proj_weight"
    W = hip[name].shape[1]
    head = hip[name].clone()
    head[W + 5 * 64:W + 6 * 64] = 0                             # head 5 of the k part
    zeroed = dict(hip)
    zeroed[name] = head
    assert compare_grads(zeroed, ref, BOUNDS_CFG2)[1] == [name + "[k]"]


def test_vit_b16_training_step_against_float64():
    """cfg-5 shapes (ViT-B/16: 197 tokens, 12 frames -> 4 segments, K = 100, split 4) at B = 4: the attention backward's
    64 < L <= 256 form and the larger cluster in the composition."""
    cfg = dict(_bench().FORWARD_CFGS["cfg5"], B=4)
    s = _full_step(cfg, seed_w=1, seed_batch=101)
    _check_step(s, BOUNDS_CFG5, FEAT_BOUNDS_CFG5, "cfg5 B=4")


# ------------------------------------------------------------------------------------------------ contrastive loss
def _loss_grad_call(text, vis, mask, ls, grad_scale, ls_dev=None):
    """cc_contrastive_loss_grad_f32 (ls_dev None) or cc_contrastive_loss_grad_dev_f32, for an incoming gradient grad_scale."""
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    n, Tn, E = vis.shape
    loss3, dls = torch.empty(3, device=DEV), torch.empty(1, device=DEV)
    dt, dv = torch.empty_like(text), torch.empty_like(vis)
    lib = L.lib()
    ws = L.workspace(lib.cc_contrastive_grad_workspace_bytes(n, Tn, E), text.device)
    common = (L.ptr(text), L.ptr(vis), L.ptr(mask), mask.stride(0), mask.stride(1), n, Tn, E)
    if ls_dev is None:
        rc = lib.cc_contrastive_loss_grad_f32(*common, float(ls), float(grad_scale), L.ptr(loss3), L.ptr(dt), L.ptr(dv),
                                              L.ptr(dls), L.ptr(ws), ws.numel(), _st(text))
    else:
        rc = lib.cc_contrastive_loss_grad_dev_f32(*common, 0.0, L.ptr(ls_dev), float(grad_scale), L.ptr(loss3), L.ptr(dt),
                                                  L.ptr(dv), L.ptr(dls), L.ptr(ws), ws.numel(), _st(text))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return loss3, dt, dv, dls


def _loss_bounds(t, v, m, ls):
    """Running-error bounds (float64) of cc_contrastive_loss_grad_f32's outputs from its longest serial chains: a dot over E
    is E/64 lane-strided terms and a 6-level tree, the sums over the batch in the feature gradients are serial (n terms),
    the pooling over Tn frames is serial.  The error eS of S = exp(ls) t_hat . p_hat is amplified by the softmax:
    rel. error of P_ij <= 2 eS + (n/64 + 16 + 4 max|S|) u.  -> (loss3, d_text, d_visual, d_logit_scale) bounds."""
    n, Tn, E = v.shape
    a = t.norm(dim=-1, keepdim=True)
    th = t / a
    vn = v.norm(dim=-1, keepdim=True)
    vh = v / vn
    mm = m.to(t.dtype).unsqueeze(-1)
    den = mm.sum(1).clamp_min(1.0)
    p = (vh * mm).sum(1) / den
    pn = p.norm(dim=-1, keepdim=True)
    ph = p / pn
    s = math.exp(ls)
    S = s * th @ ph.t()
    P, Q = torch.softmax(S, 1), torch.softmax(S, 0)
    G = (P + Q - 2 * torch.eye(n, dtype=t.dtype, device=t.device)) / (2 * n)
    dot = E / 64 + 8
    eS = s * (3 * dot + Tn + 8) * U
    relP = 2 * eS + (n / 64 + 16 + 4 * float(S.abs().max())) * U
    eG = (P + Q) / (2 * n) * relP + G.abs() * 4 * U

    def norm_back(x_hat, d, e_d, nrm):
        # (d - x_hat (x_hat . d)) / |x|, d known to within e_d
        dd = (x_hat.abs() * d.abs()).sum(-1, keepdim=True)
        return (e_d + x_hat.abs() * (x_hat.abs() * e_d).sum(-1, keepdim=True)
                + (dot + 4) * U * (d.abs() + x_hat.abs() * dd)) / nrm

    dth = s * G @ ph
    e_dth = s * (eG @ ph.abs() + (n + dot + Tn + 8) * U * (G.abs() @ ph.abs()))
    b_text = norm_back(th, dth, e_dth, a)
    dph = s * G.t() @ th
    e_dph = s * (eG.t() @ th.abs() + (n + dot + 8) * U * (G.abs().t() @ th.abs()))
    dp = (dph - ph * (ph * dph).sum(-1, keepdim=True)) / pn
    e_dp = norm_back(ph, dph, e_dph, pn) + (Tn + dot) * U * dp.abs()
    dvh = dp.unsqueeze(1) * mm / den.unsqueeze(1)
    e_dvh = e_dp.unsqueeze(1) * mm / den.unsqueeze(1) + 2 * U * dvh.abs()
    b_vis = norm_back(vh, dvh, e_dvh, vn)
    b_ls = float((eG * S.abs() + G.abs() * eS).sum() + (2 * n + 16) * U * (G * S).abs().sum())
    lse = max(float(torch.logsumexp(S, 1).abs().max()), float(torch.logsumexp(S, 0).abs().max()))
    b_loss = 2 * eS + (n / 64 + 32) * U * (lse + float(S.abs().max()) + 1)
    return b_loss, b_text, b_vis, b_ls


def _loss_case(n, Tn, E, seed, noncontig):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(n, E, generator=g)
    v = torch.randn(n, Tn, E, generator=g) + 0.5 * torch.randn(n, 1, E, generator=g)     # the frames of a clip correlate
    t[: n // 2] += 0.3 * v[: n // 2].mean(1)                                              # some matching pairs
    m = torch.ones(n, Tn, dtype=torch.long)
    for i in range(0, n, 3):
        m[i, Tn - 1 - (i // 3) % max(Tn - 1, 1):] = 0                                     # trailing padded frames
    m[:, 0] = 1
    m = m.to(DEV)
    if noncontig:                                                                         # a column-major view
        m = m.t().contiguous().t()
        assert m.stride() == (1, n)
    return t.to(DEV), v.to(DEV), m


LOSS_CASES = [  # (n, Tn, E, logit_scale, grad_scale, non-contiguous mask)
    (64, 3, 256, math.log(1 / 0.07), 1.0, False),
    (65, 6, 512, math.log(100.0), 65536.0, True),
    (128, 12, 1024, math.log(1 / 0.07), 65536.0, False),
    (128, 3, 512, math.log(100.0), 1.0, False),
    (256, 3, 1024, math.log(100.0), 1.0, True),
    (256, 6, 256, math.log(1 / 0.07), 1.0, False),
    (512, 12, 512, math.log(100.0), 65536.0, False),
    (512, 3, 1024, math.log(1 / 0.07), 1.0, True),
]


@pytest.mark.parametrize("n,Tn,E,ls,gs,noncontig", LOSS_CASES)
def test_contrastive_loss_grad_at_gathered_batches(n, Tn, E, ls, gs, noncontig):
    """cc_contrastive_loss_grad_f32 / _dev_f32 at the batches the loss sees after the all-gather (world 8 x B 16 = 128,
    x B 64 = 512, and around one wave), E up to the kernel's limit 1024, padded frames, a strided mask, logit_scale
    ln(1/0.07) and ln 100, grad_scale 1 and 65536: loss3, d_text, d_visual and d_logit_scale within the running-error
    bounds of oracle.clip_oracle.contrastive_loss_and_grads in float64; host and device logit_scale give the same bits."""
    t, v, m = _loss_case(n, Tn, E, seed=n * 100 + Tn * 10 + E // 256, noncontig=noncontig)
    ls32 = float(np.float32(ls))
    outs = _loss_grad_call(t, v, m, ls32, gs)
    outs_dev = _loss_grad_call(t, v, m, ls32, gs, ls_dev=torch.tensor([ls32], device=DEV))
    same = [torch.equal(a, b) for a, b in zip(outs, outs_dev)]
    loss3, dt, dv, dls = outs
    r3, rdt, rdv, rdls = clo.contrastive_loss_and_grads(t.double(), v.double(), m, ls32, dtype=torch.float64)
    assert r3.dtype == rdt.dtype == rdv.dtype == rdls.dtype == torch.float64
    b_loss, b_text, b_vis, b_ls = _loss_bounds(t.double(), v.double(), m, ls32)
    q_loss = float((loss3.double() - r3).abs().max()) / b_loss
    q_text = float(((dt.double() / gs - rdt).abs() / b_text.clamp_min(1e-300)).max())
    q_vis = float(((dv.double() / gs - rdv).abs() / b_vis.clamp_min(1e-300)).max())     # (0 / 0 on padded frames)
    q_ls = abs(float(dls) / gs - float(rdls)) / b_ls
    print(f"[loss n={n} Tn={Tn} E={E} s={math.exp(ls):.1f} gs={gs:g}] error / bound: loss {q_loss:.2f} d_text {q_text:.2f} "
          f"d_visual {q_vis:.2f} d_logit_scale {q_ls:.2f}; relative d_text {_rel(dt / gs, rdt):.1e} "
          f"d_visual {_rel(dv / gs, rdv):.1e}; host == device {same}")
    assert all(same), "host and device logit_scale entry points differ"
    assert q_loss <= 1.0 and q_text <= 1.0 and q_vis <= 1.0 and q_ls <= 1.0, (q_loss, q_text, q_vis, q_ls)
    assert bool((dv[m == 0] == 0).all())                        # padded frames receive no gradient


# ------------------------------------------------------------------------------------------------ token-cluster backward
CLUSTER_CASES = ["medoid", "mean", "embed_mult", "sparse_repeat"]


def _ref_cluster_grads(x, G, T, Tn, K, agg, med, asg, embed, mult, ids):
    """float32 torch.autograd on the CPU through the oracle's forward for the given selection -> (gx, g_embed, g_mult)."""
    from oracle import cluster_oracle as co
    xr = x.clone().requires_grad_(True)
    er = embed.clone().requires_grad_(True) if embed is not None else None
    mr = mult.clone().requires_grad_(True) if mult is not None else None
    if ids is not None:                                      # 'sparse_sampling': the same ids in every problem
        # autograd's scatter-add of a repeated index adds in no fixed order on the CPU (atomic adds across threads): the
        # CLS rows go through autograd with the token rows' gradient zeroed, and a token's gradient is the sum of the
        # G rows that picked it, added here in ascending k (the order the kernel sums in)
        P = (x.shape[1] // T) * Tn
        Gcls = G.clone()
        Gcls[1:] = 0
        clo.gather_with_medoids(xr, T, Tn, ids.unsqueeze(0).expand(P, K)).backward(Gcls)
        B = x.shape[1] // T
        Gtok = G[1:].permute(1, 0, 2).reshape(B, Tn, K, -1).permute(1, 0, 2, 3).reshape(P, K, -1)   # problem p = s * B + b
        tg = torch.zeros(P, (T // Tn) * (x.shape[0] - 1), x.shape[2])
        for k in range(K):
            tg[:, int(ids[k])] += Gtok[:, k]
        xt = torch.zeros_like(x, requires_grad=True)         # the tokens' gradient back in x's layout: a permutation
        (co.regroup_segments(xt, T, Tn)[0] * tg).sum().backward()
        return xr.grad + xt.grad, None, None
    y = co.literal_token_cluster_variant(xr, T, Tn, K, "kmediods++", None if agg == 0 else "mean", er, mr,
                                         assign=asg, medoids=med)
    y.backward(G)
    return xr.grad, (er.grad if er is not None else None), (mr.grad.reshape(-1) if mr is not None else None)


@pytest.mark.parametrize("W", [768, 1024])
@pytest.mark.parametrize("case", CLUSTER_CASES)
def test_token_cluster_backward_at_shipped_widths(case, W):
    """cc_token_cluster_backward_f32 at B = 16, T = 12 -> 3, n = K = 49, W = 768 / 1024 (the w0 loop over 256-column strips),
    both layouts: grad_x bit for bit against float32 autograd of the oracle (a copy, one exact division per element, or -
    for fixed 'sparse_sampling' ids that repeat - the same ascending sum); the cluster_embed / cls_multiplier gradients
    within (chain) * 2^-24 * sum|terms|."""
    from centerclip_amd import _lib as L
    B, T, Tn, n, K = 16, 12, 3, 49, 49
    N = (T // Tn) * n
    g = torch.Generator(device="cpu").manual_seed(W + CLUSTER_CASES.index(case))
    x = torch.randn(1 + n, B * T, W, generator=g)
    G = torch.randn(1 + K, B * Tn, W, generator=g)
    algo, agg = (2, 0) if case == "sparse_repeat" else (0, 1 if case == "mean" else 0)
    embed = mult = ids = None
    if case == "embed_mult":
        embed = torch.randn(K, W, generator=g) * W ** -0.5
        mult = 0.25 + torch.rand(T, generator=g)
    if case == "sparse_repeat":
        ids = torch.sort(torch.randint(0, N, (K,), generator=g)).values
        ids[10:14] = ids[10]                                     # one id four times, another twice
        ids[30:32] = ids[30]
    dv = lambda t: None if t is None else t.to(DEV)
    ref, ref_sel = None, None
    for frame_major in (False, True):
        xd = (x.permute(1, 0, 2).contiguous() if frame_major else x).to(DEV).requires_grad_(True)
        ed = dv(embed).requires_grad_(True) if embed is not None else None
        md = dv(mult).requires_grad_(True) if mult is not None else None
        out, med, asg = torch.ops.centerclip.token_cluster_train(xd, frame_major, T, Tn, K, L.METRIC_IDS["euclidean"], 2.0,
                                                                 1e-6, 100, 16, False, algo, agg, ed, md, dv(ids))
        out.backward((G.permute(1, 0, 2).contiguous() if frame_major else G).to(DEV))
        gx = (xd.grad.permute(1, 0, 2) if frame_major else xd.grad).cpu()
        sel = None
        if algo == 0:
            assert tuple(med.shape) == (B * Tn, K) and bool((med[:, 1:] > med[:, :-1]).all()) and int(med.max()) < N
            sel = (med.cpu(), asg.cpu())
        if ref is None or not all(torch.equal(a, b) for a, b in zip(sel or (), ref_sel or ())):
            ref = _ref_cluster_grads(x, G, T, Tn, K, agg, *(sel or (None, None)), embed, mult, ids)
            ref_sel = sel
        rx, re, rm = ref
        assert torch.equal(gx, rx), (case, W, frame_major, float((gx - rx).abs().max()))
        if embed is not None:                                    # sum over the B * T_new segments of G[1 + k]
            bound = (B * Tn + 2) * U * G[1:].abs().sum(1)
            assert bool(((ed.grad.cpu() - re).abs() <= bound).all()), (case, W, frame_major)
        if mult is not None:                                     # sum over b, w of (G[0] / fd) cls: lane-strided chains
            fd = T // Tn
            g0 = G[0].reshape(B, Tn, W).repeat_interleave(fd, dim=1)
            bound = (B * W / 64 + 8) * U * ((g0 / fd) * x[0].reshape(B, T, W)).abs().sum((0, 2))
            assert bool(((md.grad.cpu() - rm).abs() <= bound).all()), (case, W, frame_major)


# ------------------------------------------------------------------------------------------------ LinearFunction
LINEAR_CASES = {  # name: (M, K, N, input gradient, bias, weight as the .t() view of a [K, N] parameter)
    "patch_embed": (9408, 3072, 768, False, False, False),      # cfg 2: B * T * 49 patch rows of 3 * 32 * 32 against conv1
    "patch_embed_dx_bias": (9408, 3072, 768, True, True, False),
    "visual_proj": (48, 768, 512, True, False, True),           # ln_post(CLS rows of B * T_new segments) @ visual.proj
    "visual_proj_b64": (256, 768, 512, True, False, True),      # cfg 3 per GPU: B 64 x 4 segments
    "text_projection": (16, 512, 512, True, False, True),       # ln_final(EOT rows) @ text_projection
}


@pytest.mark.parametrize("name", sorted(LINEAR_CASES))
def test_linear_function_at_patch_and_head_shapes(name):
    """train.LinearFunction (fp16 operands, fp32 accumulation, the scaled-fp16 dY of the backward) at the patch embedding
    and projection-head shapes, the heads through the .t() views encode_*_train pass: y, dW, db and dx within
    (2 * 2^-11 + chain * 2^-24) * sum|terms| of float64 on the same fp16-representable x and W."""
    from centerclip_amd.train import LinearFunction
    M, K, N, x_grad, bias, view = LINEAR_CASES[name]
    g = torch.Generator(device="cpu").manual_seed(M + K + N)
    x = (torch.randn(M, K, generator=g) * 0.5).half().float().to(DEV)
    shape = (K, N) if view else (N, K)
    param = torch.nn.Parameter((torch.randn(*shape, generator=g) * K ** -0.5).half().float().to(DEV))
    w = param.t() if view else param
    b = torch.nn.Parameter((torch.randn(N, generator=g) * 0.1).to(DEV)) if bias else None
    dy = (torch.randn(M, N, generator=g) * 1e-2).to(DEV)
    xi = x.clone().requires_grad_(x_grad)
    y = LinearFunction.apply(xi, w, b)
    y.backward(dy)
    torch.cuda.synchronize()
    x64, w64, dy64 = x.double(), w.detach().double(), dy.double()
    y64 = x64 @ w64.t() + (b.detach().double() if bias else 0)
    q_y = float(((y.double() - y64).abs() / ((K + 8) * U * (x64.abs() @ w64.abs().t() + (b.detach().double().abs() if bias else 0)))).max())
    assert param.grad.shape == param.shape
    dw = param.grad.t() if view else param.grad
    dw64 = dy64.t() @ x64                                          # the gradient of the [N, K] weight (view)
    q_dw = float(((dw.double() - dw64).abs() / ((2 * H + (M + 64) * U) * (dy64.abs().t() @ x64.abs()))).max())
    q_db = q_dx = 0.0
    if bias:
        q_db = float(((b.grad.double() - dy64.sum(0)).abs() / ((2 * H + (M + 64) * U) * dy64.abs().sum(0))).max())
    if x_grad:
        q_dx = float(((xi.grad.double() - dy64 @ w64).abs() / ((2 * H + (N + 64) * U) * (dy64.abs() @ w64.abs()))).max())
    else:
        assert xi.grad is None
    print(f"[linear {name}] error / bound: y {q_y:.2f} dW {q_dw:.2f} db {q_db:.2f} dx {q_dx:.2f}; relative dW "
          f"{_rel(dw, dw64):.1e}" + (f" dx {_rel(xi.grad, dy64 @ w64):.1e}" if x_grad else ""))
    assert q_y <= 1.0 and q_dw <= 1.0 and q_db <= 1.0 and q_dx <= 1.0, (q_y, q_dw, q_db, q_dx)
