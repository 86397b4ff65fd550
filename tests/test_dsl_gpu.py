"""camoe_dsl on the MI355X (``-m gpu``): the evaluation kernels (cc_dsl_col_stats_f32 / _rescale_stats_f32 / _apply_f32), the DSL
loss with its gradient inside the fused chain (cc_contrastive_loss_grad_dsl[_dev]_f32), the whole training step eager and
captured, and eval_epoch / _run_on_single_gpu with the flag - all against the float64 restatements of tests/dsl_ref.py.
Measured maxima are printed by every test (pytest -s) and recorded in DESIGN.md ("camoe_dsl")."""
import math
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import dsl_ref as R
from centerclip_amd import torch_ops  # noqa: F401  (registers torch.ops.centerclip)
from oracle.recipes import EVAL_CASES, eval_case_batches, loss_grad_case, s3_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(HERE, "golden", "r2_golden.npz"))


@pytest.fixture(scope="module")
def g3():
    return np.load(os.path.join(HERE, "golden", "r3_golden.npz"))


# ------------------------------------------------------------------------------------------------ 1. column stats + apply
def _matrix(rows, cols, seed):
    """Logits up to the clamp of logit_scale (+-100: most terms of a column underflow), columns of a narrow range (many terms
    count), column 0 constant, column 2 with one NaN (cols >= 3)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-100.0, 100.0, size=(rows, cols)).astype(np.float32)
    narrow = np.arange(cols) % 3 == 1
    x[:, narrow] = rng.normal(20.0, 1.5, size=(rows, int(narrow.sum()))).astype(np.float32)
    x[:, 0] = np.float32(-37.25)
    nan_col = 2 if cols >= 3 else None
    if nan_col is not None:
        x[rows // 2, nan_col] = np.nan
    return x, nan_col


STATS_CASES = [(1, 1, 1, None), (3, 5, 2, None), (257, 130, 3, None), (1203, 517, 4, 640), (10000, 1000, 5, None)]
_ref_cache = {}


def _case(rows, cols, seed, stride):
    """-> (host matrix, NaN column, device view [rows, cols] with the row stride asked for, its backing tensor)"""
    key = (rows, cols, seed)
    if key not in _ref_cache:
        x, nan_col = _matrix(rows, cols, seed)
        m64, s64 = R.col_stats64(x)
        _ref_cache[key] = (x, nan_col, m64, s64, R.dual_softmax64(x))
    x, nan_col, m64, s64, d64 = _ref_cache[key]
    back = torch.full((rows, stride or cols), 7.0, device=DEV)
    view = back[:, :cols]
    view.copy_(torch.from_numpy(x))
    return x, nan_col, m64, s64, d64, view, back


@pytest.mark.parametrize("rows,cols,seed,stride", STATS_CASES)
def test_col_stats_and_apply_against_float64(rows, cols, seed, stride):
    """m exactly, s within the running-error bound derived from the inputs (dsl_ref.stats_bound), D within that bound carried
    through the rewrite; the NaN column is NaN in m, s and D and leaves every other column alone; padding beyond `cols` of a
    strided matrix is not touched; a second call gives the same bits."""
    x, nan_col, m64, s64, d64, view, back = _case(rows, cols, seed, stride)
    m, s = torch.ops.centerclip.dsl_col_stats(view)
    m2, s2 = torch.ops.centerclip.dsl_col_stats(view)
    ok = np.ones(cols, dtype=bool)
    if nan_col is not None:
        ok[nan_col] = False
        assert bool(torch.isnan(m[nan_col])) and bool(torch.isnan(s[nan_col]))
    okt = torch.from_numpy(ok).to(DEV)
    assert torch.equal(m[okt], m2[okt]) and torch.equal(s[okt], s2[okt])
    mh, sh = m.cpu().numpy().astype(np.float64), s.cpu().numpy().astype(np.float64)
    assert np.array_equal(mh[ok], m64[ok])
    bound, depth = R.stats_bound(x[:, ok])
    err = np.abs(sh[ok] - s64[ok])
    print(f"[dsl stats {rows}x{cols}] depth {depth}: max |s - s64| / s64 = {float((err / s64[ok]).max()):.2e}, "
          f"worst error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    torch.ops.centerclip.dsl_apply_(view, m, s, rows)
    d = view.cpu().numpy().astype(np.float64)
    if nan_col is not None:
        assert np.isnan(d[:, nan_col]).all()
    assert np.isfinite(d[:, ok]).all()
    db = R.d_bound(x[:, ok], rows, bound)
    derr = np.abs(d[:, ok] - d64[:, ok])
    scale = np.abs(d64[:, ok]).max()
    print(f"[dsl apply {rows}x{cols}] max |D - D64| = {float(derr.max()):.2e} (max |D| {float(scale):.3g}), "
          f"worst error / bound = {float((derr / db).max()):.3f}")
    assert (derr <= db).all()
    if stride:
        assert bool((back[:, cols:] == 7.0).all())
    # ops.dual_softmax: a new tensor with the same bits, the input untouched
    _, _, _, _, _, fresh, _ = _case(rows, cols, seed, stride)
    keep = fresh.clone()
    from centerclip_amd import ops
    out = ops.dual_softmax(fresh)
    assert torch.equal(out[:, okt], view[:, okt]) and torch.equal(fresh[:, okt], keep[:, okt]) and out.data_ptr() != fresh.data_ptr()


def test_col_stats_of_no_rows_is_the_neutral_element():
    m, s = torch.ops.centerclip.dsl_col_stats(torch.zeros(0, 130, device=DEV))
    assert bool((m == float("-inf")).all()) and bool((s == 0).all()) and m.shape == s.shape == (130,)
    empty = torch.zeros(0, 130, device=DEV)
    torch.ops.centerclip.dsl_apply_(empty, m, s, 5)         # nothing to rewrite, no launch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. shard merge
def test_shard_merge_on_one_device():
    """Two row blocks of 257 x 130 as two ranks would hold them: stats of each, MAX of m, rescale, SUM of s - against the
    whole-matrix float64 stats within the bound with one more merge level; one block empty: the other block's bits."""
    x, nan_col, m64, s64, _, view, _ = _case(257, 130, 3, None)
    ok = np.ones(130, dtype=bool)
    ok[nan_col] = False
    op = torch.ops.centerclip
    halves = [view[:128].contiguous(), view[128:].contiguous()]
    stats = [op.dsl_col_stats(h) for h in halves]
    m_all = torch.maximum(stats[0][0], stats[1][0])
    parts = []
    for m_loc, s_loc in stats:
        s_loc = s_loc.clone()
        op.dsl_rescale_stats_(s_loc, m_loc, m_all)
        parts.append(s_loc)
    s_all = (parts[0] + parts[1]).cpu().numpy().astype(np.float64)
    assert np.array_equal(m_all.cpu().numpy().astype(np.float64)[ok], m64[ok])
    bound, depth = R.stats_bound(x[:, ok], merges=1)
    err = np.abs(s_all[ok] - s64[ok])
    print(f"[dsl shard merge] depth {depth}: worst error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # one half empty
    m_e, s_e = op.dsl_col_stats(view[:0])
    m_o, s_o = op.dsl_col_stats(view)
    okt = torch.from_numpy(ok).to(DEV)
    m_g = torch.maximum(m_o, m_e)
    s_keep, s_none = s_o.clone(), s_e.clone()
    op.dsl_rescale_stats_(s_keep, m_o, m_g)
    op.dsl_rescale_stats_(s_none, m_e, m_g)
    assert torch.equal(m_g[okt], m_o[okt]) and torch.equal((s_keep + s_none)[okt], s_o[okt]) and bool((s_none[okt] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. get_similarity_logits
def _eval_model(g2, cluster_inter, **extra):
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    cfg = g2["s1_cfg"]
    T, T_new = int(cfg[11]), int(cfg[12])
    a = Namespace(cluster_inter=cluster_inter, deep_cluster=0, cluster_algo='kmediods++', max_frames=T,
                  target_frames_blocks=[4, T_new, T_new] if cluster_inter else [T, T, T], cluster_num_blocks=[16, 6, 6],
                  cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100, minkowski_norm_p=2.0,
                  aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True, sim_header='meanP',
                  linear_patch='2d', pre_visual_pooling=0, **extra)
    return CLIP4Clip.from_state_dict(sd, a).to(DEV).eval(), sd, cfg


def test_get_similarity_logits_applies_the_dual_softmax(g2):
    from centerclip_amd import ops
    off, _, cfg = _eval_model(g2, 1)
    on, _, _ = _eval_model(g2, 1, camoe_dsl=1)
    assert on.camoe_dsl and not off.camoe_dsl
    seq_list, vis_list, list_t, list_v = s3_case(int(cfg[0]), int(cfg[11]), int(cfg[12]))
    seq, vis = seq_list[0].to(DEV), vis_list[1].to(DEV)                 # (video batch 1 has no fully masked clip)
    amask, vmask = list_t[0][0].to(DEV), list_v[1][0].to(DEV)
    with torch.no_grad():
        plain, _ = off.get_similarity_logits(seq, vis, amask, vmask)
        got, _ = on.get_similarity_logits(seq, vis, amask, vmask)
    assert torch.equal(got, ops.dual_softmax(plain)) and not torch.equal(got, plain)


# ------------------------------------------------------------------------------------------------ 4. loss and gradient
def _c_call(text, vis, mask, ls, grad_scale, ls_dev=None):
    """cc_contrastive_loss_grad_dsl_f32 (ls_dev None) or _dsl_dev_f32 through the C ABI, for an incoming gradient grad_scale"""
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    n, Tn, E = vis.shape
    lib = L.lib()
    loss3, dt, dv, dls = torch.empty(3, device=DEV), torch.empty_like(text), torch.empty_like(vis), torch.empty(1, device=DEV)
    ws = L.workspace(lib.cc_contrastive_grad_dsl_workspace_bytes(n, Tn, E), text.device)
    head = (L.ptr(text), L.ptr(vis), L.ptr(mask), mask.stride(0), mask.stride(1), n, Tn, E)
    tail = (float(grad_scale), L.ptr(loss3), L.ptr(dt), L.ptr(dv), L.ptr(dls), L.ptr(ws), ws.numel(), _st(text))
    if ls_dev is None:
        rc = lib.cc_contrastive_loss_grad_dsl_f32(*head, float(ls), *tail)
    else:
        rc = lib.cc_contrastive_loss_grad_dsl_dev_f32(*head, 0.0, L.ptr(ls_dev), *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return loss3, dt, dv, dls


@pytest.mark.parametrize("tag,n", [("lg_a", 6), ("lg_b", 33)])
def test_dsl_loss_and_gradients_against_float64_autograd(g2, g3, tag, n):
    """contrastive_loss(dsl=True) on the inputs of the lg_* fixtures (masks with zeros, logit scales 2.0 and 3.5) against
    float64 torch.autograd of the restated formula.  Tolerance: the larger of the plain loss test's bounds (2e-5 on the loss
    values, 1e-4 relative to the largest entry on the gradients) and 4 x the error an fp32 CPU evaluation of the same formula
    makes against float64 - D reaches n * 100, so the plain bounds need not transfer, and a fixed-order wave-tree fp32 sum has
    no reason to be more than a small factor from ATen's fp32."""
    from centerclip_amd.losses import contrastive_loss
    cfg = g2["s1_cfg"]
    seq, vis, vmask = loss_grad_case(tag, n, int(cfg[12]), int(cfg[0]))
    scale = float(g3[f"{tag}_scale"])
    ref = R.dsl_loss64(seq, vis, vmask, scale, torch.float64)
    f32 = R.dsl_loss64(seq, vis, vmask, scale, torch.float32)
    rel = lambda a, b: float((a.double() - b).abs().max() / max(float(b.abs().max()), 1e-30))
    seq_t = torch.from_numpy(seq).to(DEV).requires_grad_(True)
    vis_t = torch.from_numpy(vis).to(DEV).requires_grad_(True)
    ls = torch.tensor(scale, device=DEV, requires_grad=True)
    mask = torch.from_numpy(vmask).to(DEV)
    loss, l1, l2 = contrastive_loss(seq_t, vis_t, mask, ls, dsl=True)
    (4.0 * loss).backward()
    got3 = torch.stack([l1, l2, loss]).detach().cpu()
    e_loss, e_loss32 = float((got3.double() - ref[0]).abs().max()), float((f32[0].double() - ref[0]).abs().max())
    errs = dict(d_seq=(rel(seq_t.grad.cpu() / 4.0, ref[1]), rel(f32[1], ref[1])),
                d_vis=(rel(vis_t.grad.cpu() / 4.0, ref[2]), rel(f32[2], ref[2])),
                d_ls=(abs(float(ls.grad) / 4.0 - float(ref[3])) / max(1.0, abs(float(ref[3]))),
                      abs(float(f32[3]) - float(ref[3])) / max(1.0, abs(float(ref[3])))))
    print(f"[dsl loss {tag}] loss {float(ref[0][2]):.6f}: |loss3 - f64| HIP {e_loss:.2e}, fp32 CPU {e_loss32:.2e}; "
          + "; ".join(f"{k} HIP {a:.2e}, fp32 CPU {b:.2e}" for k, (a, b) in errs.items()))
    assert e_loss <= max(2e-5, 4 * e_loss32)
    for k, (a, b) in errs.items():
        assert a <= max(1e-4, 4 * b), k
    # the plain loss is something else (the flag is not ignored)
    plain, _, _ = contrastive_loss(seq_t.detach(), vis_t.detach(), mask, ls.detach())
    assert abs(float(plain) - float(loss)) > 1e-3
    # the same bits on a second call, and through the host-scalar entry point
    text, visd = seq_t.detach().reshape(n, -1).contiguous(), vis_t.detach().contiguous()
    a = _c_call(text, visd, mask, scale, 1.0, ls_dev=torch.tensor([scale], device=DEV))
    b = _c_call(text, visd, mask, scale, 1.0, ls_dev=torch.tensor([scale], device=DEV))
    h = _c_call(text, visd, mask, scale, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, h))
    assert torch.equal(a[0][2], loss.detach()) and torch.equal(a[1] * 4.0, seq_t.grad.reshape(n, -1))
    # incoming gradients 2^k scale every gradient exactly; the loss values do not move
    for k in (-3, 16):
        s = _c_call(text, visd, mask, scale, 2.0 ** k)
        assert torch.equal(s[0], a[0]) and all(torch.equal(x, y * 2.0 ** k) for x, y in zip(s[1:], a[1:])), k


# ------------------------------------------------------------------------------------------------ 5. the whole step
def _model_and_batch(camoe_dsl=1):
    from centerclip_amd.clip4clip import CLIP4Clip
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    B, T = int(g["cfg"][10]), int(g["cfg"][11])
    cfg = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                    cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                    minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                    sim_header='meanP', linear_patch='2d', camoe_dsl=camoe_dsl)
    video = torch.from_numpy(g["video"]).view(B, 1, T, 3, 64, 64)
    ids = torch.from_numpy(g["t_ids"])[:B]
    batch = (ids, (ids > 0).long(), torch.zeros_like(ids), video, torch.ones(B, 1, T, dtype=torch.long))
    return (lambda: CLIP4Clip.from_state_dict(dict(sd), cfg).float().to(DEV)), batch


def test_training_forward_uses_the_dsl_loss_and_reaches_every_parameter():
    from centerclip_amd.losses import contrastive_loss
    grads = {}
    for flag in (0, 1):
        make, batch = _model_and_batch(flag)
        m = make().train()
        ids, amask, seg, video, vmask = (t.to(DEV) for t in batch)
        out = m(ids, seg, amask, video, vmask)
        out["loss"].backward()
        grads[flag] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        seg_mask = m.get_video_mask_after_cluster(vmask.view(-1, vmask.shape[-1]))
        want, _, _ = contrastive_loss(out["sequence_output"].detach(), out["visual_output"].detach(), seg_mask,
                                      m.clip.logit_scale.detach(), dsl=bool(flag))
        assert torch.equal(out["sim_loss"].detach(), want), flag
        losses = grads.setdefault("loss", {})
        losses[flag] = float(out["sim_loss"])
    assert abs(grads["loss"][0] - grads["loss"][1]) > 1e-4
    assert len(grads[0]) > 20 and set(grads[0]) <= set(grads[1])
    assert all(bool(torch.isfinite(g).all()) for g in grads[1].values())
    assert any(not torch.equal(grads[0][n], grads[1][n]) for n in grads[0])


def _build(opt_name, capturable):
    from centerclip_amd.train import AdamW, BertAdam, lr_scheduler, prep_optim_params_groups
    make, batch = _model_and_batch()
    args = Namespace(optim=opt_name, lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0 if opt_name == "AdamW" else None)
    m = make()
    if opt_name == "AdamW":
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd,
                  capturable=capturable)
        return m, o, lr_scheduler('cos', init_lr=args.lr, all_iters=10, slow_start_iters=1, weight_decay=args.wd), args, batch
    o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                 e=1e-6, max_grad_norm=1.0, capturable=capturable)
    return m, o, None, args, batch


def _state(m, o):
    out = {n: p.detach().clone() for n, p in m.named_parameters()}
    for n, p in m.named_parameters():
        st = o.state.get(p, {})
        for k in sorted(st):
            out[n + "/" + k] = st[k].clone() if torch.is_tensor(st[k]) else torch.tensor(float(st[k]))
    return out


@pytest.mark.parametrize("opt_name", ["BertAdam", "AdamW"])
def test_three_captured_dsl_steps_equal_three_eager_steps(opt_name):
    """GraphedTrainStep captures the camoe_dsl step as it is (no host read in the loss chain): three replays == three eager
    train_epoch steps, every parameter and optimizer moment bit for bit.  BertAdam without a scaler; AdamW + DeviceGradScaler."""
    from centerclip_amd.train import DeviceGradScaler, GraphedTrainStep, train_epoch
    runs = []
    for captured in (False, True):
        m, o, sched, args, batch = _build(opt_name, captured)
        assert m.camoe_dsl
        sc = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000) if opt_name == "AdamW" else None
        if captured:
            stepper = GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=args.clip_grad_norm, scaler=sc)
            for _ in range(3):
                loss = stepper(batch)
            stepper.sync()
            assert stepper.global_step == 3
        else:
            gs = 0
            for _ in range(3):
                loss, gs = train_epoch(0, args, m, [batch], DEV, o, gs, scheduler=sched, scaler=sc)
            assert gs == 3
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        if sc is not None:
            assert sc.counters() == (3, 0)
        runs.append(_state(m, o))
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert torch.equal(runs[0][k].cpu(), runs[1][k].cpu()), k
    init = {n: p.detach().clone() for n, p in _model_and_batch()[0]().named_parameters()}
    assert max(float((runs[0][n] - init[n]).abs().max()) for n in init) > 0


# ------------------------------------------------------------------------------------------------ 6. evaluation
class _Loader(list):
    pass


class _Spy:
    """HipBackend that records the matrix before and after the rewrite"""

    @staticmethod
    def make(ev, seen):
        class Spy(ev.HipBackend):
            @classmethod
            def dot_operands(cls, t_op, v_op, n_video, mult):
                out = super().dot_operands(t_op, v_op, n_video, mult)
                seen["S"] = out.clone()
                return out

            @staticmethod
            def dsl_apply(sim, m, s, n_total):
                seen["n_total"] = n_total
                seen["D"] = ev.HipBackend.dsl_apply(sim, m, s, n_total).clone()
                return sim
        return Spy


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_eval_epoch_with_camoe_dsl_on_the_fixture_loaders(g2, g3, name):
    """eval_epoch(camoe_dsl=True) on the ev_* loaders with the fixture model.  Measured here (printed): the re-ranked matrix is
    3.6e-3 (multi) and 1.8e-3 (single) from the float64 dual softmax of the fixture's stored reference matrix ev_<name>_sim - the
    towers' fp16 error,
    amplified by n P (1 + S) - while the smallest gap of that re-ranked reference between a ground-truth entry and a competitor
    is 2.1e-3 (multi) and 8.9e-4 (single): the fixtures are NOT pinned after re-ranking, so the comparison of the metric strings
    against an independent reference is made on planted features (the next test).  What holds on the fixture loaders and is
    asserted: the rewrite equals the float64 dual softmax of the loop's own matrix within the stats bound, that matrix is pinned
    at 10 x the rewrite's error, and R@1 and the four strings are the restated metrics of it, character for character; the flag
    through args and off.  (The ev_* loaders hold a clip with one masked frame; the FULLY masked clip - a NaN column - is in the
    s3 fixture of test_run_on_single_gpu_with_camoe_dsl.)"""
    from centerclip_amd import eval as ev
    model, sd, cfg = _eval_model(g2, 0)
    batches, attrs = eval_case_batches(EVAL_CASES[name], cfg)
    loader = _Loader(batches)
    loader.dataset = Namespace(**attrs)
    sentences = EVAL_CASES[name]["sentences"] if attrs else None
    seen = {}
    ref64 = R.dual_softmax64(g3[f"ev_{name}_sim"])
    a = Namespace(inference_speed_test=False)
    r1, _, info = ev.eval_epoch(model, loader, torch.device(DEV), args=a, backend=_Spy.make(ev, seen), camoe_dsl=True)
    s_own, d_own = seen["S"].cpu().numpy(), seen["D"].cpu().numpy().astype(np.float64)
    d64 = R.dual_softmax64(s_own)
    err, gap = np.abs(d_own - d64), R.rank_gap(d64, sentences)
    bound = R.d_bound(s_own, s_own.shape[0], R.stats_bound(s_own)[0])
    print(f"[eval_epoch camoe_dsl {name}] max |D - D64(fixture reference)| = {float(np.abs(d_own - ref64).max()):.2e}, rank gap of "
          f"the re-ranked reference {R.rank_gap(ref64, sentences):.2e}; against the loop's own matrix: max |D - D64| = "
          f"{float(err.max()):.2e}, rank gap {gap:.2e}")
    assert seen["n_total"] == s_own.shape[0] and (err <= bound).all()
    assert gap > 10 * float(err.max())
    r1_want, info_want = R.metrics64(d64, sentences)
    assert abs(r1 - r1_want) < 1e-4 and list(info) == info_want
    via_args = ev.eval_epoch(model, loader, torch.device(DEV), args=Namespace(inference_speed_test=False, camoe_dsl=1))
    assert list(via_args[2]) == info_want
    assert list(ev.eval_epoch(model, loader, torch.device(DEV), args=a)[2]) == [str(s) for s in g3[f"ev_{name}_info"]]


class _PlantedModel(torch.nn.Module):
    """Stands in for the towers: text features are looked up by the id in column 0, 'frames' are the per-segment features."""
    sim_header = "meanP"

    def __init__(self, text):
        super().__init__()
        self.text = text.to(DEV)

    def forward(self, input_ids=None, token_type_ids=None, attention_mask=None, video=None, video_mask=None):
        out = {'sequence_output': None, 'visual_output': None}
        if input_ids is not None:
            out['sequence_output'] = self.text[input_ids.view(-1, input_ids.shape[-1])[:, 0]].unsqueeze(1)
        if video is not None:
            out['visual_output'] = video[:, 0].float()
        return out

    def get_video_mask_after_cluster(self, m):
        return m

    def _logit_scale_value(self):
        return 2.0


def _planted(sentences, seed, E=64, T=3):
    """Features whose cosine matrix is planted: the videos' pooled directions are orthonormal (every frame of clip v is a
    positive multiple of q_v, one clip has a masked frame), text i = sum_v C[i, v] q_v + the rest of its unit length in another
    orthogonal direction, with C a shuffled lattice over [-0.1, 0.1] - logits exp(2) * C, no two closer than 1.5 / (Nt Nv).  The
    seeds of the two cases were picked on the CPU so that the RE-RANKED float64 matrix keeps a wide gap (0.046 / 0.042) - the
    column softmax squeezes the entries it suppresses towards 0, and with them their distances - against the few 1e-4 that
    rounding the text side to fp16 (the loop's default operand precision) moves it, and so that re-ranking changes the metric
    strings; the test asserts the gap it needs.
    -> (text [Nt, E] fp32, batches, dataset attributes, float64 logit matrix computed from the fp32 features)."""
    rng = np.random.default_rng(seed)
    nv, nt = len(sentences), int(sum(sentences))
    q, _ = np.linalg.qr(rng.normal(size=(E, E)))
    q = q.T                                                            # rows: orthonormal directions
    c = (rng.permutation(nt * nv).reshape(nt, nv) / (nt * nv - 1.0) - 0.5) * 0.2
    text = c @ q[:nv] + np.sqrt(1.0 - (c ** 2).sum(axis=1, keepdims=True)) * q[nv + np.arange(nt) % (E - nv)]
    text = (text * rng.uniform(0.5, 2.0, size=(nt, 1))).astype(np.float32)
    frames = (q[:nv, None, :] * rng.uniform(0.5, 2.0, size=(nv, T, 1))).astype(np.float32)
    vmask = np.ones((nv, T), dtype=np.int64)
    vmask[1, T - 1] = 0
    items, gt = [], np.repeat(np.arange(nv), sentences)
    for i in range(nt):
        ids = np.zeros((1, 4), dtype=np.int64)
        ids[0, 0] = i
        items.append((ids, np.ones_like(ids), np.zeros_like(ids), frames[gt[i]][None], vmask[gt[i]][None]))
    batches = [tuple(torch.from_numpy(np.stack([it[k] for it in items[s:s + 4]])) for k in range(5)) for s in range(0, nt, 4)]
    attrs = {}
    if any(n != 1 for n in sentences):
        attrs = dict(multi_sentence_per_video=True, cut_off_points=list(np.cumsum(sentences)), sentence_num=nt, video_num=nv)
    t64 = text.astype(np.float64)
    t64 /= np.linalg.norm(t64, axis=1, keepdims=True)
    f64 = frames.astype(np.float64)
    f64 /= np.linalg.norm(f64, axis=2, keepdims=True)
    p64 = (f64 * vmask[:, :, None]).sum(axis=1) / vmask.sum(axis=1, keepdims=True)
    p64 /= np.linalg.norm(p64, axis=1, keepdims=True)
    return torch.from_numpy(text), batches, attrs, math.exp(2.0) * t64 @ p64.T


@pytest.mark.parametrize("name,sentences,seed", [("single", [1] * 6, 328), ("multi", [3, 1, 4, 2, 3], 345)])
def test_eval_epoch_with_camoe_dsl_against_the_restated_reference_on_planted_features(name, sentences, seed):
    """The ev_* fixtures are not pinned after re-ranking (previous test), so - same protocols, same shapes - features with a
    planted margin: eval_epoch(camoe_dsl=True) through HipBackend against the float64 restatement from the features (logits,
    dual softmax, metrics): the re-ranked matrix within 1e-3 * exp(logit_scale) as the plain loop's contract reads, the smallest
    gap between a ground-truth entry and a competitor above 10 x the measured matrix error, then R@1 and the four metric
    strings character for character.  Both the default operand precision and similarity_products=3."""
    from centerclip_amd import eval as ev
    text, batches, attrs, s64 = _planted(sentences, seed)
    model = _PlantedModel(text)
    loader = _Loader(batches)
    loader.dataset = Namespace(**attrs)
    multi = sentences if attrs else None
    d64 = R.dual_softmax64(s64)
    gap = R.rank_gap(d64, multi)
    r1_want, info_want = R.metrics64(d64, multi)
    for products in (None, 3):
        seen = {}
        r1, _, info = ev.eval_epoch(model, loader, torch.device(DEV), args=Namespace(inference_speed_test=False),
                                    backend=_Spy.make(ev, seen), in_flight=1, camoe_dsl=True, similarity_products=products)
        err = float(np.abs(seen["D"].cpu().numpy() - d64).max())
        print(f"[eval_epoch camoe_dsl planted {name}, products {products}] max |D - D64| = {err:.2e}, smallest rank gap {gap:.2e}")
        assert seen["D"].shape == d64.shape and seen["n_total"] == d64.shape[0]
        assert err <= 1e-3 * math.exp(2.0) and gap > 10 * err
        assert abs(r1 - r1_want) < 1e-4 and list(info) == info_want
    plain = ev.eval_epoch(model, loader, torch.device(DEV), args=Namespace(inference_speed_test=False), in_flight=1)
    assert list(plain[2]) == R.metrics64(s64, multi)[1] and list(plain[2]) != info_want


def test_run_on_single_gpu_with_camoe_dsl(g2):
    """main.py:526-532: args.camoe_dsl = 1 -> the dual softmax once over the whole [37, 21] matrix of the s3 fixture (ragged
    batches, a fully masked clip: column 5 stays NaN, every other column is re-ranked) - within the stats bound of the matrix
    the same call returns with the flag off; the model's attribute does the same; off stays off."""
    from centerclip_amd.eval import _run_on_single_gpu
    model, sd, cfg = _eval_model(g2, 1)
    seq_list, vis_list, list_t, list_v = s3_case(int(cfg[0]), int(cfg[11]), int(cfg[12]))
    to = lambda ts: [tuple(t.to(DEV) for t in item) if isinstance(item, tuple) else item.to(DEV) for item in ts]
    with torch.no_grad():
        plain = _run_on_single_gpu(model, to(list_t), to(list_v), to(seq_list), to(vis_list), args=Namespace(camoe_dsl=0))
        got = _run_on_single_gpu(model, to(list_t), to(list_v), to(seq_list), to(vis_list), args=Namespace(camoe_dsl=1))
        none = _run_on_single_gpu(model, to(list_t), to(list_v), to(seq_list), to(vis_list))
        model.camoe_dsl = True
        attr = _run_on_single_gpu(model, to(list_t), to(list_v), to(seq_list), to(vis_list))
    assert isinstance(got, np.ndarray) and got.shape == plain.shape == (37, 21)
    assert np.array_equal(plain, none, equal_nan=True) and np.array_equal(got, attr, equal_nan=True)
    ok = np.ones(21, dtype=bool)
    ok[5] = False
    assert np.isnan(got[:, 5]).all() and np.isnan(plain[:, 5]).all() and np.isfinite(got[:, ok]).all()
    bound, _ = R.stats_bound(plain[:, ok])
    db = R.d_bound(plain[:, ok], 37, bound)
    derr = np.abs(got[:, ok].astype(np.float64) - R.dual_softmax64(plain[:, ok]))
    print(f"[_run_on_single_gpu camoe_dsl] max |D - D64| = {float(derr.max()):.2e}, worst error / bound = {float((derr / db).max()):.3f}")
    assert (derr <= db).all()


def test_two_ranks_on_one_gpu_sharded_dsl_equals_single_process():
    """World 2 over gloo with both ranks on cuda:0 (tests/dsl_worker.py): eval_epoch(shard=True, camoe_dsl=True) - local column
    stats, all-reduce MAX, rescale, all-reduce SUM, in-place rewrite with the dataset's Nt - equals the single-process call."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29583", os.path.join(HERE, "dsl_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "DSL_WORKER_OK world=2" in r.stdout
