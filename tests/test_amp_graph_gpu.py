"""Loss scaling on the device (train.DeviceGradScaler, the *_scaled_f32 / cc_grad_scaler_* entry points) eager and inside a
captured GraphedTrainStep; needs a real MI355X (``-m gpu``).  The statistics kernel against float64, the skippable optimizer
launches bit for bit, the scale update against torch.amp.GradScaler, the captured step with and without a scaler, a scripted
run with one skipped step (captured / eager DeviceGradScaler / eager torch GradScaler), a checkpoint round trip."""
import functools
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


# ------------------------------------------------------------------------------------------------ 1. the statistics kernel
STAT_SIZES = [5, 8193, 3 * 8192 + 17]            # none a multiple of a block (8192): a one-block tensor, two blocks, a partial last


def _stats(grads, inv_scale, max_norm):
    """cc_grad_norm_partials_f32 + cc_grad_scaler_stats_f32 through ctypes -> [norm, multiplier, found_inf] (floats)."""
    from centerclip_amd import _lib as L
    from centerclip_amd.train import _adamw_table
    lib = L.lib()
    raw, count, nblk = _adamw_table([(g, g, None, None, 0) for g in grads])
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    ws = torch.empty(lib.cc_grad_norm_workspace_bytes(nblk), dtype=torch.uint8, device=DEV)
    inv = torch.tensor([inv_scale], dtype=torch.float32, device=DEV)
    out = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    st = L.stream_ptr(torch.device(DEV))
    L.check(lib.cc_grad_norm_partials_f32(L.ptr(table), count, nblk, L.ptr(ws), ws.numel(), st), "partials")
    L.check(lib.cc_grad_scaler_stats_f32(L.ptr(ws), nblk, L.ptr(inv), float(max_norm), L.ptr(out), st), "stats")
    torch.cuda.synchronize()
    return out.tolist()


def _stat_grads():
    gen = torch.Generator().manual_seed(5)
    return [(torch.randn(n, generator=gen) * 2.0 ** 10 * 0.05).to(DEV) for n in STAT_SIZES]


@pytest.mark.parametrize("max_norm", [-1.0, 0.5, 1e4])
def test_stats_kernel_against_float64(max_norm):
    """Norm of the unscaled gradients and the multiplier inv_scale * min(1, max_norm / (norm + 1e-6)) against float64.
    Bounds: the fp64 partial sums are exact to ~n 2^-53, so the float norm is one rounding (2^-24) from the true one - 2^-23
    asked; the multiplier adds a float add, a divide and a multiply to it (4 roundings in all) - 5 * 2^-24 asked.  No clipping
    (max_norm < 0) and a clip that does not engage give inv_scale itself, exactly."""
    grads, inv = _stat_grads(), 2.0 ** -10
    norm, mult, found = _stats(grads, inv, max_norm)
    ref = float(torch.sqrt(sum((g.double() * inv).pow(2).sum() for g in grads)))
    print(f"[stats max_norm={max_norm}] norm {norm:.9g} (float64 {ref:.9g}), multiplier {mult:.9g}")
    assert found == 0.0 and abs(norm - ref) <= 2.0 ** -23 * ref
    if max_norm < 0 or max_norm > ref:
        assert mult == inv
    else:
        want = inv * max_norm / (ref + 1e-6)
        assert max_norm < ref and abs(mult - want) <= 5 * 2.0 ** -24 * want


@pytest.mark.parametrize("bad", [INF, float("nan")])
@pytest.mark.parametrize("where", ["first", "last", "last_partial_block"])
def test_stats_kernel_finds_one_inf_or_nan(bad, where):
    grads = _stat_grads()
    if where == "first":
        grads[0][0] = bad
    elif where == "last":
        grads[-1][-1] = bad
    else:
        grads[-1][3 * 8192 + 3] = bad            # inside the 17-element tail that the last block alone reads
    for max_norm in (-1.0, 1.0):
        assert _stats(grads, 2.0 ** -10, max_norm)[2] == 1.0


# ------------------------------------------------------------------------------------------------ 2. skippable launches
OPT_SIZES = [1, 3, 4, 8191, 8192, 8193, 3 * 8192 + 5, (1 << 17) + 3]


def _toy(kind, seed=0):
    from centerclip_amd.train import AdamW, BertAdam
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((0.5 * torch.randn(n, generator=gen)).to(DEV)) for n in OPT_SIZES]
    groups = [{'params': ps[0::2], 'weight_decay': 0.2}, {'params': ps[1::2], 'weight_decay': 0.0}]
    if kind == "AdamW":
        return ps, AdamW(groups, lr=1e-2, betas=(0.9, 0.98), eps=1e-6)
    return ps, BertAdam(groups, lr=1e-2, warmup=0.1, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98, e=1e-6,
                        max_grad_norm=1.0, capturable=(kind == "BertAdam-multi"))


def _toy_grads(step):
    gen = torch.Generator().manual_seed(100 + step)
    return [(torch.randn(n, generator=gen) * (0.1 if i % 2 else 3e-3)).to(DEV) for i, n in enumerate(OPT_SIZES)]


def _opt_tensors(ps, opt):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        st = opt.state[p]
        out += [st[k].clone() for k in sorted(st) if torch.is_tensor(st[k])]
    return out


@pytest.mark.parametrize("kind", ["AdamW", "BertAdam-multi", "BertAdam-single"])
def test_scaled_step_equals_the_step_on_divided_gradients_and_skips_bit_for_bit(kind):
    """DeviceGradScaler(2^10).step on gradients that carry the scale == optimizer.step() on the gradients divided by it, bit
    for bit (parameters, both moments, the gradients written back), over two steps; then one inf in ONE gradient element: the
    launches write nothing - every parameter and moment of every tensor keeps its bits, and the step is not counted.
    BertAdam-multi / BertAdam-single: the same record table and launch pair; they differ in how the learning rate is delivered
    (the group's device float / each record's own scheduled value)."""
    from centerclip_amd.train import DeviceGradScaler
    pa, oa = _toy(kind)
    pb, ob = _toy(kind)
    sc = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000)
    for step in range(2):
        for p, q, g in zip(pa, pb, _toy_grads(step)):
            p.grad, q.grad = g.clone(), g * 2.0 ** 10
        oa.step()
        sc.step(ob)
        sc.update()
        for x, y in zip(_opt_tensors(pa, oa) + [p.grad for p in pa], _opt_tensors(pb, ob) + [q.grad for q in pb]):
            assert torch.equal(x, y)
    sc.sync()
    assert sc.counters() == (2, 0) and all(ob.state[q]['step'] == 2 for q in pb)
    before = _opt_tensors(pb, ob)
    for q, g in zip(pb, _toy_grads(2)):
        q.grad = g * 2.0 ** 10
    pb[-2].grad[12345] = INF
    kept = [q.grad.clone() for q in pb]
    sc.step(ob)
    sc.update()
    sc.sync()
    for x, y in zip(before + kept, _opt_tensors(pb, ob) + [q.grad for q in pb]):
        assert torch.equal(x, y) or (torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x.nan_to_num(), y.nan_to_num()))
    assert sc.counters() == (2, 1) and sc.get_scale() == 2.0 ** 9 and all(ob.state[q]['step'] == 2 for q in pb)


# ------------------------------------------------------------------------------------------------ 3. the scale update
def test_scale_update_against_torch_grad_scaler():
    """Both scalers driven through scale / step / update on a toy optimizer whose gradients get an inf on the scripted steps:
    the same scale after every step, 6 steps taken and 3 skipped."""
    from centerclip_amd.train import AdamW, DeviceGradScaler
    script = [0, 0, 1, 0, 0, 0, 1, 1, 0]
    kw = dict(init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    ours, theirs = DeviceGradScaler(**kw), torch.amp.GradScaler('cuda', **kw)
    p = torch.nn.Parameter(torch.ones(100, device=DEV))
    q = torch.nn.Parameter(torch.ones(100, device=DEV))
    o_ours, o_theirs = AdamW([p], lr=1e-3), torch.optim.SGD([q], lr=1e-3)
    taken = 0
    for k, bad in enumerate(script):
        for par, sc, opt in ((p, ours, o_ours), (q, theirs, o_theirs)):
            opt.zero_grad()
            sc.scale((par * par).sum()).backward()
            if bad:
                par.grad[k] = INF
            sc.step(opt)
            sc.update()
        taken += 1 - bad
        ours.sync()
        assert ours.get_scale() == theirs.get_scale(), k
        assert ours.counters() == (taken, k + 1 - taken) and o_ours.state[p]['step'] == taken
        assert ours.state_dict() == theirs.state_dict()
    assert ours.counters() == (6, 3)


# ------------------------------------------------------------------------------------------------ the training loop
def _model_and_batch():
    from centerclip_amd.clip4clip import CLIP4Clip
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    B, T = int(g["cfg"][10]), int(g["cfg"][11])
    cfg = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                    cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                    minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                    sim_header='meanP', linear_patch='2d')
    video = torch.from_numpy(g["video"]).view(B, 1, T, 3, 64, 64)
    ids = torch.from_numpy(g["t_ids"])[:B]
    batch = (ids, (ids > 0).long(), torch.zeros_like(ids), video, torch.ones(B, 1, T, dtype=torch.long))
    return (lambda: CLIP4Clip.from_state_dict(dict(sd), cfg).float().to(DEV)), batch


def _args(opt_name):
    return Namespace(optim=opt_name, lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0 if opt_name == "AdamW" else None)


def _build(opt_name, capturable):
    """AdamW + lr_scheduler('cos') + clip 1.0, or BertAdam (its own per-tensor clipping and schedule)."""
    from centerclip_amd.train import AdamW, BertAdam, lr_scheduler, prep_optim_params_groups
    make, batch = _model_and_batch()
    args, m = _args(opt_name), make()
    if opt_name == "AdamW":
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd,
                  capturable=capturable)
        return m, o, lr_scheduler('cos', init_lr=args.lr, all_iters=10, slow_start_iters=1, weight_decay=args.wd), args, batch
    o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                 e=1e-6, max_grad_norm=1.0, capturable=capturable)
    return m, o, None, args, batch


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _moments(m, o):
    """{parameter name: (step, first moment, second moment)} for EVERY trainable parameter."""
    out = {}
    for n, p in m.named_parameters():
        if p.requires_grad:
            st = o.state.get(p, {})
            if len(st) == 0:                     # (a parameter no loss reaches: never stepped, on any path)
                out[n] = (0, torch.zeros(0), torch.zeros(0))
                continue
            tens = [st[k].clone() for k in sorted(st) if k != 'step']
            assert len(tens) == 2, n
            out[n] = (int(st['step']), tens[0], tens[1])
    stepped = sum(1 for st in o.state.values() if len(st))
    assert stepped > 0 and sum(1 for v in out.values() if v[1].numel()) == stepped        # (every tensor the optimizer holds)
    return out


def _same(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    for n in a:
        if torch.is_tensor(a[n]):
            assert torch.equal(a[n], b[n]), n
        else:
            assert a[n][0] == b[n][0] and torch.equal(a[n][1], b[n][1]) and torch.equal(a[n][2], b[n][2]), n


# ------------------------------------------------------------------------------------------------ 4. captured, scaler or none
@pytest.mark.parametrize("opt_name", ["AdamW", "BertAdam"])
def test_captured_step_with_scaler_equals_captured_step_without(opt_name):
    """Four captured steps under DeviceGradScaler(2^10) against four without a scaler: every parameter, both moments and the
    step counts bit for bit (a power of two passes through the backward exactly), and no step was skipped."""
    from centerclip_amd.train import DeviceGradScaler, GraphedTrainStep
    runs = []
    for scaler in (None, DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000)):
        m, o, sched, args, batch = _build(opt_name, True)
        stepper = GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=args.clip_grad_norm, scaler=scaler)
        for _ in range(4):
            loss = stepper(batch)
        stepper.sync()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and stepper.global_step == 4
        runs.append((_params(m), _moments(m, o)))
        if scaler is not None:
            assert scaler.counters() == (4, 0) and scaler.get_scale() == 2.0 ** 10
            assert scaler.state_dict()["_growth_tracker"] == 4
    assert all(v[0] == 4 for v in runs[0][1].values() if v[1].numel())
    _same(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])
    init = _params(_model_and_batch()[0]())
    assert max(float((runs[0][0][n] - init[n]).abs().max()) for n in init) > 0            # (the steps did move the parameters)


# ------------------------------------------------------------------------------------------------ 5. skips, deterministically
# call -> the scale forced before it (update(new_scale=...)); growth_interval = 2
FORCED = {3: INF, 4: 2.0 ** 10}
SCALES_AFTER = [2.0 ** 10, 2.0 ** 11, INF, 2.0 ** 10, 2.0 ** 11]
STEPS_AFTER = [1, 2, 2, 3, 4]


@functools.lru_cache(maxsize=None)
def _script(opt_name, kind):
    """The five-call script on one of three paths -> what each call left behind (clones) + the live objects.
    kind: 'captured' (GraphedTrainStep + DeviceGradScaler), 'eager' (train_epoch + DeviceGradScaler), 'torch' (train_epoch +
    torch.amp.GradScaler: the independent yardstick)."""
    from centerclip_amd.train import DeviceGradScaler, GraphedTrainStep, train_epoch
    kw = dict(init_scale=2.0 ** 10, growth_interval=2)
    m, o, sched, args, batch = _build(opt_name, kind == "captured")
    sc = torch.amp.GradScaler('cuda', **kw) if kind == "torch" else DeviceGradScaler(**kw)
    stepper = GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=args.clip_grad_norm, scaler=sc) if kind == "captured" else None
    params, scales, steps, counters, gs = [], [], [], [], 0
    for call in range(1, 6):
        if call in FORCED:
            sc.update(new_scale=FORCED[call])
        if stepper is not None:
            stepper(batch)
            stepper.sync()
            gs = stepper.global_step
        else:
            _, gs = train_epoch(0, args, m, [batch], DEV, o, gs, scheduler=sched, scaler=sc)
        torch.cuda.synchronize()
        params.append(_params(m))
        scales.append(sc.get_scale())
        steps.append(sorted({int(st['step']) for st in o.state.values() if len(st)}))
        counters.append(sc.counters() if kind != "torch" else None)
    return dict(params=params, scales=scales, steps=steps, counters=counters, global_step=gs, moments=_moments(m, o),
                live=(m, o, sched, args, batch, sc))


@pytest.mark.parametrize("opt_name", ["AdamW", "BertAdam"])
def test_scripted_skip_captured_against_eager_and_against_torch(opt_name):
    cap, eag, ref = (_script(opt_name, k) for k in ("captured", "eager", "torch"))
    for run in (cap, eag, ref):
        assert run["scales"] == SCALES_AFTER and run["steps"] == [[k] for k in STEPS_AFTER] and run["global_step"] == 5
    for run in (cap, eag):
        assert run["counters"] == [(1, 0), (2, 0), (2, 1), (3, 1), (4, 1)]
    # captured == eager with the same scaler, bit for bit: every parameter after every call, moments and counts at the end
    for a, b in zip(cap["params"], eag["params"]):
        _same(a, b)
    _same(cap["moments"], eag["moments"])
    # the skipped call changed nothing
    _same(cap["params"][2], cap["params"][1])
    assert max(float((cap["params"][3][n] - cap["params"][2][n]).abs().max()) for n in cap["params"][2]) > 0
    # against torch's scaler (its eager path clips with torch's norm over model.parameters(): last bits may differ) - the bound
    # test_train_epoch_with_grad_scaler (tests/test_r6_gpu.py) asserts for its scaler comparison: 2e-3 of each tensor's largest entry
    p0, p1 = ref["params"][-1], cap["params"][-1]
    assert p0.keys() == p1.keys()
    worst = max(float((p1[n] - p0[n]).abs().max() / p0[n].abs().max().clamp_min(1e-6)) for n in p0)
    print(f"[script {opt_name}] worst relative parameter difference against torch.amp.GradScaler after 5 calls: {worst:.2e}")
    assert worst <= 2e-3
    _same(ref["params"][2], ref["params"][1])


# ------------------------------------------------------------------------------------------------ 6. checkpoint round trip
def test_checkpoint_round_trip():
    """After the script: the scaler's state_dict loads into a torch.amp.GradScaler (and back: the same dict), and a fresh
    DeviceGradScaler loaded from it continues exactly as the original does - one more step, every parameter bit for bit."""
    import copy
    from centerclip_amd.train import DeviceGradScaler, train_epoch
    run = _script("AdamW", "eager")
    m, o, sched, args, batch, sc = run["live"]
    sd = sc.state_dict()
    assert sd["scale"] == 2.0 ** 11 and sd["_growth_tracker"] == 0 and sd["growth_interval"] == 2
    theirs = torch.amp.GradScaler('cuda')
    theirs.load_state_dict(sd)
    assert theirs.state_dict() == sd and theirs.get_scale() == 2.0 ** 11
    m2, o2, sched2, _, _ = _build("AdamW", False)
    m2.load_state_dict(copy.deepcopy(m.state_dict()))
    o2.load_state_dict(copy.deepcopy(o.state_dict()))
    fresh = DeviceGradScaler()
    fresh.load_state_dict(theirs.state_dict())
    _, g1 = train_epoch(0, args, m, [batch], DEV, o, run["global_step"], scheduler=sched, scaler=sc)
    _, g2 = train_epoch(0, args, m2, [batch], DEV, o2, run["global_step"], scheduler=sched2, scaler=fresh)
    torch.cuda.synchronize()
    assert g1 == g2 == 6 and fresh.get_scale() == sc.get_scale() == 2.0 ** 11
    assert fresh.state_dict() == sc.state_dict() and fresh.state_dict()["_growth_tracker"] == 1
    _same(_params(m), _params(m2))
    assert max(float((_params(m)[n] - run["params"][-1][n]).abs().max()) for n in run["params"][-1]) > 0
