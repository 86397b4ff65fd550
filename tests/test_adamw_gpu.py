"""AdamW and global gradient clipping on the HIP kernels of csrc/adamw.hip (need a real MI355X, ``-m gpu``): numerics against a
float64 restatement of torch.optim.AdamW, determinism and launch equivalence, clip_grad_norm_ against torch's, the fused
clip_and_step, a captured step replayed with a moving learning rate, and the training loop end to end (train_epoch,
GraphedTrainStep, the GradScaler branch) on the small CLIP4Clip of clip_golden.npz."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 3, 4, 8191, 8192, 8193, (1 << 20) + 3]


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((0.5 * torch.randn(n, generator=gen)).to(DEV)) for n in SIZES]


def _grads(step, seed=1):
    gen = torch.Generator().manual_seed(seed * 1000 + step)
    return [(torch.randn(n, generator=gen) * (0.1 if i % 2 else 3e-3)).to(DEV) for i, n in enumerate(SIZES)]


def _groups(ps):
    # two classes of weight decay, the reference's lr_mult / decay_mult keys
    return [{'params': ps[0::2], 'lr_mult': 1.0, 'decay_mult': 1.0}, {'params': ps[1::2], 'lr_mult': 0.5, 'decay_mult': 0.0}]


def _sched():
    from centerclip_amd.train import lr_scheduler
    return lr_scheduler('cos', init_lr=1e-2, all_iters=10, slow_start_iters=2, slow_start_lr=1e-3, weight_decay=0.2)


def _ref_step64(p, m, v, g, lr, wd, b1, b2, eps, t):
    """torch.optim.AdamW (decoupled weight decay, bias correction) in float64."""
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return p, m, v


def _maxerr(a, b):
    return max(float((x.double() - y).abs().max()) for x, y in zip(a, b))


def test_adamw_against_float64_and_torch():
    """Ten steps, lr moved by lr_scheduler between steps (step 1: bc1 = 0.1), wd 0.2 and 0, n from 1 to 2^20 + 3 in one
    launch: max |error| against float64 <= 2 x torch.optim.AdamW(foreach=False)'s in fp32 + 1e-9, for p, exp_avg, exp_avg_sq."""
    from centerclip_amd.train import AdamW
    b1, b2, eps = 0.9, 0.98, 1e-6
    ours_p, ref_p = _params(), _params()
    opt = AdamW(_groups(ours_p), lr=1e-2, betas=(b1, b2), eps=eps, weight_decay=0.2)
    tref = torch.optim.AdamW(_groups(ref_p), lr=1e-2, betas=(b1, b2), eps=eps, weight_decay=0.2, foreach=False)
    sched, sched_t = _sched(), _sched()
    p64 = [p.detach().double() for p in ours_p]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    lrs = []
    for k in range(10):
        sched(opt, global_step=k)
        sched_t(tref, global_step=k)
        gs = _grads(k)
        for p, q, g in zip(ours_p, ref_p, gs):
            p.grad, q.grad = g.clone(), g.clone()
        opt.step()
        tref.step()
        for i in range(len(SIZES)):
            grp = opt.param_groups[i % 2]
            p64[i], m64[i], v64[i] = _ref_step64(p64[i], m64[i], v64[i], gs[i].double(), grp['lr'], grp['weight_decay'], b1, b2,
                                                 eps, k + 1)
        lrs.append(opt.param_groups[0]['lr'])
    torch.cuda.synchronize()
    assert len(set(lrs)) == 10 and opt.param_groups[1]['weight_decay'] == 0.0
    for name, ours, theirs, want in (
            ("p", ours_p, ref_p, p64),
            ("exp_avg", [opt.state[p]['exp_avg'] for p in ours_p], [tref.state[p]['exp_avg'] for p in ref_p], m64),
            ("exp_avg_sq", [opt.state[p]['exp_avg_sq'] for p in ours_p], [tref.state[p]['exp_avg_sq'] for p in ref_p], v64)):
        e_ours, e_torch = _maxerr(ours, want), _maxerr(theirs, want)
        print(f"[adamw] {name}: max|err| vs float64 ours {e_ours:.3e} torch {e_torch:.3e}")
        assert e_ours <= 2 * e_torch + 1e-9, name
    assert all(opt.state[p]['step'] == 10 for p in ours_p)


def _run_steps(opt_params, make_opt, steps=3):
    sched = _sched()
    opts = make_opt(opt_params)
    for k in range(steps):
        gs = _grads(k, seed=7)
        for o in opts:
            sched(o, global_step=k)
        for p, g in zip(opt_params, gs):
            p.grad = g
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    return [p.detach().clone() for p in opt_params] + [o.state[p][k] for o in opts for p in o.state for k in ('exp_avg', 'exp_avg_sq')]


def test_adamw_deterministic_and_one_launch_equals_one_per_tensor():
    from centerclip_amd.train import AdamW
    multi = lambda ps: [AdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)]
    a = _run_steps(_params(), multi)
    b = _run_steps(_params(), multi)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # one optimizer (one launch) per tensor, in the same groups' hyper-parameters
    per = lambda ps: [AdamW([{'params': [p], 'lr_mult': 1.0 if i % 2 == 0 else 0.5, 'decay_mult': 1.0 if i % 2 == 0 else 0.0}],
                            lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2) for i, p in enumerate(ps)]
    ps = _params()
    c = _run_steps(ps, per)
    n = len(SIZES)
    assert all(torch.equal(x, y) for x, y in zip(a[:n], c[:n]))
    ref_opt_state = a[n:]                         # (exp_avg, exp_avg_sq) per parameter in group order: 0, 2, 4, 6, 1, 3, 5
    order = list(range(0, n, 2)) + list(range(1, n, 2))
    for j, i in enumerate(order):
        assert torch.equal(ref_opt_state[2 * j], c[n + 2 * i]) and torch.equal(ref_opt_state[2 * j + 1], c[n + 2 * i + 1])


@pytest.mark.parametrize("target", [0.3, 40.0])
def test_clip_grad_norm_against_torch(target):
    from centerclip_amd.train import clip_grad_norm_
    gs = _grads(0, seed=3)
    scale = target / float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
    gs = [g * scale for g in gs]
    ours, theirs = _params(), _params()
    for p, q, g in zip(ours, theirs, gs):
        p.grad, q.grad = g.clone(), g.clone()
    norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
    n_ours = clip_grad_norm_(ours, 1.0)
    n_torch = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    torch.cuda.synchronize()
    assert n_ours.dim() == 0 and n_ours.is_cuda and n_ours.dtype == torch.float32
    assert abs(float(n_ours) - norm64) <= 1e-6 * norm64 and abs(float(n_torch) - norm64) <= 1e-5 * norm64
    for p, q, g in zip(ours, theirs, gs):
        if target < 1.0:
            assert torch.equal(p.grad, g) and torch.equal(q.grad, g)              # coefficient 1: untouched
        else:
            torch.testing.assert_close(p.grad, q.grad, rtol=2e-6, atol=0)
    if target > 1.0:
        total = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ours)))
        assert abs(total - 1.0) < 1e-5


@pytest.mark.parametrize("target", [0.3, 40.0])
def test_clip_and_step_is_clip_then_step(target):
    from centerclip_amd.train import AdamW, clip_grad_norm_

    def run(fused):
        ps = _params()
        opt = AdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
        sched, norms = _sched(), []
        for k in range(3):
            gs = _grads(k, seed=5)
            scale = target / float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
            for p, g in zip(ps, gs):
                p.grad = g * scale
            sched(opt, global_step=k)
            if fused:
                norms.append(opt.clip_and_step(1.0))
            else:
                norms.append(clip_grad_norm_([p for grp in opt.param_groups for p in grp['params']], 1.0))
                opt.step()
        torch.cuda.synchronize()
        return ps, [p.grad for p in ps], norms, opt
    pa, ga, na, oa = run(True)
    pb, gb, nb, ob = run(False)
    assert all(torch.equal(x, y) for x, y in zip(na, nb))
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))                         # p.grad ends as clip leaves it
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(torch.equal(oa.state[x]['exp_avg_sq'], ob.state[y]['exp_avg_sq']) for x, y in zip(pa, pb))
    assert abs(float(na[0]) / target - 1) < 1e-5


@pytest.mark.parametrize("clip", [None, 1.0])
def test_captured_adamw_step_equals_eager_steps(clip):
    """AdamW(capturable=True) inside torch.cuda.graph (a host synchronisation would fail the capture), replayed with the
    scheduler moving lr between replays: the same bits as eager steps."""
    from centerclip_amd.train import AdamW
    steps = 5
    gs_all = [[g * 30.0 for g in _grads(k, seed=11)] for k in range(steps)]

    def do(opt, ps):
        return opt.clip_and_step(clip) if clip is not None else opt.step()

    pe = _params()
    oe = AdamW(_groups(pe), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
    se = _sched()
    for k in range(steps):
        se(oe, global_step=k)
        for p, g in zip(pe, gs_all[k]):
            p.grad = g.clone()
        do(oe, pe)
    pc = _params()
    oc = AdamW(_groups(pc), lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, capturable=True)
    sc = _sched()
    for p, g in zip(pc, gs_all[0]):
        p.grad = g.clone()                                               # static gradient buffers of the graph
    sc(oc, global_step=0)
    do(oc, pc)                                                           # eager step 1 (stages the records)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        do(oc, pc)
    for k in range(1, steps):
        for p, g in zip(pc, gs_all[k]):
            p.grad.copy_(g)
        sc(oc, global_step=k)
        oc.refresh_lr()
        graph.replay()
        oc.advance()
    torch.cuda.synchronize()
    assert len({oe.param_groups[0]['lr']} | {sc.lr_at(k) for k in range(steps)}) > 3
    assert all(oc.state[p]['step'] == steps for p in pc)
    for a, b in zip(pe, pc):
        assert torch.equal(a, b)
        assert torch.equal(oe.state[a]['exp_avg'], oc.state[b]['exp_avg'])
        assert torch.equal(oe.state[a]['exp_avg_sq'], oc.state[b]['exp_avg_sq'])


def test_adamw_refuses_non_master_weights():
    from centerclip_amd.train import AdamW
    p = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError):
        AdamW([p]).step()


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


ARGS = Namespace(optim='AdamW', lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"], gradient_accumulation_steps=1,
                 clip_grad_norm=1.0)


def _train_sched():
    from centerclip_amd.train import lr_scheduler
    return lr_scheduler('cos', init_lr=ARGS.lr, all_iters=10, slow_start_iters=1, weight_decay=ARGS.wd)


def test_train_epoch_with_adamw_matches_torch_adamw():
    """train_epoch (main.py:291-378) with AdamW + lr_scheduler + clip_grad_norm=1.0 over 3 steps: the gradients (after torch's
    clip, as train_epoch applies it) and the scheduled lr / weight_decay that reach each step also drive torch.optim.AdamW in
    fp32 and a float64 restatement on copies of the initial parameters - after 3 steps the HIP parameters are within
    2 x torch's max error against float64 + 1e-9.  (A second model trained by torch.optim.AdamW is no yardstick: the fp16
    operand casts of the forward turn last-bit parameter differences into different gradients.)"""
    from centerclip_amd.train import AdamW, prep_optim_params_groups, train_epoch
    make, batch = _model_and_batch()
    seen = []

    class Recorded(AdamW):
        def step(self, closure=None):
            seen.append([(g['lr'], g['weight_decay'], [p.grad.detach().clone() if p.grad is not None else None for p in g['params']])
                         for g in self.param_groups])
            return super().step(closure)
    model = make()
    init = [p.detach().clone() for p in model.parameters()]
    groups = prep_optim_params_groups(ARGS, model, coef_lr=0.5)
    opt = Recorded(groups, lr=ARGS.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=ARGS.wd)
    loss, gs = train_epoch(0, ARGS, model, [batch] * 3, DEV, opt, 0, scheduler=_train_sched())
    torch.cuda.synchronize()
    assert gs == 3 and np.isfinite(loss) and len(seen) == 3
    assert all(st['step'] == 3 for st in opt.state.values())
    index = {id(p): i for i, p in enumerate(model.parameters())}
    shadow = [torch.nn.Parameter(init[index[id(p)]].clone()) for g in groups for p in g['params']]
    tgroups, k = [], 0
    for g in groups:
        tgroups.append({'params': shadow[k:k + len(g['params'])], 'lr_mult': g['lr_mult'], 'decay_mult': g['decay_mult']})
        k += len(g['params'])
    tref = torch.optim.AdamW(tgroups, lr=ARGS.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=ARGS.wd, foreach=False)
    p64 = [p.detach().double() for p in shadow]
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    for t, rec in enumerate(seen, start=1):
        k = 0
        for tg, (lr, wd, grads) in zip(tref.param_groups, rec):
            tg['lr'], tg['weight_decay'] = lr, wd
            for q, gr in zip(tg['params'], grads):
                q.grad = gr
                p64[k], m64[k], v64[k] = _ref_step64(p64[k], m64[k], v64[k], gr.double(), lr, wd, 0.9, 0.98, 1e-6, t)
                k += 1
        tref.step()
    torch.cuda.synchronize()
    ours = [p for g in groups for p in g['params']]
    assert len(ours) == len(shadow) == len(index)
    e_ours, e_torch = _maxerr(ours, p64), _maxerr(shadow, p64)
    moved = max(float((a.double() - b).abs().max()) for a, b in zip(ours, [init[index[id(p)]].double() for p in ours]))
    print(f"[train_epoch] largest parameter move {moved:.3e}; max|err| vs float64: HIP AdamW {e_ours:.3e}, torch {e_torch:.3e}")
    assert moved > 5e-4 and e_ours <= 2 * e_torch + 1e-9
    assert seen[0][0][0] != seen[2][0][0]                                  # the scheduler moved lr between the steps


@pytest.mark.parametrize("opt_name", ["AdamW", "BertAdam"])
def test_graphed_train_step_with_scheduler_and_clipping(opt_name):
    """GraphedTrainStep(model, optimizer, scheduler=..., clip_grad_norm=1.0) against an eager loop of the same HIP pieces: the
    same parameters bit for bit after 3 calls, 3 optimizer steps counted."""
    from centerclip_amd.train import AdamW, BertAdam, GraphedTrainStep, clip_grad_norm_, prep_optim_params_groups
    make, batch = _model_and_batch()
    args = Namespace(**dict(vars(ARGS), optim=opt_name))

    def build(capturable):
        m = make()
        if opt_name == "AdamW":
            o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd,
                      capturable=capturable)
            return m, o, _train_sched()
        o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9,
                     b2=0.98, e=1e-6, max_grad_norm=1.0, capturable=capturable)
        return m, o, None
    m0, o0, s0 = build(False)
    m0.train()
    dev_batch = [t.to(DEV) for t in batch]
    for k in range(3):
        o0.zero_grad(set_to_none=True)
        if s0 is not None:
            s0(o0, global_step=k)
        out = m0(dev_batch[0], dev_batch[2], dev_batch[1], dev_batch[3], dev_batch[4])
        out['loss'].mean().backward()
        if opt_name == "AdamW":
            o0.clip_and_step(1.0)
        else:
            clip_grad_norm_([p for g in o0.param_groups for p in g['params']], 1.0)
            o0.step()
        with torch.no_grad():
            m0.clip.logit_scale.clamp_(0.1, 4.6052)
    m1, o1, s1 = build(True)
    stepper = GraphedTrainStep(m1, o1, scheduler=s1, clip_grad_norm=1.0)
    for _ in range(3):
        loss = stepper(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and stepper.global_step == 3
    assert all(st["step"] == 3 for st in o1.state.values())
    if s1 is not None:
        assert o1.param_groups[0]['lr'] == o0.param_groups[0]['lr']
    for (k, a), (_, b) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(a, b), k


def test_train_epoch_grad_scaler_skips_inf_step_with_adamw():
    """The GradScaler branch of train_epoch with AdamW: a scale that overflows the gradients skips both steps."""
    from centerclip_amd.train import AdamW, prep_optim_params_groups, train_epoch
    make, batch = _model_and_batch()
    model = make()
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = AdamW(prep_optim_params_groups(ARGS, model, coef_lr=0.5), lr=ARGS.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=ARGS.wd)
    big = torch.amp.GradScaler('cuda', init_scale=float("inf"), growth_interval=1000)
    loss, gs = train_epoch(0, ARGS, model, [batch] * 2, DEV, opt, 0, scheduler=_train_sched(), scaler=big)
    torch.cuda.synchronize()
    assert gs == 2 and np.isfinite(loss)
    assert all(torch.equal(p.detach(), init[n]) for n, p in model.named_parameters() if n != "clip.logit_scale")
    assert all(len(st) == 0 or st['step'] == 0 for st in opt.state.values())
