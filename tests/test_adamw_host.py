"""Host side of AdamW (no GPU): lr_scheduler against the reference's utils/lr_scheduler.py, the AdamW parameter groups of
utils/optimization.py:210-222, AdamW's construction, refusals and state-dict compatibility with torch.optim.AdamW.
Fixture: tests/golden/adamw_golden.npz (tools/gen_golden_adamw.py)."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import train as cctrain

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "adamw_golden.npz"))


def _cases(g):
    return sorted(k.split("/")[1] for k in g.files if k.startswith("sched/") and k.endswith("/cfg"))


def test_lr_scheduler_reproduces_the_reference(gold):
    cases = _cases(gold)
    assert {json.loads(str(gold["sched/%s/cfg" % c]))["mode"] for c in cases} == {"cos", "poly", "HTD", "step"}
    mults = [tuple(r) for r in gold["sched_group_mults"]]
    for c in cases:
        kw = json.loads(str(gold["sched/%s/cfg" % c]))
        sched = cctrain.lr_scheduler(**kw)
        opt = Namespace(param_groups=[{'lr': 0.0, 'weight_decay': 0.0, 'lr_mult': lm, 'decay_mult': dm} for lm, dm in mults])
        want_lr, want_wd = gold["sched/%s/lr" % c], gold["sched/%s/wd" % c]
        for T in range(want_lr.shape[0]):
            sched(opt, epoch=T // 10, global_step=T)
            got_lr = [g['lr'] for g in opt.param_groups]
            got_wd = [g['weight_decay'] for g in opt.param_groups]
            assert got_lr == list(want_lr[T]), (c, T, got_lr, list(want_lr[T]))
            assert got_wd == list(want_wd[T]), (c, T)
        assert sched.now_lr == want_lr[-1][2]
    # the warm-up boundary and the end clamp are inside the fixture's range
    lr = gold["sched/cos/lr"][:, 2]
    assert lr[0] < lr[5] < lr[6] and lr[-1] == json.loads(str(gold["sched/cos/cfg"]))["end_lr"]


def test_lr_scheduler_iteration_form_and_bad_mode():
    s = cctrain.lr_scheduler('cos', init_lr=1e-3, all_iters=100, slow_start_iters=10, iters_per_epoch=20)
    a, b = Namespace(param_groups=[{'lr_mult': 1.0, 'decay_mult': 1.0}]), Namespace(param_groups=[{'lr_mult': 1.0, 'decay_mult': 1.0}])
    s(a, i=3, epoch=2)
    s(b, global_step=43)
    assert a.param_groups[0] == b.param_groups[0]
    with pytest.raises(ValueError):
        cctrain.lr_scheduler('linear')


def test_adamw_param_groups_follow_the_reference(gold):
    from centerclip_amd.clip4clip import CLIP4Clip
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
          if k.startswith("sd/")}
    T = int(g["cfg"][11])
    cfg = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                    cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                    minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                    sim_header='meanP', linear_patch='2d')
    model = CLIP4Clip.from_state_dict(sd, cfg)                       # the small CLIP4Clip of clip_golden.npz
    names = {id(p): n for n, p in model.named_parameters()}
    ga = json.loads(str(gold["groups_args"]))
    coef_lr = ga.pop("coef_lr")
    got = cctrain.prep_optim_params_groups(Namespace(**ga), model, coef_lr=coef_lr)
    want = json.loads(str(gold["groups"]))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert [names[id(p)] for p in g['params']] == w['names']
        assert {k: v for k, v in g.items() if k != 'params'} == {k: v for k, v in w.items() if k != 'names'}
    assert all(len(w['names']) for w in want)                        # every group is populated


def test_param_groups_without_optim_stay_bertadam():
    m = torch.nn.Linear(2, 2)
    args = Namespace(lr=1e-2, wd=0.2, new_added_modules=[])
    base = cctrain.prep_optim_params_groups(args, m)
    also = cctrain.prep_optim_params_groups(Namespace(optim='BertAdam', **vars(args)), m)
    for a, b in zip(base, also):
        assert {k: v for k, v in a.items() if k != 'params'} == {k: v for k, v in b.items() if k != 'params'}
        assert 'lr_mult' not in a and 'decay_mult' not in a


def test_adamw_construction_validates_like_torch():
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            torch.optim.AdamW([p], **bad)                            # (the reference's optimizer refuses the same)
        with pytest.raises(ValueError):
            cctrain.AdamW([p], **bad)
    with pytest.raises(ValueError, match="amsgrad"):
        cctrain.AdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        cctrain.AdamW([p], maximize=True)
    opt = cctrain.AdamW([{'params': [p], 'lr_mult': 0.1, 'decay_mult': 0.0}])
    d = opt.defaults
    assert (d['lr'], d['betas'], d['eps'], d['weight_decay']) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
    assert opt.param_groups[0]['lr_mult'] == 0.1 and opt.param_groups[0]['decay_mult'] == 0.0
    assert not opt.capturable and cctrain.AdamW([p], capturable=True).capturable


def test_adamw_refuses_cpu_tensors_and_skips_params_without_grad():
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = cctrain.AdamW([p, q])
    opt.step()                                                       # no gradient anywhere: nothing to do
    assert len(opt.state) == 0
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError):                                # no CPU fallback
        opt.step()
    assert q not in opt.state or len(opt.state[q]) == 0


def test_adamw_state_dict_round_trips_with_torch():
    ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    tref = torch.optim.AdamW([{'params': [ps[0]], 'weight_decay': 0.2}, {'params': [ps[1]], 'weight_decay': 0.0}], lr=1e-2,
                             betas=(0.9, 0.98), eps=1e-6)
    for p in ps:
        p.grad = torch.randn_like(p)
    tref.step()
    tref.step()
    sd = tref.state_dict()
    assert torch.is_tensor(sd['state'][0]['step'])                   # torch keeps a tensor-valued step
    ours = cctrain.AdamW([{'params': [ps[0]], 'weight_decay': 0.2}, {'params': [ps[1]], 'weight_decay': 0.0}], lr=1e-2,
                         betas=(0.9, 0.98), eps=1e-6)
    ours.load_state_dict(sd)
    for p in ps:
        st = ours.state[p]
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and st['step'] == 2
        assert torch.equal(st['exp_avg'], tref.state[p]['exp_avg']) and torch.equal(st['exp_avg_sq'], tref.state[p]['exp_avg_sq'])
    assert ours.param_groups[1]['weight_decay'] == 0.0 and ours.param_groups[0]['betas'] == (0.9, 0.98)
    # ... and back: our state dict (an int step) loads into torch.optim.AdamW, which then steps from it
    mine = ours.state_dict()
    assert set(mine['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    back = torch.optim.AdamW([{'params': [ps[0]]}, {'params': [ps[1]]}], lr=1.0)
    back.load_state_dict(mine)
    assert float(back.state[ps[0]]['step']) == 2.0 and back.param_groups[0]['lr'] == 1e-2
    back.step()
    assert float(back.state[ps[0]]['step']) == 3.0
