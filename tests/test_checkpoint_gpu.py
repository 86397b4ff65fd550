"""Save and resume a training run (train.checkpoint, GraphedTrainStep.state_dict / load_state_dict) on the tiny model of
tests/golden/clip_golden.npz; needs a real MI355X (``-m gpu``).  An interrupted run - saved after two steps, restored into
new objects or into the same captured step, continued for two steps - against the uninterrupted run of four steps: every
parameter, both moments, every step count, the groups' lr, the scaler's state and global_step.  Every comparison is exact:
the project already relies on independently built runs agreeing bit for bit, and the control case here says so first."""
import copy
import functools
import gc
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")
OPTS = ["AdamW", "BertAdam"]
AMP = dict(init_scale=2.0 ** 10, growth_interval=2)        # a growth falls on each side of the checkpoint (calls 2 and 4)
SKIP = {2: INF, 3: 2.0 ** 10}                              # call -> the scale forced before it: call 2, the last before the save, is skipped


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The cached runs (models, optimizers, captured graphs) end with this module, and so do the dead cycles its tests left:
    a hipGraph may not be destroyed by a collection that falls into a later test's capture."""
    yield
    _captured_run.cache_clear()
    _eager_run.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ builders
def _model_and_batches():
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
    first = (ids, (ids > 0).long(), torch.zeros_like(ids), video, torch.ones(B, 1, T, dtype=torch.long))
    ids2 = ids.roll(1, 0)                                    # the second batch: every caption against its neighbour's clip
    second = (ids2, (ids2 > 0).long(), torch.zeros_like(ids2), video, torch.ones(B, 1, T, dtype=torch.long))
    return (lambda: CLIP4Clip.from_state_dict(dict(sd), cfg).float().to(DEV)), [first, second]


def _args(opt_name):
    return Namespace(optim=opt_name, lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0 if opt_name == "AdamW" else None)


def _build(opt_name, capturable):
    """AdamW + lr_scheduler('cos') + clip 1.0, or BertAdam (its own per-tensor clipping and schedule) -> new objects."""
    from centerclip_amd.train import AdamW, BertAdam, lr_scheduler, prep_optim_params_groups
    make, batches = _model_and_batches()
    args, m = _args(opt_name), make()
    if opt_name == "AdamW":
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd,
                  capturable=capturable)
        return m, o, lr_scheduler('cos', init_lr=args.lr, all_iters=10, slow_start_iters=1, weight_decay=args.wd), args, batches
    o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                 e=1e-6, max_grad_norm=1.0, capturable=capturable)
    return m, o, None, args, batches


def _stepper(opt_name, scaler_kw=None):
    from centerclip_amd.train import DeviceGradScaler, GraphedTrainStep
    m, o, sched, args, batches = _build(opt_name, True)
    sc = DeviceGradScaler(**scaler_kw) if scaler_kw else None
    return GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=args.clip_grad_norm, scaler=sc), batches


def _calls(stepper, batches, first, last, forced=None):
    """Calls first..last (counted from 1) of the run: call k trains on batch (k - 1) % 2."""
    for k in range(first, last + 1):
        if forced and k in forced:
            stepper.scaler.update(new_scale=forced[k])
        loss = stepper(batches[(k - 1) % 2])
    stepper.sync()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))


# ------------------------------------------------------------------------------------------------ what is compared
def _state(m, o, global_step, scaler=None):
    """Clones of everything a resumed run must reproduce."""
    moments, stepped = {}, 0
    for n, p in m.named_parameters():
        st = o.state.get(p, {})
        if len(st):
            stepped += 1
            assert type(st['step']) is int, n
            moments[n] = (st['step'],) + tuple(st[k].clone() for k in sorted(st) if torch.is_tensor(st[k]))
            assert len(moments[n]) == 3, n
    assert stepped > 0
    out = dict(params={n: p.detach().clone() for n, p in m.named_parameters()}, moments=moments,
               lr=[g['lr'] for g in o.param_groups], wd=[g['weight_decay'] for g in o.param_groups], global_step=global_step)
    if scaler is not None:
        out['scaler'] = (scaler.state_dict(), scaler.counters())
    return out


def _same(a, b, what):
    assert a['params'].keys() == b['params'].keys() and a['moments'].keys() == b['moments'].keys(), what
    for n in a['params']:
        assert torch.equal(a['params'][n], b['params'][n]), (what, n)
    for n, (step, m1, m2) in a['moments'].items():
        assert step == b['moments'][n][0], (what, n, step, b['moments'][n][0])
        assert torch.equal(m1, b['moments'][n][1]) and torch.equal(m2, b['moments'][n][2]), (what, n)
    assert a['lr'] == b['lr'] and a['wd'] == b['wd'], what
    assert a['global_step'] == b['global_step'], what
    assert a.get('scaler') == b.get('scaler'), (what, a.get('scaler'), b.get('scaler'))


def _addresses(m, o):
    out = [p.data_ptr() for p in m.parameters()]
    for p in m.parameters():
        out += [v.data_ptr() for k, v in sorted(o.state.get(p, {}).items()) if torch.is_tensor(v)]
    return out


# ------------------------------------------------------------------------------------------------ the uninterrupted runs
@functools.lru_cache(maxsize=None)
def _captured_run(opt_name, kind="plain"):
    """Four calls of a captured step -> the checkpoint dictionary after call 2, the state after call 4 (clones), and the
    live step.  kind: 'plain' (no scaler), 'amp' (DeviceGradScaler(AMP)), 'skip' (the same with the scales of SKIP forced)."""
    stepper, batches = _stepper(opt_name, None if kind == "plain" else AMP)
    forced = SKIP if kind == "skip" else None
    _calls(stepper, batches, 1, 2, forced)
    saved = stepper.state_dict(epoch=1, best_acc1=12.5)
    _calls(stepper, batches, 3, 4, forced)
    return dict(saved=saved, end=_state(stepper.model, stepper.optimizer, stepper.global_step, stepper.scaler), live=stepper,
                batches=batches)


@functools.lru_cache(maxsize=None)
def _eager_run(opt_name, amp=False):
    """Two epochs of train_epoch over the 2-batch list -> the checkpoint dictionary after the first, the state and the mean
    loss after the second.  amp: under DeviceGradScaler(AMP)."""
    from centerclip_amd.train import DeviceGradScaler, checkpoint_dict, train_epoch
    m, o, sched, args, batches = _build(opt_name, False)
    sc = DeviceGradScaler(**AMP) if amp else None
    _, gs = train_epoch(0, args, m, batches, DEV, o, 0, scheduler=sched, scaler=sc)
    saved = checkpoint_dict(m, o, 1, gs, best_acc1=12.5, scaler=sc)
    loss, gs = train_epoch(1, args, m, batches, DEV, o, gs, scheduler=sched, scaler=sc)
    torch.cuda.synchronize()
    return dict(saved=saved, end=_state(m, o, gs, sc), loss=loss)


def _file(tmp_path, d):
    from centerclip_amd.train import save_checkpoint
    save_checkpoint(d, False, str(tmp_path), filename='ckpt.pth.tar')
    return os.path.join(str(tmp_path), 'ckpt.pth.tar')


# ------------------------------------------------------------------------------------------------ 1. control
@pytest.mark.parametrize("opt_name", OPTS)
def test_control_two_independent_runs_agree(opt_name):
    ref = _captured_run(opt_name)
    stepper, batches = _stepper(opt_name)
    _calls(stepper, batches, 1, 4)
    _same(_state(stepper.model, stepper.optimizer, stepper.global_step), ref["end"],
          "two independently built uninterrupted runs differ: determinism, not resume, is broken")
    assert ref["end"]["global_step"] == 4 and all(v[0] == 4 for v in ref["end"]["moments"].values())


# ------------------------------------------------------------------------------------------------ 2. eager resume
@pytest.mark.parametrize("opt_name", OPTS)
def test_eager_resume(opt_name, tmp_path):
    from centerclip_amd.train import resume, train_epoch
    ref = _eager_run(opt_name)
    m, o, sched, args, batches = _build(opt_name, False)
    start, gs, best = resume(_file(tmp_path, ref["saved"]), m, o)
    assert (start, gs, best) == (1, 2, 12.5)
    loss, gs = train_epoch(start, args, m, batches, DEV, o, gs, scheduler=sched)
    torch.cuda.synchronize()
    _same(_state(m, o, gs), ref["end"], "eager resume")
    assert gs == 4 and loss == ref["loss"]


# ------------------------------------------------------------------------------------------------ 3. + 5. a fresh captured step
@pytest.mark.parametrize("kind", ["plain", "amp", "skip"])
@pytest.mark.parametrize("opt_name", OPTS)
def test_captured_resume_into_a_fresh_step(opt_name, kind, tmp_path):
    from centerclip_amd.train import resume
    ref = _captured_run(opt_name, kind)
    saved = ref["saved"]
    if kind == "skip":                                       # sync() before the save: the skipped call 2 is not counted
        assert saved["global_step"] == 2 and {st['step'] for st in saved["optimizer"]["state"].values()} == {1}
        assert saved["scaler"]["counters"] == [1, 1]
    elif kind == "amp":
        assert saved["scaler"]["scale"] == 2.0 ** 11 and saved["scaler"]["counters"] == [2, 0]
    stepper, batches = _stepper(opt_name, None if kind == "plain" else AMP)
    assert resume(_file(tmp_path, saved), stepper.model, step=stepper) == (1, 2, 12.5)
    assert stepper.global_step == 2 and stepper.graph is None
    _calls(stepper, batches, 3, 4, SKIP if kind == "skip" else None)
    _same(_state(stepper.model, stepper.optimizer, stepper.global_step, stepper.scaler), ref["end"], "captured, fresh step, " + kind)
    assert stepper.global_step == 4


# ------------------------------------------------------------------------------------------------ 4. + 5. the same captured step
@pytest.mark.parametrize("kind", ["plain", "amp", "skip"])
@pytest.mark.parametrize("opt_name", OPTS)
def test_captured_resume_into_the_same_captured_step(opt_name, kind):
    ref = _captured_run(opt_name, kind)
    stepper, graph = ref["live"], ref["live"].graph
    before = _addresses(stepper.model, stepper.optimizer)
    assert stepper.load_state_dict(copy.deepcopy(ref["saved"])) == (1, 2, 12.5)
    assert _addresses(stepper.model, stepper.optimizer) == before and stepper.graph is graph and stepper.global_step == 2
    _calls(stepper, ref["batches"], 3, 4, SKIP if kind == "skip" else None)
    assert _addresses(stepper.model, stepper.optimizer) == before and stepper.graph is graph
    _same(_state(stepper.model, stepper.optimizer, stepper.global_step, stepper.scaler), ref["end"], "captured, same step, " + kind)


def test_a_torch_grad_scaler_receives_the_restored_state():
    from centerclip_amd.train import GraphedTrainStep
    saved = _captured_run("AdamW", "amp")["saved"]
    m, o, sched, args, _ = _build("AdamW", True)
    theirs = torch.amp.GradScaler('cuda', init_scale=4.0)
    stepper = GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=args.clip_grad_norm, scaler=theirs)
    stepper.load_state_dict(copy.deepcopy(saved))
    want = {k: v for k, v in saved["scaler"].items() if k != "counters"}
    assert theirs.state_dict() == want and stepper.scaler.state_dict() == want and stepper.write_back_scaler() is theirs
    assert stepper.scaler.counters() == (2, 0)


# ------------------------------------------------------------------------------------------------ 6. cross-path
# Both paths under DeviceGradScaler(AMP): that is the configuration in which the project asserts that an eager and a captured
# step agree bit for bit (test_amp_graph_gpu.py) - both then clip with the scaler's own norm.  Without a scaler the eager loop
# clips AdamW's gradients with torch's norm over model.parameters(), whose last bits may differ from the captured clip_and_step.
@pytest.mark.parametrize("opt_name", OPTS)
def test_eager_checkpoint_into_a_captured_step(opt_name, tmp_path):
    from centerclip_amd.train import resume
    ref = _captured_run(opt_name, "amp")
    stepper, batches = _stepper(opt_name, AMP)
    assert resume(_file(tmp_path, _eager_run(opt_name, True)["saved"]), stepper.model, step=stepper) == (1, 2, 12.5)
    _calls(stepper, batches, 3, 4)
    _same(_state(stepper.model, stepper.optimizer, stepper.global_step, stepper.scaler), ref["end"],
          "eager checkpoint, captured continuation")


@pytest.mark.parametrize("opt_name", OPTS)
def test_captured_checkpoint_into_the_eager_loop(opt_name, tmp_path):
    from centerclip_amd.train import DeviceGradScaler, resume, train_epoch
    ref = _eager_run(opt_name, True)
    m, o, sched, args, batches = _build(opt_name, False)
    sc = DeviceGradScaler()
    start, gs, _ = resume(_file(tmp_path, _captured_run(opt_name, "amp")["saved"]), m, o, sc)
    loss, gs = train_epoch(start, args, m, batches, DEV, o, gs, scheduler=sched, scaler=sc)
    torch.cuda.synchronize()
    _same(_state(m, o, gs, sc), ref["end"], "captured checkpoint, eager continuation")
    assert loss == ref["loss"]


# ------------------------------------------------------------------------------------------------ 7. refusal after capture
@pytest.mark.parametrize("opt_name", OPTS)
def test_a_captured_step_refuses_a_checkpoint_without_state_for_a_parameter_it_updates(opt_name):
    ref = _captured_run(opt_name)
    stepper = ref["live"]
    bad = copy.deepcopy(ref["saved"])
    del bad["optimizer"]["state"][next(iter(bad["optimizer"]["state"]))]
    for p in bad["state_dict"].values():                     # (a write that slipped through would show)
        if p.is_floating_point():
            p.add_(1.0)
    before, gs = _state(stepper.model, stepper.optimizer, stepper.global_step), stepper.global_step
    with pytest.raises((ValueError, RuntimeError)):
        stepper.load_state_dict(bad)
    _same(_state(stepper.model, stepper.optimizer, stepper.global_step), before, "after a refused checkpoint")
    _calls(stepper, ref["batches"], gs + 1, gs + 1)
    assert stepper.global_step == gs + 1
    after = _state(stepper.model, stepper.optimizer, stepper.global_step)
    assert any(not torch.equal(after["params"][n], before["params"][n]) for n in before["params"])


# ------------------------------------------------------------------------------------------------ 8. evaluate a checkpoint
class _Loader(list):
    pass


def _evaluate(model, batches):
    """eval_epoch over the batch list -> (the similarity matrix, R@1, the metric strings)."""
    from centerclip_amd import eval as ev
    seen = {}

    class Spy(ev.HipBackend):                                # the loop's one GEMM over the cached operand planes, recorded
        @staticmethod
        def dot_operands(t_op, v_op, n_video, mult):
            seen["sim"] = ev.HipBackend.dot_operands(t_op, v_op, n_video, mult)
            return seen["sim"]
    loader = _Loader(batches)
    loader.dataset = Namespace()
    r1, _, info = ev.eval_epoch(model, loader, torch.device(DEV), args=Namespace(inference_speed_test=False), backend=Spy, in_flight=1)
    return seen["sim"].clone(), r1, list(info)


def test_evaluate_a_checkpoint(tmp_path):
    """A freshly built model that has already evaluated (its packed copies hold the initial weights) loads the file and
    evaluates as the model that wrote it: the copies refreshed."""
    from centerclip_amd.train import checkpoint_dict, resume, train_epoch
    m, o, sched, args, batches = _build("AdamW", False)
    _, gs = train_epoch(0, args, m, batches, DEV, o, 0, scheduler=sched)
    path = _file(tmp_path, checkpoint_dict(m, o, 1, gs))
    want = _evaluate(m, batches)
    fresh = _model_and_batches()[0]()
    stale = _evaluate(fresh, batches)
    assert not torch.equal(stale[0], want[0])                # (two steps at lr 1e-3 did move the similarities)
    assert resume(path, fresh, load_from_pretrained=True) == (0, 0, 0.0)
    got = _evaluate(fresh, batches)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
