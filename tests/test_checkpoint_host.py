"""Checkpoints on the host (train.checkpoint, _Optimizer.load_state_dict): CPU tensors, no library call, no GPU.  The file's
keys and that torch.load(weights_only=True) reads it, the best copy, a dictionary built the way the reference's main.py
builds it, load_from_pretrained, the in-place rule on existing optimizer state, refusals that leave everything as it was,
a missing path, and the exchange of optimizer state with torch.optim.AdamW in both directions.  All comparisons are exact."""
import copy
import os
from argparse import Namespace

import pytest
import torch

KEYS = ['epoch', 'global_step', 'arch', 'state_dict', 'best_acc1', 'optimizer']          # main.py:263-270; + 'scaler' (:271)


def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))


def _ours(net, **kw):
    from centerclip_amd.train import AdamW
    ps = list(net.parameters())
    return AdamW([{'params': ps[0::2], 'weight_decay': 0.2}, {'params': ps[1::2], 'weight_decay': 0.0}], lr=1e-2,
                 betas=(0.9, 0.98), eps=1e-6, **kw)


def _seed_state(opt, value, step=3, skip=()):
    """Moment tensors of a known value for every parameter (what a step would have created) except those in skip."""
    for p in (p for g in opt.param_groups for p in g['params']):
        if not any(p is q for q in skip):
            opt.state[p] = {'step': step, 'exp_avg': torch.full_like(p, value), 'exp_avg_sq': torch.full_like(p, 2 * value)}


def _torch_trained(net, steps=2):
    """torch.optim.AdamW after `steps` CPU steps: a tensor-valued 'step'."""
    ps = list(net.parameters())
    opt = torch.optim.AdamW([{'params': ps[0::2], 'weight_decay': 0.2}, {'params': ps[1::2], 'weight_decay': 0.0}], lr=1e-2,
                            betas=(0.9, 0.98), eps=1e-6)
    gen = torch.Generator().manual_seed(1)
    for _ in range(steps):
        opt.zero_grad()
        net(torch.randn(4, 5, generator=gen)).square().sum().backward()
        opt.step()
    return opt


def _frozen(net, opt):
    """Clones of every parameter, every state tensor (with its address) and every step count."""
    out = [p.detach().clone() for p in net.parameters()]
    for p in net.parameters():
        st = opt.state.get(p, {})
        out += [(k, st[k].data_ptr(), st[k].clone()) if torch.is_tensor(st[k]) else (k, st[k]) for k in sorted(st)]
    return out


def _assert_frozen(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if torch.is_tensor(x):
            assert torch.equal(x, y)
        else:
            assert x[:2] == y[:2] and (len(x) == 2 or torch.equal(x[2], y[2]))


def test_keys_and_weights_only_readability(tmp_path):
    from centerclip_amd.train import DeviceGradScaler, checkpoint_dict, save_checkpoint
    net = _net()
    opt = _ours(net)
    _seed_state(opt, 0.25)
    d = checkpoint_dict(net, opt, 3, 17, best_acc1=41.5)
    assert list(d) == KEYS and d['arch'] == 'CLIp4Clip' and (d['epoch'], d['global_step'], d['best_acc1']) == (3, 17, 41.5)
    assert 'scaler' not in checkpoint_dict(net, opt, 3, 17, scaler=DeviceGradScaler(enabled=False))
    d = checkpoint_dict(net, opt, 3, 17, best_acc1=41.5, scaler=DeviceGradScaler(init_scale=2.0 ** 9, growth_interval=7))
    assert list(d) == KEYS + ['scaler'] and d['scaler']['scale'] == 2.0 ** 9 and d['scaler']['growth_interval'] == 7
    # detached clones: a later write to the model or the moments does not reach the dictionary
    w = net[0].weight.detach().clone()
    with torch.no_grad():
        net[0].weight.add_(1.0)
    opt.state[net[0].weight]['exp_avg'].add_(1.0)
    assert torch.equal(d['state_dict']['0.weight'], w) and not d['state_dict']['0.weight'].requires_grad
    assert torch.equal(d['optimizer']['state'][0]['exp_avg'], torch.full_like(w, 0.25))
    save_checkpoint(d, False, str(tmp_path))
    back = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth.tar'), weights_only=True)
    assert list(back) == list(d) and back['scaler'] == d['scaler'] and back['optimizer']['param_groups'] == d['optimizer']['param_groups']
    assert all(torch.equal(back['state_dict'][k], d['state_dict'][k]) for k in d['state_dict'])
    assert back['optimizer']['state'][0]['step'] == 3 and torch.equal(back['optimizer']['state'][0]['exp_avg_sq'], torch.full_like(w, 0.5))


def test_is_best_copy_and_save_model(tmp_path):
    from centerclip_amd.train import checkpoint_dict, save_checkpoint, save_model
    net = _net()
    d = checkpoint_dict(net, _ours(net), 1, 2)
    save_checkpoint(d, False, str(tmp_path), filename='ckpt.pth.tar')
    assert sorted(os.listdir(str(tmp_path))) == ['ckpt.pth.tar']
    save_checkpoint(d, True, str(tmp_path), filename='ckpt.pth.tar')
    assert sorted(os.listdir(str(tmp_path))) == ['ckpt.best.pth.tar', 'ckpt.pth.tar']
    with open(os.path.join(str(tmp_path), 'ckpt.pth.tar'), 'rb') as a, open(os.path.join(str(tmp_path), 'ckpt.best.pth.tar'), 'rb') as b:
        assert a.read() == b.read()
    path = save_model(4, Namespace(output_dir=str(tmp_path)), torch.nn.DataParallel(net), type_name="best")
    assert os.path.basename(path) == 'pytorch_model.bin.best.4'
    assert os.path.basename(save_model(5, Namespace(output_dir=str(tmp_path)), net)) == 'pytorch_model.bin.5'
    sd = torch.load(path, weights_only=True)
    assert sd.keys() == net.state_dict().keys() and all(torch.equal(sd[k], v) for k, v in net.state_dict().items())


def _foreign(tmp_path):
    """A checkpoint built the way main.py:263-271 builds it, from a DataParallel-wrapped model, torch.optim.AdamW and a
    torch.amp.GradScaler-format scaler dictionary -> (path, the model that wrote it, its optimizer)."""
    src = _net(seed=3)
    opt = _torch_trained(src)
    scaler_sd = {"scale": 2.0 ** 12, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 50, "_growth_tracker": 7}
    ckpt = {'epoch': 2, 'global_step': 9, 'arch': 'CLIp4Clip', 'state_dict': torch.nn.DataParallel(src).state_dict(),
            'best_acc1': 33.25, 'optimizer': opt.state_dict(), 'scaler': scaler_sd}
    assert all(k.startswith('module.') for k in ckpt['state_dict'])
    assert all(torch.is_tensor(st['step']) for st in ckpt['optimizer']['state'].values())
    path = os.path.join(str(tmp_path), 'foreign.pth.tar')
    torch.save(ckpt, path)
    return path, src, opt


def test_resume_a_foreign_checkpoint(tmp_path):
    from centerclip_amd.train import DeviceGradScaler, resume
    path, src, src_opt = _foreign(tmp_path)
    net = _net(seed=0)
    opt, sc = _ours(net), DeviceGradScaler()
    versions = [p._version for p in net.parameters()]
    assert resume(path, net, opt, sc) == (2, 9, 33.25)
    for p, q, v in zip(net.parameters(), src.parameters(), versions):
        assert torch.equal(p, q) and p._version > v and p.requires_grad        # (copy_, not .data: the cached copies refresh)
        st, ref = opt.state[p], src_opt.state[q]
        assert type(st['step']) is int and st['step'] == 2
        assert torch.equal(st['exp_avg'], ref['exp_avg']) and torch.equal(st['exp_avg_sq'], ref['exp_avg_sq'])
    assert [g['weight_decay'] for g in opt.param_groups] == [0.2, 0.0] and opt._last == []
    assert sc.state_dict() == {"scale": 2.0 ** 12, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 50,
                               "_growth_tracker": 7}
    theirs = torch.amp.GradScaler('cpu')                    # the same file into torch's own objects, as main.py:204-207 does
    assert resume(path, _net(seed=0), None, theirs)[:2] == (2, 9) and theirs.get_growth_interval() == 50


def test_load_from_pretrained_takes_the_weights_alone(tmp_path):
    from centerclip_amd.train import DeviceGradScaler, resume
    path, src, _ = _foreign(tmp_path)
    net = _net(seed=0)
    opt, sc = _ours(net), DeviceGradScaler(init_scale=4.0)
    _seed_state(opt, 0.5)
    objs = [opt.state[p]['exp_avg'] for p in net.parameters()]
    before = _frozen(net, opt)[len(list(net.parameters())):]
    assert resume(path, net, opt, sc, load_from_pretrained=True) == (0, 0, 0.0)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), src.parameters()))
    assert all(opt.state[p]['exp_avg'] is o for p, o in zip(net.parameters(), objs))
    _assert_frozen(before, _frozen(net, opt)[len(objs):])
    assert sc.get_scale() == 4.0


def test_optimizer_restore_is_in_place_where_state_exists():
    src = _net(seed=3)
    file_sd = copy.deepcopy(_torch_trained(src).state_dict())
    net = _net(seed=0)
    opt = _ours(net)
    bare = net[1].bias                                       # this parameter has no state yet
    _seed_state(opt, 0.5, skip=[bare])
    opt._last = [net[0].weight]
    ptrs = {p: (opt.state[p]['exp_avg'].data_ptr(), opt.state[p]['exp_avg_sq'].data_ptr()) for p in net.parameters() if p is not bare}
    opt.load_state_dict(file_sd)
    order = [p for g in opt.param_groups for p in g['params']]
    for i, p in enumerate(order):
        st, want = opt.state[p], file_sd['state'][i]
        assert type(st['step']) is int and st['step'] == 2
        assert torch.equal(st['exp_avg'], want['exp_avg']) and torch.equal(st['exp_avg_sq'], want['exp_avg_sq'])
        if p is not bare:
            assert (st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()) == ptrs[p]
    assert opt._last == []
    assert opt.param_groups[0]['lr'] == 1e-2 and opt.param_groups[0]['betas'] == (0.9, 0.98)


def test_bertadam_restore_is_in_place_too():
    from centerclip_amd.train import BertAdam
    net = _net()
    mk = lambda: BertAdam(list(net.parameters()), lr=1e-2, warmup=0.1, t_total=20, b1=0.9, b2=0.98)
    a, b = mk(), mk()
    for i, p in enumerate(net.parameters()):
        a.state[p] = {'step': 5, 'next_m': torch.full_like(p, 1.0 + i), 'next_v': torch.full_like(p, 2.0 + i)}
        b.state[p] = {'step': 1, 'next_m': torch.zeros_like(p), 'next_v': torch.zeros_like(p)}
    ptrs = [(b.state[p]['next_m'].data_ptr(), b.state[p]['next_v'].data_ptr()) for p in net.parameters()]
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for i, (p, pt) in enumerate(zip(net.parameters(), ptrs)):
        st = b.state[p]
        assert st['step'] == 5 and (st['next_m'].data_ptr(), st['next_v'].data_ptr()) == pt
        assert torch.equal(st['next_m'], torch.full_like(p, 1.0 + i)) and torch.equal(st['next_v'], torch.full_like(p, 2.0 + i))


def _bad_checkpoints(tmp_path):
    path, _, _ = _foreign(tmp_path)
    good = torch.load(path, weights_only=True)
    shape = copy.deepcopy(good)
    shape['state_dict']['module.0.weight'] = torch.zeros(3, 6)
    missing = copy.deepcopy(good)
    del missing['state_dict']['module.1.bias']
    moment = copy.deepcopy(good)
    moment['optimizer']['state'][1]['exp_avg_sq'] = torch.zeros(7)
    groups = copy.deepcopy(good)
    groups['optimizer']['param_groups'][0]['params'] = [0]
    return {"parameter shape": shape, "missing key": missing, "moment shape": moment, "group structure": groups}


@pytest.mark.parametrize("what", ["parameter shape", "missing key", "moment shape", "group structure"])
def test_refusals_leave_everything_untouched(tmp_path, what):
    from centerclip_amd.train import DeviceGradScaler, resume
    path = os.path.join(str(tmp_path), 'bad.pth.tar')
    torch.save(_bad_checkpoints(tmp_path)[what], path)
    net = _net(seed=0)
    opt, sc = _ours(net), DeviceGradScaler(init_scale=4.0)
    _seed_state(opt, 0.5)
    before, groups = _frozen(net, opt), copy.deepcopy(opt.state_dict()['param_groups'])
    with pytest.raises((ValueError, RuntimeError)):
        resume(path, net, opt, sc)
    _assert_frozen(before, _frozen(net, opt))
    assert opt.state_dict()['param_groups'] == groups and sc.get_scale() == 4.0 and sc.get_growth_interval() == 2000


def test_a_captured_step_refuses_another_value_for_a_frozen_parameter():
    """What GraphedTrainStep.load_state_dict asks of the restore once a graph holds the model's addresses: a frozen parameter
    is not written (its packed copy stays valid) and must already hold the checkpoint's value."""
    from centerclip_amd.train import checkpoint_dict
    from centerclip_amd.train.checkpoint import restore
    src = _net(seed=0)
    d = checkpoint_dict(src, _ours(src), 1, 4)
    net = _net(seed=0)
    net[0].weight.requires_grad_(False)
    with torch.no_grad():
        net[1].weight.zero_()
    v = net[0].weight._version
    assert restore(d, net, captured=True) == (1, 4, 0.0)
    assert net[0].weight._version == v and torch.equal(net[1].weight, src[1].weight)
    with torch.no_grad():
        net[0].weight.add_(1.0)
        net[1].weight.zero_()
    with pytest.raises(ValueError):
        restore(d, net, captured=True)
    assert not net[1].weight.any()


def test_missing_path_raises(tmp_path):
    from centerclip_amd.train import resume
    net = _net()
    with pytest.raises(FileNotFoundError):
        resume(os.path.join(str(tmp_path), 'nothing.pth.tar'), net, _ours(net))


def test_round_trip_to_torch_adamw(tmp_path):
    """ours.state_dict() -> (through a file) -> torch.optim.AdamW.load_state_dict, and that optimizer's state_dict back."""
    from centerclip_amd.train import checkpoint_dict, save_checkpoint
    net = _net()
    ours = _ours(net)
    _seed_state(ours, 0.125, step=4)
    save_checkpoint(checkpoint_dict(net, ours, 1, 4), False, str(tmp_path))
    sd = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth.tar'), weights_only=True)['optimizer']
    ps = list(net.parameters())
    theirs = torch.optim.AdamW([{'params': ps[0::2]}, {'params': ps[1::2]}])
    theirs.load_state_dict(sd)
    for p in ps:
        assert float(theirs.state[p]['step']) == 4 and torch.equal(theirs.state[p]['exp_avg'], torch.full_like(p, 0.125))
    assert theirs.param_groups[0]['weight_decay'] == 0.2 and tuple(theirs.param_groups[0]['betas']) == (0.9, 0.98)
    back = _ours(net)
    back.load_state_dict(theirs.state_dict())
    for p in ps:
        assert back.state[p]['step'] == 4 and type(back.state[p]['step']) is int
        assert torch.equal(back.state[p]['exp_avg_sq'], torch.full_like(p, 0.25))


def test_state_a_captured_step_holds_is_restored_in_place_or_not_at_all():
    """AdamW._cap is what a capture leaves behind (the parameters the graph updates): a state dict without state for one of
    them, or with different counts for parameters the graph counts together, raises and changes nothing."""
    net = _net()
    opt = _ours(net)
    _seed_state(opt, 0.5)
    ps = [p for g in opt.param_groups for p in g['params']]
    opt._cap = dict(classes=[(0, ps[0]), (1, ps[2])], params=ps)
    good = copy.deepcopy(opt.state_dict())
    for st in good['state'].values():
        st['step'], st['exp_avg'] = 9, st['exp_avg'] + 1.0
    lacking = copy.deepcopy(good)
    del lacking['state'][1]
    uneven = copy.deepcopy(good)
    uneven['state'][1]['step'] = 8
    before = _frozen(net, opt)
    for bad in (lacking, uneven):
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
        _assert_frozen(before, _frozen(net, opt))
    opt.load_state_dict(good)
    after = _frozen(net, opt)
    assert [x[:2] for x in after if not torch.is_tensor(x) and x[0] != 'step'] == \
        [x[:2] for x in before if not torch.is_tensor(x) and x[0] != 'step']                  # the same addresses
    assert all(opt.state[p]['step'] == 9 and torch.equal(opt.state[p]['exp_avg'], torch.full_like(p, 1.5)) for p in ps)
