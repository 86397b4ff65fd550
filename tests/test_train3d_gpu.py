"""Training with linear_patch='3d' on the GPU: the 3-d patch gather (cc_patch_gather3d_f16) bit for bit against torch indexing,
the conv2 patch embedding and its weight gradient against float64 conv3d, the whole step against the reference's float64
autograd fixture (tests/golden/train3d*_golden.npz, tools/gen_golden_3d.py), the step drivers, and the refusals."""
import ctypes
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import train3d_fixture as fx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CC_OK, CC_ERR_INVALID = 0, -1                               # include/centerclip_hip.h
GUARD = 4096


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# ----------------------------------------------------------------------------- 1. the gather
def _unfold3d(x, T, p):
    """x [F, 3, R, R] -> [F * g * g, 9 * p * p] with columns (c, kt, kh, kw): windows of the clip-wise zero-padded
    [B, C, T + 2, H, W] tensor (Conv3d kernel (3, p, p), stride (1, p, p), padding (1, 0, 0)), by torch indexing alone."""
    F, C, R, _ = x.shape
    g = R // p
    v = torch.nn.functional.pad(x.view(F // T, T, C, R, R).permute(0, 2, 1, 3, 4), (0, 0, 0, 0, 1, 1))
    u = v.unfold(2, 3, 1).unfold(3, p, p).unfold(4, p, p)                       # [B, C, T, g, g, kt, kh, kw]
    return u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(F * g * g, C * 3 * p * p)


def _gather_raw(frames, F, T, res, p, fill=-7.0, data_offset=0):
    """cc_patch_gather3d_f16 through ctypes into a buffer with a guard region -> (status, matrix, guard)."""
    from centerclip_amd import _lib as L
    from centerclip_amd.clip import frames_descriptor
    g = res // p if p > 0 else 0
    n = F * g * g * 9 * p * p
    out = torch.full((n + GUARD,), fill, dtype=torch.float16, device=DEV)
    fr, keep = frames_descriptor(frames)
    fr.data = keep.data_ptr() + data_offset
    rc = L.lib().cc_patch_gather3d_f16(ctypes.byref(fr), F, T, res, p, L.ptr(out), L.stream_ptr(out.device))
    torch.cuda.synchronize()
    return rc, out[:n].view(F * g * g, 9 * p * p), out[n:]


GATHER_SHAPES = [(32, 8, 6, 3), (32, 8, 2, 1), (32, 8, 4, 2), (64, 16, 3, 3), (224, 32, 6, 3)]


@pytest.mark.parametrize("res,p,F,T", GATHER_SHAPES)
def test_gather_is_the_unfold_of_the_padded_clips(res, p, F, T):
    """fp32 frames with fp16-representable values (multiples of 1/16 below 8, none of them zero): the matrix equals the torch
    indexing bit for bit, its centre-tap columns are patch_gather's matrix, taps outside the clip are exact zeros - also where the
    neighbouring frame exists but belongs to the next / previous clip - and the guard region keeps its fill."""
    gen = torch.Generator().manual_seed(res + 7 * F + T)
    x = (torch.randint(1, 128, (F, 3, res, res), generator=gen).float() / 16) * (torch.randint(0, 2, (F, 3, res, res), generator=gen) * 2 - 1)
    want = _unfold3d(x, T, p).half()
    rc, a, guard = _gather_raw(x.to(DEV), F, T, res, p)
    assert rc == CC_OK
    assert torch.equal(a.cpu(), want)
    assert bool((guard == -7.0).all())
    op = torch.ops.centerclip.patch_gather3d(x.to(DEV), T, res, p)
    assert op.dtype == torch.float16 and torch.equal(op, a)
    g, pp = res // p, p * p
    cols = a.view(F, g * g, 3, 3, pp)                                             # [f, patch, c, kt, kh * kw]
    a2d = torch.ops.centerclip.patch_gather(x.to(DEV), res, p)
    assert torch.equal(cols[:, :, :, 1].reshape(F * g * g, 3 * pp), a2d)
    for f in range(F):
        first, last = f % T == 0, f % T == T - 1
        assert bool((cols[f, :, :, 0] == 0).all()) == first and bool((cols[f, :, :, 2] == 0).all()) == last, f
        if not first:
            assert torch.equal(cols[f, :, :, 0], cols[f - 1, :, :, 1])
        if not last:
            assert torch.equal(cols[f, :, :, 2], cols[f + 1, :, :, 1])


@pytest.mark.parametrize("res,p,F,T", GATHER_SHAPES)
def test_gather_from_uint8_frames_is_the_loader_transform(res, p, F, T):
    """uint8 CHW = uint8 HWC = the float input the loader's three fp32 operations make of the same frames (computed in torch,
    rounded to fp16), bit for bit, and equal to the torch indexing of that input."""
    from oracle import clip_oracle as clo
    gen = torch.Generator().manual_seed(res + 7 * F + T + 1)
    chw = torch.randint(0, 256, (F, 3, res, res), dtype=torch.uint8, generator=gen)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    flt = clo.loader_normalize(chw, channels_last=False)
    assert torch.equal(flt, clo.loader_normalize(hwc, channels_last=True)) and flt.dtype == torch.float32
    want = _unfold3d(flt, T, p).half()
    outs = []
    for frames in (chw, hwc, flt):
        rc, a, guard = _gather_raw(frames.to(DEV), F, T, res, p)
        assert rc == CC_OK and bool((guard == -7.0).all())
        outs.append(a.cpu())
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want) and torch.equal(outs[2], want)


def test_gather_rejects_bad_arguments_and_writes_nothing():
    x = torch.ones(6, 3, 48, 48, device=DEV)
    u8 = torch.ones(6 * 3 * 48 * 48 + 8, dtype=torch.uint8, device=DEV)
    u8f = u8[:6 * 3 * 48 * 48].view(6, 3, 48, 48)
    cases = [(x, 6, 4, 48, 8, 0),            # F % T
             (x, 6, 3, 48, 12, 0),           # patch % 8
             (x, 6, 3, 44, 8, 0),            # resolution % patch
             (x, 6, 0, 48, 8, 0),            # T
             (u8f, 6, 3, 48, 8, 3),          # a uint8 base off the 8-byte grid
             (x, 6, 3, 48, 8, 4)]            # an fp32 base off the 16-byte grid
    for frames, F, T, res, p, off in cases:
        rc, a, guard = _gather_raw(frames, F, T, res, p, data_offset=off)
        assert rc == CC_ERR_INVALID, (F, T, res, p, off)
        assert bool((a == -7.0).all()) and bool((guard == -7.0).all())
    rc, a, _ = _gather_raw(u8f, 6, 3, 48, 8)                                       # the same frames, aligned: accepted
    assert rc == CC_OK and not bool((a == -7.0).any())


# ----------------------------------------------------------------------------- 2. the patch embedding
@pytest.mark.parametrize("W,res,p,F,T", [(64, 32, 8, 6, 3), (768, 224, 32, 6, 3)])
def test_patch_embedding_and_weight_gradient_against_float64_conv3d(W, res, p, F, T):
    """LinearFunction on the gathered matrix against torch.nn.functional.conv3d in float64 on the CPU, same (fp16-representable)
    frames and weights: the forward and conv2.weight's gradient for a random upstream gradient within 2e-3 of the tensor's
    largest entry (the bound tests/test_backward_gpu.py asserts for a Linear).  W = 768 / p = 32: the 9,216-column weight
    gradient on wgrad_tn_kernel (72 column tiles), 294 rows."""
    from centerclip_amd.train import LinearFunction
    gen = torch.Generator().manual_seed(W + p)
    x = torch.randn(F, 3, res, res, generator=gen).half().float()
    w = (torch.randn(W, 3, 3, p, p, generator=gen) * (9 * p * p) ** -0.5).half().float()
    g = res // p
    dy = torch.randn(F * g * g, W, generator=gen)
    w64 = w.double().requires_grad_(True)
    y64 = torch.nn.functional.conv3d(x.double().view(F // T, T, 3, res, res).permute(0, 2, 1, 3, 4), w64, stride=(1, p, p),
                                     padding=(1, 0, 0))                            # [B, W, T, g, g]
    y64 = y64.permute(0, 2, 3, 4, 1).reshape(F * g * g, W)
    (y64 * dy.double()).sum().backward()
    wd = w.to(DEV).requires_grad_(True)
    a = torch.ops.centerclip.patch_gather3d(x.to(DEV), T, res, p)
    y = LinearFunction.apply(a, wd.view(W, -1), None)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    ey, ew = relerr(y.detach().cpu(), y64.detach()), relerr(wd.grad.cpu(), w64.grad)
    print("W %d p %d: rows %d, K %d; forward %.2e, weight gradient %.2e of the largest entry" % (W, p, F * g * g, 9 * p * p, ey, ew))
    assert y.dtype == torch.float32 and wd.grad.shape == w.shape
    assert ey < 2e-3 and ew < 2e-3


# ----------------------------------------------------------------------------- 3. the whole step
def _step(model, batch):
    ids, mask, seg, video, vmask = (t.to(DEV) for t in batch)
    model.zero_grad(set_to_none=True)
    out = model(ids, seg, mask, video, vmask)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("freeze", [None, 0])
@pytest.mark.parametrize("T", [3, 1])
def test_step_against_reference_autograd(T, freeze):
    """CLIP4Clip.forward in training mode + backward on the fixture model: loss and both towers' features <= 2e-3, every
    parameter gradient <= 1e-2 of its largest entry (the bounds of the 2-d whole-step tests), and exactly the reference's set
    of parameters has a gradient - visual.conv1.weight has none.  freeze_cip_layers(0) freezes nothing for a '3d' model (the
    reference's rule) and the step is the same.  T = 1: both temporal neighbours of every frame are padding.
    Measured on the MI355X: loss within 3e-5, features 2.8e-4 / 6.3e-4, conv2's gradient 1.4e-3, the worst gradient 1.00e-2 at
    T = 3 (visual block 1's c_proj.weight, just inside the bound) and 8.0e-3 at T = 1."""
    g = fx.load(T)
    model = fx.model(T).to(DEV).train()
    if freeze is not None:
        model.freeze_cip_layers(freeze)
        assert all(p.requires_grad for p in model.parameters())
    out = _step(model, fx.batch(g))
    E = int(g["cfg"][0])
    loss, want_loss = float(out["loss"].detach()), float(g["loss"])
    ev = relerr(out["visual_output"].detach().reshape(-1, E).cpu(), torch.from_numpy(g["vfeat"]))
    et = relerr(out["sequence_output"].detach().reshape(-1, E).cpu(), torch.from_numpy(g["tfeat"]))
    print("T %d: loss %.6f fixture %.6f, visual %.2e, text %.2e" % (T, loss, want_loss, ev, et))
    assert abs(loss - want_loss) < 2e-3 * max(1.0, abs(want_loss)) and ev < 2e-3 and et < 2e-3
    named, want = dict(model.clip.named_parameters()), fx.gradients(g)
    assert {n for n, p in named.items() if p.grad is None} == fx.no_grad_names(g) == {"visual.conv1.weight"}
    worst = (0.0, None)
    for n, w in want.items():
        e = relerr(named[n].grad.detach().cpu().reshape(w.shape), w)
        worst = max(worst, (e, n))
        assert e < 1e-2, (n, e)
    print("T %d: %d gradients, worst %.2e (%s), conv2 %.2e" % (T, len(want), worst[0], worst[1],
                                                                 relerr(named["visual.conv2.weight"].grad.cpu(), want["visual.conv2.weight"])))
    assert len(want) == len(named) - 1


@pytest.mark.parametrize("channels_last", [False, True])
def test_uint8_frames_give_the_float_runs_bits(channels_last):
    from oracle import clip_oracle as clo
    g = fx.load(3)
    ids, mask, seg, video, vmask = fx.batch(g)
    B, T, R = video.shape[0], video.shape[2], video.shape[-1]
    shape = (B * T, R, R, 3) if channels_last else (B * T, 3, R, R)
    u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    flt = clo.loader_normalize(u8, channels_last=channels_last)
    model = fx.model(3).to(DEV).train()
    out_u8 = _step(model, (ids, mask, seg, u8.view((B, 1, T) + shape[1:]), vmask))
    loss_u8 = out_u8["loss"].detach().clone()
    grads_u8 = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    out_f = _step(model, (ids, mask, seg, flt.view(B, 1, T, 3, R, R), vmask))
    assert torch.isfinite(loss_u8) and torch.equal(loss_u8, out_f["loss"].detach())
    assert torch.equal(out_u8["visual_output"], out_f["visual_output"])
    for n, p in model.named_parameters():
        assert (p.grad is None) == (grads_u8[n] is None), n
        assert p.grad is None or torch.equal(p.grad, grads_u8[n]), n
    assert sum(v is None for v in grads_u8.values()) == 1


# ----------------------------------------------------------------------------- 4. the loop
def _args(opt_name):
    return Namespace(optim=opt_name, lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0 if opt_name == "AdamW" else None)


def _build(opt_name, capturable):
    """AdamW + lr_scheduler('cos') + clip 1.0, or BertAdam (its own per-tensor clipping and schedule)."""
    from centerclip_amd.train import AdamW, BertAdam, lr_scheduler, prep_optim_params_groups
    args, m = _args(opt_name), fx.model(3).to(DEV).train()
    if opt_name == "AdamW":
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd,
                  capturable=capturable)
        return m, o, lr_scheduler('cos', init_lr=args.lr, all_iters=10, slow_start_iters=1, weight_decay=args.wd), args
    o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                 e=1e-6, max_grad_norm=1.0, capturable=capturable)
    return m, o, None, args


def _check_conv1(m, o, init):
    conv1 = m.clip.visual.conv1.weight
    assert conv1.requires_grad and conv1.grad is None
    assert torch.equal(conv1.detach(), init["clip.visual.conv1.weight"])
    assert len(o.state.get(conv1, {})) == 0
    assert any(p is conv1 for gr in o.param_groups for p in gr['params'])          # (it is in the groups, as main.py builds them)


@pytest.mark.parametrize("opt_name", ["AdamW", "BertAdam"])
def test_train_epoch_lowers_the_loss(opt_name):
    from centerclip_amd.train import train_epoch
    m, o, sched, args = _build(opt_name, False)
    init = {n: p.detach().clone() for n, p in m.named_parameters()}
    losses = []
    _, gs = train_epoch(0, args, m, [fx.batch(fx.load(3))] * 5, DEV, o, 0, scheduler=sched,
                        log=lambda ep, step, loss, sim, gstep: losses.append(loss))
    torch.cuda.synchronize()
    print(opt_name, "losses", ["%.4f" % v for v in losses])
    assert gs == 5 and len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    _check_conv1(m, o, init)
    conv2 = m.clip.visual.conv2.weight
    assert not torch.equal(conv2.detach(), init["clip.visual.conv2.weight"]) and o.state[conv2]['step'] == 5


@functools.lru_cache(maxsize=None)
def _eager_states(opt_name, amp):
    """Three eager steps on the repeated batch -> the parameters after each."""
    from centerclip_amd.train import DeviceGradScaler, clip_grad_norm_, train_epoch
    m, o, sched, args = _build(opt_name, False)
    batch = fx.batch(fx.load(3))
    states = []
    if amp:
        sc, gs = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000), 0
        for _ in range(3):
            _, gs = train_epoch(0, args, m, [batch], DEV, o, gs, scheduler=sched, scaler=sc)
            states.append({n: p.detach().clone() for n, p in m.named_parameters()})
        return states
    dev = [t.to(DEV) for t in batch]
    for k in range(3):
        o.zero_grad(set_to_none=True)
        if sched is not None:
            sched(o, global_step=k)
        m(dev[0], dev[2], dev[1], dev[3], dev[4])['loss'].mean().backward()
        if opt_name == "AdamW":
            o.clip_and_step(1.0)
        else:
            clip_grad_norm_([p for gr in o.param_groups for p in gr['params']], 1.0)
            o.step()
        with torch.no_grad():
            m.clip.logit_scale.clamp_(0.1, 4.6052)
        states.append({n: p.detach().clone() for n, p in m.named_parameters()})
    return states


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("opt_name", ["AdamW", "BertAdam"])
def test_graphed_step_equals_eager(opt_name, amp):
    """GraphedTrainStep on a model with a parameter that never gets a gradient (conv1), with and without DeviceGradScaler,
    against the eager steps of the same pieces: the same bits after each of three calls; conv1 at its initial bits and without
    optimizer state."""
    from centerclip_amd.train import DeviceGradScaler, GraphedTrainStep
    eager = _eager_states(opt_name, amp)
    m, o, sched, args = _build(opt_name, True)
    init = {n: p.detach().clone() for n, p in m.named_parameters()}
    sc = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000) if amp else None
    stepper = GraphedTrainStep(m, o, scheduler=sched, clip_grad_norm=1.0 if (opt_name == "AdamW" or not amp) else None, scaler=sc)
    batch = fx.batch(fx.load(3))
    for k in range(3):
        loss = stepper(batch)
        stepper.sync()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        for n, p in m.named_parameters():
            assert torch.equal(p.detach(), eager[k][n]), (k, n)
    assert stepper.global_step == 3 and (sc is None or sc.counters() == (3, 0))
    assert not torch.equal(m.clip.visual.conv2.weight.detach(), init["clip.visual.conv2.weight"])
    _check_conv1(m, o, init)


# ----------------------------------------------------------------------------- 5. refusals, and '2d' as it was
def test_refusals_on_the_device():
    from centerclip_amd.train import encode_image_train
    model = fx.model(3).to(DEV).train()
    video = torch.zeros(6, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="video_frame"):
        encode_image_train(model.clip, video, 4)
    ids, mask, seg, vid, vmask = fx.batch(fx.load(3))
    with pytest.raises(ValueError, match="video_frame"):                          # through CLIP4Clip.forward: 2 clips of 3, T = 3 only
        encode_image_train(model.clip, vid.view(6, 3, 32, 32)[:5].to(DEV), 3)
    shift = fx.model(3, cluster_inter=1, cluster_algo='token_shift', target_frames_blocks=[2, 2], cluster_num_blocks=[15, 14])
    with pytest.raises(NotImplementedError, match="original_frame"):
        encode_image_train(shift.to(DEV).train().clip, video, 2)


def test_2d_tower_is_bit_identical_to_the_glue_front():
    """The '2d' training tower after the '3d' path was added: its features and every gradient equal, bit for bit, those of the
    towers' torch-glue front kept under train.towers._GLUE_FRONT (the comparison tests/test_freeze_gpu.py uses) - on the fixture
    model without conv2."""
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.train import encode_image_train
    from centerclip_amd.train import towers as cctrain
    sd = {k: v for k, v in fx.state_dict().items() if k != "visual.conv2.weight"}
    g = fx.load(3)
    video = fx.batch(g)[3].view(-1, 3, 32, 32).to(DEV)
    dy = torch.randn(video.shape[0], int(g["cfg"][0]), generator=torch.Generator().manual_seed(5)).to(DEV)
    runs = []
    for glue in (False, True):
        model = CLIP4Clip.from_state_dict(dict(sd), fx.cfg(3, 2, linear_patch='2d')).float().to(DEV).train()
        cctrain._GLUE_FRONT = glue
        try:
            feats, _ = encode_image_train(model.clip, video, 3)
            feats.backward(dy)
        finally:
            cctrain._GLUE_FRONT = False
        torch.cuda.synchronize()
        runs.append((feats.detach().clone(), {n: p.grad.clone() for n, p in model.clip.visual.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1].keys() == runs[1][1].keys() and "conv1.weight" in runs[0][1]
    for n, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][n]), n
