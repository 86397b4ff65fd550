"""The device frame transform on a real MI355X (``-m gpu``): cc_resize_crop_u8 / torch.ops.centerclip.resize_center_crop /
preprocess.FrameTransform against the NumPy restatement of Pillow's bicubic Resize + torchvision's CenterCrop
(tests/resize_ref.py) and against Pillow's own outputs (tests/golden/resize_golden.npz), then through the encoder, eval_epoch,
DeviceFeeder and train_epoch.  Every comparison is byte (bit) equality, no pixel excluded."""
import ctypes
import functools
import gc
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096

# (H, W, n_px, F): non-integer downscale with an odd crop; portrait (vertical crop, the row range is cut); upscale (5 taps);
# no crop; no resampling at all; shrink 9.4 (about 39 taps, windows clipped at the borders); one real shape
CASES = {"down": (33, 57, 32, 5), "portrait": (100, 37, 32, 5), "up": (17, 64, 32, 5), "nocrop": (50, 50, 32, 5),
         "same": (32, 57, 32, 5), "shrink": (512, 300, 32, 5), "real": (360, 640, 224, 12)}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    _reference.cache_clear()
    gc.collect()                          # (no dead cycle's hipGraph may be destroyed inside a later test's capture)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _reference(H, W, n_px, F, kind, resize=True):
    """-> (frames [F, H, W, 3] uint8, the restatement's [F, n_px, n_px, 3]); computed once, shared, never written"""
    x = R.make_input(H, W, kind, seed=H * 7 + W, frames=F)
    y = R.resize_center_crop(x, n_px, resize)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _layout(a, fmt):
    """[F, H, W, 3] -> contiguous NumPy array in the layout of the uint8 code fmt (1 = CHW, 2 = HWC)"""
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2)) if fmt == 1 else np.ascontiguousarray(a)


def _call(x_hwc, fmt, n_px, dst_fmt, resize=1, offset=0):
    """cc_resize_crop_u8 through ctypes on a source placed `offset` bytes into its buffer -> (status, dst as [F, n, n, 3] NumPy,
    whether the guard region behind dst is untouched)."""
    from centerclip_amd import _lib as L
    from centerclip_amd import torch_ops as T
    lib = L.lib()
    F, H, W = x_hwc.shape[:3]
    src = torch.from_numpy(_layout(x_hwc, fmt).reshape(-1).copy())
    buf = torch.empty(src.numel() + offset, dtype=torch.uint8, device=DEV)
    buf[offset:].copy_(src)
    assert (buf.data_ptr() + offset) % 4 == offset % 4
    n_out = F * 3 * n_px * n_px
    dst = torch.full((n_out + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    plan = T.resize_plan(H, W, n_px, resize, torch.device(DEV))
    nws = lib.cc_resize_crop_workspace_bytes(F, H, W, n_px, resize)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
    rc = lib.cc_resize_crop_u8(ctypes.c_void_p(buf.data_ptr() + offset), fmt, F, H, W, L.ptr(plan), n_px, resize, L.ptr(dst), dst_fmt,
                               L.ptr(ws), nws, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    out = dst[:n_out].cpu().numpy()
    out = out.reshape(F, 3, n_px, n_px).transpose(0, 2, 3, 1) if dst_fmt == 1 else out.reshape(F, n_px, n_px, 3)
    return rc, out, bool((dst[n_out:] == 0xA5).all())


@pytest.mark.parametrize("kind", ["noise", "checker"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_restatement_in_every_layout(case, kind):
    H, W, n_px, F = CASES[case]
    x, want = _reference(H, W, n_px, F, kind)
    for fmt in (2, 1):
        for dst_fmt in (2, 1):
            rc, got, guard_ok = _call(x, fmt, n_px, dst_fmt)
            assert rc == 0 and guard_ok, (fmt, dst_fmt, rc, guard_ok)
            assert np.array_equal(got, want), (case, kind, fmt, dst_fmt, int((got != want).sum()))


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("F", [1, 5])
def test_source_at_any_byte_address(F, offset):
    """Rows of 3 * 57 = 171 bytes from a base moved off every vector alignment; nothing is written behind dst."""
    for case in ("down", "portrait", "same"):
        H, W, n_px, _ = CASES[case]
        x, want = _reference(H, W, n_px, 5, "noise")
        for fmt in (2, 1):
            rc, got, guard_ok = _call(x[:F], fmt, n_px, fmt, offset=offset)
            assert rc == 0 and guard_ok
            assert np.array_equal(got, want[:F]), (case, F, offset, fmt)


def test_op_equals_pillow_golden_file():
    g = np.load(os.path.join(HERE, "golden", "resize_golden.npz"))
    n_px = int(g["n_px"])
    for name in sorted(R.cases()):
        x, want = torch.from_numpy(g["in/" + name]), torch.from_numpy(g["out/" + name])
        got = torch.ops.centerclip.resize_center_crop(x.to(DEV), n_px, True)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want), name
        got = torch.ops.centerclip.resize_center_crop(x.permute(0, 3, 1, 2).contiguous().to(DEV), n_px, True)
        assert torch.equal(got.cpu(), want.permute(0, 3, 1, 2)), name


def test_crop_only_is_the_slice():
    from centerclip_amd import _lib as L
    from centerclip_amd.preprocess import resize_center_crop
    x = torch.from_numpy(R.make_input(57, 64, "noise", frames=3))
    got = resize_center_crop(x.to(DEV), 32, resize=False)
    assert torch.equal(got.cpu(), x[:, 12:44, 16:48])               # top = round(12.5) = 12 (half to even), left = 16
    got = resize_center_crop(x.permute(0, 3, 1, 2).contiguous().to(DEV), 32, resize=False)
    assert torch.equal(got.cpu(), x[:, 12:44, 16:48].permute(0, 3, 1, 2))
    rc, out, guard_ok = _call(x.numpy(), 2, 32, 1, resize=0)
    assert rc == 0 and guard_ok and np.array_equal(out, x[:, 12:44, 16:48].numpy())
    with pytest.raises(L.CenterClipHipError, match="unsupported"):
        resize_center_crop(torch.zeros(2, 31, 64, 3, dtype=torch.uint8, device=DEV), 32, resize=False)


def test_python_api_forms():
    """The loaders' 6-D video in both layouts comes back 6-D; a batch at the model's resolution passes through untouched."""
    from centerclip_amd.preprocess import FrameTransform, resize_center_crop
    x, want = _reference(33, 57, 32, 5, "noise")
    v = torch.from_numpy(x[:4].copy()).view(2, 1, 2, 33, 57, 3).to(DEV)
    w = torch.from_numpy(want[:4].copy()).view(2, 1, 2, 32, 32, 3)
    t = FrameTransform(32)
    assert torch.equal(t(v).cpu(), w) and torch.equal(resize_center_crop(v, 32).cpu(), w)
    assert torch.equal(t(v.permute(0, 1, 2, 5, 3, 4).contiguous()).cpu(), w.permute(0, 1, 2, 5, 3, 4))
    ready = torch.zeros(3, 32, 32, 3, dtype=torch.uint8, device=DEV)
    assert t(ready) is ready
    out = torch.empty(2, 1, 2, 32, 32, 3, dtype=torch.uint8, device=DEV)
    assert t(v, out=out) is out and torch.equal(out.cpu(), w)
    assert list(t._plans) == [(33, 57, "cuda", 0)]


def test_captured_with_a_cached_plan_replays_on_new_frames():
    from centerclip_amd.preprocess import FrameTransform
    x, want = _reference(100, 37, 32, 5, "noise")
    x2, want2 = _reference(100, 37, 32, 5, "checker")
    t = FrameTransform(32)
    static = torch.from_numpy(x.copy()).to(DEV)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        eager = t(static).clone()                                    # (plan uploaded, workspace of this stream allocated)
    stream.synchronize()
    assert np.array_equal(eager.cpu().numpy(), want)
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        y = t(static)
    static.copy_(torch.from_numpy(x2.copy()))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), want2)
    assert torch.equal(y, t(static))
    del graph


# ------------------------------------------------------------------------------------------ through the product's loops
def _golden():
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    return g, sd, int(g["cfg"][10]), int(g["cfg"][11]), int(g["video"].shape[-1])


def _cfg(T):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                     sim_header='meanP', linear_patch='2d')


RAW = (80, 100)           # decoded frames of the loop tests: 80 x 100 -> 64 x 80 -> the tiny model's 64 x 64


@functools.lru_cache(maxsize=None)
def _batches(n):
    """n loader batches of the tiny model twice: with raw uint8 video [B, 1, T, 80, 100, 3] and with the restatement's frames."""
    g, _, B, T, res = _golden()
    ids = torch.from_numpy(g["t_ids"])[:B]
    raw, cooked = [], []
    for k in range(n):
        x, y = _reference(RAW[0], RAW[1], res, B * T, "noise" if k % 2 == 0 else "ramp")
        x, y = np.roll(x, k, axis=0), np.roll(y, k, axis=0)
        idk = ids.roll(k, 0)
        head = (idk, (idk > 0).long(), torch.zeros_like(idk))
        mask = torch.ones(B, 1, T, dtype=torch.long)
        raw.append(head + (torch.from_numpy(x.copy()).view(B, 1, T, RAW[0], RAW[1], 3), mask))
        cooked.append(head + (torch.from_numpy(y.copy()).view(B, 1, T, res, res, 3), mask))
    return raw, cooked


def test_encoder_on_transformed_frames_is_bitwise_the_encoder_on_the_restatement():
    from centerclip_amd.clip import build_clip_model
    from centerclip_amd.preprocess import FrameTransform
    g, sd, B, T, res = _golden()
    args = _cfg(T)
    model, _ = build_clip_model(dict(sd), args=args)
    model = model.to(DEV)
    x, y = _reference(RAW[0], RAW[1], res, B * T, "noise")
    got, _ = model.visual.encode(FrameTransform(res)(torch.from_numpy(x.copy()).to(DEV)), T)
    want, _ = model.visual.encode(torch.from_numpy(y.copy()).to(DEV), T)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


class _Loader(list):
    pass


def _evaluate(model, batches, **kw):
    from centerclip_amd import eval as ev
    seen = {}

    class Spy(ev.HipBackend):                                # the loop's one GEMM over the cached operand planes, recorded
        @classmethod
        def dot_operands(cls, t_op, v_op, n_video, mult):
            seen["sim"] = super().dot_operands(t_op, v_op, n_video, mult)
            return seen["sim"]
    loader = _Loader(batches)
    loader.dataset = Namespace()
    r1, _, info = ev.eval_epoch(model, loader, torch.device(DEV), args=Namespace(inference_speed_test=False), backend=Spy, **kw)
    return seen["sim"].clone(), r1, list(info)


@pytest.mark.parametrize("mode", ["in_flight_1", "in_flight_2", "graphed"])
def test_eval_epoch_with_frame_transform(mode):
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.preprocess import FrameTransform
    _, sd, B, T, res = _golden()
    model = CLIP4Clip.from_state_dict(dict(sd), _cfg(T)).float().to(DEV)
    raw, cooked = _batches(3)
    kw = dict(in_flight_1=dict(in_flight=1), in_flight_2=dict(in_flight=2), graphed=dict(in_flight=1, graphed=True))[mode]
    want = _evaluate(model, cooked, **kw)
    got = _evaluate(model, raw, frame_transform=FrameTransform(res), **kw)
    assert want[0].shape == (3 * B, 3 * B) and bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    for attr in ("_eval_graphs", "_eval_lanes"):
        if hasattr(model, attr):
            delattr(model, attr)
    gc.collect()


def test_device_feeder_yields_transformed_frames_at_stable_addresses():
    from centerclip_amd.feeder import DeviceFeeder
    from centerclip_amd.preprocess import FrameTransform
    _, _, B, T, res = _golden()
    raw, cooked = _batches(3)
    host = [tuple(t.pin_memory() for t in b) for b in raw + raw[:2]]          # 5 batches over 2 slots
    want = cooked + cooked[:2]
    feeder = DeviceFeeder(DEV, depth=2, frame_transform=FrameTransform(res))
    addresses, got = {}, []
    for slot, tensors in feeder(host):
        assert len(tensors) == 5 and tensors[3].shape == (B, 1, T, res, res, 3) and tensors[3].dtype == torch.uint8
        addresses.setdefault(slot, set()).add(tuple(t.data_ptr() for t in tensors))
        got.append(tuple(t.clone() for t in tensors))
    torch.cuda.synchronize()
    assert sorted(addresses) == [0, 1] and all(len(v) == 1 for v in addresses.values())
    assert len(got) == 5
    for g_, w_ in zip(got, want):
        assert all(torch.equal(a.cpu(), b) for a, b in zip(g_, w_))
    # without a transform the feeder is what it was: the raw tensors themselves
    plain = DeviceFeeder(DEV, depth=2)
    for slot, tensors in plain(host[:1]):
        assert tensors is plain.slots[slot] and torch.equal(tensors[3].cpu(), host[0][3])


def test_train_epoch_step_with_frame_transform():
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.preprocess import FrameTransform
    from centerclip_amd.train import AdamW, prep_optim_params_groups, train_epoch
    _, sd, B, T, res = _golden()
    raw, cooked = _batches(1)
    args = Namespace(optim="AdamW", lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0)
    params = []
    for batch, kw in ((cooked[0], {}), (raw[0], dict(frame_transform=FrameTransform(res)))):
        m = CLIP4Clip.from_state_dict(dict(sd), _cfg(T)).float().to(DEV)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd)
        loss, gs = train_epoch(0, args, m, [batch], DEV, o, 0, **kw)
        torch.cuda.synchronize()
        assert gs == 1 and np.isfinite(loss)
        params.append({n: p.detach().clone() for n, p in m.named_parameters()})
        assert any(not torch.equal(before[n], params[-1][n]) for n in before)           # (the step did move the weights)
    assert params[0].keys() == params[1].keys()
    for n in params[0]:
        assert torch.equal(params[0][n], params[1][n]), n
