"""CPU-only checks of the device frame transform (Resize(n_px, BICUBIC) -> CenterCrop(n_px) on uint8 frames): the NumPy
restatement against Pillow and the golden file, the library's host-built plan against the restatement, geometry, range
refusals, the fake kernel and the exports.  Everything is byte equality; nothing here touches a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402

from conftest import GOLDEN  # noqa: E402

SIDES = (17, 32, 33, 37, 57, 64, 100, 300)
EXTRA = ((240, 320), (360, 640), (224, 398), (480, 360))
HDR = 16


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "resize_golden.npz"))


def build_plan(lib, H, W, n_px, resize=1):
    nbytes = lib.cc_resize_plan_bytes(H, W, n_px, resize)
    assert nbytes > 0 and nbytes % 4 == 0, (H, W, n_px, resize, nbytes)
    buf = np.full(nbytes // 4 + 4, -77, np.int32)                   # (4 guard words behind the plan)
    rc = lib.cc_resize_plan_build(H, W, n_px, resize, ctypes.c_void_p(buf.ctypes.data))
    assert rc == 0, (H, W, n_px, resize, rc)
    assert (buf[-4:] == -77).all() and buf[15] == nbytes // 4
    return buf[:-4]


def plan_tables(plan, which):
    """-> (first, count, coef [n_px, ksize]) of the horizontal (0) / vertical (1) table, as include/centerclip_hip.h lays it out"""
    n_px, ksize, off = int(plan[3]), int(plan[11 + which]), int(plan[13 + which])
    first, count = plan[off:off + n_px], plan[off + n_px:off + 2 * n_px]
    coef = plan[off + 2 * n_px:off + 2 * n_px + n_px * ksize].reshape(n_px, ksize)
    return first, count, coef


def apply_plan(plan, frames):
    """The plan applied with NumPy as the kernels apply it: horizontal pass over source rows [row0, row1) for the window's
    columns, vertical pass on those bytes for the window's rows; a pass with ksize 0 is a slice."""
    H, W, n_px = int(plan[1]), int(plan[2]), int(plan[3])
    top, left, row0, row1, kh, kv = (int(plan[i]) for i in (7, 8, 9, 10, 11, 12))
    assert frames.shape[1:3] == (H, W) and 0 <= row0 < row1 <= H
    mid = frames[:, row0:row1]
    if kh:
        mid = R.apply_axis(mid, -2, *plan_tables(plan, 0))
    else:
        mid = mid[:, :, left:left + n_px]
    if kv:
        first, count, coef = plan_tables(plan, 1)
        assert (first >= row0).all() and (first + count <= row1).all()
        return R.apply_axis(mid, -3, first - row0, count, coef)
    assert (row0, row1) == (top, top + n_px)
    return mid


def test_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    for (H, W) in ((33, 57), (100, 37), (17, 64), (50, 50), (32, 57), (512, 300), (240, 320), (57, 55), (59, 55)):
        for kind in ("noise", "checker"):
            x = R.make_input(H, W, kind, seed=H)
            oh, ow = R.resized_size(H, W, 32)
            img = Image.fromarray(x[0])
            if (oh, ow) != (H, W):
                img = img.resize((ow, oh), Image.BICUBIC)
            top, left = R.crop_offset(oh, 32), R.crop_offset(ow, 32)
            want = np.asarray(img)[top:top + 32, left:left + 32]
            assert np.array_equal(R.resize_center_crop(x, 32)[0], want), (H, W, kind)


def test_restatement_equals_golden(golden):
    n_px = int(golden["n_px"])
    names = sorted(k[3:] for k in golden.files if k.startswith("in/"))
    assert names == sorted(R.cases())
    for name in names:
        assert np.array_equal(R.resize_center_crop(golden["in/" + name], n_px), golden["out/" + name]), name


def _sweep():
    return [(H, W) for H in SIDES for W in SIDES] + list(EXTRA)


@pytest.mark.parametrize("n_px", (14, 32, 224))
def test_plan_equals_restatement(lib, n_px):
    """The host-built tables, applied with NumPy, against the restatement - and the tables themselves against the restatement's
    coefficients, over every size of the sweep: a contracted multiply-add or a reciprocal in the host code shows up here as a
    coefficient one unit off."""
    for (H, W) in _sweep():
        plan = build_plan(lib, H, W, n_px)
        oh, ow = R.resized_size(H, W, n_px)
        top, left = R.crop_offset(oh, n_px), R.crop_offset(ow, n_px)
        assert tuple(plan[1:9]) == (H, W, n_px, 1, oh, ow, top, left), (H, W, n_px)
        for which, (n_in, n_out, org) in enumerate(((W, ow, left), (H, oh, top))):
            first, count, coef = plan_tables(plan, which)
            if n_in == n_out:
                assert plan[11 + which] == 0 and np.array_equal(first, org + np.arange(n_px)) and not count.any()
                continue
            ksize, xmin, cnt, ref = R.axis_coefficients(n_in, n_out)
            assert plan[11 + which] == ksize
            assert np.array_equal(first, xmin[org:org + n_px]) and np.array_equal(count, cnt[org:org + n_px])
            assert np.array_equal(coef, ref[org:org + n_px]), (H, W, n_px, which)
        # the pixels: one frame of noise and one of checkerboard
        x = np.concatenate([R.make_input(H, W, "noise", seed=H * 1000 + W), R.make_input(H, W, "checker")], 0)
        assert np.array_equal(apply_plan(plan, x), R.resize_center_crop(x, n_px)), (H, W, n_px)


def test_crop_only_plan(lib):
    plan = build_plan(lib, 57, 64, 32, resize=0)
    assert tuple(plan[4:13]) == (0, 57, 64, 12, 16, 12, 44, 0, 0)
    x = R.make_input(57, 64, "noise")
    assert np.array_equal(apply_plan(plan, x), x[:, 12:44, 16:48])
    assert lib.cc_resize_crop_workspace_bytes(4, 57, 64, 32, 0) == 0


def test_crop_offsets_round_half_to_even(lib):
    # landscape 32 x (32 + d): ow - n_px = 23 -> 11.5 -> 12, 25 -> 12.5 -> 12; portrait the same for top
    for d, want in ((23, 12), (25, 12), (24, 12), (26, 13), (1, 0), (3, 2)):
        assert R.crop_offset(32 + d, 32) == want
        assert build_plan(lib, 32, 32 + d, 32)[8] == want and build_plan(lib, 32, 32 + d, 32)[7] == 0
        assert build_plan(lib, 32 + d, 32, 32)[7] == want and build_plan(lib, 32 + d, 32, 32, resize=0)[7] == want
    # through a resize: 64 x 110 -> 32 x 55 (ow - n_px = 23), 64 x 114 -> 32 x 57 (25)
    assert tuple(build_plan(lib, 64, 110, 32)[5:9]) == (32, 55, 0, 12)
    assert tuple(build_plan(lib, 64, 114, 32)[5:9]) == (32, 57, 0, 12)


def test_workspace_is_the_horizontal_result(lib):
    plan = build_plan(lib, 100, 37, 32)
    assert plan[11] and plan[12]
    assert lib.cc_resize_crop_workspace_bytes(5, 100, 37, 32, 1) == 5 * 3 * int(plan[10] - plan[9]) * 32
    assert int(plan[10] - plan[9]) < 100                             # portrait: only the rows the window reads
    assert lib.cc_resize_crop_workspace_bytes(5, 32, 57, 32, 1) == 0 # no resampling at all
    assert lib.cc_resize_crop_workspace_bytes(5, 64, 114, 32, 1) > 0


def test_range_refusals_need_no_gpu(lib):
    UNSUPPORTED, INVALID, WORKSPACE = -2, -1, -3
    buf = np.zeros(1 << 16, np.int32)
    host = ctypes.c_void_p(buf.ctypes.data)
    for (H, W, n_px, resize) in ((3, 64, 32, 1), (64, 3, 32, 1), (8193, 64, 32, 1), (64, 8193, 32, 1), (64, 64, 0, 1),
                                 (64, 64, 1025, 1),
                                 (520, 520, 32, 1), (224, 398, 14, 1),      # 67 / 69 taps: the launches stop at 65
                                 (31, 64, 32, 0), (64, 31, 32, 0)):        # crop of a smaller frame: the padding is not built
        if min(H, W) >= 224:                                                # (the plan builder alone takes any tap count)
            assert max(build_plan(lib, H, W, n_px)[11:13]) > 65
        else:
            assert lib.cc_resize_plan_bytes(H, W, n_px, resize) == 0, (H, W, n_px, resize)
            assert lib.cc_resize_plan_build(H, W, n_px, resize, host) == UNSUPPORTED, (H, W, n_px, resize)
        assert lib.cc_resize_crop_workspace_bytes(1, H, W, n_px, resize) == 0
        # (non-NULL pointers that are never followed: the refusal comes before any launch)
        assert lib.cc_resize_crop_u8(host, 2, 1, H, W, host, n_px, resize, host, 2, None, 0, None) == UNSUPPORTED
    assert not buf.any()
    assert lib.cc_resize_plan_bytes(512, 512, 32, 1) > 0                 # shrink 16: 65 taps, the last size built
    assert tuple(build_plan(lib, 512, 512, 32)[11:13]) == (65, 65)
    assert lib.cc_resize_plan_build(64, 64, 32, 2, host) == INVALID
    assert lib.cc_resize_plan_build(64, 64, 32, 1, None) == INVALID
    ok = (2, 1, 64, 114)
    assert lib.cc_resize_crop_u8(None, *ok, host, 32, 1, host, 2, host, 1 << 16, None) == INVALID
    assert lib.cc_resize_crop_u8(host, *ok, None, 32, 1, host, 2, host, 1 << 16, None) == INVALID
    assert lib.cc_resize_crop_u8(host, *ok, host, 32, 1, None, 2, host, 1 << 16, None) == INVALID
    assert lib.cc_resize_crop_u8(host, 0, 1, 64, 114, host, 32, 1, host, 2, host, 1 << 16, None) == INVALID   # fp32 code
    assert lib.cc_resize_crop_u8(host, 2, 0, 64, 114, host, 32, 1, host, 2, host, 1 << 16, None) == INVALID
    assert lib.cc_resize_crop_u8(host, *ok, host, 32, 1, host, 2, None, 0, None) == WORKSPACE
    need = lib.cc_resize_crop_workspace_bytes(1, 64, 114, 32, 1)
    assert lib.cc_resize_crop_u8(host, *ok, host, 32, 1, host, 2, host, need - 1, None) == WORKSPACE


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from centerclip_amd import torch_ops
    assert "resize_center_crop" in torch_ops.OPS and "resize_center_crop_out" in torch_ops.OPS
    with FakeTensorMode():
        hwc = torch.empty(5, 33, 57, 3, device="cuda", dtype=torch.uint8)
        chw = torch.empty(5, 3, 33, 57, device="cuda", dtype=torch.uint8)
        y = torch.ops.centerclip.resize_center_crop(hwc, 32, True)
        assert y.shape == (5, 32, 32, 3) and y.dtype == torch.uint8 and y.device.type == "cuda"
        assert torch.ops.centerclip.resize_center_crop(chw, 32, True).shape == (5, 3, 32, 32)
        v = torch.empty(2, 1, 4, 240, 320, 3, device="cuda", dtype=torch.uint8)
        assert torch.ops.centerclip.resize_center_crop(v, 224, True).shape == (2, 1, 4, 224, 224, 3)
        assert torch.ops.centerclip.resize_center_crop(v.permute(0, 1, 2, 5, 3, 4), 224, False).shape == (2, 1, 4, 3, 224, 224)
        with pytest.raises(ValueError):
            torch.ops.centerclip.resize_center_crop(torch.empty(33, 57, 3, device="cuda", dtype=torch.uint8), 32, True)


def test_python_api_refuses_cpu_tensors_and_other_dtypes():
    from centerclip_amd.preprocess import FrameTransform, resize_center_crop
    x = torch.zeros(2, 33, 57, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        resize_center_crop(x, 32)
    with pytest.raises(RuntimeError):
        FrameTransform(32)(x)
    with pytest.raises(RuntimeError):
        FrameTransform(32)(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))      # even where it would pass through
    t = FrameTransform(32)
    assert t.output_shape((2, 1, 4, 3, 100, 37)) == (2, 1, 4, 3, 32, 32)
    assert t.passes_through((7, 32, 32, 3)) and not t.passes_through((7, 32, 33, 3))


def test_unseen_size_inside_a_capture_is_refused(monkeypatch):
    """The plan upload cannot be captured: a size without a cached plan raises before anything touches the device."""
    from centerclip_amd import _lib, torch_ops
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(_lib.CenterClipHipError, match="captured"):
        torch_ops.resize_plan(123, 77, 32, True, "cuda:0")
    assert not any(k[:2] == (123, 77) for k in torch_ops._RESIZE_PLANS)


def test_hooks_default_to_none():
    import inspect
    from centerclip_amd.eval import eval_epoch
    from centerclip_amd.feeder import DeviceFeeder
    from centerclip_amd.train.loop import train_epoch
    for fn in (eval_epoch, train_epoch, DeviceFeeder.__init__):
        assert inspect.signature(fn).parameters["frame_transform"].default is None
    assert inspect.signature(DeviceFeeder.__init__).parameters["video_index"].default is None


def test_header_declares_and_library_exports_the_entry_points(lib):
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "centerclip_hip.h")).read()
    for name in ("cc_resize_plan_bytes", "cc_resize_plan_build", "cc_resize_crop_workspace_bytes", "cc_resize_crop_u8"):
        assert name + "(" in text and hasattr(lib, name)
    assert "#define CC_RESIZE_PLAN_HEADER %d" % HDR in text


def test_product_code_never_imports_pillow():
    pkg = os.path.join(os.path.dirname(GOLDEN), "..", "centerclip_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "import PIL" not in src and "from PIL" not in src, f
