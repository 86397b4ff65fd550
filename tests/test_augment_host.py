"""CPU-only checks of the train-time augmentation (preprocess.TrainFrameTransform, torch.ops.centerclip.resized_crop_flip,
cc_resized_crop_flip_u8): the samplers against the reference's recorded boxes (tests/golden/augment_boxes.json,
tools/gen_golden_augment.py) and torchvision's published properties, the ABI's early returns, the fake kernels, and the float64
restatement the GPU test compares bytes against (tests/augment_ref.py), anchored to torch's own interpolate.  Nothing here
touches a GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR  # noqa: E402

from conftest import GOLDEN  # noqa: E402

SIZES = {(320, 240, 224), (640, 360, 224), (226, 300, 224), (224, 224, 224), (60, 45, 32)}          # (W, H, n_px)


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "augment_boxes.json")))


def _assert_case(case, **kw):
    from centerclip_amd.preprocess import TrainFrameTransform
    t = TrainFrameTransform(case["n_px"], crop="multiscale", seed=case["seed"], flip=case["flip"], **kw)
    got = t.sample(len(case["boxes"]), case["H"], case["W"])
    assert got.dtype == torch.int32 and got.shape == (len(case["boxes"]), 5) and not got.is_cuda
    want = [[oh, ow, ch, cw, fl] for (cw, ch, ow, oh), fl in zip(case["boxes"], case.get("flips", [0] * len(case["boxes"])))]
    assert got.tolist() == want, (case["seed"], case["W"], case["H"], kw)


def test_multiscale_sampler_draws_the_reference_boxes_and_flips(recorded):
    cases = recorded["cases"]
    assert {(c["W"], c["H"], c["n_px"]) for c in cases} == SIZES and len({c["seed"] for c in cases}) >= 3
    assert all(len(c["boxes"]) == 8 for c in cases) and {c["flip"] for c in cases} == {False, True}
    assert any(1 in c["flips"] for c in cases if c["flip"]) and any(0 in c["flips"] for c in cases if c["flip"])
    for c in cases:
        _assert_case(c)
    assert sorted(recorded["variants"]) == ["five_offsets", "free_offsets", "no_distort"]
    for v in recorded["variants"].values():
        for c in v["cases"]:
            _assert_case(c, **v["kwargs"])


def test_sampler_draws_per_clip_in_order():
    """One generator: a clip's box, then its flip; two objects with one seed agree, and 3 + 5 clips are the 8 of one call."""
    from centerclip_amd.preprocess import TrainFrameTransform
    for crop in ("multiscale", "random_resized", "center"):
        a, b = (TrainFrameTransform(32, crop=crop, flip=True, seed=11) for _ in range(2))
        whole = a.sample(8, 45, 60)
        assert torch.equal(torch.cat([b.sample(3, 45, 60), b.sample(5, 45, 60)]), whole)
        assert set(whole[:, 4].tolist()) <= {0, 1}
    assert TrainFrameTransform(32, crop="center", seed=0).sample(2, 45, 61).tolist() == [[6, 14, 32, 32, 0]] * 2    # 6.5 -> 6, 14.5 -> 14
    assert TrainFrameTransform(32, crop="center", seed=0).sample(1, 47, 63).tolist() == [[8, 16, 32, 32, 0]]        # 7.5 -> 8, 15.5 -> 16
    assert TrainFrameTransform(224).interp == 0 and TrainFrameTransform(224, crop="random_resized").interp == 1
    assert TrainFrameTransform(224, interpolation="bicubic").interp == 1
    with pytest.raises(ValueError):
        TrainFrameTransform(224, crop="five")
    with pytest.raises(ValueError):
        TrainFrameTransform(224, interpolation="nearest")


@pytest.mark.parametrize("H,W", [(240, 320), (45, 60)])
def test_random_resized_boxes_have_torchvision_properties(H, W):
    """200 draws: every box lies in the frame; unless it is the fallback, its area lies in scale x H W and its ratio in `ratio`
    - up to the rounding of w and h to integers (each side moves by at most 1/2: |w h - w* h*| <= (w + h + 1) / 2 + 1/4, and
    w* / h* lies in [(w - 1/2) / (h + 1/2), (w + 1/2) / (h - 1/2)])."""
    from centerclip_amd.preprocess import TrainFrameTransform
    for scale, ratio in (((0.9, 1.0), (3 / 4, 4 / 3)), ((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 0.6), (0.5, 0.9))):
        t = TrainFrameTransform(32, crop="random_resized", scale=scale, ratio=ratio, seed=5)
        boxes = t.sample(200, H, W)
        fallback = t.fallback_box(H, W)
        regular = 0
        for top, left, h, w, flip in boxes.tolist():
            assert 0 <= top and 0 <= left and 1 <= h and 1 <= w and top + h <= H and left + w <= W and flip == 0
            if (top, left, h, w) == fallback:
                continue
            regular += 1
            slack = (w + h + 1) / 2 + 0.25
            assert scale[0] * H * W - slack <= h * w <= scale[1] * H * W + slack, (h, w)
            assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / (h - 0.5) >= ratio[0], (h, w)
        assert regular >= 20                                    # (the properties were looked at)
        assert len({tuple(b) for b in boxes.tolist()}) > 10     # and the boxes do vary
    # the fallback itself: a frame wider / taller than `ratio` allows is cut to the nearer bound, centred
    t = TrainFrameTransform(32, crop="random_resized", seed=0)
    assert t.fallback_box(100, 400) == (0, 133, 100, 133) and t.fallback_box(400, 100) == (133, 0, 133, 100)
    assert t.fallback_box(240, 320) == (0, 0, 240, 320)


def test_a_crop_that_leaves_the_frame_raises():
    from centerclip_amd.preprocess import TrainFrameTransform
    with pytest.raises(ValueError, match="leaves"):
        TrainFrameTransform(224, crop="center").sample(1, 200, 320)
    with pytest.raises(ValueError, match="leaves"):                       # min side 222 -> crop size 224 (within 3): wider than the frame
        TrainFrameTransform(224, crop="multiscale", scales=(1,), seed=0).sample(1, 222, 320)
    with pytest.raises(ValueError):
        TrainFrameTransform(224, crop="multiscale", scales=(1,), fix_crop=False, seed=0).sample(1, 222, 320)


# ---- the C ABI's early returns.  Pointers that are only tested against NULL point into this host buffer; no case reaches a launch.
_BUF = (ctypes.c_char * 4096)()
PTR = ctypes.c_void_p(ctypes.addressof(_BUF))


def test_abi_early_returns_need_no_gpu(lib):
    INVALID, UNSUPPORTED = -1, -2

    def call(src=PTR, fmt=2, F=4, H=45, W=60, fpc=2, boxes=PTR, n_px=32, interp=0, dst=PTR, dst_fmt=2):
        return lib.cc_resized_crop_flip_u8(src, fmt, F, H, W, fpc, boxes, n_px, interp, dst, dst_fmt, None)
    for kw in (dict(src=None), dict(dst=None), dict(boxes=None), dict(F=0), dict(F=-3), dict(fpc=0), dict(fpc=-1),
               dict(fmt=0), dict(fmt=3), dict(dst_fmt=0), dict(interp=2), dict(interp=-1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(n_px=0), dict(n_px=1025), dict(H=3), dict(W=3), dict(H=8193), dict(W=8193)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(src=None, n_px=0) == INVALID                              # (arguments before ranges)
    assert bytes(_BUF) == bytes(4096)


def test_header_declares_and_library_exports_the_entry_point(lib):
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "centerclip_hip.h")).read()
    assert "cc_resized_crop_flip_u8(" in text and hasattr(lib, "cc_resized_crop_flip_u8")
    from centerclip_amd import build
    assert build.STRICT["augment.hip"] == ["-ffp-contract=off"]


def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from centerclip_amd import torch_ops
    assert "resized_crop_flip" in torch_ops.OPS and "resized_crop_flip_out" in torch_ops.OPS
    op = torch.ops.centerclip.resized_crop_flip
    with FakeTensorMode():
        boxes = lambda n: torch.empty(n, 5, device="cuda", dtype=torch.int32)                       # noqa: E731
        hwc = torch.empty(6, 45, 60, 3, device="cuda", dtype=torch.uint8)
        chw = torch.empty(6, 3, 45, 60, device="cuda", dtype=torch.uint8)
        y = op(hwc, boxes(1), 32, 6, 0)
        assert y.shape == (6, 32, 32, 3) and y.dtype == torch.uint8 and y.device.type == "cuda"
        assert op(chw, boxes(2), 32, 3, 1).shape == (6, 3, 32, 32)
        assert op(chw, boxes(2), 32, 4, 1).shape == (6, 3, 32, 32)          # the last clip is short: ceil(6 / 4) rows
        v = torch.empty(2, 1, 4, 240, 320, 3, device="cuda", dtype=torch.uint8)
        assert op(v, boxes(2), 224, 4, 1).shape == (2, 1, 4, 224, 224, 3)
        assert op(v.permute(0, 1, 2, 5, 3, 4), boxes(2), 224, 4, 0).shape == (2, 1, 4, 3, 224, 224)
        out = torch.empty(2, 1, 4, 224, 224, 3, device="cuda", dtype=torch.uint8)
        assert torch.ops.centerclip.resized_crop_flip_out(v, boxes(2), 224, 4, 1, out) is None
        for bad in (lambda: op(hwc, boxes(2), 32, 6, 0),                    # one clip, two rows
                    lambda: op(hwc, boxes(1).long(), 32, 6, 0),
                    lambda: op(hwc, boxes(1), 32, 6, 2),
                    lambda: op(hwc, boxes(6), 32, 0, 0),
                    lambda: op(hwc.float(), boxes(1), 32, 6, 0),
                    lambda: op(torch.empty(45, 60, 3, device="cuda", dtype=torch.uint8), boxes(1), 32, 1, 0)):
            with pytest.raises(ValueError):
                bad()
    assert "Tensor(a" in str(torch.ops.centerclip.resized_crop_flip_out.default._schema)


def test_python_api_refuses_cpu_tensors_and_describes_its_output():
    from centerclip_amd.preprocess import TrainFrameTransform
    t = TrainFrameTransform(32, seed=0, flip=True)
    x = torch.zeros(2, 1, 3, 45, 60, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        t(x)
    with pytest.raises(RuntimeError):
        t.apply(x, t.sample(2, 45, 60))
    with pytest.raises(RuntimeError):
        torch.ops.centerclip.resized_crop_flip(x, torch.zeros(2, 5, dtype=torch.int32), 32, 3, 0)
    assert not t.passes_through((7, 32, 32, 3)) and not t.passes_through((2, 1, 3, 45, 60, 3))
    assert t.output_shape((2, 1, 3, 3, 45, 60)) == (2, 1, 3, 3, 32, 32) and t.output_shape((7, 45, 60, 3)) == (7, 32, 32, 3)
    assert t._clips((2, 1, 3, 45, 60, 3)) == (2, 3) and t._clips((7, 3, 45, 60)) == (1, 7)
    import centerclip_amd.preprocess as P
    assert "TrainFrameTransform" in P.__all__


# ---- the float64 restatement
BOXES = {(45, 60): [(0, 0, 45, 45), (1, 3, 39, 33), (16, 27, 29, 33), (0, 0, 45, 60)],
         (37, 53): [(0, 0, 37, 37), (1, 3, 32, 27), (13, 26, 24, 27), (0, 0, 37, 53)]}


@pytest.mark.parametrize("H,W", sorted(BOXES))
def test_restatement_is_anchored_to_torch_interpolate(H, W):
    """255 * F.interpolate(crop / 255, (32, 32), mode, align_corners=False) on the CPU, whose coordinates and weights are fp32,
    against the float64 restatement: within 1e-3 of a level (measured: <= 6.3e-5; the margin is for other torch builds); and with flip it is the reversed columns."""
    frames = np.random.default_rng(0).integers(0, 256, (2, 3, H, W), np.uint8)
    worst = 0.0
    for interp, mode in ((0, "bilinear"), (1, "bicubic")):
        for (top, left, h, w) in BOXES[(H, W)]:
            crop = torch.from_numpy(frames[:, :, top:top + h, left:left + w].copy())
            want = 255 * torch.nn.functional.interpolate(crop.float() / 255, (32, 32), mode=mode, align_corners=False)
            got = AR.resized_crop_flip(frames, (top, left, h, w), 32, interp)
            worst = max(worst, float(np.abs(got - want.double().numpy()).max()))
            assert np.array_equal(AR.resized_crop_flip(frames, (top, left, h, w), 32, interp, flip=True), got[..., ::-1])
    print("largest |restatement - 255 interpolate(x / 255)|: %.2e" % worst)
    assert worst <= 1e-3


def test_restatement_of_an_identity_box_is_the_slice():
    frames = np.random.default_rng(0).integers(0, 256, (2, 3, 45, 60), np.uint8)
    for interp in (0, 1):
        for dtype in (np.float64, np.float32):
            v = AR.resized_crop_flip(frames, (2, 5, 32, 32), 32, interp, dtype=dtype)
            assert np.array_equal(v, frames[:, :, 2:34, 5:37].astype(dtype))
            idx, w = AR.axis_taps(32, 32, interp, dtype)
            assert set(np.unique(w)) == {0.0, 1.0}


@pytest.mark.parametrize("interp", [0, 1])
def test_the_kernels_arithmetic_keeps_the_derived_bound(interp):
    """The kernel's operations in IEEE single (augment_ref.kernel_fp32) against the float64 values on the GPU test's small boxes:
    the fp32 value stays within DELTA of the exact one, so its bytes pass the rule the GPU test applies."""
    assert AR.DELTA[interp] <= 1e-2
    worst = 0.0
    for (H, W), boxes in sorted(BOXES.items()):
        frames = np.random.default_rng(0).integers(0, 256, (2, 3, H, W), np.uint8)
        for box in boxes:
            for flip in (False, True):
                v = AR.resized_crop_flip(frames, box, 32, interp, flip)
                v32 = AR.resized_crop_flip(frames, box, 32, interp, flip, np.float32)
                assert v32.dtype == np.float32
                worst = max(worst, float(np.abs(v32.astype(np.float64) - v).max()))
                AR.check_bytes(AR.to_bytes(v32), v, AR.DELTA[interp])
    print("largest |fp32 value - float64 value| (interp %d): %.2e of a level, bound %.1e" % (interp, worst, AR.DELTA[interp]))
    assert worst <= AR.DELTA[interp]
