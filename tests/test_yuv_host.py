"""YUV 4:2:0 sources without a GPU: the coefficient tables, the integer definition against the real formula over all 256^3
triples, the descriptor checks of the C ABI (pointers that are never followed) and the ops' fake kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import _lib as L, build
    build.build(verbose=False)
    return L.lib()


@pytest.mark.parametrize("matrix,full", Y.MODES)
def test_coefficients_are_the_published_tables(lib, matrix, full):
    from centerclip_amd.preprocess import yuv_coefficients
    assert yuv_coefficients(matrix, full) == Y.TABLE[(matrix, full)] == Y.coefficients(matrix, full)
    out = (ctypes.c_int32 * 5)()
    assert lib.cc_yuv_coefficients(2, 0, out) == INVALID and lib.cc_yuv_coefficients(0, 2, out) == INVALID
    with pytest.raises(ValueError):
        yuv_coefficients("bt2020")


@pytest.mark.parametrize("matrix,full", Y.MODES)
def test_integer_definition_is_within_one_lsb_of_the_real_formula(matrix, full):
    """All 256^3 (Y, Cb, Cr) triples, one luma value at a time: the largest difference is 1 and under 0.1 % of the samples
    differ at all (a cap; the restatement gives below 0.03 %)."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, differ = 0, 0
    for y in range(256):
        d = np.abs(Y.convert(np.full_like(u, y), u, v, matrix, full).astype(np.int16)
                   - Y.convert_real(np.full_like(u, y), u, v, matrix, full).astype(np.int16))
        worst, differ = max(worst, int(d.max())), differ + int(np.count_nonzero(d))
    share = differ / (3 * 256 ** 3)
    print("%s full=%s: max |diff| %d, differing samples %.5f %%" % (matrix, full, worst, 100 * share))
    assert worst == 1
    assert share < 1e-3


def test_known_colours():
    """Limited-range black, white and grey, and the full-range identity on grey."""
    f = lambda y, u, v, **kw: Y.convert(np.array([y]), np.array([u]), np.array([v]), **kw)[0].tolist()
    assert f(16, 128, 128) == [0, 0, 0] and f(235, 128, 128) == [255, 255, 255] and f(0, 128, 128) == [0, 0, 0]
    assert f(126, 128, 128) == [128, 128, 128] and f(77, 128, 128, full_range=True) == [77, 77, 77]
    assert f(255, 128, 128) == [255, 255, 255]
    red = f(81, 90, 240)                                            # BT.601 red, (81.5, 90.2, 240) rounded to bytes
    assert red[0] >= 253 and red[1] <= 2 and red[2] <= 2


def _tight(lib, kind, H, W, matrix=0, rng=0):
    from centerclip_amd import _lib as L
    lay = L.Yuv420Layout()
    return lib.cc_yuv420_layout_tight(kind, H, W, matrix, rng, ctypes.byref(lay)), lay


def test_tight_layouts(lib):
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import yuv420_tight_layout
    n, lay = _tight(lib, 0, 5, 7)
    assert n == 35 + 2 * 12 == lay.frame_stride
    assert (lay.y_pitch, lay.u_offset, lay.v_offset, lay.c_pitch, lay.c_step, lay.matrix, lay.range) == (7, 35, 47, 4, 1, 0, 0)
    n, lay = _tight(lib, 1, 5, 7, 1, 1)
    assert n == 59 and (lay.y_pitch, lay.u_offset, lay.v_offset, lay.c_pitch, lay.c_step, lay.matrix, lay.range) == \
        (7, 35, 36, 8, 2, 1, 1)
    for kind, name in ((0, "i420"), (1, "nv12")):
        for H, W in ((4, 4), (5, 7), (6, 4), (64, 66)):
            assert yuv420_tight_layout(name, H, W, "bt709", True) == Y.layout(name, H, W, "bt709", True)
    for bad in ((2, 5, 7, 0, 0), (0, 0, 7, 0, 0), (0, 5, 8193, 0, 0), (0, 5, 7, 2, 0), (0, 5, 7, 0, -1)):
        assert lib.cc_yuv420_layout_tight(*bad, ctypes.byref(L.Yuv420Layout())) == 0, bad
    with pytest.raises(ValueError):
        yuv420_tight_layout("yv12", 4, 4, "bt601", False)


def test_descriptor_is_checked_before_any_launch(lib):
    """Non-NULL pointers that are never followed: every call below is refused (or, for the last group, stops at the missing
    workspace) before a launch.  H = 3 is outside 4 .. 8192: CC_ERR_UNSUPPORTED, as the RGB entries give."""
    from centerclip_amd import _lib as L
    one = ctypes.c_void_p(16)
    F, H, W, n_px = 3, 12, 20, 8
    n, good = _tight(lib, 1, H, W)
    assert n == 360

    def variant(**kw):
        lay = L.Yuv420Layout()
        ctypes.pointer(lay)[0] = good
        for k, v in kw.items():
            setattr(lay, k, v)
        return lay

    def calls(lay, src_bytes, H=H, src=one, dst=one):
        p = ctypes.byref(lay) if lay is not None else None
        return (lib.cc_yuv420_to_rgb_u8(src, src_bytes, p, F, H, W, dst, 2, None),
                lib.cc_resize_crop_yuv420_u8(src, src_bytes, p, F, H, W, one, n_px, 1, dst, 2, None, 0, None),
                lib.cc_resized_crop_flip_yuv420_u8(src, src_bytes, p, F, H, W, 1, one, n_px, 0, dst, 2, None))

    total = F * n
    for lay, nbytes in ((good, total - 1),                          # the last chroma byte of the last frame is outside
                        (variant(c_step=3), total), (variant(c_step=0), total), (variant(matrix=2), total),
                        (variant(range=2), total), (variant(range=-1), total),
                        (variant(y_pitch=W - 1), total), (variant(c_pitch=W - 2), total), (variant(u_offset=-1), total),
                        (variant(v_offset=good.v_offset + 1), total), (variant(frame_stride=n + 1), total),
                        (variant(frame_stride=-1), 1 << 40), (variant(y_pitch=W + 12), total), (None, total)):
        assert calls(lay, nbytes) == (INVALID,) * 3, (lay and [getattr(lay, k) for k, _ in lay._fields_], nbytes)
    assert calls(good, total, src=None) == (INVALID,) * 3 and calls(good, total, dst=None) == (INVALID,) * 3
    assert calls(good, total, H=3) == (UNSUPPORTED,) * 3
    assert lib.cc_resize_crop_u8(one, 2, F, 3, W, one, n_px, 1, one, 2, None, 0, None) == UNSUPPORTED      # (as the RGB entry)
    assert lib.cc_yuv420_to_rgb_u8(one, total, ctypes.byref(good), F, H, W, one, 3, None) == INVALID      # dst_fmt
    # a sound descriptor gets as far as the RGB entry does: both passes run for 12 x 20 -> 8, so the missing workspace stops it
    nws = lib.cc_resize_crop_workspace_bytes(F, H, W, n_px, 1)
    assert nws > 0
    args = (F, H, W, one, n_px, 1, one, 2)
    assert lib.cc_resize_crop_yuv420_u8(one, total, ctypes.byref(good), *args, None, 0, None) == WORKSPACE \
        == lib.cc_resize_crop_u8(one, 2, *args, None, 0, None)
    assert lib.cc_resize_crop_yuv420_u8(one, total, ctypes.byref(good), *args, one, nws - 1, None) == WORKSPACE
    # a pitched surface that fits: y_pitch = W + 3 needs 3 bytes more per luma row
    pitched = variant(y_pitch=W + 3, u_offset=H * (W + 3), v_offset=H * (W + 3) + 1, frame_stride=n + 3 * H)
    assert calls(pitched, F * (n + 3 * H) - 1)[0] == INVALID
    assert lib.cc_resize_crop_yuv420_u8(one, F * (n + 3 * H), ctypes.byref(pitched), *args, None, 0, None) == WORKSPACE
    # the tap bound is the RGB entry's: a 16-fold shrink (65 taps) is taken, 66 and more refused
    assert lib.cc_resize_crop_status(128, 128, 8, 1) == 0 and lib.cc_resize_crop_status(130, 130, 8, 1) == UNSUPPORTED
    n130, lay130 = _tight(lib, 0, 130, 130)
    assert lib.cc_resize_crop_yuv420_u8(one, n130, ctypes.byref(lay130), 1, 130, 130, one, 8, 1, one, 2, one, 1 << 20, None) \
        == UNSUPPORTED


def test_ragged_entries_validate_before_any_launch(lib):
    one = ctypes.c_void_p(16)
    n = 2 * 360                                                    # two tight 12 x 20 frames
    ok, over = (ctypes.c_int64 * 4)(0, 2, 12, 20), (ctypes.c_int64 * 4)(1, 2, 12, 20)
    ev = lambda kind, m, r, clips, nb=n: lib.cc_collate_resize_crop_yuv420_u8(one, nb, kind, m, r, clips, 1, one, 6, one, 64, 8, 1, one,
                                                                              2, None, 0, None)
    tr = lambda kind, m, r, clips, nb=n: lib.cc_collate_crop_flip_yuv420_u8(one, nb, kind, m, r, clips, 1, one, 6, 8, one, 2, None)
    for f in (ev, tr):
        assert f(2, 0, 0, ok) == INVALID and f(0, 2, 0, ok) == INVALID and f(0, 0, 2, ok) == INVALID
        assert f(0, 0, 0, over) == INVALID and f(1, 0, 0, ok, n - 1) == INVALID
        assert f(0, 0, 0, (ctypes.c_int64 * 4)(0, 2, 3, 20)) == UNSUPPORTED
    # a sound call gets as far as the RGB entry: the missing workspace (the RGB clip of these sizes needs 3 H W bytes a frame)
    assert ev(0, 0, 0, ok) == WORKSPACE
    assert lib.cc_collate_resize_crop_u8(one, 4 * n, 2, ok, 1, one, 6, one, 64, 8, 1, one, 2, None, 0, None) == WORKSPACE


def test_header_declares_the_entry_points_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("cc_yuv_coefficients", "cc_yuv420_layout_tight", "cc_yuv420_to_rgb_u8", "cc_resize_crop_yuv420_u8",
                "cc_resized_crop_flip_yuv420_u8", "cc_collate_resize_crop_yuv420_u8", "cc_collate_crop_flip_yuv420_u8"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
    for row in Y.TABLE.values():
        assert re.search(r"\s+".join(map(str, row)), text), row
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "YUV 4:2:0 sources" in design and "swscale" in design
    for row in Y.TABLE.values():
        assert all(str(v) in design for v in row), row


def test_fake_kernels_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import centerclip_amd.torch_ops as TO
    for name in ("yuv420_to_rgb", "resize_center_crop_yuv420", "resize_center_crop_yuv420_out", "resized_crop_flip_yuv420",
                 "resized_crop_flip_yuv420_out", "collate_clips_yuv420", "collate_clips_yuv420_out",
                 "collate_clips_crop_flip_yuv420", "collate_clips_crop_flip_yuv420_out"):
        assert name in TO.OPS
    lay = Y.layout("nv12", 12, 20)
    with FakeTensorMode():
        src = torch.empty(3, 18, 20, dtype=torch.uint8)
        for chw, shape in ((False, (3, 8, 8, 3)), (True, (3, 3, 8, 8))):
            assert tuple(torch.ops.centerclip.yuv420_to_rgb(src, 3, 12, 20, lay, chw).shape) == \
                ((3, 3, 12, 20) if chw else (3, 12, 20, 3))
            out = torch.ops.centerclip.resize_center_crop_yuv420(src, 3, 12, 20, lay, 8, True, chw)
            assert tuple(out.shape) == shape and out.dtype == torch.uint8
            boxes = torch.empty(3, 5, dtype=torch.int32)
            assert tuple(torch.ops.centerclip.resized_crop_flip_yuv420(src, 3, 12, 20, lay, boxes, 8, 1, 1, chw).shape) == shape
            rows = torch.empty(6, TO.COLLATE_ROW, dtype=torch.int64)
            flat, plans = src.view(-1), torch.empty(100, dtype=torch.int32)
            assert tuple(torch.ops.centerclip.collate_clips_yuv420(flat, rows, plans, [0, 3, 12, 20], 8, True, 1, 0, False,
                                                                   chw).shape) == (6,) + shape[1:]
            rows = torch.empty(6, TO.COLLATE_BOX_ROW, dtype=torch.int64)
            assert tuple(torch.ops.centerclip.collate_clips_crop_flip_yuv420(flat, rows, [0, 3, 12, 20], 8, 0, 1, True,
                                                                             chw).shape) == (6,) + shape[1:]
        with pytest.raises(ValueError, match="eight integers"):
            torch.ops.centerclip.yuv420_to_rgb(src, 3, 12, 20, lay[:7], False)
        with pytest.raises(ValueError, match="kind"):
            torch.ops.centerclip.collate_clips_yuv420(flat, torch.empty(6, TO.COLLATE_ROW, dtype=torch.int64), plans,
                                                      [0, 3, 12, 20], 8, True, 2, 0, False, False)


def test_python_level_checks_need_no_gpu():
    """Shapes that are no [..., 3H/2, W], unknown names, and CPU tensors raise; packing is host work."""
    from centerclip_amd import _lib as L
    from centerclip_amd import preprocess as P
    x = torch.zeros(2, 18, 20, dtype=torch.uint8)
    for f in (lambda: P.yuv420_to_rgb(x), lambda: P.YuvFrameTransform(8)(x),
              lambda: P.YuvTrainFrameTransform(8, crop="center")(x)):
        with pytest.raises(L.CenterClipHipError):
            f()
    with pytest.raises(ValueError):
        P.YuvFrameTransform(8, layout="yv12")
    with pytest.raises(ValueError):
        P.YuvFrameTransform(8, matrix="bt2020")
    t = P.YuvFrameTransform(8, layout="nv12")
    assert t.output_shape((2, 1, 4, 18, 20)) == (2, 1, 4, 8, 8, 3) and not t.passes_through((2, 18, 20))
    for bad in ((2, 17, 20), (2, 18, 21), (18, 20)):
        with pytest.raises(ValueError, match="3H/2"):
            t.output_shape(bad)
    tr = P.YuvTrainFrameTransform(8, layout="nv12", crop="multiscale", flip=True, seed=5)
    twin = P.TrainFrameTransform(8, crop="multiscale", flip=True, seed=5)
    assert isinstance(tr, P.TrainFrameTransform) and "sample" not in vars(P.YuvTrainFrameTransform)      # the box drawing is reused
    assert torch.equal(tr.sample(4, 12, 20), twin.sample(4, 12, 20)) and tr.output_shape((3, 18, 20)) == (3, 8, 8, 3)
    clips = [np.arange(1 * 18 * 20, dtype=np.uint8).reshape(1, 18, 20), np.ones((3, 24, 16), np.uint8), np.zeros((2, 15, 14), np.uint8)]
    packed = P.pack_yuv_clips(clips, "nv12")
    assert isinstance(packed, P.PackedClips) and packed.layout == "nv12" and not packed.chw
    assert packed.table.tolist() == [[0, 1, 12, 20], [360, 3, 16, 16], [360 + 3 * 384, 2, 10, 14]]
    assert packed.data.numel() == 360 + 3 * 384 + 2 * 210 and np.array_equal(packed.clip(0).numpy(), clips[0])
    assert packed.video_mask(3).tolist() == [[1, 0, 0], [1, 1, 1], [1, 1, 0]]
    assert packed[[2, 0]].table.tolist() == [[0, 2, 10, 14], [420, 1, 12, 20]] and packed[[2, 0]].layout == "nv12"
    collate = P.YuvClipCollate(8, max_frames=3, layout="nv12")
    assert collate.output_shape(packed) == (3, 1, 3, 8, 8, 3)
    with pytest.raises(L.CenterClipHipError):
        collate(packed)
    with pytest.raises(ValueError):
        P.pack_yuv_clips([np.zeros((1, 17, 20), np.uint8)])
    with pytest.raises(ValueError):
        P.pack_yuv_clips(clips, "yv12")
