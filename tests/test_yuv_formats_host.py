"""YUV sources in general (4:2:2, 4:4:4, 10 / 12 / 16-bit) without a GPU: the coefficient tables, the integer definition against
the real formula on a lattice of every depth, the tight layouts, the descriptor checks of the C ABI (pointers that are never
followed), the Python refusals and shapes, and the ops' fake kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_formats_ref as R  # noqa: E402
import yuv_ref as Y8  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = sorted(R.FORMATS)


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import _lib as L, build
    build.build(verbose=False)
    return L.lib()


def test_the_name_table_is_the_restatement():
    from centerclip_amd.torch_ops import YUV_FORMATS
    assert YUV_FORMATS == R.FORMATS and len(NAMES) == 12


def test_coefficients_are_the_published_tables(lib):
    from centerclip_amd.preprocess import yuv_coefficients
    for (depth, matrix, full), row in R.TABLE.items():
        assert yuv_coefficients(matrix, full, depth=depth) == row == R.coefficients(matrix, full, depth)
    out = (ctypes.c_int32 * 5)()
    for depth in R.DEPTHS:
        for matrix, full in R.MODES:
            assert lib.cc_yuv_coefficients_depth(R.MATRICES.index(matrix), int(full), depth, out) == 0
            assert tuple(out) == R.coefficients(matrix, full, depth), (depth, matrix, full)
            if depth == 8:                                           # the existing tables and the two-argument meaning stay
                assert tuple(out) == Y8.TABLE[(matrix, full)] == yuv_coefficients(matrix, full)
    for bad in ((2, 0, 10), (0, 2, 10), (0, 0, 9), (0, 0, 14), (0, 0, 0), (0, -1, 8)):
        assert lib.cc_yuv_coefficients_depth(*bad, out) == INVALID, bad
    assert lib.cc_yuv_coefficients_depth(0, 0, 10, None) == INVALID
    with pytest.raises(ValueError):
        yuv_coefficients("bt2020")
    with pytest.raises(ValueError):
        yuv_coefficients("bt2020", depth=10)


@pytest.mark.parametrize("depth", R.DEPTHS)
def test_integer_definition_on_the_lattice(depth):
    """Every 2^d / 1024-th luma value x every 2^d / 96-th chroma value squared (plus both ends and the two centre values): the
    int32 accumulator holds every sum (the issue's figure, 5.8e8, is the cap), and the result is within 1 LSB of
    clamp(floor(real + 0.5)).  The share of differing samples is printed, not bounded: it is 0.02 % at depth 8 and grows to 0.6 %
    of the samples (1.8 % of the triples) at depth 16, whose coefficients keep 12 significant bits."""
    luma, chroma = R.lattice(depth)
    assert luma[0] == 0 and luma[-1] == 2 ** depth - 1 and {0, 2 ** depth - 1, 2 ** (depth - 1) - 1, 2 ** (depth - 1)} <= set(chroma.tolist())
    y, u, v = np.meshgrid(luma, chroma, chroma, indexing="ij")
    for matrix, full in R.MODES:
        acc = R.accumulators(y, u, v, matrix, full, depth)
        top = int(np.abs(acc).max())
        got, real = R.convert(y, u, v, matrix, full, depth), R.convert_real(y, u, v, matrix, full, depth)
        d = np.abs(got.astype(np.int16) - real.astype(np.int16))
        print("d=%d %s full=%s: max |acc| %.3e, max |diff| %d, differing samples %.4f %%, triples %.4f %%"
              % (depth, matrix, full, top, d.max(), 100 * np.count_nonzero(d) / d.size, 100 * np.count_nonzero(d.max(-1)) / d[..., 0].size))
        assert top < 2 ** 31 and top <= 5.8e8
        assert int(d.max()) <= 1
        if depth == 8:
            assert np.array_equal(got, Y8.convert(y, u, v, matrix, full))


def _tight(lib, name, H, W, matrix=0, rng=0):
    from centerclip_amd import _lib as L
    lay = L.YuvLayout()
    return lib.cc_yuv_layout_tight(R.FORMATS[name][0], H, W, matrix, rng, ctypes.byref(lay)), lay


def _ints(lay):
    return [getattr(lay, k) for k, _ in lay._fields_]


@pytest.mark.parametrize("name", NAMES)
def test_tight_layouts(lib, name):
    from centerclip_amd.torch_ops import yuv_tight_layout
    for H, W in ((12, 20), (13, 21)):
        n, lay = _tight(lib, name, H, W, 1, 1)
        want = R.layout(name, H, W, "bt709", True)
        assert n == want[0] and _ints(lay) == want == yuv_tight_layout(name, H, W, "bt709", True)
        planes = R.random_planes(name, 2, H, W)
        assert R.pack(*planes, name).nbytes == 2 * n                  # the packing fills exactly the frames the layout describes


def test_tight_layout_refusals_and_the_420_entry(lib):
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import yuv420_tight_layout, yuv_tight_layout
    for bad in ((12, 5, 7, 0, 0), (-1, 5, 7, 0, 0), (0, 0, 7, 0, 0), (7, 5, 8193, 0, 0), (7, 5, 7, 2, 0), (7, 5, 7, 0, -1)):
        assert lib.cc_yuv_layout_tight(*bad, ctypes.byref(L.YuvLayout())) == 0, bad
    assert lib.cc_yuv_layout_tight(0, 5, 7, 0, 0, None) == 0
    for name in ("i420", "nv12"):                                    # the 8-bit 4:2:0 descriptor is the general one's subset
        g, old = yuv_tight_layout(name, 13, 21, "bt709", True), yuv420_tight_layout(name, 13, 21, "bt709", True)
        assert g[:6] + g[10:] == old == Y8.layout(name, 13, 21, "bt709", True) and g[6:10] == [1, 1, 8, 0]
    with pytest.raises(ValueError):
        yuv_tight_layout("yv12", 4, 4, "bt601", False)
    with pytest.raises(ValueError):
        yuv_tight_layout("p010", 4, 4, "bt2020", False)


def test_descriptor_is_checked_before_any_launch(lib):
    """Non-NULL pointers that are never followed: every call below is refused (or, for the last group, stops at the missing
    workspace) before a launch."""
    from centerclip_amd import _lib as L
    one = ctypes.c_void_p(16)
    F, H, W, n_px = 3, 12, 20, 8
    n, good = _tight(lib, "p010", H, W)
    assert n == 720
    n8, good8 = _tight(lib, "i422", H, W)
    assert n8 == 480

    def variant(base=good, **kw):
        lay = L.YuvLayout()
        ctypes.pointer(lay)[0] = base
        for k, v in kw.items():
            setattr(lay, k, v)
        return lay

    def calls(lay, src_bytes, H=H, W=W, src=one, dst=one):
        p = ctypes.byref(lay) if lay is not None else None
        return (lib.cc_yuv_to_rgb_u8(src, src_bytes, p, F, H, W, dst, 2, None),
                lib.cc_resize_crop_yuv_u8(src, src_bytes, p, F, H, W, one, n_px, 1, dst, 2, None, 0, None),
                lib.cc_resized_crop_flip_yuv_u8(src, src_bytes, p, F, H, W, 1, one, n_px, 0, dst, 2, None))

    total, big = F * n, 1 << 40
    invalid = [
        (good, total - 1),                                            # the last chroma byte of the last frame is outside
        (variant(depth=9), big), (variant(depth=14), big), (variant(depth=0), big), (variant(depth=32), big),   # depth
        (variant(shift=7), big), (variant(shift=-1), big), (variant(depth=12, shift=5), big), (variant(depth=16, shift=1), big),
        (variant(good8, shift=1), big),                               # a shift at depth 8
        (variant(sub_x=2), big), (variant(sub_y=-1), big), (variant(sub_y=2), big),
        (variant(c_step=1), big), (variant(c_step=3), big), (variant(c_step=8), big), (variant(c_step=0), big),   # 2 or 4 at 16 bits
        (variant(good8, c_step=4), big), (variant(good8, c_step=0), big),                                         # 1 or 2 at 8 bits
        (variant(matrix=2), big), (variant(range=2), big), (variant(range=-1), big),
        (variant(frame_stride=-2), big), (variant(u_offset=-2), big), (variant(v_offset=-2), big),                # a negative field
        (variant(y_pitch=2 * W - 2), big), (variant(c_pitch=2 * W - 4), big), (variant(y_pitch=-2), big),          # pitch < row
        (variant(good8, y_pitch=W - 1), big), (variant(good8, c_pitch=W // 2 - 1), big),
        (variant(frame_stride=n + 1), big), (variant(y_pitch=2 * W + 1), big), (variant(u_offset=good.u_offset + 1), big),
        (variant(v_offset=good.v_offset + 1), big), (variant(c_pitch=good.c_pitch + 1), big),                     # odd positions
        (variant(v_offset=good.v_offset + 2), total), (variant(frame_stride=n + 2), total), (variant(y_pitch=2 * W + 24), total),
        (None, total)]
    for lay, nbytes in invalid:
        assert calls(lay, nbytes) == (INVALID,) * 3, (lay and _ints(lay), nbytes)
    assert calls(good, total, src=ctypes.c_void_p(17)) == (INVALID,) * 3          # 16-bit samples at an odd address
    assert calls(good, total, src=None) == (INVALID,) * 3 and calls(good, total, dst=None) == (INVALID,) * 3
    # sizes outside 4 .. 8192 are CC_ERR_UNSUPPORTED, after the descriptor's own fields and before its positions
    assert calls(good, big, H=3) == (UNSUPPORTED,) * 3 and calls(good, big, W=8194) == (UNSUPPORTED,) * 3
    assert calls(variant(depth=9), big, H=3) == (INVALID,) * 3
    assert lib.cc_yuv_to_rgb_u8(one, total, ctypes.byref(good), F, H, W, one, 3, None) == INVALID            # dst_fmt
    assert lib.cc_yuv_to_rgb_u8(one, total, ctypes.byref(good), 0, H, W, one, 2, None) == INVALID            # F
    # a sound descriptor gets as far as the RGB entry does: both passes run for 12 x 20 -> 8, so the missing workspace stops it
    nws = lib.cc_resize_crop_workspace_bytes(F, H, W, n_px, 1)
    assert nws > 0
    args = (F, H, W, one, n_px, 1, one, 2)
    for lay, nbytes, src in ((good, total, one), (good8, F * n8, ctypes.c_void_p(17))):
        assert lib.cc_resize_crop_yuv_u8(src, nbytes, ctypes.byref(lay), *args, None, 0, None) == WORKSPACE
        assert lib.cc_resize_crop_yuv_u8(src, nbytes, ctypes.byref(lay), *args, one, nws - 1, None) == WORKSPACE
    # odd H and W are legal: chroma planes of ceil(H / 2) x ceil(W / 2)
    n13, lay13 = _tight(lib, "p010", 13, 21)
    assert n13 == 2 * (13 * 21 + 2 * 7 * 11)
    assert lib.cc_resize_crop_yuv_u8(one, F * n13, ctypes.byref(lay13), F, 13, 21, one, n_px, 1, one, 2, None, 0, None) == WORKSPACE
    assert lib.cc_resize_crop_yuv_u8(one, F * n13 - 1, ctypes.byref(lay13), F, 13, 21, one, n_px, 1, one, 2, None, 0, None) == INVALID
    # a pitched surface that fits, and the same one byte short
    pitched = variant(y_pitch=2 * W + 6, u_offset=H * (2 * W + 6), v_offset=H * (2 * W + 6) + 2, frame_stride=n + 6 * H)
    assert calls(pitched, F * (n + 6 * H) - 1)[0] == INVALID
    assert lib.cc_resize_crop_yuv_u8(one, F * (n + 6 * H), ctypes.byref(pitched), *args, None, 0, None) == WORKSPACE
    # the tap bound is the RGB entry's
    n130, lay130 = _tight(lib, "i444p16", 130, 130)
    assert lib.cc_resize_crop_yuv_u8(one, n130, ctypes.byref(lay130), 1, 130, 130, one, 8, 1, one, 2, one, 1 << 20, None) == UNSUPPORTED


def test_ragged_entries_validate_before_any_launch(lib):
    one = ctypes.c_void_p(16)
    P010, I444 = R.FORMATS["p010"][0], R.FORMATS["i444"][0]
    n = 2 * 720                                                    # two tight 12 x 20 P010 frames
    ok, over, odd = (ctypes.c_int64 * 4)(0, 2, 12, 20), (ctypes.c_int64 * 4)(2, 2, 12, 20), (ctypes.c_int64 * 4)(1, 1, 12, 20)
    ev = lambda fmt, m, r, clips, nb=n, src=one: lib.cc_collate_resize_crop_yuv_u8(src, nb, fmt, m, r, clips, 1, one, 6, one, 64, 8, 1,
                                                                                   one, 2, None, 0, None)
    tr = lambda fmt, m, r, clips, nb=n, src=one: lib.cc_collate_crop_flip_yuv_u8(src, nb, fmt, m, r, clips, 1, one, 6, 8, one, 2, None)
    for f in (ev, tr):
        assert f(12, 0, 0, ok) == INVALID and f(-1, 0, 0, ok) == INVALID and f(P010, 2, 0, ok) == INVALID and f(P010, 0, 2, ok) == INVALID
        assert f(P010, 0, 0, over) == INVALID and f(P010, 0, 0, ok, n - 1) == INVALID
        assert f(P010, 0, 0, odd) == INVALID                         # 16-bit frames at an odd byte offset
        assert f(P010, 0, 0, ok, src=ctypes.c_void_p(17)) == INVALID
        assert f(P010, 0, 0, (ctypes.c_int64 * 4)(0, 2, 3, 20)) == UNSUPPORTED
        assert f(I444, 0, 0, (ctypes.c_int64 * 4)(1, 2, 12, 20), 1 + 2 * 720 - 1) == INVALID       # 4:4:4 8-bit: 720 bytes a frame
    assert ev(P010, 0, 0, ok) == WORKSPACE                           # a sound call gets as far as the RGB entry
    assert ev(I444, 0, 0, (ctypes.c_int64 * 4)(1, 2, 12, 20), 1 + 2 * 720, ctypes.c_void_p(17)) == WORKSPACE


def test_header_and_design_state_the_definition():
    text = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("cc_yuv_coefficients_depth", "cc_yuv_layout_tight", "cc_yuv_to_rgb_u8", "cc_resize_crop_yuv_u8",
                "cc_resized_crop_flip_yuv_u8", "cc_collate_resize_crop_yuv_u8", "cc_collate_crop_flip_yuv_u8"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for row in R.TABLE.values():
        assert re.search(r"\s+".join(map(str, row)), text), row
        assert all(str(v) in design for v in row), row
    for doc in (text, design, open(os.path.join(ROOT, "centerclip_amd", "csrc", "cc_pixels.h")).read()):
        for word in ("BT.2020", "YUYV", "big-endian", "4:1:1", "alpha", "siting", "dithering"):
            assert word in doc, word                                # what is out of scope is said


def test_fake_kernels_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import centerclip_amd.torch_ops as TO
    for name in ("yuv_to_rgb", "resize_center_crop_yuv", "resize_center_crop_yuv_out", "resized_crop_flip_yuv",
                 "resized_crop_flip_yuv_out", "collate_clips_yuv", "collate_clips_yuv_out", "collate_clips_crop_flip_yuv",
                 "collate_clips_crop_flip_yuv_out"):
        assert name in TO.OPS
    ops = torch.ops.centerclip
    lay, fmt = R.layout("p010", 12, 20), R.FORMATS["p010"][0]
    with FakeTensorMode():
        for src in (torch.empty(3, 18, 20, dtype=torch.uint16), torch.empty(3, 18, 20, dtype=torch.int16),
                    torch.empty(3 * 720, dtype=torch.uint8)):
            for chw, shape in ((False, (3, 8, 8, 3)), (True, (3, 3, 8, 8))):
                out = ops.yuv_to_rgb(src, 3, 12, 20, lay, chw)
                assert tuple(out.shape) == ((3, 3, 12, 20) if chw else (3, 12, 20, 3)) and out.dtype == torch.uint8
                out = ops.resize_center_crop_yuv(src, 3, 12, 20, lay, 8, True, chw)
                assert tuple(out.shape) == shape and out.dtype == torch.uint8
                assert ops.resize_center_crop_yuv_out(src, 3, 12, 20, lay, 8, True, chw, torch.empty(shape, dtype=torch.uint8)) is None
                boxes = torch.empty(3, 5, dtype=torch.int32)
                out = ops.resized_crop_flip_yuv(src, 3, 12, 20, lay, boxes, 8, 1, 1, chw)
                assert tuple(out.shape) == shape and out.dtype == torch.uint8
                assert ops.resized_crop_flip_yuv_out(src, 3, 12, 20, lay, boxes, 8, 1, 1, chw, torch.empty(shape, dtype=torch.uint8)) is None
        flat, plans = torch.empty(3 * 720, dtype=torch.uint8), torch.empty(100, dtype=torch.int32)
        for chw, shape in ((False, (6, 8, 8, 3)), (True, (6, 3, 8, 8))):
            rows = torch.empty(6, TO.COLLATE_ROW, dtype=torch.int64)
            buf = torch.empty(shape, dtype=torch.uint8)
            assert tuple(ops.collate_clips_yuv(flat, rows, plans, [0, 3, 12, 20], 8, True, fmt, 0, False, chw).shape) == shape
            assert ops.collate_clips_yuv_out(flat, rows, plans, [0, 3, 12, 20], 8, True, fmt, 0, False, chw, buf) is None
            rows = torch.empty(6, TO.COLLATE_BOX_ROW, dtype=torch.int64)
            assert tuple(ops.collate_clips_crop_flip_yuv(flat, rows, [0, 3, 12, 20], 8, fmt, 1, True, chw).shape) == shape
            assert ops.collate_clips_crop_flip_yuv_out(flat, rows, [0, 3, 12, 20], 8, fmt, 1, True, chw, buf) is None
        src = torch.empty(3, 18, 20, dtype=torch.uint16)
        boxes = torch.empty(3, 5, dtype=torch.int32)
        for call in (lambda l: ops.yuv_to_rgb(src, 3, 12, 20, l, False), lambda l: ops.resize_center_crop_yuv(src, 3, 12, 20, l, 8, True, False),
                     lambda l: ops.resized_crop_flip_yuv(src, 3, 12, 20, l, boxes, 8, 1, 0, False)):
            for wrong in (lay[:11], lay + [0], lay[:8]):
                with pytest.raises(ValueError, match="twelve integers"):
                    call(wrong)
        with pytest.raises(ValueError, match="uint16"):               # words of an 8-bit layout
            ops.yuv_to_rgb(src, 3, 12, 20, R.layout("nv12", 12, 20), False)
        with pytest.raises(ValueError, match="format"):
            ops.collate_clips_yuv(flat, torch.empty(6, TO.COLLATE_ROW, dtype=torch.int64), plans, [0, 3, 12, 20], 8, True, 12, 0, False,
                                  False)
        with pytest.raises(ValueError, match="format"):
            ops.collate_clips_crop_flip_yuv(flat, torch.empty(6, TO.COLLATE_BOX_ROW, dtype=torch.int64), [0, 3, 12, 20], 8, -1, 0,
                                            False, False)


def test_python_level_checks_need_no_gpu():
    """Every new name is taken, shapes follow the sampling (3H/2, 2H, 3H rows), dtypes follow the depth, unknown names and CPU
    tensors raise; packing is host work."""
    from centerclip_amd import _lib as L
    from centerclip_amd import preprocess as P
    from centerclip_amd.feeder import DeviceFeeder
    for name in NAMES:
        _, sx, sy, depth, _, _ = R.FORMATS[name]
        rows = R.frame_rows(name, 12)
        assert rows == {2: 18, 1: 24, 0: 36}[sx + sy]
        dt = torch.uint8 if depth == 8 else torch.uint16
        t = P.YuvFrameTransform(8, layout=name, matrix="bt709")
        assert t.frame_dtypes == ((torch.uint8,) if depth == 8 else (torch.uint16, torch.int16))
        assert t.output_shape((2, 1, 4, rows, 20)) == (2, 1, 4, 8, 8, 3) and not t.passes_through((2, rows, 20))
        tr = P.YuvTrainFrameTransform(8, layout=name, crop="center")
        assert tr.output_shape((3, rows, 20)) == (3, 8, 8, 3)
        x = torch.zeros(2, rows, 20, dtype=dt)
        for f in (lambda: P.yuv_to_rgb(x, name), lambda: t(x), lambda: tr(x)):
            with pytest.raises(L.CenterClipHipError):                # a CPU tensor
                f()
        for bad in ((2, rows + 1, 20), (rows, 20)) + (((2, rows, 21),) if sx else ()):
            with pytest.raises(ValueError, match={2: "3H/2", 1: "2H", 0: "3H"}[sx + sy]):
                t.output_shape(bad)
        if sy:                                                       # an odd H where rows are subsampled: 3 * 13 / 2 is no integer
            with pytest.raises(ValueError):
                t.output_shape((2, 19, 20))
        npdt = np.uint8 if depth == 8 else np.uint16
        clips = [torch.from_numpy(np.full((1, rows, 20), 7, npdt)), torch.from_numpy(np.ones((3, R.frame_rows(name, 16), 16), npdt))]
        packed = P.pack_yuv_clips(clips, name)
        n0, n1 = R.layout(name, 12, 20)[0], R.layout(name, 16, 16)[0]
        assert packed.layout == name and packed.data.dtype == torch.uint8 and packed.data.numel() == n0 + 3 * n1
        assert packed.table.tolist() == [[0, 1, 12, 20], [n0, 3, 16, 16]]
        assert packed.clip(0).dtype == dt and torch.equal(packed.clip(0).view(torch.uint8), clips[0].view(torch.uint8))
        assert packed[[1]].table.tolist() == [[0, 3, 16, 16]] and packed[[1]].layout == name
        collate = P.YuvClipCollate(8, max_frames=3, layout=name)
        assert collate.output_shape(packed) == (2, 1, 3, 8, 8, 3)
        with pytest.raises(L.CenterClipHipError):
            collate(packed)
        wrong = torch.zeros(1, rows, 20, dtype=torch.uint16 if depth == 8 else torch.uint8)
        with pytest.raises(ValueError):
            P.pack_yuv_clips([wrong], name)
    # int16 with the same bits is taken where uint16 is
    words = np.arange(18 * 20, dtype=np.uint16).reshape(1, 18, 20) * 150
    a, b = P.pack_yuv_clips([words], "p010"), P.pack_yuv_clips([words.view(np.int16)], "p010")
    assert torch.equal(a.data, b.data) and np.array_equal(a.clip(0).numpy(), words)
    for name in ("yv12", "nv21", "p210", "yuyv"):
        with pytest.raises(ValueError):
            P.YuvFrameTransform(8, layout=name)
        with pytest.raises(ValueError):
            P.pack_yuv_clips([words], name)
        with pytest.raises(ValueError):
            P.yuv_to_rgb(torch.zeros(1, 18, 20, dtype=torch.uint8), name)
    with pytest.raises(ValueError):
        P.YuvFrameTransform(8, layout="p010", matrix="bt2020")
    # DeviceFeeder finds the 16-bit video of a batch by the transform's dtypes
    batch = (torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 1, 3, 18, 20, dtype=torch.uint16), torch.zeros(2, 1, 3, dtype=torch.long))
    feeder = DeviceFeeder.__new__(DeviceFeeder)
    feeder.frame_transform, feeder.video_index = P.YuvFrameTransform(8, layout="p010"), None
    assert feeder._video_index(batch) == 1
    feeder.frame_transform = P.YuvFrameTransform(8, layout="nv12")
    with pytest.raises(ValueError):
        feeder._video_index(batch)
