"""YUV 4:2:0 sources on a real MI355X (``-m gpu``): the stand-alone conversion against the NumPy restatement
(tests/yuv_ref.py), bit for bit; every fused entry - resize + crop, crop + flip, the ragged forms - against the RGB entry applied
to the conversion's output, bit for bit; then through eval_epoch and DeviceFeeder with the tiny model of
tests/golden/clip_golden.npz.  Every comparison is exact equality."""
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
import yuv_ref as Y  # noqa: E402

import centerclip_amd.torch_ops  # noqa: E402,F401  (registers torch.ops.centerclip.*)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
N_PX = 8
CONSTANTS = (0, 16, 128, 235, 240, 255)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    for f in (_planes, _loop_batches):
        f.cache_clear()
    gc.collect()                          # (no dead cycle's hipGraph may be destroyed inside a later test's capture)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _planes(F, H, W, seed=0, constants=False):
    """-> (Y, U, V) uint8 planes of F random frames (+ one constant frame per value of CONSTANTS); shared, never written"""
    y, u, v = Y.random_planes(F, H, W, seed)
    if constants:
        full = lambda a: np.concatenate([a] + [np.full_like(a[:1], c) for c in CONSTANTS], 0)
        y, u, v = full(y), full(u), full(v)
    return y, u, v


def _source(planes, kind, matrix="bt601", full=False):
    """-> (device uint8 source, eight layout integers) of the planes in arrangement ``kind``; "pitched_nv12": y_pitch = W + 3,
    c_pitch = 2 cw + 5, every gap filled with 0xAA, and the source starts one byte into its allocation"""
    y, u, v = planes
    F, H, W = y.shape
    if kind != "pitched_nv12":
        return torch.from_numpy(Y.pack(y, u, v, kind)).to(DEV), Y.layout(kind, H, W, matrix, full)
    ch, cw = Y.chroma(H), Y.chroma(W)
    yp, cp = W + 3, 2 * cw + 5
    stride = H * yp + ch * cp
    buf = np.full(1 + F * stride, 0xAA, np.uint8)
    for f in range(F):
        frame = buf[1 + f * stride:1 + (f + 1) * stride]            # (contiguous slices: the reshapes below are views)
        frame[:H * yp].reshape(H, yp)[:, :W] = y[f]
        uv = frame[H * yp:].reshape(ch, cp)
        uv[:, 0:2 * cw:2], uv[:, 1:2 * cw:2] = u[f], v[f]
    dev = torch.from_numpy(buf).to(DEV)[1:]
    assert dev.data_ptr() % 2 == 1
    return dev, [stride, yp, H * yp, H * yp + 1, cp, 2, ["bt601", "bt709"].index(matrix), int(full)]


def _to_rgb(src, F, H, W, lay, chw=False):
    return torch.ops.centerclip.yuv420_to_rgb(src, F, H, W, lay, chw)


# ------------------------------------------------------------------------------------------ the conversion
@pytest.mark.parametrize("kind", ["i420", "nv12", "nv21", "yv12", "pitched_nv12"])
@pytest.mark.parametrize("size", [(4, 4), (5, 7), (6, 4), (64, 66)], ids=lambda s: "%dx%d" % s)
def test_conversion_is_the_restatement_bit_for_bit(size, kind):
    """Two random frames and the six constant ones, the four colour modes, both output formats."""
    H, W = size
    planes = _planes(2, H, W, seed=H * 100 + W, constants=True)
    F = planes[0].shape[0]
    assert F == 2 + len(CONSTANTS)
    for matrix, full in Y.MODES:
        want = Y.planes_to_rgb(*planes, matrix, full)
        src, lay = _source(planes, kind, matrix, full)
        hwc, chw = _to_rgb(src, F, H, W, lay, False), _to_rgb(src, F, H, W, lay, True)
        assert hwc.shape == (F, H, W, 3) and chw.shape == (F, 3, H, W) and hwc.dtype == torch.uint8
        assert np.array_equal(hwc.cpu().numpy(), want), (matrix, full)
        assert np.array_equal(chw.cpu().numpy(), want.transpose(0, 3, 1, 2)), (matrix, full)


def test_python_conversion_takes_what_a_decoder_returns():
    """[..., 3H/2, W] as PyAV's to_ndarray() gives it, any leading dimensions; a descriptor that leaves the buffer raises."""
    from centerclip_amd import _lib as L
    from centerclip_amd.preprocess import yuv420_to_rgb
    planes = _planes(6, 12, 20, seed=1)
    for kind in ("i420", "nv12"):
        x = torch.from_numpy(Y.pack(*planes, kind)).view(2, 1, 3, 18, 20).to(DEV)
        got = yuv420_to_rgb(x, layout=kind, matrix="bt709", full_range=True)
        assert got.shape == (2, 1, 3, 12, 20, 3)
        assert np.array_equal(got.view(6, 12, 20, 3).cpu().numpy(), Y.planes_to_rgb(*planes, "bt709", True))
    src, lay = _source(planes, "nv12")
    with pytest.raises(L.CenterClipHipError):
        _to_rgb(src.view(-1)[:-1], 6, 12, 20, lay)                            # the last chroma byte is outside
    with pytest.raises(L.CenterClipHipError):
        _to_rgb(src, 6, 12, 20, lay[:5] + [3] + lay[6:])             # c_step = 3


# ------------------------------------------------------------------------------------------ resize + crop
@pytest.mark.parametrize("kind", ["i420", "nv12"])
@pytest.mark.parametrize("case", [(12, 20, True), (13, 21, True), (8, 20, True), (20, 8, True), (12, 20, False)],
                         ids=["12x20", "13x21", "8x20", "20x8", "12x20_crop"])
def test_resize_crop_equals_the_rgb_op_on_the_converted_frames(case, kind):
    from centerclip_amd import _lib as L
    from centerclip_amd.preprocess import YuvFrameTransform, resize_center_crop
    H, W, resize = case
    F = 3
    nws = L.lib().cc_resize_crop_workspace_bytes(F, H, W, N_PX, int(resize))
    # 12 x 20 and 13 x 21 run both passes; a short side that already is n_px leaves the frame to the crop, as resize=False does
    assert (nws > 0) == (case[:2] in ((12, 20), (13, 21)) and resize)
    planes = _planes(F, H, W, seed=7)
    for matrix, full in (("bt601", False), ("bt709", True)):
        src, lay = _source(planes, kind, matrix, full)
        rgb = _to_rgb(src, F, H, W, lay)
        want = resize_center_crop(rgb, N_PX, resize)
        got = torch.ops.centerclip.resize_center_crop_yuv420(src, F, H, W, lay, N_PX, resize, False)
        assert got.shape == (F, N_PX, N_PX, 3) and torch.equal(got, want)
        planar = torch.ops.centerclip.resize_center_crop_yuv420(src, F, H, W, lay, N_PX, resize, True)
        assert torch.equal(planar, want.permute(0, 3, 1, 2))
        out = torch.full((F, N_PX, N_PX, 3), 0xFF, dtype=torch.uint8, device=DEV)
        torch.ops.centerclip.resize_center_crop_yuv420_out(src, F, H, W, lay, N_PX, resize, False, out)
        assert torch.equal(out, want)
        if H % 2 == 0 and W % 2 == 0:                               # the decoder's array form
            t = YuvFrameTransform(N_PX, resize=resize, layout=kind, matrix=matrix, full_range=full)
            x = src.view(1, 1, F, H * 3 // 2, W)
            assert t.output_shape(x.shape) == (1, 1, F, N_PX, N_PX, 3) and torch.equal(t(x).view(want.shape), want)
    if not resize:                                                  # the crop alone is a slice of the conversion
        top, left = round((H - N_PX) / 2.0), round((W - N_PX) / 2.0)
        assert torch.equal(want, rgb[:, top:top + N_PX, left:left + N_PX])


def test_pitched_surface_and_the_tap_bound():
    """A pitched NV12 surface at an odd address through the fused entry; a 16-fold shrink (65 taps) is taken, 130 -> 8 (67
    taps) refused - as the RGB op does."""
    from centerclip_amd import _lib as L
    from centerclip_amd.preprocess import resize_center_crop
    planes = _planes(3, 13, 21, seed=7)
    src, lay = _source(planes, "pitched_nv12")
    want = resize_center_crop(_to_rgb(src, 3, 13, 21, lay), N_PX, True)
    assert torch.equal(torch.ops.centerclip.resize_center_crop_yuv420(src, 3, 13, 21, lay, N_PX, True, False), want)
    planes = _planes(1, 128, 128, seed=9)
    src, lay = _source(planes, "i420")
    want = resize_center_crop(_to_rgb(src, 1, 128, 128, lay), N_PX, True)
    assert torch.equal(torch.ops.centerclip.resize_center_crop_yuv420(src, 1, 128, 128, lay, N_PX, True, False), want)
    planes = _planes(1, 130, 130, seed=9)
    src, lay = _source(planes, "i420")
    with pytest.raises(L.CenterClipHipError):
        resize_center_crop(_to_rgb(src, 1, 130, 130, lay), N_PX, True)
    with pytest.raises(L.CenterClipHipError):
        torch.ops.centerclip.resize_center_crop_yuv420(src, 1, 130, 130, lay, N_PX, True, False)


# ------------------------------------------------------------------------------------------ crop + flip
@pytest.mark.parametrize("kind", ["i420", "nv12", "pitched_nv12"])
@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "bicubic"])
def test_crop_flip_equals_the_rgb_op_on_the_converted_frames(interp, kind):
    """Per frame one box: a downscale, the whole frame flipped, an n_px x n_px box (a byte copy of the conversion), the same
    flipped, an upscale of an odd-sized box, and a box that leaves the frame (zeros)."""
    H, W = 13, 21
    boxes = torch.tensor([[2, 3, 10, 17, 0], [0, 0, 13, 21, 1], [1, 5, 8, 8, 0], [5, 13, 8, 8, 1], [4, 6, 5, 3, 1], [6, 10, 8, 12, 0]],
                         dtype=torch.int32, device=DEV)
    F = boxes.shape[0]
    planes = _planes(F, H, W, seed=3)
    src, lay = _source(planes, kind, "bt709", False)
    rgb = _to_rgb(src, F, H, W, lay)
    want = torch.ops.centerclip.resized_crop_flip(rgb, boxes, N_PX, 1, interp)
    got = torch.ops.centerclip.resized_crop_flip_yuv420(src, F, H, W, lay, boxes, N_PX, 1, interp, False)
    assert torch.equal(got, want)
    assert torch.equal(torch.ops.centerclip.resized_crop_flip_yuv420(src, F, H, W, lay, boxes, N_PX, 1, interp, True),
                       want.permute(0, 3, 1, 2))
    assert torch.equal(got[2], rgb[2, 1:9, 5:13]) and torch.equal(got[3], rgb[3, 5:13, 13:21].flip(1))
    assert int(got[5].max()) == 0 and int(got[:5].max()) > 0
    # two frames per clip: frames 2 k and 2 k + 1 share box k
    pair = torch.ops.centerclip.resized_crop_flip_yuv420(src, F, H, W, lay, boxes[:3], N_PX, 2, interp, False)
    assert torch.equal(pair, torch.ops.centerclip.resized_crop_flip(rgb, boxes[:3], N_PX, 2, interp))


def test_train_transform_draws_the_rgb_transform_s_boxes():
    from centerclip_amd.preprocess import TrainFrameTransform, YuvTrainFrameTransform, yuv420_to_rgb
    planes = _planes(6, 12, 20, seed=4)
    x = torch.from_numpy(Y.pack(*planes, "nv12")).view(2, 1, 3, 18, 20).to(DEV)
    kw = dict(crop="random_resized", scale=(0.3, 1.0), flip=True, seed=11)
    got = YuvTrainFrameTransform(N_PX, layout="nv12", **kw)(x)
    want = TrainFrameTransform(N_PX, **kw)(yuv420_to_rgb(x, layout="nv12"))
    assert got.shape == (2, 1, 3, N_PX, N_PX, 3) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------ ragged batches
RAGGED = ((1, 12, 20), (3, 16, 16), (2, 10, 14))        # (t, H, W); max_frames = 3


def _ragged(kind):
    clips = []
    for i, (t, H, W) in enumerate(RAGGED):
        clips.append(torch.from_numpy(Y.pack(*_planes(t, H, W, seed=20 + i), kind)).view(t, H * 3 // 2, W))
    return clips


def _hip():
    """The HIP runtime this process already has loaded."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def _launches(call):
    """The number of launches ``call`` enqueues: captured into a graph on a stream of its own - never replayed - and the
    graph's nodes counted.  ``call`` runs once eagerly on that stream first, so workspaces exist before the capture."""
    hip, stream = _hip(), torch.cuda.Stream(DEV)
    graph, n = ctypes.c_void_p(), ctypes.c_size_t()
    with torch.cuda.stream(stream):
        call()
        stream.synchronize()
        handle = ctypes.c_void_p(stream.cuda_stream)
        assert hip.hipStreamBeginCapture(handle, 2) == 0             # hipStreamCaptureModeRelaxed
        try:
            call()
        finally:
            assert hip.hipStreamEndCapture(handle, ctypes.byref(graph)) == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    return n.value


@pytest.mark.parametrize("kind", ["i420", "nv12"])
def test_ragged_evaluation_form(kind):
    """Every output frame is the per-size transform of its source frame, padding frames are zero, a corrupted table row gives a
    zero frame, and the call is at most two launches - no more than the RGB entry on the same sizes."""
    from centerclip_amd import preprocess as P
    clips = _ragged(kind)
    packed = P.pack_yuv_clips(clips, kind)
    assert packed.table.tolist() == [[0, 1, 12, 20], [360, 3, 16, 16], [360 + 3 * 384, 2, 10, 14]]
    seen = {}

    class Spy(P.YuvClipCollate):
        def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
            seen["args"] = (packed.data, rows_dev, plans_dev, clips)
            return P.YuvClipCollate._eval_op(self, packed, rows_dev, plans_dev, clips, out)
    for resize in (True, False):
        collate = Spy(N_PX, max_frames=3, resize=resize, layout=kind, matrix="bt709")
        single = P.YuvFrameTransform(N_PX, resize=resize, layout=kind, matrix="bt709")
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        assert out.shape == (3, 1, 3, N_PX, N_PX, 3) and collate(packed.to(DEV), out=out) is out
        for b, (t, _, _) in enumerate(RAGGED):
            assert torch.equal(out[b, 0, :t], single(clips[b].to(DEV))), (resize, b)
            assert int(out[b, 0, t:].max() if t < 3 else 0) == 0
        assert torch.equal(collate(packed.to(DEV)), out)
    # (resize=False left its tables in `seen`) a row whose frame leaves the buffer, and one whose plan offset is wrong
    data, rows, plans, table = seen["args"]
    bad = rows.clone()
    bad[3, 1] = data.numel() - 100                                  # a 16 x 16 frame is 384 bytes
    bad[4, 4] = 1
    got = torch.ops.centerclip.collate_clips_yuv420(data, bad, plans, table, N_PX, False, P.T.YUV_KINDS[kind], 1, False, False)
    want = out.view(9, N_PX, N_PX, 3).clone()
    want[3:5] = 0
    assert torch.equal(got, want) and int(out.view(9, N_PX, N_PX, 3)[3:5].max()) > 0
    # launches: both passes run for 12 x 20 and 10 x 14 with the resize
    collate = Spy(N_PX, max_frames=3, resize=True, layout=kind)
    collate(packed.to(DEV))
    data, rows, plans, table = seen["args"]
    buf = torch.empty(9, N_PX, N_PX, 3, dtype=torch.uint8, device=DEV)
    n = _launches(lambda: torch.ops.centerclip.collate_clips_yuv420_out(data, rows, plans, table, N_PX, True,
                                                                        P.T.YUV_KINDS[kind], 0, False, False, buf))
    rgb = [P.yuv420_to_rgb(c.to(DEV), layout=kind) for c in clips]
    seen_rgb = {}

    class SpyRgb(P.ClipCollate):
        def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
            seen_rgb["args"] = (packed.data, rows_dev, plans_dev, clips)
            return P.ClipCollate._eval_op(self, packed, rows_dev, plans_dev, clips, out)
    want = SpyRgb(N_PX, max_frames=3)(P.pack_clips(rgb))
    assert torch.equal(buf.view(want.shape), want)
    d2, r2, p2, t2 = seen_rgb["args"]
    buf2 = torch.empty_like(buf)
    n_rgb = _launches(lambda: torch.ops.centerclip.collate_clips_out(d2, r2, p2, t2, N_PX, True, False, buf2))
    assert n == n_rgb == 2


@pytest.mark.parametrize("kind", ["i420", "nv12"])
def test_ragged_training_form(kind):
    from centerclip_amd import preprocess as P
    clips = _ragged(kind)
    packed = P.pack_yuv_clips(clips, kind).to(DEV)
    seen = {}

    class Spy(P.YuvClipCollate):
        def _train_op(self, packed, rows_dev, clips, out):
            seen["args"] = (packed.data, rows_dev, clips)
            return P.YuvClipCollate._train_op(self, packed, rows_dev, clips, out)
    for interp in ("bilinear", "bicubic"):
        kw = dict(crop="random_resized", scale=(0.3, 1.0), flip=True, interpolation=interp)
        collate = Spy(N_PX, max_frames=3, train=P.TrainFrameTransform(N_PX, seed=5, **kw), layout=kind)
        single = P.YuvTrainFrameTransform(N_PX, layout=kind, **kw)
        boxes = collate.sample(packed)
        twin = P.TrainFrameTransform(N_PX, seed=5, **kw)
        assert torch.equal(boxes, torch.cat([twin.sample(1, H, W) for _, H, W in RAGGED], 0))
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        assert collate.apply(packed, boxes, out=out) is out
        for b, (t, _, _) in enumerate(RAGGED):
            assert torch.equal(out[b, 0, :t], single.apply(clips[b].to(DEV), boxes[b:b + 1])), (interp, b)
            assert int(out[b, 0, t:].max() if t < 3 else 0) == 0
    data, rows, table = seen["args"]
    bad = rows.clone()
    bad[3, 1] = data.numel() - 100                                  # the frame leaves the buffer
    bad[4, 6] = 17                                                  # the box leaves its 16 x 16 frame
    bad[7, 9] = 2                                                   # no such interpolation
    kind_id = P.T.YUV_KINDS[kind]
    got = torch.ops.centerclip.collate_clips_crop_flip_yuv420(data, bad, table, N_PX, kind_id, 0, False, False)
    want = out.view(9, N_PX, N_PX, 3).clone()
    assert int(want[[3, 4, 7]].reshape(3, -1).max(1).values.min()) > 0
    want[[3, 4, 7]] = 0
    assert torch.equal(got, want)
    buf = torch.empty(9, N_PX, N_PX, 3, dtype=torch.uint8, device=DEV)
    n = _launches(lambda: torch.ops.centerclip.collate_clips_crop_flip_yuv420_out(data, rows, table, N_PX, kind_id, 0, False, False,
                                                                                  buf))
    assert n == 1 and torch.equal(buf, out.view(9, N_PX, N_PX, 3))


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
LOOP_KIND = "nv12"


def _smooth_planes(F, H, W, seed):
    """Frames with structure (random bytes as 4:2:0 give near-grey noise after the resize): ramps + a little noise"""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.stack([(yy * (f + 2) + xx * 3 + g.randint(0, 24, (H, W))) % 256 for f in range(F)]).astype(np.uint8)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    u = np.stack([(cx * 5 + f * 31 + g.randint(0, 8, cy.shape)) % 256 for f in range(F)]).astype(np.uint8)
    v = np.stack([(cy * 7 + f * 17 + g.randint(0, 8, cy.shape)) % 256 for f in range(F)]).astype(np.uint8)
    return y, u, v


@functools.lru_cache(maxsize=None)
def _loop_batches(n):
    """n loader batches of the tiny model twice: with the 4:2:0 video [B, 1, T, 120, 100] and with yuv420_to_rgb of it"""
    from centerclip_amd.preprocess import yuv420_to_rgb
    g, _, B, T, _ = _golden()
    ids = torch.from_numpy(g["t_ids"])[:B]
    yuv, rgb = [], []
    for k in range(n):
        x = torch.from_numpy(Y.pack(*_smooth_planes(B * T, RAW[0], RAW[1], 40 + k), LOOP_KIND)).view(B, 1, T, RAW[0] * 3 // 2, RAW[1])
        idk = ids.roll(k, 0)
        head = (idk, (idk > 0).long(), torch.zeros_like(idk))
        mask = torch.ones(B, 1, T, dtype=torch.long)
        yuv.append(head + (x, mask))
        rgb.append(head + (yuv420_to_rgb(x.to(DEV), layout=LOOP_KIND).cpu(), mask))
    torch.cuda.synchronize()
    return yuv, rgb


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


def test_eval_epoch_and_device_feeder_with_the_yuv_transform():
    """eval_epoch on 4:2:0 batches + YuvFrameTransform gives, bit for bit, the similarity matrix of the RGB transform on
    yuv420_to_rgb of the same frames - eagerly, graphed, and from batches a DeviceFeeder cooked from pinned host memory."""
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.feeder import DeviceFeeder
    from centerclip_amd.preprocess import FrameTransform, YuvFrameTransform
    _, sd, B, T, res = _golden()
    model = CLIP4Clip.from_state_dict(dict(sd), _cfg(T)).float().to(DEV)
    yuv, rgb = _loop_batches(3)
    eager = None
    for kw in (dict(in_flight=1), dict(in_flight=1, graphed=True)):
        want = _evaluate(model, rgb, frame_transform=FrameTransform(res), **kw)
        eager = eager or want
        got = _evaluate(model, yuv, frame_transform=YuvFrameTransform(res, layout=LOOP_KIND), **kw)
        assert want[0].shape == (3 * B, 3 * B) and bool(torch.isfinite(want[0]).all())
        assert float(want[0].std()) > 0                             # (the frames are told apart: not a constant matrix)
        assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], kw
    host = [tuple(t.pin_memory() for t in b) for b in yuv]
    feeder = DeviceFeeder(DEV, depth=2, frame_transform=YuvFrameTransform(res, layout=LOOP_KIND))
    cooked, addresses = [], {}
    for slot, tensors in feeder(host):
        assert len(tensors) == 5 and tensors[3].shape == (B, 1, T, res, res, 3) and tensors[3].dtype == torch.uint8
        addresses.setdefault(slot, set()).add(tensors[3].data_ptr())
        cooked.append(tuple(t.clone().cpu() for t in tensors))
    torch.cuda.synchronize()
    assert len(cooked) == 3 and all(len(v) == 1 for v in addresses.values())
    fed = _evaluate(model, cooked, in_flight=1)
    assert torch.equal(fed[0], eager[0]) and fed[1] == eager[1] and fed[2] == eager[2]
    for attr in ("_eval_graphs", "_eval_lanes"):
        if hasattr(model, attr):
            delattr(model, attr)
    gc.collect()


def test_captured_replay_equals_the_eager_call():
    from centerclip_amd.preprocess import YuvFrameTransform
    a = torch.from_numpy(Y.pack(*_planes(5, 100, 38, seed=1), "i420")).view(5, 150, 38)
    b = torch.from_numpy(Y.pack(*_planes(5, 100, 38, seed=2), "i420")).view(5, 150, 38)
    t = YuvFrameTransform(32, layout="i420")
    static = a.to(DEV)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        eager = t(static).clone()                                    # (plan uploaded, workspace of this stream allocated)
    stream.synchronize()
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        y = t(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, t(static)) and not torch.equal(y, eager)
    del graph
