"""YUV sources in general on a real MI355X (``-m gpu``): 4:2:2, 4:4:4 and 10 / 12 / 16-bit frames.  The stand-alone conversion of
every named format against the NumPy restatement (tests/yuv_formats_ref.py), bit for bit; the four fused entries - resize + crop,
crop + flip and their ragged forms - against the RGB entry applied to the conversion's output, bit for bit; the general entries at
i420 / nv12 against the ``*_yuv420`` entries; launch counts from a captured graph; one eval_epoch run fed P010 frames.  Every
comparison is exact equality, and every test uses an op the parent does not have."""
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
import yuv_formats_ref as R  # noqa: E402
import yuv_ref as Y8  # noqa: E402

import centerclip_amd.torch_ops  # noqa: E402,F401  (registers torch.ops.centerclip.*)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
OPS = torch.ops.centerclip
FUSED = ("p010_pitched", "i420p10", "i422", "i444", "p016", "i444p16")
# (H, W, n_px, resize): 12 x 20 and 13 x 21 (odd: ceil-sized chroma planes) run both passes; 36 x 52 -> 8 has 19 and 28 taps; the
# crop alone where the frame is no smaller than the crop
CASES = ((12, 20, 8, True), (13, 21, 8, True), (36, 52, 8, True), (36, 52, 16, True), (12, 20, 8, False), (36, 52, 16, False))


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    _planes.cache_clear()
    gc.collect()                          # (no dead cycle's hipGraph may be destroyed inside a later test's capture)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _planes(name, F, H, W, seed=0):
    """Sample values of F random frames of the named format, with 0, the maximum and both centre values; shared, never written"""
    return R.random_planes(name, F, H, W, seed)


def _source(kind, F, H, W, seed=0, matrix="bt601", full=False):
    """-> (device source, twelve layout integers): tight frames of the named format as [F, samples] words (uint8 / uint16), or
    "<name>_pitched": a pitched surface as bytes, every gap filled with 0xAA"""
    name = kind.replace("_pitched", "")
    planes = _planes(name, F, H, W, seed)
    if kind.endswith("_pitched"):
        buf, lay = R.pack_pitched(*planes, name, matrix=matrix, full_range=full)
        assert lay[1] > W * 2 and lay[0] > H * lay[1] + R.chroma(H, 1) * lay[4]          # pitch > row, frame stride > frame
        return torch.from_numpy(buf).to(DEV), lay
    return torch.from_numpy(R.pack(*planes, name)).to(DEV), R.layout(name, H, W, matrix, full)


# ------------------------------------------------------------------------------------------ the conversion
@pytest.mark.parametrize("name", sorted(R.FORMATS))
def test_conversion_is_the_restatement_bit_for_bit(name):
    """12 x 20 and 13 x 21, three random frames holding 0, the maximum and both centre values, the four colour modes, both
    output formats; 16-bit words as uint16 and as int16 with the same bits."""
    depth = R.FORMATS[name][3]
    for H, W in ((12, 20), (13, 21)):
        planes = _planes(name, 3, H, W, seed=H)
        for k, (matrix, full) in enumerate(R.MODES):
            want = R.planes_to_rgb(*planes, name, matrix, full)
            src, lay = _source(name, 3, H, W, H, matrix, full)
            assert src.dtype == (torch.uint8 if depth == 8 else torch.uint16)
            if depth > 8 and k == 1:
                src = src.view(torch.int16)
            hwc, chw = OPS.yuv_to_rgb(src, 3, H, W, lay, False), OPS.yuv_to_rgb(src, 3, H, W, lay, True)
            assert hwc.shape == (3, H, W, 3) and chw.shape == (3, 3, H, W) and hwc.dtype == torch.uint8
            assert np.array_equal(hwc.cpu().numpy(), want), (H, W, matrix, full)
            assert np.array_equal(chw.cpu().numpy(), want.transpose(0, 3, 1, 2)), (H, W, matrix, full)


@pytest.mark.parametrize("name", ["p010", "p012"])
def test_bits_below_the_shift_change_nothing(name):
    from centerclip_amd.preprocess import yuv_to_rgb
    shift = R.FORMATS[name][4]
    planes = _planes(name, 3, 12, 20, seed=5)
    g = np.random.RandomState(6)
    low = tuple(g.randint(1, 1 << shift, p.shape) for p in planes)   # nonzero everywhere
    clean, dirty = R.pack(*planes, name), R.pack(*planes, name, low)
    assert np.array_equal(clean >> shift, dirty >> shift) and int(((clean ^ dirty) != 0).sum()) == clean.size
    lay = R.layout(name, 12, 20, "bt709", False)
    want = R.planes_to_rgb(*planes, name, "bt709", False)
    for words in (clean, dirty):
        assert np.array_equal(OPS.yuv_to_rgb(torch.from_numpy(words).to(DEV), 3, 12, 20, lay, False).cpu().numpy(), want)
    # the decoder's array form through the Python entry: [..., 3H/2, W] uint16
    x = torch.from_numpy(dirty).view(1, 3, 18, 20).to(DEV)
    assert np.array_equal(yuv_to_rgb(x, name, "bt709").view(3, 12, 20, 3).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ the per-size fused entries
@pytest.mark.parametrize("kind", FUSED)
def test_resize_crop_equals_the_rgb_op_on_the_converted_frames(kind):
    from centerclip_amd.preprocess import YuvFrameTransform, resize_center_crop
    F = 3
    for H, W, n_px, resize in CASES:
        matrix, full = ("bt709", True) if resize else ("bt601", False)
        src, lay = _source(kind, F, H, W, 7, matrix, full)
        want = resize_center_crop(OPS.yuv_to_rgb(src, F, H, W, lay, False), n_px, resize)
        got = OPS.resize_center_crop_yuv(src, F, H, W, lay, n_px, resize, False)
        assert got.shape == (F, n_px, n_px, 3) and torch.equal(got, want), (H, W, n_px, resize)
        assert torch.equal(OPS.resize_center_crop_yuv(src, F, H, W, lay, n_px, resize, True), want.permute(0, 3, 1, 2))
        out = torch.full((F, n_px, n_px, 3), 0xFF, dtype=torch.uint8, device=DEV)
        OPS.resize_center_crop_yuv_out(src, F, H, W, lay, n_px, resize, False, out)
        assert torch.equal(out, want)
        if kind in R.FORMATS and H % 2 == 0:                        # the decoder's array form
            t = YuvFrameTransform(n_px, resize=resize, layout=kind, matrix=matrix, full_range=full)
            x = src.view(1, 1, F, R.frame_rows(kind, H), W)
            assert t.output_shape(x.shape) == (1, 1, F, n_px, n_px, 3) and torch.equal(t(x).view(want.shape), want)


@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "bicubic"])
def test_crop_flip_equals_the_rgb_op_on_the_converted_frames(interp, kind):
    """Two boxes for frames in clips of two - a downscale and a flipped odd-sized box - then per frame: the whole frame flipped,
    an n_px x n_px box (a byte copy of the conversion), and a box that leaves the frame (zeros)."""
    from centerclip_amd.preprocess import YuvTrainFrameTransform
    for H, W, n_px in ((13, 21, 8), (36, 52, 16)):
        F = 4
        src, lay = _source(kind, F, H, W, 3, "bt709", False)
        rgb = OPS.yuv_to_rgb(src, F, H, W, lay, False)
        two = torch.tensor([[2, 3, 10, 17, 0], [4, 6, 5, 3, 1]], dtype=torch.int32, device=DEV)
        got = OPS.resized_crop_flip_yuv(src, F, H, W, lay, two, n_px, 2, interp, False)
        assert torch.equal(got, OPS.resized_crop_flip(rgb, two, n_px, 2, interp)), (H, W)
        assert torch.equal(OPS.resized_crop_flip_yuv(src, F, H, W, lay, two, n_px, 2, interp, True), got.permute(0, 3, 1, 2))
        each = torch.tensor([[0, 0, H, W, 1], [1, 5, n_px, n_px, 0], [5, 2, n_px, n_px, 1], [6, 10, H - 5, W - 9, 0]],
                            dtype=torch.int32, device=DEV)
        out = torch.full((F, n_px, n_px, 3), 0xFF, dtype=torch.uint8, device=DEV)
        OPS.resized_crop_flip_yuv_out(src, F, H, W, lay, each, n_px, 1, interp, False, out)
        assert torch.equal(out, OPS.resized_crop_flip(rgb, each, n_px, 1, interp))
        assert torch.equal(out[1], rgb[1, 1:1 + n_px, 5:5 + n_px]) and torch.equal(out[2], rgb[2, 5:5 + n_px, 2:2 + n_px].flip(1))
        assert int(out[3].max()) == 0 and int(out[:3].max()) > 0
    if kind in R.FORMATS:                                           # the transform on the decoder's array form draws the RGB boxes
        from centerclip_amd.preprocess import TrainFrameTransform, yuv_to_rgb
        src, lay = _source(kind, 4, 36, 52, 3)
        x = src.view(2, 1, 2, R.frame_rows(kind, 36), 52)
        kw = dict(crop="random_resized", scale=(0.3, 1.0), flip=True, seed=11, interpolation=("bilinear", "bicubic")[interp])
        assert torch.equal(YuvTrainFrameTransform(16, layout=kind, **kw)(x), TrainFrameTransform(16, **kw)(yuv_to_rgb(x, kind)))


def test_general_entries_at_i420_and_nv12_equal_the_yuv420_entries():
    from centerclip_amd import preprocess as P
    F, H, W, n_px = 3, 13, 21, 8
    boxes = torch.tensor([[2, 3, 10, 17, 0], [0, 0, 13, 21, 1], [4, 6, 5, 3, 1]], dtype=torch.int32, device=DEV)
    for name in ("i420", "nv12"):
        src, lay = _source(name, F, H, W, 9, "bt709", True)
        old = Y8.layout(name, H, W, "bt709", True)
        assert lay[:6] + lay[10:] == old
        assert torch.equal(OPS.yuv_to_rgb(src, F, H, W, lay, False), OPS.yuv420_to_rgb(src, F, H, W, old, False))
        for resize in (True, False):
            assert torch.equal(OPS.resize_center_crop_yuv(src, F, H, W, lay, n_px, resize, False),
                               OPS.resize_center_crop_yuv420(src, F, H, W, old, n_px, resize, False))
        for interp in (0, 1):
            assert torch.equal(OPS.resized_crop_flip_yuv(src, F, H, W, lay, boxes, n_px, 1, interp, False),
                               OPS.resized_crop_flip_yuv420(src, F, H, W, old, boxes, n_px, 1, interp, False))
        # the ragged forms on the same tables
        clips = [torch.from_numpy(R.pack(*_planes(name, t, h, w, 20 + i), name)).view(t, h * 3 // 2, w)
                 for i, (t, h, w) in enumerate(RAGGED["p010"])]
        packed = P.pack_yuv_clips(clips, name).to(DEV)
        seen = {}

        class Spy(P.YuvClipCollate):
            def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
                seen["eval"] = (packed.data, rows_dev, plans_dev, clips)
                return P.YuvClipCollate._eval_op(self, packed, rows_dev, plans_dev, clips, out)

            def _train_op(self, packed, rows_dev, clips, out):
                seen["train"] = (packed.data, rows_dev, clips)
                return P.YuvClipCollate._train_op(self, packed, rows_dev, clips, out)
        got = Spy(n_px, max_frames=3, layout=name)(packed)
        data, rows, plans, table = seen["eval"]
        assert torch.equal(got.view(9, n_px, n_px, 3), OPS.collate_clips_yuv420(data, rows, plans, table, n_px, True, P.T.YUV_KINDS[name], 0,
                                                                                False, False))
        train = P.TrainFrameTransform(n_px, crop="random_resized", scale=(0.3, 1.0), flip=True, seed=5)
        got = Spy(n_px, max_frames=3, train=train, layout=name)(packed)
        data, rows, table = seen["train"]
        assert torch.equal(got.view(9, n_px, n_px, 3), OPS.collate_clips_crop_flip_yuv420(data, rows, table, n_px, P.T.YUV_KINDS[name], 0,
                                                                                          False, False))


# ------------------------------------------------------------------------------------------ ragged batches
RAGGED = {"p010": ((1, 12, 20), (3, 16, 16), (2, 10, 14)),           # (t, H, W); max_frames = 3
          "i444": ((1, 12, 20), (3, 13, 21), (2, 9, 15))}            # (4:4:4 has no subsampled axis: odd sizes pack too)
INDEX = [[0, -1, -1], [2, -1, 0], [1, 0, -1]]                        # one slot index of -1 inside clip 1's frames


def _ragged(name):
    return [torch.from_numpy(R.pack(*_planes(name, t, H, W, 20 + i), name)).view(t, R.frame_rows(name, H), W)
            for i, (t, H, W) in enumerate(RAGGED[name])]


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


@pytest.mark.parametrize("name", ["p010", "i444"])
def test_ragged_forms_equal_a_loop_of_per_clip_transforms(name):
    """Three clips of different sizes, an index with -1 slots: the whole batch against the per-clip transforms, for the
    evaluation form (resize on and off) and the training form (both interpolations); launches counted from a captured graph."""
    from centerclip_amd import preprocess as P
    n_px = 8
    clips = _ragged(name)
    packed = P.pack_yuv_clips(clips, name)
    frame = [R.layout(name, H, W)[0] for _, H, W in RAGGED[name]]
    assert packed.table.tolist() == [[0, 1] + list(RAGGED[name][0][1:]), [frame[0], 3] + list(RAGGED[name][1][1:]),
                                     [frame[0] + 3 * frame[1], 2] + list(RAGGED[name][2][1:])]
    packed = packed.to(DEV)
    dev = [c.to(DEV) for c in clips]
    with pytest.raises(ValueError, match="packed as"):
        P.YuvClipCollate(n_px, max_frames=3, layout="i422")(packed)
    seen = {}

    class Spy(P.YuvClipCollate):
        def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
            seen["eval"] = (packed.data, rows_dev, plans_dev, clips)
            return P.YuvClipCollate._eval_op(self, packed, rows_dev, plans_dev, clips, out)

        def _train_op(self, packed, rows_dev, clips, out):
            seen["train"] = (packed.data, rows_dev, clips)
            return P.YuvClipCollate._train_op(self, packed, rows_dev, clips, out)

    def loop(per_clip):
        want = torch.zeros(3, 1, 3, n_px, n_px, 3, dtype=torch.uint8, device=DEV)
        for b, row in enumerate(INDEX):
            frames = per_clip(b)
            for s, i in enumerate(row):
                if i >= 0:
                    want[b, 0, s] = frames[i]
        return want
    for resize in (True, False):
        collate = Spy(n_px, max_frames=3, resize=resize, layout=name, matrix="bt709")
        single = P.YuvFrameTransform(n_px, resize=resize, layout=name, matrix="bt709")
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        assert collate(packed, index=INDEX, out=out) is out
        assert torch.equal(out, loop(lambda b: single(dev[b]))), resize
        assert torch.equal(collate(packed, index=INDEX), out) and int(out[1, 0, 1].max()) == 0 and int(out[1, 0, 2].max()) > 0
    collate = Spy(n_px, max_frames=3, resize=True, layout=name)      # both passes run for every size here
    collate(packed, index=INDEX)
    data, rows, plans, table = seen["eval"]
    buf = torch.empty(9, n_px, n_px, 3, dtype=torch.uint8, device=DEV)
    assert _launches(lambda: OPS.collate_clips_yuv_out(data, rows, plans, table, n_px, True, R.FORMATS[name][0], 0, False, False,
                                                       buf)) == 2
    for interp in ("bilinear", "bicubic"):
        kw = dict(crop="random_resized", scale=(0.3, 1.0), flip=True, interpolation=interp)
        collate = Spy(n_px, max_frames=3, train=P.TrainFrameTransform(n_px, seed=5, **kw), layout=name)
        single = P.YuvTrainFrameTransform(n_px, layout=name, **kw)
        boxes = collate.sample(packed)
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        assert collate.apply(packed, boxes, index=INDEX, out=out) is out
        assert torch.equal(out, loop(lambda b: single.apply(dev[b], boxes[b:b + 1]))), interp
    data, rows, table = seen["train"]
    assert _launches(lambda: OPS.collate_clips_crop_flip_yuv_out(data, rows, table, n_px, R.FORMATS[name][0], 0, False, False,
                                                                 buf)) == 1
    assert torch.equal(buf, out.view(9, n_px, n_px, 3))
    # a row whose frame leaves the buffer, and (16-bit samples) one at an odd byte offset: zero frames, nothing else changes
    bad = rows.clone()
    bad[0, 1] = data.numel() - 100
    if R.FORMATS[name][3] > 8:
        bad[3, 1] += 1
    got = OPS.collate_clips_crop_flip_yuv(data, bad, table, n_px, R.FORMATS[name][0], 0, False, False)
    want = out.view(9, n_px, n_px, 3).clone()
    want[0] = 0
    if R.FORMATS[name][3] > 8:
        assert int(want[3].max()) > 0
        want[3] = 0
    assert torch.equal(got, want)


def test_per_size_entries_are_at_most_two_and_one_launch():
    F, H, W, n_px = 3, 36, 52, 16
    src, lay = _source("p010", F, H, W, 7)
    buf = torch.empty(F, n_px, n_px, 3, dtype=torch.uint8, device=DEV)
    assert _launches(lambda: OPS.resize_center_crop_yuv_out(src, F, H, W, lay, n_px, True, False, buf)) == 2
    assert _launches(lambda: OPS.resize_center_crop_yuv_out(src, F, H, W, lay, n_px, False, False, buf)) == 1
    boxes = torch.tensor([[2, 3, 20, 17, 1]], dtype=torch.int32, device=DEV)
    assert _launches(lambda: OPS.resized_crop_flip_yuv_out(src, F, H, W, lay, boxes, n_px, F, 1, False, buf)) == 1


# ------------------------------------------------------------------------------------------ through the product's loop
def _golden():
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    return g, sd, int(g["cfg"][10]), int(g["cfg"][11]), int(g["video"].shape[-1])


def _cfg(T):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                     sim_header='meanP', linear_patch='2d')


RAW = (80, 100)           # decoded frames of the loop test: 80 x 100 -> 64 x 80 -> the tiny model's 64 x 64


def _smooth_planes(F, H, W, seed):
    """10-bit frames with structure (random samples give near-grey noise after the resize): ramps + a little noise"""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.stack([(yy * (f + 2) * 4 + xx * 13 + g.randint(0, 96, (H, W))) % 1024 for f in range(F)])
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    u = np.stack([(cx * 21 + f * 125 + g.randint(0, 32, cy.shape)) % 1024 for f in range(F)])
    v = np.stack([(cy * 29 + f * 67 + g.randint(0, 32, cy.shape)) % 1024 for f in range(F)])
    return y, u, v


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


def test_eval_epoch_fed_p010_frames():
    """eval_epoch on uint16 P010 batches + YuvFrameTransform gives the metrics and, bit for bit, the similarity matrix of the RGB
    transform on yuv_to_rgb of the same frames."""
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.preprocess import FrameTransform, YuvFrameTransform, yuv_to_rgb
    g, sd, B, T, res = _golden()
    model = CLIP4Clip.from_state_dict(dict(sd), _cfg(T)).float().to(DEV)
    ids = torch.from_numpy(g["t_ids"])[:B]
    yuv, rgb = [], []
    for k in range(2):
        words = R.pack(*_smooth_planes(B * T, RAW[0], RAW[1], 40 + k), "p010")
        x = torch.from_numpy(words).view(B, 1, T, RAW[0] * 3 // 2, RAW[1])
        assert x.dtype == torch.uint16
        idk = ids.roll(k, 0)
        head = (idk, (idk > 0).long(), torch.zeros_like(idk))
        mask = torch.ones(B, 1, T, dtype=torch.long)
        yuv.append(head + (x, mask))
        rgb.append(head + (yuv_to_rgb(x.to(DEV), "p010", "bt709").cpu(), mask))
    want = _evaluate(model, rgb, frame_transform=FrameTransform(res), in_flight=1)
    got = _evaluate(model, yuv, frame_transform=YuvFrameTransform(res, layout="p010", matrix="bt709"), in_flight=1)
    assert want[0].shape == (2 * B, 2 * B) and bool(torch.isfinite(want[0]).all())
    assert float(want[0].std()) > 0                                 # (the frames are told apart: not a constant matrix)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    for attr in ("_eval_graphs", "_eval_lanes"):
        if hasattr(model, attr):
            delattr(model, attr)
    gc.collect()
