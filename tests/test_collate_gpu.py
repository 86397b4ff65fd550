"""Ragged clip batches on a real MI355X (``-m gpu``): preprocess.ClipCollate / torch.ops.centerclip.collate_clips[_crop_flip]
against the per-clip ops they must equal byte for byte (resize_center_crop, resized_crop_flip) and the NumPy restatement of
Pillow's resize (tests/resize_ref.py), then through DeviceFeeder and eval_epoch.  n_px = 32, T = 4, random bytes as frames;
every comparison is torch.equal.  (eval_epoch runs the tiny model of tests/golden/clip_golden.npz, whose resolution is 64 and
whose T is 4: that one test collates to 64 px.)"""
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
N_PX, T = 32, 4

# (t, H, W): two passes; the copy path with two zero slots; neither axis resampled, crop only; an odd size - the next clip
# starts at an odd byte; a long clip that is sampled; an index with a repeat, a step back and a zero slot
EVAL = [(4, 40, 56), (2, 32, 32), (4, 64, 32), (1, 33, 47), (9, 96, 50), (3, 50, 96)]
CROP = [(4, 32, 43), (2, 32, 57), (3, 48, 32), (1, 40, 40)]


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    for f in (_clips, _want_eval, _index):
        f.cache_clear()
    gc.collect()                          # (no dead cycle's hipGraph may be destroyed inside a later test's capture)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _clips(sizes, chw, seed=0):
    """-> host uint8 tensors [t, H, W, 3] ([t, 3, H, W] with chw) of random bytes; computed once, shared, never written"""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randint(0, 256, (t, H, W, 3), dtype=torch.uint8, generator=g) for t, H, W in sizes]
    return tuple(c.permute(0, 3, 1, 2).contiguous() if chw else c for c in out)


@functools.lru_cache(maxsize=None)
def _index(sizes):
    from centerclip_amd.sampling import uniform_sampling
    rows = [[s if s < t else -1 for s in range(T)] for t, _, _ in sizes]
    if sizes == tuple(EVAL):
        rows[4] = uniform_sampling(T, 9).tolist()
        rows[5] = [2, 2, 0, -1]
    return np.array(rows, dtype=np.int64)


def _per_clip(clips, index, chw, op):
    """-> host [B, 1, T, ...]: op(clip b's frames index[b] on the device, b) per clip, zeros where the index is -1"""
    shape = (3, N_PX, N_PX) if chw else (N_PX, N_PX, 3)
    want = torch.zeros((len(clips), 1, T) + shape, dtype=torch.uint8)
    for b, c in enumerate(clips):
        slots = [s for s in range(T) if index[b, s] >= 0]
        got = op(c[[int(index[b, s]) for s in slots]].to(DEV), b)
        want[b, 0, slots] = got.cpu()
    return want


@functools.lru_cache(maxsize=None)
def _want_eval(sizes, chw, resize):
    from centerclip_amd.preprocess import resize_center_crop
    want = _per_clip(_clips(sizes, chw), _index(sizes), chw, lambda x, b: resize_center_crop(x, N_PX, resize))
    torch.cuda.synchronize()
    return want


def _packed(sizes, chw):
    from centerclip_amd.preprocess import pack_clips
    return pack_clips(list(_clips(sizes, chw)))


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("resize", [True, False], ids=["resize", "crop"])
def test_evaluation_form_equals_the_per_clip_op(resize, chw):
    from centerclip_amd.preprocess import ClipCollate
    sizes = tuple(EVAL if resize else CROP)
    packed, index, want = _packed(sizes, chw), _index(sizes), _want_eval(sizes, chw, resize)
    if resize:
        assert int(packed.table[4, 0]) % 2 == 1                   # the clip behind the 33 x 47 one starts at an odd byte
    collate = ClipCollate(N_PX, max_frames=T, resize=resize)
    dev = packed.to(DEV)
    out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
    assert collate(dev, index=index, out=out) is out
    assert torch.equal(out.cpu(), want)
    zero = torch.from_numpy(index < 0)
    assert bool(zero.any()) and int(out.cpu()[:, 0][zero].max()) == 0          # every zero slot of the 0xFF buffer came back zero
    fresh = collate(dev, index=index)
    assert fresh.shape == out.shape and torch.equal(fresh, out)
    if resize:                                                    # ... and the restatement of Pillow's arithmetic says the same
        hwc = _clips(sizes, False)
        for b in (0, 4):
            ref = R.resize_center_crop(hwc[b][index[b]].numpy(), N_PX, True)
            got = out[b, 0].permute(0, 2, 3, 1) if chw else out[b, 0]
            assert np.array_equal(got.cpu().numpy(), ref), b
    if not resize and not chw:                                    # the default index is the zero padding of short clips
        assert torch.equal(collate(dev), out)


def test_pack_clips_of_device_tensors():
    """Clips that already are on the device (one of them a non-contiguous view) pack into the same bytes and table."""
    from centerclip_amd.preprocess import ClipCollate, pack_clips
    sizes = tuple(EVAL)
    host = _packed(sizes, False)
    clips = [c.to(DEV) for c in _clips(sizes, False)]
    clips[3] = _clips(sizes, True)[3].to(DEV).permute(0, 2, 3, 1)             # [1, 33, 47, 3] as a view of [1, 3, 33, 47]
    dev = pack_clips(clips)
    assert dev.is_cuda and not dev.table.is_cuda and torch.equal(dev.table, host.table) and torch.equal(dev.data.cpu(), host.data)
    assert torch.equal(ClipCollate(N_PX, max_frames=T)(dev, index=_index(sizes)).cpu(), _want_eval(sizes, False, True))


def test_refused_sizes_raise_before_anything_is_launched():
    """A frame smaller than the crop (32 x 24 with the crop alone; the resize would scale it up) and the smallest size over 65
    taps per axis at n_px = 32 (513 x 513: 67; a 32 x 2048 clip is NOT refused - its short side already is n_px, so it is only
    cropped): ValueError naming the clip, `out` untouched."""
    from centerclip_amd import _lib as L
    from centerclip_amd.preprocess import ClipCollate, pack_clips, resize_center_crop
    g = torch.Generator().manual_seed(3)
    mk = lambda t, H, W: torch.randint(0, 256, (t, H, W, 3), dtype=torch.uint8, generator=g)
    for resize, bad, name in ((False, (1, 32, 24), "clip 2"), (True, (1, 513, 513), "clip 2")):
        with pytest.raises(L.CenterClipHipError):
            resize_center_crop(mk(*bad).to(DEV), N_PX, resize)    # the per-clip op refuses this size
        packed = pack_clips([mk(2, 40, 56), mk(4, 32, 32), mk(*bad)]).to(DEV)
        collate = ClipCollate(N_PX, max_frames=T, resize=resize)
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match=name):
            collate(packed, out=out)
        torch.cuda.synchronize()
        assert int(out.min()) == 0xFF
    wide = pack_clips([mk(1, 32, 2048)]).to(DEV)
    assert torch.equal(ClipCollate(N_PX, max_frames=T)(wide)[0, 0, 0], resize_center_crop(wide.clip(0), N_PX, True)[0])


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("crop", ["multiscale", "random_resized"])
def test_training_form_equals_the_per_clip_op(crop, chw):
    from centerclip_amd.preprocess import ClipCollate, TrainFrameTransform
    sizes = tuple(EVAL)
    packed, index, clips = _packed(sizes, chw), _index(sizes), _clips(sizes, chw)
    collate = ClipCollate(N_PX, max_frames=T, train=TrainFrameTransform(N_PX, crop=crop, flip=True, seed=11))
    twin = TrainFrameTransform(N_PX, crop=crop, flip=True, seed=11)
    boxes = collate.sample(packed)
    want_boxes = torch.cat([twin.sample(1, H, W) for _, H, W in sizes], 0)
    assert boxes.dtype == torch.int32 and torch.equal(boxes, want_boxes) and len({tuple(b) for b in boxes.tolist()}) > 1
    want = _per_clip(clips, index, chw, lambda x, b: twin.apply(x, boxes[b:b + 1]))
    out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
    dev = packed.to(DEV)
    assert collate.apply(dev, boxes, index=index, out=out) is out
    assert torch.equal(out.cpu(), want)
    assert int(out.cpu()[:, 0][torch.from_numpy(index < 0)].max()) == 0
    # __call__ is sample + apply: the next draws of the same stream
    again = collate(dev, index=index)
    boxes2 = torch.cat([twin.sample(1, H, W) for _, H, W in sizes], 0)
    assert torch.equal(again.cpu(), _per_clip(clips, index, chw, lambda x, b: twin.apply(x, boxes2[b:b + 1])))
    with pytest.raises(ValueError, match="clip 1"):
        bad = boxes.clone()
        bad[1, 3] = 33                                            # wider than its 32 x 32 frame
        collate.apply(dev, bad, index=index)


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
def test_one_clip_and_more_frames_than_grid_planes(chw):
    """B = 1, and n_out = 4100 output frames over COLLATE_MAX_PLANES = 4096 planes of the grid's third dimension: the frames
    behind the last plane are folded onto the first ones.  32 x 32 frames, so both forms are copies."""
    from centerclip_amd import torch_ops as TO
    from centerclip_amd.preprocess import ClipCollate, TrainFrameTransform, pack_clips
    sizes = tuple(EVAL)
    one = pack_clips([_clips(sizes, chw)[0]]).to(DEV)
    assert torch.equal(ClipCollate(N_PX, max_frames=T)(one).cpu(), _want_eval(sizes, chw, True)[:1])
    B = TO.COLLATE_MAX_PLANES // T + 1
    assert B * T > TO.COLLATE_MAX_PLANES
    frames = torch.randint(0, 256, (B, T, N_PX, N_PX, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    if chw:
        frames = frames.permute(0, 1, 4, 2, 3).contiguous()
    packed = pack_clips(list(frames))
    index = np.tile(np.arange(T, dtype=np.int64), (B, 1))
    index[0], index[-1] = [1, -1, 0, 0], [3, 3, -1, 2]            # in the first planes and in the folded ones
    want = frames[torch.arange(B)[:, None], torch.from_numpy(np.maximum(index, 0))]
    want[torch.from_numpy(index < 0)] = 0
    dev = packed.to(DEV)
    for collate in (ClipCollate(N_PX, max_frames=T), ClipCollate(N_PX, max_frames=T, resize=False),
                    ClipCollate(N_PX, max_frames=T, train=TrainFrameTransform(N_PX, crop="center"))):
        out = torch.full(collate.output_shape(packed), 0xFF, dtype=torch.uint8, device=DEV)
        collate(dev, index=index, out=out)
        assert torch.equal(out.cpu()[:, 0], want)


def test_device_feeder_takes_ragged_batches_at_stable_addresses():
    from centerclip_amd.feeder import DeviceFeeder
    from centerclip_amd.preprocess import ClipCollate, pack_clips
    ev, cr = _clips(tuple(EVAL), False), _clips(tuple(CROP), False)
    batches = [[cr[3], ev[1], ev[3]], [ev[0], ev[2], cr[0]], [ev[5], ev[0], ev[2]], [ev[1], cr[3], ev[3]]]     # 3 clips each
    host = [(torch.arange(3) + k, pack_clips(b), pack_clips(b).video_mask(T)) for k, b in enumerate(batches)]
    sizes = [h[1].data.numel() for h in host]
    assert sizes[2] > sizes[0] and sizes[3] < sizes[1] and len(set(sizes)) >= 3            # slot 0 grows, slot 1 must not shrink
    collate = ClipCollate(N_PX, max_frames=T)
    want = [collate(h[1].to(DEV)).cpu() for h in host]
    feeder = DeviceFeeder(DEV, depth=2, frame_transform=ClipCollate(N_PX, max_frames=T))
    addresses, raw, got = {}, {}, []
    for slot, tensors in feeder(host):
        assert len(tensors) == 3 and tensors[1].shape == (3, 1, T, N_PX, N_PX, 3) and tensors[1].dtype == torch.uint8
        addresses.setdefault(slot, set()).add(tensors[1].data_ptr())
        raw.setdefault(slot, []).append(feeder.raw[slot].numel())
        got.append(tuple(t.clone() for t in tensors))
    torch.cuda.synchronize()
    assert sorted(addresses) == [0, 1] and all(len(v) == 1 for v in addresses.values())
    assert raw[0][1] >= sizes[2] > raw[0][0] and raw[1][1] == raw[1][0]
    for k, (g_, h) in enumerate(zip(got, host)):
        assert torch.equal(g_[0].cpu(), h[0]) and torch.equal(g_[1].cpu(), want[k]) and torch.equal(g_[2].cpu(), h[2])
    with pytest.raises(ValueError, match="ClipCollate"):
        next(iter(DeviceFeeder(DEV, depth=2)(host)))


# ------------------------------------------------------------------------------------------ through eval_epoch
def _golden():
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    return g, sd, int(g["cfg"][10]), int(g["cfg"][11]), int(g["video"].shape[-1])


def _cfg(frames):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=frames, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                     sim_header='meanP', linear_patch='2d')


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


def test_eval_epoch_takes_packed_clips():
    """A loader that yields PackedClips of mixed sizes and lengths + a ClipCollate gives what a loader that yields the collated
    uint8 tensor gives without a transform.  (Every clip keeps at least two real frames: with three zero frames of four this
    tiny model's similarity row is NaN on either path - a segment of the clustering then holds constant frames only.)"""
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.preprocess import ClipCollate, pack_clips
    g, sd, B, frames, res = _golden()
    assert (B, frames) == (2, T)
    model = CLIP4Clip.from_state_dict(dict(sd), _cfg(frames)).float().to(DEV)
    ids = torch.from_numpy(g["t_ids"])[:B]
    gen = torch.Generator().manual_seed(5)
    mk = lambda t, H, W: torch.randint(0, 256, (t, H, W, 3), dtype=torch.uint8, generator=gen)
    ragged = [[mk(4, 80, 100), mk(2, 64, 64)], [mk(3, 100, 70), mk(4, 64, 90)], [mk(3, 77, 65), mk(4, 90, 120)]]
    collate = ClipCollate(res, max_frames=frames)
    raw, cooked = [], []
    for k, clips in enumerate(ragged):
        idk = ids.roll(k, 0)
        packed = pack_clips(clips)
        head, mask = (idk, (idk > 0).long(), torch.zeros_like(idk)), packed.video_mask(frames).view(B, 1, frames)
        raw.append(head + (packed, mask))
        cooked.append(head + (collate(packed.to(DEV)).cpu(), mask))
    for kw in (dict(in_flight=1), dict(in_flight=2), dict(in_flight=1, graphed=True)):
        want = _evaluate(model, cooked, **kw)
        got = _evaluate(model, raw, frame_transform=ClipCollate(res, max_frames=frames), **kw)
        assert want[0].shape == (3 * B, 3 * B) and bool(torch.isfinite(want[0]).all())
        assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], kw
    for attr in ("_eval_graphs", "_eval_lanes"):
        if hasattr(model, attr):
            delattr(model, attr)
    gc.collect()
