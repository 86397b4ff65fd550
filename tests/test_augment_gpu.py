"""The train-time augmentation on a real MI355X (``-m gpu``): cc_resized_crop_flip_u8 / torch.ops.centerclip.resized_crop_flip /
preprocess.TrainFrameTransform against the float64 restatement (tests/augment_ref.py, anchored to torch's interpolate in
tests/test_augment_host.py), then through train_epoch and DeviceFeeder.

The rule for resampled bytes: a byte equals clamp(rint(v)) of the float64 value v wherever v is farther than delta from a
half-integer, and may differ by one inside that band.  delta is the bound on the kernel's own fp32 error, derived operation
by operation in tests/augment_ref.py (DELTA): 2e-4 of a level for bilinear, 1.5e-3 for bicubic.  Identity boxes, layouts and the
loops are byte (bit) equality."""
import functools
import gc
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))

# (H, W, n_px) -> boxes (top, left, h, w): borders (clamped bicubic taps), distortion, upscaling, the whole frame
CASES = {(45, 60, 32): [(0, 0, 45, 45), (1, 3, 39, 33), (16, 27, 29, 33), (0, 0, 45, 60)],
         (37, 53, 32): [(0, 0, 37, 37), (1, 3, 32, 27), (13, 26, 24, 27), (0, 0, 37, 53)],
         (240, 320, 224): [(1, 3, 210, 180), (82, 140, 158, 180)]}
FRAMES = 2                                                   # per clip in the comparisons against float64
BAND_SHARE = 0.03


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    _frames.cache_clear()
    _values.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _frames(F, H, W):
    x = np.random.default_rng(0).integers(0, 256, (F, 3, H, W), np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _values(F, H, W, box, n_px, interp, flip):
    """The float64 values of one clip; computed once, shared, never written."""
    v = AR.resized_crop_flip(_frames(F, H, W), box, n_px, interp, flip)
    v.setflags(write=False)
    return v


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(len(rows), 5)


def _op(x_chw, rows, n_px, fpc, interp):
    """NumPy [F, 3, H, W] through the op -> NumPy [F, 3, n_px, n_px]"""
    from centerclip_amd import torch_ops  # noqa: F401  (registers torch.ops.centerclip.*)
    y = torch.ops.centerclip.resized_crop_flip(torch.from_numpy(np.array(x_chw)).to(DEV), _table(rows), n_px, fpc, interp)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "bicubic"])
@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "%dx%d_to_%d" % c)
def test_bytes_against_float64(case, interp):
    """Every box of the case, without and with flip, as the clips of ONE launch on the same frames."""
    H, W, n_px = case
    rows = [box + (flip,) for box in CASES[case] for flip in (0, 1)]
    x = _frames(FRAMES, H, W)
    got = _op(np.concatenate([x] * len(rows)), rows, n_px, FRAMES, interp)
    assert got.shape == (len(rows) * FRAMES, 3, n_px, n_px) and got.dtype == np.uint8
    v = np.concatenate([_values(FRAMES, H, W, r[:4], n_px, interp, bool(r[4])) for r in rows])
    share, differing = AR.check_bytes(got, v, AR.DELTA[interp])
    print("\n%dx%d -> %d interp %d: %.3f %% of the pixels within %.1e of a half-integer, %d of %d bytes differ there"
          % (H, W, n_px, interp, 100 * share, AR.DELTA[interp], differing, got.size))
    assert AR.DELTA[interp] <= 1e-2 and share <= BAND_SHARE


@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "bicubic"])
def test_identity_boxes_are_the_slice(interp):
    for (H, W, n_px) in ((45, 60, 32), (240, 320, 224)):
        x = _frames(FRAMES, H, W)
        got = _op(np.concatenate([x, x]), [(2, 5, n_px, n_px, 0), (2, 5, n_px, n_px, 1)], n_px, FRAMES, interp)
        want = x[:, :, 2:2 + n_px, 5:5 + n_px]
        assert np.array_equal(got[:FRAMES], want) and np.array_equal(got[FRAMES:], want[..., ::-1]), (H, W, interp)


ROWS2 = [(1, 3, 39, 33, 1), (16, 27, 29, 33, 0)]             # two clips: another box and another flip bit each


@functools.lru_cache(maxsize=None)
def _two_clips(interp):
    """-> (frames [6, 3, 45, 60], the kernel's bytes [6, 3, 32, 32] as the CHW 4-D op gives them, checked against float64)"""
    x = _frames(6, 45, 60)
    got = _op(x, ROWS2, 32, 3, interp)
    v = np.concatenate([AR.resized_crop_flip(x[3 * i:3 * i + 3], r[:4], 32, interp, bool(r[4])) for i, r in enumerate(ROWS2)])
    AR.check_bytes(got, v, AR.DELTA[interp])
    assert not np.array_equal(got[:3], got[3:])
    got.setflags(write=False)
    return x, got


@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "bicubic"])
def test_layouts_forms_out_and_odd_addresses(interp):
    """Two clips of three frames: HWC and CHW, 4-D with frames_per_clip = 3 and the loaders' 6-D video, out=, and a source that
    starts at an odd byte address - all the same bytes."""
    from centerclip_amd.preprocess import TrainFrameTransform
    x, want = _two_clips(interp)
    t = TrainFrameTransform(32, interpolation=interp)
    boxes = _table(ROWS2)
    chw = torch.from_numpy(x.copy()).to(DEV)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    want_t = torch.from_numpy(want.copy())
    want_hwc = want_t.permute(0, 2, 3, 1)
    assert torch.equal(t.apply(chw, boxes, frames_per_clip=3).cpu(), want_t)
    assert torch.equal(t.apply(hwc, boxes, frames_per_clip=3).cpu(), want_hwc)
    assert torch.equal(t.apply(hwc, boxes.cpu(), frames_per_clip=3).cpu(), want_hwc)                  # a host table is uploaded
    y6 = t.apply(hwc.view(2, 1, 3, 45, 60, 3), boxes)
    assert y6.shape == (2, 1, 3, 32, 32, 3) and torch.equal(y6.cpu().view(6, 32, 32, 3), want_hwc)
    y6 = t.apply(chw.view(2, 1, 3, 3, 45, 60), boxes)
    assert y6.shape == (2, 1, 3, 3, 32, 32) and torch.equal(y6.cpu().view(6, 3, 32, 32), want_t)
    out = torch.full((2, 1, 3, 32, 32, 3), 0xA5, dtype=torch.uint8, device=DEV)
    assert t.apply(hwc.view(2, 1, 3, 45, 60, 3), boxes, out=out) is out and torch.equal(out.cpu().view(6, 32, 32, 3), want_hwc)
    with pytest.raises(ValueError):
        t.apply(hwc, boxes, out=out[0], frames_per_clip=3)
    for src in (hwc, chw):
        buf = torch.empty(src.numel() + 1, dtype=torch.uint8, device=DEV)
        view = buf[1:].view(src.shape)
        view.copy_(src)
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        assert torch.equal(t.apply(view, boxes, frames_per_clip=3), t.apply(src, boxes, frames_per_clip=3))
    # one 4-D clip by default, and a short last clip: frames 0-3 and 4-5
    assert torch.equal(t.apply(chw, boxes[:1]).cpu()[:3], want_t[:3])
    y = t.apply(chw, boxes, frames_per_clip=4).cpu()
    assert torch.equal(y[:3], want_t[:3]) and torch.equal(y[4:], want_t[4:])


def test_a_table_row_outside_the_frame_gives_zeros_for_its_clip():
    """The kernel checks the row and never forms an address from it; the other clip is untouched by its neighbour's row."""
    x, want = _two_clips(1)
    big = 2 ** 31 - 1
    bad_rows = [(-1, 3, 39, 33, 0), (1, -3, 39, 33, 0), (1, 3, 0, 33, 0), (1, 3, 39, 0, 1), (1, 3, -39, 33, 0), (7, 3, 39, 33, 0),
                (1, 28, 39, 33, 0), (1, 3, 46, 33, 0), (big, big, big, big, 1), (-big - 1, 0, 1, 1, 0), (0, 0, big, 1, 0),
                (big, 0, 1, 1, 0), (0, big, 1, 1, 0)]
    rows = [r for bad in bad_rows for r in (bad, ROWS2[1])]               # clips: bad, good, bad, good, ...
    src = np.concatenate([x] * len(bad_rows))
    got = _op(src, rows, 32, 3, 1).reshape(len(bad_rows), 2, 3, 3, 32, 32)
    assert not got[:, 0].any()
    assert all(np.array_equal(g, want[3:]) for g in got[:, 1])
    # the box that just fits is followed: the last row and column of the frame
    edge = _op(x[:3], [(6, 27, 39, 33, 0)], 32, 3, 1)
    AR.check_bytes(edge, AR.resized_crop_flip(x[:3], (6, 27, 39, 33), 32, 1), AR.DELTA[1])
    assert edge.any()


def test_captured_call_follows_the_table_at_replay():
    """The op reads the device table itself: a captured call replays on new frames AND new boxes written into the same buffers."""
    from centerclip_amd.preprocess import TrainFrameTransform
    x, want = _two_clips(0)
    t = TrainFrameTransform(32, interpolation="bilinear")
    static = torch.from_numpy(x.copy()).to(DEV)
    boxes = _table([ROWS2[1], ROWS2[0]])
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        eager = t.apply(static, boxes, frames_per_clip=3).clone()
    stream.synchronize()
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        y = t.apply(static, boxes, frames_per_clip=3)
    boxes.copy_(_table(ROWS2))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.from_numpy(want.copy())) and not torch.equal(y, eager)
    del graph


# ------------------------------------------------------------------------------------------ through the product's loops
RAW = (45, 60)


def _golden():
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    return g, sd, int(g["cfg"][10]), int(g["cfg"][11]), int(g["video"].shape[-1])


def _cfg(T):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                     sim_header='meanP', linear_patch='2d')


def _raw_batches(n):
    """n loader batches of the tiny model with raw uint8 video [B, 1, T, 45, 60, 3]"""
    g, _, B, T, _ = _golden()
    ids = torch.from_numpy(g["t_ids"])[:B]
    out = []
    for k in range(n):
        video = torch.from_numpy(np.random.default_rng(10 + k).integers(0, 256, (B, 1, T, RAW[0], RAW[1], 3), np.uint8))
        idk = ids.roll(k, 0)
        out.append((idk, (idk > 0).long(), torch.zeros_like(idk), video, torch.ones(B, 1, T, dtype=torch.long)))
    return out


def test_train_epoch_with_the_augmenting_transform():
    """train_epoch(frame_transform=TrainFrameTransform(res, seed=3, flip=True)) on raw 45 x 60 uint8 batches: the losses and the
    parameters, bit for bit, of train_epoch without a transform on batches augmented beforehand by a second object with the
    same seed (sample, then apply).  res is the tiny model's own resolution (64: its positional embedding has 4 x 4 + 1 rows),
    so the crops are enlarged."""
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.preprocess import TrainFrameTransform
    from centerclip_amd.train import AdamW, prep_optim_params_groups, train_epoch
    _, sd, B, T, res = _golden()
    raw = _raw_batches(2)
    aug, aug2 = TrainFrameTransform(res, seed=3, flip=True), TrainFrameTransform(res, seed=3, flip=True)
    cooked, tables = [], []
    for b in raw:
        tables.append(aug2.sample(B, *RAW))
        y = aug.apply(b[3].to(DEV), tables[-1])
        assert y.shape == (B, 1, T, res, res, 3) and y.dtype == torch.uint8
        cooked.append(b[:3] + (y.cpu(),) + b[4:])
    assert len({tuple(r) for t_ in tables for r in t_.tolist()}) > 1               # (the clips did get different boxes)
    args = Namespace(optim="AdamW", lr=1e-3, wd=0.2, new_added_modules=["ln_final", "text_projection"],
                     gradient_accumulation_steps=1, clip_grad_norm=1.0)
    runs = []
    for batches, kw in ((cooked, {}), (raw, dict(frame_transform=TrainFrameTransform(res, seed=3, flip=True)))):
        m = CLIP4Clip.from_state_dict(dict(sd), _cfg(T)).float().to(DEV)
        o = AdamW(prep_optim_params_groups(args, m, coef_lr=0.5), lr=args.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=args.wd)
        losses = []
        mean, gs = train_epoch(0, args, m, batches, DEV, o, 0, log=lambda e, s, loss, sim, g_: losses.append(loss), **kw)
        torch.cuda.synchronize()
        assert gs == 2 and len(losses) == 2 and np.isfinite(losses).all()
        runs.append((losses, mean, {n: p.detach().clone() for n, p in m.named_parameters()}))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], (runs[0][0], runs[1][0])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n


def test_device_feeder_yields_the_bytes_of_the_direct_call():
    from centerclip_amd.feeder import DeviceFeeder
    from centerclip_amd.preprocess import TrainFrameTransform
    _, _, B, T, res = _golden()
    raw = _raw_batches(3)
    host = [tuple(t.pin_memory() for t in b) for b in raw]                        # 3 batches over 2 slots
    kw = dict(crop="random_resized", seed=5, flip=True)
    direct = TrainFrameTransform(res, **kw)
    want = [direct(b[3].to(DEV)).cpu() for b in raw]
    feeder = DeviceFeeder(DEV, depth=2, frame_transform=TrainFrameTransform(res, **kw))
    addresses, got = {}, []
    for slot, tensors in feeder(host):
        assert len(tensors) == 5 and tensors[3].shape == (B, 1, T, res, res, 3) and tensors[3].dtype == torch.uint8
        addresses.setdefault(slot, set()).add(tensors[3].data_ptr())
        got.append(tensors[3].clone())
    torch.cuda.synchronize()
    assert sorted(addresses) == [0, 1] and all(len(v) == 1 for v in addresses.values())
    assert len(got) == 3 and all(torch.equal(g_.cpu(), w_) for g_, w_ in zip(got, want))
    assert not torch.equal(want[0], want[1])
