"""Windows of long videos on the MI355X (``-m gpu``): ``video_window_pool_planes`` against the op it shares its device code
with, ``FeatureGallery.add_window_features`` / ``add_windows`` against a second gallery filled window by window, on the small
model of tests/golden/r2_golden.npz (E = 64, T = 4 frames, 2 frames per final segment when it clusters).

Exactness: wherever both sides run the same arithmetic on the same features the rows are compared bit for bit.  Where the
encoder (or the seqTransf head) sees another batch - the window across a chunk boundary, the head on windows batched by
length - the dequantised rows (hi + lo) / 1024 are held to 1e-3, the README's parity bound on embeddings; the measured
maxima are printed and recorded in DESIGN.md §7."""
import io
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd.search import FeatureGallery, window_table
from oracle.recipes import dyadic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
op = torch.ops.centerclip


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _dequant(rows):
    """video-side planes [n, 3E] (hi | lo | hi) -> the rows they stand for, float64"""
    E = rows.shape[1] // 3
    return (rows[:, :E].double() + rows[:, E:2 * E].double()) / 1024.0


def _ones(n, s):
    return torch.ones(n, s, dtype=torch.long, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel
#  (Bv, S), lengths, window, stride -> nW = 1, 5 and 39 = 4 * 9 + 3 (the tail of the four-waves-per-workgroup grid)
TABLES = [((1, 1), [1], 1, None, 1), ((3, 5), [2, 5, 3], 3, None, 5), ((2, 37), [37, 30], [4, 16], None, 39)]


@pytest.mark.parametrize("E", [64, 512, 1024])
@pytest.mark.parametrize("shape,lengths,window,stride,nW", TABLES)
def test_window_pool_is_the_pooling_op_on_every_window(E, shape, lengths, window, stride, nW):
    Bv, S = shape
    table = window_table(lengths, 1, window, stride, segments=S)
    assert table.shape[0] == nW and (nW in (1, 5) or nW % 4 == 3)
    g = torch.Generator().manual_seed(1000 * E + S)
    visual = (torch.randn(Bv, S, E, generator=g) * (0.25 + 4 * torch.rand(Bv, S, 1, generator=g))).to(DEV)
    rows = op.video_window_pool_planes(visual, torch.from_numpy(table.astype(np.int32)).to(DEV))
    assert rows.shape == (nW, 3 * E) and rows.dtype == torch.float16
    want = torch.cat([op.video_pool_normalize_planes(visual[v:v + 1, a:b].contiguous(), _ones(1, b - a))
                      for v, a, b in table.tolist()])
    assert _bits(rows, want)
    # independently: float64 normalise - mean - normalise of the same slice; the row is a unit vector along it
    got = _dequant(rows).cpu()
    worst = 0.0
    for w, (v, a, b) in enumerate(table.tolist()):
        x = visual[v, a:b].double().cpu()
        mean = (x / x.norm(dim=-1, keepdim=True)).mean(0)
        worst = max(worst, abs(float(got[w] @ (mean / mean.norm())) - 1.0))
    print("window pool E=%d nW=%d: |row . float64 unit - 1| max %.3g" % (E, nW, worst))
    assert worst <= 5e-6


# ------------------------------------------------------------------------------------------------ the small model
@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(HERE, "golden", "r2_golden.npz"))


def _state(g2):
    return {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
            for k in g2.files if k.startswith("s1_sd/")}


def _eval_model(g2, cluster_inter, sd=None, **extra):
    """tests/test_search_gpu.py::_eval_model"""
    from centerclip_amd.clip4clip import CLIP4Clip
    cfg = g2["s1_cfg"]
    Tf, T_new = int(cfg[11]), int(cfg[12])
    kw = dict(cluster_inter=cluster_inter, deep_cluster=0, cluster_algo='kmediods++', max_frames=Tf,
              target_frames_blocks=[4, T_new, T_new] if cluster_inter else [Tf, Tf, Tf], cluster_num_blocks=[16, 6, 6],
              cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100, minkowski_norm_p=2.0,
              aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True, sim_header='meanP',
              linear_patch='2d', pre_visual_pooling=0)
    kw.update(extra)
    return CLIP4Clip.from_state_dict(_state(g2) if sd is None else sd, Namespace(**kw)).to(DEV).eval()


@pytest.fixture(scope="module")
def clustered(g2):
    return _eval_model(g2, 1)


@pytest.fixture(scope="module")
def unclustered(g2):
    return _eval_model(g2, 0)


def _features(b, S, E, seed):
    return torch.randn(b, S, E, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _fill_by_window(gal, visual, table, fd, group=None):
    """the gallery the windows are held against: every window as a clip of its own, through add_features"""
    for i, (v, a, b) in enumerate(table.tolist()):
        a, b = a // fd, b // fd
        gal.add_features(visual[v:v + 1, a:b], _ones(1, b - a), group=None if group is None else int(group[i]))


# ------------------------------------------------------------------------------------------------ 2. add_window_features
def test_add_window_features_rows_plain(clustered):
    fd = clustered.f_frame_duration
    assert fd == 2
    visual = _features(3, 10, 64, seed=11)
    lengths = [20, 15, 9]                                                  # 10, 7 and 4 whole segments
    gal, ref = FeatureGallery(clustered, capacity=2), FeatureGallery(clustered)
    pos, windows = gal.add_window_features(visual, lengths, [4 * fd, 6 * fd])
    assert windows.dtype == torch.int64 and windows.device.type == "cpu"
    assert np.array_equal(windows.numpy(), window_table(lengths, fd, [4 * fd, 6 * fd]) * np.array([1, fd, fd]))
    assert torch.equal(pos, torch.arange(windows.shape[0])) and gal.span == len(gal) == windows.shape[0]
    _fill_by_window(ref, visual, windows, fd)
    assert _bits(gal.rows, ref.rows)
    assert torch.equal(gal.windows(pos), windows[:, 1:])
    more, w2 = gal.add_window_features(visual[:1], torch.tensor([20]), 10 * fd, stride=fd)     # a second call: positions go on
    assert more.tolist() == [gal.span - 1] and w2.tolist() == [[0, 0, 20]]
    plain = gal.add_features(visual[:1], _ones(1, 10))
    assert _bits(gal.rows[more], gal.rows[plain])                          # the whole video as a window = the clip
    assert gal.windows(plain).tolist() == [[-1, -1]]
    with pytest.raises(ValueError):
        gal.add_window_features(visual, lengths, 4 * fd, group=1)          # a plain gallery refuses group=
    with pytest.raises(ValueError):
        gal.add_window_features(visual, [22, 15, 9], 4 * fd)               # more valid segments than features


def test_add_window_features_rows_grouped(clustered):
    fd = clustered.f_frame_duration
    visual = _features(3, 9, 64, seed=12)
    lengths, labels = [18, 11, 7], [40, 7, 19]
    gal, ref = FeatureGallery(clustered, grouped=True), FeatureGallery(clustered, grouped=True)
    span = gal.span
    with pytest.raises(ValueError):
        gal.add_window_features(visual, lengths, 4 * fd)                   # a grouped gallery wants group=
    with pytest.raises(ValueError):
        gal.add_window_features(visual, lengths, 4 * fd, group=[40, 7, 40])             # a label returns
    assert gal.span == span == 0
    pos, windows = gal.add_window_features(visual, lengths, 4 * fd, stride=fd, group=labels)
    per_row = np.asarray(labels)[windows[:, 0].numpy()]
    _fill_by_window(ref, visual, windows, fd, group=per_row)
    assert _bits(gal.rows, ref.rows)
    assert np.array_equal(gal.labels.numpy(), per_row) and torch.equal(gal.labels, ref.labels)
    assert gal.num_groups == 3 and torch.equal(gal.windows(pos), windows[:, 1:])
    q = _features(4, 1, 64, seed=13)
    a, b = gal.search_groups_features(q, k=3), ref.search_groups_features(q, k=3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    one, w1 = gal.add_window_features(visual[:1], [18], 4 * fd, group=5)   # one int for the call
    assert gal.labels[one].tolist() == [5] * w1.shape[0] and gal.num_groups == 4


def test_add_window_features_rows_dual_softmax(clustered):
    fd = clustered.f_frame_duration
    visual = _features(2, 8, 64, seed=14)
    bank, q = _features(9, 1, 64, seed=15), _features(3, 1, 64, seed=16)
    gal, ref = FeatureGallery(clustered, dual_softmax=True), FeatureGallery(clustered, dual_softmax=True)
    gal.set_query_bank_features(bank)
    ref.set_query_bank_features(bank)
    pos, windows = gal.add_window_features(visual, [16, 10], [2 * fd, 6 * fd])
    _fill_by_window(ref, visual, windows, fd)
    assert _bits(gal.rows, ref.rows)
    a, b = gal.search_features(q, k=5), ref.search_features(q, k=5)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 3. localisation
def test_search_groups_finds_the_video_and_the_window(g2):
    sd = _state(g2)
    g = torch.Generator().manual_seed(21)
    sd["text_projection"] = torch.randn(128, 512, generator=g) * 0.05
    sd["visual.proj"] = torch.randn(sd["visual.proj"].shape[0], 512, generator=g) * 0.05
    model = _eval_model(g2, 1, sd=sd)
    fd = model.f_frame_duration
    gal = FeatureGallery(model, grouped=True)
    assert gal.E == 512 and fd == 2
    visual = torch.randn(4, 12, 512, generator=g)
    visual = visual / visual.norm(dim=-1, keepdim=True)
    q = torch.randn(512, generator=g)
    q = q / q.norm()
    visual[2, 4:6] = q
    pos, windows = gal.add_window_features(visual.to(DEV), [12 * fd] * 4, 2 * fd, stride=fd, group=[10, 11, 12, 13])
    assert windows.shape[0] == 4 * 11
    scores, labels, best = gal.search_groups_features(q.view(1, 1, 512).to(DEV), k=1)
    assert labels.tolist() == [[12]]
    assert gal.windows(best.cpu().reshape(-1)).tolist() == [[4 * fd, 6 * fd]]
    assert windows[int(best)].tolist() == [2, 4 * fd, 6 * fd]
    mult = math.exp(model._logit_scale_value())
    assert abs(float(scores) / mult - 1.0) <= 1e-3
    # its half-overlapping neighbours stand near mult * 0.71: no tie to resolve
    s2, p2 = gal.search_features(q.view(1, 1, 512).to(DEV), k=3)
    assert int(p2[0, 0]) == int(best) and float(s2[0, 1]) / mult < 0.8


# ------------------------------------------------------------------------------------------------ 4./5. end to end
def _long_video(g2, b, chunks, seed):
    cfg = g2["s1_cfg"]
    RES, Tf = int(cfg[1]), int(cfg[11])
    return torch.from_numpy(dyadic(seed, (b, 1, chunks * Tf, 3, RES, RES)) * np.float32(1.5)).to(DEV), Tf


def test_add_windows_of_whole_clips_is_add(g2, clustered):
    video, Tf = _long_video(g2, 1, 3, seed=31)
    gal, ref = FeatureGallery(clustered), FeatureGallery(clustered)
    pos, windows = gal.add_windows(video, [3 * Tf], Tf, stride=Tf, encode_batch=3)
    assert windows.tolist() == [[0, 0, Tf], [0, Tf, 2 * Tf], [0, 2 * Tf, 3 * Tf]] and pos.tolist() == [0, 1, 2]
    ref.add(video.reshape((3, 1, Tf) + tuple(video.shape[3:])), torch.ones(3, 1, Tf, dtype=torch.long, device=DEV))
    assert _bits(gal.rows, ref.rows)                                       # one encode of the same shape, the same pooling
    assert not clustered.training
    # two videos, the second shorter, in encode batches of 4 + 2: positions, labels and records line up
    video2, _ = _long_video(g2, 2, 3, seed=32)
    grouped = FeatureGallery(clustered, grouped=True)
    pos, windows = grouped.add_windows(video2, torch.tensor([3 * Tf, 2 * Tf + 1]), [Tf, 2 * Tf], group=[3, 4], encode_batch=4)
    fd = clustered.f_frame_duration
    assert np.array_equal(windows.numpy(), window_table([3 * Tf, 2 * Tf + 1], fd, [Tf, 2 * Tf]) * np.array([1, fd, fd]))
    assert grouped.labels.tolist() == [3 + int(v) for v in windows[:, 0]] and torch.equal(grouped.windows(pos), windows[:, 1:])
    clips = video2.reshape((6, 1, Tf) + tuple(video2.shape[3:]))           # the same encodes by hand: clips 0..3, then 4..5
    with torch.no_grad():
        parts = [clustered(video=c, video_mask=torch.ones(c.shape[0], Tf, dtype=torch.long, device=DEV))['visual_output']
                 for c in (clips[:4], clips[4:])]
    by_hand = FeatureGallery(clustered)
    by_hand.add_window_features(torch.cat(parts).reshape(2, 3 * Tf // fd, -1), [3 * Tf, 2 * Tf + 1], [Tf, 2 * Tf])
    assert _bits(grouped.rows, by_hand.rows)
    span = gal.span
    with pytest.raises(ValueError):
        gal.add_windows(video[:, :, :Tf + 1], [Tf], Tf)                    # F % T
    with pytest.raises(ValueError):
        gal.add_windows(video, [3 * Tf + 1], Tf)                           # longer than the frames given
    assert gal.span == span


def test_add_windows_across_a_chunk_boundary(g2, unclustered):
    video, Tf = _long_video(g2, 1, 2, seed=33)
    assert Tf % 2 == 0 and unclustered.f_frame_duration == 1
    gal, ref = FeatureGallery(unclustered), FeatureGallery(unclustered)
    pos, windows = gal.add_windows(video, [2 * Tf], Tf, stride=Tf // 2)
    assert windows[1].tolist() == [0, Tf // 2, 3 * Tf // 2]
    ref.add(video[:, :, Tf // 2:3 * Tf // 2].contiguous(), torch.ones(1, 1, Tf, dtype=torch.long, device=DEV))
    err = float((_dequant(gal.rows[1:2]) - _dequant(ref.rows)).abs().max())
    print("add_windows: the window [T/2, 3T/2) against the clip cut out of the frames, dequantised rows differ by at most %.3g"
          % err)
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------ 6. seqTransf
def test_add_window_features_runs_the_seqtransf_head_per_window(g2):
    sd = _state(g2)
    g = torch.Generator().manual_seed(5)
    sd["text_projection"] = torch.randn(128, 128, generator=g) * 0.05
    sd["visual.proj"] = torch.randn(sd["visual.proj"].shape[0], 128, generator=g) * 0.05
    model = _eval_model(g2, 0, sd=sd, sim_header='seqTransf', cross_num_hidden_layers=2)
    table_rows = model.frame_position_embeddings.num_embeddings
    visual = torch.randn(2, 7, 128, generator=g).to(DEV)
    gal, ref = FeatureGallery(model), FeatureGallery(model)
    pos, windows = gal.add_window_features(visual, [7, 5], [2, 4], stride=[1, 2])
    assert sorted(set((windows[:, 2] - windows[:, 1]).tolist())) == [2, 4]
    _fill_by_window(ref, visual, windows, 1)
    err = float((_dequant(gal.rows) - _dequant(ref.rows)).abs().max())
    print("seqTransf: windows batched by length against one head call per window, dequantised rows differ by at most %.3g" % err)
    assert err <= 1e-3
    plain = torch.cat([op.video_pool_normalize_planes(visual[v:v + 1, a:b].contiguous(), _ones(1, b - a))
                       for v, a, b in windows.tolist()])
    assert not _bits(gal.rows, plain)                                      # the head ran
    long = torch.randn(1, table_rows + 1, 128, generator=g).to(DEV)
    span = gal.span
    with pytest.raises(ValueError, match="position table"):
        gal.add_window_features(long, [table_rows + 1], [2, table_rows + 1])
    assert gal.span == span and len(gal) == span


# ------------------------------------------------------------------------------------------------ 7. persistence
def test_window_records_persist_and_compact(clustered):
    fd = clustered.f_frame_duration
    visual = _features(2, 8, 64, seed=41)
    gal = FeatureGallery(clustered)
    first = gal.add_features(visual[:, :2], _ones(2, 2))
    pos, windows = gal.add_window_features(visual, [16, 11], 4 * fd)
    assert "windows" in gal.state_dict() and "windows" not in FeatureGallery(clustered).state_dict()
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    fresh = FeatureGallery(clustered)
    fresh.load_state_dict(torch.load(buf))
    everything = torch.arange(gal.span)
    assert fresh.span == gal.span and _bits(fresh.rows, gal.rows)
    assert torch.equal(fresh.windows(everything), gal.windows(everything))
    assert fresh.windows(first).tolist() == [[-1, -1]] * 2 and torch.equal(fresh.windows(pos), windows[:, 1:])
    before_rows, before = fresh.rows.clone(), fresh.windows(everything)
    gone = [0, int(pos[1]), int(pos[-1])]
    fresh.remove(gone)
    assert torch.equal(fresh.windows(everything), before)
    new_pos = fresh.compact()
    keep = torch.tensor([p for p in range(gal.span) if p not in gone])
    assert new_pos[keep].tolist() == list(range(len(keep))) and fresh.span == len(keep)
    assert _bits(fresh.rows, before_rows[keep.to(DEV)]) and torch.equal(fresh.windows(torch.arange(len(keep))), before[keep])
    fresh.clear()
    assert fresh.span == 0 and "windows" not in fresh.state_dict()
