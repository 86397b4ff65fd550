"""Windows of long videos without a GPU: ``search.window_table`` (the host builder that keeps the device table valid), the
fake kernel and the argument checks of ``video_window_pool_planes`` / ``cc_video_window_pool_planes_f32`` (they end before
anything is read or launched, so never-dereferenced pointers do), the refusals of ``FeatureGallery.add_windows`` /
``add_window_features`` that need no device, and the bookkeeping of the window records on CPU stand-in rows."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from centerclip_amd.search import FeatureGallery, window_table

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = -1, -2


def _rows(table):
    return [tuple(r) for r in table.tolist()]


# ------------------------------------------------------------------------------------------------ 1. window_table
def test_window_table_worked_cases():
    t = window_table([12], 2, 4, 2)
    assert t.dtype == np.int64 and t.shape == (5, 3)
    assert _rows(t) == [(0, 0, 2), (0, 1, 3), (0, 2, 4), (0, 3, 5), (0, 4, 6)]
    # 7 frames of 2: three whole segments; scale 4: starts 0 and the tail 1; scale 8: the video is shorter: (0, 3)
    assert _rows(window_table([7], 2, [4, 8], 4)) == [(0, 0, 2), (0, 1, 3), (0, 0, 3)]
    t = window_table([3, 8], 2, [4, 8], 4)
    assert _rows(t[t[:, 0] == 0]) == [(0, 0, 1)]                           # both scales give (0, 1): it appears once
    one = _rows(t[t[:, 0] == 1])
    assert one[:2] == [(1, 0, 2), (1, 2, 4)]
    assert one[2:] == [(1, 0, 4)]                                          # n_i <= w at scale 8: the single window (0, n_i)
    assert _rows(window_table(torch.tensor([12]), 2, 4, 2)) == _rows(window_table([12], 2, 4, 2))
    assert _rows(window_table(np.array([12]), 2, (4,), (2,))) == _rows(window_table([12], 2, 4, 2))
    assert window_table([], 2, 4).shape == (0, 3)


def test_window_table_default_strides_and_the_tail_window():
    # half the window, in whole segments: 8 frames of 2 -> 4 segments -> stride 2 segments
    assert _rows(window_table([20], 2, 8)) == [(0, 0, 4), (0, 2, 6), (0, 4, 8), (0, 6, 10)]
    # 6 frames of 2 -> 3 segments -> half is 1.5 -> 1 segment
    assert _rows(window_table([12], 2, 6)) == [(0, 0, 3), (0, 1, 4), (0, 2, 5), (0, 3, 6)]
    # one segment per window: half rounds to 0 -> at least one segment
    assert _rows(window_table([6], 2, 2)) == [(0, 0, 1), (0, 1, 2), (0, 2, 3)]
    # a stride per scale
    assert _rows(window_table([12], 2, [4, 8], [4, 2])) == [(0, 0, 2), (0, 2, 4), (0, 4, 6), (0, 0, 4), (0, 1, 5), (0, 2, 6)]
    # tail: 7 segments, window 3, stride 3: starts 0, 3 and one more at 4; 9 segments: 0, 3, 6 and no tail
    assert _rows(window_table([7], 1, 3, 3)) == [(0, 0, 3), (0, 3, 6), (0, 4, 7)]
    assert _rows(window_table([9], 1, 3, 3)) == [(0, 0, 3), (0, 3, 6), (0, 6, 9)]
    # a partial last segment is dropped: 13 frames of 2 are the 6 segments of 12
    assert _rows(window_table([13], 2, 4, 2)) == _rows(window_table([12], 2, 4, 2))
    # the order: video, scale as given, start
    t = window_table([12, 12], 2, [8, 4], 4)
    assert _rows(t) == [(0, 0, 4), (0, 2, 6), (0, 0, 2), (0, 2, 4), (0, 4, 6), (1, 0, 4), (1, 2, 6), (1, 0, 2), (1, 2, 4), (1, 4, 6)]


def test_window_table_refusals():
    with pytest.raises(ValueError, match="video 1"):
        window_table([4, 1], 2, 4)                                         # n_i == 0
    with pytest.raises(ValueError, match="video 0"):
        window_table([0], 1, 1)
    with pytest.raises(ValueError, match="video 2"):
        window_table([8, 8, 10], 2, 4, segments=4)                         # n_i > segments
    assert window_table([8, 8, 9], 2, 4, segments=4).shape[0] == 9
    for kw in (dict(window=3), dict(window=[4, 5]), dict(window=4, stride=3), dict(window=[4, 8], stride=[2, 3]),
               dict(window=0), dict(window=-4), dict(window=4, stride=0), dict(window=[]), dict(window=4.0)):
        with pytest.raises(ValueError):
            window_table([12], 2, **kw)                                    # not positive multiples of fd
    with pytest.raises(ValueError):
        window_table([12], 2, [4, 8], [2, 2, 2])                           # one stride per scale
    with pytest.raises(ValueError, match="synchronise"):
        window_table(torch.empty(2, dtype=torch.int64, device="meta"), 2, 4)
    with pytest.raises(ValueError):
        window_table(torch.tensor([12], dtype=torch.int32), 2, 4)
    with pytest.raises(ValueError):
        window_table([12.5], 2, 4)


def test_window_table_rows_lie_inside_and_cover_every_segment():
    rng = np.random.default_rng(3)
    for _ in range(200):
        fd = int(rng.integers(1, 5))
        lengths = rng.integers(fd, 40 * fd, size=int(rng.integers(1, 5)))
        ws = [int(w) * fd for w in rng.integers(1, 12, size=int(rng.integers(1, 4)))]
        # (a stride beyond its window skips segments by construction: coverage is a property of strides up to the window)
        stride = None if rng.random() < 0.4 else [int(rng.integers(1, w // fd + 1)) * fd for w in ws]
        t = window_table(lengths.tolist(), fd, ws, stride)
        assert t.dtype == np.int64 and t.ndim == 2 and t.shape[1] == 3
        assert (np.diff(t[:, 0]) >= 0).all()
        for i, length in enumerate(lengths.tolist()):
            n = length // fd
            mine = t[t[:, 0] == i][:, 1:]
            assert len(mine) and (mine[:, 0] >= 0).all() and (mine[:, 1] <= n).all() and (mine[:, 0] < mine[:, 1]).all()
            assert len({tuple(r) for r in mine.tolist()}) == len(mine)                     # a pair appears once
            for w in ws:                                                                   # every scale covers every segment
                size = min(w // fd, n)
                covered = np.zeros(n, dtype=bool)
                for a, b in mine[(mine[:, 1] - mine[:, 0]) == size].tolist():
                    covered[a:b] = True
                assert covered.all(), (lengths, fd, ws, stride, i, w)


# ------------------------------------------------------------------------------------------------ 2. the op and the C entry
def test_fake_kernel_gives_shapes_on_the_meta_device():
    assert "video_window_pool_planes" in torch_ops.OPS
    visual = torch.empty(3, 20, 512, device="meta")
    table = torch.empty(7, 3, device="meta", dtype=torch.int32)
    planes = torch.ops.centerclip.video_window_pool_planes(visual, table)
    assert planes.shape == (7, 3 * 512) and planes.dtype == torch.float16 and planes.device.type == "meta"
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        torch.ops.centerclip.video_window_pool_planes(torch.zeros(1, 2, 64), torch.zeros(1, 3, dtype=torch.int32))


def _call(lib, visual=256, windows=256, Bv=2, S=5, nW=3, E=64, planes=256):
    p = lambda v: ctypes.c_void_p(v) if v else None                       # (addresses that are never dereferenced)
    return lib.cc_video_window_pool_planes_f32(p(visual), p(windows), Bv, S, nW, E, p(planes), None)


def test_entry_refuses_before_touching_memory():
    from centerclip_amd import build
    build.build(verbose=False)
    lib = L.lib()
    assert _call(lib, visual=0) == INVALID
    assert _call(lib, windows=0) == INVALID
    assert _call(lib, planes=0) == INVALID
    assert _call(lib, E=96) == INVALID
    assert _call(lib, E=1088) == UNSUPPORTED
    assert _call(lib, nW=0) == INVALID
    assert _call(lib, nW=-2) == INVALID
    assert _call(lib, Bv=0) == INVALID and _call(lib, S=0) == INVALID and _call(lib, E=0) == INVALID


# ------------------------------------------------------------------------------------------------ 3. FeatureGallery without a device
def _cpu_model(**extra):
    """tests/test_search_host.py::_cpu_model"""
    from centerclip_amd.clip4clip import CLIP4Clip
    g2 = np.load(os.path.join(HERE, "golden", "r2_golden.npz"))
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    T = int(g2["s1_cfg"][11])
    kw = dict(cluster_inter=0, deep_cluster=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T, T, T],
              cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
              minkowski_norm_p=2.0, aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True,
              sim_header='meanP', linear_patch='2d', pre_visual_pooling=0)
    kw.update(extra)
    return CLIP4Clip.from_state_dict(sd, Namespace(**kw)).eval(), T


def _cpu_gallery(model, side="video", E=64, grouped=False):
    """a gallery as its constructor leaves it, minus the device (tests/test_search_host.py)"""
    import centerclip_amd.search as S
    gal = FeatureGallery.__new__(FeatureGallery)
    gal.model = gal.core = model
    gal.side, gal.products, gal.E, gal._n = side, 2, E, 0
    gal.device = torch.device("cpu")
    gal.backend = S.HipBackend
    gal._rows = torch.zeros(0, 3 * E, dtype=torch.float16)
    if grouped:
        gal.grouped = True
        gal._head = torch.zeros(0, dtype=torch.int32)
        gal._label_dev = torch.full((1,), -1, dtype=torch.int64)
        gal._reset_groups()
    return gal


def test_gallery_refusals_that_need_no_device():
    model, T = _cpu_model()
    video = torch.zeros(1, 1, 2 * T, 3, 8, 8)
    text = _cpu_gallery(model, side="text")
    with pytest.raises(ValueError, match="side"):
        text.add_windows(video, [2 * T], T)
    with pytest.raises(ValueError, match="side"):
        text.add_window_features(torch.zeros(1, 2 * T, 64), [2 * T], T)
    with pytest.raises(ValueError, match="shift"):
        _cpu_gallery(_cpu_model(cluster_algo='token_shift')[0]).add_windows(video, [2 * T], T)
    with pytest.raises(ValueError, match="shift"):
        _cpu_gallery(_cpu_model(cluster_algo='temporal_shift')[0]).add_windows(video, [2 * T], T)
    with pytest.raises(ValueError, match="linear_patch"):
        _cpu_gallery(_cpu_model(linear_patch='3d')[0]).add_windows(video, [2 * T], T)
    gal = _cpu_gallery(model)
    with pytest.raises(ValueError, match="multiple"):
        gal.add_windows(torch.zeros(1, 1, 2 * T + 1, 3, 8, 8), [2 * T], T)                 # F % T != 0
    with pytest.raises(ValueError, match="longer"):
        gal.add_windows(video, [2 * T + 1], T)                                             # lengths[i] > F
    with pytest.raises(ValueError, match="group="):
        gal.add_windows(video, [2 * T], T, group=3)                                        # a plain gallery refuses group=
    with pytest.raises(ValueError):
        gal.add_windows(video, [2 * T, T], T)                                              # one length per video
    with pytest.raises(ValueError):
        gal.add_windows(video, torch.empty(1, dtype=torch.int64, device="meta"), T)
    # nothing above encoded anything; a valid call on CPU tensors stops at the device check, as add does
    with pytest.raises(L.CenterClipHipError):
        gal.add_windows(video, [2 * T], T)
    with pytest.raises(L.CenterClipHipError):
        gal.add_window_features(torch.zeros(1, 2 * T, 64), [2 * T], T)
    assert len(gal) == 0 and gal.span == 0


def _stand_in(n, E=64, seed=0):
    return torch.randn(n, 3 * E, generator=torch.Generator().manual_seed(seed)).to(torch.float16)


def test_window_records_follow_their_rows():
    model, _ = _cpu_model()
    gal = _cpu_gallery(model)
    assert "windows" not in gal.state_dict()
    gal._append(_stand_in(2, seed=1))                                                      # rows of add: no record
    assert gal.windows([0, 1]).tolist() == [[-1, -1], [-1, -1]] and "windows" not in gal.state_dict()
    frames = np.array([[0, 4], [2, 6], [4, 8]])
    pos = gal._append_windows(_stand_in(3, seed=2), frames)
    assert pos.tolist() == [2, 3, 4]
    gal._append(_stand_in(1, seed=3))                                                      # and a plain row behind them
    want = [[-1, -1], [-1, -1], [0, 4], [2, 6], [4, 8], [-1, -1]]
    w = gal.windows(torch.arange(6))
    assert w.dtype == torch.int64 and w.tolist() == want
    assert gal.windows(3).tolist() == [[2, 6]] and gal.windows([4, 0]).tolist() == [[4, 8], [-1, -1]]
    with pytest.raises(ValueError):
        gal.windows([6])
    gal.remove([0, 3])                                                                     # the records survive remove
    assert gal.windows(torch.arange(6)).tolist() == want
    state = gal.state_dict()
    assert state["windows"].tolist() == want and state["live"].tolist() == [False, True, True, False, True, True]
    other = _cpu_gallery(model)
    other._append_windows(_stand_in(1, seed=9), np.array([[7, 9]]))
    other.load_state_dict(state)
    assert torch.equal(other.rows, gal.rows) and other.windows(torch.arange(6)).tolist() == want and len(other) == 4
    with pytest.raises(ValueError):
        other.load_state_dict(dict(state, windows=state["windows"][:3]))
    new_pos = gal.compact()                                                                # renumbered with their rows
    assert new_pos.tolist() == [-1, 0, 1, -1, 2, 3]
    assert gal.windows(torch.arange(4)).tolist() == [[-1, -1], [0, 4], [4, 8], [-1, -1]]
    assert torch.equal(gal.rows, other.rows[[1, 2, 4, 5]])
    gal.clear()
    assert gal.span == 0 and "windows" not in gal.state_dict()
    gal._append(_stand_in(1))
    assert gal.windows([0]).tolist() == [[-1, -1]]
    # a state without the key drops the records of the gallery it is loaded into
    other.load_state_dict(gal.state_dict())
    assert other.windows([0]).tolist() == [[-1, -1]] and "windows" not in other.state_dict()


def test_window_groups_are_labelled_per_video():
    model, _ = _cpu_model()
    gal = _cpu_gallery(model, grouped=True)
    table = window_table([8, 4], 1, 4, 2)
    assert gal._window_groups(7, table, 2, "add_windows") == 7
    assert gal._window_groups([5, 9], table, 2, "add_windows").tolist() == [5, 5, 5, 9]
    assert gal._window_groups(torch.tensor([5, 9]), table, 2, "add_windows").tolist() == [5, 5, 5, 9]
    with pytest.raises(ValueError, match="per video"):
        gal._window_groups([5, 5, 5, 9], table, 2, "add_windows")                          # one label per video, not per row
    with pytest.raises(ValueError):
        gal._window_groups(None, table, 2, "add_windows")                                  # a grouped gallery wants group=
    with pytest.raises(ValueError):
        gal._window_groups(torch.empty(2, dtype=torch.int64, device="meta"), table, 2, "add_windows")
    gal._append_windows(_stand_in(4), table[:, 1:], gal._window_groups([5, 9], table, 2, "add_windows"))
    assert gal.labels.tolist() == [5, 5, 5, 9] and gal.num_groups == 2
    assert gal.windows(torch.arange(4)).tolist() == [[0, 4], [2, 6], [4, 8], [0, 4]]
