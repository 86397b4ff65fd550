"""Ragged clip batches without a GPU: pack_clips / PackedClips, ClipCollate's index rules, the sampling helpers against the
reference's recorded indices (tests/golden/sampling_golden.npz, tools/gen_golden_sampling.py), the fake kernels of the new ops
and the header's new symbols."""
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_PX, T = 32, 4


def _clips(sizes, chw=False, seed=0):
    rng = np.random.RandomState(seed)
    out = [rng.randint(0, 256, (t, H, W, 3), dtype=np.uint8) for t, H, W in sizes]
    return [np.ascontiguousarray(c.transpose(0, 3, 1, 2)) for c in out] if chw else out


# ------------------------------------------------------------------------------------------ pack_clips
@pytest.mark.parametrize("chw", [False, True])
def test_pack_clips_is_back_to_back_with_the_right_table(chw):
    from centerclip_amd.preprocess import PackedClips, pack_clips
    sizes = [(4, 40, 56), (1, 33, 47), (2, 32, 32), (3, 5, 7)]
    clips = _clips(sizes, chw)
    p = pack_clips(clips[:2] + [torch.from_numpy(c) for c in clips[2:]])          # arrays and tensors alike
    assert isinstance(p, PackedClips) and len(p) == 4 and p.chw == chw
    assert p.data.dtype == torch.uint8 and p.data.dim() == 1 and p.table.dtype == torch.int64 and not p.table.is_cuda
    want, off = [], 0
    for t, H, W in sizes:
        want.append([off, t, H, W])
        off += t * H * W * 3
    assert p.table.tolist() == want and p.data.numel() == off
    assert want[2][0] % 2 == 1                                    # an odd size gives the next clip an odd byte offset: no padding
    for b, c in enumerate(clips):
        assert np.array_equal(p.data[want[b][0]:want[b][0] + c.size].numpy(), c.reshape(-1))
        assert np.array_equal(p.clip(b).numpy(), c)
    assert torch.equal(p[[3, 1]].clip(0), p.clip(3)) and p[[3, 1]].table.tolist() == [[0, 3, 5, 7], [315, 1, 33, 47]]
    assert pack_clips(clips, layout="chw" if chw else "hwc").table.tolist() == want


def _pack_second(batch):
    from centerclip_amd.preprocess import pack_clips
    return torch.stack([i for i, _ in batch]), pack_clips([c for _, c in batch])


def test_pack_clips_as_a_dataloader_collate_fn():
    from centerclip_amd.preprocess import pack_clips
    clips = _clips([(2, 8, 9), (1, 6, 5), (3, 4, 4)])
    items = [(torch.tensor([i]), torch.from_numpy(c)) for i, c in enumerate(clips)]
    loader = torch.utils.data.DataLoader(items, batch_size=2, collate_fn=lambda b: (torch.stack([i for i, _ in b]),
                                                                                     pack_clips([c for _, c in b])))
    got = list(loader)
    workers = list(torch.utils.data.DataLoader(items, batch_size=2, num_workers=1, collate_fn=_pack_second))
    assert [p.table.tolist() for _, p in workers] == [p.table.tolist() for _, p in got]
    assert all(torch.equal(a.data, b.data) and not a.data.is_pinned() for (_, a), (_, b) in zip(workers, got))
    assert [len(p) for _, p in got] == [2, 1] and got[0][1].table.tolist() == [[0, 2, 8, 9], [432, 1, 6, 5]]
    assert np.array_equal(got[1][1].clip(0).numpy(), clips[2])


def test_pack_clips_refuses_mixed_layouts_and_empty_clips():
    from centerclip_amd.preprocess import pack_clips
    hwc, chw = _clips([(2, 8, 9)])[0], _clips([(2, 8, 9)], chw=True)[0]
    with pytest.raises(ValueError, match="one layout per batch"):
        pack_clips([hwc, chw])
    with pytest.raises(ValueError, match="one layout per batch"):
        pack_clips([hwc, hwc], layout="chw")
    with pytest.raises(ValueError, match="empty"):
        pack_clips([hwc, np.zeros((0, 8, 9, 3), dtype=np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        pack_clips([hwc.astype(np.float32)])
    with pytest.raises(ValueError):
        pack_clips([])


def test_video_mask():
    from centerclip_amd.preprocess import pack_clips
    p = pack_clips(_clips([(2, 4, 4), (4, 4, 4), (9, 4, 4)]))                     # t < T, t = T, t > T
    m = p.video_mask(T)
    assert m.dtype == torch.int64 and m.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert p.video_mask(T, lengths=[1, 0, 3]).tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]
    with pytest.raises(ValueError):
        p.video_mask(T, lengths=[1, 5, 3])
    with pytest.raises(ValueError):
        p.video_mask(T, lengths=[1, 2])


# ------------------------------------------------------------------------------------------ ClipCollate's index
def test_index_default_and_validation():
    from centerclip_amd.preprocess import ClipCollate, pack_clips
    c = ClipCollate(N_PX, max_frames=T)
    p = pack_clips(_clips([(2, 40, 56), (4, 33, 47)]))
    assert c.index(p).tolist() == [[0, 1, -1, -1], [0, 1, 2, 3]]
    assert c.index(p, [[1, 1, 0, -1], [3, 2, 1, 0]]).tolist() == [[1, 1, 0, -1], [3, 2, 1, 0]]   # repeats, any order
    assert c.output_shape(p) == (2, 1, T, N_PX, N_PX, 3)
    with pytest.raises(ValueError, match=r"index\[0, 2\] = 2"):
        c.index(p, [[0, 1, 2, -1], [0, 1, 2, 3]])                  # >= t_b
    with pytest.raises(ValueError, match=r"index\[1, 0\] = -2"):
        c.index(p, [[0, 1, -1, -1], [-2, 1, 2, 3]])                # < -1
    with pytest.raises(ValueError, match="must be integers"):
        c.index(p, [[0, 1, -1], [0, 1, 2]])                        # wrong shape
    with pytest.raises(ValueError, match="must be integers"):
        c.index(p, np.zeros((2, T), dtype=np.float32))
    long = pack_clips(_clips([(2, 40, 56), (9, 33, 47)]))
    with pytest.raises(ValueError, match="clip 1 has 9 frames"):
        c.index(long)                                              # default index with t_b > T: the caller must sample
    from centerclip_amd.sampling import uniform_sampling
    assert c.index(long, [[0, 1, -1, -1], uniform_sampling(T, 9)]).tolist() == [[0, 1, -1, -1], [1, 3, 5, 7]]


def test_sizes_the_per_clip_op_refuses_name_the_clip():
    from centerclip_amd.preprocess import ClipCollate
    c = ClipCollate(N_PX, max_frames=T)
    with pytest.raises(ValueError, match="clip 3: 32 x 24"):
        ClipCollate(N_PX, max_frames=T, resize=False).plan(32, 24, clip=3)    # smaller than the crop (resize=True scales it up)
    assert c.plan(32, 24)[5:7].tolist() == [42, 32]
    with pytest.raises(ValueError, match="clip 0: 513 x 513"):
        c.plan(513, 513, clip=0)                                   # 67 taps
    assert c.plan(512, 512)[11] == 65 and c.plan(32, 2048)[11] == 0   # 65 taps are taken; a short side of n_px is not resized
    with pytest.raises(ValueError, match="TrainFrameTransform"):
        from centerclip_amd.preprocess import TrainFrameTransform
        ClipCollate(N_PX, train=TrainFrameTransform(64))


def test_table_upload_inside_a_capture_is_refused(monkeypatch):
    """A call's tables are uploaded, which cannot be captured: the call raises before anything touches the device."""
    from centerclip_amd import _lib
    from centerclip_amd.preprocess import ClipCollate
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.CenterClipHipError, match="capture"):
        ClipCollate(N_PX, max_frames=T)._upload(np.zeros(8, dtype=np.int64), "cuda:0")


# ------------------------------------------------------------------------------------------ sampling
CASES = ((12, 300), (12, 24), (12, 17), (12, 13), (12, 12), (12, 5), (12, 1), (4, 9))
DATA2 = ((4, 5), (4, 6))
DATA3 = ((4, 5),)         # three frames per offset, one frame more than the clip: the only way into the choice branch


def test_sampling_helpers_reproduce_the_reference():
    from centerclip_amd.sampling import multi_segments_sampling, uniform_sampling
    g = np.load(os.path.join(HERE, "golden", "sampling_golden.npz"))
    seen = 0
    for tag, cases, kw in (("", CASES, {}), ("2", DATA2, dict(data_length=2)), ("3", DATA3, dict(data_length=3))):
        for c, n in cases:
            for twice in (0, 1):
                got = uniform_sampling(c, n, twice_sample=bool(twice), **kw)
                assert np.array_equal(got, g["uniform%s/%d_%d_%d" % (tag, c, n, twice)]), (tag, c, n, twice)
                seen += 1
            for shift in (0, 1):
                for seed in range(5):
                    key = "segments%s/%d_%d_%d_%d" % (tag, c, n, shift, seed)
                    np.random.seed(seed)
                    assert np.array_equal(multi_segments_sampling(c, n, random_shift=bool(shift), **kw), g[key]), key
                    got = multi_segments_sampling(c, n, random_shift=bool(shift), rng=np.random.RandomState(seed), **kw)
                    assert np.array_equal(got, g[key]), key       # the same draws from a generator of the caller's
                    seen += 1
    assert seen == len(g.files) == 132
    # the choice branch did draw: four of five frames, sorted, and the seeds do not all agree
    drawn = {tuple(g["segments3/4_5_1_%d" % s]) for s in range(5)}
    assert len(drawn) > 1 and all(len(set(d)) == 4 and list(d) == sorted(d) and max(d) <= 4 for d in drawn)


# ------------------------------------------------------------------------------------------ ops and ABI
@pytest.mark.parametrize("chw", [False, True])
def test_fake_kernels_give_shapes_and_dtypes(chw):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import centerclip_amd.torch_ops as TO
    shape = (3, N_PX, N_PX) if chw else (N_PX, N_PX, 3)
    clips = [0, 2, 40, 56, 13440, 4, 33, 47]
    with FakeTensorMode():
        src = torch.empty(13440 + 4 * 33 * 47 * 3, dtype=torch.uint8)
        plans = torch.empty(100, dtype=torch.int32)
        rows = torch.empty(2 * T, TO.COLLATE_ROW, dtype=torch.int64)
        out = torch.ops.centerclip.collate_clips(src, rows, plans, clips, N_PX, True, chw)
        assert tuple(out.shape) == (2 * T,) + shape and out.dtype == torch.uint8
        buf = torch.empty((2, 1, T) + shape, dtype=torch.uint8)
        assert torch.ops.centerclip.collate_clips_out(src, rows, plans, clips, N_PX, True, chw, buf) is None
        boxes = torch.empty(2 * T, TO.COLLATE_BOX_ROW, dtype=torch.int64)
        out = torch.ops.centerclip.collate_clips_crop_flip(src, boxes, clips, N_PX, chw)
        assert tuple(out.shape) == (2 * T,) + shape and out.dtype == torch.uint8
        assert torch.ops.centerclip.collate_clips_crop_flip_out(src, boxes, clips, N_PX, chw, buf) is None
        with pytest.raises(ValueError, match="frame table"):
            torch.ops.centerclip.collate_clips(src, boxes, plans, clips, N_PX, True, chw)
        with pytest.raises(ValueError, match="out must be"):
            torch.ops.centerclip.collate_clips_out(src, rows, plans, clips, N_PX, True, chw, buf[:1])


def test_header_declares_the_new_symbols_and_constants():
    import centerclip_amd.torch_ops as TO
    text = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("cc_collate_resize_crop_u8", "cc_collate_resize_crop_workspace_bytes", "cc_collate_crop_flip_u8",
                "cc_resize_crop_status"):
        assert re.search(r"\b%s\s*\(" % sym, code), sym
    consts = dict(re.findall(r"#define (CC_COLLATE_[A-Z_]+) (\d+)", code))
    assert (int(consts["CC_COLLATE_ROW"]), int(consts["CC_COLLATE_BOX_ROW"]), int(consts["CC_COLLATE_MAX_PLANES"])) == \
        (TO.COLLATE_ROW, TO.COLLATE_BOX_ROW, TO.COLLATE_MAX_PLANES)
    assert "at most TWO launches" in text                          # the launch bound is stated where the entry points are


def test_entry_points_validate_before_any_launch():
    """NULL pointers, n_out <= 0 and a clip that does not lie inside the packed bytes: CC_ERR_INVALID, no GPU needed."""
    import ctypes
    from centerclip_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(16)                                      # (never followed: every call below is refused first)
    ok = (ctypes.c_int64 * 4)(0, 2, 40, 56)
    over = (ctypes.c_int64 * 4)(1, 2, 40, 56)
    n = 2 * 40 * 56 * 3
    ev = lambda src, clips, rows, n_out, plans, dst: lib.cc_collate_resize_crop_u8(src, n, 2, clips, 1, rows, n_out, plans, 64, N_PX, 1,
                                                                                    dst, 2, None, 0, None)
    tr = lambda src, clips, rows, n_out, dst: lib.cc_collate_crop_flip_u8(src, n, 2, clips, 1, rows, n_out, N_PX, dst, 2, None)
    for args in ((None, ok, one, 8, one, one), (one, None, one, 8, one, one), (one, ok, None, 8, one, one),
                 (one, ok, one, 8, None, one), (one, ok, one, 8, one, None), (one, ok, one, 0, one, one),
                 (one, over, one, 8, one, one)):
        assert ev(*args) == -1, args
    for args in ((None, ok, one, 8, one), (one, None, one, 8, one), (one, ok, None, 8, one), (one, ok, one, 8, None),
                 (one, ok, one, -1, one), (one, over, one, 8, one)):
        assert tr(*args) == -1, args
    small = (ctypes.c_int64 * 4)(0, 1, 32, 24)
    assert lib.cc_collate_resize_crop_u8(one, n, 2, small, 1, one, 4, one, 64, N_PX, 0, one, 2, None, 0, None) == \
        lib.cc_resize_crop_status(32, 24, N_PX, 0) != 0           # the crop alone of a frame smaller than the crop
    # ... and with the resize it runs both passes: no workspace, no launch
    assert lib.cc_collate_resize_crop_u8(one, n, 2, small, 1, one, 4, one, 64, N_PX, 1, one, 2, None, 0, None) == -3
    assert lib.cc_resize_crop_status(40, 56, N_PX, 1) == 0
    both = (ctypes.c_int64 * 8)(0, 1, 40, 56, 6720, 1, 32, 32)
    per_frame = lib.cc_resize_crop_workspace_bytes(1, 40, 56, N_PX, 1)
    assert per_frame > 0 and lib.cc_collate_resize_crop_workspace_bytes(both, 2, 8, N_PX, 1) == 8 * per_frame
