"""The frame ops (resize + centre crop, resized crop + flip, the two ragged collates and the conversion; RGB, 4:2:0 and general
YUV sources) at the dispatcher, without a GPU: their schemas are the recorded ones, every one is in ``torch_ops.OPS``, and the
fake kernel of an ``_out`` op refuses what its allocating twin refuses - both run the operation's one body."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from centerclip_amd import torch_ops

SCHEMAS = {
    "resize_center_crop": "centerclip::resize_center_crop(Tensor frames, SymInt n_px, bool resize) -> Tensor",
    "resize_center_crop_out": "centerclip::resize_center_crop_out(Tensor frames, SymInt n_px, bool resize, Tensor(a3!) out) -> ()",
    "resize_center_crop_yuv420": "centerclip::resize_center_crop_yuv420(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, SymInt n_px, bool resize, bool chw) -> Tensor",
    "resize_center_crop_yuv420_out": "centerclip::resize_center_crop_yuv420_out(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, SymInt n_px, bool resize, bool chw, Tensor(a8!) out) -> ()",
    "resize_center_crop_yuv": "centerclip::resize_center_crop_yuv(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, SymInt n_px, bool resize, bool chw) -> Tensor",
    "resize_center_crop_yuv_out": "centerclip::resize_center_crop_yuv_out(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, SymInt n_px, bool resize, bool chw, Tensor(a8!) out) -> ()",
    "resized_crop_flip": "centerclip::resized_crop_flip(Tensor frames, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp) -> Tensor",
    "resized_crop_flip_out": "centerclip::resized_crop_flip_out(Tensor frames, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp, Tensor(a5!) out) -> ()",
    "resized_crop_flip_yuv420": "centerclip::resized_crop_flip_yuv420(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp, bool chw) -> Tensor",
    "resized_crop_flip_yuv420_out": "centerclip::resized_crop_flip_yuv420_out(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp, bool chw, Tensor(a10!) out) -> ()",
    "resized_crop_flip_yuv": "centerclip::resized_crop_flip_yuv(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp, bool chw) -> Tensor",
    "resized_crop_flip_yuv_out": "centerclip::resized_crop_flip_yuv_out(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp, bool chw, Tensor(a10!) out) -> ()",
    "collate_clips": "centerclip::collate_clips(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, bool chw) -> Tensor",
    "collate_clips_out": "centerclip::collate_clips_out(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, bool chw, Tensor(a7!) out) -> ()",
    "collate_clips_yuv420": "centerclip::collate_clips_yuv420(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, SymInt kind, SymInt matrix, bool full_range, bool chw) -> Tensor",
    "collate_clips_yuv420_out": "centerclip::collate_clips_yuv420_out(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, SymInt kind, SymInt matrix, bool full_range, bool chw, Tensor(a10!) out) -> ()",
    "collate_clips_yuv": "centerclip::collate_clips_yuv(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, SymInt fmt, SymInt matrix, bool full_range, bool chw) -> Tensor",
    "collate_clips_yuv_out": "centerclip::collate_clips_yuv_out(Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, SymInt fmt, SymInt matrix, bool full_range, bool chw, Tensor(a10!) out) -> ()",
    "collate_clips_crop_flip": "centerclip::collate_clips_crop_flip(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, bool chw) -> Tensor",
    "collate_clips_crop_flip_out": "centerclip::collate_clips_crop_flip_out(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, bool chw, Tensor(a5!) out) -> ()",
    "collate_clips_crop_flip_yuv420": "centerclip::collate_clips_crop_flip_yuv420(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, SymInt kind, SymInt matrix, bool full_range, bool chw) -> Tensor",
    "collate_clips_crop_flip_yuv420_out": "centerclip::collate_clips_crop_flip_yuv420_out(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, SymInt kind, SymInt matrix, bool full_range, bool chw, Tensor(a8!) out) -> ()",
    "collate_clips_crop_flip_yuv": "centerclip::collate_clips_crop_flip_yuv(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, SymInt fmt, SymInt matrix, bool full_range, bool chw) -> Tensor",
    "collate_clips_crop_flip_yuv_out": "centerclip::collate_clips_crop_flip_yuv_out(Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, SymInt fmt, SymInt matrix, bool full_range, bool chw, Tensor(a8!) out) -> ()",
    "yuv420_to_rgb": "centerclip::yuv420_to_rgb(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, bool chw) -> Tensor",
    "yuv_to_rgb": "centerclip::yuv_to_rgb(Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout, bool chw) -> Tensor",
}

F, H, W, N_PX = 3, 12, 20, 8
NV12 = [360, 20, 240, 241, 20, 2, 0, 0]                       # tight 12 x 20 NV12, the eight integers of cc_yuv420_layout
P010 = [720, 40, 480, 482, 40, 4, 1, 1, 10, 6, 0, 0]          # tight 12 x 20 P010, the twelve integers of cc_yuv_layout
CLIPS, N_OUT = [0, F, H, W], 6                                # one packed clip of three frames, six output slots


def test_schemas_are_the_recorded_ones_and_every_op_is_listed():
    assert len(SCHEMAS) == 26
    for name, schema in SCHEMAS.items():
        assert str(getattr(torch.ops.centerclip, name).default._schema) == schema
        assert name in torch_ops.OPS
    assert len(set(torch_ops.OPS)) == len(torch_ops.OPS)


def _cases():
    """name of the allocating op -> (its arguments, the source first; the shape its result has)."""
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8)
    boxes, plans = torch.empty(F, 5, dtype=torch.int32), torch.empty(100, dtype=torch.int32)
    rows = torch.empty(N_OUT, torch_ops.COLLATE_ROW, dtype=torch.int64)
    box_rows = torch.empty(N_OUT, torch_ops.COLLATE_BOX_ROW, dtype=torch.int64)
    planes, words = u8(F, 3 * H // 2, W), torch.empty(F, 3 * H // 2, W, dtype=torch.uint16)
    frames, collated = (F, N_PX, N_PX, 3), (N_OUT, N_PX, N_PX, 3)
    return {
        "resize_center_crop": ((u8(F, H, W, 3), N_PX, True), frames),
        "resize_center_crop_yuv420": ((planes, F, H, W, NV12, N_PX, True, False), frames),
        "resize_center_crop_yuv": ((words, F, H, W, P010, N_PX, True, False), frames),
        "resized_crop_flip": ((u8(F, H, W, 3), boxes, N_PX, 1, 1), frames),
        "resized_crop_flip_yuv420": ((planes, F, H, W, NV12, boxes, N_PX, 1, 1, False), frames),
        "resized_crop_flip_yuv": ((words, F, H, W, P010, boxes, N_PX, 1, 1, False), frames),
        "collate_clips": ((u8(F * H * W * 3), rows, plans, CLIPS, N_PX, True, False), collated),
        "collate_clips_yuv420": ((u8(F * 360), rows, plans, CLIPS, N_PX, True, 1, 0, False, False), collated),
        "collate_clips_yuv": ((u8(F * 720), rows, plans, CLIPS, N_PX, True, 7, 0, False, False), collated),
        "collate_clips_crop_flip": ((u8(F * H * W * 3), box_rows, CLIPS, N_PX, False), collated),
        "collate_clips_crop_flip_yuv420": ((u8(F * 360), box_rows, CLIPS, N_PX, 1, 0, False, False), collated),
        "collate_clips_crop_flip_yuv": ((u8(F * 720), box_rows, CLIPS, N_PX, 7, 0, False, False), collated),
    }


@pytest.mark.parametrize("name", [n[:-4] for n in SCHEMAS if n.endswith("_out")])
def test_out_fakes_refuse_what_their_allocating_twins_refuse(name):
    """A float source and an ``out`` one pixel too wide: ValueError naming the op, from the ``_out`` fake as from the twin's."""
    ops = torch.ops.centerclip
    with FakeTensorMode():
        args, shape = _cases()[name]
        plain, into = getattr(ops, name), getattr(ops, name + "_out")
        got = plain(*args)
        assert tuple(got.shape) == shape and got.dtype == torch.uint8
        assert into(*args, torch.empty(shape, dtype=torch.uint8)) is None
        wrong_src = (torch.empty(args[0].shape, dtype=torch.float32),) + args[1:]
        with pytest.raises(ValueError, match=name):
            plain(*wrong_src)
        with pytest.raises(ValueError, match=name):
            into(*wrong_src, torch.empty(shape, dtype=torch.uint8))
        for wrong_out in (torch.empty(shape[:-2] + (N_PX + 1, 3), dtype=torch.uint8), torch.empty(shape, dtype=torch.float32)):
            with pytest.raises(ValueError, match=name + ".*out must be"):
                into(*args, wrong_out)
