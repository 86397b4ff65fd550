"""The frame transform of CLIP's loader on the device: ``Resize(n_px, BICUBIC)`` -> ``CenterCrop(n_px)`` of
dataloaders/rawvideo_util.py:16-23 (the pyAV loader's ``CenterCrop`` alone with ``resize=False``, dataloaders/decode.py:37,46),
byte for byte what Pillow / torchvision produce, on decoded uint8 frames of any size.  ``ToTensor`` and ``Normalize`` - the
transform's other two steps - run inside the encoders' uint8 patch gather, so

    transform = FrameTransform(224)
    out = model(ids, seg, mask, transform(video_u8), video_mask)         # video_u8 [B, 1, T, H, W, 3] as decoded

is the whole loader transform with one byte per sample crossing PCIe and nothing on a CPU core.  No decoding, sampling or
dataset code lives here.  HIP only: a CPU tensor raises, as everywhere in the package.
"""
import torch

from . import _lib as L
from . import torch_ops as T


def _check(frames):
    L.require_device(frames)
    if frames.dtype != torch.uint8:
        raise ValueError("the frame transform takes the decoder's uint8 frames, got %s" % frames.dtype)
    if frames.dim() not in (4, 6):
        raise ValueError("frames must be [F,H,W,3], [F,3,H,W] or the loaders' 6-D video [B,1,T,H,W,3] / [B,1,T,3,H,W], got %s"
                         % (tuple(frames.shape),))
    return T._raw_frames_geometry(frames.shape)


def resize_center_crop(frames, n_px=224, resize=True):
    """uint8 [F,H,W,3] / [F,3,H,W] / 6-D video -> the same form at n_px x n_px (torch.ops.centerclip.resize_center_crop)."""
    _check(frames)
    return torch.ops.centerclip.resize_center_crop(frames, int(n_px), bool(resize))


class FrameTransform:
    """``resize_center_crop`` as a callable for the loops' ``frame_transform`` hooks (eval_epoch, train_epoch, DeviceFeeder).
    The device plan of a frame size (geometry + integer coefficient tables, a few KB) is built and uploaded on the first batch of
    that size and kept per (H, W, device); an upload cannot be captured, so inside a stream capture a size that was not seen
    before is an error.  A batch that already has the model's resolution passes through untouched (the same tensor)."""

    def __init__(self, n_px=224, resize=True):
        self.n_px, self.resize = int(n_px), bool(resize)
        self._plans = {}

    def plan(self, H, W, device):
        device = torch.device(device)
        key = (int(H), int(W), device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._plans:
            self._plans[key] = T.resize_plan(H, W, self.n_px, self.resize, device)
        return self._plans[key]

    def passes_through(self, shape):
        _, H, W = T._raw_frames_geometry(shape)
        return H == self.n_px and W == self.n_px

    def output_shape(self, shape):
        return T._resize_crop_shape(shape, self.n_px)

    def __call__(self, frames, out=None):
        """``out``: a uint8 buffer of ``output_shape(frames.shape)`` to write instead of a fresh tensor (not with a batch that
        passes through)."""
        _, H, W = _check(frames)
        if H == self.n_px and W == self.n_px:
            if out is not None:
                raise ValueError("frames of the model's resolution pass through untouched: there is nothing to write to `out`")
            return frames
        self.plan(H, W, frames.device)
        if out is None:
            return torch.ops.centerclip.resize_center_crop(frames, self.n_px, self.resize)
        torch.ops.centerclip.resize_center_crop_out(frames, self.n_px, self.resize, out)
        return out


__all__ = ["resize_center_crop", "FrameTransform"]
