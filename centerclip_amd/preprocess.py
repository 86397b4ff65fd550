"""The frame transform of CLIP's loader on the device: ``Resize(n_px, BICUBIC)`` -> ``CenterCrop(n_px)`` of
dataloaders/rawvideo_util.py:16-23 (the pyAV loader's ``CenterCrop`` alone with ``resize=False``, dataloaders/decode.py:37,46),
byte for byte what Pillow / torchvision produce, on decoded uint8 frames of any size.  ``ToTensor`` and ``Normalize`` - the
transform's other two steps - run inside the encoders' uint8 patch gather, so

    transform = FrameTransform(224)
    out = model(ids, seg, mask, transform(video_u8), video_mask)         # video_u8 [B, 1, T, H, W, 3] as decoded

is the whole loader transform with one byte per sample crossing PCIe and nothing on a CPU core.  No decoding, sampling or
dataset code lives here.  HIP only: a CPU tensor raises, as everywhere in the package.

``TrainFrameTransform`` is the training loader's counterpart (dataloaders/decode.py:32-41): a multi-scale or random-resized
crop and a horizontal flip per clip, the boxes drawn on the host, one launch on the clip's uint8 frames.
"""
import math
import random

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


_INTERP = {"bilinear": 0, "bicubic": 1, 0: 0, 1: 1}


class TrainFrameTransform:
    """The training loader's augmentations (dataloaders/decode.py:32-41) as a ``frame_transform`` for train_epoch and
    DeviceFeeder: per clip ONE crop box, resized to n_px x n_px, and ONE horizontal flip bit, drawn on the host and applied to
    the clip's decoded uint8 frames by one launch (torch.ops.centerclip.resized_crop_flip).

    ``crop``:
      "multiscale"      TensorMultiScaleCrop(n_px, scales, max_distort, fix_crop, more_fix_crop) (dataloaders/transforms.py:
                        37-134): crop sizes int(min(W, H) * s), replaced by n_px where within 3 of it; the (w, h) pairs whose
                        scale indices differ by at most max_distort; one ``choice`` of the pair, one ``choice`` of the 5 / 13
                        fixed offsets (two ``randint`` with fix_crop=False).  With the same seed it draws the reference's
                        boxes: the same calls on the same generator class.  Default interpolation: bilinear.
      "random_resized"  torchvision's published RandomResizedCrop.get_params(scale, ratio): ten tries of area * U(scale) with a
                        log-uniform aspect ratio, then the central fallback.  The draws come from this object's
                        random.Random, not from torch's generator as torchvision's do, so torchvision's stream of boxes is
                        NOT reproduced - only its distribution.  Default interpolation: bicubic.
      "center"          torchvision's CenterCrop(n_px) box (no resampling), so that ``flip`` alone is available.
    ``flip=True``: TensorRandomHorizontalFlip (transforms.py:168-196) - after each clip's box one ``random() < 0.5``.
    ``interpolation``: "bilinear" / "bicubic" (or 0 / 1); None: the default of ``crop``.  Both are F.interpolate's
    align_corners=False arithmetic without antialias, as torchvision's resized_crop on a tensor.  The one difference from the
    reference's float pipeline: the result is rounded and clamped to bytes ("Train-time augmentation").
    A sampled box that leaves the frame - the reference would zero-pad - raises ValueError: padding is not built.

    ``sample`` draws, ``apply`` is the deterministic device op, ``__call__`` is both.  HIP only: a CPU tensor raises."""

    def __init__(self, n_px=224, crop="multiscale", scales=(1, .875, .75, .66), max_distort=1, fix_crop=True,
                 more_fix_crop=True, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), interpolation=None, flip=False, seed=None):
        if crop not in ("multiscale", "random_resized", "center"):
            raise ValueError("crop must be 'multiscale', 'random_resized' or 'center', got %r" % (crop,))
        if interpolation is None:
            interpolation = "bicubic" if crop == "random_resized" else "bilinear"
        if interpolation not in _INTERP:
            raise ValueError("interpolation must be 'bilinear' or 'bicubic', got %r" % (interpolation,))
        self.n_px, self.crop, self.interp = int(n_px), crop, _INTERP[interpolation]
        self.scales, self.max_distort = tuple(scales), int(max_distort)
        self.fix_crop, self.more_fix_crop = bool(fix_crop), bool(more_fix_crop)
        self.scale, self.ratio, self.flip = tuple(scale), tuple(ratio), bool(flip)
        self.rng = random.Random(seed)

    # ---- the boxes, as (top, left, height, width)
    def _multiscale_box(self, H, W):
        n, rng = self.n_px, self.rng
        sizes = [int(min(W, H) * s) for s in self.scales]
        sizes = [n if abs(x - n) < 3 else x for x in sizes]
        pairs = [(w, h) for i, h in enumerate(sizes) for j, w in enumerate(sizes) if abs(i - j) <= self.max_distort]
        w, h = rng.choice(pairs)
        if not self.fix_crop:
            if w > W or h > H:
                raise ValueError("multiscale crop %dx%d does not fit a %dx%d frame (padding is not built)" % (h, w, H, W))
            left = rng.randint(0, W - w)
            return rng.randint(0, H - h), left, h, w
        ws, hs = (W - w) // 4, (H - h) // 4
        offsets = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]       # corners, centre
        if self.more_fix_crop:
            offsets += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0),          # edge centres
                        (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]                # quarters
        left, top = rng.choice(offsets)
        return top, left, h, w

    def _random_resized_box(self, H, W):
        rng, area = self.rng, H * W
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for _ in range(10):
            target = area * rng.uniform(self.scale[0], self.scale[1])
            aspect = math.exp(rng.uniform(lo, hi))
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = rng.randint(0, H - h)
                return top, rng.randint(0, W - w), h, w
        return self.fallback_box(H, W)

    def fallback_box(self, H, W):
        """The central crop torchvision's get_params falls back to after ten failed tries: the whole frame cut to the nearer
        bound of ``ratio``."""
        w, h = W, H
        if W / H < min(self.ratio):
            h = int(round(W / min(self.ratio)))
        elif W / H > max(self.ratio):
            w = int(round(H * max(self.ratio)))
        return (H - h) // 2, (W - w) // 2, h, w

    def _center_box(self, H, W):
        n = self.n_px
        return int(round((H - n) / 2.0)), int(round((W - n) / 2.0)), n, n          # (round: half to even, as CenterCrop)

    def sample(self, clips, H, W):
        """-> int32 [clips, 5] on the host, rows (top, left, height, width, flip): per clip, in order, the box and then (with
        flip=True) one ``random() < 0.5`` from this object's random.Random(seed)."""
        H, W = int(H), int(W)
        box = dict(multiscale=self._multiscale_box, random_resized=self._random_resized_box, center=self._center_box)[self.crop]
        rows = []
        for _ in range(int(clips)):
            top, left, h, w = box(H, W)
            if top < 0 or left < 0 or h < 1 or w < 1 or top + h > H or left + w > W:
                raise ValueError("the sampled crop (top %d, left %d, %d x %d) leaves the %d x %d frame: the reference would "
                                 "zero-pad, which is not built" % (top, left, h, w, H, W))
            rows.append((top, left, h, w, int(self.rng.random() < 0.5) if self.flip else 0))
        return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 5)

    @staticmethod
    def _clips(shape):
        """-> (clips, frames per clip): the loaders' 6-D video [B, 1, T, ...] is B clips of T frames, 4-D frames are one clip"""
        lead = tuple(shape[:-3])
        return (math.prod(lead[:-1]), int(lead[-1])) if len(lead) > 1 else (1, int(lead[0]))

    def passes_through(self, shape):
        return False

    def output_shape(self, shape):
        return T._resize_crop_shape(shape, self.n_px)

    def apply(self, frames, boxes, out=None, frames_per_clip=None):
        """The device op on given boxes.  ``boxes``: the table of ``sample`` - a host tensor is uploaded (not inside a stream
        capture), a device tensor is used as it is: no upload, and a captured call follows what the buffer holds at replay.
        ``frames_per_clip``: from the shape by default (6-D: T; 4-D: all frames are one clip).  ``out`` as FrameTransform's."""
        _check(frames)
        fpc = self._clips(frames.shape)[1] if frames_per_clip is None else int(frames_per_clip)
        if not boxes.is_cuda:
            if torch.cuda.is_current_stream_capturing():
                raise L.CenterClipHipError("TrainFrameTransform.apply: a host box table cannot be uploaded while the stream is "
                                           "being captured - pass a device tensor and refill it between replays")
            boxes = boxes.to(device=frames.device, dtype=torch.int32)
        if out is None:
            return torch.ops.centerclip.resized_crop_flip(frames, boxes, self.n_px, fpc, self.interp)
        torch.ops.centerclip.resized_crop_flip_out(frames, boxes, self.n_px, fpc, self.interp, out)
        return out

    def __call__(self, frames, out=None):
        _, H, W = _check(frames)
        return self.apply(frames, self.sample(self._clips(frames.shape)[0], H, W), out=out)


__all__ = ["resize_center_crop", "FrameTransform", "TrainFrameTransform"]
