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

Both take one uniform tensor.  What a decoder produces is ragged - clips of mixed H x W and mixed lengths - and goes through
``pack_clips`` (one byte buffer + a host table, usable as a DataLoader ``collate_fn``) and ``ClipCollate`` (either transform
on every clip of the batch, zero padding included, in at most two launches):

    packed = pack_clips([clip_0, clip_1, ...])                           # uint8 [t_i, H_i, W_i, 3] each, t_i <= T
    video = ClipCollate(224, max_frames=12)(packed.to(device))           # uint8 [B, 1, T, 224, 224, 3]
    out = model(ids, seg, mask, video, packed.video_mask(12))

All of the above start from RGB bytes.  Decoders produce YUV; the ``Yuv*`` counterparts at the end of this file take the planes
as decoded ([..., 3H/2, W], PyAV's ``to_ndarray()`` of yuv420p / nv12; 4:2:2, 4:4:4 and the 10-, 12- and 16-bit layouts - "p010",
"i420p10", ... as uint16 - the same way) and convert inside the first resampling pass:

    video = YuvFrameTransform(224, layout="nv12", matrix="bt709")(video_yuv)     # uint8 [B, 1, T, 3H/2, W] -> [B, 1, T, 224, 224, 3]
"""
import ctypes
import math
import random

import numpy as np
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


def _run(op, args, out, shape):
    """The tail of every transform: torch.ops.centerclip.<op> as a fresh tensor viewed as ``shape``, or <op>_out into ``out``."""
    if out is None:
        return getattr(torch.ops.centerclip, op)(*args).view(shape)
    getattr(torch.ops.centerclip, op + "_out")(*args, out)
    return out


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
        return _run("resize_center_crop", (frames, self.n_px, self.resize), out, self.output_shape(frames.shape))


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

    def _device_boxes(self, boxes, device):
        """A host box table is uploaded (not inside a stream capture), a device tensor is used as it is."""
        if boxes.is_cuda:
            return boxes
        if torch.cuda.is_current_stream_capturing():
            raise L.CenterClipHipError("%s.apply: a host box table cannot be uploaded while the stream is being captured - pass a "
                                       "device tensor and refill it between replays" % type(self).__name__)
        return boxes.to(device=device, dtype=torch.int32)

    def apply(self, frames, boxes, out=None, frames_per_clip=None):
        """The device op on given boxes.  ``boxes``: the table of ``sample`` - a host tensor is uploaded (not inside a stream
        capture), a device tensor is used as it is: no upload, and a captured call follows what the buffer holds at replay.
        ``frames_per_clip``: from the shape by default (6-D: T; 4-D: all frames are one clip).  ``out`` as FrameTransform's."""
        _check(frames)
        fpc = self._clips(frames.shape)[1] if frames_per_clip is None else int(frames_per_clip)
        return _run("resized_crop_flip", (frames, self._device_boxes(boxes, frames.device), self.n_px, fpc, self.interp), out,
                    self.output_shape(frames.shape))

    def __call__(self, frames, out=None):
        _, H, W = _check(frames)
        return self.apply(frames, self.sample(self._clips(frames.shape)[0], H, W), out=out)



# ------------------------------------------------------------------------------------------ ragged clip batches
class PackedClips:
    """A ragged batch of decoded clips: ``data`` - the clips' bytes back to back in one 1-D uint8 tensor, no alignment padding
    (odd sizes give odd offsets; the kernels read single bytes) - and ``table`` - HOST int64 [B, 4] rows (byte offset, frames
    t, H, W).  ``chw``: every clip is [t, 3, H, W] instead of [t, H, W, 3].  Built by ``pack_clips``."""

    def __init__(self, data, table, chw):
        self.data, self.table, self.chw = data, table, bool(chw)

    def __len__(self):
        return int(self.table.shape[0])

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    def to(self, device=None, non_blocking=False, **_):
        """ONE host-to-device copy of the bytes (asynchronous from the pinned buffer with non_blocking=True); the table stays
        on the host."""
        return PackedClips(self.data.to(device=device, non_blocking=non_blocking), self.table, self.chw)

    def pin_memory(self):
        return self if self.data.is_pinned() else PackedClips(self.data.pin_memory(), self.table, self.chw)

    def clip(self, b):
        """Clip b as a view of the bytes: [t, H, W, 3] or [t, 3, H, W]."""
        off, t, H, W = (int(v) for v in self.table[b])
        return self.data[off:off + t * H * W * 3].view((t, 3, H, W) if self.chw else (t, H, W, 3))

    def __getitem__(self, rows):
        """The clips ``rows`` (an index tensor or list) as a new PackedClips - a copy of their bytes (eval_epoch uses it for a
        DistributedSampler's padded tail only)."""
        return pack_clips([self.clip(int(b)) for b in torch.as_tensor(rows).reshape(-1).tolist()], "chw" if self.chw else "hwc")

    def video_mask(self, T, lengths=None):
        """-> int64 [B, T], ones in the first min(t_b, T) slots of clip b - or in the first lengths[b] slots, e.g. the
        reference's min(num_frames, T) for a clip sampled down to T frames (sampling.py).  Host work only."""
        n = self.table[:, 1].clamp(max=int(T)) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
        if n.numel() != len(self) or bool((n < 0).any()) or bool((n > int(T)).any()):
            raise ValueError("video_mask: lengths must be %d values in [0, %d], got %s" % (len(self), T, n.tolist()))
        return (torch.arange(int(T)).unsqueeze(0) < n.unsqueeze(1)).to(torch.int64)


def pack_clips(clips, layout=None):
    """A list of B uint8 arrays / tensors [t_i, H_i, W_i, 3] or [t_i, 3, H_i, W_i] (t_i >= 1; one layout per batch: "hwc",
    "chw" or None = what the shapes say) -> ``PackedClips``.  Host clips are copied once into one pinned buffer (plain host
    memory where no device is present and inside a DataLoader worker process), so ``.to(device)`` is one asynchronous copy;
    usable as, or inside, a DataLoader ``collate_fn``.  Device tensors are accepted too and packed with ONE ``torch.cat`` of their flat views: a device-to-device
    copy of every byte (and the non-contiguous ones once more) - decode into host memory where that matters."""
    clips = [torch.from_numpy(np.ascontiguousarray(c)) if isinstance(c, np.ndarray) else c for c in clips]
    if not clips:
        raise ValueError("pack_clips: no clips")
    if layout not in (None, "hwc", "chw"):
        raise ValueError("pack_clips: layout must be 'hwc', 'chw' or None, got %r" % (layout,))
    for i, c in enumerate(clips):
        if not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or c.dim() != 4:
            raise ValueError("pack_clips: clip %d is not a 4-D uint8 array or tensor" % i)
    # the one layout every clip reads as; [t, 3, H, W] wins where both do, as everywhere in the package
    reads = {"chw": all(c.shape[1] == 3 for c in clips), "hwc": all(c.shape[3] == 3 for c in clips)}
    if not reads["chw" if layout is None and reads["chw"] else (layout or "hwc")]:
        raise ValueError("pack_clips: one layout per batch - the clips %s are not all %s"
                         % ([tuple(c.shape) for c in clips], {"chw": "[t, 3, H, W]", "hwc": "[t, H, W, 3]",
                                                              None: "[t, H, W, 3] nor all [t, 3, H, W]"}[layout]))
    chw = reads["chw"] if layout is None else layout == "chw"
    rows, off = [], 0
    for i, c in enumerate(clips):
        t, H, W = (int(c.shape[0]), int(c.shape[2]), int(c.shape[3])) if chw else (int(c.shape[0]), int(c.shape[1]), int(c.shape[2]))
        if t < 1 or H < 1 or W < 1:
            raise ValueError("pack_clips: clip %d is empty: %s" % (i, tuple(c.shape)))
        rows.append((off, t, H, W))
        off += t * H * W * 3
    table = torch.tensor(rows, dtype=torch.int64)
    if any(c.is_cuda for c in clips):
        if not all(c.is_cuda for c in clips):
            raise ValueError("pack_clips: host and device clips in one batch")
        return PackedClips(torch.cat([c.contiguous().view(-1) for c in clips]), table, chw)
    # (a DataLoader worker process must not touch the device: it packs into plain memory, and DataLoader(pin_memory=True)
    #  pins the batch through PackedClips.pin_memory in the main process)
    pin = torch.cuda.is_available() and torch.utils.data.get_worker_info() is None
    data = torch.empty(off, dtype=torch.uint8, pin_memory=pin)
    for (o, t, H, W), c in zip(rows, clips):
        data[o:o + t * H * W * 3].view(c.shape).copy_(c)
    return PackedClips(data, table, chw)


class ClipCollate:
    """A ``PackedClips`` on the device -> the loaders' uniform video, uint8 [B, 1, T, n_px, n_px, 3] ([B, 1, T, 3, n_px, n_px]
    for a channels-first batch), T = max_frames: per clip the evaluation transform (``train=None``: Resize(n_px, BICUBIC) +
    CenterCrop(n_px), the crop alone with resize=False - byte for byte ``resize_center_crop`` of that clip) or the training
    transform (``train=TrainFrameTransform(...)``: one box and one flip per clip, drawn by that object for the clips in batch
    order, each with exactly the calls of ``train.sample(1, H_b, W_b)``, applied to all T slots - byte for byte
    ``resized_crop_flip`` of that clip), in at most two launches whatever the batch holds (torch.ops.centerclip.collate_clips /
    collate_clips_crop_flip).  A ``frame_transform`` for eval_epoch, train_epoch and DeviceFeeder.

    ``index``: host ints [B, T]; slot s of clip b is frame index[b, s] of that clip, -1 a zero frame; repeats and any order
    are allowed.  Default: frame s for s < t_b and zero frames behind (the CV2 loaders' padding); a clip longer than T must be
    sampled by the caller (sampling.py).  Zero frames are written by the launch: a reused ``out`` never shows a stale frame.

    Everything is checked on the host before anything is launched - ValueError for an index outside [-1, t_b), a clip longer
    than T without an index, a size the per-clip op refuses (a frame smaller than the crop, more than 65 taps per axis; the
    error names the clip).  The resize plans are built once per (H, W) and kept on the host; a call's tables (frame rows + the
    plans of its sizes) go to the device in ONE small copy from pinned memory - which cannot be captured: inside a stream
    capture the call raises CenterClipHipError.  No host synchronisation anywhere."""

    def __init__(self, n_px=224, max_frames=12, resize=True, train=None):
        self.n_px, self.max_frames, self.resize, self.train = int(n_px), int(max_frames), bool(resize), train
        if train is not None and train.n_px != self.n_px:
            raise ValueError("ClipCollate(n_px=%d) with a TrainFrameTransform(n_px=%d)" % (self.n_px, train.n_px))
        self._plans = {}                                         # (H, W) -> the host plan, int32

    def passes_through(self, packed):
        return False

    def output_shape(self, packed):
        n = self.n_px
        return (len(packed), 1, self.max_frames) + ((3, n, n) if packed.chw else (n, n, 3))

    def plan(self, H, W, clip=None):
        """The host plan (cc_resize_plan_build) of a frame size, built once; ValueError for a size resize_center_crop refuses."""
        key = (int(H), int(W))
        if key not in self._plans:
            lib = L.lib()
            if lib.cc_resize_crop_status(key[0], key[1], self.n_px, int(self.resize)) != L.CC_OK:
                raise ValueError("ClipCollate: %s %d x %d frames are outside what resize_center_crop(n_px=%d, resize=%s) takes (a "
                                 "frame smaller than the crop, or more than 65 taps per axis)"
                                 % ("clip %d:" % clip if clip is not None else "", key[0], key[1], self.n_px, self.resize))
            host = np.empty(lib.cc_resize_plan_bytes(key[0], key[1], self.n_px, int(self.resize)) // 4, dtype=np.int32)
            L.check(lib.cc_resize_plan_build(key[0], key[1], self.n_px, int(self.resize), host.ctypes.data), "cc_resize_plan_build")
            self._plans[key] = host
        return self._plans[key]

    def index(self, packed, index=None):
        """The validated frame index, int64 [B, T] NumPy (the default where index is None)."""
        B, T, t = len(packed), self.max_frames, packed.table[:, 1].numpy()
        if index is None:
            if (t > T).any():
                raise ValueError("ClipCollate: clip %d has %d frames for %d slots - sample it (sampling.uniform_sampling) and pass "
                                 "the index, or pack the sampled frames only" % (int((t > T).argmax()), int(t.max()), T))
            s = np.arange(T, dtype=np.int64)[None, :]
            return np.where(s < t[:, None], s, -1)
        index = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
        if index.shape != (B, T) or index.dtype.kind not in "iu":
            raise ValueError("ClipCollate: index must be integers [%d, %d], got %s %s" % (B, T, index.dtype, index.shape))
        index = index.astype(np.int64)
        bad = (index < -1) | (index >= t[:, None])
        if bad.any():
            b, s = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError("ClipCollate: index[%d, %d] = %d, clip %d has frames 0 .. %d (-1: a zero frame)"
                             % (b, s, index[b, s], b, t[b] - 1))
        return index

    @staticmethod
    def _frame_bytes(tab):
        """Bytes of one frame of every clip of the host table."""
        return tab[:, 2] * tab[:, 3] * 3

    def _rows(self, packed, index, width):
        """The first four columns of the frame table: kind, byte offset of the source frame, H, W."""
        tab = packed.table.numpy()
        rows = np.zeros((index.shape[0], index.shape[1], width), dtype=np.int64)
        frame = self._frame_bytes(tab)
        rows[:, :, 0] = index >= 0
        rows[:, :, 1] = tab[:, :1] + np.maximum(index, 0) * frame[:, None]
        rows[:, :, 2] = tab[:, 2:3]
        rows[:, :, 3] = tab[:, 3:4]
        return rows

    def _upload(self, host, device):
        if torch.cuda.is_current_stream_capturing():
            raise L.CenterClipHipError("ClipCollate: a call's tables are uploaded, which cannot be part of a stream capture")
        return torch.from_numpy(host).pin_memory().to(device, non_blocking=True)

    def _check(self, packed, out):
        if not isinstance(packed, PackedClips):
            raise ValueError("ClipCollate takes a PackedClips (pack_clips), got %s" % type(packed).__name__)
        L.require_device(packed.data)
        if out is not None and tuple(out.shape) != self.output_shape(packed):
            raise ValueError("ClipCollate: out must be %s, got %s" % (self.output_shape(packed), tuple(out.shape)))

    def _eval(self, packed, index, out):
        self._check(packed, out)
        index = self.index(packed, index)
        tab = packed.table.numpy()
        offsets, parts, at = {}, [], 0                           # the call's plans one behind the other: (H, W) -> int32 offset
        for b, (H, W) in enumerate(zip(tab[:, 2].tolist(), tab[:, 3].tolist())):
            if (H, W) not in offsets:
                plan = self.plan(H, W, clip=b)
                offsets[(H, W)] = at
                parts.append(plan)
                at += plan.size
        B, S = index.shape
        rows = self._rows(packed, index, T.COLLATE_ROW)
        rows[:, :, 4] = np.array([offsets[(H, W)] for H, W in zip(tab[:, 2].tolist(), tab[:, 3].tolist())], dtype=np.int64)[:, None]
        clips = tab.reshape(-1).tolist()
        nws = L.lib().cc_collate_resize_crop_workspace_bytes(T._clips_host(clips), B, B * S, self.n_px, int(self.resize))
        rows[:, :, 5] = np.arange(B * S, dtype=np.int64).reshape(B, S) * (nws // (B * S))
        head = rows.reshape(-1)
        host = np.zeros(head.size + (at + 1) // 2, dtype=np.int64)
        host[:head.size] = head
        host[head.size:].view(np.int32)[:at] = np.concatenate(parts)
        dev = self._upload(host, packed.device)
        rows_dev, plans_dev = dev[:head.size].view(B * S, T.COLLATE_ROW), dev[head.size:].view(torch.int32)
        return self._eval_op(packed, rows_dev, plans_dev, clips, out)

    def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
        return _run("collate_clips", (packed.data, rows_dev, plans_dev, clips, self.n_px, self.resize, packed.chw), out,
                    self.output_shape(packed))

    def sample(self, packed):
        """-> int32 [B, 5] on the host, rows (top, left, height, width, flip): for the clips in batch order, each the draws of
        ``train.sample(1, H_b, W_b)``."""
        if self.train is None:
            raise ValueError("ClipCollate.sample: no TrainFrameTransform was given (train=None is the evaluation transform)")
        return torch.cat([self.train.sample(1, int(H), int(W)) for _, _, H, W in packed.table.tolist()], 0)

    def apply(self, packed, boxes, index=None, out=None):
        """The training transform on given boxes (host ints [B, 5] as ``sample`` gives them): deterministic."""
        if self.train is None:
            raise ValueError("ClipCollate.apply: no TrainFrameTransform was given (train=None is the evaluation transform)")
        self._check(packed, out)
        index = self.index(packed, index)
        B, S = index.shape
        tab = packed.table.numpy()
        boxes = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes).astype(np.int64)
        if boxes.shape != (B, 5):
            raise ValueError("ClipCollate.apply: boxes must be [%d, 5] rows (top, left, height, width, flip), got %s" % (B, boxes.shape))
        top, left, h, w = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
        bad = (top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > tab[:, 2]) | (left + w > tab[:, 3]) | (tab[:, 2] < 4) | (tab[:, 3] < 4)
        if bad.any():
            b = int(bad.argmax())
            raise ValueError("ClipCollate.apply: clip %d: the box (top %d, left %d, %d x %d) does not lie inside its %d x %d frame "
                             "(at least 4 x 4)" % (b, top[b], left[b], h[b], w[b], tab[b, 2], tab[b, 3]))
        rows = self._rows(packed, index, T.COLLATE_BOX_ROW)
        rows[:, :, 4:9] = boxes[:, None, :]
        rows[:, :, 9] = self.train.interp
        dev = self._upload(rows.reshape(-1), packed.device).view(B * S, T.COLLATE_BOX_ROW)
        return self._train_op(packed, dev, tab.reshape(-1).tolist(), out)

    def _train_op(self, packed, rows_dev, clips, out):
        return _run("collate_clips_crop_flip", (packed.data, rows_dev, clips, self.n_px, packed.chw), out, self.output_shape(packed))

    def __call__(self, packed, index=None, out=None):
        if self.train is None:
            return self._eval(packed, index, out)
        if not isinstance(packed, PackedClips):
            raise ValueError("ClipCollate takes a PackedClips (pack_clips), got %s" % type(packed).__name__)
        return self.apply(packed, self.sample(packed), index=index, out=out)


# ------------------------------------------------------------------------------------------ YUV sources
# What decoders produce before any colour conversion ("YUV sources").  At this level frames are [..., rows, W] arrays
# with the layout tight - exactly PyAV's ``frame.to_ndarray()``: H rows of Y, then the chroma bytes as further rows of W samples,
# rows = 3H/2 for 4:2:0 ("i420": the U plane and the V plane, each H/2 x W/2; "nv12": H/2 rows of interleaved UV), 2H for 4:2:2
# and 3H for 4:4:4; uint8 for the 8-bit layouts, uint16 (or int16 with the same bits) for the 10-, 12- and 16-bit ones; H and W
# even where the axis is subsampled.  torch_ops.YUV_FORMATS is the one table of what a layout name means.  A pitched or
# odd-sized surface goes through the ops (torch_ops.yuv_*) with an explicit layout.
def yuv_coefficients(matrix="bt601", full_range=False, depth=8):
    """-> (CY, CRV, CGU, CGV, CBU), the fixed-point coefficients of the conversion (cc_yuv_coefficients_depth): 16 fraction bits
    at depth 8, 20 at depth 10 / 12 / 16."""
    if matrix not in T.YUV_MATRICES:
        raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
    out = (ctypes.c_int32 * 5)()
    L.check(L.lib().cc_yuv_coefficients_depth(T.YUV_MATRICES[matrix], int(bool(full_range)), int(depth), out),
            "cc_yuv_coefficients_depth")
    return tuple(int(v) for v in out)


def _yuv_geometry(shape, layout="i420"):
    """[..., rows, W] with at least one leading dimension -> (leading dimensions, H, W); rows = H (2^s + 2) / 2^s with s the
    number of subsampled axes: 3H/2, 2H or 3H."""
    _, sub_x, sub_y, _, _, _ = T.YUV_FORMATS[layout]
    den = 1 << (sub_x + sub_y)
    num = den + 2
    name = {4: "3H/2", 2: "2H", 1: "3H"}[den]
    H = int(shape[-2]) * den // num if len(shape) >= 3 else 0
    if len(shape) < 3 or int(shape[-2]) * den % num or H < 1 or shape[-1] < 1 or (sub_y and H % 2) or (sub_x and shape[-1] % 2):
        raise ValueError("%s frames must be [..., %s, W] with a leading frame dimension and H / W even where chroma is subsampled (a "
                         "decoder's to_ndarray()), got %s" % (layout, name, tuple(shape)))
    return tuple(shape[:-2]), H, int(shape[-1])


def _yuv_frame_dtypes(layout):
    """The dtypes of a named layout's frames: bytes at depth 8, 16-bit words (either signedness, the same bits) above."""
    return (torch.uint8,) if T.YUV_FORMATS[layout][3] == 8 else (torch.uint16, torch.int16)


class _YuvSource:
    """What the YUV transforms share: the colour description, the checks, the tight layout of a frame size."""

    def _init_yuv(self, layout, matrix, full_range):
        if layout not in T.YUV_FORMATS or matrix not in T.YUV_MATRICES:
            raise ValueError("layout must be one of %s and matrix 'bt601' or 'bt709', got %r, %r"
                             % (", ".join(sorted(T.YUV_FORMATS)), layout, matrix))
        self.layout, self.matrix, self.full_range = layout, matrix, bool(full_range)

    @property
    def frame_dtypes(self):
        """The dtypes of this layout's frames (what DeviceFeeder recognises as the video of a batch)."""
        return _yuv_frame_dtypes(self.layout)

    def _source(self, frames):
        """-> (leading dimensions, F, H, W, the twelve layout integers) of device frames [..., rows, W]"""
        L.require_device(frames)
        if frames.dtype not in self.frame_dtypes:
            raise ValueError("the %s frame transform takes the decoder's %s planes, got %s"
                             % (self.layout, " / ".join(str(d).replace("torch.", "") for d in self.frame_dtypes), frames.dtype))
        lead, H, W = _yuv_geometry(frames.shape, self.layout)
        return lead, math.prod(lead), H, W, T.yuv_tight_layout(self.layout, H, W, self.matrix, self.full_range)

    def output_shape(self, shape):
        lead, _, _ = _yuv_geometry(shape, self.layout)
        return lead + (self.n_px, self.n_px, 3)


def yuv_to_rgb(frames, layout="i420", matrix="bt601", full_range=False):
    """[..., rows, W] frames of a named layout -> uint8 [..., H, W, 3] RGB (torch.ops.centerclip.yuv_to_rgb): the fixed integer
    conversion of the header for the layout's depth, chroma replicated.  The fused transforms below never store this image; it is
    the stand-alone form and what they are defined against."""
    src = _YuvSource()
    src._init_yuv(layout, matrix, full_range)
    lead, F, H, W, lay = src._source(frames)
    return torch.ops.centerclip.yuv_to_rgb(frames, F, H, W, lay, False).view(lead + (H, W, 3))


def yuv420_to_rgb(frames, layout="i420", matrix="bt601", full_range=False):
    """``yuv_to_rgb`` for the two 8-bit 4:2:0 layouts: uint8 [..., 3H/2, W] -> uint8 [..., H, W, 3]."""
    if layout not in T.YUV_KINDS:
        raise ValueError("layout must be 'i420' or 'nv12', got %r" % (layout,))
    return yuv_to_rgb(frames, layout, matrix, full_range)


class YuvFrameTransform(_YuvSource):
    """``FrameTransform`` on YUV frames as decoded: [..., rows, W] -> uint8 [..., n_px, n_px, 3], bit for bit
    ``FrameTransform(n_px, resize)(yuv_to_rgb(frames, ...))`` with the conversion inside the first resampling pass - half the
    bytes (4:2:0, 8-bit) cross PCIe and are read, and no ``to_rgb()`` runs on a CPU core.  The same protocol (eval_epoch,
    train_epoch, DeviceFeeder); nothing passes through: a frame of the model's size is still converted."""
    frame_dims = (3, 5)                              # what DeviceFeeder recognises as this transform's video: [F, ..] / [B, 1, T, ..]

    def __init__(self, n_px=224, resize=True, layout="i420", matrix="bt601", full_range=False):
        self.n_px, self.resize = int(n_px), bool(resize)
        self._init_yuv(layout, matrix, full_range)

    def passes_through(self, shape):
        return False

    def __call__(self, frames, out=None):
        lead, F, H, W, lay = self._source(frames)
        T.resize_plan(H, W, self.n_px, self.resize, frames.device)
        return _run("resize_center_crop_yuv", (frames, F, H, W, lay, self.n_px, self.resize, False), out,
                    lead + (self.n_px, self.n_px, 3))


class YuvTrainFrameTransform(_YuvSource, TrainFrameTransform):
    """``TrainFrameTransform`` on YUV frames as decoded: the same boxes from the same draws (``sample`` is that class's), applied
    by one launch that converts its taps - bit for bit ``TrainFrameTransform.apply(yuv_to_rgb(frames, ...), boxes)``."""
    frame_dims = (3, 5)

    def __init__(self, n_px=224, layout="i420", matrix="bt601", full_range=False, **train):
        TrainFrameTransform.__init__(self, n_px, **train)
        self._init_yuv(layout, matrix, full_range)

    def apply(self, frames, boxes, out=None, frames_per_clip=None):
        lead, F, H, W, lay = self._source(frames)
        fpc = self._clips(lead + (H, W, 3))[1] if frames_per_clip is None else int(frames_per_clip)
        return _run("resized_crop_flip_yuv", (frames, F, H, W, lay, self._device_boxes(boxes, frames.device), self.n_px, fpc,
                                              self.interp, False), out, lead + (self.n_px, self.n_px, 3))

    def __call__(self, frames, out=None):
        lead, _, H, W, _ = self._source(frames)
        return self.apply(frames, self.sample(self._clips(lead + (H, W, 3))[0], H, W), out=out)


def _yuv_frame_bytes(layout, H, W):
    """Bytes of one tight frame of a named layout; H, W: ints or integer arrays."""
    _, sub_x, sub_y, depth, _, _ = T.YUV_FORMATS[layout]
    return (H * W + 2 * ((H + sub_y) >> sub_y) * ((W + sub_x) >> sub_x)) * (1 if depth == 8 else 2)


class PackedYuvClips(PackedClips):
    """``PackedClips`` of tight YUV clips of one named layout: ``data`` the bytes (uint8, whatever the sample size), ``table`` rows
    (byte offset, frames t, H, W).  Built by ``pack_yuv_clips``."""

    def __init__(self, data, table, layout):
        PackedClips.__init__(self, data, table, False)
        self.layout = layout

    def to(self, device=None, non_blocking=False, **_):
        return PackedYuvClips(self.data.to(device=device, non_blocking=non_blocking), self.table, self.layout)

    def pin_memory(self):
        return self if self.data.is_pinned() else PackedYuvClips(self.data.pin_memory(), self.table, self.layout)

    def clip(self, b):
        """Clip b as a view of the bytes: [t, rows, W], uint8 or (16-bit samples) uint16."""
        off, t, H, W = (int(v) for v in self.table[b])
        n = t * _yuv_frame_bytes(self.layout, H, W)
        flat = self.data[off:off + n]
        if T.YUV_FORMATS[self.layout][3] > 8:
            flat = flat.view(torch.uint16)
        return flat.view(t, -1, W)

    def __getitem__(self, rows):
        return pack_yuv_clips([self.clip(int(b)) for b in torch.as_tensor(rows).reshape(-1).tolist()], self.layout)


def pack_yuv_clips(clips, layout="i420"):
    """``pack_clips`` for YUV clips: a list of B arrays / tensors [t_i, rows_i, W_i] of one named layout (uint8, or uint16 / int16
    for the 10-, 12- and 16-bit layouts) -> ``PackedYuvClips`` (a ``PackedClips``: one pinned byte buffer + the host table), for
    ``YuvClipCollate``."""
    if layout not in T.YUV_FORMATS:
        raise ValueError("pack_yuv_clips: layout must be one of %s, got %r" % (", ".join(sorted(T.YUV_FORMATS)), layout))
    dtypes = _yuv_frame_dtypes(layout)
    clips = [torch.from_numpy(np.ascontiguousarray(c)) if isinstance(c, np.ndarray) else c for c in clips]
    if not clips:
        raise ValueError("pack_yuv_clips: no clips")
    rows, off = [], 0
    for i, c in enumerate(clips):
        if not isinstance(c, torch.Tensor) or c.dtype not in dtypes or c.dim() != 3 or c.shape[0] < 1:
            raise ValueError("pack_yuv_clips: clip %d is not a %s array or tensor [t >= 1, rows, W] of layout %s"
                             % (i, " / ".join(str(d).replace("torch.", "") for d in dtypes), layout))
        _, H, W = _yuv_geometry(c.shape, layout)
        rows.append((off, int(c.shape[0]), H, W))
        off += c.numel() * c.element_size()
    table = torch.tensor(rows, dtype=torch.int64)
    flat = [c.contiguous().view(torch.uint8).reshape(-1) for c in clips]                 # the clips' bytes
    if any(c.is_cuda for c in clips):
        if not all(c.is_cuda for c in clips):
            raise ValueError("pack_yuv_clips: host and device clips in one batch")
        return PackedYuvClips(torch.cat(flat), table, layout)
    pin = torch.cuda.is_available() and torch.utils.data.get_worker_info() is None
    data = torch.empty(off, dtype=torch.uint8, pin_memory=pin)
    for (o, _, _, _), c in zip(rows, flat):
        data[o:o + c.numel()].copy_(c)
    return PackedYuvClips(data, table, layout)


class YuvClipCollate(_YuvSource, ClipCollate):
    """``ClipCollate`` on a ``PackedYuvClips``: the same tables, checks and launch bound, every clip's taps converted on the way
    in - each output frame bit for bit ``YuvFrameTransform`` / ``YuvTrainFrameTransform.apply`` of its clip.  ``train``: a
    ``TrainFrameTransform`` (or its Yuv subclass - only its box drawing and interpolation are used).  -> uint8
    [B, 1, T, n_px, n_px, 3]."""

    def __init__(self, n_px=224, max_frames=12, resize=True, train=None, layout="i420", matrix="bt601", full_range=False):
        ClipCollate.__init__(self, n_px, max_frames, resize, train)
        self._init_yuv(layout, matrix, full_range)

    output_shape = ClipCollate.output_shape          # of a PackedClips; _YuvSource's, first in the MRO, is the frame transforms'

    def _frame_bytes(self, tab):
        return _yuv_frame_bytes(self.layout, tab[:, 2], tab[:, 3])

    def _check(self, packed, out):
        ClipCollate._check(self, packed, out)
        if getattr(packed, "layout", self.layout) != self.layout:
            raise ValueError("YuvClipCollate(layout=%r) on clips packed as %r" % (self.layout, packed.layout))
        tab = packed.table.numpy()
        _, sub_x, sub_y, _, _, _ = T.YUV_FORMATS[self.layout]
        if (((tab[:, 2] & sub_y) | (tab[:, 3] & sub_x)) & 1).any():
            raise ValueError("YuvClipCollate: packed %s clips have even H / W where chroma is subsampled, got %s"
                             % (self.layout, tab[:, 2:].tolist()))

    def _kind(self):
        return T.YUV_FORMATS[self.layout][0], T.YUV_MATRICES[self.matrix], self.full_range

    def _eval_op(self, packed, rows_dev, plans_dev, clips, out):
        return _run("collate_clips_yuv", (packed.data, rows_dev, plans_dev, clips, self.n_px, self.resize, *self._kind(), False), out,
                    self.output_shape(packed))

    def _train_op(self, packed, rows_dev, clips, out):
        return _run("collate_clips_crop_flip_yuv", (packed.data, rows_dev, clips, self.n_px, *self._kind(), False), out,
                    self.output_shape(packed))


__all__ = ["resize_center_crop", "FrameTransform", "TrainFrameTransform", "PackedClips", "pack_clips", "ClipCollate",
           "yuv_coefficients", "yuv_to_rgb", "yuv420_to_rgb", "YuvFrameTransform", "YuvTrainFrameTransform", "PackedYuvClips",
           "pack_yuv_clips", "YuvClipCollate"]
