"""NumPy restatement of the frame transform of CLIP's loader (dataloaders/rawvideo_util.py:16-23): torchvision's
``Resize(n_px, BICUBIC)`` - Pillow's 8-bit ``Image.resize`` - followed by ``CenterCrop(n_px)``, in integers.  Written from the
text of the arithmetic ("Resize and centre crop"), not from the HIP source: the tests compare the library's plan
and kernels against this, and this against Pillow (live where it is installed, and through tests/golden/resize_golden.npz).

    frames uint8 [F, H, W, 3]  ->  uint8 [F, n_px, n_px, 3]
"""
import math

import numpy as np

PRECISION_BITS = 22


def resized_size(H, W, n_px):
    """torchvision Resize(int): the short side becomes n_px, the long side int(n_px * long / short) (true division, then
    truncation); a frame whose short side already is n_px keeps its size (it is not resampled at all)."""
    if W <= H:
        if W == n_px:
            return H, W
        return int(n_px * H / W), n_px
    if H == n_px:
        return H, W
    return n_px, int(n_px * W / H)


def crop_offset(size, n_px):
    """torchvision CenterCrop: int(round((size - n_px) / 2.0)), Python's round - half to even."""
    return int(round((size - n_px) / 2.0))


def _bicubic(x):
    a = -0.5
    t = -x if x < 0.0 else x
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def axis_coefficients(n_in, n_out):
    """-> (ksize, xmin [n_out], n [n_out], coef int32 [n_out, ksize]) of one axis, every step in IEEE double in the order of the
    text (Python floats are doubles and nothing here is fused)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(n_out, np.int32)
    cnt = np.zeros(n_out, np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        x0 = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - x0
        w = [_bicubic(((x + x0) - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], cnt[xx] = x0, n
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return ksize, xmin, cnt, coef


def apply_axis(img, axis, xmin, cnt, coef):
    """One pass along `axis` of img [..., H, W, C] uint8 (axis -3 = rows, -2 = columns): int32 accumulation from 2^21,
    arithmetic shift by 22, clamp to a byte.  -> uint8 with len(xmin) entries along the axis."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(xmin),) + src.shape[1:], np.uint8)
    for j in range(len(xmin)):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for k in range(int(cnt[j])):
            acc += src[int(xmin[j]) + k] * int(coef[j, k])
        assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)          # (the product accumulates in int32)
        out[j] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(frames, oh, ow):
    """Pillow's two passes on [F, H, W, 3] uint8: horizontal first, rounded to bytes, then vertical; a pass whose size does not
    change is skipped."""
    H, W = frames.shape[-3], frames.shape[-2]
    out = frames
    if ow != W:
        _, xmin, cnt, coef = axis_coefficients(W, ow)
        out = apply_axis(out, -2, xmin, cnt, coef)
    if oh != H:
        _, ymin, cnt, coef = axis_coefficients(H, oh)
        out = apply_axis(out, -3, ymin, cnt, coef)
    return out


def resize_center_crop(frames, n_px, resize=True):
    """[F, H, W, 3] uint8 -> [F, n_px, n_px, 3] uint8."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    H, W = frames.shape[1], frames.shape[2]
    oh, ow = resized_size(H, W, n_px) if resize else (H, W)
    if oh < n_px or ow < n_px:
        raise ValueError("a %dx%d frame is smaller than the %d crop (the zero padding is not built)" % (oh, ow, n_px))
    top, left = crop_offset(oh, n_px), crop_offset(ow, n_px)
    return np.ascontiguousarray(resize_u8(frames, oh, ow)[:, top:top + n_px, left:left + n_px])


def cases():
    """The fixture cases of tests/golden/resize_golden.npz: name -> (H, W, kind), all at n_px = 32."""
    return {"down_33x57": (33, 57, "noise"), "portrait_100x37": (100, 37, "noise"), "up_17x64": (17, 64, "noise"),
            "square_50x50": (50, 50, "ramp"), "same_32x57": (32, 57, "noise"), "shrink_300x100": (300, 100, "checker"),
            "ramp_64x40": (64, 40, "ramp")}


def make_input(H, W, kind, seed=0, frames=1):
    """Deterministic test frames [frames, H, W, 3] uint8: uniform noise, a 0/255 checkerboard (drives the cubic's overshoot
    into both clamps) or diagonal ramps."""
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, (frames, H, W, 3)).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    if kind == "checker":
        img = (((y // 3 + x // 2 + c) % 2) * 255).astype(np.uint8)
    else:
        img = ((3 * y + 5 * x + 40 * c) % 256).astype(np.uint8)
    return np.stack([np.roll(img, f, axis=1) for f in range(frames)], 0)
