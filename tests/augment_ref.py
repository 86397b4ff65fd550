"""The float64 restatement of cc_resized_crop_flip_u8 the augmentation tests compare against (NumPy, no GPU): the crop of a box,
resized to n_px x n_px with the separable weights of torch.nn.functional.interpolate(align_corners=False, no antialias), the
coordinates taken from the exact rational ((2 o + 1) crop - n_px) / (2 n_px), then the optional column reversal.  Values, not
bytes: ``check_bytes`` applies the rule a byte result is held to.  ``kernel_fp32`` is the kernel's own arithmetic - the same
operations in the same order in IEEE single - so that the error bound can be looked at without a device."""
from fractions import Fraction

import numpy as np

# The bound DELTA[interp] on |kernel's fp32 value - exact value| (in levels of 255), derived from the kernel's arithmetic
# (csrc/augment.hip, compiled without contraction: every operation rounds once, relative error <= u = 2^-24):
#   t = rem / den, one division of exact integers: |dt| <= u.  s = 1 - t: |ds| <= 2 u.
#   bilinear: weights (s, t): sum of weight errors E <= 3 u, sum of |weights| S = 1.
#   bicubic:  outer taps A t s s and A s t t (3 products, values <= 0.12, derivatives <= 0.75 in t and s): <= 4 u each;
#             inner taps ((1.25 x - 2.25) x) x + 1 for x = t, s: five roundings of intermediates <= 1.25, 2.25, 2.25, 1, 1,
#             the first three still to be multiplied by x, x^2 <= 1: <= 7.75 u, plus |d/dx| <= 1.35 times dx: <= 10 u (x = t),
#             <= 11 u (x = s).  E <= 29 u, rounded up to 30 u;  S = 1 + 2 * 0.1875 = 1.375 (largest at t = 1/2).
#   a row:    h = sum_k w_k p_k, p <= 255, summed left to right: 255 E (weights) + 255 S u (products) + 3 * 255 S u (adds; one
#             add for bilinear) =: e_h;  |h| <= 255 S.
#   a pixel:  v = sum_r w_r h_r: S e_h + 255 S E (weights) + 255 S^2 u (products) + 3 * 255 S^2 u (adds) =: e_v.
#   bilinear: e_h = 255 (3 + 1 + 1) u = 1275 u; e_v = 1275 u + 765 u + 255 u + 255 u = 2550 u = 1.52e-4  -> 2e-4
#   bicubic:  e_h = 255 (30 + 1.375 + 4.125) u = 9053 u; e_v = 12448 u + 10519 u + 483 u + 1447 u = 24897 u = 1.484e-3 -> 1.5e-3
# (second-order terms are below 1e-9).  rint and the clamp are exact and monotone: a value farther than DELTA from every
# half-integer rounds as the exact value does.
DELTA = {0: 2e-4, 1: 1.5e-3}
A = -0.75


def axis_taps(crop, n_px, interp, dtype=np.float64):
    """-> (idx [n_px, taps] into the crop, w [n_px, taps]) of an axis resized from crop to n_px samples.  float64: the weights
    from the exact fraction, each polynomial in its textbook form; float32: the kernel's operations in the kernel's order."""
    taps = 2 if interp == 0 else 4
    idx, w = np.zeros((n_px, taps), np.int64), np.zeros((n_px, taps), dtype)
    den = 2 * n_px
    for o in range(n_px):
        num = (2 * o + 1) * crop - n_px
        if interp == 0 and num < 0:
            num = 0
        i0, rem = divmod(num, den)                               # floor, remainder in [0, den)
        if dtype == np.float32:
            t = np.float32(rem) / np.float32(den)
            s = np.float32(1) - t
        else:
            t, s = Fraction(rem, den), 1 - Fraction(rem, den)
        if interp == 0:
            idx[o] = (i0, min(i0 + 1, crop - 1))
            w[o] = (s, t)
            continue
        idx[o] = np.clip(np.arange(i0 - 1, i0 + 3), 0, crop - 1)
        if dtype == np.float32:
            a, c1, c2, one = np.float32(A), np.float32(1.25), np.float32(2.25), np.float32(1)
            w[o] = (a * t * s * s, (c1 * t - c2) * t * t + one, (c1 * s - c2) * s * s + one, a * s * t * t)
        else:
            a = Fraction(-3, 4)
            inner = lambda x: ((a + 2) * x - (a + 3)) * x * x + 1                          # noqa: E731
            outer = lambda x: ((a * x - 5 * a) * x + 8 * a) * x - 4 * a                    # noqa: E731
            w[o] = [float(v) for v in (outer(t + 1), inner(t), inner(s), outer(s + 1))]
    return idx, w


def resized_crop_flip(frames, box, n_px, interp, flip=False, dtype=np.float64):
    """frames uint8 [F, 3, H, W], box (top, left, h, w) -> values [F, 3, n_px, n_px] before rounding: columns first, then rows,
    each sum left to right (the order matters only for dtype=float32, the kernel's arithmetic)."""
    top, left, h, w = box
    crop = frames[:, :, top:top + h, left:left + w].astype(dtype)
    ix, wx = axis_taps(w, n_px, interp, dtype)
    iy, wy = axis_taps(h, n_px, interp, dtype)
    if flip:
        ix, wx = ix[::-1], wx[::-1]
    rows = np.zeros(crop.shape[:3] + (n_px,), dtype)
    for k in range(ix.shape[1]):
        rows = rows + wx[:, k] * crop[:, :, :, ix[:, k]]
    out = np.zeros(crop.shape[:2] + (n_px, n_px), dtype)
    for r in range(iy.shape[1]):
        out = out + wy[:, r, None] * rows[:, :, iy[:, r], :]
    return out


def kernel_fp32(frames, box, n_px, interp, flip=False):
    """The bytes of the kernel's own fp32 arithmetic."""
    return to_bytes(resized_crop_flip(frames, box, n_px, interp, flip, np.float32))


def to_bytes(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def check_bytes(got, v, delta):
    """The rule: a byte equals clamp(rint(v)) wherever the float64 value v is farther than delta from a half-integer; inside
    that band it may differ by one.  -> (share of the pixels inside the band, number of bytes that differ at all)."""
    want = to_bytes(v)
    band = np.abs(v - np.floor(v) - 0.5) <= delta
    diff = got.astype(np.int64) - want.astype(np.int64)
    assert not (diff[~band] != 0).any(), "%d bytes differ outside the band, e.g. value %r" % (
        int((diff[~band] != 0).sum()), float(v[~band][diff[~band] != 0][0]))
    assert (np.abs(diff[band]) <= 1).all()
    return float(band.mean()), int((diff != 0).sum())
