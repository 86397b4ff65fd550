"""NumPy restatement of the general YUV -> RGB conversion of include/centerclip_hip.h ("YUV sources in general"; DESIGN.md
section 7) for depth 8 / 10 / 12 / 16 and any shift, in int64, the real (float64) formula it approximates, the packing of every
named format (tight frames, pitched surfaces, odd sizes) and the twelve descriptor integers.  No GPU, no library: the tests hold
the kernels to ``convert`` bit for bit and ``convert`` to ``convert_real`` within 1 LSB."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRICES = ("bt601", "bt709")
MODES = [(m, f) for m in MATRICES for f in (False, True)]
DEPTHS = (8, 10, 12, 16)
# name: (CC_YUV_* code, sub_x, sub_y, depth, shift, interleaved) - restated here, not read from the package
FORMATS = {"i420": (0, 1, 1, 8, 0, False), "nv12": (1, 1, 1, 8, 0, True), "i422": (2, 1, 0, 8, 0, False), "i444": (3, 0, 0, 8, 0, False),
           "i420p10": (4, 1, 1, 10, 0, False), "i422p10": (5, 1, 0, 10, 0, False), "i444p10": (6, 0, 0, 10, 0, False),
           "p010": (7, 1, 1, 10, 6, True), "i420p12": (8, 1, 1, 12, 0, False), "p012": (9, 1, 1, 12, 4, True),
           "p016": (10, 1, 1, 16, 0, True), "i444p16": (11, 0, 0, 16, 0, False)}
# the tables of the issue / the header, (depth, matrix, full_range) -> (CY, CRV, CGU, CGV, CBU)
TABLE = {(10, "bt601", False): (305236, 418389, 102698, 213115, 528805), (10, "bt601", True): (261375, 366448, 89949, 186658, 463157),
         (10, "bt709", False): (305236, 469956, 55902, 139699, 553753), (10, "bt709", True): (261375, 411614, 48962, 122356, 485008),
         (16, "bt601", False): (4769, 6537, 1605, 3330, 8263), (16, "bt709", False): (4769, 7343, 873, 2183, 8652)}


def fraction_bits(depth):
    return 16 if depth == 8 else 20


def real_coefficients(matrix, full_range, depth):
    """-> (oy, centre, cY, cRV, cGU, cGV, cBU) as Python floats (IEEE double)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    up = float(2 ** (depth - 8))
    sy, sc = (255.0 / (2 ** depth - 1),) * 2 if full_range else (255.0 / (219.0 * up), 255.0 / (224.0 * up))
    return (0 if full_range else 16 * 2 ** (depth - 8), 2 ** (depth - 1), sy, 2.0 * (1.0 - kr) * sc, 2.0 * kb * (1.0 - kb) / kg * sc,
            2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc)


def coefficients(matrix, full_range, depth):
    """-> (CY, CRV, CGU, CGV, CBU) = floor(c 2^Q + 0.5)"""
    one = float(2 ** fraction_bits(depth))
    return tuple(int(np.floor(c * one + 0.5)) for c in real_coefficients(matrix, full_range, depth)[2:])


def accumulators(Y, U, V, matrix, full_range, depth):
    """The three int64 sums (rounding constant included) of sample VALUES Y, U, V -> int64 [..., 3]"""
    CY, CRV, CGU, CGV, CBU = coefficients(matrix, full_range, depth)
    oy, centre = real_coefficients(matrix, full_range, depth)[:2]
    half = 1 << (fraction_bits(depth) - 1)
    y, u, v = Y.astype(np.int64) - oy, U.astype(np.int64) - centre, V.astype(np.int64) - centre
    return np.stack([CY * y + CRV * v + half, CY * y - CGU * u - CGV * v + half, CY * y + CBU * u + half], -1)


def convert(Y, U, V, matrix="bt601", full_range=False, depth=8):
    """Sample values 0 .. 2^depth - 1 of one shape -> uint8 [..., 3], the integer definition in int64"""
    acc = accumulators(Y, U, V, matrix, full_range, depth)
    assert int(np.abs(acc).max()) < 2 ** 31                          # the kernels' int32 accumulator holds it
    return np.clip(acc >> fraction_bits(depth), 0, 255).astype(np.uint8)       # (>> on int64 is arithmetic)


def convert_real(Y, U, V, matrix="bt601", full_range=False, depth=8):
    """clamp(floor(real + 0.5)) of the float64 formula"""
    oy, centre, cy, crv, cgu, cgv, cbu = real_coefficients(matrix, full_range, depth)
    y, u, v = Y.astype(np.float64) - oy, U.astype(np.float64) - centre, V.astype(np.float64) - centre
    rgb = np.stack([cy * y + crv * v, cy * y - cgu * u - cgv * v, cy * y + cbu * u], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def lattice(depth):
    """-> (luma values, chroma values): every 2^d / 1024-th luma value and every 2^d / 96-th chroma value, plus both ends and the
    two centre values"""
    top = 2 ** depth - 1
    luma = np.unique(np.minimum(np.floor(np.arange(1025) * 2.0 ** depth / 1024), top).astype(np.int64))
    chroma = np.unique(np.concatenate([np.minimum(np.floor(np.arange(97) * 2.0 ** depth / 96), top).astype(np.int64),
                                       [0, top, 2 ** (depth - 1) - 1, 2 ** (depth - 1)]]))
    return luma, chroma


def chroma(n, sub):
    return (n + sub) >> sub


def word_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def random_planes(name, F, H, W, seed=0):
    """-> (Y, U, V) sample VALUES (int64) of F frames of the named format, chroma planes ceil(H / 2^sub_y) x ceil(W / 2^sub_x);
    the first samples of every plane of frame 0 are 0, the maximum and the two centre values"""
    _, sx, sy, depth, _, _ = FORMATS[name]
    g = np.random.RandomState(seed)
    shapes = ((F, H, W), (F, chroma(H, sy), chroma(W, sx)), (F, chroma(H, sy), chroma(W, sx)))
    planes = [g.randint(0, 2 ** depth, s).astype(np.int64) for s in shapes]
    for p in planes:
        p[0].reshape(-1)[:4] = (0, 2 ** depth - 1, 2 ** (depth - 1) - 1, 2 ** (depth - 1))
    return tuple(planes)


def planes_to_rgb(Y, U, V, name, matrix="bt601", full_range=False):
    """Sample values -> uint8 [F, H, W, 3]; luma (y, x) uses chroma (y >> sub_y, x >> sub_x)"""
    _, sx, sy, depth, _, _ = FORMATS[name]
    H, W = Y.shape[-2:]
    up = lambda c: np.repeat(np.repeat(c, 1 << sy, -2), 1 << sx, -1)[..., :H, :W]
    return convert(Y, up(U), up(V), matrix, full_range, depth)


def words(values, name, low=None):
    """Sample values -> the words as stored: value << shift, the bits below the shift from ``low`` (an array of that shape)"""
    _, _, _, depth, shift, _ = FORMATS[name]
    w = values.astype(np.int64) << shift
    if low is not None:
        w |= low.astype(np.int64) & ((1 << shift) - 1)
    return w.astype(word_dtype(depth))


def pack(Y, U, V, name, low=None):
    """Tight frames one behind the other -> words [F, H W + 2 ch cw] (uint8, or uint16 for depth > 8): the Y plane, then the U
    and the V plane, or one interleaved UV plane.  Any H, W (odd ones included).  low: (ly, lu, lv) bits below the shift."""
    F = Y.shape[0]
    ly, lu, lv = low if low is not None else (None, None, None)
    y, u, v = words(Y, name, ly), words(U, name, lu), words(V, name, lv)
    if FORMATS[name][5]:
        return np.concatenate([y.reshape(F, -1), np.stack([u, v], -1).reshape(F, -1)], 1)
    return np.concatenate([y.reshape(F, -1), u.reshape(F, -1), v.reshape(F, -1)], 1)


def layout(name, H, W, matrix="bt601", full_range=False):
    """The twelve integers of cc_yuv_layout for ``pack``'s frames (positions in bytes)"""
    _, sx, sy, depth, shift, inter = FORMATS[name]
    b = 1 if depth == 8 else 2
    ch, cw = chroma(H, sy), chroma(W, sx)
    u = H * W * b
    v = u + (b if inter else ch * cw * b)
    return [(H * W + 2 * ch * cw) * b, W * b, u, v, (2 if inter else 1) * cw * b, (2 if inter else 1) * b, sx, sy, depth, shift,
            MATRICES.index(matrix), int(full_range)]


def pack_pitched(Y, U, V, name, pad_y=6, pad_c=10, pad_frame=14, fill=0xAA, matrix="bt601", full_range=False):
    """A pitched surface of a semi-planar or planar format: every luma row pad_y BYTES longer than its samples, every chroma row
    pad_c, every frame pad_frame bytes behind the last plane (all even), the gaps filled with ``fill`` -> (uint8 bytes [F * stride],
    the twelve layout integers)"""
    _, sx, sy, depth, shift, inter = FORMATS[name]
    b = 1 if depth == 8 else 2
    F, H, W = Y.shape
    ch, cw = U.shape[-2:]
    yp = W * b + pad_y
    cp = (2 if inter else 1) * cw * b + pad_c
    planes = 1 if inter else 2
    stride = H * yp + planes * ch * cp + pad_frame
    buf = np.full(F * stride, fill, np.uint8)
    dt = word_dtype(depth)
    y, u, v = words(Y, name), words(U, name), words(V, name)
    for f in range(F):
        frame = buf[f * stride:(f + 1) * stride]                     # (contiguous slices: the reshapes below are views)
        frame[:H * yp].reshape(H, yp)[:, :W * b].view(dt)[:] = y[f]
        c = frame[H * yp:H * yp + planes * ch * cp].reshape(planes * ch, cp)
        if inter:
            uv = c[:, :2 * cw * b].view(dt)
            uv[:, 0::2], uv[:, 1::2] = u[f], v[f]
        else:
            c[:ch, :cw * b].view(dt)[:] = u[f]
            c[ch:, :cw * b].view(dt)[:] = v[f]
    u_off = H * yp
    v_off = u_off + (b if inter else ch * cp)
    return buf, [stride, yp, u_off, v_off, cp, (2 if inter else 1) * b, sx, sy, depth, shift, MATRICES.index(matrix), int(full_range)]


def frame_rows(name, H):
    """Rows of the decoder's [rows, W] array form of one frame: 3H/2, 2H or 3H"""
    _, sx, sy, _, _, _ = FORMATS[name]
    den = 1 << (sx + sy)
    return H * (den + 2) // den
