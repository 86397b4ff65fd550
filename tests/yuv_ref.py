"""NumPy restatement of the YUV 4:2:0 -> RGB conversion of include/centerclip_hip.h ("YUV 4:2:0 sources"; DESIGN.md section
7), in int64, and the real (float64) formula it approximates, built from Kr and Kb.  No GPU, no library: the tests hold the
kernels to ``convert`` bit for bit and ``convert`` to ``convert_real`` within 1 LSB."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MODES = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]
# the tables of the issue / the header, (CY, CRV, CGU, CGV, CBU)
TABLE = {("bt601", False): (76309, 104597, 25675, 53279, 132201), ("bt601", True): (65536, 91881, 22553, 46802, 116130),
         ("bt709", False): (76309, 117489, 13975, 34925, 138438), ("bt709", True): (65536, 103206, 12276, 30679, 121609)}


def real_coefficients(matrix, full_range):
    """-> (oy, cY, cRV, cGU, cGV, cBU) as Python floats (IEEE double)"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full_range else 16, sy, 2.0 * (1.0 - kr) * sc, 2.0 * kb * (1.0 - kb) / kg * sc, 2.0 * kr * (1.0 - kr) / kg * sc,
            2.0 * (1.0 - kb) * sc)


def coefficients(matrix, full_range):
    """-> (CY, CRV, CGU, CGV, CBU) = round(c 2^16)"""
    return tuple(int(np.floor(c * 65536.0 + 0.5)) for c in real_coefficients(matrix, full_range)[1:])


def convert(Y, U, V, matrix="bt601", full_range=False):
    """Y, U, V: integer arrays of one shape, values 0 .. 255 -> uint8 [..., 3], the integer definition in int64"""
    CY, CRV, CGU, CGV, CBU = coefficients(matrix, full_range)
    y = Y.astype(np.int64) - (0 if full_range else 16)
    u, v = U.astype(np.int64) - 128, V.astype(np.int64) - 128
    rgb = np.stack([CY * y + CRV * v + 32768, CY * y - CGU * u - CGV * v + 32768, CY * y + CBU * u + 32768], -1)
    assert int(np.abs(rgb).max()) < 2 ** 31                          # the kernels' int32 accumulator holds it
    return np.clip(rgb >> 16, 0, 255).astype(np.uint8)              # (>> on int64 is arithmetic)


def convert_real(Y, U, V, matrix="bt601", full_range=False):
    """clamp(floor(real + 0.5)) of the float64 formula"""
    oy, cy, crv, cgu, cgv, cbu = real_coefficients(matrix, full_range)
    y, u, v = Y.astype(np.float64) - oy, U.astype(np.float64) - 128.0, V.astype(np.float64) - 128.0
    rgb = np.stack([cy * y + crv * v, cy * y - cgu * u - cgv * v, cy * y + cbu * u], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def chroma(n):
    return (n + 1) // 2


def planes_to_rgb(Y, U, V, matrix="bt601", full_range=False):
    """Y [F, H, W], U / V [F, ceil(H/2), ceil(W/2)] -> uint8 [F, H, W, 3]; luma (y, x) uses chroma (y >> 1, x >> 1)"""
    H, W = Y.shape[-2:]
    up = lambda c: np.repeat(np.repeat(c, 2, -2), 2, -1)[..., :H, :W]
    return convert(Y, up(U), up(V), matrix, full_range)


def pack(Y, U, V, kind):
    """Tight frames one behind the other -> uint8 [F, H W + 2 ch cw]: "i420" (Y, U, V), "yv12" (Y, V, U), "nv12" (Y, UV
    interleaved), "nv21" (Y, VU interleaved).  Any H, W (odd ones included)."""
    F = Y.shape[0]
    if kind in ("i420", "yv12"):
        a, b = (U, V) if kind == "i420" else (V, U)
        return np.concatenate([Y.reshape(F, -1), a.reshape(F, -1), b.reshape(F, -1)], 1)
    a, b = (U, V) if kind == "nv12" else (V, U)
    return np.concatenate([Y.reshape(F, -1), np.stack([a, b], -1).reshape(F, -1)], 1)


def layout(kind, H, W, matrix="bt601", full_range=False):
    """The eight integers of cc_yuv420_layout for ``pack``'s frames"""
    ch, cw = chroma(H), chroma(W)
    first, second = H * W, H * W + (ch * cw if kind in ("i420", "yv12") else 1)
    u, v = (first, second) if kind in ("i420", "nv12") else (second, first)
    planar = kind in ("i420", "yv12")
    return [H * W + 2 * ch * cw, W, u, v, cw if planar else 2 * cw, 1 if planar else 2, ["bt601", "bt709"].index(matrix),
            int(full_range)]


def random_planes(F, H, W, seed=0):
    g = np.random.RandomState(seed)
    return (g.randint(0, 256, (F, H, W)).astype(np.uint8), g.randint(0, 256, (F, chroma(H), chroma(W))).astype(np.uint8),
            g.randint(0, 256, (F, chroma(H), chroma(W))).astype(np.uint8))
