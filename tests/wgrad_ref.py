"""Plain references for the weight-gradient kernel (csrc/wgrad.hip: cc_wgrad_tn_f16), shared by tests/test_wgrad_host.py and
tests/test_wgrad_gpu.py.  numpy only, no device.

  * the case table: every (N1, N2, M) the GPU test launches, with the property of the work split it is listed for (pipeline
    depth nk, valid rows of the last stage, short / empty slices, a one-slice group in the reduce, bias chunk counts).  The
    slice count S is what the library reports (cc_wgrad_tn_workspace_bytes); the host test holds every entry to it;
  * operands: integer lattices (|v| <= 4, so that every fp32 partial sum is an integer below 2^24 and the result is exact in any
    order) and two float recipes (a heavy-tailed gradient against outlier channels; cancelling row pairs);
  * references: the float64 (and, for cross-checking, int64) product, the per-element bound M 2^-24 (|dY|^T |X|) / scale;
  * an emulation of the documented work split - slices by the documented rule, 32-row stages through the swizzled LDS image,
    padding rows that re-read the slice's last row and are cleared, partials added in slice order in groups of eight, the bias
    gradient's eight chunk segments - and mutants of it (MUTANTS), each one a defect the kernel could have.
"""
import math
from collections import namedtuple

import numpy as np

BN, BK = 128, 32                     # output tile edge, rows per stage
U = 2.0 ** -24                       # unit roundoff of fp32

Case = namedtuple("Case", "N1 N2 M want")          # want: the properties the case is listed for (see properties())


def case_id(c):
    return "%dx%d-M%d" % (c.N1, c.N2, c.M)


# ---------------------------------------------------------------------------------------------------- the case table

# one slice, depth 1 .. 8 with full and one-row last stages
DEPTH = [Case(128, 256, M, {"S": 1, "nk": -(-M // 32), "tail": M - (-(-M // 32) - 1) * 32})
         for M in (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 256)]
# one slice, the fourth stage (the first one requested inside the loop's ring) holds t = 1 .. 31 valid rows
TAIL = [Case(128, 256, 96 + t, {"S": 1, "nk": 4, "tail": t}) for t in range(1, 32)]
# N1 != N2 in both orders, and a square shape (dY and X are different matrices)
PLACEMENT = [Case(128, 384, 200, {"S": 1}), Case(384, 128, 200, {"S": 1}), Case(256, 128, 200, {"S": 1}),
             Case(256, 256, 200, {"S": 1})]
# S > 1.  last_rows: rows of the last slice that has any; empty: the slices behind it; single_group: S = 8 k + 1
SLICES = [
    Case(128, 128, 257, {"S": 2, "last_rows": 97, "last_tail": 1, "empty": []}),
    Case(128, 128, 2049, {"S": 9, "last_rows": 1, "last_tail": 1, "empty": [], "single_group": True}),
    Case(128, 128, 4097, {"S": 17, "last_rows": 1, "last_tail": 1, "empty": [], "single_group": True}),
    Case(128, 128, 6145, {"S": 25, "last_rows": 1, "last_tail": 1, "empty": [], "single_group": True}),
    Case(128, 128, 8200, {"S": 32, "last_rows": 136, "last_tail": 8, "empty": [29, 30, 31]}),
    Case(512, 512, 9856, {"S": 32, "last_rows": 256, "last_tail": 32, "empty": [31]}),       # text out_proj, 128 captions
    Case(768, 768, 9600, {"S": 14, "last_rows": 448, "last_tail": 32, "empty": []}),         # a shipped visual shape
]
SCALE = [Case(128, 256, 200, {"S": 1}), Case(128, 128, 257, {"S": 2})]
SCALES = (2.0 ** -20, 1.0, 8.0, 2.0 ** 100, None)             # None: a NULL scale_dev
# The bias gradient folded into the reduce launch.  One slice at up to 1,000 rows needs more than 256 output tiles (the plan
# wants two workgroups per CU before it stops cutting the rows): 17 x 17 tiles.  chunks = 64-row tiles of dY.
BIAS_ONE = [Case(2176, 2176, M, {"S": 1, "chunks": ch})
            for M, ch in ((1, 1), (63, 1), (64, 1), (65, 2), (500, 8), (513, 9), (1000, 16))]
BIAS_SLICED = [Case(128, 128, 257, {"S": 2, "chunks": 5}), Case(128, 128, 2049, {"S": 9, "chunks": 33})]
# float operands, per element: the slice-table shapes with at most 2,049 rows
FLOAT = [c for c in SLICES if c.M <= 2049]

GROUPS = {"depth": DEPTH, "tail": TAIL, "placement": PLACEMENT, "slices": SLICES, "scale": SCALE, "bias_one": BIAS_ONE,
          "bias_sliced": BIAS_SLICED}
LATTICE_CASES = [c for g in ("depth", "tail", "placement", "slices", "bias_one") for c in GROUPS[g]]


# ---------------------------------------------------------------------------------------------------- the work split

def _cdiv_trunc(a, b):
    """C's integer division (towards zero): what the kernel computes for the stage count of an empty slice."""
    return int(a / b) if a < 0 else a // b


def plan(M, S):
    """The documented split of M rows into S slices: rows_per_slice = ceil(ceil(M / 32) / S) * 32; per slice
    (m_begin, m_end, nk, tail_rows) with nk the number of 32-row stages and tail_rows the valid rows of the last one.  A slice
    that starts behind the last row is empty: m_end = M <= m_begin and nk <= 0."""
    steps = -(-M // BK)
    rps = -(-steps // S) * BK
    out = []
    for s in range(S):
        m_begin = s * rps
        m_end = min(M, m_begin + rps)
        nk = _cdiv_trunc(m_end - m_begin + BK - 1, BK)
        out.append((m_begin, m_end, nk, (m_end - m_begin) - (nk - 1) * BK))
    return rps, out


def properties(M, S):
    """What the case table names, derived from a slice count S."""
    rps, sl = plan(M, S)
    live = [i for i, (b, e, nk, t) in enumerate(sl) if e > b]
    last = sl[live[-1]]
    return {"S": S, "rows_per_slice": rps, "nk": sl[0][2], "tail": sl[0][3], "nks": [s[2] for s in sl],
            "last_rows": last[1] - last[0], "last_tail": last[3], "empty": [i for i in range(S) if i not in live],
            "single_group": S > 1 and S % 8 == 1, "chunks": -(-M // 64)}


def slices_from_workspace_bytes(nbytes, N1, N2):
    """S as cc_wgrad_tn_workspace_bytes reports it: S partial copies of dW, or 256 bytes for one slice."""
    if nbytes == 256:
        return 1
    assert nbytes % (4 * N1 * N2) == 0 and nbytes > 0, nbytes
    return nbytes // (4 * N1 * N2)


# ---------------------------------------------------------------------------------------------------- operands

_ROW_DY = np.array([1, -2, 1, 2, -1, 1, -2])                  # period 7
_ROW_X = np.array([1, 2, -1, 1, -2])                          # period 5: the pair has period 35, coprime to 32


def lattice(c, seed=0):
    """dY [M, N1], X [M, N2] as fp16 integers in {+-1, +-2, +-4}: seeded draws from {+-1, +-2} times a row pattern whose
    period is coprime to the 32-row stage.  No entry is zero, so a doubled or dropped row changes every element of dW; the
    two matrices are drawn independently (a transposed square tile cannot pass)."""
    rng = np.random.default_rng([seed, c.N1, c.N2, c.M])
    vals = np.array([-2, -1, 1, 2])
    m = np.arange(c.M)
    dy = rng.choice(vals, (c.M, c.N1)) * _ROW_DY[m % 7][:, None]
    x = rng.choice(vals, (c.M, c.N2)) * _ROW_X[m % 5][:, None]
    return dy.astype(np.float16), x.astype(np.float16)


def heavy_tailed(c, seed=1):
    """Recipe one: (dY fp32, X fp16).  dY: log-normal magnitudes (sigma 1.5, clipped to e^-3 .. e^4) with random signs times
    1e-3, every seventh row 30 times louder, column 5 quieter by 2^-10 - a range of 3.4e7, so that the fp16 copy scaled to
    8,192 .. 16,384 holds no subnormal.  X: unit Gaussians, four channels 100 times the rest."""
    rng = np.random.default_rng([seed, c.N1, c.N2, c.M])
    mag = np.exp(np.clip(1.5 * rng.standard_normal((c.M, c.N1)), -3.0, 4.0))
    dy = mag * rng.choice([-1.0, 1.0], (c.M, c.N1)) * 1e-3
    dy[::7] *= 30.0
    dy[:, 5] *= 2.0 ** -10
    x = rng.standard_normal((c.M, c.N2))
    x[:, [3, 64, 77, c.N2 - 1]] *= 100.0
    return dy.astype(np.float32), x.astype(np.float16)


def cancelling(c, seed=2):
    """Recipe two: (dY fp16, X fp16).  The contraction runs over the rows, so the pairs are row pairs: rows 2 k and 2 k + 1
    of dY have equal magnitudes and opposite signs, the two rows of X are equal up to a relative 2^-9 - every entry of dW is
    a sum of terms that cancel pair by pair, |dW| << sum |terms|."""
    rng = np.random.default_rng([seed, c.N1, c.N2, c.M])
    half = -(-c.M // 2)
    a = (1.0 + np.abs(rng.standard_normal((half, c.N1)))) * rng.choice([-1.0, 1.0], (half, c.N1))
    b = (1.0 + np.abs(rng.standard_normal((half, c.N2)))) * rng.choice([-1.0, 1.0], (half, c.N2))
    dy = np.repeat(a, 2, axis=0)[:c.M]
    dy[1::2] *= -1.0
    x = np.repeat(b, 2, axis=0)[:c.M]
    x[1::2] *= 1.0 + 2.0 ** -9 * rng.standard_normal(x[1::2].shape)
    return dy.astype(np.float16), x.astype(np.float16)


# ---------------------------------------------------------------------------------------------------- references

def exact(dy, x, scale=None):
    """dY^T X / scale in float64 on the given operands."""
    ref = dy.astype(np.float64).T @ x.astype(np.float64)
    return ref if scale is None else ref / scale


def exact_int(dy, x):
    return dy.astype(np.int64).T @ x.astype(np.int64)


def bound(dy, x, scale=None):
    """Per element: exact fp16 products, at most M - 1 fp32 additions in any order."""
    b = dy.shape[0] * U * (np.abs(dy.astype(np.float64)).T @ np.abs(x.astype(np.float64)))
    return b if scale is None else b / scale


# ---------------------------------------------------------------------------------------------------- the emulation

MUTANTS = {                                    # name: the case(s) of the table that must reject it
    "tail_not_cleared": [TAIL[0]],
    "tail_boundary_off_by_one": [TAIL[16]],                      # the entry (g, h, e) = (2, 0, 1): row 17 of the stage
    "last_stage_dropped": [DEPTH[0], DEPTH[3]],
    "empty_slice_adds_last_row": [SLICES[4]],
    "reduce_drops_ninth_slice": [SLICES[1]],
    "chunks_swapped": [PLACEMENT[0]],
    "tile_transposed": [PLACEMENT[3], PLACEMENT[0]],
    "t1_t2_swapped": [PLACEMENT[3]],
    "bias_segment_off_by_one": [BIAS_ONE[3]],
}
OFF_BY_ONE_ROW = 17                            # 8 g + 4 h + e of the mutated entry


def swz(m):
    return 2 * ((m & 3) | (((m >> 3) & 1) << 2))


def _lds_gather(mutant):
    """[32 rows][16 chunks] -> the source chunk a fragment read of chunk c receives.  The writer puts chunk p ^ swz(m) at
    position p (the swizzle on the source side), the reader fetches position c ^ swz(m): the identity.  chunks_swapped: on
    rows with (m >> 3) & 1 the writer exchanges chunks 0 and 8."""
    m = np.arange(BK)[:, None]
    pos = np.arange(16)[None, :] ^ swz(m)                        # position the reader fetches for chunk c
    src = pos ^ swz(m)                                           # chunk the writer put there
    if mutant == "chunks_swapped":
        odd = ((m >> 3) & 1) == 1
        src = np.where(odd & (src == 0), 8, np.where(odd & (src == 8), 0, src))
    return src


def _through_lds(rows, gather):
    """rows [32, n * 128] -> what the fragment reads return, per 128-column tile of 16 chunks of 8 halves."""
    t = rows.reshape(BK, -1, 16, 8)
    return np.take_along_axis(t, gather[:, None, :, None], axis=2).reshape(BK, -1)


def emulate(dy, x, S, scale=None, mutant=None):
    """dW fp32 as the documented work split computes it (fp32 accumulation per stage; on a lattice every order is exact).
    mutant: one of MUTANTS (the bias one is bias_emulate's)."""
    M, N1 = dy.shape
    N2 = x.shape[1]
    rps, slices = plan(M, S)
    gather = _lds_gather(mutant)
    r = np.arange(BK)
    partial = np.zeros((S, N1, N2), np.float32)
    for s, (m_begin, m_end, nk, tail_rows) in enumerate(slices):
        acc = partial[s]
        stages = list(range(max(nk, 0)))
        if mutant == "last_stage_dropped":
            stages = stages[:-1]
        if mutant == "empty_slice_adds_last_row" and m_end <= m_begin:        # a stage fetched from m_end - 1 < m_begin
            acc += np.outer(dy[m_end - 1], x[m_end - 1]).astype(np.float32)
        for kt in stages:
            rows = np.minimum(m_begin + kt * BK + r, m_end - 1)               # padding rows re-read the slice's last row
            ty = _through_lds(dy[rows].astype(np.float32), gather)
            tx = _through_lds(x[rows].astype(np.float32), gather)
            if kt == nk - 1 and tail_rows < BK:                               # ... and are cleared in the X fragments
                keep = r < tail_rows
                if mutant == "tail_not_cleared":
                    keep = r >= 0
                elif mutant == "tail_boundary_off_by_one":
                    keep[OFF_BY_ONE_ROW] = OFF_BY_ONE_ROW < tail_rows + 1
                tx = tx * keep[:, None]
            acc += ty.T @ tx
    inv = np.float32(1.0) / np.float32(scale) if scale is not None else np.float32(1.0)
    if S == 1:
        dw = partial[0] * inv
    else:
        total = np.zeros((N1, N2), np.float32)
        for s0 in range(0, S, 8):                                             # groups of eight, in slice order
            for s in range(s0, min(S, s0 + 8)):
                if not (mutant == "reduce_drops_ninth_slice" and s == 8):
                    total += partial[s]
        dw = total * inv
    if mutant == "tile_transposed":
        dw = dw.reshape(N1 // BN, BN, N2 // BN, BN).transpose(0, 3, 2, 1).reshape(N1, N2)
    elif mutant == "t1_t2_swapped":                                           # tile (t1, t2) computed from the columns of (t2, t1)
        assert N1 == N2
        dw = dw.reshape(N1 // BN, BN, N2 // BN, BN).transpose(2, 1, 0, 3).reshape(N1, N2)
    return np.ascontiguousarray(dw)


def bias_emulate(dy32, mutant=None):
    """The bias gradient as the reduce launch adds it: one partial sum per 64 rows of dY (cc_cast_transpose_f16), eight
    segments of ceil(chunks / 8) chunks each added in chunk order, then the segment sums in segment order."""
    M, C = dy32.shape
    chunks = -(-M // 64)
    part = [dy32[64 * i: 64 * i + 64].sum(0, dtype=np.float32) for i in range(chunks)]
    per = -(-chunks // 8)
    red = []
    for seg in range(8):
        i0 = seg * per
        i1 = min(chunks, i0 + per + (1 if mutant == "bias_segment_off_by_one" else 0))
        s = np.zeros(C, np.float32)
        for i in range(i0, i1):                                                # (i1 < i0 behind the last chunk: nothing)
            s += part[i]
        red.append(s)
    t = red[0].copy()
    for k in range(1, 8):
        t += red[k]
    return t


def existing_max_norm_measure(dw, ref, M):
    """The measure of test_weight_gradient_without_transposed_copies: (largest error, what it allows)."""
    return float(np.abs(dw.astype(np.float64) - ref).max()), 2e-6 * M ** 0.5 * float(np.abs(ref).max()) / max(1.0, M ** 0.5 / 8) + 1e-4


def is_power_of_two(v):
    m, _ = math.frexp(v)
    return v > 0 and m == 0.5
