"""Plain restatements shared by tests/test_metrics_ops_host.py and tests/test_metrics_ops_gpu.py: the rank counts, the
per-group row maxima, CrossEn and the LayerNorm + projection head, written from their definitions (utils/metrics.py:11-26,
38-76; modules/losses.py:8-18; ln_post / ln_final followed by the projection, modules/clip.py) in NumPy - comparisons on the
fp32 values themselves, arithmetic in float64 - plus the running-error bounds the GPU tests hold the fp32 kernels to and a
bit-level emulation of the float maximum that group_max_rows publishes with integer atomics.  No project imports."""
import math

import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32
ULP = 2.0 ** -23                    # relative size of one fp32 ulp (at most)
TINY = 2.0 ** -126                  # smallest normal fp32 number: below it no relative bound holds
LIBM_ULPS = 2.0                     # ASSUMED error of the device expf / logf, in ulps (HIP documents 1; not measured here)
SAFETY = 2.0                        # over the whole bound, for what a first-order analysis leaves out


# ------------------------------------------------------------------------------------------------ rank counts
def rank_counts_ref(sim, g_or_vals):
    """sim [R, C] fp32; g_or_vals [R]: integers = the ground-truth column of every row, floats = the value to rank against.
    -> (#greater, #equal, #equal in front of g) per row, int64 [R] each (the third is 0 where a value was handed in).
    IEEE comparisons on fp32: a NaN compares false with everything (a NaN truth gives 0, 0, 0), -0.0 == +0.0."""
    s = np.asarray(sim, dtype=np.float32)
    R, C = s.shape
    q = np.asarray(g_or_vals)
    by_col = q.dtype.kind in "iu"
    gt, eq, front = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    for i in range(R):
        d = s[i, int(q[i])] if by_col else np.float32(q[i])
        for j in range(C):
            v = s[i, j]
            if v > d:
                gt[i] += 1
            if v == d:
                eq[i] += 1
                if by_col and j < int(q[i]):
                    front[i] += 1
    return gt, eq, front


def ranks_from_counts(gt, eq):
    """compute_metrics' `ind` (utils/metrics.py:11-26): every sorted position that holds the truth value, row after row."""
    return np.concatenate([np.arange(a, a + b) for a, b in zip(gt, eq)]) if len(gt) else np.zeros(0, np.int64)


# ------------------------------------------------------------------------------------------------ group maxima
def group_max_ref(sim, group, n_groups):
    """-> float64 [n_groups, C]: the maximum over the rows r with group[r] == g of sim[r, :], NaN entries ignored, rows whose
    id lies outside [0, n_groups) ignored, -inf where nothing is left."""
    s = np.asarray(sim, dtype=np.float32)
    out = np.full((int(n_groups), s.shape[1]), -np.inf)
    for r, g in enumerate(np.asarray(group).tolist()):
        if 0 <= g < n_groups:
            for c in range(s.shape[1]):
                v = float(s[r, c])
                if v == v and v > out[g, c]:
                    out[g, c] = v
    return out


def _ordered_max_bits(stored, v):
    """One publication of the FIXED atomic_max_f32 on uint32 bit patterns: by the sign bit of v, a signed-integer max
    (sign bit clear) or an unsigned-integer min (sign bit set) of the two patterns."""
    stored, v = int(stored) & 0xFFFFFFFF, int(v) & 0xFFFFFFFF
    signed = lambda b: b - (1 << 32) if b & 0x80000000 else b
    if not v & 0x80000000:
        return v if signed(v) > signed(stored) else stored
    return min(stored, v)


def _unfixed_max_bits(stored, v):
    """The same publication routed by `v >= 0.f`, as the kernel did before: -0.0 takes the signed-integer branch."""
    stored, v = int(stored) & 0xFFFFFFFF, int(v) & 0xFFFFFFFF
    signed = lambda b: b - (1 << 32) if b & 0x80000000 else b
    if float(np.array(v, np.uint32).view(np.float32)) >= 0.0:
        return v if signed(v) > signed(stored) else stored
    return min(stored, v)


def emulated_max(values, fixed=True):
    """fp32 values published one after the other into a cell that holds -inf -> the fp32 value left in the cell."""
    cell = int(np.array(-np.inf, np.float32).view(np.uint32))
    step = _ordered_max_bits if fixed else _unfixed_max_bits
    for v in values:
        cell = step(cell, int(np.array(v, np.float32).view(np.uint32)))
    return np.array(cell, np.uint32).view(np.float32)[()]


# ------------------------------------------------------------------------------------------------ CrossEn
def _nce_rows64(s, drop_last=False):
    """float64 [n, n] -> nce_i = logsumexp(row i) - s_ii; drop_last leaves the last column out of every row sum (a
    deliberately wrong reference: what a lane loop that stops one element early computes)."""
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    if drop_last:
        e = e[:, :-1]
    return np.log(e.sum(axis=1)) + m[:, 0] - np.diag(s)


def crossen_ref(sim, drop_last=False):
    """sim [n, n] -> float64 (mean row nce, mean column nce, their mean): CrossEn(sim), CrossEn(sim.T) and the symmetric
    loss from a float64 log-softmax of the values given."""
    s = np.asarray(sim, dtype=np.float64)
    l1, l2 = _nce_rows64(s, drop_last).mean(), _nce_rows64(s.T.copy(), drop_last).mean()
    return np.array([l1, l2, (l1 + l2) / 2])


def crossen_bound(sim):
    """A-priori running-error bound (float64, [3]) of cc_contrastive_loss_f32's outputs on the fp32 matrix `sim`, from the
    kernel's own chains.  Per row (cross_entropy_rows_kernel; a column is a row through the strides):
      * the maximum mx is exact;
      * t_j = x_j - mx rounds once: |t_j| U on the exponent = that much relative on exp(t_j); expf costs LIBM_ULPS ulps; a
        term below the smallest normal number is off by at most TINY absolutely;
      * s = the sum of ceil(n / 64) lane-strided terms and a 6-level tree: at most ceil(n / 64) + 6 additions of positive
        numbers, each U of a partial sum <= s;
      -> relative error ds of s; log(s) moves by -log(1 - ds), logf adds LIBM_ULPS ulps of |log s|;
      * (log s + mx) - x_i: two roundings, U |log s + mx| and U |nce_i|.
    The mean (contrastive_mean_kernel): a thread adds ceil(n / 256) terms, the wave tree 6 levels, the four waves 2 more ->
    ceil(n / 256) + 8 additions of (non-negative) terms, the division by n one rounding; (l1 + l2) / 2 one more.
    Everything times SAFETY."""
    s = np.asarray(sim, dtype=np.float64)
    n = s.shape[0]
    add_s, add_m = math.ceil(n / 64) + 6, math.ceil(n / 256) + 8

    def side(x):
        m = x.max(axis=1, keepdims=True)
        t = x - m
        e = np.exp(t)
        tot = e.sum(axis=1)
        ds = ((np.abs(t) * U + LIBM_ULPS * ULP) * e).sum(axis=1) / tot + n * TINY / tot + add_s * U
        lg = np.log(tot)
        nce = lg + m[:, 0] - np.diag(x)
        err = -np.log1p(-ds) + LIBM_ULPS * ULP * np.abs(lg) + U * np.abs(lg + m[:, 0]) + U * np.abs(nce)
        mean = nce.mean()
        return mean, (err.sum() + add_m * U * np.abs(nce).sum()) / n + U * abs(mean)
    (l1, b1), (l2, b2) = side(s), side(s.T.copy())
    b3 = (b1 + b2) / 2 + U * abs(l1 + l2) / 2
    return SAFETY * np.array([b1, b2, b3])


# ------------------------------------------------------------------------------------------------ LayerNorm + projection
def head_project_ref(h, row_of, gamma, beta, proj, eps=1e-5, drop_last_k=False):
    """h [N, W], row_of [R] row numbers, gamma / beta [W], proj [W, E] -> float64 [R, E] = LayerNorm(h[row_of]) @ proj with the
    biased variance and eps inside the root.  drop_last_k leaves the last channel out of the dot product (a deliberately
    wrong reference: a k-slice that stops one element early)."""
    x = np.asarray(h, dtype=np.float64)[np.asarray(row_of, dtype=np.int64)]
    g, b, p = (np.asarray(a, dtype=np.float64) for a in (gamma, beta, proj))
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    y = (x - mean) / np.sqrt(var + eps) * g + b
    return y[:, :-1] @ p[:-1] if drop_last_k else y @ p


def head_project_bound(h, row_of, gamma, beta, proj, eps=1e-5):
    """A-priori running-error bound (float64, [R, E]) of head_project_kernel's outputs, from its chains (W channels, 256
    threads, 16 k-slices):
      * mean: a thread adds ceil(W / 256) terms, the wave tree 6 levels, the four waves 3 additions, the division one
        rounding -> |c| <= dm = (ceil(W / 256) + 10) U mean|x| for the error c of the mean.  c is the SAME for every channel
        of the row, so it shifts every normalised value by c * rstd and the output by c * rstd * sum_w gamma_w proj_we - a
        signed sum; this is the term that counts for rows whose mean is large against their spread;
      * d = x - mean rounds once; the variance about the shifted mean is var + c^2 exactly (the deviations sum to zero),
        summed as the mean was with two more roundings per term (the difference, the square); + eps, sqrtf, the division
        (one rounding each, 2 U allowed for the root), the product d * rstd:
        each normalised value to  k_hat U |x_hat|,  k_hat = (ceil(W / 256) + 12) / 2 + 6  ("a few ulp"), plus c^2 / (2 (var + eps));
      * y = x_hat * gamma + beta: two roundings (one where the compiler fuses);
      * the dot: a k-slice adds ceil(W / 16) fused terms, 16 partials are added in order: ceil(W / 16) + 16 roundings of
        partial sums <= sum_w |y_w| |proj_we|.
    Everything times SAFETY."""
    x = np.asarray(h, dtype=np.float64)[np.asarray(row_of, dtype=np.int64)]
    g, b, p = (np.asarray(a, dtype=np.float64) for a in (gamma, beta, proj))
    W = x.shape[1]
    chain = math.ceil(W / 256)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    y = xh * g + b
    dm = (chain + 10) * U * np.abs(x).mean(axis=1, keepdims=True)                      # |c| <=
    k_hat = (chain + 12) / 2 + 6
    e_xh = np.abs(xh) * (k_hat * U + dm ** 2 / (2 * (var + eps)))                      # per channel, the common shift apart
    e_y = np.abs(g) * e_xh + U * np.abs(xh * g) + U * np.abs(y)
    shift = dm * rstd * np.abs(g[None, :] @ p)                                          # [R, E]
    dot = (math.ceil(W / 16) + 16) * U * (np.abs(y) @ np.abs(p))
    return SAFETY * (shift + e_y @ np.abs(p) + dot)


# ------------------------------------------------------------------------------------------------ seeded inputs
def loss_case(n, scale, seed=0):
    """fp32 [n, n] logits = scale * cos: cos uniform in [-1, 1], the diagonal planted in [0.95, 1] (matching pairs)."""
    rng = np.random.default_rng(7000 + 13 * n + int(scale) + seed)
    cos = rng.uniform(-1.0, 1.0, size=(n, n))
    cos[np.arange(n), np.arange(n)] = 1.0 - 0.05 * rng.uniform(size=n)
    return (scale * cos).astype(np.float32)


def head_case(W, E, R, seed=0, row_mul=1, with_idx=False, mean=0.0, std=1.0, gamma_zero=False):
    """-> dict(h [N, W], row_of [R], row_idx [R] int32 or None, gamma, beta [W], proj [W, E]) fp32, rows ~ N(mean, std^2);
    row_of[r] = r * row_mul + row_idx[r] as the kernel addresses them."""
    rng = np.random.default_rng(8000 + W + 7 * E + 31 * R + seed)
    N = R * row_mul + (3 if with_idx else 0)
    h = (mean + std * rng.standard_normal((N, W))).astype(np.float32)
    gamma = (1.0 + 0.2 * rng.standard_normal(W)).astype(np.float32)
    if gamma_zero:
        gamma[rng.permutation(W)[: W // 2]] = 0.0
    beta = (0.1 * rng.standard_normal(W)).astype(np.float32)
    proj = (rng.standard_normal((W, E)) * W ** -0.5).astype(np.float32)
    row_idx = rng.integers(0, 4, size=R).astype(np.int32) if with_idx else None
    row_of = np.arange(R) * row_mul + (row_idx if with_idx else 0)
    assert int(row_of.max()) < N
    return dict(h=h, row_of=row_of, row_idx=row_idx, row_mul=row_mul, gamma=gamma, beta=beta, proj=proj)
