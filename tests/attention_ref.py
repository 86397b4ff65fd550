"""Float64 reference, a-priori error bounds, input recipes and a numpy emulation for the matrix-core attention kernels
(attention_wave_kernel / attention_kernel of transformer.hip, attention_long_kernel, the in_proj + attention epilogue of
gemm.hip, and the backward kernels of backward.hip).  Pure numpy / torch-CPU: importable without a GPU.

Layout everywhere: qkv16 is a numpy float16 array [rows, 3 W], W = heads * 64; token t of sequence s is row offs[s] + t and
has lens[s] tokens; head h owns columns h*64 .. h*64+63 of each of the q | k | v thirds.  Outputs are [rows, W] (forward)
and [rows, 3 W] (backward); rows outside every sequence are 0 in references and bounds.

The documented arithmetic (kernel headers)
------------------------------------------
resident (wave and workgroup kernels, the fused form): S = q k^T as an fp32 MFMA sum of 64 exact fp16 products, times the
  exact factor 1/8; m = row max; e_j = __expf(S_j - m); l = fp32 sum of e_j; P_j = fp16(fp32(e_j * (1 / l))); O = fp32 MFMA
  sum of P_j v_j over the padded key tiles; y = fp16(O).  The fused form above 56 tokens rounds e_j itself to fp16 and
  multiplies O by 1 / l afterwards; its rounding error of P is the same 2^-11 relative and at most the same 2^-25 absolute.
streamed (long kernel): per 64-key tile t the running maximum m_t = max(m_{t-1}, tile max), alpha = __expf(m_{t-1} - m_t),
  e_j = __expf(S_j - m_t), l = l * alpha + sum of the UNROUNDED e_j, O = O * alpha + MFMA sum of fp16(e_j) v_j; y = fp16(O / l).
backward (per sequence and head): P in fp32 as above; s_o = 2^k with s_o max|dO| in [2^13, 2^14); dO16 = fp16(dO s_o);
  dP = dO16 v^T; D = sum_j P dP; dS = P (dP - D); s_s likewise from max|dS|; dS16 = fp16(dS s_s); P16 = fp16(P);
  dQ = dS16 k / (8 s_o s_s), dK = dS16^T q / (8 s_o s_s), dV = P16^T dO16 / s_o, all fp32 MFMA sums.  Above 64 tokens the
  scales are chosen per 64-query tile / per wave (finer, so never worse), and the key side rebuilds P = __expf(S - lse).

forward_bound: the terms, u = 2^-11, w = 2^-24, n = keys of the row, A_d = sum_j p_j |v_jd|
  E1  rounding of S: |dS_ij| <= 64 w sum_d |q_id k_jd| / 8 (64 fp32 additions of exact products; any order).  With dmax the
      largest such value over the row's keys every p_j moves by a factor within exp(+-2 dmax): E1 = expm1(2 dmax) A_d.
  E2  __expf = v_exp_f32(x log2 e): the fp32 subtraction S - m (w |x|), the rounded constant and product (2 w |x|) and the
      instruction's own 1 ulp (2 w); counted as eps(x) = (4 |x| + 4) w, at most 1 (a flushed result).  It acts on the
      numerator and, through l, on every key: E2 = sum_j p_j eps_j |v_jd| + (sum_j p_j eps_j) A_d.  Streamed: x is taken
      against the running maximum of the key's tile, and each later replacement of the maximum multiplies the earlier keys by
      a rounded alpha: eps_j += sum over later tiles of (4 |m_t - m_{t-1}| + 6) w.
  E3  l (n fp32 additions), 1 / l and the product with it: (n + 4) w A_d.
  E4  P to fp16: max(u p_j, 2^-25) per key (2^-11 relative for normal values; half the subnormal quantum 2^-24 otherwise).
      Streamed: the rounded value is exp(S_j - m_t), so the absolute floor is 2^-25 exp(m_t - m) / l in units of p.
      E4 = sum_j that |v_jd|.
  E5  fp32 accumulation of P V over the padded keys (n rounded up to 64) and, streamed, two roundings per tile for the
      rescaling of O and l: (n_pad + 2 tiles) w A_d.
  E6  the output's fp16 rounding: max(u (|y| + E1..5), 2^-25).
  bound = 1.05 (E1 + .. + E5) + E6; the factor 1.05 pays for products of two first-order terms (the largest single term here is
  below 3 % of A_d).

backward_bound: the same quantities carried through the chain rule, per (sequence, head) and per element
  eO_id  = u |dO_id| + 2^-38 max_head|dO|            (2^-25 / s_o with s_o >= 2^13 / max|dO|: entries that flush)
  eP_ij  = sum_d eO_id |v_jd| + 64 w sum_d |dO_id v_jd|
  ep_ij  = relative error of the fp32 P: eps_ij + sum_k p_ik eps_ik + expm1(2 dmax_i) + (n + 4) w + 4 w (|m_i| + ln n + 1)
           (the last term: the key side's log-sum-exp, stored in fp32)
  eD_i   = sum_j p_ij (eP_ij + ep_ij |dP_ij|) + (n + 1) w sum_j p_ij |dP_ij|
  eS_ij  = p_ij (eP_ij + eD_i) + (ep_ij + 2 w) |dS_ij|, then fp16: + u (|dS_ij| + eS_ij) + 2^-38 max_head|dS|
  dQ_id: sum_j eS_ij |k_jd| / 8 + (n + 64) w sum_j |dS_ij k_jd| / 8;   dK_jd: the same over i with q
  dV_jd: sum_i [(max(u p_ij, 2^-25) + ep_ij p_ij) (|dO_id| + eO_id) + p_ij eO_id] + (n + 64) w sum_i p_ij |dO_id|
  each times 1.05 for the second-order products.
"""
import numpy as np

U = 2.0 ** -11
W24 = 2.0 ** -24
FLOOR = 2.0 ** -25
SLACK = 1.05
FORMS = ("resident", "streamed")
RECIPES = ("peaked", "ascending", "descending", "extreme", "floor", "uniform_coded", "loud_neighbour")
FORWARD_MUTANTS = ("drop_last_key", "double_key", "stale_max", "neighbour_leak", "swap_norm", "causal_off_by_one")
BACKWARD_MUTANTS = ("launch_scale",)


def uniform_layout(nseq, L):
    return [L] * nseq, [s * L for s in range(nseq)]


def _heads_of(qkv16, off, n, heads, dtype):
    """-> q, k, v [heads, n, 64] of the sequence at rows off .. off + n."""
    x =np.asarray(qkv16[off:off + n]).astype(dtype).reshape(n, 3, heads, 64)
    return x[:, 0].transpose(1, 0, 2), x[:, 1].transpose(1, 0, 2), x[:, 2].transpose(1, 0, 2)


def _mask(n, causal, shift=0):
    """True where key j is visible to query i."""
    if not causal:
        return np.ones((n, n), dtype=bool)
    return np.arange(n)[None, :] <= np.arange(n)[:, None] + shift


def _softmax64(q, k, causal):
    n = q.shape[0]
    s = q @ k.T / 8.0
    s = np.where(_mask(n, causal), s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    return s, m, e / e.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------- reference
def attention_float64(qkv16, lens, offs, heads, causal):
    W = heads * 64
    out = np.zeros((qkv16.shape[0], W))
    for n, off in zip(lens, offs):
        q, k, v = _heads_of(qkv16, off, n, heads, np.float64)
        for h in range(heads):
            _, _, p = _softmax64(q[h], k[h], causal)
            out[off:off + n, h * 64:(h + 1) * 64] = p @ v[h]
    return out


def attention_backward_float64(qkv16, d_out, lens, offs, heads, causal):
    """d_qkv [rows, 3 W] float64 from torch.autograd in float64 on the same fp16 q, k, v and the fp32 d_out."""
    import torch
    W = heads * 64
    out = np.zeros((qkv16.shape[0], 3 * W))
    for n, off in zip(lens, offs):
        x = torch.from_numpy(np.asarray(qkv16[off:off + n]).astype(np.float64)).view(n, 3, heads, 64).permute(1, 2, 0, 3)
        x = x.detach().clone().requires_grad_(True)
        sc = x[0] @ x[1].transpose(-1, -2) / 8.0
        if causal:
            sc = sc + torch.full((n, n), float("-inf"), dtype=torch.float64).triu_(1)
        y = (sc.softmax(dim=-1) @ x[2]).permute(1, 0, 2).reshape(n, W)
        (y * torch.from_numpy(np.asarray(d_out[off:off + n]).astype(np.float64))).sum().backward()
        out[off:off + n] = x.grad.permute(2, 0, 1, 3).reshape(n, 3 * W).numpy()
    return out


# -------------------------------------------------------------------------------------------------------------- bounds
def _running_max(s):
    """s [n, n] with -inf at masked keys -> (m_t at each key's tile [n, n], per-tile running maxima [n, tiles])."""
    n = s.shape[0]
    nt = (n + 63) // 64
    pad = np.full((n, nt * 64), -np.inf)
    pad[:, :n] = s
    run = np.maximum.accumulate(pad.reshape(n, nt, 64).max(axis=2), axis=1)
    return np.repeat(run, 64, axis=1)[:, :n], run


def _softmax_terms(q, k, causal, form):
    """-> s, m, p, eps (relative error of the exponentials), dmax (rounding of S, per row), floor_scale (E4's absolute floor
    in units of p), tiles."""
    n = q.shape[0]
    s, m, p = _softmax64(q, k, causal)
    vis = _mask(n, causal)
    delta = np.where(vis, 64.0 * W24 * (np.abs(q) @ np.abs(k).T) / 8.0, 0.0)
    dmax = delta.max(axis=1, keepdims=True)
    tiles = (n + 63) // 64
    if form == "resident":
        x = np.where(vis, s - m, 0.0)
        eps = (4.0 * np.abs(x) + 4.0) * W24
        floor_scale = np.ones_like(p)
    else:
        m_key, run = _running_max(s)
        x = np.where(vis, s - m_key, 0.0)
        eps = (4.0 * np.abs(x) + 4.0) * W24
        upd = np.zeros_like(run)
        upd[:, 1:] = (4.0 * np.abs(run[:, 1:] - run[:, :-1]) + 6.0) * W24
        later = upd.sum(axis=1, keepdims=True) - np.cumsum(upd, axis=1)
        eps = eps + np.repeat(later, 64, axis=1)[:, :n]
        l = np.exp(np.where(vis, s - m, -np.inf)).sum(axis=1, keepdims=True)
        floor_scale = np.exp(m_key - m) / l
    eps = np.where(vis, np.minimum(eps, 1.0), 0.0)
    return s, m, p, eps, dmax, np.where(vis, floor_scale, 0.0), tiles


def _forward_bound_head(q, k, v, causal, form):
    n = q.shape[0]
    s, m, p, eps, dmax, floor_scale, tiles = _softmax_terms(q, k, causal, form)
    av = np.abs(v)
    A = p @ av
    e1 = np.expm1(2.0 * dmax) * A
    pe = p * eps
    e2 = pe @ av + pe.sum(axis=1, keepdims=True) * A
    e3 = (n + 4.0) * W24 * A
    e4 = np.maximum(U * p, FLOOR * floor_scale) @ av
    e5 = (64.0 * tiles + (2.0 * tiles if form == "streamed" else 0.0)) * W24 * A
    ey = e1 + e2 + e3 + e4 + e5
    e6 = np.maximum(U * (np.abs(p @ v) + ey), FLOOR)
    return SLACK * ey + e6


def forward_bound(qkv16, lens, offs, heads, causal, form):
    """Per-element bound on |kernel output - attention_float64| for the documented arithmetic of ``form``."""
    assert form in FORMS
    W = heads * 64
    out = np.zeros((qkv16.shape[0], W))
    for n, off in zip(lens, offs):
        q, k, v = _heads_of(qkv16, off, n, heads, np.float64)
        for h in range(heads):
            out[off:off + n, h * 64:(h + 1) * 64] = _forward_bound_head(q[h], k[h], v[h], causal, form)
    return out


def _backward_bound_head(q, k, v, do, causal):
    n = q.shape[0]
    s, m, p, eps, dmax, _, _ = _softmax_terms(q, k, causal, "resident")
    ado, av = np.abs(do), np.abs(v)
    dp = do @ v.T
    D = (p * dp).sum(axis=1, keepdims=True)
    ds = p * (dp - D)
    e_o = U * ado + 2.0 ** -38 * ado.max()
    e_dp = e_o @ av.T + 64.0 * W24 * (ado @ av.T)
    ep = eps + (p * eps).sum(axis=1, keepdims=True) + np.expm1(2.0 * dmax) + (n + 4.0) * W24 \
        + 4.0 * W24 * (np.abs(m) + np.log(n) + 1.0)
    e_D = (p * (e_dp + ep * np.abs(dp))).sum(axis=1, keepdims=True) + (n + 1.0) * W24 * (p * np.abs(dp)).sum(axis=1, keepdims=True)
    e_s = p * (e_dp + e_D) + (ep + 2.0 * W24) * np.abs(ds)
    e_s = e_s + U * (np.abs(ds) + e_s) + 2.0 ** -38 * np.abs(ds).max()
    acc = (n + 64.0) * W24
    e_q = e_s @ np.abs(k) / 8.0 + acc * (np.abs(ds) @ np.abs(k)) / 8.0
    e_k = e_s.T @ np.abs(q) / 8.0 + acc * (np.abs(ds).T @ np.abs(q)) / 8.0
    e_v = (np.maximum(U * p, np.where(_mask(n, causal), FLOOR, 0.0)) + ep * p).T @ (ado + e_o) + p.T @ e_o + acc * (p.T @ ado)
    return SLACK * e_q, SLACK * e_k, SLACK * e_v


def backward_bound(qkv16, d_out, lens, offs, heads, causal):
    """Per-element bound on |kernel d_qkv - attention_backward_float64| [rows, 3 W]; every (sequence, head) block depends on that
    head's own q, k, v and d_out only."""
    W = heads * 64
    out = np.zeros((qkv16.shape[0], 3 * W))
    for n, off in zip(lens, offs):
        q, k, v = _heads_of(qkv16, off, n, heads, np.float64)
        do = np.asarray(d_out[off:off + n]).astype(np.float64).reshape(n, heads, 64).transpose(1, 0, 2)
        for h in range(heads):
            parts = _backward_bound_head(q[h], k[h], v[h], do[h], causal)
            for part in range(3):
                out[off:off + n, part * W + h * 64:part * W + (h + 1) * 64] = parts[part]
    return out


def share_of_bound(err, bound):
    """Largest err / bound; an element with bound 0 must have err 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), "non-finite output inside a sequence"
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def head_blocks(x, lens, offs, heads, parts=1):
    """Yield ((sequence, head), block) for a [rows, parts * W] array: block is [parts, n, 64]."""
    W = heads * 64
    for s, (n, off) in enumerate(zip(lens, offs)):
        for h in range(heads):
            yield (s, h), np.stack([x[off:off + n, part * W + h * 64:part * W + (h + 1) * 64] for part in range(parts)])


# ------------------------------------------------------------------------------------------------------------- recipes
def _recipe_head(recipe, n, rng, seq):
    """q, k, v [n, 64] float16 of one head of sequence number ``seq``."""
    q = rng.standard_normal((n, 64))
    k = rng.standard_normal((n, 64))
    v = rng.standard_normal((n, 64))
    j = np.arange(n)
    if recipe == "gaussian":
        pass
    elif recipe == "peaked":
        # dimension c has one "special" key 20 e_c; query i points at special key i mod (their number): score 50 against |3|
        ns = min(n, 64)
        pos = rng.permutation(n)[:ns]
        pos[pos == n - 1] = pos[0]
        pos[0] = n - 1                                        # the last key (a ragged tile's edge) is somebody's peak
        if ns > 1:
            pos[pos == 0] = pos[1]
            pos[1] = 0 if n > 1 else pos[1]
        q, k = q * 0.25, k * 0.25
        k[pos] = 0.0
        k[pos, np.arange(ns)] = 20.0
        q[j, j % ns] = 20.0
    elif recipe in ("ascending", "descending"):
        q, k = q * 0.5, k * 0.5
        q[:, 0] = 4.0
        k[:, 0] = 0.75 * (j if recipe == "ascending" else (n - 1 - j))      # score 0.375 per key: 24 per 64-key tile
    elif recipe == "extreme":
        q = np.sign(q) * rng.uniform(10.0, 20.0, size=q.shape)
        k = np.sign(k) * rng.uniform(10.0, 20.0, size=k.shape)
        third = j[j % 3 == 0]
        q[third] = k[rng.integers(0, n, size=third.size)]     # aligned pairs: |score| about 64 * 225 / 8
    elif recipe == "floor":
        q[:] = 0.0
        q[:, 0] = 8.0
        k[:, 0] = np.array([-10.0, -12.0, -16.6, -18.0])[j % 4]
        k[(seq * 37) % n, 0] = 0.0
        v = v * 4.0
    elif recipe == "uniform_coded":
        q[:] = 0.0
        v[:] = 0.0
        v[j, j % 64] = 1 + j // 64
    elif recipe == "loud_neighbour":
        if seq % 2 == 0:                                      # quiet
            k = k * 0.1
            v = rng.uniform(-1.0, 1.0, size=v.shape)
        else:                                                 # loud
            k = np.sign(k) * 15.0
            v = np.sign(v) * 30000.0
    else:
        raise ValueError(recipe)
    return q.astype(np.float16), k.astype(np.float16), v.astype(np.float16)


def make_qkv(recipe, lens, offs, heads, seed, rows=None, fill=0.0):
    """qkv16 [rows, 3 W] float16 holding the recipe's sequences at their rows; every other row holds ``fill``."""
    W = heads * 64
    rows = max(o + n for n, o in zip(lens, offs)) if rows is None else rows
    out = np.full((rows, 3 * W), fill, dtype=np.float16)
    rng = np.random.default_rng([seed, RECIPES.index(recipe) if recipe in RECIPES else 99])
    for s, (n, off) in enumerate(zip(lens, offs)):
        for h in range(heads):
            q, k, v = _recipe_head(recipe, n, rng, s)
            for part, x in enumerate((q, k, v)):
                out[off:off + n, part * W + h * 64:part * W + (h + 1) * 64] = x
    return out


def make_d_out(lens, offs, heads, seed, rows=None):
    """fp32 d_out [rows, W]: Gaussian, the magnitude of (sequence s, head h) is 2^(-12 (heads s + h)): a factor 2^12 between
    the heads of a sequence and between neighbouring sequences."""
    W = heads * 64
    rows = max(o + n for n, o in zip(lens, offs)) if rows is None else rows
    rng = np.random.default_rng([seed, 4242])
    out = np.zeros((rows, W), dtype=np.float32)
    for s, (n, off) in enumerate(zip(lens, offs)):
        for h in range(heads):
            out[off:off + n, h * 64:(h + 1) * 64] = rng.standard_normal((n, 64)) * 2.0 ** (-12 * (heads * s + h))
    return out


def uniform_coded_expected(lens, offs, heads, causal, form, rows=None):
    """The exact fp16 output for the ``uniform_coded`` recipe, from the documented arithmetic.  All scores are 0, so every
    exponential is exactly 1 and l = n (the row's visible keys).  resident: P = fp16(fp32(1 / n)) and O[d] = P * (the sum of
    the codes 1 + j // 64 of the visible keys j = d mod 64) is exact in fp32 (an 11-bit P times an integer below 64), so
    y = fp16(O) whatever the order.  streamed: P = 1, O[d] = that integer, y = fp16(fp32(O * fp32(1 / n)))."""
    W = heads * 64
    rows = max(o + n for n, o in zip(lens, offs)) if rows is None else rows
    out = np.zeros((rows, W), dtype=np.float16)
    for n, off in zip(lens, offs):
        j = np.arange(n)
        code = np.zeros((n, 64), dtype=np.float32)
        code[j, j % 64] = 1 + j // 64
        csum = np.cumsum(code, axis=0) if causal else np.broadcast_to(code.sum(axis=0), (n, 64))
        nvis = (j + 1 if causal else np.full(n, n)).astype(np.float32)[:, None]
        inv = np.float32(1.0) / nvis
        y = (csum * inv.astype(np.float16).astype(np.float32)) if form == "resident" else (csum * inv)
        out[off:off + n] = np.tile(y.astype(np.float32).astype(np.float16), (1, heads))
    return out


# ----------------------------------------------------------------------------------------------------------- emulation
def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def _emulate_forward_head(q, k, v, causal, form, mutant, v_next):
    """q, k, v [n, 64] float32 (fp16 values).  fp32 numpy arithmetic in the documented order of roundings."""
    n = q.shape[0]
    vis = _mask(n, causal, 1 if mutant == "causal_off_by_one" else 0)
    if mutant == "drop_last_key":
        vis = vis.copy()
        vis[:, n - 1] = False
        vis[0, 0] = True
    s = (q @ k.T) * np.float32(0.125)
    s = np.where(vis, s, np.float32(-3.0e38)).astype(np.float32)
    twice = np.zeros(n, dtype=np.float32)
    if mutant == "double_key":
        twice[n - 1 - (n - 1) % 16] = 1.0                    # the first key of the last 16-key tile enters twice
    if form == "resident":
        m = s.max(axis=1, keepdims=True)
        e = np.where(vis, np.exp(s - m), np.float32(0)).astype(np.float32)
        e = e * (1 + twice)[None, :]
        l = e.sum(axis=1, keepdims=True, dtype=np.float32)
        inv = np.float32(1.0) / l
        if mutant == "swap_norm":
            o = (_f16(e) @ v).astype(np.float32) * inv
        else:
            o = (_f16(e * inv) @ v).astype(np.float32)
    else:
        m_run = np.full((n, 1), -3.0e38, dtype=np.float32)
        l_run = np.zeros((n, 1), dtype=np.float32)
        o = np.zeros((n, 64), dtype=np.float32)
        for t in range((n + 63) // 64):
            sl = slice(t * 64, min(n, t * 64 + 64))
            live = vis[:, sl].any(axis=1, keepdims=True)      # (causal: tiles behind the query tile are not visited)
            m_new = np.maximum(m_run, s[:, sl].max(axis=1, keepdims=True))
            alpha = np.where(m_run > -1.0e38, np.exp(m_run - m_new), np.float32(0)).astype(np.float32)
            if mutant == "stale_max":
                alpha = np.where(m_run > -1.0e38, np.float32(1), np.float32(0))
            e = np.where(vis[:, sl], np.exp(s[:, sl] - m_new), np.float32(0)).astype(np.float32) * (1 + twice[sl])[None, :]
            l_new = l_run * alpha + e.sum(axis=1, keepdims=True, dtype=np.float32)
            o_new = o * alpha + (_f16(e) @ v[sl]).astype(np.float32)
            m_run, l_run, o = np.where(live, m_new, m_run), np.where(live, l_new, l_run), np.where(live, o_new, o)
        if mutant == "swap_norm":                             # the resident rule: the normalised weights are what is rounded
            e = np.where(vis, np.exp(s - m_run), np.float32(0)).astype(np.float32)
            o = (_f16(e * (np.float32(1.0) / l_run)) @ v).astype(np.float32)
        else:
            o = o * (np.float32(1.0) / l_run)
    if mutant == "neighbour_leak" and v_next is not None:
        pad = (-n) % 64 if form == "streamed" else (-n) % 32  # the padding keys of the last tile
        pad = min(pad, v_next.shape[0])
        o = o + np.float32(1e-6) * v_next[:pad].sum(axis=0, dtype=np.float32)[None, :]
    return o.astype(np.float16)


def emulate_forward(qkv16, lens, offs, heads, causal, form, mutant=None):
    """The documented arithmetic in numpy (fp32 sums, fp16 P and output) -> [rows, W] float16.  ``mutant``: one of
    FORWARD_MUTANTS, a deliberately wrong variant the bound (or the bit-exact case) must reject."""
    assert form in FORMS and (mutant is None or mutant in FORWARD_MUTANTS)
    W = heads * 64
    out = np.zeros((qkv16.shape[0], W), dtype=np.float16)
    for i, (n, off) in enumerate(zip(lens, offs)):
        q, k, v = _heads_of(qkv16, off, n, heads, np.float32)
        nxt = None
        if i + 1 < len(lens):
            nxt = _heads_of(qkv16, offs[i + 1], lens[i + 1], heads, np.float32)[2]
        for h in range(heads):
            out[off:off + n, h * 64:(h + 1) * 64] = _emulate_forward_head(q[h], k[h], v[h], causal, form, mutant,
                                                                            None if nxt is None else nxt[h])
    return out


def pow2_scale(amax):
    """cc_pow2_scale: the power of two s with s * amax in [2^13, 2^14)."""
    amax = float(amax)
    return float(2.0 ** np.floor(np.log2(16384.0 / max(amax, 2.0 ** -112)))) if amax > 0 and np.isfinite(amax) else 1.0


def _backward_p_dp(q, k, v, do16, causal):
    n = q.shape[0]
    vis = _mask(n, causal)
    s = np.where(vis, (q @ k.T) * np.float32(0.125), np.float32(-3.0e38)).astype(np.float32)
    e = np.where(vis, np.exp(s - s.max(axis=1, keepdims=True)), np.float32(0)).astype(np.float32)
    p = e * (np.float32(1.0) / e.sum(axis=1, keepdims=True, dtype=np.float32))
    dp = (do16 @ v.T).astype(np.float32)
    dot = (p * dp).sum(axis=1, keepdims=True, dtype=np.float32)
    return p, (p * (dp - dot)).astype(np.float32)


def emulate_backward(qkv16, d_out, lens, offs, heads, causal, mutant=None):
    """The documented backward arithmetic with one pair of fp16 scales per (sequence, head) -> d_qkv [rows, 3 W] float32.
    mutant "launch_scale": one pair of scales for the whole launch."""
    assert mutant is None or mutant in BACKWARD_MUTANTS
    W = heads * 64
    out = np.zeros((qkv16.shape[0], 3 * W), dtype=np.float32)
    d_out = np.asarray(d_out, dtype=np.float32)
    jobs = []
    for n, off in zip(lens, offs):
        q, k, v = _heads_of(qkv16, off, n, heads, np.float32)
        do = d_out[off:off + n].reshape(n, heads, 64).transpose(1, 0, 2)
        for h in range(heads):
            jobs.append((n, off, h, q[h], k[h], v[h], do[h]))
    launch_o = pow2_scale(max(float(np.abs(j[6]).max()) for j in jobs))
    staged = []
    for n, off, h, q, k, v, do in jobs:
        s_o = launch_o if mutant == "launch_scale" else pow2_scale(np.abs(do).max())
        do16 = _f16(do * np.float32(s_o))
        p, ds = _backward_p_dp(q, k, v, do16, causal)
        staged.append((s_o, do16, p, ds))
    launch_s = pow2_scale(max(float(np.abs(st[3]).max()) for st in staged))
    for (n, off, h, q, k, v, do), (s_o, do16, p, ds) in zip(jobs, staged):
        s_s = launch_s if mutant == "launch_scale" else min(pow2_scale(np.abs(ds).max()), 2.0 ** 123 / s_o)
        ds16 = _f16(ds * np.float32(s_s))
        un_q = np.float32(0.125) / (np.float32(s_o) * np.float32(s_s))
        cols = slice(h * 64, (h + 1) * 64)
        out[off:off + n, cols] = (ds16 @ k).astype(np.float32) * un_q
        out[off:off + n, W + h * 64:W + (h + 1) * 64] = (ds16.T @ q).astype(np.float32) * un_q
        out[off:off + n, 2 * W + h * 64:2 * W + (h + 1) * 64] = (_f16(p).T @ do16).astype(np.float32) * (np.float32(1.0) / np.float32(s_o))
    return out


# ------------------------------------------------------------------------------- the cases both test files walk through
NSEQ, HEADS = 3, 2
FORWARD_LENGTHS = {"wave": (1, 17, 50, 56), "block": (57, 64, 65, 197, 256), "long": (257, 321, 577, 640)}
PACKED_LENGTHS = ((56, 1, 40), (256, 33, 200), (257, 40), (640, 300))
FUSED_LENGTHS = (32, 50, 56, 57, 77, 197, 256)
FUSED_KINDS = ("high_gain", "loud_neighbour")
BACKWARD_LENGTHS = (1, 50, 64, 65, 197, 256, 257, 320)
BACKWARD_RECIPES = ("peaked", "ascending", "extreme", "loud_neighbour", "gaussian")


def kernel_of(L):
    return "wave" if L <= 56 else "block" if L <= 256 else "long"


def form_of(L):
    return "streamed" if L > 256 else "resident"


def packed_layout(lens, gap=3, guard=5):
    """Row offsets with ``gap`` unused rows between sequences and ``guard`` before the first and after the last -> offs, rows."""
    offs, row = [], guard
    for n in lens:
        offs.append(row)
        row += n + gap
    return offs, row - gap + guard


def fused_inputs(kind, lens, heads, seed):
    """Inputs of the LayerNorm-folded in_proj for back-to-back sequences: x [rows, W] fp32, in_proj weight [3 W, W] and bias,
    LayerNorm gamma and beta (fp32 numpy).
    high_gain: the q and k rows of the weight times 6: peaked softmax rows, |score| in the hundreds.
    loud_neighbour: odd sequences carry a large component along a zero-mean direction d0 that the k and v rows of the weight
    amplify (|k| about 15, |v| in the thousands); even sequences are orthogonal to d0 and stay quiet."""
    W = heads * 64
    rng = np.random.default_rng([seed, FUSED_KINDS.index(kind), 77])
    rows = int(sum(lens))
    x = rng.standard_normal((rows, W)) * 1.5 + 0.3
    w = rng.standard_normal((3 * W, W)) * 1.25 * W ** -0.5
    b = rng.standard_normal(3 * W) * 0.1
    gamma, beta = 1.0 + 0.1 * rng.standard_normal(W), 0.1 * rng.standard_normal(W)
    if kind == "high_gain":
        w[:2 * W] *= 6.0
    else:
        gamma[:], beta[:] = 1.0, 0.0
        w *= 0.25
        d0 = np.where(rng.permutation(W) % 2 == 0, 1.0, -1.0) * W ** -0.5
        w[W:2 * W] += 1.4 * np.sign(rng.standard_normal((W, 1))) * d0[None, :]
        w[2 * W:] += 280.0 * np.sign(rng.standard_normal((W, 1))) * d0[None, :]
        row = 0
        for s, n in enumerate(lens):
            xs = x[row:row + n]
            xs -= (xs @ d0)[:, None] * d0[None, :]
            if s % 2 == 1:
                xs += 3.0 * W ** 0.5 * np.sign(rng.standard_normal((n, 1))) * d0[None, :]
            row += n
    return tuple(a.astype(np.float32) for a in (x, w, b, gamma, beta))


def fused_qkv_float64(x, w, b, gamma, beta, eps=1e-5):
    """fp16(LayerNorm(x) w^T + b) in float64: what the in_proj holds up to its own rounding (host tests only)."""
    x = x.astype(np.float64)
    xh = (x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, keepdims=True) + eps)
    return ((xh * gamma + beta) @ w.astype(np.float64).T + b).astype(np.float16)
