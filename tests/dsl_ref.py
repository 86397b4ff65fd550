"""Float64 restatements shared by tests/test_dsl_host.py and tests/test_dsl_gpu.py (camoe_dsl): the dual softmax, the DSL
loss, the retrieval metrics with eval_epoch's string format, and the running-error bound of the column statistics.
Written from the formulas (D = S * softmax(S, dim=0) * len(S); utils/metrics.py:11-26,38-76), not from the library's code."""
import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32
SLAB, WAVES = 128, 4                # cc_dsl_col_stats_f32: rows per slab, waves of a workgroup (documented in csrc/dsl.hip)


def dual_softmax64(sim, n_total=None):
    """sim [rows, cols] (numpy, any float) -> float64 D = n_total * sim * softmax(sim, axis=0); NaN propagates per column."""
    s = np.asarray(sim, dtype=np.float64)
    n = s.shape[0] if n_total is None else n_total
    with np.errstate(invalid="ignore", over="ignore"):
        m = s.max(axis=0, keepdims=True) if s.shape[0] else np.full((1, s.shape[1]), -np.inf)
        e = np.exp(s - m)
        return n * s * e / e.sum(axis=0, keepdims=True)


def col_stats64(sim):
    s = np.asarray(sim, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = s.max(axis=0)
        return m, np.exp(s - m[None, :]).sum(axis=0)


def stats_bound(sim, merges=0):
    """Running-error bound of the fp32 column sums s_j against float64 (the rule of tests/test_backward_gpu.py: every fp32
    operation a term passes through costs one unit roundoff of the running magnitude, and all terms are positive, so the
    magnitude is s itself).
    A term exp(x - m) passes through
      * the subtractions x - m_wave, m_wave - m_slab, m_slab - m (and one more per extra merge of a caller): each rounds to
        U of its result, the partial maxima lie between x and m, so |x - m| * U absolute on the exponent in total, i.e. that
        much relative on the term;
      * expf (HIP documents 1 ulp; 2 U allowed here) once per level: the term itself, the wave merge, the slab merge, each
        extra merge;
      * additions: the serial chain of its wave (at most SLAB / WAVES), WAVES in the wave merge, one per slab in the slab
        merge, one per extra merge; and one multiplication by the rescale factor per merge level.
    -> depth = chain + (WAVES + 3) + (slabs + 3) + 2 + 4 * merges  roundings of a quantity <= s, and per column
       |s - s64| <= U * (depth * s64 + sum_i |x_i - m| exp(x_i - m)).  Returns (bound [cols], depth)."""
    s = np.asarray(sim, dtype=np.float64)
    rows = s.shape[0]
    slabs = -(-rows // SLAB)
    chain = min(rows, SLAB // WAVES)
    depth = chain + (WAVES + 3) + (slabs + 3) + 2 + 4 * merges
    m, s64 = col_stats64(s)
    t = np.exp(s - m[None, :])
    return U * (depth * s64 + (np.abs(s - m[None, :]) * t).sum(axis=0)), depth


def d_bound(sim, n_total, s_bound):
    """The bound carried to D_ij = (n x) * (exp(x - m) / s): relative error of s (s_bound / s64), the exponent term |x - m| U,
    expf (2 ulp), the division, two multiplications and the fp32 rounding of the stored value: 6 U more.  Below the smallest
    normal fp32 number (2^-126) no relative bound holds - exp(x - m) underflows from x - m < -87 on - so the exponential and
    the result each get that much absolute error on top."""
    s = np.asarray(sim, dtype=np.float64)
    m, s64 = col_stats64(s)
    d = np.abs(dual_softmax64(s, n_total))
    tiny = 2.0 ** -126
    return d * (s_bound / s64)[None, :] + d * U * (6.0 + np.abs(s - m[None, :])) + (n_total * np.abs(s) / s64[None, :] + 1.0) * tiny


def _ranks_plain(x):
    """compute_metrics (utils/metrics.py:11-26): positions of the diagonal value in every descending-sorted row"""
    sx = np.sort(-x, axis=1)
    return np.where(sx - np.diag(-x)[:, None] == 0)[1]


def _dict_plain(ind):
    return dict(R1=float(np.sum(ind == 0)) * 100 / len(ind), R5=float(np.sum(ind < 5)) * 100 / len(ind),
                R10=float(np.sum(ind < 10)) * 100 / len(ind), MR=np.median(ind) + 1, MeanR=np.mean(ind) + 1)


FMT = ' (metric) >>>  {p}R@1: {:.1f} - {p}R@5: {:.1f} - {p}R@10: {:.1f} - {p}Median R: {:.1f} - {p}Mean R: {:.1f}'
KEYS = ('R1', 'R5', 'R10', 'MR', 'MeanR')


def metrics64(mat, sentences=None):
    """-> (R@1 text->video, the four strings eval_epoch returns) for a [Nt, Nv] matrix; ``sentences``: per-video sentence
    counts (multi-sentence protocol, utils/metrics.py:38-76: sentence ranks, then the best sentence of a group per video)."""
    x = np.asarray(mat, dtype=np.float64)
    if sentences is None:
        tv, vt = _dict_plain(_ranks_plain(x)), _dict_plain(_ranks_plain(x.T))
    else:
        gt = np.repeat(np.arange(len(sentences)), sentences)
        truth = x[np.arange(len(gt)), gt]
        valid = np.isfinite(truth)
        with np.errstate(invalid="ignore"):
            ranks = (x > truth[:, None]).sum(axis=1)[valid]
        n = np.float32(len(ranks))
        tv = {"R%d" % k: float(np.float32(np.sum(ranks < k) * 100) / n) for k in (1, 5, 10)}
        tv["MR"] = float(np.sort(ranks + 1)[(len(ranks) - 1) // 2])
        tv["MeanR"] = float(np.mean(ranks + 1))
        clean = np.where(np.isnan(x), -np.inf, x)
        best = np.stack([clean[gt == v].max(axis=0) for v in range(len(sentences))])        # [group, video]
        vt = _dict_plain(_ranks_plain(best.T))
    info = ["Text-to-Video:", FMT.format(*[tv[k] for k in KEYS], p=""), "Video-to-Text:", FMT.format(*[vt[k] for k in KEYS], p="V2T$")]
    return tv['R1'], info


def rank_gap(mat, sentences=None):
    """Smallest distance, over every ranking the metrics read, between a ground-truth entry and any competitor."""
    x = np.asarray(mat, dtype=np.float64)

    def rows_gap(y, gt):
        g = np.inf
        for i in range(y.shape[0]):
            d = np.abs(y[i] - y[i, gt[i]])
            d[gt[i]] = np.inf
            d[np.isnan(d)] = np.inf                     # (NaN entries - a fully masked clip - never outrank anything)
            g = min(g, float(d.min()))
        return g
    if sentences is None:
        return min(rows_gap(x, np.arange(len(x))), rows_gap(x.T, np.arange(x.shape[1])))
    gt = np.repeat(np.arange(len(sentences)), sentences)
    best = np.stack([x[gt == v].max(axis=0) for v in range(len(sentences))])
    return min(rows_gap(x, gt), rows_gap(best.T, np.arange(len(sentences))))


def dsl_loss64(seq, vis, vmask, logit_scale, dtype=torch.float64):
    """The training branch's loss with the dual softmax (clip4clip.py:245-262,305-316,357-366 + D = n S softmax(S, dim=0)) in
    torch on the CPU, `dtype` arithmetic, with torch.autograd's gradients -> (loss3 [3], d_seq, d_vis, d_logit_scale)."""
    seq = torch.as_tensor(seq).to(dtype).clone().requires_grad_(True)
    vis = torch.as_tensor(vis).to(dtype).clone().requires_grad_(True)
    ls = torch.tensor(float(logit_scale), dtype=dtype, requires_grad=True)
    mk = torch.as_tensor(vmask).to(dtype).unsqueeze(-1)
    t = seq.reshape(seq.shape[0], -1)
    t = t / t.norm(dim=-1, keepdim=True)
    v = vis / vis.norm(dim=-1, keepdim=True)
    den = mk.sum(dim=1)
    den = torch.where(den == 0, torch.ones_like(den), den)
    p = (v * mk).sum(dim=1) / den
    p = p / p.norm(dim=-1, keepdim=True)
    s = ls.exp() * t @ p.t()
    d = s * torch.softmax(s, dim=0) * s.shape[0]
    l1 = -torch.diag(torch.log_softmax(d, dim=-1)).mean()
    l2 = -torch.diag(torch.log_softmax(d.t(), dim=-1)).mean()
    loss = (l1 + l2) / 2
    loss.backward()
    return torch.stack([l1, l2, loss]).detach(), seq.grad, vis.grad, ls.grad
