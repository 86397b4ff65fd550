"""The token-cluster distance and selection kernels on generic floats - inputs on which fp32 arithmetic rounds.
Needs a real MI355X: run with ``-m gpu``.  (tests/test_cluster_generic_host.py shows, without a GPU, that the bounds used here
hold for the kernels' documented arithmetic and fail for a kernel that loses a plane, a k-slice or a mirrored element, and that
every input below meets the conditions the bit-for-bit cases need - nothing here skips.)

  * gram_dist_kernel (L2, cosine) against float64, pair by pair, within oracle.gram_error_bound - shapes with several row tiles,
    mirrored off-diagonal tiles, a ragged last tile, up to 12 k-slices (four trips round the 3-stage register ring);
  * lp_dist_kernel<0> (general p) within oracle.minkowski_error_bound, lp_dist_kernel<2> (p = inf) bit for bit;
  * the fused op == oracle.select_streamlined on the D that pairwise_distance returns for the same chunk, bit for bit, for
    every instantiation of kmedoids_select_kernel the dispatch reaches up to N = 1,000, and for the module's strided tokens.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cluster_oracle as co
from oracle import recipes as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = co.U32


@pytest.fixture(scope="module")
def cl():
    import centerclip_amd.cluster as cluster
    return cluster


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _share(d, d64, bound):
    err = np.abs(d.astype(np.float64) - d64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


def _check_flags(cl, Xd, raw, metric, p):
    """The shift and the diagonal, bit for bit from the raw tensor: (raw - max) - 1 with the maximum of the WHOLE batch that
    was passed, the diagonal - 1 more.  Returns the fully shifted tensor."""
    f = np.float32
    N = raw.shape[-1]
    idx = np.arange(N)
    mx = f(raw.max())
    assert (raw.max(axis=(1, 2)) < mx).any()                      # a per-problem maximum would show
    neg = cl.pairwise_distance(Xd, Xd, metric=metric, self_nearest=False, all_negative=True, p=p).cpu().numpy()
    assert np.array_equal(neg, (raw - mx) - f(1.0))
    near = cl.pairwise_distance(Xd, Xd, metric=metric, self_nearest=True, all_negative=False, p=p).cpu().numpy()
    want = raw.copy()
    want[:, idx, idx] -= f(1.0)
    assert np.array_equal(near, want)
    both = cl.pairwise_distance(Xd, Xd, metric=metric, self_nearest=True, all_negative=True, p=p).cpu().numpy()
    assert np.array_equal(both, co.shifted_distance(raw))
    assert np.array_equal(both, both.transpose(0, 2, 1))
    return both, mx


# ------------------------------------------------------------------------------- Gram kernel against float64
@pytest.mark.parametrize("metric", co.METRICS)
@pytest.mark.parametrize("seed,N,W,recipe", R.gram_sweep_cases())
def test_gram_distance_within_derived_bound(cl, seed, N, W, recipe, metric):
    """|d_hip - d_float64| <= gram_error_bound for every pair; D bitwise symmetric; the euclidean diagonal exactly 0 before the
    shift and exactly (-max - 1) - 1 after it (cosine: 1 - g_ii * iv_i^2, a rounding away from 0, held to the bound like any
    pair); the shifted tensors are the raw one shifted by the maximum of the whole batch.  Printed, not asserted: the share of
    the bound the kernel used and the error of the literal reference (ATen's fp32 cdist / bmm on the CPU) on the same tokens."""
    X = R.GENERIC_RECIPES[recipe](seed, (R.GRAM_SWEEP_P, N, W))
    Xd = dev(X)
    d64 = co.float64_distance(X, metric)
    bound = co.gram_error_bound(X, metric)
    raw = cl.pairwise_distance(Xd, Xd, metric=metric, self_nearest=False, all_negative=False).cpu().numpy()
    assert raw.dtype == np.float32 and raw.shape == (R.GRAM_SWEEP_P, N, N) and np.isfinite(raw).all()
    err = np.abs(raw.astype(np.float64) - d64)
    share = float((err[bound > 0] / bound[bound > 0]).max())
    Xt = torch.from_numpy(X)
    lit = co.literal_pairwise_distance(Xt, Xt, metric, False, False, 2.0).numpy().astype(np.float64)
    off = ~np.eye(N, dtype=bool)
    lerr = np.abs(lit - d64)
    print(f"[gram {recipe} N={N} W={W} {metric}] kernel: share of bound {share:.4f}, max|err| off-diagonal {err[:, off].max():.3e}"
          f" diagonal {np.einsum('bii->bi', err).max():.3e}; literal fp32 reference: max|err| off-diagonal {lerr[:, off].max():.3e}"
          f" (= {float((lerr / np.maximum(bound, 1e-300))[:, off].max()):.3f} of the bound) diagonal {np.einsum('bii->bi', lerr).max():.3e}")
    assert (err <= bound).all(), (share, np.unravel_index(np.argmax(err - bound), err.shape))
    assert np.array_equal(raw, raw.transpose(0, 2, 1))
    diag = np.einsum("bii->bi", raw)
    if metric == "euclidean":
        assert not diag.any()
    both, mx = _check_flags(cl, Xd, raw, metric, 2.0)
    if metric == "euclidean":
        assert (np.einsum("bii->bi", both) == (np.float32(0.0) - mx) - np.float32(1.0) - np.float32(1.0)).all()
    # and the shifted tensor against float64 directly: the pair's bound, the bound of the pair that holds the maximum, and the
    # roundings of the two subtractions (three on the diagonal)
    ref = co.shifted_distance(d64)
    tol = bound + bound.max() + 3.0 * U * (np.abs(ref) + 2.0)
    assert (np.abs(both.astype(np.float64) - ref) <= tol).all()


# ------------------------------------------------------------------------------- Minkowski kernel against float64
def _structural(a, m, N, K):
    assert (np.diff(m, axis=1) > 0).all()                                  # ascending, distinct
    assert (m >= 0).all() and (m < N).all() and (a >= 0).all() and (a < K).all()
    for p in range(m.shape[0]):
        assert np.array_equal(a[p, m[p]], np.arange(K))                    # a medoid belongs to its own cluster


@pytest.mark.parametrize("p", R.MINKOWSKI_P)
@pytest.mark.parametrize("seed,P,N,W,recipe", R.MINKOWSKI_CASES)
def test_minkowski_self_distance(cl, seed, P, N, W, recipe, p):
    """pairwise_distance(X, X, p=...) off the two exact settings: general p through powf within minkowski_error_bound, p = inf
    equal to the float64 maximum rounded to fp32; symmetric, zero diagonal, the shift as for the Gram kernel; and the k-medoids
    that run on these distances return a structurally valid clustering."""
    X = R.GENERIC_RECIPES[recipe](seed, (P, N, W))
    Xd = dev(X)
    d64 = co.float64_distance(X, "euclidean", p)
    raw = cl.pairwise_distance(Xd, Xd, metric="euclidean", self_nearest=False, all_negative=False, p=p).cpu().numpy()
    assert np.isfinite(raw).all()
    if np.isinf(p):
        assert np.array_equal(raw, d64.astype(np.float32))
    else:
        bound = co.minkowski_error_bound(X, p)
        err = np.abs(raw.astype(np.float64) - d64)
        print(f"[lp p={p} {recipe} N={N} W={W}] share of bound {_share(raw, d64, bound):.4f}, max|err| {err.max():.3e}")
        assert (err <= bound).all()
    assert np.array_equal(raw, raw.transpose(0, 2, 1)) and not np.einsum("bii->bi", raw).any()
    _check_flags(cl, Xd, raw, "euclidean", p)
    K = 9
    a, m = cl.batch_fast_kmedoids(Xd, K, distance="euclidean", threshold=1e-6, iter_limit=100, id_sort=True, norm_p=p)
    _structural(a.cpu().numpy(), m.cpu().numpy(), N, K)


# ------------------------------------------------------------------------------- fused op == oracle selection on the kernel's D
def _library_norms(Xd):
    from centerclip_amd import _lib as L
    P, N, W = Xd.shape
    lay = L.TokenLayout(P, 1, 1, N, N * W, 0, 0, W)
    norms = torch.empty(P, N, device=DEV)
    ws = L.workspace(L.lib().cc_cluster_workspace_bytes(P, N, W, 1), Xd.device)
    L.check(L.lib().cc_token_norms_f32(L.ptr(Xd), ctypes.byref(lay), W, L.ptr(norms), L.ptr(ws), ws.numel(),
                                       L.stream_ptr(Xd.device)), "norms")
    return norms


def _distance_launch_norms(Xc):
    """The row norms the Gram launch of pairwise_distance publishes next to D (the ones the fused op's KKZ init reads)."""
    from centerclip_amd import _lib as L
    P, N, W = Xc.shape
    lay = L.TokenLayout(P, 1, 1, N, N * W, 0, 0, W)
    dist = torch.empty(P, N, N, device=DEV)
    norms = torch.empty(P, N, device=DEV)
    ws = L.workspace(L.lib().cc_cluster_workspace_bytes(P, N, W, 0), Xc.device)
    L.check(L.lib().cc_pairwise_distance_f32(L.ptr(Xc), ctypes.byref(lay), W, 0, 2.0, 1, 1, P, L.ptr(dist), L.ptr(norms),
                                             L.ptr(ws), ws.numel(), L.stream_ptr(Xc.device)), "distance")
    return norms.cpu().numpy()


def _oracle_on_kernel_distance(cl, tokens, first_of, K, split, metric, norm_p, id_sort):
    A, M = [], []
    for c0 in range(0, tokens.shape[0], split):
        Xc = tokens[c0:c0 + split].contiguous()
        D = cl.pairwise_distance(Xc, Xc, metric=metric, self_nearest=True, all_negative=True, p=norm_p).cpu().numpy()
        for b in range(Xc.shape[0]):
            a_s, m_s, steps = co.select_streamlined(D[b], first_of(c0, b, Xc), K, iter_limit=100, id_sort=id_sort)
            assert steps < 100
            A.append(a_s)
            M.append(m_s)
    return np.stack(A), np.stack(M)


def _first_from_float64(X):
    return lambda c0, b, Xc: int(np.argmax((X[c0 + b].astype(np.float64) ** 2).sum(-1)))


@pytest.mark.parametrize("tag", list(R.BITWISE_CASES))
def test_fused_op_equals_oracle_selection_on_the_kernels_own_distance(cl, tag):
    """batch_fast_kmedoids_with_split == select_streamlined (ATen's summation association) on pairwise_distance of the same
    split chunk, medoids and assignment bit for bit.  P = 5 with split_size = 2: chunks of 2, 2 and 1 problems, each shifted
    by its own maximum.  The first medoid comes from float64 norms (the host test asserts a 1e-4 relative gap); with pre_norm
    every clustered token has norm 1 to rounding, so there it comes from the norms the distance launch itself publishes, and D
    from the library's own normalised tokens."""
    cfg = R.BITWISE_CASES[tag]
    X = R.bitwise_tokens(cfg)
    Xd = dev(X)
    K, split = cfg["K"], cfg["split"]
    a, m = cl.batch_fast_kmedoids_with_split(Xd, K, distance=cfg["metric"], threshold=1e-6, iter_limit=100,
                                             id_sort=cfg["id_sort"], norm_p=cfg["norm_p"], split_size=split,
                                             pre_norm=cfg["pre_norm"])
    if cfg["pre_norm"]:
        tokens = Xd / (_library_norms(Xd).unsqueeze(-1) + 1e-6)
        first_of = lambda c0, b, Xc: int(np.argmax(_distance_launch_norms(Xc)[b]))
    else:
        tokens, first_of = Xd, _first_from_float64(X)
    ao, mo = _oracle_on_kernel_distance(cl, tokens, first_of, K, split, cfg["metric"], cfg["norm_p"], cfg["id_sort"])
    a, m = a.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(m, mo), (tag, np.nonzero((m != mo).any(1))[0])
    assert np.array_equal(a, ao), (tag, np.nonzero((a != ao).any(1))[0])


def test_module_on_strided_tokens_equals_oracle_selection_on_the_kernels_own_distance(cl):
    """TokenClusterInter (eval) reads its problems through the token layout (problem s*B + b, token f*n + i of x [1+n, B*T, W]),
    not from contiguous [P, N, W] tokens: its medoid ids equal the oracle selection on pairwise_distance of the regrouped
    tokens, and its output rows are those tokens (and the segments' CLS means), bit for bit, in both memory layouts."""
    c = R.BITWISE_MODULE_CASE
    B, T, T_new, n, K, W = (c[k] for k in ("B", "T", "T_new", "n", "K", "W"))
    x = R.generic(c["seed"], (1 + n, B * T, W))
    mod = cl.TokenClusterInter(algorithm="kmediods++", block_id=7, before_cluster_num=n, cluster_num=K,
                               before_block_frames=T, after_block_frames=T_new, original_frame=T, distance="euclidean",
                               threshold=1e-6, iter_limit=100, id_sort=True, aggregation=None, split_size=c["split"],
                               norm_p=2.0, transformer_width=W).eval()
    tokens, cls = co.regroup_segments(torch.from_numpy(x), T, T_new)
    _, med = _oracle_on_kernel_distance(cl, tokens.to(DEV), _first_from_float64(tokens.numpy()), K, c["split"], "euclidean",
                                        2.0, True)
    P, fd = tokens.shape[0], T // T_new
    picked = tokens[torch.arange(P).unsqueeze(-1), torch.from_numpy(med)]
    picked = picked.reshape(T_new, B, K, W).permute(1, 0, 2, 3).reshape(B * T_new, K, W)
    seg_cls = torch.stack([c_.mean(dim=1) for c_ in torch.split(cls, fd, dim=1)], dim=1)
    want = torch.cat([seg_cls.reshape(B * T_new, 1, W), picked], dim=1).permute(1, 0, 2).contiguous().numpy()
    y, res = mod(dev(x))
    assert res is None and np.array_equal(mod.last_medoids.cpu().numpy(), med)
    assert np.array_equal(y.cpu().numpy(), want)
    y2 = mod.cluster_frame_major(dev(x).permute(1, 0, 2).contiguous(), keep_ids=True)
    assert np.array_equal(mod.last_medoids.cpu().numpy(), med)
    assert np.array_equal(y2.permute(1, 0, 2).cpu().numpy(), want)
