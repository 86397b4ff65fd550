"""The yardsticks of tests/test_cluster_generic_gpu.py, checked without a GPU.

The GPU tests hold the Gram distance kernel to a derived per-pair error bound on generic floats.  Such a test is only worth
something if (a) the emulation the bound was derived from is the kernel's arithmetic - shown here on inputs where that
arithmetic is exact -, and (b) the bound is wide enough for every faithful evaluation and too narrow for a kernel that loses
its lo plane, one of the two cross products, a k-slice or a mirrored element.  Both are asserted here for every case of the
GPU sweep.  Detected at every shape of the sweep, W = 768 (the shipped width) included: "lo", "hi_lo", "lo_hi" by the bound
on at least one pair; "kslice" (shapes with W > 64) by the bound; "mirror" by plain inequality (D stops being symmetric).

The conditions the bit-for-bit GPU tests need from their inputs (an unambiguous first medoid, convergence before the
iteration limit) are asserted here too, for every problem, so that no GPU case ever has to skip.
"""
import numpy as np
import pytest
import torch

from oracle import cluster_oracle as co
from oracle import recipes as R


def _share(d, d64, bound):
    """Largest |d - d64| / bound over the pairs with a non-zero bound; pairs with bound 0 must be exact."""
    err = np.abs(d.astype(np.float64) - d64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


# ------------------------------------------------------------------------------- the emulation is the kernel's arithmetic
@pytest.mark.parametrize("metric", co.METRICS)
def test_emulation_equals_exact_distance_on_lattices(metric):
    for seed, shape in ((5, (3, 70, 96)), (6, (2, 130, 200)), (7, (1, 196, 768))):
        X = R.lattice(seed, shape)
        want = co.exact_zero_diag_distance(X, metric)
        assert np.array_equal(co.emulated_gram_distance(X, metric), want)
        for acc in ("f32_asc", "f32_desc"):                      # exact sums: no order, no rounding
            assert np.array_equal(co.emulated_gram_distance(X, metric, accumulate=acc), want)
    hi, lo = co.split_hi_lo(R.lattice(5, (3, 70, 96)))
    assert not lo.any()


@pytest.mark.parametrize("tag", ["n12", "n32"])
def test_emulation_within_c3_fixture_tolerance(cluster_golden, tag):
    g = cluster_golden
    X = g[f"c3_{tag}_x"]
    off = ~np.eye(X.shape[1], dtype=bool)
    for metric, mtag in (("euclidean", "l2"), ("cosine", "cos")):
        for flag in (False, True):
            d = co.emulated_gram_distance(X, metric, shift=flag)
            ref = g[f"c3_{tag}_{mtag}_an{int(flag)}_sn{int(flag)}"]
            np.testing.assert_allclose(d[:, off], ref[:, off], rtol=0, atol=2e-4)
            np.testing.assert_allclose(np.einsum("bii->bi", d), np.einsum("bii->bi", ref), rtol=0, atol=0.04)


def test_split_is_the_kernels():
    """hi + lo reproduces x to 22 bits where lo is a normal fp16 number, and to 2^-25 absolute where it is subnormal."""
    x = R.generic(1, (4096,))
    hi, lo = co.split_hi_lo(x)
    r = x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert (np.abs(r) <= np.maximum(np.abs(x) * 2.0 ** -22, 2.0 ** -25)).all()
    t = R.tiny_lo(2, (4096,))
    hi, lo = co.split_hi_lo(t)
    assert (np.abs(lo.astype(np.float64)) < 2.0 ** -14).all() and lo.any()         # the whole lo plane is subnormal
    assert np.abs(t.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)).max() <= 2.0 ** -25


# ------------------------------------------------------------------------------- the bound separates right from wrong
@pytest.mark.parametrize("metric", co.METRICS)
@pytest.mark.parametrize("seed,N,W,recipe", R.gram_sweep_cases())
def test_bound_holds_for_faithful_and_fails_every_broken_variant(seed, N, W, recipe, metric):
    X = R.GENERIC_RECIPES[recipe](seed, (R.GRAM_SWEEP_P, N, W))
    d64 = co.float64_distance(X, metric)
    bound = co.gram_error_bound(X, metric)
    assert np.isfinite(bound).all() and (bound >= 0).all()
    line = []
    faithful = co.emulated_gram_distance(X, metric, shift=False)
    for acc in ("f64", "f32_asc", "f32_desc"):
        d = faithful if acc == "f64" else co.emulated_gram_distance(X, metric, accumulate=acc, shift=False)
        s = _share(d, d64, bound)
        line.append(f"{acc} {s:.3f}")
        assert s <= 1.0, (acc, s)
        assert np.array_equal(d, d.transpose(0, 2, 1))
    for drop in ("lo", "hi_lo", "lo_hi") + (("kslice",) if W > 64 else ()):
        d = co.emulated_gram_distance(X, metric, drop=drop, shift=False)
        s = float((np.abs(d.astype(np.float64) - d64)[bound > 0] / bound[bound > 0]).max())
        line.append(f"{drop} {s:.1f}")
        assert s > 1.0, (drop, s)
    if N > 33:
        d = co.emulated_gram_distance(X, metric, drop="mirror", shift=False)
        assert not np.array_equal(d, d.transpose(0, 2, 1)) and not np.array_equal(d, faithful)
        line.append("mirror: asymmetric")
    print(f"[bound N={N} W={W} {recipe} {metric}] share of the bound: " + ", ".join(line))


def test_sweep_contains_every_size_and_recipe():
    cases = R.gram_sweep_cases()
    assert len(cases) == 16 and len(set(cases)) == 16
    assert {c[1] for c in cases} == set(R.GRAM_SWEEP_N) and {c[2] for c in cases} == set(R.GRAM_SWEEP_W)
    assert {c[3] for c in cases} == set(R.GENERIC_RECIPES)
    assert (196, 768, "offset") in {c[1:] for c in cases} and (65, 64, "near_dup") in {c[1:] for c in cases}


def test_shifted_bound_follows_from_the_raw_one():
    """The GPU test checks the shifted tensor as (raw - max) - 1 in fp32, bit for bit; here: that identity holds for the
    emulation, with the maximum of the whole batch and with a maximum handed in."""
    X = R.generic(11, (3, 65, 96))
    raw = co.emulated_gram_distance(X, shift=False)
    assert np.array_equal(co.emulated_gram_distance(X), co.shifted_distance(raw))
    b = int(np.argmin(raw.max(axis=(1, 2))))                      # a problem that does not hold the batch maximum
    assert raw.max() > raw[b].max()
    assert np.array_equal(co.emulated_gram_distance(X[b:b + 1], chunk_max=raw.max()), co.shifted_distance(raw, raw.max())[b:b + 1])
    assert not np.array_equal(co.emulated_gram_distance(X[b:b + 1]), co.shifted_distance(raw)[b:b + 1])


# ------------------------------------------------------------------------------- Minkowski
def _lp_kernel_emulation(X, p, drop_last=False):
    """lp_dist_kernel in numpy: fp32 terms, one fp32 accumulator per pair in ascending k, the final power in fp32."""
    f = np.float32
    X = np.asarray(X, dtype=f)
    W = X.shape[-1] - (1 if drop_last else 0)
    acc = np.zeros(X.shape[:2] + (X.shape[1],), f)
    for k in range(W):
        t = np.abs(X[:, :, None, k] - X[:, None, :, k])
        if np.isinf(p):
            acc = np.maximum(acc, t)
        else:
            acc = acc + (t if p == 1.0 else np.power(t, f(p)))
    return acc if p == 1.0 or np.isinf(p) else np.power(acc, f(1.0) / f(p))


@pytest.mark.parametrize("p", R.MINKOWSKI_P)
@pytest.mark.parametrize("seed,P,N,W,recipe", R.MINKOWSKI_CASES[:4])
def test_minkowski_bound_holds_for_faithful_and_fails_a_lost_element(seed, P, N, W, recipe, p):
    X = R.GENERIC_RECIPES[recipe](seed, (P, N, W))
    d64 = co.float64_distance(X, "euclidean", p)
    d = _lp_kernel_emulation(X, p)
    assert np.array_equal(d, d.transpose(0, 2, 1)) and not np.einsum("bii->bi", d).any()
    if np.isinf(p):
        assert np.array_equal(d, d64.astype(np.float32))
        assert not np.array_equal(_lp_kernel_emulation(X, p, drop_last=True), d)
        return
    bound = co.minkowski_error_bound(X, p)
    s = _share(d, d64, bound)
    bad = _lp_kernel_emulation(X, p, drop_last=True).astype(np.float64)
    sb = float((np.abs(bad - d64)[bound > 0] / bound[bound > 0]).max())
    print(f"[lp bound p={p} N={N} W={W} {recipe}] faithful {s:.3f}, last element lost {sb:.1f}")
    assert s <= 1.0 and sb > 1.0


# ------------------------------------------------------------------------------- conditions of the bit-for-bit GPU cases
def _dispatch(N, K):
    """run_select's choice of kmedoids_select_kernel<D in LDS, 64-token chunks>."""
    ne = -(-N // 64)
    if R.select_d_in_lds(N, K):
        return True, min(max(ne, 1), 4)
    return False, next(v for v in (4, 7, 10, 16, 25, 40, 64, 128) if ne <= v)


def test_bitwise_cases_reach_the_instantiations_they_name():
    for tag, cfg in R.BITWISE_CASES.items():
        assert _dispatch(cfg["N"], cfg["K"]) == cfg["sel"], tag
    assert {cfg["sel"] for cfg in R.BITWISE_CASES.values()} == {(True, 1), (True, 2), (True, 3), (True, 4), (False, 4),
                                                                  (False, 7), (False, 10), (False, 16)}
    assert R.select_d_in_lds(201, 20) and not R.select_d_in_lds(202, 20)       # 202 is the first N that leaves LDS at K = 20


def _host_distance(Xc, cfg):
    """The chunk's shifted D as the kernels would form it, from the emulation (Gram) or float64 rounded (Minkowski)."""
    if cfg["metric"] == "euclidean" and cfg["norm_p"] != 2.0:
        return co.shifted_distance(co.float64_distance(Xc, "euclidean", cfg["norm_p"]).astype(np.float32))
    return co.emulated_gram_distance(Xc, cfg["metric"])


def _check_problem_conditions(X, cfg, tag, norm_gap=True):
    for c0 in range(0, X.shape[0], cfg["split"]):
        Xc = X[c0:c0 + cfg["split"]]
        D = _host_distance(Xc, cfg)
        for b in range(Xc.shape[0]):
            nrm = np.sqrt((Xc[b].astype(np.float64) ** 2).sum(-1))
            top = np.sort(nrm)[-2:]
            if norm_gap:
                assert top[1] - top[0] > 1e-4 * top[1], (tag, c0 + b, top)
            _, _, steps = co.select_streamlined(D[b], int(np.argmax(nrm)), cfg["K"], iter_limit=100, id_sort=cfg["id_sort"])
            assert steps < 100, (tag, c0 + b)


@pytest.mark.parametrize("tag", list(R.BITWISE_CASES))
def test_bitwise_case_has_an_unambiguous_first_medoid_and_converges(tag):
    """Every problem (none is left out): the two largest token norms differ by more than 1e-4 relative in float64, so any
    fp32 norm picks the same first KKZ medoid, and the oracle selection on the emulated D stops before iter_limit.
    One case cannot meet the first condition by construction: with pre_norm the tokens that are clustered all have norm
    1 to rounding, and the first medoid is whichever of them the kernel's fp32 norm rounds highest.  The GPU test takes
    that case's first medoid from the norms the distance launch itself publishes; here the gap is checked on the tokens
    before normalisation and the convergence on the normalised ones."""
    cfg = R.BITWISE_CASES[tag]
    X = R.bitwise_tokens(cfg)
    if cfg["pre_norm"]:
        _check_problem_conditions(X, cfg, tag)
        Xt = torch.from_numpy(X)
        X = (Xt / (Xt.norm(dim=-1, keepdim=True) + 1e-6)).numpy()
        _check_problem_conditions(X, cfg, tag, norm_gap=False)
    else:
        _check_problem_conditions(X, cfg, tag)


def test_bitwise_module_case_conditions():
    c = R.BITWISE_MODULE_CASE
    x = R.generic(c["seed"], (1 + c["n"], c["B"] * c["T"], c["W"]))
    tokens, _ = co.regroup_segments(torch.from_numpy(x), c["T"], c["T_new"])
    assert tuple(tokens.shape) == (c["T_new"] * c["B"], 98, c["W"])
    cfg = dict(split=c["split"], K=c["K"], metric="euclidean", norm_p=2.0, id_sort=True)
    _check_problem_conditions(tokens.numpy(), cfg, "module")
