"""CPU half of the per-op tests of the retrieval tail (tests/test_metrics_ops_gpu.py): the plain references of
tests/metrics_ref.py held against the outputs of the reference project that are already committed under tests/golden/
(compute_metrics on a 40 x 40 matrix with a tie, the ragged 12-video / 33-sentence problem, CrossEn on a 9 x 9 matrix), the
integer emulation of the float maximum group_max_rows publishes, and the power of the two running-error bounds: a reference
that is wrong by one element must stand far outside them."""
import itertools
import os

import numpy as np
import pytest

import metrics_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gc():
    return np.load(os.path.join(GOLDEN, "clip_golden.npz"))


def _five(m):
    return [m["R1"], m["R5"], m["R10"], m["MR"], m["MeanR"]]


def test_rank_counts_ref_gives_the_reference_metrics(gc):
    """compute_metrics (utils/metrics.py:11-26) on n1_sim and its transpose, ties included: 41 entries for 40 rows."""
    from centerclip_amd.metrics import metrics_from_counts
    sim = gc["n1_sim"]
    for x, want, cols in ((sim, gc["n1_t2v"], gc["n1_t2v_cols"]), (sim.T, gc["n1_v2t"], None)):
        gt, eq, _ = mr.rank_counts_ref(x, np.arange(x.shape[0]))
        got = metrics_from_counts(np.stack([gt, eq], 1))
        np.testing.assert_allclose(_five(got), want, rtol=0, atol=1e-12)
        if cols is not None:
            assert got["cols"] == [int(c) for c in cols] and len(got["cols"]) == 41
            assert np.array_equal(mr.ranks_from_counts(gt, eq), cols)


def test_references_give_the_multi_sentence_fixture():
    """tensor_text_to_video_metrics / tensor_video_to_text_sim (utils/metrics.py:38-76) on sim3 [12, 5, 12] with its -inf
    padding rows: the sentence ranks from the three counts, the per-(group, video) maxima entry for entry, their ranks."""
    from centerclip_amd.metrics import metrics_from_counts, multi_sentence_metrics_from_counts
    gm = np.load(os.path.join(GOLDEN, "metrics_multi_golden.npz"))
    sim3 = gm["sim3"]
    G, Lmax, C = sim3.shape
    flat, gt_cols = sim3.reshape(G * Lmax, C), np.repeat(np.arange(G), Lmax)
    gt, eq, front = mr.rank_counts_ref(flat, gt_cols)
    valid = np.isfinite(flat[np.arange(G * Lmax), gt_cols])
    assert int(valid.sum()) == 33
    tv = multi_sentence_metrics_from_counts(np.stack([gt, eq, front], 1), valid)
    np.testing.assert_allclose([tv["R1"], tv["R5"], tv["R10"], tv["MedianR"], tv["MeanR"], tv["Std_Rank"]], gm["tv"], rtol=0,
                               atol=1e-12)
    best = mr.group_max_ref(flat, gt_cols, G)                    # [group, video]
    assert np.array_equal(best.T, gm["v2t_sim"].astype(np.float64))
    a, b, _ = mr.rank_counts_ref(best.T.astype(np.float32), np.arange(C))
    np.testing.assert_allclose(_five(metrics_from_counts(np.stack([a, b], 1))), gm["vt"], rtol=0, atol=1e-12)


def test_group_max_ref_edges():
    sim = np.array([[1.0, np.nan], [np.nan, np.nan], [-2.0, -0.0], [-3.0, -1.0], [5.0, 5.0], [7.0, 7.0]], np.float32)
    out = mr.group_max_ref(sim, [0, 0, 2, 2, -1, 4], 4)
    assert np.array_equal(out, np.array([[1.0, -np.inf], [-np.inf, -np.inf], [-2.0, 0.0], [-np.inf, -np.inf]]))


def test_rank_counts_ref_edges():
    sim = np.array([[0.0, -0.0, np.nan, np.inf, 1.0], [np.nan, 1.0, 1.0, 1.0, -np.inf]], np.float32)
    assert [a.tolist() for a in mr.rank_counts_ref(sim, np.array([1, 0]))] == [[2, 0], [2, 0], [1, 0]]
    assert [a.tolist() for a in mr.rank_counts_ref(sim, np.array([3, 3]))] == [[0, 0], [1, 3], [0, 2]]
    assert [a.tolist() for a in mr.rank_counts_ref(sim, np.array([0.5, np.nan], np.float32))] == [[2, 0], [0, 0], [0, 0]]


def test_crossen_ref_gives_the_reference_losses():
    """CrossEn (modules/losses.py:8-18) on n4_sim and its transpose; the fixture holds the reference's fp32 results (a 9-term
    log-softmax of values near 4.6: a few ulps of 2^-21)."""
    g = np.load(os.path.join(GOLDEN, "r2_golden.npz"))
    got = mr.crossen_ref(g["n4_sim"])
    np.testing.assert_allclose(got[:2], g["n4_crossen"].astype(np.float64), rtol=0, atol=2e-6)
    assert got[2] == (got[0] + got[1]) / 2


SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, np.inf, -np.inf]            # +-0, +-tiny (the smallest subnormal), +-1, +-inf


def _bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def test_emulated_float_max_orders_signed_zeros_and_infinities():
    """The fixed publication - by the sign bit, maximum of signed patterns or minimum of unsigned ones - leaves the IEEE maximum
    in a cell that held -inf, for every pair and triple of {+-0, +-tiny, +-1, +-inf} in every order, with the same bits in
    every order; a maximum of -0.0 stays a zero.  The routing by `v >= 0.f` is shown to lose exactly the -0.0 cases."""
    for k in (1, 2, 3):
        for vals in itertools.product(SPECIALS, repeat=k):
            want = max(np.float32(v) for v in vals)
            got = {_bits(mr.emulated_max(p)) for p in itertools.permutations(vals)}
            assert len(got) == 1, (vals, got)
            cell = np.array(got.pop(), np.uint32).view(np.float32)[()]
            assert cell == want, (vals, cell, want)
    assert mr.emulated_max([-0.0]) == 0.0 and mr.emulated_max([-1.0, -0.0]) == 0.0 and mr.emulated_max([-0.0, -np.inf]) == 0.0
    assert _bits(mr.emulated_max([-0.0, 0.0])) == _bits(mr.emulated_max([0.0, -0.0])) == 0
    # the defect: -0.0 through the signed maximum is INT_MIN
    assert mr.emulated_max([-0.0], fixed=False) == -np.inf and mr.emulated_max([-1.0, -0.0], fixed=False) == -1.0
    wrong = [v for v in itertools.product(SPECIALS, repeat=2)
             if mr.emulated_max(v, fixed=False) != max(np.float32(a) for a in v)]
    assert wrong and all(max(np.float32(a) for a in v) == 0 and all(_bits(a) != 0 for a in v) for v in wrong)


@pytest.mark.parametrize("scale", [1, 100])
def test_loss_bound_is_small_against_the_values(scale):
    """The bound is a few hundred unit roundoffs of the loss's terms, not a tolerance that swallows errors."""
    for n in (1, 2, 65, 300):
        sim = mr.loss_case(n, scale)
        ref, b = mr.crossen_ref(sim), mr.crossen_bound(sim)
        assert np.all(b > 0) and np.all(b <= 400 * mr.U * (np.abs(ref) + np.abs(sim).max() + 1)), (n, b, ref)


def test_loss_bound_has_power_at_n65():
    """n = 65 is the first size whose lane loop wraps: a row sum without its last column (the lane-0 element of the second
    pass) must differ from the reference by more than 10x the bound."""
    sim = mr.loss_case(65, 1)
    ref, b = mr.crossen_ref(sim), mr.crossen_bound(sim)
    wrong = mr.crossen_ref(sim, drop_last=True)
    ratio = np.abs(wrong - ref) / b
    print("loss n=65 scale=1: |ref without the last column - ref| / bound =", ratio)
    assert np.all(ratio > 10), ratio


def _head_power(case, **wrong):
    ref = mr.head_project_ref(case["h"], case["row_of"], case["gamma"], case["beta"], case["proj"])
    b = mr.head_project_bound(case["h"], case["row_of"], case["gamma"], case["beta"], case["proj"])
    bad = mr.head_project_ref(case["h"], case["row_of"], case["gamma"], case["beta"], case["proj"], **wrong)
    return float((np.abs(bad - ref) / b).max())


def test_head_bound_power():
    """On rows of mean 100 and deviation 1 the variance is 1 and eps = 1e-5 moves an output by 5e-6 of itself, while the bound
    there is led by the error of the mean (10 roundings of numbers near 100, common to the row's channels): the reference
    without eps stays INSIDE 10x the bound (ratio printed: 0.105), so it cannot serve as the power check of that case.
    Two perturbations stand in for it: the last channel left out of the dot product on the same rows (a k-slice that stops
    one element early), and eps dropped on rows of deviation 0.01, where eps is a tenth of the variance."""
    big = mr.head_case(768, 512, 5, mean=100.0, std=1.0)
    r_eps = _head_power(big, eps=0.0)
    r_k = _head_power(big, drop_last_k=True)
    small = mr.head_case(768, 512, 5, mean=0.0, std=0.01)
    r_small = _head_power(small, eps=0.0)
    print("head power: mean-100 rows, eps dropped %.3g; last channel dropped %.3g; deviation-0.01 rows, eps dropped %.3g"
          % (r_eps, r_k, r_small))
    assert r_eps < 10            # (stated, not wished for: see the docstring)
    assert r_k > 10 and r_small > 10
