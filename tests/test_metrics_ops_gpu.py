"""Per-op tests of the retrieval tail on the MI355X (``-m gpu``) against the plain references of tests/metrics_ref.py
(pinned to the reference project's outputs by tests/test_metrics_ops_host.py):

  * rank_counts / rank_counts_cols / rank_counts_ref (rank_counts_kernel): integer-exact on rows full of exact ties with
    +-inf, NaN (off and at the truth column) and -0.0 next to +0.0 planted; 1 / 63 / 64 / 65 / 129 / 257 columns (one, exact
    and wrapped lane strides) x 1 / 3 / 4 / 5 / 9 rows (4 row-waves a workgroup); transposed, strided, offset diagonals;
  * group_max_rows (group_max_rows_kernel + its float atomic): entry for entry, groups over several 64-row chunks, ids that
    come back, ids out of range, empty / all-NaN / all-negative groups, +-inf, a row stride, run-to-run bits; and the groups
    whose maximum is -0.0, which the atomic lost to the -inf fill before it chose its branch by the sign bit;
  * contrastive_loss (cross_entropy_rows_kernel + contrastive_mean_kernel) against float64 at n = 1 ... 300 and logit scales 1
    and 100, inside the a-priori running-error bound metrics_ref.crossen_bound;
  * ops.head_project (head_project_kernel) against float64 inside metrics_ref.head_project_bound;
  * the refusals of the op wrappers, which hand bare pointers on.

The two bounds ASSUME 2 ulps for the device expf / logf (HIP documents 1; not measured here) and carry a factor 2 over the
whole first-order analysis.  Measured max error / bound on gfx950, as printed by the tests (a ratio above 1 would be a
finding, not a reason to widen anything):

  contrastive_loss   n =      1      2      63     64     65     128    257    300
      scale 1              0.000  0.004  0.016  0.043  0.037  0.047  0.014  0.030
      scale 100            0.000  0.000  0.034  0.032  0.026  0.010  0.014  0.006
      n = 65, scale 100:   -1e30 entries 0.031    sim.t() 0.008    strided view 0.008
  head_project   (W, E) =  (4, 4)  (100, 60)  (192, 64)  (512, 68)  (768, 512)  (1024, 768)
      R = 1                0.035   0.010      0.005      0.004      0.003       0.003
      R = 5                0.026   0.014      0.008      0.007      0.003       0.004
      row_mul = 7 0.012   row_idx 0.012   rows of mean 100 0.026   gamma = 0 on half 0.005   rows of deviation 0.01 0.004

The bounds are worst-case ones (every rounding of a chain in the same direction), so ratios of a few hundredths are what a
correct kernel gives; their power is asserted on the CPU in tests/test_metrics_ops_host.py: a row sum that misses one
column stands 1,700x outside the loss bound at n = 65, a dot product that misses one channel 550x outside the head bound.
"""
import math

import numpy as np
import pytest
import torch

import metrics_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

COLS = [1, 63, 64, 65, 129, 257]
ROWS = [1, 3, 4, 5, 9]


def _op():
    import centerclip_amd.torch_ops  # noqa: F401  (registers torch.ops.centerclip)
    return torch.ops.centerclip


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ================================================================================================ rank counts
def _tied(rows, cols, g, seed):
    """fp32 [rows, cols] of small integers / 4 (many exact ties in every row) with, per row and off its truth column g[i]
    (None: no truth column), -0.0 next to +0.0, +inf, -inf and a NaN planted as far as the row has room; the truth entry
    itself is left, or made NaN / -0.0 / +inf / -inf, by turns."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-8, 9, size=(rows, cols)) / 4).astype(np.float32)
    for i in range(rows):
        gi = -1 if g is None else int(g[i])
        pairs = [j for j in rng.permutation(max(cols - 1, 0)) if gi not in (j, j + 1)]
        taken = {gi}
        if pairs:
            s[i, pairs[0]], s[i, pairs[0] + 1] = -0.0, 0.0
            taken |= {int(pairs[0]), int(pairs[0]) + 1}
        free = [j for j in rng.permutation(cols) if j not in taken]
        for j, v in zip(free, (np.inf, -np.inf, np.nan)):
            s[i, j] = v
        if gi >= 0:
            kind = i % 5 if rows > 1 else seed % 5               # row 1 of every matrix: a NaN truth entry
            if kind:
                s[i, gi] = (np.nan, -0.0, np.inf, -np.inf)[kind - 1]
    return s


def _check2(counts, s, g_or_vals, what):
    gt, eq, _ = mr.rank_counts_ref(s, g_or_vals)
    got = counts.cpu().numpy()
    assert got.shape == (s.shape[0], 2) and got.dtype == np.int32
    assert np.array_equal(got[:, 0], gt) and np.array_equal(got[:, 1], eq), (what, got.tolist(), gt.tolist(), eq.tolist())


@pytest.mark.parametrize("cols", COLS)
def test_rank_counts_diagonals_transposed_and_strided(cols):
    """cc_rank_counts_f32: the truth column of row i is diag_offset + i, for offsets 0, 3 and cols - rows (the last legal
    one), on the contiguous matrix, on its transpose through transpose=True (a [cols, rows] tensor: not square) and on two
    views of wider buffers (a row stride; a column stride of 2 over cells that would change every count if read)."""
    from centerclip_amd._lib import CenterClipHipError
    op = _op()
    for rows in ROWS:
        if rows > cols:
            with pytest.raises(CenterClipHipError, match=r"invalid argument \(-1\)"):
                op.rank_counts(torch.zeros(rows, cols, device=DEV), False, 0)
            continue
        for off in sorted({0, 3, cols - rows}):
            if off + rows > cols:
                continue
            g = off + np.arange(rows)
            s = _tied(rows, cols, g, 100 * cols + 10 * rows + off)
            if rows >= 3:                                        # NaN at the truth column: all counts 0
                assert np.isnan(s[np.arange(rows), g]).any()
            d = _dev(s)
            _check2(op.rank_counts(d, False, off), s, g, ("plain", rows, cols, off))
            t = _dev(s.T)
            assert t.shape == (cols, rows)
            _check2(op.rank_counts(t, True, off), s, g, ("transposed", rows, cols, off))
            wide = torch.full((rows, cols + 7), 1e9, device=DEV)
            wide[:, 2:2 + cols] = d
            _check2(op.rank_counts(wide[:, 2:2 + cols], False, off), s, g, ("row stride", rows, cols, off))
            wide2 = torch.full((rows, 2 * cols + 3), 1e9, device=DEV)
            view = wide2[:, 1:1 + 2 * cols:2]
            view.copy_(d)
            assert view.shape == (rows, cols) and (cols == 1 or view.stride() == (2 * cols + 3, 2))
            _check2(op.rank_counts(view, False, off), s, g, ("column stride", rows, cols, off))
        for bad in (cols - rows + 1, -1):                          # diag_offset + rows > cols: CC_ERR_INVALID (-1)
            with pytest.raises(CenterClipHipError, match=r"invalid argument \(-1\)"):
                op.rank_counts(torch.zeros(rows, cols, device=DEV), False, bad)


def test_rank_counts_metrics_wrapper_is_the_op():
    from centerclip_amd.metrics import rank_counts
    g = np.arange(5)
    s = _tied(5, 65, g, 3)
    _check2(rank_counts(_dev(s)), s, g, "metrics.rank_counts")
    _check2(rank_counts(_dev(s.T), transpose=True), s, g, "metrics.rank_counts transposed")


@pytest.mark.parametrize("cols", COLS)
def test_rank_counts_cols_edge_columns(cols):
    """cc_rank_counts_cols_f32: truth columns all 0, all C - 1 and drawn with repeats; the third count is the number of
    entries equal to the truth value IN FRONT of the truth column."""
    op = _op()
    for rows in ROWS:
        rng = np.random.default_rng(cols + rows)
        drawn = rng.integers(0, cols, size=rows)
        if rows > 1:
            drawn[1] = drawn[0]
        for tag, g in (("first", np.zeros(rows, np.int64)), ("last", np.full(rows, cols - 1)), ("repeated", drawn)):
            s = _tied(rows, cols, g, 1000 * cols + 10 * rows + len(tag))
            gt, eq, front = mr.rank_counts_ref(s, g)
            got = op.rank_counts_cols(_dev(s), _dev(g, torch.int32)).cpu().numpy()
            assert got.shape == (rows, 3) and got.dtype == np.int32
            assert np.array_equal(got, np.stack([gt, eq, front], 1)), (tag, rows, cols, got.tolist())
            if tag == "first":
                assert not got[:, 2].any()
            if tag == "last" and cols > 1:
                assert np.array_equal(got[:, 2], np.maximum(got[:, 1] - 1, 0))       # every other tie stands in front


@pytest.mark.parametrize("cols", COLS)
def test_rank_counts_ref_values(cols):
    """cc_rank_counts_ref_f32: the value to rank against is handed in - one that occurs in the row, one that does not (the
    fill is in quarters, 0.125 is absent: eq == 0), NaN (0, 0), +0.0 (equal to the row's -0.0 and +0.0) and +inf, by turns;
    rows of sim and, through the strides, columns of its transpose."""
    op = _op()
    for rows in ROWS:
        s = _tied(rows, cols, None, 77 * cols + rows)
        rng = np.random.default_rng(cols * rows)
        vals = np.empty(rows, np.float32)
        for i in range(rows):
            kind = (i + cols) % 5
            vals[i] = (s[i, rng.integers(0, cols)], 0.125, np.nan, 0.0, np.inf)[kind]
        gt, eq, _ = mr.rank_counts_ref(s, vals)
        absent = vals == np.float32(0.125)
        assert not eq[absent].any() and not gt[np.isnan(vals)].any() and not eq[np.isnan(vals)].any()
        _check2(op.rank_counts_ref(_dev(s), _dev(vals), False), s, vals, ("rows", rows, cols))
        _check2(op.rank_counts_ref(_dev(s.T), _dev(vals), True), s, vals, ("columns", rows, cols))


# ================================================================================================ group maxima
def _group_case(rows, cols, seed):
    """Values in quarters (never -0.0) with NaN, +inf and -inf sprinkled; group ids in runs of 1 ... 40 rows that skip ids (empty
    groups), one run laid over the 64-row chunk boundary, the first id coming back on the last row, ids -1 and n_groups on two
    rows, one group all NaN, one group all negative."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-8, 9, size=(rows, cols)) / 4).astype(np.float32)
    ids, gid = [], 0
    while len(ids) < rows:
        ids += [gid] * int(rng.integers(1, 41))
        gid += int(rng.integers(1, 3))
    ids = np.array(ids[:rows], dtype=np.int32)
    n_groups = gid + 2
    if rows >= 70:
        ids[58:70] = ids[58]                                       # rows 58 ... 69: chunks 0 and 1
    if rows > 2:
        ids[rows - 1] = ids[0]                                     # not a neighbour of the group's other rows
    if rows >= 8:
        ids[3], ids[6] = -1, n_groups
    mask = rng.uniform(size=s.shape)
    s[mask < 0.05] = np.nan
    s[(mask >= 0.05) & (mask < 0.07)] = np.inf
    s[(mask >= 0.07) & (mask < 0.10)] = -np.inf
    if rows >= 8:
        real = [g for g in np.unique(ids) if 0 <= g < n_groups]
        s[ids == real[len(real) // 2]] = np.nan
        neg = ids == real[-1]
        s[neg] = -np.abs(rng.integers(1, 9, size=(int(neg.sum()), cols)) / 4).astype(np.float32)
    return s, ids, n_groups


def _group_check(got, ref):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and not np.isnan(got).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), "the -inf pattern differs"
    assert np.array_equal(got, ref)                                # == entry for entry; the sign of a zero is not compared


@pytest.mark.parametrize("rows,cols", [(0, 257), (1, 1), (63, 255), (64, 256), (65, 257), (130, 1), (130, 256), (130, 257)])
def test_group_max_rows_against_reference(rows, cols):
    op = _op()
    s, ids, n_groups = _group_case(rows, cols, 31 * rows + cols)
    ref = mr.group_max_ref(s, ids, n_groups)
    if rows >= 8:
        assert np.isneginf(ref).all(axis=1).sum() >= 3              # empty groups and the all-NaN one
        assert (ref[~np.isneginf(ref).all(axis=1)].max(axis=1) < 0).any()           # the all-negative one
    d, gd = _dev(s) if rows else torch.zeros(0, cols, device=DEV), _dev(ids)
    a = op.group_max_rows(d, gd, n_groups)
    _group_check(a, ref)
    b = op.group_max_rows(d, gd, n_groups)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ in bits"
    wide = torch.full((rows, cols + 9), float("inf"), device=DEV)   # a view with a row stride > cols
    wide[:, :cols] = d
    assert rows < 2 or not wide[:, :cols].is_contiguous()
    _group_check(op.group_max_rows(wide[:, :cols], gd, n_groups), ref)


@pytest.mark.parametrize("where", ["same_chunk", "other_chunk", "alone"])
def test_group_max_of_negative_zero(where):
    """A group whose best entry is -0.0 and whose other entries are negative: the maximum is a zero, not -inf and not the
    best negative.  `same_chunk`: the thread that walks the chunk publishes -0.0 once, against the -inf fill; `other_chunk`:
    the -0.0 and the negatives are published by different chunks (on even columns the -0.0 lies in chunk 0, on odd ones in
    chunk 1), against each other in either order; `alone`: a one-row group of -0.0."""
    op = _op()
    rows, cols, n_groups = 130, 257, 4
    rng = np.random.default_rng(5)
    s = -(rng.integers(1, 9, size=(rows, cols)) / 4).astype(np.float32)
    ids = np.full(rows, 1, np.int32)
    even = np.arange(cols) % 2 == 0
    if where == "same_chunk":
        ids[10:21] = 2
        s[15, :] = -0.0
    elif where == "other_chunk":
        ids[62:67] = 2
        s[63, even] = -0.0
        s[65, ~even] = -0.0
    else:
        ids[129] = 2
        s[129, :] = -0.0
    ref = mr.group_max_ref(s, ids, n_groups)
    assert (ref[2] == 0).all() and (ref[1] < 0).all() and np.isneginf(ref[[0, 3]]).all()
    got = op.group_max_rows(_dev(s), _dev(ids), n_groups)
    _group_check(got, ref)


# ================================================================================================ loss values
def _loss_check(tag, dev_sim, host_sim):
    ref, bound = mr.crossen_ref(host_sim), mr.crossen_bound(host_sim)
    got = _op().contrastive_loss(dev_sim).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print("contrastive_loss %-18s loss %.6g  max error / bound = %.3f" % (tag, ref[2], ratio.max()))
    assert got.shape == (3,) and np.all(ratio <= 1), (tag, got, ref, bound)


@pytest.mark.parametrize("scale", [1, 100])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 257, 300])
def test_contrastive_loss_against_float64(n, scale):
    sim = mr.loss_case(n, scale)
    _loss_check("n=%d scale=%d" % (n, scale), _dev(sim), sim)


def test_contrastive_loss_with_masked_entries():
    """-1e30 is what nan_to_num writes for the logits of a fully masked clip: such entries carry no weight."""
    sim = mr.loss_case(65, 100)
    for i, j in ((0, 64), (7, 3), (64, 0), (30, 31), (31, 30)):
        sim[i, j] = -1e30
    _loss_check("n=65 -1e30", _dev(sim), sim)


def test_contrastive_loss_on_views():
    sim = mr.loss_case(65, 100, seed=1)
    sim[0, 5] += 3.0                                               # rows and columns differ visibly
    d = _dev(sim)
    _loss_check("n=65 sim.t()", d.t(), sim.T)
    ref = mr.crossen_ref(sim)
    assert abs(ref[0] - ref[1]) > 1e-3 and np.allclose(mr.crossen_ref(sim.T)[:2], ref[1::-1], rtol=0, atol=1e-12)
    buf = torch.full((70, 140), 1e9, device=DEV)
    view = buf[2:67, 3:133:2]
    view.copy_(d)
    assert view.shape == (65, 65) and view.stride() == (140, 2)
    _loss_check("n=65 strided view", view, sim)


# ================================================================================================ head projection
HEAD_SHAPES = [(4, 4), (100, 60), (192, 64), (512, 68), (768, 512), (1024, 768)]
HEAD_SPECIAL = {"row_mul7": dict(W=192, E=64, R=5, row_mul=7), "row_idx": dict(W=192, E=64, R=5, with_idx=True),
                "mean100": dict(W=768, E=512, R=5, mean=100.0, std=1.0), "gamma0": dict(W=768, E=512, R=5, gamma_zero=True),
                "std0.01": dict(W=768, E=512, R=5, mean=0.0, std=0.01)}


def _head_check(tag, c):
    from centerclip_amd import ops
    ref = mr.head_project_ref(c["h"], c["row_of"], c["gamma"], c["beta"], c["proj"])
    bound = mr.head_project_bound(c["h"], c["row_of"], c["gamma"], c["beta"], c["proj"])
    got = ops.head_project(_dev(c["h"]), _dev(c["gamma"]), _dev(c["beta"]), _dev(c["proj"]), row_mul=c["row_mul"],
                           row_idx=None if c["row_idx"] is None else _dev(c["row_idx"]), rows=len(c["row_of"]))
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    ratio = np.abs(got - ref) / bound
    print("head_project %-22s max|out| %.3g  max error / bound = %.3f" % (tag, np.abs(ref).max(), ratio.max()))
    assert np.all(ratio <= 1), (tag, float(ratio.max()))


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("W,E", HEAD_SHAPES)
def test_head_project_against_float64(W, E, R):
    _head_check("W=%d E=%d R=%d" % (W, E, R), mr.head_case(W, E, R))


@pytest.mark.parametrize("tag", sorted(HEAD_SPECIAL))
def test_head_project_special_rows(tag):
    c = mr.head_case(**HEAD_SPECIAL[tag])
    if tag == "row_mul7":
        assert c["h"].shape[0] == 35 and c["row_of"].tolist() == [0, 7, 14, 21, 28]
    if tag == "row_idx":
        assert (c["row_of"] != np.arange(5)).any()
    _head_check(tag, c)


def test_head_project_refuses_rows_wider_than_its_lds():
    """W = 1028 > 1024 would overrun xn[1024] in LDS: CC_ERR_UNSUPPORTED (-2), nothing is launched."""
    from centerclip_amd import ops
    from centerclip_amd._lib import CenterClipHipError
    h, g, p = torch.zeros(2, 1028, device=DEV), torch.ones(1028, device=DEV), torch.zeros(1028, 64, device=DEV)
    with pytest.raises(CenterClipHipError, match=r"unsupported configuration \(-2\)"):
        ops.head_project(h, g, g, p)


# ================================================================================================ wrapper refusals
def test_wrappers_refuse_what_the_kernels_would_misread():
    """contrastive_loss, rank_counts_cols, rank_counts_ref and group_max_rows hand bare pointers to the kernels: a tensor of
    another dtype, shape, layout or device is refused from its metadata, before any launch (the tensors here are never read:
    the CPU ones could not be)."""
    op = _op()
    sim = torch.zeros(6, 8, device=DEV)
    sq = torch.zeros(6, 6, device=DEV)
    g32 = torch.zeros(6, dtype=torch.int32, device=DEV)
    v32 = torch.zeros(6, device=DEV)
    bad = [
        lambda: op.contrastive_loss(sim),                                         # not square
        lambda: op.contrastive_loss(torch.zeros(6, device=DEV)),                   # not 2-D
        lambda: op.contrastive_loss(torch.zeros(2, 6, 6, device=DEV)),
        lambda: op.contrastive_loss(sq.half()),                                    # not fp32
        lambda: op.contrastive_loss(sq.double()),
        lambda: op.rank_counts_cols(torch.zeros(8, 6, device=DEV).t(), g32),       # not contiguous
        lambda: op.rank_counts_cols(torch.zeros(6, 16, device=DEV)[:, ::2], g32),
        lambda: op.rank_counts_cols(sim.half(), g32),
        lambda: op.rank_counts_cols(sim, g32.long()),                              # dtype
        lambda: op.rank_counts_cols(sim, g32[:5]),                                 # length
        lambda: op.rank_counts_cols(sim, torch.zeros(12, dtype=torch.int32, device=DEV)[::2]),
        lambda: op.rank_counts_cols(sim, g32.cpu()),                               # device
        lambda: op.rank_counts_ref(sim, v32.double(), False),
        lambda: op.rank_counts_ref(sim, v32, True),                                # 8 columns, 6 values
        lambda: op.rank_counts_ref(sim, torch.zeros(8, device=DEV), False),
        lambda: op.rank_counts_ref(sim, v32.cpu(), False),
        lambda: op.rank_counts_ref(sim.double(), v32, False),
        lambda: op.group_max_rows(sim, g32.long(), 3),
        lambda: op.group_max_rows(sim, g32[:5], 3),
        lambda: op.group_max_rows(sim, g32.cpu(), 3),
        lambda: op.group_max_rows(torch.zeros(8, 6, device=DEV).t(), g32, 3),      # column stride 6
        lambda: op.group_max_rows(torch.zeros(6, 16, device=DEV)[:, ::2], g32, 3),
        lambda: op.group_max_rows(sim.half(), g32, 3),
        lambda: op.group_max_rows(sim, g32, 0),
        lambda: op.group_max_rows(sim, g32, -1),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was not refused" % i)
    # the same tensors, well-formed: accepted
    assert op.contrastive_loss(sq).shape == (3,) and op.rank_counts_cols(sim, g32).shape == (6, 3)
    assert op.rank_counts_ref(sim, torch.zeros(8, device=DEV), True).shape == (8, 2)
    assert op.group_max_rows(sim, g32, 3).shape == (3, 8)
