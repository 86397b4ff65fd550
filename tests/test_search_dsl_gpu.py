"""Dual-softmax (camoe_dsl) search on the MI355X (``-m gpu``): torch.ops.centerclip.dsl_col_stats_planes and similarity_topk_dsl
against the existing ops they must reproduce, and FeatureGallery(dual_softmax=True) on the small model.

References (existing code, never the code under test):
    S = scaled_dot_planes(text planes, video copy padded with zero rows, n_video, mult, products)          [Bt, Bv]
    m: S.max(0), bit for bit.   s: float64 col_stats64(S) within the bound below.
    D = dsl_apply_(copy of S, m, s, n_total);  order = np.argsort(-D, kind="stable")[:, :k]: ids equal, scores bit-equal.

The bound on s is dsl_ref.stats_bound's rule - every fp32 operation a term passes through costs one unit roundoff U of the
running magnitude (all terms are positive: the magnitude is s), and the subtractions inside expf cost |x - m| U on the exponent
because the partial maxima rise from x to m - with the depth of cc_dsl_col_stats_planes_f32's tree (csrc/search.hip):
  * lane: per 16-row text tile of its wave  s <- (((s * expf(m - m') + e0) + e1) + e2) + e3, e_r = expf(x_r - m'): an old term
    passes expf (2 U allowed, as dsl_ref) + 1 multiplication + 4 additions = 7 roundings a tile, a new one 2 + at most 4;
    a wave takes every fourth tile of its slice, a slice holds at most ceil(tiles / slices) tiles:
    chain = ceil(ceil(tiles / slices) / 4) steps;
  * workgroup: 16 pairs (4 waves x 4 lane groups) under their maximum: expf 2 + 1 multiplication + 16 additions = 19;
  * second launch: the slices' pairs under their maximum: expf 2 + 1 multiplication + one addition per slice = slices + 3.
  depth = 7 * chain + 19 + slices + 3,   |s - s64| <= U * (depth * s64 + sum_i |x_i - m| exp(x_i - m)).
D then carries it as dsl_ref.d_bound does."""
import io
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

import dsl_ref as R
from centerclip_amd import _lib as L
from test_search_gpu import (BQS, DEV, KS, MULT, N_CLIPS, NS, PRODUCTS, _assert_topk, _bits, _dataset, _eval_model,
                             _matrix, _planes, _split, g2)  # noqa: F401  (g2: the fixture)

pytestmark = pytest.mark.gpu
op = torch.ops.centerclip
BEHIND = 37                                                               # non-zero rows behind n, on both sides


def planes_stats_bound(S, slices):
    """-> (bound [cols], depth) for the [Bt, Bv] fp32 matrix S (texts as rows): the docstring's rule"""
    x = np.asarray(S, dtype=np.float64)
    tiles = -(-x.shape[0] // 16)
    chain = -(-(-(-tiles // slices)) // 4)
    depth = 7 * chain + 19 + slices + 3
    m, s64 = R.col_stats64(x)
    t = np.exp(x - m[None, :])
    return R.U * (depth * s64 + (np.abs(x - m[None, :]) * t).sum(axis=0)), depth


def _text_video(seed, Bt, Bv, E):
    g = torch.Generator().manual_seed(seed)
    return _planes(torch.randn(Bt + BEHIND, E, generator=g), False), _planes(torch.randn(Bv + BEHIND, E, generator=g), True)


def _S(text, video, Bt, Bv, products, mult=MULT):
    return _matrix(text[:Bt].contiguous(), video, Bv, mult, products)


def _u32(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. statistics
STATS = [(1, 1, 64, 1), (3, 5, 64, 2), (17, 33, 64, 3), (257, 130, 64, 1), (1203, 517, 64, 2), (4099, 5, 64, 3),
         (300, 40, 512, 2)]
_stats_cache = {}


def _stats_case(Bt, Bv, E, products):
    """the planes, the matrix op's S and its float64 statistics, computed once per shape and left unchanged"""
    key = (Bt, Bv, E, products)
    if key not in _stats_cache:
        text, video = _text_video(7 * Bt + Bv, Bt, Bv, E)
        S = _S(text, video, Bt, Bv, products)
        Sn = S.cpu().numpy()
        _stats_cache[key] = (text, video, S, Sn) + R.col_stats64(Sn)
    return _stats_cache[key]


@pytest.mark.parametrize("Bt,Bv,E,products", STATS)
def test_statistics_against_the_matrix_op(Bt, Bv, E, products):
    text, video, S, Sn, m64, s64 = _stats_case(Bt, Bv, E, products)
    slices = L.lib().cc_dsl_col_stats_planes_slices(Bt)
    if Bt == 4099:
        assert slices >= 2
    m, s = op.dsl_col_stats_planes(text, video, Bt, Bv, MULT, products)
    m2, s2 = op.dsl_col_stats_planes(text, video, Bt, Bv, MULT, products)
    assert m.shape == s.shape == (Bv,) and m.dtype == s.dtype == torch.float32
    assert torch.equal(_u32(m), _u32(m2)) and torch.equal(_u32(s), _u32(s2))               # the same bits on every run
    assert torch.equal(_u32(m), _u32(S.max(dim=0).values))                                 # the matrix op's column maximum
    assert np.array_equal(m.cpu().numpy().astype(np.float64), m64)
    bound, depth = planes_stats_bound(Sn, slices)
    err = np.abs(s.cpu().numpy().astype(np.float64) - s64)
    print(f"[dsl planes stats {Bt}x{Bv} E{E} p{products}] slices {slices} depth {depth}: max |s - s64| / s64 = "
          f"{float((err / s64).max()):.2e}, worst |s - s64| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    D = S.clone()
    op.dsl_apply_(D, m, s, Bt)
    db = R.d_bound(Sn, Bt, bound)
    derr = np.abs(D.cpu().numpy().astype(np.float64) - R.dual_softmax64(Sn))
    print(f"[dsl planes stats {Bt}x{Bv} E{E} p{products}] worst |D - D64| / d_bound = {float((derr / db).max()):.3f}")
    assert (derr <= db).all()


def test_statistics_of_no_text_row_are_the_neutral_pair():
    text, video = _text_video(5, 4, 19, 64)
    m, s = op.dsl_col_stats_planes(text, video, 0, 19, MULT, 2)
    assert bool(torch.isneginf(m).all()) and bool((s == 0).all()) and m.shape == (19,)
    m, s = op.dsl_col_stats_planes(text[:0], video, 0, 19, MULT, 2)                        # (no text storage at all)
    assert bool(torch.isneginf(m).all()) and bool((s == 0).all())


@pytest.mark.parametrize("Bt", [257, 4099])
def test_a_video_rows_pair_does_not_depend_on_the_rows_it_shares_the_call_with(Bt):
    text, video = _text_video(31 + Bt, Bt, 100, 64)
    m, s = op.dsl_col_stats_planes(text, video, Bt, 100, MULT, 2)
    at = 0
    for chunk in (1, 16, 17, 66):
        mc, sc = op.dsl_col_stats_planes(text, video[at:at + chunk], Bt, chunk, MULT, 2)
        assert torch.equal(_u32(mc), _u32(m[at:at + chunk])) and torch.equal(_u32(sc), _u32(s[at:at + chunk])), chunk
        at += chunk
    assert at == 100


# ------------------------------------------------------------------------------------------------ 2. top-k
def _sweep():
    """tests/test_search_gpu.py::_sweep's recipe: every axis dealt out in a shuffled cycle over 12 cases, two more for k > n
    from both sides of a tile; then the statistics' side and source dealt over them.  One gallery row (n = 1) has no order
    to change, and one query row under its own statistics has D = S (softmax over one text = 1), so those cases get
    query-side resp. handed-in statistics; k = 1 on the gallery side gets handed-in statistics too (they move the maximum)."""
    rng = np.random.default_rng(20261)
    cols = [[axis[i] for i in np.resize(rng.permutation(len(axis)), 12)] for axis in (BQS, NS, KS, PRODUCTS)]
    cases = list(zip(*cols)) + [(17, 15, 65, 2), (1, 1, 128, 3)]
    for axis, col in zip((BQS, NS, KS, PRODUCTS), zip(*cases)):
        assert set(axis) == set(col)
    assert any(k > n for _, n, k, _ in cases)
    out = []
    for i, (Bq, n, k, products) in enumerate(cases):
        side = 0 if n == 1 else (i + 1) % 2
        given = (i // 2) % 2 == 1 or (side == 1 and (Bq == 1 or k == 1))
        out.append((int(Bq), int(n), int(k), int(products), side, "given" if given else "op"))
    assert {(c[4], c[5]) for c in out} == {(0, "op"), (0, "given"), (1, "op"), (1, "given")}
    return out


def _given_stats(S_tv, seed):
    """statistics handed in for the columns of S_tv [texts, videos]: m within +-20 of a score of the column, s log-uniform in
    [1, 1e3]"""
    rng = np.random.default_rng(seed)
    Sn = S_tv.cpu().numpy()
    pick = Sn[rng.integers(0, Sn.shape[0], size=Sn.shape[1]), np.arange(Sn.shape[1])]
    m = (pick + rng.uniform(-20, 20, size=Sn.shape[1])).astype(np.float32)
    s = np.exp(rng.uniform(0, math.log(1e3), size=Sn.shape[1])).astype(np.float32)
    return torch.from_numpy(m).to(DEV), torch.from_numpy(s).to(DEV)


def _order_differs(D, S, k):
    Dn, Sn = D.cpu().numpy(), S.cpu().numpy()
    return not np.array_equal(np.argsort(-Dn, axis=1, kind="stable")[:, :k], np.argsort(-Sn, axis=1, kind="stable")[:, :k])


def _check_dsl(q, gal, n, products, k, side, source, seed=0, n_total=None, mult=MULT):
    """q / gal: query / gallery planes.  side 1: text queries, a clip gallery, statistics per gallery row over the queries (or
    handed in); side 0: clip queries, a caption gallery, statistics per query row over the gallery (or handed in)."""
    Bq = q.shape[0]
    if side:
        S_tv = _matrix(q, gal, n, mult, products)                                          # [Bq texts, n videos]
        stats = op.dsl_col_stats_planes(q, gal, Bq, n, mult, products) if source == "op" else _given_stats(S_tv, seed)
        nt = (Bq if source == "op" else 1000) if n_total is None else n_total
    else:
        S_tv = _matrix(gal[:n].contiguous(), q, Bq, mult, products)                        # [n texts, Bq videos]
        stats = op.dsl_col_stats_planes(gal, q, n, Bq, mult, products) if source == "op" else _given_stats(S_tv, seed)
        nt = (n if source == "op" else 1000) if n_total is None else n_total
    D = S_tv.clone()
    op.dsl_apply_(D, stats[0], stats[1], nt)
    S_qg, D_qg = (S_tv, D) if side else (S_tv.t().contiguous(), D.t().contiguous())
    if side and n > 1:
        assert _order_differs(D_qg, S_qg, k), "the case cannot tell D from S"              # a kernel that ranks S must fail
    if side:                                                                               # statistics behind n: never read
        stats = tuple(torch.cat([t, torch.full((5,), float("nan"), device=DEV)]) for t in stats)
    scores, ids = op.similarity_topk_dsl(q, gal, n, mult, products, k, stats[0], stats[1], side, nt)
    _assert_topk(scores, ids, D_qg, k)
    return scores, ids, D_qg


@pytest.mark.parametrize("Bq,n,k,products,side,source", _sweep())
def test_shape_sweep_e64(Bq, n, k, products, side, source):
    g = torch.Generator().manual_seed(1000 * Bq + n + k)
    queries, rows = torch.randn(Bq, 64, generator=g), torch.randn(n + BEHIND, 64, generator=g)
    q, gal = _planes(queries, not side), _planes(rows, bool(side))
    _check_dsl(q, gal, n, products, k, side, source, seed=Bq + n)


def test_identical_gallery_rows_with_identical_statistics_come_in_id_order():
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(5, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(4099, 64), True)
    m, s = torch.full((4099,), 3.0, device=DEV), torch.full((4099,), 7.0, device=DEV)
    D = _matrix(q, gal, 4099, MULT, 2)
    op.dsl_apply_(D, m, s, 5)
    for k in (10, 128):
        scores, ids = op.similarity_topk_dsl(q, gal, 4099, MULT, 2, k, m, s, 1, 5)
        _assert_topk(scores, ids, D, k)
        assert torch.equal(ids.cpu(), torch.arange(k).expand(5, k))


def test_one_row_under_seven_distinct_statistics():
    n = 4099
    g = torch.Generator().manual_seed(13)
    q = _planes(torch.randn(17, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(n, 64), True)
    rng = np.random.default_rng(13)
    pick = rng.integers(0, 7, size=n)
    m = torch.from_numpy(rng.uniform(-20, 20, size=7).astype(np.float32)[pick]).to(DEV)
    s = torch.from_numpy(np.exp(rng.uniform(0, math.log(1e3), size=7)).astype(np.float32)[pick]).to(DEV)
    S = _matrix(q, gal, n, MULT, 3)
    D = S.clone()
    op.dsl_apply_(D, m, s, 17)
    assert len(np.unique(S.cpu().numpy()[0])) == 1 and len(np.unique(D.cpu().numpy()[0])) == 7
    for k in (1, 65, 128):
        scores, ids = op.similarity_topk_dsl(q, gal, n, MULT, 3, k, m, s, 1, 17)
        _assert_topk(scores, ids, D, k)


def test_underflow_gives_negative_zeros_in_id_order():
    """Captions opposite to the query clips, query-side statistics with m = +20: S = -mult, expf(S - m) underflows to 0 and
    every D is (n * S) * 0 = -0.0 - equal scores, id order, the sign bit kept."""
    n, k = 1000, 65
    g = torch.Generator().manual_seed(17)
    x = torch.randn(1, 64, generator=g)
    q = _planes(x.expand(3, 64), True)
    gal = _planes((-x).expand(n + 3, 64), False)
    m, s = torch.full((3,), 20.0, device=DEV), torch.full((3,), 2.0, device=DEV)
    D = _matrix(gal[:n].contiguous(), q, 3, MULT, 2)
    assert float(D.max()) < -90.0
    op.dsl_apply_(D, m, s, n)
    scores, ids = op.similarity_topk_dsl(q, gal, n, MULT, 2, k, m, s, 0, n)
    _assert_topk(scores, ids, D.t().contiguous(), k)
    assert bool((_u32(scores) == -(1 << 31)).all())                                        # 0x80000000: -0.0
    assert torch.equal(ids.cpu(), torch.arange(k).expand(3, k))


def test_many_slices_and_many_video_groups():
    Bq, n, k = 3, 200003, 100
    assert L.lib().cc_similarity_topk_slices(Bq, n, k) >= 3
    g = torch.Generator(device=DEV).manual_seed(14)
    gal = op.normalize_rows_planes(torch.randn(n + 5, 64, device=DEV, generator=g), True)
    q = op.normalize_rows_planes(torch.randn(Bq, 64, device=DEV, generator=g), False)
    # the statistics of 200,003 clips (12,501 groups of video rows) over the 3 captions ...
    Sn = _matrix(q, gal, n, MULT, 2).cpu().numpy()
    m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, 2)
    m64, s64 = R.col_stats64(Sn)
    assert np.array_equal(m.cpu().numpy().astype(np.float64), m64)
    assert (np.abs(s.cpu().numpy().astype(np.float64) - s64) <= planes_stats_bound(Sn, 1)[0]).all()
    # ... leave the first 100 of a row in S's order (where a score is large its softmax over 3 captions is 1): the top-k
    # takes handed-in statistics
    _check_dsl(q, gal, n, 2, k, 1, "given", seed=14)


def test_graph_capture_and_replay_of_statistics_and_topk():
    """a caption gallery: the query clips' statistics over the gallery and the top-k under them, in one graph"""
    Bq, n, k = 5, 4099, 10
    g = torch.Generator().manual_seed(15)
    gal = _planes(torch.randn(n, 64, generator=g), False)
    q, q2 = _planes(torch.randn(Bq, 64, generator=g), True), _planes(torch.randn(Bq, 64, generator=g), True)

    def run(x):
        m, s = op.dsl_col_stats_planes(gal, x, n, Bq, MULT, 2)
        return (m, s) + tuple(op.similarity_topk_dsl(x, gal, n, MULT, 2, k, m, s, 0, n))
    qbuf = q.clone()
    run(qbuf)                                                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m, s, scores, ids = run(qbuf)
    for new in (q2, q):
        qbuf.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        wm, ws, wscores, wids = run(new)
        assert torch.equal(_u32(m), _u32(wm)) and torch.equal(_u32(s), _u32(ws))
        assert torch.equal(ids, wids) and torch.equal(_u32(scores), _u32(wscores))
        D = _matrix(gal, new, Bq, MULT, 2)
        op.dsl_apply_(D, wm, ws, n)
        _assert_topk(scores, ids, D.t().contiguous(), k)


# ------------------------------------------------------------------------------------------------ 3. FeatureGallery
@pytest.mark.parametrize("cluster_inter", [0, 1])
def test_feature_gallery_dual_softmax_on_the_small_model(g2, cluster_inter):
    from centerclip_amd import eval as E
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, cluster_inter)
    video, vmask, ids = _dataset(g2["s1_cfg"])
    n = N_CLIPS
    with torch.no_grad():
        seq = model(input_ids=ids)['sequence_output']
        vis_list = [model(video=v, video_mask=m)['visual_output'] for v, m in zip(_split(video), _split(vmask))]
        masks = [(m,) for m in _split(vmask)]
        S = E._similarity_matrix(model, None, masks, [seq], vis_list)
        D_run = E._run_on_single_gpu(model, None, masks, [seq], vis_list, args=Namespace(camoe_dsl=1))
    Sn = S.cpu().numpy()
    # side="video", the bank = the captions, set before the clips arrive in uneven batches (the buffer grows 4 -> 8 -> 16)
    gal = FeatureGallery(model, capacity=4, dual_softmax=True)
    with pytest.raises(ValueError, match="set_query_bank"):
        gal.search(ids[:2], k=3)
    gal.set_query_bank(ids)
    s0, i0 = gal.search(ids[:2], k=3)                                      # an empty gallery: the fill alone
    assert bool((i0 == -1).all()) and bool(torch.isneginf(s0).all())
    pos = [gal.add(v, m) for v, m in zip(_split(video), _split(vmask))]
    assert torch.equal(torch.cat(pos), torch.arange(n)) and len(gal) == n
    D = gal.similarity(ids)
    assert _bits(gal.similarity_features(seq), D) and D.shape == (n, n)
    assert torch.equal(_u32(gal._m[:n]), _u32(S.max(dim=0).values))
    bound, depth = planes_stats_bound(Sn, L.lib().cc_dsl_col_stats_planes_slices(n))
    db = R.d_bound(Sn, n, bound)
    Dn = D.cpu().numpy().astype(np.float64)
    derr, rerr = np.abs(Dn - R.dual_softmax64(Sn)), np.abs(Dn - D_run.astype(np.float64))
    print(f"[FeatureGallery dual_softmax, cluster_inter={cluster_inter}] depth {depth}: worst |D - D64| / d_bound = "
          f"{float((derr / db).max()):.3f}, against _run_on_single_gpu {float((rerr / db).max()):.3f}")
    assert (derr <= db).all() and (rerr <= db).all()
    for k in (1, 5, 20):                                                   # 20 > 12 clips: the fill
        scores, idx = gal.search(ids, k=k)
        _assert_topk(scores, idx, D, k)
        s2, i2 = gal.search_features(seq, k=k)
        assert _bits(s2, scores) and torch.equal(i2, idx)
    # the bank after the clips, other batches, no growth / other growth: the same bits
    feats = torch.cat(vis_list)
    for capacity, cuts in ((16, (12,)), (0, (1, 11)), (2, (7, 2, 3))):
        other = FeatureGallery(model, capacity=capacity, dual_softmax=True)
        for f, m in zip(torch.split(feats, list(cuts)), torch.split(vmask, list(cuts))):
            other.add_features(f, m)
        other.set_query_bank_features(seq)
        assert _bits(other.rows, gal.rows) and _bits(other._m[:n], gal._m[:n]) and _bits(other._s[:n], gal._s[:n]), cuts
        a, b = other.search(ids, k=5), gal.search(ids, k=5)
        assert _bits(a[0], b[0]) and torch.equal(a[1], b[1])
    other.set_query_bank_features(seq[:7])                                 # replacing the bank recomputes every pair
    assert not _bits(other._s[:n], gal._s[:n]) and torch.equal(_u32(other._m[:n]), _u32(S[:7].max(dim=0).values))
    sc, ix = other.search_features(seq[:7], k=4)
    _assert_topk(sc, ix, other.similarity_features(seq[:7]), 4)
    # side="text": rows of D^T, the statistics taken at search time over the captions held
    tg = FeatureGallery(model, side="text", capacity=4, dual_softmax=True)
    with pytest.raises(ValueError):
        tg.set_query_bank(ids)
    for b in _split(ids):
        tg.add(b)
    Dt = D.t().contiguous()
    assert _bits(tg.similarity_features(feats, vmask), Dt)
    scores, idx = tg.search_features(feats, k=7, mask=vmask)
    _assert_topk(scores, idx, Dt, 7)
    scores, idx = tg.search(video, vmask, k=7)                             # (the clips encoded by the gallery itself)
    _assert_topk(scores, idx, tg.similarity(video, vmask), 7)
    # save / load
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    fresh = FeatureGallery(model, products=3, dual_softmax=True)
    fresh.load_state_dict(torch.load(buf))
    assert len(fresh) == n and fresh.products == gal.products and _bits(fresh.rows, gal.rows)
    assert _bits(fresh._m[:n], gal._m[:n]) and _bits(fresh._s[:n], gal._s[:n]) and _bits(fresh._bank, gal._bank)
    a, b = fresh.search(ids, k=5), gal.search(ids, k=5)
    assert _bits(a[0], b[0]) and torch.equal(a[1], b[1]) and _bits(fresh.similarity(ids), D)
    plain = FeatureGallery(model)
    plain.add_features(feats, vmask)
    assert set(plain.state_dict()) == {"rows", "count", "E", "side", "products"}
    with pytest.raises(ValueError, match="dual_softmax"):
        plain.load_state_dict(gal.state_dict())
    with pytest.raises(ValueError, match="dual_softmax"):
        fresh.load_state_dict(plain.state_dict())
    assert len(fresh) == n and len(plain) == n and _bits(plain.similarity(ids), S)
    gal.clear()
    assert len(gal) == 0 and gal._bank is not None
    gal.add_features(feats[:3], vmask[:3])                                 # the bank was kept: the pairs come with the rows
    assert _bits(gal._s[:3], fresh._s[:3])
    # a camoe_dsl model is accepted with the keyword
    dsl_model = _eval_model(g2, cluster_inter, camoe_dsl=1)
    dg = FeatureGallery(dsl_model, dual_softmax=True)
    dg.set_query_bank(ids)
    dg.add(video, vmask)
    a = dg.search(ids, k=5)
    _assert_topk(a[0], a[1], dg.similarity(ids), 5)
