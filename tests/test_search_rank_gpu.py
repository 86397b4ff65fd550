"""Rank of a known row or group on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_rank, FeatureGallery.rank* on the
small model, and eval_epoch(matrix_free=True).

Every reference is existing code on the same rows, never the code under test: S = scaled_dot_planes on a zero-padded copy
(``_matrix``), for the dual softmax D = dsl_apply_ on S; then rank_counts_cols(S, target) for rows without a mask, and for
masks and groups ``rank_ref`` of tests/test_search_rank_host.py - the contract restated in NumPy on S (the matrix ops have no
notion of a target that is not selectable).  Counts integer-equal, score bit-equal to S[q, target].  E = 64 unless said;
galleries carry 37 non-zero rows behind n and masks carry ones above n in their last word, none of which may be counted."""
import io
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from test_search_gpu import DEV, MULT, N_CLIPS, _bits, _dataset, _eval_model, _matrix, _planes, g2  # noqa: F401  (g2: the fixture)
from test_search_grouped_gpu import LABELS, PATTERN, _heads
from test_search_masked_gpu import BEHIND, _case, _mask, _randn_planes
from test_search_rank_host import rank_ref

pytestmark = pytest.mark.gpu
op = torch.ops.centerclip


def _dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _assert_rank(got, M, target, sel=None, head=None):
    """(counts, score) of the op against the matrix M [Bq, n]: rank_ref always, rank_counts_cols too where it applies"""
    counts, score = got
    Mn = M.cpu().numpy() if torch.is_tensor(M) else M
    target = np.asarray(target)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (Mn.shape[0], 3)
    assert score.dtype == torch.float32 and tuple(score.shape) == (Mn.shape[0],)
    want_counts, want_score = rank_ref(Mn, target, sel, None if head is None else head[:Mn.shape[1]])
    assert np.array_equal(counts.cpu().numpy(), want_counts), "counts differ from the contract restated on the matrix"
    assert np.array_equal(score.cpu().numpy().view(np.uint32), want_score.view(np.uint32)), "score is not the matrix op's bits"
    if sel is None and head is None and torch.is_tensor(M) and ((target >= 0) & (target < Mn.shape[1])).all():
        cols = op.rank_counts_cols(M.contiguous(), _dev(target, torch.int32))
        assert torch.equal(counts, cols), "counts differ from rank_counts_cols on the matrix"
        assert _bits(score, M.gather(1, _dev(target).view(-1, 1)).squeeze(1))


def _target_sets(Bq, n, seed):
    """targets at 0, at n - 1, on both sides of a tile edge, and random: one vector each"""
    rng = np.random.default_rng(seed)
    fixed = sorted({0, n - 1, min(15, n - 1), min(16, n - 1), (n - 1) // 16 * 16, max((n - 1) // 16 * 16 - 1, 0)})
    return [np.full(Bq, v) for v in fixed] + [rng.integers(0, n, size=Bq), np.resize(np.array(fixed), Bq)]


# ------------------------------------------------------------------------------------------------ 1. shapes
NS, BQS, PRODUCTS = (1, 15, 16, 17, 255, 257, 1000, 4099), (1, 5, 16, 17, 33), (1, 2, 3)


def _sweep():
    """every n once; Bq and products dealt out in shuffled cycles so that every value of both shows"""
    rng = np.random.default_rng(20264)
    cols = [[axis[i] for i in np.resize(rng.permutation(len(axis)), len(NS))] for axis in (BQS, PRODUCTS)]
    cases = list(zip(NS, *cols))
    assert {c[1] for c in cases} == set(BQS) and {c[2] for c in cases} == set(PRODUCTS)
    return [tuple(int(v) for v in c) for c in cases]


@pytest.mark.parametrize("n,Bq,products", _sweep())
def test_shape_sweep_e64(n, Bq, products):
    if n == 4099:
        assert L.lib().cc_similarity_topk_slices(Bq, n, 1) >= 2              # the smallest n that gives several slices
    q, gal, S = _case(3 * n + Bq, Bq, n, products=products)
    for target in _target_sets(Bq, n, n + Bq):
        for dtype in (torch.int64, torch.int32):
            _assert_rank(op.similarity_rank(q, gal, n, MULT, products, _dev(target, dtype)), S, target)


def test_wide_rows():
    E, Bq, n, products = 512, 16, 3001, 2
    q, gal = _randn_planes(E + n, Bq, n + 5, E)
    S = _matrix(q, gal, n, MULT, products)
    for target in _target_sets(Bq, n, E)[-2:]:
        _assert_rank(op.similarity_rank(q, gal, n, MULT, products, _dev(target)), S, target)
    sel = (np.random.default_rng(E).random(n) < 0.5) & ((np.arange(n) // 16) % 5 != 2)
    _assert_rank(op.similarity_rank(q, gal, n, MULT, products, _dev(target), _mask(sel, n)), S, target, sel)
    q3, gal3 = _randn_planes(7, 3, 100, 1024)                                # the widest rows, three products: no exclusion
    S3 = _matrix(q3, gal3, 100, MULT, 3)
    _assert_rank(op.similarity_rank(q3, gal3, 100, MULT, 3, _dev([0, 50, 99])), S3, [0, 50, 99])


def test_targets_outside_the_gallery_count_nothing():
    Bq, n = 5, 257
    q, gal, S = _case(91, Bq, n)
    target = np.array([-1, n, 3, n + 20, -(2 ** 31)])
    counts, score = op.similarity_rank(q, gal, n, MULT, 2, _dev(target))
    _assert_rank((counts, score), S, target)
    assert counts[[0, 1, 3, 4]].eq(0).all() and bool(torch.isneginf(score[[0, 1, 3, 4]]).all()) and int(counts[2, 1]) >= 1
    hd = torch.from_numpy(_heads(PATTERN, n)).to(DEV)
    _assert_rank(op.similarity_rank(q, gal, n, MULT, 2, _dev(target), group_head=hd), S, target, head=_heads(PATTERN, n))


# ------------------------------------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_target_among_its_duplicates(which):
    n, Bq = 4099, 5
    q, gal = _randn_planes(21, Bq, n + BEHIND, 64)
    copies = [700, 2051, 4098]                                              # three slices of the eight
    gal[copies] = gal[copies[0]].clone()
    S = _matrix(q, gal, n, MULT, 2)
    target = np.full(Bq, copies[which])
    want = op.rank_counts_cols(S, _dev(target, torch.int32)).cpu().numpy()
    assert (want[:, 1] == 3).all() and (want[:, 2] == which).all()          # the ties are certain, on the reference
    got = op.similarity_rank(q, gal, n, MULT, 2, _dev(target))
    _assert_rank(got, S, target)
    assert got[0][:, 1].eq(3).all() and got[0][:, 2].eq(which).all()


def test_all_rows_identical():
    n, Bq = 4099, 5
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(Bq, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(n, 64), True)
    S = _matrix(q, gal, n, MULT, 2)
    target = np.array([0, 1, 2050, 4097, 4098])
    counts, score = op.similarity_rank(q, gal, n, MULT, 2, _dev(target))
    _assert_rank((counts, score), S, target)
    assert counts.cpu().tolist() == [[0, n, int(t)] for t in target]


# ------------------------------------------------------------------------------------------------ 3. NaN, rows mode
def test_nan_rows_count_as_rank_counts_cols_counts_them():
    Bq, n = 17, 1000
    q, gal = _randn_planes(33, Bq, n + BEHIND, 64)
    gal[300] = float("nan")
    q[4] = float("nan")
    S = _matrix(q, gal, n, MULT, 2)
    assert bool(torch.isnan(S[:, 300]).all()) and bool(torch.isnan(S[4]).all()) and int(torch.isnan(S).sum()) == Bq + n - 1
    for target in (np.full(Bq, 300), np.arange(Bq) * 50, np.full(Bq, 299)):
        counts, score = op.similarity_rank(q, gal, n, MULT, 2, _dev(target))
        want = op.rank_counts_cols(S, _dev(target, torch.int32))
        assert torch.equal(counts, want)
        truth = S.gather(1, _dev(target).view(-1, 1)).squeeze(1)
        assert torch.equal(torch.isnan(score), torch.isnan(truth)) and _bits(score[~torch.isnan(truth)], truth[~torch.isnan(truth)])
    assert op.similarity_rank(q, gal, n, MULT, 2, _dev(np.full(Bq, 300)))[0].eq(0).all()      # a NaN target: (0, 0, 0)


# ------------------------------------------------------------------------------------------------ 4. masks
def test_masks_against_the_contract():
    Bq, n = 17, 4099
    q, gal, S = _case(41, Bq, n)
    rng = np.random.default_rng(41)
    rows = np.arange(n)
    target = rng.integers(0, n, size=Bq)
    dead_tiles = ((rows // 16) % 7 != 3) & (rng.random(n) < 0.7)            # whole dead tiles, and half-live ones
    dead_tiles[(rows >= 1024) & (rows < 1536)] = False                      # one slice of the eight without a live tile
    per_query = rng.random((Bq, n)) < 0.5
    own_clear = np.ones(n, dtype=bool)
    own_clear[target] = False                                               # every target's own bit is clear
    own_clear_per_query = np.ones((Bq, n), dtype=bool)
    own_clear_per_query[np.arange(Bq), target] = False
    for sel in (dead_tiles, per_query, own_clear, own_clear_per_query, np.zeros(n, dtype=bool), np.zeros((Bq, n), dtype=bool),
                np.ones(n, dtype=bool)):
        got = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(sel, n))
        _assert_rank(got, S, target, sel)
        assert _bits(got[1], S.gather(1, _dev(target).view(-1, 1)).squeeze(1))       # the score never asks the mask
    assert got[0].equal(op.similarity_rank(q, gal, n, MULT, 2, _dev(target))[0])     # all ones: the unmasked counts
    none = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(np.zeros(n, dtype=bool), n))
    assert none[0].eq(0).all()
    clear = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(own_clear, n))
    assert bool((clear[0][:, 1] == 0).all())                                # not selectable: not even equal to itself


@pytest.mark.parametrize("n", [17, 257, 1000])
def test_masks_on_small_galleries(n):
    Bq = 5
    q, gal, S = _case(43 + n, Bq, n, products=3)
    rng = np.random.default_rng(n)
    target = rng.integers(0, n, size=Bq)
    for sel in (rng.random(n) < 0.5, rng.random((Bq, n)) < 0.3, (np.arange(n) // 16) % 2 == 0):
        _assert_rank(op.similarity_rank(q, gal, n, MULT, 3, _dev(target), _mask(sel, n)), S, target, sel)


# ------------------------------------------------------------------------------------------------ 5. groups
@pytest.mark.parametrize("n", [17, 4099])
def test_singleton_groups_are_rows_mode_bit_for_bit(n):
    Bq = 17
    q, gal, S = _case(5 * n, Bq, n)
    hd = torch.arange(n + BEHIND, device=DEV, dtype=torch.int32)
    sel = np.random.default_rng(n).random(n) < 0.4
    for target in _target_sets(Bq, n, n)[-2:]:
        a = op.similarity_rank(q, gal, n, MULT, 2, _dev(target))
        b = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), group_head=hd)
        assert torch.equal(a[0], b[0]) and _bits(a[1], b[1])
        _assert_rank(b, S, target)
        sel_t = sel.copy()
        sel_t[target] = True                                                # (a dead singleton target scores -inf: not rows mode)
        a = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(sel_t, n))
        b = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(sel_t, n), group_head=hd)
        assert torch.equal(a[0], b[0]) and _bits(a[1], b[1])


def _long_group_heads(n):
    """singleton groups up to row 600, one group of 1000 rows (a wave's share of 4099 rows in 8 slices is 128), the pattern"""
    return np.concatenate([np.arange(600), np.full(1000, 600), 1600 + _heads(PATTERN, n - 1600)]).astype(np.int32)


@pytest.mark.parametrize("heads", ["pattern", "long group", "single group"])
def test_groups_against_the_contract(heads):
    Bq, n, products = 17, 4099, 3
    q, gal, S = _case(n + 1, Bq, n, products=products)
    head = {"pattern": _heads(PATTERN, n), "long group": _long_group_heads(n),
            "single group": np.concatenate([np.zeros(n), np.arange(n, n + BEHIND)]).astype(np.int32)}[heads]
    hd = torch.from_numpy(head).to(DEV)
    rng = np.random.default_rng(len(heads))
    rows = np.arange(n)
    targets = [rng.integers(0, n, size=Bq), np.resize(np.array([0, n - 1, 600, 1599, 1600, 615, 616, 2047, 2048]), Bq)]
    for target in targets:
        _assert_rank(op.similarity_rank(q, gal, n, MULT, products, _dev(target), group_head=hd), S, target, head=head)
    target = targets[0]
    starts = np.unique(head[:n])
    dead_starts = ~np.isin(rows // 16, starts // 16) | (rng.random(n) < 0.2)          # the tiles that hold group starts: mostly dead
    dead_tiles = ((rows // 16) % 3 != 1)
    target_dead = np.ones(n, dtype=bool)
    for t in target[:5]:
        target_dead[head[:n] == head[t]] = False                            # five target groups without a selectable row
    per_query = rng.random((Bq, n)) < 0.3
    for sel in (dead_starts, dead_tiles, target_dead, target_dead & dead_tiles, per_query, np.zeros(n, dtype=bool)):
        got = op.similarity_rank(q, gal, n, MULT, products, _dev(target), _mask(sel, n), group_head=hd)
        _assert_rank(got, S, target, sel, head)
    dead = op.similarity_rank(q, gal, n, MULT, products, _dev(target), _mask(target_dead, n), group_head=hd)
    assert bool(torch.isneginf(dead[1][:5]).all()) and bool((dead[0][:5, 1:] == 0).all())
    if heads != "single group":
        assert bool((dead[0][:5, 0] > 0).all())                             # -inf: every group with a selectable row is greater


@pytest.mark.parametrize("n", [17, 257])
def test_groups_on_small_galleries(n):
    Bq = 5
    q, gal, S = _case(47 + n, Bq, n)
    head = _heads(PATTERN, n)
    hd = torch.from_numpy(head).to(DEV)
    rng = np.random.default_rng(n)
    for target in _target_sets(Bq, n, n)[-2:]:
        _assert_rank(op.similarity_rank(q, gal, n, MULT, 2, _dev(target), group_head=hd), S, target, head=head)
        for sel in (rng.random(n) < 0.5, rng.random((Bq, n)) < 0.5):
            _assert_rank(op.similarity_rank(q, gal, n, MULT, 2, _dev(target), _mask(sel, n), group_head=hd), S, target, sel, head)


# ------------------------------------------------------------------------------------------------ 6. dual softmax
@pytest.mark.parametrize("Bq,n", [(33, 1000), (5, 4099)])
@pytest.mark.parametrize("side", [0, 1])
def test_dual_softmax(Bq, n, side):
    """side 1: text queries, a clip gallery, statistics per gallery row; side 0: clip queries, a caption gallery, statistics
    per query row - from dsl_col_stats_planes, D from dsl_apply_ on S as tests/test_search_masked_gpu.py does"""
    q, gal = _randn_planes(100 * Bq + n + side, Bq, n + BEHIND, text_queries=bool(side))
    head, products = _heads(PATTERN, n), 2
    hd = torch.from_numpy(head).to(DEV)
    if side:
        S_tv = _matrix(q, gal, n, MULT, products)
        m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, products)
        nt = Bq
    else:
        S_tv = _matrix(gal[:n].contiguous(), q, Bq, MULT, products)
        m, s = op.dsl_col_stats_planes(gal, q, n, Bq, MULT, products)
        nt = n
    D = S_tv.clone()
    op.dsl_apply_(D, m, s, nt)
    D_qg = D if side else D.t().contiguous()
    if side:                                                               # statistics behind n: never read
        m, s = (torch.cat([t, torch.full((BEHIND,), float("nan"), device=DEV)]) for t in (m, s))
    rng = np.random.default_rng(Bq + n + side)
    for target in (rng.integers(0, n, size=Bq), np.resize(np.array([0, n - 1, 15, 16]), Bq)):
        tg = _dev(target)
        _assert_rank(op.similarity_rank(q, gal, n, MULT, products, tg, None, m, s, side, nt), D_qg, target)
        _assert_rank(op.similarity_rank(q, gal, n, MULT, products, tg, None, m, s, side, nt, hd), D_qg, target, head=head)
        for sel in (rng.random(n) < 0.5, (np.arange(n) >= 37) & (np.arange(n) < 137), rng.random((Bq, n)) < 0.5):
            _assert_rank(op.similarity_rank(q, gal, n, MULT, products, tg, _mask(sel, n), m, s, side, nt), D_qg, target, sel)
            _assert_rank(op.similarity_rank(q, gal, n, MULT, products, tg, _mask(sel, n), m, s, side, nt, hd), D_qg, target, sel, head)


# ------------------------------------------------------------------------------------------------ 7. against the search
@pytest.mark.parametrize("mode", ["rows", "masked", "grouped", "dual softmax"])
def test_the_rank_is_the_place_in_the_search(mode):
    """for every query with rank < k: search's ids[q, rank] == target[q], the score bits agree.  Half the targets are taken
    from search's own result at seeded ranks, so at least half the queries are checked - asserted before it is relied on"""
    Bq, n, k = 32, 4099, 64
    q, gal, _ = _case(53, Bq, n)
    rng = np.random.default_rng(53)
    kw, head = {}, None
    mask = _mask(rng.random(n) < 0.5, n) if mode == "masked" else None
    if mode == "grouped":
        head = _heads(PATTERN, n)
        kw = dict(group_head=torch.from_numpy(head).to(DEV))
    if mode == "dual softmax":
        m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, 2)
        kw = dict(m=m, s=s, stats_on_gallery=1, n_total=Bq)
    ones = _mask(np.ones(n, dtype=bool), n)
    scores, ids = op.similarity_topk_masked(q, gal, n, MULT, 2, k, ones if mask is None else mask, **kw)
    assert bool((ids >= 0).all())
    at = rng.integers(0, k, size=Bq)
    target = rng.integers(0, n, size=Bq)
    target[::2] = ids.cpu().numpy()[np.arange(Bq), at][::2]
    counts, score = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), mask, **kw)
    rank = (counts[:, 0] + counts[:, 2]).cpu().numpy()
    assert (rank[::2] == at[::2]).all()
    inside = np.flatnonzero(rank < k)
    assert len(inside) >= Bq // 2
    got_ids = ids.cpu().numpy()[inside, rank[inside]]
    if head is None:
        assert (got_ids == target[inside]).all()
    else:
        assert (head[got_ids] == head[target[inside]]).all()                # the best row of the target's group
    sel_score = score.cpu().numpy()[inside].view(np.uint32)
    if mode == "masked":                                                    # an unselectable target is not in the search
        live = (mask.cpu().numpy().view(np.uint32)[target[inside] >> 5] >> (target[inside] & 31).astype(np.uint32)) & 1
        assert live[np.isin(inside, np.arange(0, Bq, 2))].all()
        inside, got_ids, sel_score = inside[live == 1], got_ids[live == 1], sel_score[live == 1]
        assert len(inside) >= Bq // 2 and (got_ids == target[inside]).all()
    assert np.array_equal(scores.cpu().numpy()[inside, rank[inside]].view(np.uint32), sel_score)


# ------------------------------------------------------------------------------------------------ 8. capture
def test_graph_capture_and_replay_with_changing_targets():
    Bq, n = 5, 4099
    q, gal, S = _case(15, Bq, n)
    rng = np.random.default_rng(15)
    sel = rng.random(n) < 0.5
    mask = _mask(sel, n)
    tbuf = _dev(np.zeros(Bq, dtype=np.int64), torch.int32)
    op.similarity_rank(q, gal, n, MULT, 2, tbuf, mask)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        counts, score = op.similarity_rank(q, gal, n, MULT, 2, tbuf, mask)
    for target in (rng.integers(0, n, size=Bq), np.array([0, n - 1, n, -1, 2048]), np.zeros(Bq, dtype=np.int64)):
        tbuf.copy_(_dev(target, torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        _assert_rank((counts, score), S, target, sel)


# ------------------------------------------------------------------------------------------------ 9. FeatureGallery
GONE = (0, 3, 5, 6)


@pytest.mark.parametrize("side", ["video", "text"])
@pytest.mark.parametrize("grouped", [False, True])
def test_feature_gallery_rank(g2, side, grouped):
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, 0)
    video, vmask, ids = _dataset(g2["s1_cfg"])
    n = N_CLIPS
    items = (lambda sl: (video[sl], vmask[sl])) if side == "video" else (lambda sl: (ids[sl],))
    query = (ids,) if side == "video" else (video, vmask)
    gal = FeatureGallery(model, capacity=4, side=side, grouped=grouped)
    for i in range(n):
        gal.add(*items(slice(i, i + 1)), **(dict(group=[LABELS[i]]) if grouped else {}))
    head = np.unique(np.asarray(LABELS), return_index=True)[1][np.unique(np.asarray(LABELS), return_inverse=True)[1]]
    M = gal.similarity(*query)
    rng = np.random.default_rng(12)
    targets = [np.arange(n), rng.integers(0, n, size=n), np.full(n, 7)]

    def check(g, M_scores, live, allow=None, sel=None):
        """rank / rank_features (and rank_groups) of `g` against the matrix, and against g's own search"""
        sel = live if sel is None else sel
        checked = 0
        for target in targets:
            for tg in (target.tolist(), torch.from_numpy(target), _dev(target), _dev(target, torch.int32)):
                ranks, scores, counts = g.rank(*query, target=tg, allow=allow)
                _assert_rank((counts, scores), M_scores, target, sel)
                assert ranks.dtype == torch.int64 and torch.equal(ranks, counts[:, 0].long() + counts[:, 2])
            found, pos = g.search(*query, k=n, allow=allow)
            at = ranks.cpu().numpy()
            ok = sel[target] if sel.ndim == 1 else sel[np.arange(n), target]
            checked += int(ok.sum())                                         # (a target that is not selectable is not in the search)
            assert (pos.cpu().numpy()[np.flatnonzero(ok), at[ok]] == target[ok]).all()
            assert _bits(found[torch.from_numpy(np.flatnonzero(ok)).to(DEV), _dev(at[ok])], scores[_dev(ok, torch.bool)])
            if grouped:
                labels = np.asarray(LABELS)[target]
                ranks, scores, counts = g.rank_groups(*query, target=labels.tolist(), allow=allow)
                _assert_rank((counts, scores), M_scores, target, sel, head)
                _, found_labels, _ = g.search_groups(*query, k=n, allow=allow)
                at = ranks.cpu().numpy()
                alive = np.isfinite(scores.cpu().numpy())
                assert alive.any() and (found_labels.cpu().numpy()[np.flatnonzero(alive), at[alive]] == labels[alive]).all()
                again = g.rank_groups(*query, target=torch.from_numpy(labels), allow=allow)
                assert torch.equal(again[0], ranks) and _bits(again[1], scores)
        assert checked >= n // 2
    live = np.ones(n, dtype=bool)
    check(gal, M, live)
    feats = model(input_ids=ids)['sequence_output'] if side == "video" else model(video=video, video_mask=vmask)['visual_output']
    a = gal.rank_features(feats, targets[1].tolist(), mask=None if side == "video" else vmask)
    b = gal.rank(*query, target=targets[1].tolist())
    assert all(_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="outside"):
        gal.rank(*query, target=[0] * (n - 1) + [n])
    with pytest.raises(ValueError, match="per query"):
        gal.rank(*query, target=[0] * (n - 1))
    # after remove: a removed target keeps its score and is not counted
    gal.remove(list(GONE))
    live[list(GONE)] = False
    check(gal, M, live)
    # allow= from row_mask, and one mask per query
    pick = [1, 2, 5, 7, 8, 11]
    allowed = np.isin(np.arange(n), pick) & live
    check(gal, M, live, allow=gal.row_mask(positions=pick), sel=allowed)
    per_query = torch.ones(n, n, dtype=torch.bool, device=DEV)
    per_query[torch.arange(n), torch.arange(n)] = False
    check(gal, M, live, allow=per_query, sel=per_query.cpu().numpy() & live[None, :])
    # save / load
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    loaded = FeatureGallery(model, side=side, grouped=grouped)
    loaded.load_state_dict(torch.load(buf))
    a, b = loaded.rank(*query, target=targets[1].tolist()), gal.rank(*query, target=targets[1].tolist())
    assert torch.equal(a[0], b[0]) and _bits(a[1], b[1]) and torch.equal(a[2], b[2])
    # after compact(): the gallery of the survivors, its own matrix
    keep = np.flatnonzero(live)
    gal.compact()
    Mc = gal.similarity(*query)
    assert _bits(Mc, M[:, torch.from_numpy(keep).to(DEV)].contiguous())
    target = rng.integers(0, len(keep), size=n)
    ranks, scores, counts = gal.rank(*query, target=target.tolist())
    _assert_rank((counts, scores), Mc, target)
    if grouped:
        kept_labels = np.asarray(LABELS)[keep]
        kept_head = np.unique(kept_labels, return_index=True)[1][np.unique(kept_labels, return_inverse=True)[1]]
        ranks, scores, counts = gal.rank_groups(*query, target=kept_labels[target].tolist())
        _assert_rank((counts, scores), Mc, target, None, kept_head)
        with pytest.raises(ValueError, match="label"):
            gal.rank_groups(*query, target=[LABELS[3]] * n)                  # the group that was removed whole
    empty = FeatureGallery(model, side=side)
    with pytest.raises(ValueError, match="outside"):
        empty.rank(*query, target=[0] * n)
    ranks, scores, counts = empty.rank(*query, target=_dev(np.zeros(n, dtype=np.int64)))      # a device target: not looked at
    assert counts.eq(0).all() and ranks.eq(0).all() and bool(torch.isneginf(scores).all())


# ------------------------------------------------------------------------------------------------ 10. eval_epoch
@pytest.mark.parametrize("dsl", [False, True])
@pytest.mark.parametrize("name,sentences,seed", [("single", [1] * 6, 328), ("multi", [3, 1, 4, 2, 3], 345)])
def test_eval_epoch_matrix_free_equals_the_matrix_path(monkeypatch, name, sentences, seed, dsl):
    """the planted features of tests/test_dsl_gpu.py (no two entries close): R@1, both metric dicts and the strings are the
    matrix path's, and the matrix op is never called"""
    from centerclip_amd import eval as ev
    from test_dsl_gpu import _Loader, _planted, _PlantedModel
    text, batches, attrs, _ = _planted(sentences, seed)
    model = _PlantedModel(text)
    loader = _Loader(batches)
    loader.dataset = Namespace(**attrs)
    seen = {}
    inner_sharded, inner_free = ev._sharded_metrics, ev.matrix_free_metrics

    def sharded(*a, **kw):
        seen["matrix"] = inner_sharded(*a, **kw)
        return seen["matrix"]

    def free(*a, **kw):
        seen["free"] = inner_free(*a, **kw)
        return seen["free"]
    monkeypatch.setattr(ev, "_sharded_metrics", sharded)
    monkeypatch.setattr(ev, "matrix_free_metrics", free)

    class NoMatrix(ev.HipBackend):
        @classmethod
        def dot_operands(cls, *a, **kw):
            raise AssertionError("matrix_free=True formed the matrix")
    args = Namespace(inference_speed_test=False)
    want = ev.eval_epoch(model, loader, torch.device(DEV), args=args, in_flight=1, camoe_dsl=dsl)
    got = ev.eval_epoch(model, loader, torch.device(DEV), args=args, in_flight=1, camoe_dsl=dsl, backend=NoMatrix, matrix_free=True)
    assert got[0] == want[0] and list(got[2]) == list(want[2])
    for a, b in zip(seen["free"], seen["matrix"][:2]):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with pytest.raises(AssertionError, match="formed the matrix"):          # (the guard itself: the default path does call it)
        ev.eval_epoch(model, loader, torch.device(DEV), args=args, in_flight=1, camoe_dsl=dsl, backend=NoMatrix)
