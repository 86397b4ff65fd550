"""Deep lists and cursors on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_topk_deep and FeatureGallery's
``k`` up to 4096 / ``after=``.

Every assertion is exact and runs over every row of every case.  The reference is the existing matrix op on the same rows
    S = scaled_dot_planes(query planes, gallery copy padded to padded_video_rows(n) with zero rows, n, mult, products)
(followed by ``dsl_apply_`` for the dual softmax), then per query row ``np.argsort(-S, kind="stable")`` over the selectable
columns (groups: of that order the first row of every group), then - with a cursor (score, id) - the entries strictly behind
it in that order (a smaller score, or an equal score and a larger id), the first k of them, and the fill (-inf, -1): ids
equal, scores bit-equal.  E = 64 unless a test says otherwise; the shapes are the smallest at which paging can go wrong:
lists that end inside page 1, exactly at a page edge and inside a later page, ties that straddle page edges, groups whose
second-best row beats other groups' best."""
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
MULT = math.exp(4.6052)
op = torch.ops.centerclip
BEHIND = 37                                                                # non-zero rows behind n: they must not appear


# ------------------------------------------------------------------------------------------------ helpers (tests/test_search_gpu.py's)
def _planes(rows, video_side):
    return op.normalize_rows_planes(rows.to(DEV).float().contiguous(), video_side)


def _randn_planes(seed, Bq, rows, E):
    g = torch.Generator().manual_seed(seed)
    return _planes(torch.randn(Bq, E, generator=g), False), _planes(torch.randn(rows, E, generator=g), True)


def _matrix(q, gal, n, mult, products):
    pad = torch.zeros(max(n, T.padded_video_rows(n)), gal.shape[1], device=DEV, dtype=torch.float16)
    pad[:n] = gal[:n]
    return op.scaled_dot_planes(q, pad, n, mult, products)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                    b.view(torch.int32) if b.dtype == torch.float32 else b)


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mask(sel, n):
    """bool [n] or [Bq, n] -> the ops' mask words on the device (bit b of word w = row 32 w + b)"""
    sel = np.asarray(sel, dtype=bool)
    words = -(-n // 32)
    padded = np.zeros(sel.shape[:-1] + (32 * words,), dtype=bool)
    padded[..., :n] = sel[..., :n]
    return _dev(np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<i4").astype(np.int32))


# ------------------------------------------------------------------------------------------------ the reference
def deep_ref(S, k, sel=None, head=None, after=None):
    """S [Bq, n] scores; sel bool [n] or [Bq, n] (None: all); head [n] group labels (None: rows); after (scores [Bq], ids [Bq])
    -> (scores [Bq, k] of S's dtype, ids [Bq, k] int64)"""
    S = _np(S)
    Bq, n = S.shape
    sel = np.ones((Bq, n), dtype=bool) if sel is None else np.broadcast_to(np.asarray(sel, dtype=bool)[..., :n], (Bq, n))
    scores = np.full((Bq, k), -np.inf, dtype=S.dtype)
    ids = np.full((Bq, k), -1, dtype=np.int64)
    for q in range(Bq):
        cols = np.flatnonzero(sel[q])
        order = cols[np.argsort(-S[q, cols], kind="stable")]
        if head is not None:
            _, first = np.unique(np.asarray(head)[order], return_index=True)
            order = order[np.sort(first)]
        if after is not None:
            a_s, a_i = float(_np(after[0])[q]), int(_np(after[1])[q])
            x = S[q, order]
            order = order[(x < a_s) | ((x == a_s) & (order > a_i))] if a_i >= 0 else order[:0]
        order = order[:k]
        ids[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order]
    return scores, ids


def test_the_reference_on_a_hand_written_example():
    S = np.array([[1, 5, 5, 2, 5, 3, 0, -0.0, 4]], dtype=np.float32)
    assert deep_ref(S, 9)[1].tolist() == [[1, 2, 4, 8, 5, 3, 0, 6, 7]]
    assert deep_ref(S, 3, after=([5.0], [2]))[1].tolist() == [[4, 8, 5]]                   # inside a run of equal scores
    assert deep_ref(S, 3, after=([0.0], [6]))[1].tolist() == [[7, -1, -1]]                 # -0 == +0: the larger id follows
    assert deep_ref(S, 2, after=([-np.inf], [-1]))[1].tolist() == [[-1, -1]]               # behind the fill: the fill
    assert deep_ref(S, 3, after=([5.0], [2]), sel=np.arange(9) != 4)[1].tolist() == [[8, 5, 3]]
    head = np.array([0, 0, 0, 3, 4, 4, 6, 6, 6])
    assert deep_ref(S, 5, head=head)[1].tolist() == [[1, 4, 8, 3, -1]]
    assert deep_ref(S, 5, head=head, after=([5.0], [1]))[1].tolist() == [[4, 8, 3, -1, -1]]  # row 2 of group 0 does not return


def _assert_list(got, want):
    (scores, ids), (want_scores, want_ids) = got, want
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and tuple(ids.shape) == tuple(scores.shape) == want_ids.shape
    got_ids, got_scores = ids.cpu().numpy(), scores.cpu().numpy()
    assert np.array_equal(got_ids, want_ids), "ids differ from the reference ordering (first difference at %s)" % (
        np.argwhere(got_ids != want_ids)[0].tolist(),)
    assert np.array_equal(got_scores.view(np.uint32), want_scores.view(np.uint32)), "scores are not the matrix op's bits"


def _deep(q, gal, n, products, k, mask=None, head=None, after=None, stats=None, mult=MULT):
    m, s, side, nt = stats if stats is not None else (None, None, 1, 0)
    a = after if after is not None else (None, None)
    return op.similarity_topk_deep(q, gal, n, mult, products, k, mask, m, s, side, nt, None if head is None else _dev(head),
                                   a[0], a[1])


def _last(result):
    return result[0][:, -1].contiguous(), result[1][:, -1].contiguous()


# ------------------------------------------------------------------------------------------------ 1. shapes
BQS, NS, KS, PRODUCTS = (1, 5, 17, 33), (1, 15, 128, 129, 256, 257, 1000, 4099), (129, 130, 256, 257, 300, 1000, 4096), (1, 2, 3)


def _sweep():
    """A seeded subset of the product: every axis is dealt out in a shuffled cycle, so 12 cases show every value of every
    axis; five more make sure the fill begins inside page 1, exactly at a page edge (n = 128, 256) and inside a later page."""
    rng = np.random.default_rng(20261)
    cols = [[axis[i] for i in np.resize(rng.permutation(len(axis)), 12)] for axis in (BQS, NS, KS, PRODUCTS)]
    cases = list(zip(*cols)) + [(17, 15, 130, 2), (5, 128, 300, 1), (33, 256, 257, 3), (1, 257, 300, 2), (5, 1000, 4096, 1)]
    for axis, col in zip((BQS, NS, KS, PRODUCTS), zip(*cases)):
        assert set(axis) == set(col)
    assert any(n < 128 < k for _, n, k, _ in cases) and any(n == 128 < k for _, n, k, _ in cases)
    assert any(n == 256 < k for _, n, k, _ in cases) and any(128 < n < k and n % 128 for _, n, k, _ in cases)
    return [tuple(int(v) for v in c) for c in cases]


@pytest.mark.parametrize("Bq,n,k,products", _sweep())
def test_shape_sweep_e64(Bq, n, k, products):
    q, gal = _randn_planes(1000 * Bq + n + k, Bq, n + BEHIND, 64)
    _assert_list(_deep(q, gal, n, products, k), deep_ref(_matrix(q, gal, n, MULT, products), k))


# ------------------------------------------------------------------------------------------------ 2. the first page
def test_the_first_128_columns_are_the_plain_ops():
    q, gal = _randn_planes(21, 17, 4099 + BEHIND, 64)
    for products in (1, 2, 3):
        deep, plain = _deep(q, gal, 4099, products, 300), op.similarity_topk(q, gal, 4099, MULT, products, 128)
        assert torch.equal(deep[1][:, :128], plain[1]) and _bits(deep[0][:, :128].contiguous(), plain[0])


def _mode_case(n):
    """-> (head int32 [n + BEHIND], one mask bool [n], per-query masks bool [5, n]) with a group boundary inside a tile and
    one group that has an all-dead tile between two live ones under the one mask"""
    if n == 40:
        sizes, dead = (3, 34, 3), (16, 32)                                 # the middle group: tiles 0 and 2 live, tile 1 dead
    else:
        sizes, dead = (7,) * 85 + (1000,) + (5,) * 500 + (4,), (640, 704)  # the group of 1000 rows [595, 1595): tiles 40..43 dead
    assert sum(sizes) == n
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    head = np.concatenate([np.repeat(starts, sizes), np.arange(n, n + BEHIND)]).astype(np.int32)
    rng = np.random.default_rng(n)
    one = rng.random(n) < 0.75
    one[dead[0]:dead[1]] = False
    one[[dead[0] - 2, dead[1] + 2]] = True
    assert (starts % 16 != 0).any() and dead[0] % 16 == 0 and dead[1] % 16 == 0
    assert head[dead[0] - 2] == head[dead[1] + 2]                           # one group on both sides of the dead tiles
    return head, one, rng.random((5, n)) < 0.5


@pytest.mark.parametrize("n", [4099, 40])
def test_without_a_cursor_the_deep_op_is_the_specialised_op_of_every_mode(n):
    """k <= 128: one page, the launches of the specialised op - scores as int32 bits, ids equal.  n = 4099: 8 slices and a
    ragged last tile; n = 40: one slice and the fill beyond 40.  Bq = 5: a partial group of 16 query rows."""
    Bq, products = 5, 2
    assert L.lib().cc_similarity_topk_slices(Bq, n, 128) == (8 if n == 4099 else 1)
    g = torch.Generator().manual_seed(150 + n)
    rows_q, rows_g = torch.randn(Bq, 64, generator=g), torch.randn(n + BEHIND, 64, generator=g)
    q, gal = _planes(rows_q, False), _planes(rows_g, True)                 # text queries, a clip gallery
    q0, gal0 = _planes(rows_q, True), _planes(rows_g, False)               # clip queries, a caption gallery
    on_gallery = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, products) + (1, Bq)
    on_query = op.dsl_col_stats_planes(gal0, q0, n, Bq, MULT, products) + (0, n)
    head, one, per_query = _mode_case(n)
    hd, one_w, per_query_w = _dev(head), _mask(one, n), _mask(per_query, n)
    for k in (17, 128):
        pairs = {
            "plain": (_deep(q, gal, n, products, k), op.similarity_topk(q, gal, n, MULT, products, k)),
            "dual softmax, gallery side": (_deep(q, gal, n, products, k, stats=on_gallery),
                                           op.similarity_topk_dsl(q, gal, n, MULT, products, k, *on_gallery)),
            "dual softmax, query side": (_deep(q0, gal0, n, products, k, stats=on_query),
                                         op.similarity_topk_dsl(q0, gal0, n, MULT, products, k, *on_query)),
            "grouped": (_deep(q, gal, n, products, k, head=head), op.similarity_topk_grouped(q, gal, n, MULT, products, k, hd)),
            "grouped + dual softmax": (_deep(q, gal, n, products, k, head=head, stats=on_gallery),
                                       op.similarity_topk_grouped_dsl(q, gal, n, MULT, products, k, *on_gallery, hd)),
            "one mask": (_deep(q, gal, n, products, k, mask=one_w), op.similarity_topk_masked(q, gal, n, MULT, products, k, one_w)),
            "per-query masks": (_deep(q, gal, n, products, k, mask=per_query_w),
                                op.similarity_topk_masked(q, gal, n, MULT, products, k, per_query_w)),
            "masked + grouped": (_deep(q, gal, n, products, k, mask=one_w, head=head),
                                 op.similarity_topk_masked(q, gal, n, MULT, products, k, one_w, group_head=hd)),
        }
        for mode, (deep, special) in pairs.items():
            assert bool((special[1][:, 0] >= 0).all()), mode                   # (a list, not the fill)
            assert torch.equal(deep[1], special[1]) and _bits(deep[0], special[0]), (mode, k)
        if n == 40 and k == 128:                                               # the fill begins behind the 40 rows
            ids = pairs["plain"][1][1]
            assert bool((ids[:, :40] >= 0).all()) and bool((ids[:, 40:] == -1).all())


# ------------------------------------------------------------------------------------------------ 3. ties across page edges
def test_identical_gallery_rows_come_in_id_order():
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(5, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(4099, 64), True)
    scores, ids = _deep(q, gal, 4099, 2, 1000)
    assert torch.equal(ids.cpu(), torch.arange(1000).expand(5, 1000))
    _assert_list((scores, ids), deep_ref(_matrix(q, gal, 4099, MULT, 2), 1000))


def _seven_rows(n=4099, Bq=17):
    g = torch.Generator().manual_seed(13)
    base = torch.randn(7, 64, generator=g)
    pick = torch.from_numpy(np.random.default_rng(13).integers(0, 7, size=n))
    return _planes(torch.randn(Bq, 64, generator=g), False), _planes(base[pick], True)


def test_seven_distinct_rows_repeated():
    q, gal = _seven_rows()
    for products in (1, 2, 3):
        S = _matrix(q, gal, 4099, MULT, products)
        assert len(np.unique(S[0].cpu().numpy())) <= 7                     # runs of ~585 equal scores: every page edge is inside one
        _assert_list(_deep(q, gal, 4099, products, 700), deep_ref(S, 700))


# ------------------------------------------------------------------------------------------------ 4. cursors
def test_three_calls_with_a_cursor_are_the_columns_of_one():
    n = 1000
    q, gal = _randn_planes(41, 5, n + BEHIND, 64)
    S = _matrix(q, gal, n, MULT, 2)
    want = deep_ref(S, 300)
    whole = _deep(q, gal, n, 2, 300)
    _assert_list(whole, want)
    part, after = [], None
    for _ in range(3):
        got = _deep(q, gal, n, 2, 100, after=after)
        _assert_list(got, deep_ref(S, 100, after=after))
        part.append(got)
        after = _last(got)
    assert torch.equal(torch.cat([p[1] for p in part], 1), whole[1]) and _bits(torch.cat([p[0] for p in part], 1), whole[0])
    # int32 positions, and a cursor that is no row's pair (a score between two rows'): the entries behind that place
    got = _deep(q, gal, n, 2, 150, after=(after[0], after[1].int()))
    _assert_list(got, deep_ref(S, 150, after=after))
    between = (whole[0][:, 10] + whole[0][:, 11]) / 2, torch.zeros(5, dtype=torch.int64, device=DEV)
    _assert_list(_deep(q, gal, n, 2, 200, after=between), deep_ref(S, 200, after=between))


def test_a_cursor_inside_a_run_of_equal_scores():
    q, gal = _seven_rows()
    S = _matrix(q, gal, 4099, MULT, 2)
    first = _deep(q, gal, 4099, 2, 50)
    after = _last(first)
    nxt = _deep(q, gal, 4099, 2, 250, after=after)
    assert torch.equal(S.gather(1, nxt[1][:, :1]).view(torch.int32), after[0][:, None].view(torch.int32))    # the run goes on
    _assert_list(nxt, deep_ref(S, 250, after=after))
    whole = deep_ref(S, 300)
    assert np.array_equal(np.concatenate([first[1].cpu().numpy(), nxt[1].cpu().numpy()], 1), whole[1])


def test_a_cursor_equal_to_the_fill_gives_the_fill():
    n = 15
    q, gal = _randn_planes(43, 5, n + BEHIND, 64)
    first = _deep(q, gal, n, 2, 20)                                        # 15 rows: the last column is the fill
    assert bool((first[1][:, -1] == -1).all())
    for k in (7, 300):
        scores, ids = _deep(q, gal, n, 2, k, after=_last(first))
        assert bool((ids == -1).all()) and bool(torch.isneginf(scores).all())
    # one query behind the fill, the others behind a row
    S = _matrix(q, gal, n, MULT, 2)
    after = (first[0][:, 3].clone(), first[1][:, 3].clone())
    after[0][2], after[1][2] = float("-inf"), -1
    _assert_list(_deep(q, gal, n, 2, 130, after=after), deep_ref(S, 130, after=after))


def test_per_query_masks_one_query_runs_dry_before_the_other():
    n, k = 4099, 100
    q, gal = _randn_planes(44, 3, n + BEHIND, 64)
    S = _matrix(q, gal, n, MULT, 2)
    rng = np.random.default_rng(44)
    sel = np.zeros((3, n), dtype=bool)
    sel[0, rng.choice(n, 5, replace=False)] = True
    sel[1, rng.choice(n, 300, replace=False)] = True
    sel[2] = rng.random(n) < 0.5
    mask = _mask(sel, n)
    whole = _deep(q, gal, n, 2, 3 * k, mask=mask)                          # inside one call: query 0's later pages are bounded by 0
    _assert_list(whole, deep_ref(S, 3 * k, sel=sel))
    after, part = None, []
    for page in range(3):
        got = _deep(q, gal, n, 2, k, mask=mask, after=after)
        _assert_list(got, deep_ref(S, k, sel=sel, after=after))
        part.append(got)
        after = _last(got)
        if page:
            assert bool((got[1][0] == -1).all()) and bool((got[1][1] >= 0).all())
    assert torch.equal(torch.cat([p[1] for p in part], 1), whole[1]) and bool((whole[1][1] >= 0).all())
    assert int((whole[1][0] >= 0).sum()) == 5


def test_a_cursor_whose_row_was_removed_continues_behind_its_place():
    n = 1000
    q, gal = _randn_planes(45, 5, n + BEHIND, 64)
    S = _matrix(q, gal, n, MULT, 3)
    first = _deep(q, gal, n, 3, 150)
    after = _last(first)
    sel = np.ones(n, dtype=bool)
    sel[after[1].cpu().numpy()] = False                                    # every query's cursor row leaves, and some others
    sel[first[1][:, 10].cpu().numpy()] = False
    sel[deep_ref(S, 200)[1][:, 170]] = False
    want = deep_ref(S, 200, sel=sel, after=after)
    _assert_list(_deep(q, gal, n, 3, 200, mask=_mask(sel, n), after=after), want)
    assert not sel[after[1].cpu().numpy()].any() and (want[1] >= 0).all()


# ------------------------------------------------------------------------------------------------ 5. masks
def test_masked_lists():
    n, k = 4099, 300
    q, gal = _randn_planes(51, 5, n + BEHIND, 64)
    S = _matrix(q, gal, n, MULT, 2)
    rng = np.random.default_rng(51)
    tiles = np.repeat((np.arange(-(-n // 16)) % 5) == 2, 16)[:n]           # whole 16-row tiles empty: four of every five
    for sel in (rng.random(n) < 0.5, tiles, tiles & (rng.random(n) < 0.7), rng.random((5, n)) < 0.3,
                np.arange(n) < 200, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)):
        _assert_list(_deep(q, gal, n, 2, k, mask=_mask(sel, n)), deep_ref(S, k, sel=sel))
    assert int(tiles.sum()) > k and not tiles[:32].any()


# ------------------------------------------------------------------------------------------------ 6. dual softmax
@pytest.mark.parametrize("side", [1, 0])
def test_dual_softmax_lists(side):
    """side 1: text queries, a clip gallery, statistics per gallery row over the queries; side 0: clip queries, a caption
    gallery, statistics per query row over the gallery"""
    Bq, n, k = 9, 1000, 300
    g = torch.Generator().manual_seed(60 + side)
    q = _planes(torch.randn(Bq, 64, generator=g), not side)
    gal = _planes(torch.randn(n + BEHIND, 64, generator=g), bool(side))
    if side:
        S_tv = _matrix(q, gal, n, MULT, 2)
        m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, 2)
        nt = Bq
    else:
        S_tv = _matrix(gal[:n].contiguous(), q, Bq, MULT, 2)
        m, s = op.dsl_col_stats_planes(gal, q, n, Bq, MULT, 2)
        nt = n
    D = S_tv.clone()
    op.dsl_apply_(D, m, s, nt)
    D_qg, S_qg = (D, S_tv) if side else (D.t().contiguous(), S_tv.t().contiguous())
    if side:
        assert not np.array_equal(deep_ref(D_qg, k)[1], deep_ref(S_qg, k)[1]), "the case cannot tell D from S"
    stats = (m, s, side, nt)
    whole = _deep(q, gal, n, 2, k, stats=stats)
    _assert_list(whole, deep_ref(D_qg, k))
    first = _deep(q, gal, n, 2, 130, stats=stats)
    after = _last(first)
    _assert_list(_deep(q, gal, n, 2, 170, stats=stats, after=after), deep_ref(D_qg, 170, after=after))
    sel = np.random.default_rng(6).random(n) < 0.6
    _assert_list(_deep(q, gal, n, 2, k, mask=_mask(sel, n), stats=stats), deep_ref(D_qg, k, sel=sel))


# ------------------------------------------------------------------------------------------------ 7. groups
def _grouped_case(seed, Bq, sizes, spread=0.05):
    """rows of a group = one direction plus a little noise, so a group's second-best row scores close to its best and above
    the best rows of most other groups -> (q, gal, head [n + BEHIND], n)"""
    g = torch.Generator().manual_seed(seed)
    sizes = np.asarray(sizes)
    n = int(sizes.sum())
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    head = np.concatenate([np.repeat(starts, sizes), np.arange(n, n + BEHIND)]).astype(np.int32)
    base = torch.randn(len(sizes), 64, generator=g)
    rows = base[torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes))] + spread * torch.randn(n, 64, generator=g)
    rows = torch.cat([rows, torch.randn(BEHIND, 64, generator=g)])
    return _planes(torch.randn(Bq, 64, generator=g), False), _planes(rows, True), head, n


def _group_sizes(seed, n, lo, hi, first=()):
    """sizes of adjacent groups that cover n rows: `first`, then uniform draws from [lo, hi], the last one cut to fit"""
    rng = np.random.default_rng(seed)
    sizes = list(first)
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(lo, hi + 1)), n - sum(sizes)))
    return sizes


def test_groups_whose_second_best_row_beats_other_groups_best():
    sizes = _group_sizes(70, 3000, 1, 13, first=(3, 40, 1, 17, 33))         # 1 to 40 rows, about 7 on average
    assert sum(sizes) == 3000 and 380 <= len(sizes) <= 450 and min(sizes) == 1 and max(sizes) == 40
    q, gal, head, n = _grouped_case(70, 5, sizes)
    k = 300
    S = _matrix(q, gal, n, MULT, 2)
    want = deep_ref(S, k, head=head[:n])
    # the trap is set: in many of the groups that are returned the second-best row beats the best row of the k-th group, so
    # a bound applied to rows (not to finished groups) would bring those groups back on a later page
    Sn = S.cpu().numpy()
    for qi in range(5):
        kth = Sn[qi, want[1][qi, k - 1]]
        second = [np.sort(Sn[qi, head[:n] == head[i]])[-2] for i in want[1][qi, :128] if (head[:n] == head[i]).sum() > 1]
        assert sum(x > kth for x in second) >= 64
    got = _deep(q, gal, n, 2, k, head=head)
    _assert_list(got, want)
    labels = head[got[1].cpu().numpy()]
    assert all(len(set(row)) == k for row in labels.tolist()), "a group appears twice"
    # with a cursor: the position is the group's best row
    first = _deep(q, gal, n, 2, 100, head=head)
    after = _last(first)
    rest = _deep(q, gal, n, 2, 200, head=head, after=after)
    _assert_list(rest, deep_ref(S, 200, head=head[:n], after=after))
    assert torch.equal(torch.cat([first[1], rest[1]], 1), got[1])
    # more entries than groups: the fill inside a later page
    _assert_list(_deep(q, gal, n, 2, 600, head=head), deep_ref(S, 600, head=head[:n]))
    assert len(sizes) < 600


def test_one_group_of_a_thousand_rows_among_singletons():
    sizes = [1] * 200 + [1000] + [1] * 300
    q, gal, head, n = _grouped_case(71, 5, sizes, spread=0.5)
    k = 300
    S = _matrix(q, gal, n, MULT, 2)
    got = _deep(q, gal, n, 2, k, head=head)
    _assert_list(got, deep_ref(S, k, head=head[:n]))
    assert bool(((head[got[1].cpu().numpy()] == 200).sum(1) == 1).all())   # the large group: once, in every query's list
    rng = np.random.default_rng(71)
    tiles = np.repeat((np.arange(-(-n // 16)) % 3) != 1, 16)[:n]
    for sel in (rng.random(n) < 0.5, tiles, rng.random((5, n)) < 0.4):     # a group is ranked by its best SELECTABLE row
        _assert_list(_deep(q, gal, n, 2, k, mask=_mask(sel, n), head=head), deep_ref(S, k, sel=sel, head=head[:n]))
    sel = rng.random(n) < 0.7
    first = _deep(q, gal, n, 2, 100, mask=_mask(sel, n), head=head)
    after = _last(first)
    rest = _deep(q, gal, n, 2, 200, mask=_mask(sel, n), head=head, after=after)
    _assert_list(rest, deep_ref(S, 200, sel=sel, head=head[:n], after=after))
    whole = deep_ref(S, 300, sel=sel, head=head[:n])
    assert np.array_equal(np.concatenate([first[1].cpu().numpy(), rest[1].cpu().numpy()], 1), whole[1])


# ------------------------------------------------------------------------------------------------ 8. wide rows
@pytest.mark.parametrize("E,Bq,n,k,products", [(512, 16, 3001, 300, 2), (1024, 7, 400, 300, 3)])
def test_wide_rows(E, Bq, n, k, products):
    """(1024, 3): the streaming launch's LDS holds lists of 127, so the pages are 127 long"""
    q, gal = _randn_planes(E + n, Bq, n + 5, E)
    S = _matrix(q, gal, n, MULT, products)
    _assert_list(_deep(q, gal, n, products, k), deep_ref(S, k))
    first = _deep(q, gal, n, products, 127)
    _assert_list(_deep(q, gal, n, products, 128, after=_last(first)), deep_ref(S, 128, after=_last(first)))


# ------------------------------------------------------------------------------------------------ 9. rank
def test_the_rank_is_the_index_in_the_deep_list():
    n, Bq = 1000, 5
    q, gal = _randn_planes(90, Bq, n + BEHIND, 64)
    scores, ids = _deep(q, gal, n, 2, 1000)
    at = torch.tensor([129, 200, 383, 640, 999], device=DEV)
    target = ids.gather(1, at[:, None])[:, 0]
    counts, tscore = op.similarity_rank(q, gal, n, MULT, 2, target)
    assert torch.equal(counts[:, 0].long() + counts[:, 2], at) and _bits(tscore, scores.gather(1, at[:, None])[:, 0].contiguous())
    sizes = _group_sizes(91, n, 1, 5)
    head = np.concatenate([np.repeat(np.concatenate(([0], np.cumsum(sizes)[:-1])), sizes), np.arange(n, n + BEHIND)]).astype(np.int32)
    gs, gi = _deep(q, gal, n, 2, 300, head=head)
    at = torch.tensor([128, 129, 200, 255, 299], device=DEV)
    target = gi.gather(1, at[:, None])[:, 0]
    assert bool((target >= 0).all())
    counts, tscore = op.similarity_rank(q, gal, n, MULT, 2, target, group_head=_dev(head))
    assert torch.equal(counts[:, 0].long() + counts[:, 2], at) and _bits(tscore, gs.gather(1, at[:, None])[:, 0].contiguous())


# ------------------------------------------------------------------------------------------------ 10. FeatureGallery
@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(HERE, "golden", "r2_golden.npz"))


@pytest.fixture(scope="module")
def model(g2):
    from centerclip_amd.clip4clip import CLIP4Clip
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    Tf = int(g2["s1_cfg"][11])
    kw = dict(cluster_inter=0, deep_cluster=0, cluster_algo='kmediods++', max_frames=Tf, target_frames_blocks=[Tf, Tf, Tf],
              cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
              minkowski_norm_p=2.0, aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True,
              sim_header='meanP', linear_patch='2d', pre_visual_pooling=0)
    return CLIP4Clip.from_state_dict(sd, Namespace(**kw)).to(DEV).eval()


N_ROWS, N_Q = 500, 6


def _features(g2, seed):
    """(clip features [N_ROWS, E] pooled rows, caption features [N_ROWS, 1, E], query captions [N_Q, 1, E], query clips
    [N_Q, T, E] and their mask [N_Q, 1, T])"""
    E, Tf = int(g2["s1_cfg"][0]), int(g2["s1_cfg"][11])
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones(N_Q, 1, Tf, dtype=torch.long)
    mask[2, 0, 2:] = 0
    return tuple(t.to(DEV) for t in (torch.randn(N_ROWS, E, generator=g), torch.randn(N_ROWS, 1, E, generator=g),
                                     torch.randn(N_Q, 1, E, generator=g), torch.randn(N_Q, Tf, E, generator=g), mask))


def test_feature_gallery_rows_lists_and_cursors(g2, model):
    from centerclip_amd.search import FeatureGallery
    clips, _, seq, _, _ = _features(g2, 100)
    gal = FeatureGallery(model, capacity=64)
    for part in torch.split(clips, [200, 1, 299]):
        gal.add_features(part)
    S = gal.similarity_features(seq)
    assert S.shape == (N_Q, N_ROWS)
    got = gal.search_features(seq, k=200)
    _assert_list(got, deep_ref(S, 200))
    _assert_list(gal.search_features(seq, k=600), deep_ref(S, 600))        # more than the gallery holds: the fill
    # k <= 128 without after=: the plain op, as before
    plain = op.similarity_topk(gal._query_rows(seq, None), gal._rows, gal._n, gal._mult(), gal.products, 100)
    small = gal.search_features(seq, k=100)
    assert torch.equal(small[1], plain[1]) and _bits(small[0], plain[0])
    _assert_list(small, deep_ref(S, 100))
    # after=: the next entries; k + after = the columns of one call
    nxt = gal.search_features(seq, k=100, after=_last(small))
    assert torch.equal(torch.cat([small[1], nxt[1]], 1), got[1]) and _bits(torch.cat([small[0], nxt[0]], 1), got[0])
    tenant = np.random.default_rng(100).random(N_ROWS) < 0.5
    allow = gal.row_mask(positions=np.flatnonzero(tenant).tolist())
    _assert_list(gal.search_features(seq, k=150, allow=allow, after=_last(small)), deep_ref(S, 150, sel=tenant, after=_last(small)))
    # a cursor whose row is removed between the two calls still continues behind it
    gone = torch.unique(torch.cat([small[1][:, -1], small[1][:, 5], got[1][:, 150]])).cpu()
    gal.remove(gone)
    live = np.ones(N_ROWS, dtype=bool)
    live[gone.numpy()] = False
    S2 = gal.similarity_features(seq)
    assert bool(torch.isneginf(S2[:, gone.to(DEV)]).all())
    _assert_list(gal.search_features(seq, k=200, after=_last(small)), deep_ref(S, 200, sel=live, after=_last(small)))
    _assert_list(gal.search_features(seq, k=200), deep_ref(S, 200, sel=live))
    _assert_list(gal.search_features(seq, k=130, allow=allow), deep_ref(S, 130, sel=live & tenant))
    empty = FeatureGallery(model)
    for kw in (dict(k=300), dict(k=5, after=_last(small))):
        s0, i0 = empty.search_features(seq, **kw)
        assert tuple(i0.shape) == (N_Q, kw["k"]) and bool((i0 == -1).all()) and bool(torch.isneginf(s0).all())
    for bad in (dict(k=4097), dict(k=0), dict(k=5, after=(small[0][:, -1].cpu(), small[1][:, -1])), dict(k=5, after=_last(small)[0])):
        with pytest.raises(ValueError):
            gal.search_features(seq, **bad)


def test_feature_gallery_groups_lists_and_cursors(g2, model):
    from centerclip_amd.search import FeatureGallery
    _, caps, _, vis, vmask = _features(g2, 101)
    sizes = _group_sizes(101, N_ROWS, 1, 3)
    labels = np.repeat(1000 + 7 * np.arange(len(sizes)), sizes)
    assert len(sizes) > 200
    tg = FeatureGallery(model, side="text", grouped=True)
    for a, b in ((0, 123), (123, N_ROWS)):                                 # (a group continues across the two calls)
        tg.add_features(caps[a:b], group=labels[a:b].tolist())
    S = tg.similarity_features(vis, vmask)
    assert S.shape == (N_Q, N_ROWS)
    want = deep_ref(S, 200, head=labels)
    scores, labs, pos = tg.search_groups_features(vis, k=200, mask=vmask)
    _assert_list((scores, pos), want)
    assert np.array_equal(labs.cpu().numpy(), labels[want[1]]) and all(len(set(r)) == 200 for r in labs.tolist())
    s1, l1, p1 = tg.search_groups_features(vis, k=70, mask=vmask)
    s2, l2, p2 = tg.search_groups_features(vis, k=130, mask=vmask, after=(s1[:, -1], p1[:, -1]))
    assert torch.equal(torch.cat([p1, p2], 1), pos) and torch.equal(torch.cat([l1, l2], 1), labs)
    assert _bits(torch.cat([s1, s2], 1), scores)
    s3, l3, p3 = tg.search_groups_features(vis, k=300, mask=vmask, after=(s2[:, -1], p2[:, -1]))      # runs into the fill
    _assert_list((s3, p3), deep_ref(S, 300, head=labels, after=(s2[:, -1], p2[:, -1])))
    assert bool((l3[:, -1] == -1).all()) and bool((p3[:, -1] == -1).all())
    _assert_list(tg.search_features(vis, k=200, mask=vmask), deep_ref(S, 200))                      # search* keep ranking rows


def test_feature_gallery_dual_softmax_both_sides(g2, model):
    from centerclip_amd.search import FeatureGallery
    clips, caps, seq, vis, vmask = _features(g2, 102)
    gal = FeatureGallery(model, dual_softmax=True)
    gal.set_query_bank_features(caps[:40])
    gal.add_features(clips)
    D = gal.similarity_features(seq)
    whole = gal.search_features(seq, k=200)
    _assert_list(whole, deep_ref(D, 200))
    first = gal.search_features(seq, k=60)
    _assert_list(gal.search_features(seq, k=140, after=_last(first)), deep_ref(D, 140, after=_last(first)))
    tg = FeatureGallery(model, side="text", dual_softmax=True)             # the queries' statistics: once per call
    tg.add_features(caps)
    Dt = tg.similarity_features(vis, vmask)
    whole = tg.search_features(vis, k=200, mask=vmask)
    _assert_list(whole, deep_ref(Dt, 200))
    first = tg.search_features(vis, k=60, mask=vmask)
    _assert_list(tg.search_features(vis, k=140, mask=vmask, after=_last(first)), deep_ref(Dt, 140, after=_last(first)))
    tg.remove(sorted({3, 77, int(whole[1][0, 0])}))                        # the softmax runs over the captions still held
    Dt2 = tg.similarity_features(vis, vmask)
    _assert_list(tg.search_features(vis, k=200, mask=vmask), deep_ref(Dt2, 200, sel=~torch.isneginf(Dt2[0]).cpu().numpy()))


# ------------------------------------------------------------------------------------------------ 11. no host synchronisation
def _sync_debug_mode_is_honoured():
    """does this torch build raise on a synchronising call under set_sync_debug_mode("error")?"""
    x = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.sum().item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_a_deep_search_does_not_synchronise_with_the_host(g2, model):
    from centerclip_amd.search import FeatureGallery
    clips, _, seq, _, _ = _features(g2, 103)
    gal = FeatureGallery(model)
    gal.add_features(clips)
    gal.remove([5, 250])
    warm = gal.search_features(seq, k=300)                                 # warm-up: workspaces, the cached logit scale
    after = _last(gal.search_features(seq, k=40))
    want_after = gal.search_features(seq, k=300, after=after)
    torch.cuda.synchronize()
    if _sync_debug_mode_is_honoured():
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = gal.search_features(seq, k=300)
            got_after = gal.search_features(seq, k=300, after=after)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:                                                                  # a capture fails on any synchronising call
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            gal.search_features(seq, k=300, after=after)                   # (this stream's workspace)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            got = gal.search_features(seq, k=300)
            got_after = gal.search_features(seq, k=300, after=after)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[1], warm[1]) and _bits(got[0], warm[0])
    assert torch.equal(got_after[1], want_after[1]) and _bits(got_after[0], want_after[0])
    S = gal.similarity_features(seq)
    _assert_list(got, deep_ref(S, 300, sel=~torch.isneginf(S[0]).cpu().numpy()))
