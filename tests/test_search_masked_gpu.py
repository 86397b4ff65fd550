"""Masked search on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_topk_masked, dsl_col_stats_planes_masked and
pack_row_mask, and FeatureGallery's remove / compact / allow= on the small model.

Every reference is existing code on the same rows, never the code under test: S = scaled_dot_planes on a zero-padded copy
(``_matrix``), for the dual softmax D = dsl_apply_ on S, then ``masked_topk_ref`` of tests/test_search_masked_host.py - the
unselectable columns dropped, np.argsort(-S, kind="stable") (grouped: grouped_topk_ref over the selectable rows).  Ids
equal, scores bit-equal, the fill (-inf, -1) exact.  The one tolerance is the statistics sum s: planes_stats_bound's rule with
the depth of the full Bt tree and the sums over the selectable rows.  E = 64 unless said; galleries carry 37 non-zero rows
behind n and masks carry ones above n in their last word, none of which may appear."""
import io

import numpy as np
import pytest
import torch

import dsl_ref as R
from centerclip_amd import _lib as L
from test_search_dsl_gpu import planes_stats_bound
from test_search_gpu import DEV, MULT, N_CLIPS, _bits, _dataset, _eval_model, _matrix, _planes, g2  # noqa: F401  (g2: the fixture)
from test_search_grouped_gpu import LABELS, PATTERN, _heads
from test_search_masked_host import masked_topk_ref, pack_bits

pytestmark = pytest.mark.gpu
op = torch.ops.centerclip
BEHIND = 37


def _randn_planes(seed, Bq, rows, E=64, text_queries=True):
    g = torch.Generator().manual_seed(seed)
    return _planes(torch.randn(Bq, E, generator=g), not text_queries), _planes(torch.randn(rows, E, generator=g), text_queries)


def _mask(sel, n):
    """bool [n] or [Bq, n] -> device mask words; the bits at n or above in the last word are ones (garbage to ignore)"""
    words = pack_bits(np.asarray(sel, dtype=bool)[..., :n])
    if n % 32:
        words[..., -1] |= np.int32(-1) << np.int32(n % 32)
    return torch.from_numpy(words).to(DEV)


def _assert_masked(scores, ids, M, sel, k, head=None):
    Mn = M.cpu().numpy() if torch.is_tensor(M) else M
    want_scores, want_ids = masked_topk_ref(Mn, sel, k, None if head is None else head[:Mn.shape[1]])
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and tuple(ids.shape) == tuple(scores.shape) == (Mn.shape[0], k)
    assert np.array_equal(ids.cpu().numpy(), want_ids), "ids differ from the stable descending sort of the selectable rows"
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want_scores.view(np.uint32)), "scores are not the matrix op's bits"


_cache = {}


def _case(seed, Bq, n, E=64, products=2):
    """planes and the matrix op's S, computed once per case and left unchanged"""
    key = (seed, Bq, n, E, products)
    if key not in _cache:
        q, gal = _randn_planes(seed, Bq, n + BEHIND, E)
        _cache[key] = (q, gal, _matrix(q, gal, n, MULT, products))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. all ones
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 255, 257, 1000, 4099])
def test_an_all_ones_mask_is_the_unmasked_op_bit_for_bit(n):
    k, products = 10, 2
    head = _heads(PATTERN, n)
    hd = torch.from_numpy(head).to(DEV)
    for Bq in (1, 16, 17, 33):
        if n == 4099 and Bq <= 16:
            assert L.lib().cc_similarity_topk_slices(Bq, n, k) >= 2
        q, gal, S = _case(n, Bq, n)
        m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, products)
        plain = op.similarity_topk(q, gal, n, MULT, products, k)
        grouped = op.similarity_topk_grouped(q, gal, n, MULT, products, k, hd)
        dsl = op.similarity_topk_dsl(q, gal, n, MULT, products, k, m, s, 1, Bq)
        both = op.similarity_topk_grouped_dsl(q, gal, n, MULT, products, k, m, s, 1, Bq, hd)
        for mask in (_mask(np.ones(n, dtype=bool), n), _mask(np.ones((Bq, n), dtype=bool), n)):
            for want, extra in ((plain, {}), (grouped, dict(group_head=hd)), (dsl, dict(m=m, s=s, n_total=Bq)),
                                (both, dict(m=m, s=s, n_total=Bq, group_head=hd))):
                got = op.similarity_topk_masked(q, gal, n, MULT, products, k, mask, **extra)
                assert torch.equal(got[1], want[1]) and _bits(got[0], want[0]), (Bq, tuple(mask.shape), sorted(extra))


# ------------------------------------------------------------------------------------------------ 2. shared masks
def _shared_masks():
    rng = np.random.default_rng(20262)
    n = 4099
    rows = np.arange(n)
    one_per_tile = np.zeros(n, dtype=bool)
    one_per_tile[(rows // 16) * 16 + (rows // 16) % 16 == rows] = True
    t0, t1 = 257 * 3 // 8, 257 * 4 // 8                                    # slice 3 of the 8 slices of 257 tiles
    cases = [("none", n, np.zeros(n, dtype=bool)), ("row 0", n, rows == 0), ("row n-1", n, rows == n - 1),
             ("a middle row", n, rows == 2051), ("every other row", n, rows % 2 == 0), ("one row per tile", n, one_per_tile),
             ("a block off the tile grid", n, (rows >= 37) & (rows < 137)),
             ("one wave's tiles dead", 1000, (np.arange(1000) // 16) % 4 != 1),
             ("one slice dead", n, (rows < 16 * t0) | (rows >= 16 * t1)),
             ("p = 0.5", n, rng.random(n) < 0.5), ("p = 0.02", 1000, rng.random(1000) < 0.02),
             ("p = 0.5, odd n", 257, rng.random(257) < 0.5)]
    ks = (1, 10, 65, 128)
    return [pytest.param(nn, sel, 64 if name == "p = 0.02" else ks[i % 4], 1 + i % 3, id=name)
            for i, (name, nn, sel) in enumerate(cases)]


@pytest.mark.parametrize("n,sel,k,products", _shared_masks())
def test_shared_masks_against_the_reference(n, sel, k, products):
    assert L.lib().cc_similarity_topk_slices(17, 4099, k) == 8
    if k == 64:
        assert 0 < int(sel.sum()) < k                                      # k above the selectable count: the fill starts early
    for Bq in (5, 17):
        q, gal, S = _case(7 * n + Bq, Bq, n, products=products)
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, k, _mask(sel, n))
        _assert_masked(scores, ids, S, sel, k)


# ------------------------------------------------------------------------------------------------ 3. per-query masks
@pytest.mark.parametrize("Bq", [5, 17, 33])
def test_per_query_masks(Bq):
    n = 1000
    q, gal, S = _case(31 + Bq, Bq, n)
    rng = np.random.default_rng(Bq)
    own = np.ones((Bq, n), dtype=bool)
    own[np.arange(Bq), np.arange(Bq) * 29] = False                         # "query i may not see row 29 i"
    best = S.argmax(dim=1).cpu().numpy()
    not_best = np.ones((Bq, n), dtype=bool)
    not_best[np.arange(Bq), best] = False                                  # ... nor its best row
    for sel, k in ((rng.random((Bq, n)) < 0.5, 10), (rng.random((Bq, n)) < 0.01, 65), (own, 128), (not_best, 1)):
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, 2, k, _mask(sel, n))
        _assert_masked(scores, ids, S, sel, k)
    assert not bool((ids[:, 0].cpu() == torch.from_numpy(best)).any())


# ------------------------------------------------------------------------------------------------ 4. ties
def test_identical_rows_come_in_id_order_among_the_selectable():
    n = 4099
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(5, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(n, 64), True)
    sel = np.arange(n) % 3 == 1
    S = _matrix(q, gal, n, MULT, 2)
    for k in (10, 128):
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, 2, k, _mask(sel, n))
        _assert_masked(scores, ids, S, sel, k)
        assert torch.equal(ids.cpu(), (1 + 3 * torch.arange(k)).expand(5, k))


# ------------------------------------------------------------------------------------------------ 5. groups
def _group_masks(head, n, S):
    starts = np.unique(head[:n])
    ends = np.append(starts[1:], n)
    group = np.searchsorted(starts, head[:n])                              # the group index of every row
    rows = np.arange(n)
    best0 = np.array([s + int(np.argmax(S[0, s:e])) for s, e in zip(starts, ends)])       # query 0's best row of every group
    out = {"whole groups dead": group % 3 != 1,
           "only the best row dead": ~np.isin(rows, best0),
           "only the head row dead": ~np.isin(rows, starts),
           "all but the last row dead": np.isin(rows, ends - 1),
           "whole groups and single rows dead": (group % 2 == 0) & (rows % 5 != 0)}
    return out


@pytest.mark.parametrize("n", [257, 4099])
def test_grouped_masks_against_the_reference(n):
    Bq, products = 17, 3
    q, gal, S = _case(n + 1, Bq, n, products=products)
    head = _heads(PATTERN, n)
    hd = torch.from_numpy(head).to(DEV)
    for name, sel in _group_masks(head, n, S.cpu().numpy()).items():
        for k in (1, 10, 128):
            scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, k, _mask(sel, n), group_head=hd)
            _assert_masked(scores, ids, S, sel, k, head)
    rng = np.random.default_rng(n)
    per_query = rng.random((Bq, n)) < 0.3                                  # one mask per query row: nothing is skipped
    scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, 10, _mask(per_query, n), group_head=hd)
    _assert_masked(scores, ids, S, per_query, 10, head)


def test_dead_tiles_full_of_heads_and_a_dead_tile_inside_a_long_group():
    n, Bq, k = 4099, 5, 128
    q, gal, S = _case(77, Bq, n)
    rows = np.arange(n)
    # singleton groups up to row 600, one group of 1000 rows, then the pattern again
    head = np.concatenate([np.arange(600), np.full(1000, 600), 1600 + _heads(PATTERN, n - 1600)]).astype(np.int32)
    hd = torch.from_numpy(head).to(DEV)
    runs = np.ones(n, dtype=bool)
    runs[100:133] = False                                                  # 33 dead singletons: one dead tile full of heads
    runs[200:290] = False                                                  # 90 more: five of them
    long_group = np.ones(n, dtype=bool)
    long_group[640:700] = False                                            # dead tiles inside the long group, off the grid
    long_group[1120:1136] = False                                          # and exactly one tile of it
    head_and_tail = np.ones(n, dtype=bool)
    head_and_tail[592:1590] = False                                        # the group's head tile dead; its last rows live
    only_inside = np.zeros(n, dtype=bool)
    only_inside[[650, 1599, 3000]] = True                                  # nearly every tile dead
    for sel in (runs, long_group, runs & long_group, head_and_tail, only_inside):
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, 2, k, _mask(sel, n), group_head=hd)
        _assert_masked(scores, ids, S, sel, k, head)


@pytest.mark.parametrize("n", [17, 4099])
def test_singleton_groups_with_a_mask_are_the_masked_plain_op(n):
    q, gal, S = _case(5 * n, 17, n)
    sel = np.random.default_rng(n).random(n) < 0.4
    sel[0] = True
    hd = torch.arange(n + BEHIND, device=DEV, dtype=torch.int32)
    for k in (1, 10, 128):
        a = op.similarity_topk_masked(q, gal, n, MULT, 2, k, _mask(sel, n))
        b = op.similarity_topk_masked(q, gal, n, MULT, 2, k, _mask(sel, n), group_head=hd)
        assert torch.equal(a[1], b[1]) and _bits(a[0], b[0])
        _assert_masked(a[0], a[1], S, sel, k)


# ------------------------------------------------------------------------------------------------ 6. dual softmax
@pytest.mark.parametrize("Bq,n", [(33, 1000), (5, 4099)])
@pytest.mark.parametrize("side", [0, 1])
def test_dual_softmax(Bq, n, side):
    """side 1: text queries, a clip gallery, statistics per gallery row; side 0: clip queries, a caption gallery, statistics
    per query row - from dsl_col_stats_planes, D from dsl_apply_ on S as tests/test_search_dsl_gpu.py does"""
    q, gal = _randn_planes(100 * Bq + n + side, Bq, n + BEHIND, text_queries=bool(side))
    head, k, products = _heads(PATTERN, n), 10, 2
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
    for sel in (rng.random(n) < 0.5, (np.arange(n) >= 37) & (np.arange(n) < 137), rng.random((Bq, n)) < 0.5):
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, k, _mask(sel, n), m, s, side, nt)
        _assert_masked(scores, ids, D_qg, sel, k)
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, k, _mask(sel, n), m, s, side, nt, hd)
        _assert_masked(scores, ids, D_qg, sel, k, head)


# ------------------------------------------------------------------------------------------------ 7. masked statistics
def masked_stats_bound(S, live, slices):
    """planes_stats_bound's rule for the masked tree: the depth of the FULL Bt tree (the masked rows only leave terms out),
    the sums over the live rows"""
    _, depth = planes_stats_bound(S, slices)
    x = np.asarray(S, dtype=np.float64)[live]
    m, s64 = R.col_stats64(x)
    t = np.exp(x - m[None, :])
    return R.U * (depth * s64 + (np.abs(x - m[None, :]) * t).sum(axis=0)), m, s64


def _stats_masks():
    rng = np.random.default_rng(20263)
    assert -(-4099 // 16) // 32 == 8                                       # 8 slices of the 257 text tiles (Bt alone)
    t0, t1 = 257 * 1 // 8, 257 * 2 // 8
    return [pytest.param(1203, np.arange(1203) >= 160, id="the first tiles dead"),
            pytest.param(1203, (np.arange(1203) // 16) % 4 != 2, id="one wave's tiles dead"),
            pytest.param(4099, (np.arange(4099) < 16 * t0) | (np.arange(4099) >= 16 * t1), id="one slice dead"),
            pytest.param(17, rng.random(17) < 0.5, id="p = 0.5, 17"), pytest.param(257, rng.random(257) < 0.5, id="p = 0.5, 257"),
            pytest.param(1203, rng.random(1203) < 0.5, id="p = 0.5, 1203")]


@pytest.mark.parametrize("Bt,live", _stats_masks())
def test_masked_statistics(Bt, live):
    Bv, products = 37, 2
    g = torch.Generator().manual_seed(Bt)
    text, video = _planes(torch.randn(Bt + BEHIND, 64, generator=g), False), _planes(torch.randn(Bv + BEHIND, 64, generator=g), True)
    S = _matrix(text[:Bt].contiguous(), video, Bv, MULT, products)
    slices = L.lib().cc_dsl_col_stats_planes_slices(Bt)
    assert (slices >= 2 or Bt != 4099) and live.any()
    plain = op.dsl_col_stats_planes(text, video, Bt, Bv, MULT, products)
    ones = op.dsl_col_stats_planes_masked(text, video, Bt, Bv, MULT, products, _mask(np.ones(Bt, dtype=bool), Bt))
    assert _bits(ones[0], plain[0]) and _bits(ones[1], plain[1])           # all ones: the unmasked op bit for bit
    m, s = op.dsl_col_stats_planes_masked(text, video, Bt, Bv, MULT, products, _mask(live, Bt))
    m2, s2 = op.dsl_col_stats_planes_masked(text, video, Bt, Bv, MULT, products, _mask(live, Bt))
    assert _bits(m, m2) and _bits(s, s2) and m.shape == s.shape == (Bv,)
    assert not bool(torch.isnan(m).any()) and not bool(torch.isnan(s).any())
    assert _bits(m, S[torch.from_numpy(live).to(DEV)].max(dim=0).values)   # the matrix op's maximum over the live rows
    bound, m64, s64 = masked_stats_bound(S.cpu().numpy(), live, slices)
    err = np.abs(s.cpu().numpy().astype(np.float64) - s64)
    print(f"[masked planes stats {Bt}x{Bv}, {int(live.sum())} live] worst |s - s64| / bound = {float((err / bound).max()):.3f}")
    assert np.array_equal(m.cpu().numpy().astype(np.float64), m64) and (err <= bound).all()
    m, s = op.dsl_col_stats_planes_masked(text, video, Bt, Bv, MULT, products, _mask(np.zeros(Bt, dtype=bool), Bt))
    assert bool(torch.isneginf(m).all()) and bool((s == 0).all())          # no live row: the neutral pair


# ------------------------------------------------------------------------------------------------ 8. packing
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 1000])
def test_pack_row_mask(n, R_):
    flags = np.random.default_rng(n + R_).random((R_, n)) < 0.5
    want = np.packbits(flags, axis=1, bitorder="little")
    want = np.concatenate([want, np.zeros((R_, -want.shape[1] % 4), dtype=np.uint8)], axis=1).view("<u4")
    for t in (torch.from_numpy(flags), torch.from_numpy(flags.astype(np.uint8) * 7)):     # bool, and non-zero bytes
        out = op.pack_row_mask(t.to(DEV))
        assert out.dtype == torch.int32 and tuple(out.shape) == (R_, (n + 31) // 32)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(op.pack_row_mask(torch.from_numpy(flags[0]).to(DEV)).cpu().numpy().view(np.uint32), want[:1])
    assert np.array_equal(want.view(np.int32), pack_bits(flags))           # (the host helper the other tests use)


# ------------------------------------------------------------------------------------------------ 9. wide rows
@pytest.mark.parametrize("E,Bq,n,k,products", [(512, 16, 3001, 100, 2), (768, 7, 2000, 128, 3)])
def test_wide_rows(E, Bq, n, k, products):
    q, gal = _randn_planes(E + n, Bq, n + 5, E)
    S = _matrix(q, gal, n, MULT, products)
    rng = np.random.default_rng(E)
    sel = (rng.random(n) < 0.5) & ((np.arange(n) // 16) % 5 != 2)          # dead tiles and half-live ones
    scores, ids = op.similarity_topk_masked(q, gal, n, MULT, products, k, _mask(sel, n))
    _assert_masked(scores, ids, S, sel, k)


# ------------------------------------------------------------------------------------------------ 10. capture
def test_graph_capture_and_replay_with_a_changing_mask():
    Bq, n, k = 5, 4099, 10
    q, gal, S = _case(15, Bq, n)
    rng = np.random.default_rng(15)
    masks = [rng.random(n) < 0.5, (np.arange(n) // 16) % 7 == 3, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)]
    mbuf = _mask(masks[-1], n).clone()
    op.similarity_topk_masked(q, gal, n, MULT, 2, k, mbuf)                 # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, ids = op.similarity_topk_masked(q, gal, n, MULT, 2, k, mbuf)
    for sel in masks:
        mbuf.copy_(_mask(sel, n))
        graph.replay()
        torch.cuda.synchronize()
        _assert_masked(scores, ids, S, sel, k)


# ------------------------------------------------------------------------------------------------ 11. FeatureGallery
GONE = (0, 3, 5, 6)                                                        # of the 12 clips: a head row, a whole group (row 3), rows inside one


def _state_equal(a, b):
    assert set(a) == set(b)
    for key in a:
        if torch.is_tensor(a[key]):
            assert _bits(a[key].cpu(), b[key].cpu()), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("cluster_inter", [0, 1])
@pytest.mark.parametrize("side", ["video", "text"])
@pytest.mark.parametrize("dual_softmax,grouped", [(False, False), (True, True)])
def test_feature_gallery_remove_compact_allow(g2, cluster_inter, side, dual_softmax, grouped):
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, cluster_inter)
    video, vmask, ids = _dataset(g2["s1_cfg"])
    n, keep = N_CLIPS, [i for i in range(N_CLIPS) if i not in GONE]
    kw = dict(side=side, dual_softmax=dual_softmax, grouped=grouped)
    items = (lambda sl: (video[sl], vmask[sl])) if side == "video" else (lambda sl: (ids[sl],))
    query = (ids,) if side == "video" else (video, vmask)
    label = (lambda sl: dict(group=list(LABELS[sl]))) if grouped else (lambda sl: {})

    def build(order):
        gal = FeatureGallery(model, capacity=4, **kw)
        if dual_softmax and side == "video":
            gal.set_query_bank(ids)
        for i in order:
            gal.add(*items(slice(i, i + 1)), **label(slice(i, i + 1)))
        return gal
    gal, fresh = build(range(n)), build(keep)
    gal.remove(list(GONE[:2]))
    gal.remove(torch.tensor(GONE[2:]))
    assert len(gal) == len(keep) and gal.span == n and len(fresh) == len(keep)
    to_old = torch.tensor(keep + [-1], device=DEV)                         # fresh position -> position here (-1: the fill)

    def same(a, b):                                                        # results of `gal` against `fresh`, positions mapped
        assert _bits(a[0], b[0]) and torch.equal(a[-1], to_old[b[-1]])
        if len(a) == 3:
            assert torch.equal(a[1], b[1])
    # side="text" under the dual softmax: the statistics run over the live captions in the tree of all 12 positions - the
    # fresh gallery's tree of 8 rounds s differently, so there the scores are checked against float64 below, not bit for bit
    exact = not (dual_softmax and side == "text")
    M, Mf = gal.similarity(*query), fresh.similarity(*query)
    live = np.isin(np.arange(n), keep)
    assert M.shape == (n, n) and bool(torch.isneginf(M[:, list(GONE)]).all()) and (not exact or _bits(M[:, keep].contiguous(), Mf))
    for k in (1, 5, 20):
        got = gal.search(*query, k=k)
        _assert_masked(got[0], got[1], M, live, k)
        if exact:
            same(got, fresh.search(*query, k=k))
        if grouped:
            got = gal.search_groups(*query, k=k)
            _assert_masked(got[0], got[2], M, live, k, np.asarray(LABELS))
            if exact:
                same(got, fresh.search_groups(*query, k=k))
    if grouped:
        assert gal.num_groups == fresh.num_groups == 4
    if not exact:                                                          # n_total = len(gallery); D against float64 over the live captions
        plain = FeatureGallery(model, side="text")
        for i in keep:
            plain.add(ids[i:i + 1])
        Sn = plain.similarity(*query).t().contiguous().cpu().numpy()       # [live captions, clips]: the matrix op's S
        bound, _ = planes_stats_bound(Sn, L.lib().cc_dsl_col_stats_planes_slices(n))
        db = R.d_bound(Sn, len(gal), bound)
        derr = np.abs(M[:, keep].t().cpu().numpy().astype(np.float64) - R.dual_softmax64(Sn, len(gal)))
        assert (derr <= db).all()
    # allow=: a device bool tensor, row_mask(), one mask per query; the ranking sees allow & live
    pick = [1, 2, 5, 7, 8, 11]                                             # 5 is removed: allow cannot bring it back
    flags = torch.zeros(n, dtype=torch.bool, device=DEV)
    flags[pick] = True
    sel = np.isin(np.arange(n), [p for p in pick if p in keep])
    head = np.asarray(LABELS)
    for allow in (flags, gal.row_mask(positions=pick), flags.expand(n, n).contiguous()):
        scores, pos = gal.search(*query, k=5, allow=allow)
        _assert_masked(scores, pos, M, sel, 5)
        if grouped:
            scores, labels, pos = gal.search_groups(*query, k=5, allow=allow)
            _assert_masked(scores, pos, M, sel, 5, head)
            assert torch.equal(labels.cpu(), torch.where(pos.cpu() >= 0, torch.tensor(LABELS)[pos.cpu().clamp(min=0)], -1))
    per_query = torch.ones(n, n, dtype=torch.bool, device=DEV)
    per_query[torch.arange(n), torch.arange(n)] = False                    # everything except the query's own partner
    scores, pos = gal.search(*query, k=3, allow=per_query)
    _assert_masked(scores, pos, M, per_query.cpu().numpy() & np.isin(np.arange(n), keep)[None, :], 3)
    if grouped:
        a = gal.search_groups(*query, k=5, allow=gal.row_mask(groups=[52, 74]))
        _assert_masked(a[0], a[2], M, np.isin(head, [52, 74]) & np.isin(np.arange(n), keep), 5, head)
    with pytest.raises(ValueError, match="allow="):
        gal.search(*query, k=3, allow=flags[:5])
    # save / load with removals
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    loaded = FeatureGallery(model, **kw)
    loaded.load_state_dict(torch.load(buf))
    assert len(loaded) == len(keep) and loaded.span == n
    a, b = loaded.search(*query, k=5), gal.search(*query, k=5)
    assert _bits(a[0], b[0]) and torch.equal(a[1], b[1])
    # rows added after a removal get new positions; then compact(): the gallery of the survivors, tensor by tensor
    extra = slice(0, 1)
    lab = dict(group=[99]) if grouped else {}
    assert gal.add(*items(extra), **lab).tolist() == [n] and len(gal) == len(keep) + 1 and gal.span == n + 1
    fresh.add(*items(extra), **lab)
    new_pos = gal.compact()
    assert new_pos.tolist() == [keep.index(i) if i in keep else -1 for i in range(n)] + [len(keep)]
    assert len(gal) == gal.span == len(keep) + 1
    _state_equal(gal.state_dict(), fresh.state_dict())
    a, b = gal.search(*query, k=20), fresh.search(*query, k=20)
    assert _bits(a[0], b[0]) and torch.equal(a[1], b[1])
    if grouped:
        gal.remove_groups([52])
        assert gal.num_groups == fresh.num_groups - 1
        got = gal.search_groups(*query, k=20)
        assert not bool((got[1] == 52).any()) and int((got[1][0] >= 0).sum()) == gal.num_groups
