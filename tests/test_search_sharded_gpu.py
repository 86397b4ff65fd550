"""A gallery split in shards on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_topk_merge against the NumPy statement
of tests/test_search_sharded_host.py, similarity_target_score / similarity_count against similarity_rank and the matrix, and
ShardedGallery (in-process; one two-rank run over gloo) against the concatenated FeatureGallery - one gallery that holds shard
0's positions, then shard 1's, and so on.  Everything is exact: scores by their bits, ids and counts as integers.  E = 64."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_search_deep_gpu import DEV, MULT, _bits, _matrix, _planes, g2, model  # noqa: F401  (g2, model: the fixtures)
from test_search_grouped_gpu import _heads
from test_search_masked_gpu import _mask
from test_search_sharded_host import FRONT_ALL, merge_ref

pytestmark = pytest.mark.gpu
op = torch.ops.centerclip
HERE = os.path.dirname(os.path.abspath(__file__))
VALUES = np.array([3.0, 1.5, 0.0, -0.0, -2.0, -np.inf], dtype=np.float32)   # at most 6 distinct scores: ties cross the lists


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the merge op alone
def _lists(seed, S, Bq, k, fill="mixed"):
    """S valid lists per query row: random scores out of VALUES, distinct random ids, in the lists' order (descending ordered
    score - +0 and -0 tie -, then smaller id), the fill behind; a list holds 0..k entries (mixed), none (all) or k (none)"""
    rng = np.random.default_rng(seed)
    scores = rng.choice(np.float32([7.0, -7.0]), size=(S, Bq, k)).astype(np.float32)           # fills: garbage scores, never read
    ids = np.full((S, Bq, k), -1, dtype=np.int32)
    for s in range(S):
        for q in range(Bq):
            n = {"mixed": int(rng.choice([0, k, rng.integers(0, k + 1)])), "all": 0, "none": k}[fill]
            sc = rng.choice(VALUES, size=n)
            lid = rng.choice(max(2 * k, 8), size=n, replace=False)
            order = np.lexsort((lid, -(sc + np.float32(0.0))))                                 # (-inf sorts last; -0 + 0 = +0)
            scores[s, q, :n], ids[s, q, :n] = sc[order], lid[order]
    return scores, ids


def _assert_merge(scores, ids, seed=0):
    S, Bq, k = scores.shape
    got = op.similarity_topk_merge(_dev(scores), _dev(ids))
    want = merge_ref(scores, ids)
    assert (got[0].dtype, got[1].dtype, got[2].dtype) == (torch.float32, torch.int64, torch.int32)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)), "scores (bits, the sign of zero included)"
    assert np.array_equal(got[1].cpu().numpy(), want[1]), "global ids"
    assert np.array_equal(got[2].cpu().numpy(), want[2]), "src"
    payload = np.random.default_rng(seed).integers(-2 ** 40, 2 ** 40, size=(S, Bq, k))          # what travels with the entries
    flat = _dev(payload).permute(1, 0, 2).reshape(Bq, S * k)
    taken = torch.where(got[2] < 0, -1, flat.gather(1, got[2].clamp(min=0).long())).cpu().numpy()
    sh, lid = want[1] >> 32, want[1] & 0xFFFFFFFF
    for q in range(Bq):                                                                        # the payload of the entry with that id
        for j in np.flatnonzero(want[1][q] >= 0):
            i = int(np.flatnonzero(ids[sh[q, j], q] == lid[q, j])[0])
            assert taken[q, j] == payload[sh[q, j], q, i]
        assert (taken[q][want[1][q] < 0] == -1).all()
    return got


@pytest.mark.parametrize("S", [1, 2, 3, 5, 64])
def test_merge_against_the_numpy_statement(S):
    for k in (1, 7, 128, 129, 300):
        for Bq in (1, 17):
            _assert_merge(*_lists(1000 * S + 10 * k + Bq, S, Bq, k), seed=k)


def test_merge_of_the_longest_lists():
    _assert_merge(*_lists(4096, 2, 17, 4096))
    _assert_merge(*_lists(4097, 2, 1, 4096, fill="none"))


def test_merge_fills_and_zeros():
    for S, k in ((1, 5), (3, 7), (64, 129)):
        got = _assert_merge(*_lists(S + k, S, 3, k, fill="all"))
        assert bool(torch.isneginf(got[0]).all()) and bool((got[1] == -1).all()) and bool((got[2] == -1).all())
        _assert_merge(*_lists(S * k, S, 3, k, fill="none"))
    scores = np.float32([[[0.0, -0.0, -0.0]], [[-0.0, 0.0, -1.0]], [[-0.0, -5.0, 9.0]]])       # +0 against -0 across three lists
    ids = np.int32([[[4, 5, 9]], [[0, 7, 8]], [[3, 6, -1]]])
    got = _assert_merge(scores, ids)
    assert got[1].cpu().tolist() == [[4, 5, 9]] and np.signbit(got[0].cpu().numpy()).tolist() == [[False, True, True]]
    assert op.similarity_topk_merge(_dev(scores[:, :0]), _dev(ids[:, :0]))[1].shape == (0, 3)   # no query row: no launch


# ------------------------------------------------------------------------------------------------ 2. the count op alone
N_COUNT, BQ_COUNT = 333, 9


@pytest.fixture(scope="module")
def count_case():
    """planes with every gallery row held several times (so `==` finds more than one row) and the matrix op's S"""
    g = torch.Generator().manual_seed(5)
    pool = torch.randn(40, 64, generator=g)
    pick = np.random.default_rng(5).integers(0, 40, size=N_COUNT + 37)
    q, gal = _planes(torch.randn(BQ_COUNT, 64, generator=g), False), _planes(pool[pick], True)
    return q, gal, _matrix(q, gal, N_COUNT, MULT, 2).cpu().numpy()


def _count_ref(S, bound, front, sel=None):
    S = S if sel is None else np.where(sel, S, np.nan)                                         # (a NaN is never counted)
    idx = np.arange(S.shape[1])[None, :]
    bound, front = np.asarray(bound, dtype=np.float32)[:, None], np.asarray(front, dtype=np.int64)[:, None]
    on = front >= 0
    return np.stack([((S > bound) & on).sum(1), ((S == bound) & on).sum(1), ((S == bound) & (idx < front) & on).sum(1)], 1)


def test_count_against_the_matrix(count_case):
    q, gal, S = count_case
    n, Bq = N_COUNT, BQ_COUNT
    rng = np.random.default_rng(6)
    cols = rng.integers(0, n, size=Bq)
    bound = S[np.arange(Bq), cols]
    fronts = [np.full(Bq, v) for v in (-1, 0, n, FRONT_ALL)] + [cols, np.resize([-1, 0, 17, n, FRONT_ALL, -(2 ** 31)], Bq)]
    for front in fronts:
        got = op.similarity_count(q, gal, n, MULT, 2, _dev(bound), _dev(front, torch.int32))
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), _count_ref(S, bound, front))
    assert (_count_ref(S, bound, fronts[3])[:, 1] > 1).all() and (_count_ref(S, bound, fronts[3])[:, 2] > 1).all()
    assert (_count_ref(S, bound, fronts[0]) == 0).all() and (_count_ref(S, bound, fronts[1])[:, 2] == 0).all()
    between = np.nextafter(bound, np.float32(np.inf))                                          # a bound equal to no row
    got = op.similarity_count(q, gal, n, MULT, 2, _dev(between), _dev(fronts[3], torch.int32)).cpu().numpy()
    assert np.array_equal(got, _count_ref(S, between, fronts[3])) and (got[:, 1:] == 0).all() and got[:, 0].sum() > 0
    nan = bound.copy()
    nan[::2] = np.nan                                                                          # a NaN bound counts nothing
    got = op.similarity_count(q, gal, n, MULT, 2, _dev(nan), _dev(fronts[3], torch.int32)).cpu().numpy()
    assert np.array_equal(got, _count_ref(S, nan, fronts[3])) and (got[::2] == 0).all() and (got[1::2, 1] > 0).all()
    sel = rng.random(n) < 0.6                                                                  # under a mask, one and per query
    got = op.similarity_count(q, gal, n, MULT, 2, _dev(bound), _dev(cols, torch.int32), _mask(sel, n)).cpu().numpy()
    assert np.array_equal(got, _count_ref(S, bound, cols, sel[None, :]))
    selq = rng.random((Bq, n)) < 0.6
    got = op.similarity_count(q, gal, n, MULT, 2, _dev(bound), _dev(cols, torch.int32), _mask(selq, n)).cpu().numpy()
    assert np.array_equal(got, _count_ref(S, bound, cols, selq))


@pytest.mark.parametrize("n1", [0, 1, 16, 100, 332, 333])
def test_counts_over_any_split_add_up(count_case, n1):
    q, gal, S = count_case
    n, Bq = N_COUNT, BQ_COUNT
    cols = np.random.default_rng(n1).integers(0, n, size=Bq)
    bound, front = _dev(S[np.arange(Bq), cols]), _dev(cols, torch.int32)
    whole = op.similarity_count(q, gal, n, MULT, 2, bound, front)
    a = op.similarity_count(q, gal[:n1], n1, MULT, 2, bound, front)                            # (a front at or above n1: all in front)
    b = op.similarity_count(q, gal[n1:].contiguous(), n - n1, MULT, 2, bound, (front - n1).clamp(min=0))
    assert torch.equal(a + b, whole) and int(whole[:, 1].min()) > 1


def test_target_score_and_count_are_the_launches_of_rank(count_case):
    """score = similarity_rank's; counts against that score with front = the target's row (its group's head) = its counts -
    rows and groups, with and without a mask, under the dual softmax on either side"""
    q, gal, _ = count_case
    n, Bq = N_COUNT, BQ_COUNT
    rng = np.random.default_rng(8)
    head = _heads((3, 1, 2, 5), n)
    gen = torch.Generator().manual_seed(1)
    stat_g = ((torch.randn(n, generator=gen) + 100).to(DEV), (torch.rand(n, generator=gen) + 0.5).to(DEV))
    stat_q = (stat_g[0][:Bq].contiguous(), stat_g[1][:Bq].contiguous())
    sel = rng.random((Bq, n)) < 0.5
    target = rng.integers(0, n, size=Bq)
    target[0], target[1] = -1, n + 3                                                           # outside: -inf, and nothing counted
    for mask in (None, _mask(sel[0], n), _mask(sel, n)):
        for m, s, side in ((None, None, 1), stat_g + (1,), stat_q + (0,)):
            for hd in (None, _dev(head)):
                tail = (mask, m, s, side, 77, hd)
                counts, score = op.similarity_rank(q, gal, n, MULT, 2, _dev(target), *tail)
                got = op.similarity_target_score(q, gal, n, MULT, 2, _dev(target), *tail)
                assert _bits(got, score)
                inside = (target >= 0) & (target < n)
                front = np.where(inside, head[np.clip(target, 0, n - 1)] if hd is not None else target, -1)
                assert torch.equal(op.similarity_count(q, gal, n, MULT, 2, got, _dev(front, torch.int32), *tail), counts)
    assert bool(torch.isneginf(got[:2]).all()) and bool((counts[:2] == 0).all())
    none = op.similarity_target_score(q, gal[:0], 0, MULT, 2, _dev(target))                    # no row: no launch
    assert bool(torch.isneginf(none).all()) and int(op.similarity_count(q, gal[:0], 0, MULT, 2, none, _dev(target, torch.int32)).sum()) == 0


# ------------------------------------------------------------------------------------------------ 3. ShardedGallery, in-process
POOL, N_Q = 8, 5
ORDERS = ((17, 0, 33, 1, 130, 16, 15), (0, 130, 15, 17, 1, 33, 16), (16, 33, 17), (1,), (0, 0))


def _world(model, g2, spans, seed, grouped=False, dual_softmax=False, products=None, side="video"):
    """(ShardedGallery over len(spans) shards, the concatenated FeatureGallery, base [S] = the first concatenated position of
    every shard, queries, labels or None): rows out of a pool of 8 distinct ones, so duplicates fall on different shards;
    grouped: runs of equal labels that never cross a shard's end.  side="video": clips in, queries = caption features
    [N_Q, 1, E]; side="text": captions in, queries = (clip features [N_Q, T, E], their mask [N_Q, 1, T])"""
    from centerclip_amd.search import FeatureGallery
    from centerclip_amd.search_sharded import ShardedGallery
    E = int(g2["s1_cfg"][0])
    assert E == 64
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    pool, seq = torch.randn(POOL, E, generator=g).to(DEV), torch.randn(N_Q, 1, E, generator=g).to(DEV)
    seq[1] = pool[3][None] * 2                                                                 # one query along a pool row
    total = int(sum(spans))
    rows = pool[torch.from_numpy(rng.integers(0, POOL, size=total)).to(DEV)]
    base = np.concatenate(([0], np.cumsum(spans)))[:-1]
    labels = None
    if grouped:
        labels = np.concatenate([1000 * (i + 1) + np.cumsum(rng.random(n) < 0.45) for i, n in enumerate(spans)] + [[]]).astype(np.int64)
    if side == "text":
        Tf = int(g2["s1_cfg"][11])
        rows, vmask = rows[:, None, :], torch.ones(N_Q, 1, Tf, dtype=torch.long, device=DEV)
        vmask[2, 0, 2:] = 0
        seq = (torch.randn(N_Q, Tf, E, generator=g).to(DEV), vmask)
    kw = dict(grouped=grouped, dual_softmax=dual_softmax, products=products, side=side)
    shards, cat = [FeatureGallery(model, capacity=4, **kw) for _ in spans], FeatureGallery(model, **kw)
    sg = ShardedGallery(shards=shards)
    if dual_softmax:
        bank = torch.randn(23, 1, E, generator=g).to(DEV)
        sg.set_query_bank_features(bank)
        cat.set_query_bank_features(bank)
    for i, (b, n) in enumerate(zip(base, spans)):
        if n:
            group = dict(group=labels[b:b + n].tolist()) if grouped else {}
            ids = sg.add_features(rows[b:b + n], shard=i, **group)
            assert ids.tolist() == [(i << 32) | p for p in range(n)]
    if total:
        cat.add_features(rows, **(dict(group=labels.tolist()) if grouped else {}))
    assert len(sg) == total == len(cat) and sg.span == cat.span
    return sg, cat, torch.from_numpy(base).to(DEV), seq, labels


def _flat(ids, base):
    """global ids -> positions of the concatenated gallery"""
    from centerclip_amd.search_sharded import ShardedGallery
    shard, local = ShardedGallery.split(ids)
    return torch.where(ids < 0, -1, base[shard.clamp(min=0)] + local)


def _gids(flat, base, spans):
    """positions of the concatenated gallery (host ints) -> global ids"""
    ends = np.cumsum(spans)
    shard = np.searchsorted(ends, np.asarray(flat), side="right")
    return [(int(s) << 32) | int(p - base[s]) for s, p in zip(shard, np.asarray(flat))]


def _same_list(got, want, base, groups=False):
    assert _bits(got[0], want[0]), "scores differ from the concatenated gallery's bits"
    assert torch.equal(_flat(got[-1], base), want[-1]), "ids differ from the concatenated gallery's order"
    if groups:
        assert torch.equal(got[1], want[1]), "labels"


def _ks(selectable):
    return sorted({1, 5, max(selectable - 1, 1), max(selectable, 1), selectable + 7, 129, 300})


@pytest.mark.parametrize("spans", ORDERS)
@pytest.mark.parametrize("products", [1, 3])
def test_search_equals_the_concatenated_gallery(g2, model, spans, products):
    sg, cat, base, seq, _ = _world(model, g2, spans, 7 + len(spans), products=products)
    for k in _ks(sum(spans)):
        _same_list(sg.search_features(seq, k=k), cat.search_features(seq, k=k), base)
    if sum(spans) == 0:
        return
    ties = cat.search_features(seq, k=min(sum(spans), 200))[0]
    assert sum(spans) < 20 or bool((ties[:, 1:] == ties[:, :-1]).any())                          # equal scores are everywhere
    # with remove, then with allow= on top of it
    rng = np.random.default_rng(sum(spans))
    gone = np.flatnonzero(rng.random(sum(spans)) < 0.3)
    if gone.size:
        sg.remove(_gids(gone, base.cpu().numpy(), spans))
        cat.remove(gone)
    assert len(sg) == len(cat) == sum(spans) - gone.size
    for k in _ks(len(cat)):
        _same_list(sg.search_features(seq, k=k), cat.search_features(seq, k=k), base)
    flags = torch.from_numpy(rng.random(sum(spans)) < 0.5).to(DEV)
    per_shard = [flags[b:b + n] for b, n in zip(base.cpu().tolist(), spans)]
    if len(spans) > 2:
        per_shard[1] = None                                                                    # a shard without a mask of its own
        flags[int(base[1]):int(base[1]) + spans[1]] = True
    left = int((flags.cpu().numpy() & cat._live).sum() if cat._live is not None else flags.sum())
    for k in _ks(left):
        _same_list(sg.search_features(seq, k=k, allow=per_shard), cat.search_features(seq, k=k, allow=flags), base)
    words = sg.row_mask(positions=_gids(np.flatnonzero(flags.cpu().numpy()), base.cpu().numpy(), spans))
    _same_list(sg.search_features(seq, k=40, allow=words), cat.search_features(seq, k=40, allow=flags), base)


@pytest.mark.parametrize("spans", ORDERS[:3])
def test_search_under_the_dual_softmax(g2, model, spans):
    sg, cat, base, seq, _ = _world(model, g2, spans, 31, dual_softmax=True)
    plain = _world(model, g2, spans, 31)[1].search_features(seq, k=5)[0]
    assert not torch.equal(plain, cat.search_features(seq, k=5)[0])                            # D, not S
    for k in _ks(sum(spans)):
        _same_list(sg.search_features(seq, k=k), cat.search_features(seq, k=k), base)
    target = np.random.default_rng(3).integers(0, sum(spans), size=N_Q)
    got = sg.rank_features(seq, _gids(target, base.cpu().numpy(), spans))
    want = cat.rank_features(seq, target.tolist())
    assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("spans", ORDERS)
def test_search_groups_equals_the_concatenated_gallery(g2, model, spans):
    sg, cat, base, seq, labels = _world(model, g2, spans, 11 + len(spans), grouped=True)
    sg.validate()
    groups = cat.num_groups
    for k in _ks(groups):
        _same_list(sg.search_groups_features(seq, k=k), cat.search_groups_features(seq, k=k), base, groups=True)
        _same_list(sg.search_features(seq, k=k), cat.search_features(seq, k=k), base)          # rows of a grouped gallery
    if groups < 4:
        return
    rng = np.random.default_rng(groups)
    gone = rng.choice(np.unique(labels), size=groups // 4, replace=False)
    sg.remove_groups(gone.tolist())
    cat.remove_groups(gone.tolist())
    flags = torch.from_numpy(rng.random(sum(spans)) < 0.5).to(DEV)
    per_shard = [flags[b:b + n] for b, n in zip(base.cpu().tolist(), spans)]
    for k in _ks(cat.num_groups):
        _same_list(sg.search_groups_features(seq, k=k), cat.search_groups_features(seq, k=k), base, groups=True)
        _same_list(sg.search_groups_features(seq, k=k, allow=per_shard), cat.search_groups_features(seq, k=k, allow=flags), base,
                   groups=True)


def test_a_caption_gallery_ranks_videos_across_shards(g2, model):
    """side="text", grouped: the multi-sentence form - clips as queries, a video's sentences as a group"""
    from centerclip_amd.search import FeatureGallery
    from centerclip_amd.search_sharded import ShardedGallery
    spans = (17, 0, 33, 16)
    sg, cat, base, (vis, vmask), labels = _world(model, g2, spans, 71, grouped=True, side="text")
    for k in _ks(cat.num_groups):
        _same_list(sg.search_groups_features(vis, k=k, mask=vmask), cat.search_groups_features(vis, k=k, mask=vmask), base, groups=True)
        _same_list(sg.search_features(vis, k=k, mask=vmask), cat.search_features(vis, k=k, mask=vmask), base)
    first = sg.search_groups_features(vis, k=6, mask=vmask)
    page = sg.search_groups_features(vis, k=9, mask=vmask, after=_last(first))
    assert all(_bits(torch.cat([a, b], 1), c) for a, b, c in zip(first, page, sg.search_groups_features(vis, k=15, mask=vmask)))
    target = np.random.default_rng(71).choice(np.unique(labels), size=N_Q).tolist()
    got, want = sg.rank_groups_features(vis, target, mask=vmask), cat.rank_groups_features(vis, target, mask=vmask)
    assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
    with pytest.raises(ValueError, match="out of scope"):                                      # its statistics run over every shard
        ShardedGallery(shards=[FeatureGallery(model, side="text", dual_softmax=True)])


# ------------------------------------------------------------------------------------------------ 4. cursors
def _last(res):
    return res[0][:, -1].contiguous(), res[-1][:, -1].contiguous()


@pytest.mark.parametrize("grouped", [False, True])
def test_cursor_pages_are_the_columns_of_one_list(g2, model, grouped):
    from centerclip_amd.search_sharded import ShardedGallery
    spans = (16, 17, 33)
    sg, cat, base, seq, _ = _world(model, g2, spans, 19, grouped=grouped)
    find = sg.search_groups_features if grouped else sg.search_features
    total = cat.num_groups if grouped else sum(spans)
    full = find(seq, k=total + 9)
    _same_list(full, (cat.search_groups_features if grouped else cat.search_features)(seq, k=total + 9), base, groups=grouped)
    assert int((full[-1] >= 0).sum(1).min()) == total
    cut_inside = set()                                                                        # shards in which a run of equal scores was cut
    shards_of_run = {}
    b = 7
    for a in list(range(1, total, 1 if grouped else 2)) + [total, total + 3]:
        first = find(seq, k=a)
        assert all(_bits(x, y[:, :a].contiguous()) for x, y in zip(first, full))
        page = find(seq, k=b, after=_last(first))
        want = [y[:, a:a + b] for y in full]
        pad = b - want[0].shape[1]
        if pad > 0:                                                                            # behind the list's end: the fill
            want = [torch.cat([w, torch.full((N_Q, pad), f, device=DEV, dtype=w.dtype)], 1) for w, f in zip(want, (float("-inf"), -1, -1))]
        assert all(_bits(x, y.contiguous()) for x, y in zip(page, want)), "a page is not the list's columns [%d, %d)" % (a, a + b)
        if a < total:
            s, i = full[0][1].cpu().numpy(), ShardedGallery.split(full[-1][1])[0].cpu().numpy()  # query 1: along a pool row
            if s[a - 1] == s[a]:
                cut_inside.add(int(i[a - 1]))
                shards_of_run.setdefault(float(s[a]), set()).update((int(i[a - 1]), int(i[a])))
    assert cut_inside == {0, 1, 2} and any(v == {0, 1, 2} for v in shards_of_run.values())
    fill = find(seq, k=5, after=(torch.full((N_Q,), float("-inf"), device=DEV), torch.full((N_Q,), -1, device=DEV)))
    assert bool(torch.isneginf(fill[0]).all()) and all(bool((x == -1).all()) for x in fill[1:])
    fill = find(seq, k=5, after=(torch.full((N_Q,), 3.0, device=DEV), torch.full((N_Q,), -1, device=DEV)))
    assert bool(torch.isneginf(fill[0]).all()) and bool((fill[-1] == -1).all())


def test_a_cursor_of_infinite_score_holds_nothing_back(g2, model):
    """(+inf, a row of shard 0): no shard behind it may lose its entries - the corner nextafter does not cover"""
    sg, cat, base, seq, _ = _world(model, g2, (5, 9, 4), 23)
    inf = torch.full((N_Q,), float("inf"), device=DEV)
    got = sg.search_features(seq, k=20, after=(inf, torch.zeros(N_Q, dtype=torch.int64, device=DEV)))
    want = cat.search_features(seq, k=20, after=(inf, torch.zeros(N_Q, dtype=torch.int64, device=DEV)))
    _same_list(got, want, base)
    assert int((got[1] >= 0).sum()) == N_Q * 18


# ------------------------------------------------------------------------------------------------ 5. rank
@pytest.mark.parametrize("spans", ORDERS[:3])
def test_rank_equals_the_concatenated_gallery(g2, model, spans):
    sg, cat, base, seq, _ = _world(model, g2, spans, 41 + len(spans))
    total, host_base = sum(spans), base.cpu().numpy()
    full = sg.search_features(seq, k=total)
    rng = np.random.default_rng(total)
    per_shard = [int(b + rng.integers(0, n)) for b, n in zip(host_base, spans) if n]            # a target in every shard
    sets = [np.resize(per_shard, N_Q), np.resize(per_shard[::-1], N_Q), rng.integers(0, total, size=N_Q),
            np.array([0, total - 1, int(host_base[-1]), int(host_base[-1]) - 1, total // 2])]
    for target in sets:
        got = sg.rank_features(seq, _gids(target, host_base, spans))
        want = cat.rank_features(seq, target.tolist())
        assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
        assert got[0].dtype == torch.int64 and got[2].dtype == torch.int32
        assert int(want[2][:, 1].min()) > 1                                                    # the targets stand among duplicates
        assert torch.equal(_flat(full[1].gather(1, got[0][:, None])[:, 0], base), _dev(target))     # the place in search(k=span)
        dev = sg.rank_features(seq, _dev(_gids(target, host_base, spans)))                     # a device tensor: passed through
        assert torch.equal(dev[2], want[2]) and _bits(dev[1], want[1])
    # duplicates in front of and behind the target's shard: equal scores on both sides were counted
    shard_of = np.searchsorted(np.cumsum(spans), sets[0], side="right")
    assert bool(((want[2][:, 2] > 0) & (want[2][:, 1] - want[2][:, 2] > 1)).any()) and len(set(shard_of.tolist())) > 1
    # a removed target and a disallowed one keep their score and are not counted
    target = sets[2]
    gone = np.unique(np.concatenate((target[:2], rng.integers(0, total, size=total // 5))))
    sg.remove(_gids(gone, host_base, spans))
    cat.remove(gone)
    flags = torch.ones(total, dtype=torch.bool, device=DEV)
    flags[_dev(target[2:4])] = False
    flags[_dev(rng.integers(0, total, size=total // 5))] = False
    per_shard = [flags[b:b + n] for b, n in zip(host_base.tolist(), spans)]
    for kw_s, kw_c in ((dict(allow=per_shard), dict(allow=flags)), (dict(), dict())):
        got = sg.rank_features(seq, _gids(target, host_base, spans), **kw_s)
        want = cat.rank_features(seq, target.tolist(), **kw_c)
        assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
        assert bool(torch.isfinite(got[1]).all())
    # ids outside every shard: (0, 0, 0) and -inf, next to a real one
    outside = [(len(spans) << 32) | 0, (0 << 32) | (spans[0] + 5), (40 << 32) | 3, -1, _gids(target[4:5], host_base, spans)[0]]
    got = sg.rank_features(seq, outside)
    assert bool((got[2][:4] == 0).all()) and bool(torch.isneginf(got[1][:4]).all()) and bool((got[0][:4] == 0).all())
    assert torch.equal(got[2][4], want[2][4]) and _bits(got[1][4:], want[1][4:])


@pytest.mark.parametrize("spans", ORDERS[:3])
def test_rank_groups_equals_the_concatenated_gallery(g2, model, spans):
    sg, cat, base, seq, labels = _world(model, g2, spans, 53 + len(spans), grouped=True)
    rng = np.random.default_rng(len(spans))
    held = np.unique(labels)
    per_shard = [int(rng.choice(held[held // 1000 == i + 1])) for i, n in enumerate(spans) if n]
    full = sg.search_groups_features(seq, k=held.size)
    flags = torch.from_numpy(rng.random(sum(spans)) < 0.6).to(DEV)
    allow = [flags[b:b + n] for b, n in zip(base.cpu().tolist(), spans)]
    for target in (np.resize(per_shard, N_Q), np.resize(per_shard[::-1], N_Q), rng.choice(held, size=N_Q)):
        got = sg.rank_groups_features(seq, target.tolist())
        want = cat.rank_groups_features(seq, target.tolist())
        assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
        assert torch.equal(full[1].gather(1, got[0][:, None])[:, 0], _dev(target))             # the place in search_groups
        got = sg.rank_groups_features(seq, target.tolist(), allow=allow)
        want = cat.rank_groups_features(seq, target.tolist(), allow=flags)
        assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
    gone = [int(target[0])]                                                                    # a removed group: scored -inf, counted over the rest
    sg.remove_groups(gone)
    cat.remove_groups(gone)
    got, want = sg.rank_groups_features(seq, target.tolist()), cat.rank_groups_features(seq, target.tolist())
    assert torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2], want[2])
    assert bool(torch.isneginf(got[1][0])) and int(got[2][0, 0]) == cat.num_groups
    nobody = sg.rank_groups_features(seq, [99, int(target[1]), -5, 99, 12345])                 # a label nobody holds
    assert bool((nobody[2][[0, 2, 3, 4]] == 0).all()) and bool(torch.isneginf(nobody[1][[0, 2, 3, 4]]).all())
    assert torch.equal(nobody[2][1], got[2][1]) and _bits(nobody[1][1:2], got[1][1:2])


# ------------------------------------------------------------------------------------------------ 6. capture
def test_merge_target_score_and_count_replay_in_a_graph(count_case):
    """one stream, no parallel branches: the three ops are recorded once and replayed on changed inputs"""
    q, gal, _ = count_case
    n, Bq, S, k = N_COUNT, BQ_COUNT, 3, 20
    lists = [_lists(seed, S, Bq, k) for seed in (1, 2)]
    targets = [np.random.default_rng(seed).integers(0, n, size=Bq).astype(np.int32) for seed in (1, 2)]
    scores, ids, target = _dev(lists[0][0]), _dev(lists[0][1]), _dev(targets[0])

    def run():
        merged = op.similarity_topk_merge(scores, ids)
        score = op.similarity_target_score(q, gal, n, MULT, 2, target)
        return merged + (score, op.similarity_count(q, gal, n, MULT, 2, score, target))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()                                                                                  # (this stream's workspace)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run()
    for i in (1, 0):
        scores.copy_(_dev(lists[i][0])), ids.copy_(_dev(lists[i][1])), target.copy_(_dev(targets[i]))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        want = run()
        assert all(_bits(a, b) for a, b in zip(got, want))
        counts, score = op.similarity_rank(q, gal, n, MULT, 2, target)
        assert torch.equal(got[4], counts) and _bits(got[3], score)
        assert np.array_equal(got[1].cpu().numpy(), merge_ref(*lists[i])[1])


def test_in_process_calls_do_not_synchronise_with_the_host(g2, model):
    """a capture fails on any synchronising call: search behind a cursor and under masks, search_groups and rank with device
    targets are recorded on one stream and replayed"""
    spans = (16, 33, 17)
    sg, cat, base, seq, _ = _world(model, g2, spans, 61, grouped=True)
    host_base = base.cpu().numpy()
    flags = torch.from_numpy(np.random.default_rng(61).random(sum(spans)) < 0.7).to(DEV)
    allow = [flags[b:b + n] for b, n in zip(host_base.tolist(), spans)]
    after = _last(sg.search_features(seq, k=9))
    ids = _dev(_gids([3, 20, 40, 60, 65], host_base, spans))

    def run():
        return (sg.search_features(seq, k=150, allow=allow, after=after) + sg.search_groups_features(seq, k=12)
                + sg.rank_features(seq, ids, allow=allow))
    want = run()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()                                                                                  # (this stream's workspace)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        got = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(got, want))
    _same_list(got[:2], cat.search_features(seq, k=150, allow=flags, after=(after[0], _flat(after[1], base))), base)


# ------------------------------------------------------------------------------------------------ 7. two ranks
def test_two_ranks_on_one_gpu_equal_the_concatenated_gallery():
    """World 2 over gloo with both ranks on cuda:0 (tests/search_sharded_worker.py): uneven shares, then rank 1 holding nothing;
    search, a cursor page, search_groups, rank, rank_groups and validate() against rank 0's concatenated FeatureGallery."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc-per-node", "2",
           os.path.join(HERE, "search_sharded_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SHARDED_WORKER_OK world=2" in r.stdout
