"""Grouped top-k search on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_topk_grouped / _grouped_dsl and
FeatureGallery(grouped=True).

Every assertion is exact.  The reference is the existing matrix op on the same rows (``_matrix``: scaled_dot_planes on a
zero-padded copy), followed by ``dsl_apply_`` for the dual softmax, then ``grouped_topk_ref`` of
tests/test_search_grouped_host.py (stable descending order, first occurrence of every group, first k, fill): ids equal,
scores bit-equal, the fill (-inf, -1) exact.  E = 64 unless a test says otherwise; galleries carry non-zero rows and valid
looking heads behind n, which must not appear."""
import io

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from test_search_grouped_host import grouped_topk_ref
from test_search_gpu import (BATCHES, DEV, MULT, N_CLIPS, _bits, _dataset, _eval_model, _matrix, _planes, _split, _state,
                             g2)  # noqa: F401  (g2: the fixture)

pytestmark = pytest.mark.gpu
op = torch.ops.centerclip
BEHIND = 37
PATTERN = (1, 15, 16, 17, 40, 65)                                         # group sizes around the 16-row tile


def _heads(sizes, n, behind=BEHIND):
    """group_head of n rows cut into groups of the cycling `sizes` (the last one cut short), then `behind` singleton heads"""
    out, at, i = [], 0, 0
    while at < n:
        size = min(int(sizes[i % len(sizes)]), n - at)
        out += [at] * size
        at += size
        i += 1
    return np.array(out + list(range(n, n + behind)), dtype=np.int32)


def _dev(head):
    return torch.from_numpy(np.ascontiguousarray(head)).to(DEV)


def _randn_planes(seed, Bq, rows, E, text_queries=True):
    g = torch.Generator().manual_seed(seed)
    return _planes(torch.randn(Bq, E, generator=g), not text_queries), _planes(torch.randn(rows, E, generator=g), text_queries)


def _assert_grouped(scores, ids, S, head, k):
    """scores / ids [Bq, k] against the matrix S [Bq, n] and the groups head [n]"""
    Sn = S.cpu().numpy() if torch.is_tensor(S) else S
    want_scores, want_ids = grouped_topk_ref(Sn, head[:Sn.shape[1]], k)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and tuple(ids.shape) == tuple(scores.shape) == (Sn.shape[0], k)
    assert np.array_equal(ids.cpu().numpy(), want_ids), "ids differ from the first rows of their groups in the stable order"
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want_scores.view(np.uint32)), "scores are not the matrix op's bits"


def _check(q, gal, n, products, k, head, S=None, mult=MULT):
    S = _matrix(q, gal, n, mult, products) if S is None else S
    scores, ids = op.similarity_topk_grouped(q, gal, n, mult, products, k, _dev(head))
    _assert_grouped(scores, ids, S, head, k)
    return scores, ids, S


# ------------------------------------------------------------------------------------------------ 1. shapes of groups
@pytest.mark.parametrize("n", [1, 17, 4099])
@pytest.mark.parametrize("Bq", [1, 17])
def test_singleton_groups_are_the_plain_op_bit_for_bit(n, Bq):
    q, gal = _randn_planes(1000 * Bq + n, Bq, n + BEHIND, 64)
    head = np.arange(n + BEHIND, dtype=np.int32)
    S = _matrix(q, gal, n, MULT, 2)
    for k in (1, 10, 128):
        scores, ids, _ = _check(q, gal, n, 2, k, head, S)
        plain = op.similarity_topk(q, gal, n, MULT, 2, k)
        assert torch.equal(ids, plain[1]) and _bits(scores, plain[0]), k


@pytest.mark.parametrize("n", [255, 257, 4099])
def test_group_sizes_around_the_tile(n):
    if n == 4099:                                                          # range boundaries fall inside groups before snapping
        assert L.lib().cc_similarity_topk_slices(17, n, 10) == 8
    q, gal = _randn_planes(n, 17, n + BEHIND, 64)
    head = _heads(PATTERN, n)
    S = _matrix(q, gal, n, MULT, 3)
    for k in (1, 10, 128):
        _check(q, gal, n, 3, k, head, S)


@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_one_group_larger_than_any_ranges_share(where):
    n, big = 4099, 3000
    at = {"start": 0, "middle": 547, "end": n - big}[where]
    head = np.concatenate([_heads(PATTERN, at, behind=0), np.full(big, at, dtype=np.int32),
                           at + big + _heads(PATTERN, n - at - big)]).astype(np.int32)
    assert head.shape == (n + BEHIND,) and (head[:n] <= np.arange(n)).all() and (np.diff(head[:n]) >= 0).all()
    assert (head[head[:n]] == head[:n]).all() and int((head[:n] == at).sum()) == big
    q, gal = _randn_planes(77 + at, 5, n + BEHIND, 64)
    S = _matrix(q, gal, n, MULT, 2)
    for k in (10, 128):
        _check(q, gal, n, 2, k, head, S)


def test_all_rows_in_one_group():
    n = 4099
    q, gal = _randn_planes(3, 17, n + BEHIND, 64)
    head = np.concatenate([np.zeros(n, dtype=np.int32), np.arange(n, n + BEHIND, dtype=np.int32)])
    for k in (1, 10):
        scores, ids, S = _check(q, gal, n, 2, k, head)
        assert torch.equal(ids[:, 0], S.argmax(dim=1)) and bool((ids[:, 1:] == -1).all()) and bool(torch.isneginf(scores[:, 1:]).all())


def test_fewer_groups_than_k():
    n = 300
    head = _heads((1, 15, 16, 17, 40, 65, 146), n)
    assert len(np.unique(head[:n])) == 7
    q, gal = _randn_planes(4, 5, n + BEHIND, 64)
    for k in (10, 128):
        scores, ids, _ = _check(q, gal, n, 2, k, head)
        assert bool((ids[:, :7] >= 0).all()) and bool((ids[:, 7:] == -1).all()) and bool(torch.isneginf(scores[:, 7:]).all())


def test_rows_and_heads_behind_n_do_not_appear():
    n, Bq = 1000, 3
    g = torch.Generator().manual_seed(5)
    queries, rows = torch.randn(Bq, 64, generator=g), torch.randn(n + BEHIND, 64, generator=g)
    rows[n:n + Bq] = queries                                               # the best rows there could be, behind n
    q, gal = _planes(queries, False), _planes(rows, True)
    head = _heads(PATTERN, n)
    head[n:] = np.arange(n, n + BEHIND) // 2                               # heads behind n that would reach into the rows held
    scores, ids, _ = _check(q, gal, n, 2, 128, head)
    assert int(ids.max()) < n


# ------------------------------------------------------------------------------------------------ 2. ties
def test_identical_rows_in_groups_of_three_come_by_their_first_row():
    n = 4099
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(5, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(n, 64), True)
    head = _heads((3,), n, behind=0)
    for k in (10, 128):
        _, ids, _ = _check(q, gal, n, 2, k, head)
        assert torch.equal(ids.cpu(), (3 * torch.arange(k)).expand(5, k))


def test_the_best_row_duplicated_once_in_every_group():
    n, Bq = 4099, 3
    q, gal = _randn_planes(12, Bq, n, 64)
    head = _heads(PATTERN, n, behind=0)
    starts = np.unique(head)
    best = int(_matrix(q, gal, n, MULT, 3)[0].argmax())
    at = sorted({int(s) + (int(e) - int(s)) // 2 for s, e in zip(starts, list(starts[1:]) + [n])})      # the middle of every group
    gal[at] = gal[best].clone()
    _, ids, S = _check(q, gal, n, 3, 128, head)
    got = ids[0].tolist()                                                  # equal scores: one row a group, ascending ids
    assert len(set(S[0, at].tolist())) == 1 and len(set(S[0, got].tolist())) == 1 and got == sorted(got)
    assert got[0] <= at[0] and len(set(head[got].tolist())) == 128


def test_seven_distinct_rows_repeated():
    n = 4099
    g = torch.Generator().manual_seed(13)
    base = torch.randn(7, 64, generator=g)
    pick = torch.from_numpy(np.random.default_rng(13).integers(0, 7, size=n))
    q = _planes(torch.randn(17, 64, generator=g), False)
    gal = _planes(base[pick], True)
    head = _heads(PATTERN, n, behind=0)
    for k, products in ((1, 1), (65, 2), (128, 3)):
        _check(q, gal, n, products, k, head)


def test_the_same_groups_at_other_row_offsets():
    """1..16 singleton rows in front move every group against the tiles and the planned boundaries: the same groups, the same
    scores"""
    n, Bq, k = 4099, 5, 10
    g = torch.Generator().manual_seed(21)
    queries, rows, extra = torch.randn(Bq, 64, generator=g), torch.randn(n, 64, generator=g), torch.randn(16, 64, generator=g)
    q = _planes(queries, False)
    head = _heads(PATTERN, n, behind=0)
    base_scores, base_ids, _ = _check(q, _planes(rows, True), n, 2, k, head)
    for off in range(1, 17):
        gal = _planes(torch.cat([extra[:off], rows]), True)
        moved = np.concatenate([np.arange(off, dtype=np.int32), head + off]).astype(np.int32)
        scores, ids, _ = _check(q, gal, n + off, 2, k + off, moved)
        for r in range(Bq):                                                # without the rows in front: the first k are the base's
            keep = ids[r] >= off
            assert torch.equal(ids[r][keep][:k] - off, base_ids[r]) and _bits(scores[r][keep][:k], base_scores[r]), (off, r)


# ------------------------------------------------------------------------------------------------ 3. wide rows, many rows
@pytest.mark.parametrize("E,Bq,n,k,products", [(512, 16, 3001, 100, 2), (768, 7, 2000, 128, 3)])
def test_wide_rows(E, Bq, n, k, products):
    q, gal = _randn_planes(E + n, Bq, n + 5, E)
    _check(q, gal, n, products, k, _heads(PATTERN, n, behind=5))


def test_many_slices():
    Bq, n, k = 16, 200003, 10
    g = torch.Generator(device=DEV).manual_seed(14)
    gal = op.normalize_rows_planes(torch.randn(n + 5, 64, device=DEV, generator=g), True)
    q = op.normalize_rows_planes(torch.randn(Bq, 64, device=DEV, generator=g), False)
    head = _heads(np.random.default_rng(14).integers(1, 41, size=997), n, behind=5)
    _check(q, gal, n, 2, k, head)


# ------------------------------------------------------------------------------------------------ 4. dual softmax
@pytest.mark.parametrize("Bq,n", [(33, 1000), (5, 4099)])
@pytest.mark.parametrize("side", [0, 1])
def test_dual_softmax(Bq, n, side):
    """side 1: text queries, a clip gallery, statistics per gallery row over the queries; side 0: clip queries, a caption
    gallery, statistics per query row over the gallery - both from dsl_col_stats_planes"""
    q, gal = _randn_planes(100 * Bq + n + side, Bq, n + BEHIND, 64, text_queries=bool(side))
    head, k, products = _heads(PATTERN, n), 10, 2
    if side:
        S_tv = _matrix(q, gal, n, MULT, products)                                          # [Bq texts, n videos]
        m, s = op.dsl_col_stats_planes(q, gal, Bq, n, MULT, products)
        nt = Bq
    else:
        S_tv = _matrix(gal[:n].contiguous(), q, Bq, MULT, products)                        # [n texts, Bq videos]
        m, s = op.dsl_col_stats_planes(gal, q, n, Bq, MULT, products)
        nt = n
    D = S_tv.clone()
    op.dsl_apply_(D, m, s, nt)
    D_qg = D if side else D.t().contiguous()
    if side:                                                                               # statistics behind n: never read
        m, s = (torch.cat([t, torch.full((BEHIND,), float("nan"), device=DEV)]) for t in (m, s))
    for kk in (k, 128):
        scores, ids = op.similarity_topk_grouped_dsl(q, gal, n, MULT, products, kk, m, s, side, nt, _dev(head))
        _assert_grouped(scores, ids, D_qg, head, kk)
    plain = op.similarity_topk_dsl(q, gal, n, MULT, products, k, m, s, side, nt)           # singletons: the plain op's bits
    scores, ids = op.similarity_topk_grouped_dsl(q, gal, n, MULT, products, k, m, s, side, nt,
                                                 torch.arange(n + BEHIND, device=DEV, dtype=torch.int32))
    assert torch.equal(ids, plain[1]) and _bits(scores, plain[0])


# ------------------------------------------------------------------------------------------------ 5. capture; malformed heads
def test_graph_capture_and_replay():
    Bq, n, k = 5, 4099, 10
    q, gal = _randn_planes(15, Bq, n, 64)
    q2, _ = _randn_planes(16, Bq, 1, 64)
    head = _heads(PATTERN, n, behind=0)
    hd, qbuf = _dev(head), q.clone()
    op.similarity_topk_grouped(qbuf, gal, n, MULT, 2, k, hd)              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, ids = op.similarity_topk_grouped(qbuf, gal, n, MULT, 2, k, hd)
    for new in (q2, q):
        qbuf.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want_scores, want_ids = op.similarity_topk_grouped(new, gal, n, MULT, 2, k, hd)
        assert torch.equal(ids, want_ids) and _bits(scores, want_scores)
        _assert_grouped(scores, ids, _matrix(new, gal, n, MULT, 2), head, k)


def test_a_malformed_group_head_stays_inside_the_rows():
    """decreasing heads, and heads above their row (all below n): the ranking is unspecified, the call returns"""
    n, Bq, k = 4099, 5, 10
    q, gal = _randn_planes(31, Bq, n, 64)
    rows = np.arange(n)
    for head in (rows[::-1], np.minimum(rows + 5, n - 1), np.minimum(rows * 3, n - 1)):
        assert head.min() >= 0 and head.max() < n
        scores, ids = op.similarity_topk_grouped(q, gal, n, MULT, 2, k, _dev(head.astype(np.int32)))
        torch.cuda.synchronize()
        assert tuple(scores.shape) == tuple(ids.shape) == (Bq, k) and scores.dtype == torch.float32 and ids.dtype == torch.int64


# ------------------------------------------------------------------------------------------------ 6. FeatureGallery
LABELS = (30, 30, 30, 11, 52, 52, 52, 52, 3, 3, 74, 74)                    # 5 groups of the 12 clips; BATCHES (5, 3, 4) split two


def _label_batches():
    return [list(b) for b in torch.split(torch.tensor(LABELS), list(BATCHES))]


def _assert_groups(result, M, labels, k):
    """(scores, labels, positions) of search_groups against the gallery's own matrix M [Nq, n]"""
    scores, groups, pos = result
    _assert_grouped(scores, pos, M, np.asarray(labels), k)
    want = np.where(pos.cpu().numpy() >= 0, np.asarray(labels, dtype=np.int64)[pos.cpu().numpy().clip(min=0)], -1)
    assert groups.dtype == torch.int64 and np.array_equal(groups.cpu().numpy(), want)


@pytest.mark.parametrize("cluster_inter,dual_softmax", [(0, False), (1, False), (0, True), (1, True)])
def test_feature_gallery_grouped_on_the_small_model(g2, cluster_inter, dual_softmax):
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, cluster_inter)
    video, vmask, ids = _dataset(g2["s1_cfg"])
    n = N_CLIPS
    # side="video": windows of 5 long videos, captions ask
    gal = FeatureGallery(model, capacity=4, dual_softmax=dual_softmax, grouped=True)
    if dual_softmax:
        gal.set_query_bank(ids)
    s0, g0, p0 = gal.search_groups(ids[:2], k=3)                           # an empty gallery: the fill alone
    assert bool((g0 == -1).all()) and bool((p0 == -1).all()) and bool(torch.isneginf(s0).all()) and gal.num_groups == 0
    with pytest.raises(ValueError, match="group="):
        gal.add(video[:1], vmask[:1])
    pos = [gal.add(v, m, group=lab) for v, m, lab in zip(_split(video), _split(vmask), _label_batches())]
    assert torch.equal(torch.cat(pos), torch.arange(n)) and len(gal) == n and gal.num_groups == 5
    assert gal._head[:n].tolist() == [0, 0, 0, 3, 4, 4, 4, 4, 8, 8, 10, 10] and gal.labels.tolist() == list(LABELS)
    with pytest.raises(ValueError, match="returns"):
        gal.add(video[:1], vmask[:1], group=30)
    assert len(gal) == n
    M = gal.similarity(ids)
    for k in (1, 3, 5, 20):                                                # 20 > 5 groups: the fill
        res = gal.search_groups(ids, k=k)
        _assert_groups(res, M, LABELS, k)
    with torch.no_grad():
        seq = model(input_ids=ids)['sequence_output']
    res2 = gal.search_groups_features(seq, k=5)
    assert all(_bits(a, b) for a, b in zip(res, gal.search_groups(ids, k=20))) and _bits(res2[0], res[0][:, :5])
    rows_scores, rows_ids = gal.search(ids, k=5)                           # search keeps ranking rows
    order = np.argsort(-M.cpu().numpy(), axis=1, kind="stable")[:, :5]
    assert np.array_equal(rows_ids.cpu().numpy(), order)
    # side="text": the sentences of 5 videos, clips ask; other batches
    tg = FeatureGallery(model, side="text", dual_softmax=dual_softmax, grouped=True)
    tg.add(ids[:7], group=torch.tensor(LABELS[:7]))
    tg.add(ids[7:8], group=LABELS[7])
    tg.add(ids[8:], group=np.array(LABELS[8:]))
    assert tg.num_groups == 5 and torch.equal(tg._head[:n], gal._head[:n])
    Mt = tg.similarity(video, vmask)
    for k in (2, 7):
        _assert_groups(tg.search_groups(video, vmask, k=k), Mt, LABELS, k)
    # save / load
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    fresh = FeatureGallery(model, products=3, dual_softmax=dual_softmax, grouped=True)
    fresh.load_state_dict(torch.load(buf))
    assert len(fresh) == n and fresh.num_groups == 5 and _bits(fresh.rows, gal.rows) and torch.equal(fresh._head[:n], gal._head[:n])
    assert fresh.labels.tolist() == list(LABELS)
    assert all(_bits(a, b) for a, b in zip(fresh.search_groups(ids, k=4), gal.search_groups(ids, k=4)))
    with pytest.raises(ValueError, match="returns"):
        fresh.add(video[:1], vmask[:1], group=3)
    plain = FeatureGallery(model, dual_softmax=dual_softmax)
    with pytest.raises(ValueError, match="grouped"):
        plain.load_state_dict(gal.state_dict())
    with pytest.raises(ValueError, match="grouped=True"):
        plain.search_groups(ids)
    gal.clear()
    assert len(gal) == 0 and gal.num_groups == 0
    gal.add(video[:2], vmask[:2], group=30)                                # a cleared gallery takes its labels again
    assert gal.num_groups == 1


def test_feature_gallery_grouped_runs_the_seqtransf_head(g2):
    """tests/test_search_gpu.py's seqTransf model (embed_dim = transformer_width = 128)"""
    from centerclip_amd.search import FeatureGallery
    sd = _state(g2)
    g = torch.Generator().manual_seed(5)
    sd["text_projection"] = torch.randn(128, 128, generator=g) * 0.05
    sd["visual.proj"] = torch.randn(sd["visual.proj"].shape[0], 128, generator=g) * 0.05
    model = _eval_model(g2, 0, sd=sd, sim_header='seqTransf', cross_num_hidden_layers=2)
    Tf = int(g2["s1_cfg"][11])
    vis = torch.randn(9, Tf, 128, generator=g).to(DEV)
    mask = torch.ones(9, 1, Tf, dtype=torch.long, device=DEV)
    mask[2, 0, 2:] = 0
    labels = [4, 4, 4, 4, 1, 8, 8, 8, 0]
    gal = FeatureGallery(model, grouped=True)
    gal.add_features(vis[:6], mask[:6], group=labels[:6])
    gal.add_features(vis[6:], mask[6:], group=labels[6:])
    seq = torch.randn(3, 1, 128, generator=g).to(DEV)
    for k in (2, 6):
        _assert_groups(gal.search_groups_features(seq, k=k), gal.similarity_features(seq), labels, k)


@pytest.mark.parametrize("dual_softmax", [False, True])
def test_multi_sentence_video_to_text_parity(g2, dual_softmax):
    """A caption gallery labelled by video: search_groups_features(visual, k=num_groups) is row v of
    metrics.tensor_video_to_text_sim on the gallery's own similarity_features matrix arranged [G, Lmax, C] with -inf padding -
    what eval_epoch ranks video->text on the multi-sentence sets."""
    from centerclip_amd import metrics
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, 0)
    E, Tf = int(g2["s1_cfg"][0]), int(g2["s1_cfg"][11])
    sizes = [1, 2, 20, 70, 3, 16, 17, 1, 33, 5]
    G, n, C = len(sizes), sum(sizes), 6
    g = torch.Generator().manual_seed(9)
    seq = torch.randn(n, 1, E, generator=g).to(DEV)
    visual = torch.randn(C, Tf, E, generator=g).to(DEV)
    vmask = torch.ones(C, 1, Tf, dtype=torch.long, device=DEV)
    vmask[1, 0, Tf - 1:] = 0
    labels = np.repeat(np.arange(G), sizes)
    gal = FeatureGallery(model, side="text", dual_softmax=dual_softmax, grouped=True)
    for a, b in ((0, 40), (40, 41), (41, 120), (120, n)):                  # uneven batches that split groups
        gal.add_features(seq[a:b], group=labels[a:b])
    assert gal.num_groups == G
    M = gal.similarity_features(visual, mask=vmask)                        # [C, n]: S^T, or D^T under the dual softmax
    starts = np.concatenate(([0], np.cumsum(sizes)))
    sim_tensor = torch.full((G, max(sizes), C), float("-inf"), device=DEV)
    for i in range(G):
        sim_tensor[i, :sizes[i]] = M[:, starts[i]:starts[i + 1]].t()
    v2t = metrics.tensor_video_to_text_sim(sim_tensor)                     # [C, G]
    assert tuple(v2t.shape) == (C, G)
    scores, groups, pos = gal.search_groups_features(visual, k=G, mask=vmask)
    _assert_groups((scores, groups, pos), M, labels, G)
    v2t_n = v2t.cpu().numpy()
    order = np.argsort(-v2t_n, axis=1, kind="stable")                      # (groups in row order: ties to the smaller best position)
    assert np.array_equal(groups.cpu().numpy(), order)
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), np.take_along_axis(v2t_n, order, 1).view(np.uint32))
    assert np.array_equal(np.sort(scores.cpu().numpy(), axis=1), np.sort(v2t_n, axis=1))
