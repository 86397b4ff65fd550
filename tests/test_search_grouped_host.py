"""Grouped top-k search without a GPU: the NumPy reference ranking every GPU check compares against (pinned on a hand-written
example), every early return of cc_similarity_topk_grouped_planes_f32 / cc_similarity_topk_grouped_dsl_planes_f32 and their
order (the checks end before anything is read or launched, so never-dereferenced addresses do), the workspace query, the
ops' fake kernels and ValueErrors, and FeatureGallery(grouped=True)'s refusals and label bookkeeping on a stub."""
import ctypes

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_host import _cpu_model

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def grouped_topk_ref(S, group, k):
    """The reference ranking.  S [Nq, n] scores, group [n] one label per row (group_head itself is one) ->
    (scores [Nq, k] of S's dtype, ids [Nq, k] int64): 1. the matrix, 2. its stable descending order per row, 3. the first
    occurrence of every group in that order, 4. the first k of those, then the fill (-inf, -1)."""
    S, group = np.asarray(S), np.asarray(group)
    assert S.ndim == 2 and group.shape == (S.shape[1],)
    order = np.argsort(-S, axis=1, kind="stable")
    scores = np.full((S.shape[0], k), -np.inf, dtype=S.dtype)
    ids = np.full((S.shape[0], k), -1, dtype=np.int64)
    for q in range(S.shape[0]):
        _, first = np.unique(group[order[q]], return_index=True)
        keep = order[q][np.sort(first)][:k]
        ids[q, :len(keep)] = keep
        scores[q, :len(keep)] = S[q, keep]
    return scores, ids


def test_the_reference_ranking_on_a_hand_written_example():
    head = np.array([0, 0, 0, 3, 4, 4, 6, 6, 6])                           # groups of 3, 1, 2, 3 rows
    S = np.array([[1, 5, 5, 2, 5, 3, 0, -0.0, 4],
                  [-1, -1, -1, 7, -3, -2, 7, 7, 9]], dtype=np.float32)
    # row 0: order 1 2 4 8 5 3 0 6 7 -> first of their group: 1 (rows 1 and 2 tie: the smaller), 4 (ties with group 0: the
    #        smaller best row first), 8, 3.   row 1: order 8 3 6 7 0 1 2 5 4 -> 8, 3 (7 ties with rows 6, 7 of the group
    #        that already appeared), 0 (of three equal rows), 5
    inf = np.float32("-inf")
    scores, ids = grouped_topk_ref(S, head, 3)
    assert ids.tolist() == [[1, 4, 8], [8, 3, 0]] and scores.tolist() == [[5, 5, 4], [9, 7, -1]]
    scores, ids = grouped_topk_ref(S, head, 6)
    assert ids.tolist() == [[1, 4, 8, 3, -1, -1], [8, 3, 0, 5, -1, -1]]
    assert scores.tolist() == [[5, 5, 4, 2, inf, inf], [9, 7, -1, -2, inf, inf]] and scores.dtype == np.float32
    scores, ids = grouped_topk_ref(S, head, 1)
    assert ids.tolist() == [[1], [8]]
    # labels instead of heads: the same groups; singletons: the plain stable order; -0 == +0 (row 6 before row 7)
    assert np.array_equal(grouped_topk_ref(S, np.array([7, 7, 7, 2, 9, 9, 4, 4, 4]), 6)[1], grouped_topk_ref(S, head, 6)[1])
    scores, ids = grouped_topk_ref(S, np.arange(9), 9)
    assert ids.tolist() == [[1, 2, 4, 8, 5, 3, 0, 6, 7], [8, 3, 6, 7, 0, 1, 2, 5, 4]]
    assert np.signbit(scores[0, 8]) and not np.signbit(scores[0, 7])
    one = grouped_topk_ref(S, np.zeros(9, dtype=np.int64), 2)                  # all rows in one group
    assert one[1].tolist() == [[1, -1], [8, -1]] and one[0].tolist() == [[5, inf], [9, inf]]


# ------------------------------------------------------------------------------------------------ the library
def _p(v):
    return ctypes.c_void_p(v) if v else None                               # (addresses that are never dereferenced)


def _plain(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=10, head=256, scores=256, ids=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
    return lib.cc_similarity_topk_grouped_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, k, _p(head), _p(scores), _p(ids),
                                                     _p(ws), ws_bytes, None)


def _dsl(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=10, m=256, s=256, side=1, n_total=100, head=256, scores=256,
         ids=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
    return lib.cc_similarity_topk_grouped_dsl_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, k, _p(m), _p(s), side, n_total,
                                                         _p(head), _p(scores), _p(ids), _p(ws), ws_bytes, None)


@pytest.mark.parametrize("call,own_nulls,own_invalid", [
    (_plain, ("head",), ()),
    (_dsl, ("head", "m", "s"), (dict(n_total=-1), dict(side=2), dict(side=-1)))])
def test_entries_refuse_before_touching_memory_in_the_plain_entrys_order(call, own_nulls, own_invalid):
    lib = L.lib()
    for null in ("q", "g", "scores", "ids") + own_nulls:
        assert call(lib, **{null: 0}) == INVALID, null
    for kw in (dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(Bg=-5), dict(E=-64)) + own_invalid:
        assert call(lib, **kw) == INVALID, kw
    for kw in (dict(k=0), dict(k=129), dict(k=-3), dict(products=0), dict(products=4), dict(E=96), dict(E=1088),
               dict(E=1024, products=3, k=128), dict(Bq=16 * 65535 + 1)):
        assert call(lib, **kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_topk_workspace_bytes(4, 100, 10)
    assert need > 0
    assert call(lib, ws_bytes=need - 1) == WORKSPACE
    assert call(lib, ws=0) == WORKSPACE
    # the order: invalid (a NULL group_head included) before unsupported before the workspace
    assert call(lib, head=0, k=129, ws=0) == INVALID
    assert call(lib, head=0, E=96, ws_bytes=0) == INVALID
    assert call(lib, k=129, ws=0) == UNSUPPORTED
    assert call(lib, E=1024, products=3, k=128, ws=0) == UNSUPPORTED
    # the neighbours of the one excluded combination, and the most query rows, pass the limits and stop at the workspace
    for kw in (dict(E=1024, products=3, k=127), dict(E=1024, products=2, k=128), dict(E=768, products=3, k=128),
               dict(Bq=16 * 65535)):
        assert call(lib, ws_bytes=0, **kw) == WORKSPACE, kw


def test_the_workspace_is_the_plain_ops():
    """one query for all four entries: Bq * slices * k keys of 8 bytes, nothing of size Bq * Bg"""
    lib = L.lib()
    for Bq, Bg, k in ((1, 1, 1), (16, 4099, 10), (17, 4099, 128), (16, 200003, 10), (16, 1 << 20, 128)):
        w = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
        slices = lib.cc_similarity_topk_slices(Bq, Bg, k)
        assert Bq * slices * k * 8 <= w < Bq * slices * k * 8 + 256
        assert _plain(lib, Bq=Bq, Bg=Bg, k=k, ws_bytes=w - 1) == WORKSPACE
        assert _dsl(lib, Bq=Bq, Bg=Bg, k=k, ws_bytes=w - 1) == WORKSPACE
    assert lib.cc_similarity_topk_slices(16, 4099, 10) == 8                # (the GPU tests' several-slices shape)
    assert lib.cc_similarity_topk_workspace_bytes(16, 200000, 10) < 16 * 200000 * 4 // 16


# ------------------------------------------------------------------------------------------------ the ops
def _meta(n, E3=192, dtype=torch.float16):
    return torch.empty(n, E3, device="meta", dtype=dtype)


def test_fake_kernels_give_shapes_on_the_meta_device():
    assert "similarity_topk_grouped" in torch_ops.OPS and "similarity_topk_grouped_dsl" in torch_ops.OPS
    op = torch.ops.centerclip
    q, g = _meta(40), _meta(1000)
    head = torch.empty(1000, device="meta", dtype=torch.int32)
    stat = torch.empty(1000, device="meta")
    for scores, ids in (op.similarity_topk_grouped(q, g, 900, 20.0, 2, 17, head),
                        op.similarity_topk_grouped_dsl(q, g, 900, 20.0, 2, 17, stat, stat, 1, 900, head),
                        op.similarity_topk_grouped_dsl(q, g, 900, 20.0, 2, 17, stat[:40], stat[:40], 0, 900, head)):
        assert scores.shape == (40, 17) and scores.dtype == torch.float32 and scores.device.type == "meta"
        assert ids.shape == (40, 17) and ids.dtype == torch.int64
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        op.similarity_topk_grouped(h(2), h(8), 8, 1.0, 2, 3, torch.arange(8, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        op.similarity_topk_grouped_dsl(h(2), h(8), 8, 1.0, 2, 3, torch.zeros(8), torch.ones(8), 1, 8,
                                       torch.arange(8, dtype=torch.int32))


def test_ops_refuse_planes_and_heads_that_do_not_fit():
    op = torch.ops.centerclip
    q, g = _meta(4), _meta(100)
    head = torch.empty(100, device="meta", dtype=torch.int32)
    stat = torch.empty(100, device="meta")
    plain = lambda q=q, g=g, n=100, head=head: op.similarity_topk_grouped(q, g, n, 1.0, 2, 5, head)
    dsl = lambda q=q, g=g, n=100, head=head, m=stat, s=stat, side=1: op.similarity_topk_grouped_dsl(q, g, n, 1.0, 2, 5, m, s, side,
                                                                                                  100, head)
    for call in (plain, dsl):
        call()
        bad = [dict(head=torch.empty(100, device="meta", dtype=torch.int64)),            # not int32
               dict(head=torch.empty(200, device="meta", dtype=torch.int32)[::2]),        # not contiguous
               dict(head=torch.empty(99, device="meta", dtype=torch.int32)),              # fewer than n_gallery entries
               dict(head=torch.empty(100, 1, device="meta", dtype=torch.int32)),          # not a vector
               dict(head=torch.zeros(100, dtype=torch.int32)),                            # not on the planes' device
               dict(n=101),                                                               # more rows than the planes hold
               dict(g=_meta(100, 384)),                                                   # rows of another width
               dict(g=_meta(100, dtype=torch.float32)), dict(q=_meta(4, dtype=torch.bfloat16))]
        for kw in bad:
            with pytest.raises(ValueError):
                call(**kw)
    for kw in (dict(m=torch.empty(99, device="meta")), dict(s=torch.empty(100, device="meta", dtype=torch.float64)),
               dict(m=torch.empty(100, 1, device="meta")), dict(side=0, m=stat[:3], s=stat[:3])):
        with pytest.raises(ValueError):
            dsl(**kw)
    dsl(side=0, m=stat[:4], s=stat[:4])                                    # query-side statistics: one pair per query row


# ------------------------------------------------------------------------------------------------ FeatureGallery
def _bare(model, side="video", dual_softmax=False, grouped=False):
    """a gallery as the constructor leaves it, minus the device"""
    import centerclip_amd.search as S
    gal = S.FeatureGallery.__new__(S.FeatureGallery)
    gal.model = gal.core = model
    gal.side, gal.products, gal.E, gal._n = side, 2, 64, 0
    gal.device, gal.backend = torch.device("cpu"), S.HipBackend
    gal._rows = torch.zeros(0, 192, dtype=torch.float16)
    if dual_softmax:
        gal.dual_softmax, gal._bank, gal._m, gal._s = True, None, torch.zeros(0), torch.zeros(0)
    if grouped:
        gal.grouped = True
        gal._head, gal._label_dev = torch.zeros(0, dtype=torch.int32), torch.full((1,), -1, dtype=torch.int64)
        gal._reset_groups()
    return gal


@pytest.fixture(scope="module")
def model():
    return _cpu_model()


def test_feature_gallery_grouped_refusals(model):
    from centerclip_amd.search import FeatureGallery
    for kw in (dict(), dict(side="text"), dict(dual_softmax=True), dict(side="text", dual_softmax=True)):
        with pytest.raises(L.CenterClipHipError):                          # accepted on both sides, with and without - on a device
            FeatureGallery(model, grouped=True, **kw)
    ids, seq = torch.zeros(2, 16, dtype=torch.long), torch.zeros(2, 1, 64)
    vis, vmask = torch.zeros(2, 4, 64), torch.ones(2, 4, dtype=torch.long)
    for dual_softmax in (False, True):
        gal, plain = _bare(model, "text", dual_softmax, True), _bare(model, "text", dual_softmax)
        with pytest.raises(ValueError, match="group="):                    # a grouped gallery wants labels ...
            gal.add(ids)
        with pytest.raises(ValueError, match="group="):
            gal.add_features(seq)
        with pytest.raises(ValueError, match="grouped=True"):              # ... a plain one refuses them
            plain.add(ids, group=3)
        with pytest.raises(ValueError, match="grouped=True"):
            plain.add_features(seq, group=[0, 1])
        for bad in (torch.zeros(2, dtype=torch.long, device="meta"), torch.zeros(2, dtype=torch.int32)):
            with pytest.raises(ValueError, match="CPU LongTensor"):        # no device tensor (it would have to be read)
                gal.add(ids, group=bad)
            with pytest.raises(ValueError, match="CPU LongTensor"):
                gal.add_features(seq, group=bad)
        with pytest.raises(ValueError, match="grouped=True"):              # only a grouped gallery ranks groups
            plain.search_groups(vis, vmask)
        with pytest.raises(ValueError, match="grouped=True"):
            plain.search_groups_features(vis, mask=vmask)
        with pytest.raises(ValueError):
            plain.num_groups
        with pytest.raises(L.CenterClipHipError):                          # labels in order: CPU tensors are refused next
            gal.add(ids, group=3)
        with pytest.raises(L.CenterClipHipError):
            gal.add_features(seq, group=torch.tensor([0, 1]))
        with pytest.raises(L.CenterClipHipError):
            gal.search_groups_features(vis, mask=vmask)
        assert len(gal) == 0 and gal.num_groups == 0 and len(plain) == 0


def test_label_bookkeeping_across_add_calls(model):
    gal = _bare(model, "text", grouped=True)
    rows = lambda n: torch.ones(n, 192, dtype=torch.float16)
    assert gal._append(rows(2), 7).tolist() == [0, 1]                      # an int: the whole batch
    assert gal.num_groups == 1
    gal._append(rows(3), [7, 7, 4])                                        # a sequence; the group of 7 continues
    assert gal.num_groups == 2 and gal._head.tolist() == [0, 0, 0, 0, 4]
    gal._append(rows(4), torch.tensor([4, 9, 9, -5]))                      # a CPU LongTensor; any int64 is a label
    assert gal.num_groups == 4 and len(gal) == 9
    gal._append(rows(0), [])
    gal._append(rows(1), np.int64(-5))
    assert gal._head.tolist() == [0, 0, 0, 0, 4, 4, 6, 6, 8, 8] and gal._head.dtype == torch.int32
    assert gal.labels.tolist() == [7, 7, 7, 7, 4, 4, 9, 9, -5, -5] and gal.labels.dtype == torch.int64
    assert gal._label_dev[:10].tolist() == gal.labels.tolist() and gal._rows.shape[0] >= 10
    assert gal._label_dev.shape[0] == gal._rows.shape[0] + 1 and int(gal._label_dev[-1]) == -1       # what the fill reads
    # a label that returns after another one came in between: refused, nothing written
    before = (gal._head.clone(), gal.labels.clone(), gal.num_groups, set(gal._closed), gal._open)
    for bad in (7, 4, 9, [-5, 9], [-5, 3, -5], [1, 2, 1], [-5, -5, 8, 8, 7], torch.tensor([3, 3, 5, 3])):
        with pytest.raises(ValueError, match="returns"):
            gal._append(rows(1 if isinstance(bad, int) else len(bad)), bad)
    for bad in ([1, 2], [[1], [2], [3]], [0.5, 1.5, 2.5], torch.tensor([1, 2])):     # not one int label per row
        with pytest.raises(ValueError):
            gal._append(rows(3), bad)
    with pytest.raises(ValueError, match="group="):
        gal._append(rows(3))
    assert len(gal) == 10 and torch.equal(gal._head, before[0]) and torch.equal(gal.labels, before[1])
    assert (gal.num_groups, gal._closed, gal._open) == before[2:] == (4, {7, 4, 9}, (-5, 8))
    gal._append(rows(3), [-5, 3, 1])                                       # the open group may still continue
    assert gal.num_groups == 6 and gal._head[10:13].tolist() == [8, 11, 12]
    # the state: three keys more, and only here; clear() forgets the groups
    state = gal.state_dict()
    assert set(state) == {"rows", "count", "E", "side", "products", "grouped", "group_head", "labels"}
    assert state["grouped"] is True and state["group_head"].tolist() == gal._head[:13].tolist()
    assert state["labels"].tolist() == gal.labels.tolist() and state["labels"].device.type == "cpu"
    gal.clear()
    assert len(gal) == 0 and gal.num_groups == 0 and gal.labels.numel() == 0
    gal._append(rows(2), [7, 4])                                           # labels of before the clear() are free again
    assert gal.num_groups == 2
    gal.load_state_dict(state)
    assert len(gal) == 13 and gal.num_groups == 6 and gal._head[:13].tolist() == state["group_head"].tolist()
    assert gal.labels.tolist() == state["labels"].tolist() and gal._label_dev[:13].tolist() == state["labels"].tolist()
    with pytest.raises(ValueError, match="returns"):
        gal._append(rows(1), 7)
    # a saved state whose labels return is refused before anything is written
    with pytest.raises(ValueError, match="returns"):
        gal.load_state_dict(dict(state, labels=torch.tensor([1, 2, 1] + [5] * 10)))
    with pytest.raises(ValueError):
        gal.load_state_dict(dict(state, labels=state["labels"][:5]))
    with pytest.raises(ValueError):
        gal.load_state_dict(dict(state, group_head=state["group_head"].long()))
    assert len(gal) == 13 and gal.num_groups == 6 and gal.labels.tolist() == state["labels"].tolist()


def test_state_dict_key_sets_and_flag_mismatches(model):
    plain, dsl = _bare(model), _bare(model, dual_softmax=True)
    assert set(plain.state_dict()) == {"rows", "count", "E", "side", "products"}
    assert set(dsl.state_dict()) == {"rows", "count", "E", "side", "products", "dual_softmax", "bank", "m", "s"}
    grouped, both = _bare(model, grouped=True), _bare(model, dual_softmax=True, grouped=True)
    assert set(grouped.state_dict()) == set(plain.state_dict()) | {"grouped", "group_head", "labels"}
    assert set(both.state_dict()) == set(dsl.state_dict()) | {"grouped", "group_head", "labels"}
    grouped._append(torch.ones(3, 192, dtype=torch.float16), [1, 1, 2])
    plain._append(torch.ones(2, 192, dtype=torch.float16))
    for a, b in ((plain, grouped), (grouped, plain), (dsl, both), (both, dsl)):        # compared before anything is written
        with pytest.raises(ValueError, match="grouped"):
            a.load_state_dict(b.state_dict())
    with pytest.raises(ValueError, match="dual_softmax"):
        grouped.load_state_dict(both.state_dict())
    assert len(plain) == 2 and len(grouped) == 3 and grouped.num_groups == 2 and grouped._head[:3].tolist() == [0, 0, 2]
