"""Rank of a known row or group without a GPU: the NumPy restatement of the contract the GPU checks compare against (pinned
on a hand-written example), the header's declarations, every early return of cc_similarity_rank_planes_f32 and their order
(the checks end before anything is read or launched, so never-dereferenced addresses do), the workspace query, the op's fake
kernel and ValueErrors, and the refusals of FeatureGallery.rank* / eval_epoch(matrix_free=True) that come before any launch."""
import os

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_grouped_host import _bare, _meta, _p, model  # noqa: F401  (model: the fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rank_ref(S, target, sel=None, head=None):
    """The contract, restated on the matrix.  S [Nq, n] scores, target [Nq] rows, sel bool [n] or [Nq, n] (None: all rows
    selectable), head [n] or None -> (counts int64 [Nq, 3], score [Nq] of S's dtype).
    Rows: t = S[q, target[q]] whatever sel says; over the selectable rows (#x > t, #x == t, #x == t with r < target[q]).
    Groups (head[r] = first row of r's group): a group's score is the maximum over its selectable rows; t = the score of
    target[q]'s group, -inf without a selectable row; over the groups with a selectable row (#greater, #equal, #equal lying in
    front of the target's group).  A target outside [0, n): (0, 0, 0) and -inf.  Plain float compares."""
    S = np.asarray(S)
    nq, n = S.shape
    sel = np.ones((nq, n), dtype=bool) if sel is None else np.broadcast_to(np.asarray(sel, dtype=bool), (nq, n))
    counts = np.zeros((nq, 3), dtype=np.int64)
    score = np.full(nq, -np.inf, dtype=S.dtype)
    for q in range(nq):
        g = int(target[q])
        if not 0 <= g < n:
            continue
        if head is None:
            t = S[q, g]
            x, front = S[q, sel[q]], np.flatnonzero(sel[q]) < g
        else:
            hd = np.asarray(head)[:n]
            starts = np.unique(hd)
            best = np.full(starts.size, -np.inf, dtype=S.dtype)
            alive = np.zeros(starts.size, dtype=bool)
            gi = np.searchsorted(starts, hd)                                 # the group index of every row
            live = np.flatnonzero(sel[q])
            np.maximum.at(best, gi[live], S[q, live])
            alive[gi[live]] = True
            t = best[gi[g]] if alive[gi[g]] else S.dtype.type(-np.inf)
            x, front = best[alive], starts[alive] < hd[g]
        score[q] = t
        counts[q] = (int((x > t).sum()), int((x == t).sum()), int(((x == t) & front).sum()))
    return counts, score


def test_the_reference_counts_on_a_hand_written_example():
    assert "similarity_rank" in torch_ops.OPS                                # the op whose contract rank_ref restates
    S = np.array([[1, 5, 5, 2, 5, 3, 0, -0.0, 4],
                  [-1, -1, -1, 7, -3, -2, 7, 7, 9]], dtype=np.float32)
    inf = np.float32("-inf")
    counts, score = rank_ref(S, [4, 7])
    assert counts.tolist() == [[0, 3, 2], [1, 3, 2]] and score.tolist() == [5, 7]
    assert (counts[:, 0] + counts[:, 2]).tolist() == [2, 3]                  # the places in the stable descending sort
    assert np.argsort(-S, axis=1, kind="stable")[[0, 1], [2, 3]].tolist() == [4, 7]
    counts, score = rank_ref(S, [7, 9])                                      # -0 == +0; a target outside the rows
    assert counts.tolist() == [[7, 2, 1], [0, 0, 0]] and np.signbit(score[0]) and score[1] == inf
    sel = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)                  # rows 1, 4, 8 may not be ranked
    counts, score = rank_ref(S, [4, 8], sel)                                 # both targets unselectable: scored, not counted
    assert counts.tolist() == [[0, 1, 1], [0, 0, 0]] and score.tolist() == [5, 9]
    nan = S.copy()
    nan[0, 4] = nan[1, 0] = np.nan                                           # a NaN is neither greater nor equal
    assert rank_ref(nan, [4, 7])[0].tolist() == [[0, 0, 0], [1, 3, 2]]
    head = np.array([0, 0, 0, 3, 4, 4, 6, 6, 6])                             # groups of 3, 1, 2, 3 rows
    counts, score = rank_ref(S, [5, 2], head=head)                           # any row of the group names it
    assert counts.tolist() == [[0, 2, 1], [2, 1, 0]] and score.tolist() == [5, -1]
    counts, score = rank_ref(S, [5, 3], sel & (head != 6), head)             # group 2 loses row 4; group 3 is dead
    assert counts.tolist() == [[1, 1, 0], [0, 1, 0]] and score.tolist() == [3, 7]
    counts, score = rank_ref(S, [8, 8], sel & (head != 6), head)             # the target group has no selectable row
    assert counts.tolist() == [[3, 0, 0], [3, 0, 0]] and score.tolist() == [inf, inf]


# ------------------------------------------------------------------------------------------------ the library
def test_the_header_declares_the_two_entries():
    text = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    assert "size_t cc_similarity_rank_workspace_bytes(int32_t Bq, int32_t Bg);" in text
    decl = text[text.index("int cc_similarity_rank_planes_f32("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int cc_similarity_rank_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, "
                    "int32_t E, float mult, int32_t products, const int32_t* target, const int32_t* row_mask, int32_t mask_rows, "
                    "int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total, "
                    "const int32_t* group_head, int32_t* counts, float* score, void* ws, size_t ws_bytes, void* stream)")


def _rank(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, target=256, mask=0, mask_rows=1, words=4, m=0, s=0, side=1,
          n_total=100, head=0, counts=256, score=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_rank_workspace_bytes(Bq, Bg)
    return lib.cc_similarity_rank_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, _p(target), _p(mask), mask_rows, words, _p(m),
                                             _p(s), side, n_total, _p(head), _p(counts), _p(score), _p(ws), ws_bytes, None)


@pytest.mark.parametrize("extra", [dict(), dict(mask=256), dict(m=256, s=256), dict(head=256), dict(mask=256, m=256, s=256, head=256),
                                   dict(mask=256, mask_rows=4), dict(mask=256, mask_rows=4, m=256, s=256, side=0, head=256)])
def test_entry_refuses_before_touching_memory(extra):
    lib = L.lib()
    call = lambda **kw: _rank(lib, **dict(extra, **kw))
    for null in ("q", "g", "target", "counts", "score"):
        assert call(**{null: 0}) == INVALID, null
    own = [dict(m=256, s=0), dict(m=0, s=256)]
    if "mask" in extra:
        own += [dict(mask_rows=0), dict(mask_rows=2), dict(mask_rows=5), dict(mask_rows=-1), dict(words=3), dict(words=0)]
    if "m" in extra:
        own += [dict(n_total=-1), dict(side=2), dict(side=-1)]
    for kw in [dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(Bg=-5), dict(E=-64)] + own:
        assert call(**kw) == INVALID, kw
    for kw in (dict(products=0), dict(products=4), dict(E=96), dict(E=1088), dict(Bq=16 * 65535 + 1, mask_rows=1)):
        assert call(**kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_rank_workspace_bytes(4, 100)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws=0) == WORKSPACE
    # the order: invalid before unsupported before the workspace
    assert call(target=0, E=96, ws=0) == INVALID and call(m=256, s=0, E=96) == INVALID
    assert call(E=96, ws=0) == UNSUPPORTED
    # no lists: the widest rows with three products pass the limits (the top-k entries exclude them at k = 128)
    for kw in (dict(E=1024, products=3), dict(E=1024, products=1), dict(Bq=16 * 65535, mask_rows=1)):
        assert call(ws_bytes=0, **kw) == WORKSPACE, kw


def test_without_a_mask_or_statistics_their_arguments_are_not_looked_at():
    lib = L.lib()
    assert _rank(lib, mask_rows=7, words=0, ws_bytes=0) == WORKSPACE         # row_mask == NULL: every row
    assert _rank(lib, n_total=-1, side=7, ws_bytes=0) == WORKSPACE           # m == s == NULL ranks S


def test_the_workspace_query_needs_no_gpu():
    """slices * Bq * 3 int32 partial counts on the top-k grid, nothing of size Bq * Bg"""
    lib = L.lib()
    for Bq, Bg in ((1, 1), (16, 4099), (17, 4099), (16, 200003), (10000, 1000)):
        w = lib.cc_similarity_rank_workspace_bytes(Bq, Bg)
        slices = lib.cc_similarity_topk_slices(Bq, Bg, 1)
        assert Bq * slices * 12 <= w < Bq * slices * 12 + 256
        assert _rank(lib, Bq=Bq, Bg=Bg, words=(Bg + 31) // 32, ws_bytes=w - 1) == WORKSPACE
    assert lib.cc_similarity_rank_workspace_bytes(0, 5) == lib.cc_similarity_rank_workspace_bytes(5, 0) == 0
    assert lib.cc_similarity_rank_workspace_bytes(16, 200000) < 16 * 200000 * 4 // 16


# ------------------------------------------------------------------------------------------------ the op
def _words(*shape):
    return torch.empty(*shape, device="meta", dtype=torch.int32)


def _targets(n, dtype=torch.int64):
    return torch.empty(n, device="meta", dtype=dtype)


def test_fake_kernel_gives_shapes_on_the_meta_device():
    assert "similarity_rank" in torch_ops.OPS
    op = torch.ops.centerclip
    q, g = _meta(40), _meta(1000)
    head = torch.empty(1000, device="meta", dtype=torch.int32)
    stat = torch.empty(1000, device="meta")
    for counts, score in (op.similarity_rank(q, g, 900, 20.0, 2, _targets(40)),
                          op.similarity_rank(q, g, 900, 20.0, 2, _targets(40, torch.int32), _words(29)),
                          op.similarity_rank(q, g, 900, 20.0, 2, _targets(40), _words(40, 32)),
                          op.similarity_rank(q, g, 900, 20.0, 2, _targets(40), None, stat, stat, 1, 900),
                          op.similarity_rank(q, g, 900, 20.0, 2, _targets(40), _words(40, 29), stat[:40], stat[:40], 0, 900, head),
                          op.similarity_rank(q, g, 900, 20.0, 2, _targets(40), group_head=head)):
        assert counts.shape == (40, 3) and counts.dtype == torch.int32 and counts.device.type == "meta"
        assert score.shape == (40,) and score.dtype == torch.float32 and score.device.type == "meta"
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        op.similarity_rank(h(2), h(8), 8, 1.0, 2, torch.zeros(2, dtype=torch.long))


def test_op_refuses_arguments_that_do_not_fit():
    op = torch.ops.centerclip
    q, g = _meta(4), _meta(100)
    stat = torch.empty(100, device="meta")
    head = torch.empty(100, device="meta", dtype=torch.int32)
    call = lambda q=q, g=g, n=100, target=_targets(4), mask=None, m=None, s=None, side=1, head=None: op.similarity_rank(
        q, g, n, 1.0, 2, target, mask, m, s, side, 100, head)
    call()
    call(mask=_words(4, 9), m=stat, s=stat, head=head)
    for kw in (dict(target=_targets(3)), dict(target=_targets(5)), dict(target=torch.empty(4, 1, device="meta", dtype=torch.int64)),
               dict(target=torch.empty(4, device="meta")), dict(target=_targets(4, torch.int16)),
               dict(target=torch.zeros(4, dtype=torch.int64)),                              # not on the planes' device
               dict(mask=torch.empty(4, device="meta", dtype=torch.int64)), dict(mask=_words(8)[::2]), dict(mask=_words(3)),
               dict(mask=_words(3, 4)), dict(mask=torch.zeros(4, dtype=torch.int32)),
               dict(m=stat), dict(s=stat), dict(m=stat[:99], s=stat), dict(m=stat[:3], s=stat[:3], side=0),
               dict(head=torch.empty(99, device="meta", dtype=torch.int32)),
               dict(n=101), dict(g=_meta(100, 384)), dict(g=_meta(100, dtype=torch.float32))):
        with pytest.raises(ValueError, match="similarity_rank"):
            call(**kw)


# ------------------------------------------------------------------------------------------------ FeatureGallery
def _rows(n):
    return torch.arange(n, dtype=torch.float16)[:, None].expand(n, 192).contiguous()


def test_rank_refusals_come_before_any_launch(model):
    """on a stub without a device: a ValueError means the check ran before anything was encoded or launched (what comes next
    there is the refusal of CPU tensors, CenterClipHipError)"""
    seq = torch.zeros(3, 1, 64)
    ids = torch.zeros(3, 16, dtype=torch.long)
    gal = _bare(model)
    gal._append(_rows(70))
    for bad in ([0, 1], [0, 1, 2, 3], torch.tensor([1, 2]), 5):                                 # one position per query
        with pytest.raises(ValueError, match="per query"):
            gal.rank_features(seq, bad)
        with pytest.raises(ValueError, match="per query"):
            gal.rank(ids, target=bad)
    for bad in ([0, 1, 70], [-1, 0, 1], torch.tensor([0, 69, 70])):                             # inside [0, span)
        with pytest.raises(ValueError, match="outside"):
            gal.rank_features(seq, bad)
        with pytest.raises(ValueError, match="outside"):
            gal.rank(ids, target=bad)
    for bad in ([0.5, 1, 2], [[0, 1, 2]], "abc", torch.tensor([0, 1, 2], dtype=torch.int32)):
        with pytest.raises(ValueError, match="target"):
            gal.rank_features(seq, bad)
    for bad in (torch.zeros(2, dtype=torch.long, device="meta"), torch.zeros(3, device="meta"),
                torch.zeros(3, 1, dtype=torch.long, device="meta")):                            # a device tensor: shape and dtype only
        with pytest.raises(ValueError, match="per query"):
            gal.rank_features(seq, bad)
    with pytest.raises(L.CenterClipHipError):                                                   # the same position twice is fine
        gal.rank_features(seq, [5, 5, 69])
    gal.remove([5])
    with pytest.raises(L.CenterClipHipError):                                                   # ... and so is a removed one
        gal.rank_features(seq, torch.tensor([5, 5, 0]))
    with pytest.raises(ValueError, match="grouped=True"):
        gal.rank_groups(ids, target=[1, 2, 3])
    with pytest.raises(ValueError, match="grouped=True"):
        gal.rank_groups_features(seq, [1, 2, 3])
    empty = _bare(model)
    with pytest.raises(ValueError, match="outside"):                                            # no valid position
        empty.rank_features(seq, [0, 0, 0])


def test_rank_groups_maps_labels_to_heads_on_the_host(model):
    vis, vmask = torch.zeros(3, 4, 64), torch.ones(3, 4, dtype=torch.long)
    gal = _bare(model, "text", grouped=True)
    gal._append(_rows(11), [7] * 4 + [4] * 2 + [9] * 3 + [-5] * 2)           # heads 0 0 0 0 4 4 6 6 6 9 9
    assert gal._group_targets([9, 7, 9], 3).tolist() == [6, 0, 6] and gal._group_targets(torch.tensor([-5]), 1).tolist() == [9]
    assert gal._group_targets(4, 1).tolist() == [4]
    for bad in ([8, 7, 9], [7, 9, 12], torch.tensor([7, 7, 3])):
        with pytest.raises(ValueError, match="label 8|label 12|label 3"):
            gal.rank_groups_features(vis, bad, mask=vmask)
        with pytest.raises(ValueError, match="no row held"):
            gal.rank_groups(vis, vmask, target=bad)
    for bad in ([7, 9], [7, 9, 4, 4], 7):
        with pytest.raises(ValueError, match="per query"):
            gal.rank_groups_features(vis, bad, mask=vmask)
    for bad in (torch.zeros(3, dtype=torch.long, device="meta"), torch.tensor([7, 7, 7], dtype=torch.int32), [0.5, 1, 2]):
        with pytest.raises(ValueError, match="labels"):                      # no device tensor (it would have to be read)
            gal.rank_groups_features(vis, bad, mask=vmask)
    with pytest.raises(L.CenterClipHipError):
        gal.rank_groups_features(vis, [9, 7, 9], mask=vmask)
    gal.remove_groups([4])                                                   # a removed group keeps its label until compact()
    assert gal._group_targets([4, 9], 2).tolist() == [4, 6]
    gal.compact()
    with pytest.raises(ValueError, match="label 4"):
        gal._group_targets([4], 1)
    assert gal._group_targets([9, -5], 2).tolist() == [4, 7]


# ------------------------------------------------------------------------------------------------ eval_epoch
def test_matrix_free_with_sharding_is_refused_before_the_loader_is_touched(monkeypatch):
    from centerclip_amd import eval as E

    class Never:
        def __getattr__(self, name):
            raise AssertionError("eval_epoch touched %s before refusing" % name)
    monkeypatch.setattr(E.ccdist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="out of scope"):
        E.eval_epoch(Never(), Never(), "cpu", shard=True, matrix_free=True)
    assert "matrix_free_metrics" in E.__all__ and callable(E.matrix_free_metrics)
