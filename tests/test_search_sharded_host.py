"""A gallery split in shards without a GPU: the NumPy statement of the merge order the GPU checks compare against (pinned on a
hand-written example), the header's declarations, every early return of cc_topk_merge_lists_f32 /
cc_similarity_target_score_planes_f32 / cc_similarity_count_planes_f32 and their order (the checks end before anything is read
or launched, so never-dereferenced addresses do), the workspace query, the ops' fake kernels and ValueErrors, and on stubs
without a device ShardedGallery's refusals, its id routing and the cursor each shard is handed."""
import os

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_grouped_host import _bare, _meta, _p, model  # noqa: F401  (model: the fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT_ALL = 2 ** 31 - 1


def ordered_bits(scores):
    """the score part of the top-k key: the bits of score + 0.0 (so -0 orders as +0) mapped so that unsigned order = float order"""
    u = (np.asarray(scores, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def merge_ref(scores, ids):
    """The merge order, stated with np.lexsort.  scores fp32 / ids int [S, Bq, k] (id < 0: a fill) -> (scores [Bq, k] fp32,
    global ids [Bq, k] int64 = (shard << 32) | id, src [Bq, k] int32 = shard * k + index): fills last, then descending ordered
    score, then smaller shard, then smaller local id; the fill leaves as (-inf, -1, -1)."""
    scores, ids = np.asarray(scores, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    S, Bq, k = scores.shape
    out_s = np.full((Bq, k), -np.inf, dtype=np.float32)
    out_i = np.full((Bq, k), -1, dtype=np.int64)
    out_src = np.full((Bq, k), -1, dtype=np.int32)
    shard = np.repeat(np.arange(S, dtype=np.int64), k)
    for q in range(Bq):
        sc, lid = scores[:, q].reshape(-1), ids[:, q].reshape(-1)
        fill = lid < 0
        descending = np.where(fill, 0, np.int64(0xFFFFFFFF) - ordered_bits(sc).astype(np.int64))
        order = np.lexsort((lid, shard, descending, fill))[:k]                 # (the last key is the first criterion)
        keep = order[~fill[order]]
        out_s[q, :keep.size], out_src[q, :keep.size] = sc[keep], keep
        out_i[q, :keep.size] = (shard[keep] << 32) | lid[keep]
    return out_s, out_i, out_src


def test_the_merge_order_on_a_hand_written_example():
    for name in ("similarity_topk_merge", "similarity_target_score", "similarity_count"):
        assert name in torch_ops.OPS
    inf = np.float32("-inf")
    scores = np.array([[[5, 0.0, -1, 99]], [[5, -0.0, -2, 99]]], dtype=np.float32)     # [2, 1, 4]; the fills' scores are not read
    ids = np.array([[[3, 7, 1, -1]], [[0, 2, 9, -1]]])
    s, i, src = merge_ref(scores, ids)
    # equal scores: the smaller shard first, whatever the local ids; -0 ties with +0 and keeps its sign
    assert i.tolist() == [[3, 1 << 32, 7, (1 << 32) | 2]] and src.tolist() == [[0, 4, 1, 5]]
    assert s.tolist() == [[5, 5, 0, 0]] and np.signbit(s[0]).tolist() == [False, False, False, True]
    # inside a shard equal scores go by smaller id (the lists come that way), and the fill is last
    scores = np.array([[[2, 2, 0]], [[3, 2, 0]], [[0, 0, 0]]], dtype=np.float32)
    ids = np.array([[[4, 6, -1]], [[8, 1, -1]], [[-1, -1, -1]]])
    s, i, src = merge_ref(scores, ids)
    assert i.tolist() == [[(1 << 32) | 8, 4, 6]] and src.tolist() == [[3, 0, 1]] and s.tolist() == [[3, 2, 2]]
    s, i, src = merge_ref(scores[2:], ids[2:])                                         # nothing but fill
    assert s.tolist() == [[inf] * 3] and i.tolist() == [[-1] * 3] and src.tolist() == [[-1] * 3]
    s, i, src = merge_ref(scores[:1, :, :2], ids[:1, :, :2])                           # one shard: the list itself
    assert i.tolist() == [[4, 6]] and src.tolist() == [[0, 1]]
    neg = merge_ref(np.array([[[-np.inf]], [[-3e38]], [[np.inf]]], dtype=np.float32), np.array([[[0]], [[0]], [[0]]]))
    assert neg[1].tolist() == [[2 << 32]] and neg[0].tolist() == [[np.inf]]            # a real -inf is an entry, not a fill
    assert ordered_bits([-0.0])[0] == ordered_bits([0.0])[0] and ordered_bits([1.0])[0] > ordered_bits([-1.0])[0]


# ------------------------------------------------------------------------------------------------ the library
def _decl(text, name):
    decl = text[text.index(name + "("):]
    return " ".join(decl[:decl.index(";")].split())


def test_the_header_declares_the_three_entries_and_the_workspace_query():
    text = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    assert "#define CC_TOPK_MERGE_MAX_LISTS 64" in text and torch_ops.TOPK_MERGE_MAX_LISTS == 64
    assert "size_t cc_similarity_count_workspace_bytes(int32_t Bq, int32_t Bg);" in text
    assert _decl(text, "int cc_topk_merge_lists_f32") == (
        "int cc_topk_merge_lists_f32(const float* scores, const int32_t* ids, int32_t S, int32_t Bq, int32_t k, float* out_scores, "
        "int64_t* out_ids, int32_t* out_src, void* stream)")
    assert _decl(text, "int cc_similarity_target_score_planes_f32") == (
        "int cc_similarity_target_score_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, "
        "int32_t E, float mult, int32_t products, const int32_t* target, const int32_t* row_mask, int32_t mask_rows, "
        "int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total, "
        "const int32_t* group_head, float* score, void* stream)")
    assert _decl(text, "int cc_similarity_count_planes_f32") == (
        "int cc_similarity_count_planes_f32(const void* query_planes, const void* gallery_planes, int32_t Bq, int32_t Bg, int32_t E, "
        "float mult, int32_t products, const float* bound_scores, const int32_t* bound_front, const int32_t* row_mask, "
        "int32_t mask_rows, int32_t mask_words, const float* m, const float* s, int32_t stats_on_gallery, int32_t n_total, "
        "const int32_t* group_head, int32_t* counts, void* ws, size_t ws_bytes, void* stream)")


def _merge(lib, scores=256, ids=256, S=2, Bq=4, k=10, out_scores=256, out_ids=256, out_src=256):
    return lib.cc_topk_merge_lists_f32(_p(scores), _p(ids), S, Bq, k, _p(out_scores), _p(out_ids), _p(out_src), None)


def test_merge_entry_refuses_before_touching_memory():
    """(no workspace: INVALID, then UNSUPPORTED; a call that passes both would launch, so none is made here)"""
    lib = L.lib()
    for null in ("scores", "ids", "out_scores", "out_ids", "out_src"):
        assert _merge(lib, S=65, **{null: 0}) == INVALID, null
    for kw in (dict(S=0), dict(S=-1), dict(Bq=0), dict(Bq=-4), dict(k=0), dict(k=-1), dict(S=0, k=4097), dict(k=0, S=65)):
        assert _merge(lib, **kw) == INVALID, kw
    for kw in (dict(S=65), dict(k=4097), dict(S=1000, k=5000)):
        assert _merge(lib, **kw) == UNSUPPORTED, kw


def _target(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, target=256, mask=0, mask_rows=1, words=4, m=0, s=0, side=1,
            n_total=100, head=0, score=256):
    return lib.cc_similarity_target_score_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, _p(target), _p(mask), mask_rows, words,
                                                     _p(m), _p(s), side, n_total, _p(head), _p(score), None)


def _count(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, bound=256, front=256, mask=0, mask_rows=1, words=4, m=0, s=0,
           side=1, n_total=100, head=0, counts=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_count_workspace_bytes(Bq, Bg)
    return lib.cc_similarity_count_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, _p(bound), _p(front), _p(mask), mask_rows,
                                              words, _p(m), _p(s), side, n_total, _p(head), _p(counts), _p(ws), ws_bytes, None)


EXTRAS = [dict(), dict(mask=256), dict(m=256, s=256), dict(head=256), dict(mask=256, m=256, s=256, head=256),
          dict(mask=256, mask_rows=4), dict(mask=256, mask_rows=4, m=256, s=256, side=0, head=256)]


def _own_invalid(extra):
    own = [dict(m=256, s=0), dict(m=0, s=256)]
    if "mask" in extra:
        own += [dict(mask_rows=0), dict(mask_rows=2), dict(mask_rows=5), dict(mask_rows=-1), dict(words=3), dict(words=0)]
    if "m" in extra:
        own += [dict(n_total=-1), dict(side=2), dict(side=-1)]
    return [dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(Bg=-5), dict(E=-64)] + own


@pytest.mark.parametrize("extra", EXTRAS)
def test_target_score_entry_refuses_before_touching_memory(extra):
    """(no workspace: every call here carries an argument the entry refuses, so nothing is launched)"""
    lib = L.lib()
    call = lambda **kw: _target(lib, **dict(extra, **kw))
    for null in ("q", "g", "target", "score"):
        assert call(E=96, **{null: 0}) == INVALID, null
    for kw in _own_invalid(extra):
        assert call(**kw) == INVALID, kw
    for kw in (dict(products=0), dict(products=4), dict(E=96), dict(E=1088)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(m=256, s=0, E=96) == INVALID                               # the order: invalid before unsupported


@pytest.mark.parametrize("extra", EXTRAS)
def test_count_entry_refuses_before_touching_memory(extra):
    lib = L.lib()
    call = lambda **kw: _count(lib, **dict(extra, **kw))
    for null in ("q", "g", "bound", "front", "counts"):
        assert call(**{null: 0}) == INVALID, null
    for kw in _own_invalid(extra):
        assert call(**kw) == INVALID, kw
    for kw in (dict(products=0), dict(products=4), dict(E=96), dict(E=1088), dict(Bq=16 * 65535 + 1, mask_rows=1)):
        assert call(**kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_count_workspace_bytes(4, 100)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws=0) == WORKSPACE
    # the order: invalid before unsupported before the workspace
    assert call(front=0, E=96, ws=0) == INVALID and call(m=256, s=0, E=96) == INVALID
    assert call(E=96, ws=0) == UNSUPPORTED
    for kw in (dict(E=1024, products=3), dict(E=1024, products=1), dict(Bq=16 * 65535, mask_rows=1)):
        assert call(ws_bytes=0, **kw) == WORKSPACE, kw


def test_without_a_mask_or_statistics_their_arguments_are_not_looked_at():
    lib = L.lib()
    assert _count(lib, mask_rows=7, words=0, ws_bytes=0) == WORKSPACE         # row_mask == NULL: every row
    assert _count(lib, n_total=-1, side=7, ws_bytes=0) == WORKSPACE           # m == s == NULL counts S
    assert _target(lib, mask_rows=7, words=0, E=96) == UNSUPPORTED and _target(lib, n_total=-1, side=7, E=96) == UNSUPPORTED


def test_the_workspace_query_needs_no_gpu():
    """the rank entry's: slices * Bq * 3 int32 partial counts, nothing of size Bq * Bg"""
    lib = L.lib()
    for Bq, Bg in ((1, 1), (16, 4099), (17, 4099), (16, 200003), (10000, 1000)):
        w = lib.cc_similarity_count_workspace_bytes(Bq, Bg)
        assert w == lib.cc_similarity_rank_workspace_bytes(Bq, Bg)
        slices = lib.cc_similarity_topk_slices(Bq, Bg, 1)
        assert Bq * slices * 12 <= w < Bq * slices * 12 + 256
        assert _count(lib, Bq=Bq, Bg=Bg, words=(Bg + 31) // 32, ws_bytes=w - 1) == WORKSPACE
    assert lib.cc_similarity_count_workspace_bytes(0, 5) == lib.cc_similarity_count_workspace_bytes(5, 0) == 0


# ------------------------------------------------------------------------------------------------ the ops
def _t(*shape, dtype=torch.float32, device="meta"):
    return torch.empty(*shape, device=device, dtype=dtype)


def test_fake_kernels_give_shapes_on_the_meta_device():
    op = torch.ops.centerclip
    for S, Bq, k in ((1, 5, 1), (3, 40, 17), (64, 2, 4096)):
        scores, ids, src = op.similarity_topk_merge(_t(S, Bq, k), _t(S, Bq, k, dtype=torch.int32))
        assert scores.shape == ids.shape == src.shape == (Bq, k) and scores.device.type == "meta"
        assert (scores.dtype, ids.dtype, src.dtype) == (torch.float32, torch.int64, torch.int32)
    q, g = _meta(40), _meta(1000)
    head, stat = _t(1000, dtype=torch.int32), _t(1000)
    tg, bound, front = _t(40, dtype=torch.int64), _t(40), _t(40, dtype=torch.int32)
    for tail in ((), (_t(29, dtype=torch.int32),), (_t(40, 32, dtype=torch.int32),), (None, stat, stat, 1, 900),
                 (_t(40, 29, dtype=torch.int32), stat[:40], stat[:40], 0, 900, head), (None, None, None, 1, 0, head)):
        score = op.similarity_target_score(q, g, 900, 20.0, 2, tg, *tail)
        assert score.shape == (40,) and score.dtype == torch.float32 and score.device.type == "meta"
        counts = op.similarity_count(q, g, 900, 20.0, 2, bound, front, *tail)
        assert counts.shape == (40, 3) and counts.dtype == torch.int32 and counts.device.type == "meta"
    assert op.similarity_target_score(q, g, 900, 20.0, 2, _t(40, dtype=torch.int32)).shape == (40,)
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        op.similarity_topk_merge(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        op.similarity_target_score(h(2), h(8), 8, 1.0, 2, torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        op.similarity_count(h(2), h(8), 8, 1.0, 2, torch.zeros(2), torch.zeros(2, dtype=torch.int32))


def test_ops_refuse_arguments_that_do_not_fit():
    op = torch.ops.centerclip
    i32 = torch.int32
    for scores, ids in ((_t(0, 4, 5), _t(0, 4, 5, dtype=i32)), (_t(65, 4, 5), _t(65, 4, 5, dtype=i32)),
                        (_t(2, 4, 0), _t(2, 4, 0, dtype=i32)), (_t(2, 4, 4097), _t(2, 4, 4097, dtype=i32)),
                        (_t(2, 4, 5), _t(2, 4, 5, dtype=torch.int64)), (_t(2, 4, 5, dtype=torch.float16), _t(2, 4, 5, dtype=i32)),
                        (_t(2, 4, 5), _t(2, 4, 6, dtype=i32)), (_t(4, 5), _t(4, 5, dtype=i32)),
                        (_t(2, 4, 5), torch.zeros(2, 4, 5, dtype=i32))):                    # not on one device
        with pytest.raises(ValueError, match="similarity_topk_merge"):
            op.similarity_topk_merge(scores, ids)
    q, g = _meta(4), _meta(100)
    stat, head = _t(100), _t(100, dtype=i32)
    common = (dict(mask=_t(4, dtype=torch.int64)), dict(mask=_t(8, dtype=i32)[::2]), dict(mask=_t(3, dtype=i32)),
              dict(mask=_t(3, 4, dtype=i32)), dict(mask=torch.zeros(4, dtype=i32)), dict(m=stat), dict(s=stat),
              dict(m=stat[:99], s=stat), dict(m=stat[:3], s=stat[:3], side=0), dict(head=_t(99, dtype=i32)), dict(n=101),
              dict(g=_meta(100, 384)), dict(g=_meta(100, dtype=torch.float32)))
    target = lambda q=q, g=g, n=100, target=_t(4, dtype=torch.int64), mask=None, m=None, s=None, side=1, head=None: \
        op.similarity_target_score(q, g, n, 1.0, 2, target, mask, m, s, side, 100, head)
    target()
    target(mask=_t(4, 9, dtype=i32), m=stat, s=stat, head=head)
    for kw in (dict(target=_t(3, dtype=torch.int64)), dict(target=_t(4, 1, dtype=torch.int64)), dict(target=_t(4)),
               dict(target=_t(4, dtype=torch.int16)), dict(target=torch.zeros(4, dtype=torch.int64))) + common:
        with pytest.raises(ValueError, match="similarity_target_score"):
            target(**kw)
    count = lambda q=q, g=g, n=100, bound=_t(4), front=_t(4, dtype=i32), mask=None, m=None, s=None, side=1, head=None: \
        op.similarity_count(q, g, n, 1.0, 2, bound, front, mask, m, s, side, 100, head)
    count()
    count(mask=_t(4, 9, dtype=i32), m=stat, s=stat, head=head)
    for kw in (dict(bound=_t(3)), dict(bound=_t(4, dtype=torch.float64)), dict(bound=_t(4, 1)), dict(bound=torch.zeros(4)),
               dict(front=_t(5, dtype=i32)), dict(front=_t(4, dtype=torch.int64)), dict(front=_t(4)),
               dict(front=torch.zeros(4, dtype=i32))) + common:
        with pytest.raises(ValueError, match="similarity_count"):
            count(**kw)


# ------------------------------------------------------------------------------------------------ ShardedGallery, on stubs
def _rows(n):
    return torch.arange(n, dtype=torch.float16)[:, None].expand(n, 192).contiguous()


def _shards(model, spans, **kw):
    out = []
    for i, n in enumerate(spans):
        g = _bare(model, **kw)
        if n:
            g._append(_rows(n), *(([100 * i + j // 3 for j in range(n)],) if kw.get("grouped") else ()))
        out.append(g)
    return out


def test_construction_refusals(model):
    from centerclip_amd.search_sharded import ShardedGallery, __all__
    assert __all__ == ["ShardedGallery"]
    a, b = _shards(model, (3, 4))
    sg = ShardedGallery(shards=[a, b])
    assert (sg.S, sg.first, len(sg), sg.span, sg.global_len(), sg.distributed) == (2, 0, 7, 7, 7, False)
    for bad in (dict(), dict(shards=[a], local=a), dict(shards=[]), dict(shards=[a, "b"]), dict(shards=[a], distributed=True),
                dict(local=a), dict(shards=[a] * 65)):
        with pytest.raises(ValueError, match="ShardedGallery"):
            ShardedGallery(**bad)
    # the five settings the shards must share
    text, dsl, grouped = _bare(model, "text"), _bare(model, dual_softmax=True), _bare(model, grouped=True)
    wide, three = _bare(model), _bare(model)
    wide.E, three.products = 128, 3
    for other in (text, dsl, grouped, wide, three):
        with pytest.raises(ValueError, match="disagree"):
            ShardedGallery(shards=[a, other])
        with pytest.raises(ValueError, match="disagree"):
            ShardedGallery(shards=[other, b, a])
    with pytest.raises(ValueError, match="out of scope"):                  # the statistics would run over every shard's captions
        ShardedGallery(shards=[_bare(model, "text", dual_softmax=True)])
    with pytest.raises(ValueError, match="out of scope"):
        ShardedGallery(local=_bare(model, "text", dual_softmax=True, grouped=True), distributed=True)
    one = ShardedGallery(local=a, distributed=True)                        # no process group: one shard
    assert (one.S, one.first, len(one), one.global_len()) == (1, 0, 3, 3)
    one.validate()
    with pytest.raises(ValueError, match="its own shard"):
        one.add_features(torch.zeros(1, 64), shard=1)


def test_search_and_rank_refusals_come_before_any_launch(model):
    """on stubs without a device: a ValueError means the check ran before anything was encoded or launched (what comes next
    there is the refusal of CPU tensors, CenterClipHipError)"""
    from centerclip_amd.search_sharded import ShardedGallery
    sg = ShardedGallery(shards=_shards(model, (70, 0, 5)))
    seq, ids = torch.zeros(3, 1, 64), torch.zeros(3, 16, dtype=torch.long)
    mask = torch.zeros(3, dtype=torch.int32)
    for bad in ([None], [None] * 4, [mask, mask], mask, (mask,)):                               # one entry per shard
        for call in (lambda: sg.search_features(seq, k=5, allow=bad), lambda: sg.search(ids, k=5, allow=bad),
                     lambda: sg.rank_features(seq, [0, 1, 2], allow=bad), lambda: sg.rank(ids, target=[0, 1, 2], allow=bad)):
            with pytest.raises(ValueError, match="per shard"):
                call()
    f32, i64 = torch.zeros(3), torch.zeros(3, dtype=torch.long)
    for bad in ((f32,), (f32, i64, i64), [f32, [0, 0, 0]], f32, (f32[:2], i64[:2]), (f32, i64[:2]), (f32[None], i64[None]),
                (f32.double(), i64), (f32, i64.int()), (f32, f32), (i64, i64), (f32.to("meta"), i64), (f32, i64.to("meta"))):
        with pytest.raises(ValueError, match="after="):
            sg.search_features(seq, k=5, after=bad)
        with pytest.raises(ValueError, match="after="):
            sg.search(ids, k=5, after=bad)
    for k in (0, -1, 4097):
        with pytest.raises(ValueError, match="1 <= k <= 4096"):
            sg.search_features(seq, k=k)
    for bad in ([0, 1], [0, 1, 2, 3], torch.tensor([1, 2]), 5, torch.zeros(2, dtype=torch.long, device="meta")):
        with pytest.raises(ValueError, match="per query"):
            sg.rank_features(seq, bad)
    for bad in ([0.5, 1, 2], [[0, 1, 2]], "abc", torch.tensor([0, 1, 2], dtype=torch.int32)):
        with pytest.raises(ValueError, match="ints|LongTensor"):
            sg.rank_features(seq, bad)
    with pytest.raises(ValueError, match="per query"):                                          # global ids are 64 bits wide
        sg.rank_features(seq, torch.zeros(3, dtype=torch.int32, device="meta"))
    for call in (lambda: sg.search_groups_features(seq), lambda: sg.search_groups(ids), lambda: sg.rank_groups(ids, target=[1, 2, 3]),
                 lambda: sg.rank_groups_features(seq, [1, 2, 3]), lambda: sg.remove_groups([1]), lambda: sg.row_mask(groups=[1])):
        with pytest.raises(ValueError, match="grouped=True"):
            call()
    # everything in order: the next thing is the encoder's refusal of CPU tensors; ids outside every shard are not refused
    for call in (lambda: sg.search_features(seq, k=5), lambda: sg.search_features(seq, k=4096, allow=[None, mask, None], after=(f32, i64)),
                 lambda: sg.rank_features(seq, [0, (2 << 32) | 4, (5 << 32) | 1]), lambda: sg.rank_features(seq, i64 - 1)):
        with pytest.raises(L.CenterClipHipError):
            call()


def test_ids_route_to_their_shards(model):
    from centerclip_amd.search_sharded import ShardedGallery
    S = ShardedGallery
    sg = S(shards=_shards(model, (70, 0, 5)))
    gid = torch.tensor([0, 69, (2 << 32) | 4, -1, (63 << 32) | (2 ** 31 - 1)])
    shard, local = S.split(gid)
    assert shard.tolist() == [0, 0, 2, -1, 63] and local.tolist() == [0, 69, 4, -1, 2 ** 31 - 1]
    assert [a.tolist() for a in S.split(gid.numpy())] == [shard.tolist(), local.tolist()] and S.split(-1)[1] == -1
    assert torch.equal((shard[:3] << 32) | local[:3], gid[:3])
    # local targets: -1 wherever the shard is not the owner
    tg = sg._local_targets(torch.tensor([5, (1 << 32) | 3, (2 << 32) | 4, -1, (7 << 32) | 1, (2 << 32) | 2 ** 31]))
    assert [t.tolist() for t in tg] == [[5, -1, -1, -1, -1, -1], [-1, 3, -1, -1, -1, -1], [-1, -1, 4, -1, -1, -1]]
    assert all(t.dtype == torch.int32 for t in tg)
    sg.remove([3, (2 << 32) | 1, 68])
    assert [len(g) for g in sg.shards] == [68, 0, 4] and len(sg) == 72 and sg.span == 75
    assert not sg.shards[0]._live[[3, 68]].any() and not sg.shards[2]._live[1]
    for bad, what in (([3], "already removed"), ([(1 << 32) | 0], "outside"), ([(3 << 32) | 0], "no shard"), ([-1], "no shard"),
                      ([5, (2 << 32) | 9], "outside"), ([5, 5], "twice")):
        with pytest.raises(ValueError, match=what):
            sg.remove(bad)
    assert [len(g) for g in sg.shards] == [68, 0, 4]                                            # refused: nothing changed
    masks = sg.row_mask(positions=[1, 33, (2 << 32) | 4])
    assert [m.tolist() for m in masks] == [[2, 2, 0], [], [16]]
    assert [m.tolist() for m in sg.row_mask()] == [[-1, -1, 63], [], [31]]
    maps = sg.compact()
    assert [m.shape[0] for m in maps] == [70, 0, 5] and maps[2].tolist() == [0, -1, 1, 2, 3] and sg.span == 72
    state = sg.state_dict()
    assert state["shards"] == 3 and state["first"] == 0 and [s["count"] for s in state["states"]] == [68, 0, 4]
    with pytest.raises(ValueError, match="load_state_dict"):
        S(shards=sg.shards[:2]).load_state_dict(state)
    sg.clear()
    assert len(sg) == 0 and sg.span == 0
    for bad in (3, -1):                                                                         # (adding needs the device: only shard= here)
        with pytest.raises(ValueError, match="shard"):
            sg.add_features(torch.zeros(1, 64), shard=bad)


def test_groups_route_by_label_and_validate_finds_a_group_on_two_shards(model):
    from centerclip_amd.search_sharded import ShardedGallery
    shards = _shards(model, (7, 0, 5), side="text", grouped=True)                               # labels 0 0 0 1 1 1 2 | | 200 200 200 201 201
    sg = ShardedGallery(shards=shards)
    sg.validate()
    heads = sg._label_targets([201, 1, 9, 200], 4, "rank_groups")
    assert [h.tolist() for h in heads] == [[-1, 3, -1, -1], [-1, -1, -1, -1], [3, -1, -1, 0]] and heads[0].dtype == torch.int32
    with pytest.raises(ValueError, match="per query"):
        sg._label_targets([1, 2], 3, "rank_groups")
    with pytest.raises(ValueError, match="LongTensor"):
        sg.rank_groups_features(torch.zeros(1, 4, 64), torch.zeros(1, dtype=torch.long, device="meta"))
    masks = sg.row_mask(groups=[1, 201])
    assert [m.tolist() for m in masks] == [[0b0111000], [], [0b11000]]
    with pytest.raises(ValueError, match="label 9"):
        sg.row_mask(groups=[1, 9])
    with pytest.raises(ValueError, match="label 9"):
        sg.remove_groups([200, 9])
    assert len(sg) == 12                                                                        # refused: nothing changed
    sg.remove_groups([200, 0])
    assert [len(g) for g in shards] == [4, 0, 2]
    with pytest.raises(ValueError, match="label 200"):                                          # no row of it is held any more
        sg.remove_groups([200])
    shards[1]._append(_rows(2), [1, 1])                                                         # label 1 now lies on shards 0 and 1
    with pytest.raises(ValueError, match="labelled 1 has rows on shards 0 and 1"):
        sg.validate()
    shards[1].clear()
    shards[1]._append(_rows(1), [0])                                                            # a removed row keeps its label until compact()
    with pytest.raises(ValueError, match="labelled 0"):
        sg.validate()
    shards[0].compact()
    sg.validate()


def test_the_cursor_each_shard_is_handed():
    """(s, p_t) on the cursor's own shard; (s, 2^31 - 1) in front of it; (nextafter(s + 0.0, +inf), 2^31 - 1) behind it, a NaN
    for s = +inf (its key lies above every score's); -1 for the fill.  Pure tensor arithmetic: checked here on the host."""
    from centerclip_amd.search_sharded import ShardedGallery
    sg = ShardedGallery.__new__(ShardedGallery)
    inf = float("inf")
    s = torch.tensor([1.5, -0.0, inf, -inf, 3.0, -2.0])
    gid = torch.tensor([(1 << 32) | 7, (1 << 32) | 0, (1 << 32) | 2, (1 << 32) | 3, -1, 5])
    front, own, behind = (sg._shard_cursor((s, gid), r, "cpu") for r in (0, 1, 2))
    assert all(p.dtype == torch.int32 and c.dtype == torch.float32 for c, p in (front, own, behind))
    assert front[1].tolist() == [FRONT_ALL] * 4 + [-1, 5] and own[1].tolist() == [7, 0, 2, 3, -1, FRONT_ALL]
    assert behind[1].tolist() == [FRONT_ALL] * 4 + [-1, FRONT_ALL]
    real = [0, 1, 2, 3, 5]                                                                      # (a fill cursor's score is never read)
    assert torch.equal(front[0][real].view(torch.int32), s[real].view(torch.int32))             # the score as it came
    up = np.nextafter(np.float32([1.5, 0.0, -inf, -2.0]), np.float32(inf))
    assert torch.equal(own[0][:4].view(torch.int32), s[:4].view(torch.int32))
    assert own[0][5].item() == np.nextafter(np.float32(-2.0), np.float32(inf))                  # shard 1 lies behind shard 0's cursor
    got = behind[0].numpy()
    assert got[[0, 1, 3, 5]].tolist() == up.tolist() and got[1] > 0 and np.isnan(got[2]) and not np.signbit(got[2])
    # the keys: every score's key lies below the NaN's, and the raised bound lies above all keys of s and below the next score
    assert ordered_bits(got[2:3])[0] > ordered_bits([inf])[0]
    assert ordered_bits(got[0:1])[0] == ordered_bits([1.5])[0] + 1
