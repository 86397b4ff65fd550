"""Masked search without a GPU: the NumPy reference rankings the GPU checks compare against (pinned on a hand-written
example), every early return of cc_similarity_topk_masked_planes_f32 / cc_dsl_col_stats_planes_masked_f32 /
cc_pack_row_mask_u8 and their order (the checks end before anything is read or launched, so never-dereferenced addresses
do), the workspace query, the ops' fake kernels and ValueErrors, and FeatureGallery's removal bookkeeping on a stub."""
import ctypes

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_grouped_host import _bare, _meta, _p, grouped_topk_ref, model  # noqa: F401  (model: the fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def pack_bits(flags):
    """bool [..., n] -> int32 [..., ceil(n / 32)]: bit b of word w = flag 32 w + b (the ops' mask format)"""
    flags = np.asarray(flags, dtype=bool)
    words = -(-flags.shape[-1] // 32)
    padded = np.zeros(flags.shape[:-1] + (32 * words,), dtype=bool)
    padded[..., :flags.shape[-1]] = flags
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<i4").astype(np.int32)


def masked_topk_ref(S, sel, k, head=None):
    """The reference ranking.  S [Nq, n] scores, sel bool [n] or [Nq, n] (True = selectable), head [n] or None ->
    (scores [Nq, k] of S's dtype, ids [Nq, k] int64): per query row the matrix with the unselectable columns DROPPED, its
    stable descending order (head: grouped_topk_ref over those columns, so a group without a selectable row is left out and
    the others are ranked by their best selectable row), ids mapped back to the columns of S, then the fill (-inf, -1)."""
    S, sel = np.asarray(S), np.asarray(sel, dtype=bool)
    sel = np.broadcast_to(sel, S.shape)
    scores = np.full((S.shape[0], k), -np.inf, dtype=S.dtype)
    ids = np.full((S.shape[0], k), -1, dtype=np.int64)
    for q in range(S.shape[0]):
        cols = np.flatnonzero(sel[q])
        sub = S[q:q + 1, cols]
        if head is None:
            order = np.argsort(-sub, axis=1, kind="stable")[0, :k]
        else:
            order = grouped_topk_ref(sub, np.asarray(head)[cols], k)[1][0]
            order = order[order >= 0]
        ids[q, :len(order)] = cols[order]
        scores[q, :len(order)] = sub[0, order]
    return scores, ids


def test_the_reference_ranking_on_a_hand_written_example():
    S = np.array([[1, 5, 5, 2, 5, 3, 0, -0.0, 4],
                  [-1, -1, -1, 7, -3, -2, 7, 7, 9]], dtype=np.float32)
    inf = np.float32("-inf")
    sel = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)                  # rows 1, 4, 8 may not be ranked
    scores, ids = masked_topk_ref(S, sel, 4)
    assert ids.tolist() == [[2, 5, 3, 0], [3, 6, 7, 0]] and scores.tolist() == [[5, 3, 2, 1], [7, 7, 7, -1]]
    scores, ids = masked_topk_ref(S, sel, 8)                                 # 6 selectable rows: the fill behind them
    assert ids.tolist() == [[2, 5, 3, 0, 6, 7, -1, -1], [3, 6, 7, 0, 2, 5, -1, -1]]
    assert scores[0, 6:].tolist() == [inf, inf] and np.signbit(scores[0, 5]) and not np.signbit(scores[0, 4])
    assert masked_topk_ref(S, np.ones(9, dtype=bool), 9)[1].tolist() == np.argsort(-S, axis=1, kind="stable").tolist()
    none = masked_topk_ref(S, np.zeros(9, dtype=bool), 2)
    assert none[1].tolist() == [[-1, -1], [-1, -1]] and np.isneginf(none[0]).all()
    per_query = np.stack([sel, ~sel])                                        # one mask per query row
    assert masked_topk_ref(S, per_query, 3)[1].tolist() == [[2, 5, 3], [8, 1, 4]]
    # groups of 3, 1, 2, 3 rows: group 0 loses its best row (1), group 2 (rows 4, 5) its head, group 3 its last row
    head = np.array([0, 0, 0, 3, 4, 4, 6, 6, 6])
    scores, ids = masked_topk_ref(S, sel, 5, head)
    assert ids.tolist() == [[2, 5, 3, 6, -1], [3, 6, 0, 5, -1]] and scores.tolist() == [[5, 3, 2, 0, inf], [7, 7, -1, -2, inf]]
    dead_group = sel & (head != 6)                                           # a group none of whose rows is selectable
    assert masked_topk_ref(S, dead_group, 5, head)[1].tolist() == [[2, 5, 3, -1, -1], [3, 0, 5, -1, -1]]
    # the mask format: bit b of word w = row 32 w + b
    assert pack_bits(sel).tolist() == [0b011101101] and pack_bits(np.ones(33, dtype=bool)).tolist() == [-1, 1]
    assert pack_bits(per_query).shape == (2, 1)


# ------------------------------------------------------------------------------------------------ the library
def _masked(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=10, mask=256, mask_rows=1, words=4, m=0, s=0, side=1,
            n_total=100, head=0, scores=256, ids=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
    return lib.cc_similarity_topk_masked_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, k, _p(mask), mask_rows, words, _p(m),
                                                    _p(s), side, n_total, _p(head), _p(scores), _p(ids), _p(ws), ws_bytes, None)


@pytest.mark.parametrize("extra", [dict(), dict(m=256, s=256), dict(head=256), dict(m=256, s=256, head=256),
                                   dict(mask_rows=4), dict(mask_rows=4, m=256, s=256, side=0, head=256)])
def test_masked_entry_refuses_before_touching_memory_in_the_plain_entrys_order(extra):
    lib = L.lib()
    call = lambda **kw: _masked(lib, **dict(extra, **kw))
    for null in ("q", "g", "scores", "ids", "mask"):
        assert call(**{null: 0}) == INVALID, null
    own = [dict(mask_rows=0), dict(mask_rows=2), dict(mask_rows=5), dict(mask_rows=-1), dict(words=3), dict(words=0),
           dict(m=256, s=0), dict(m=0, s=256)]
    if "m" in extra:
        own += [dict(n_total=-1), dict(side=2), dict(side=-1)]
    for kw in [dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(Bg=-5), dict(E=-64)] + own:
        assert call(**kw) == INVALID, kw
    assert call(Bg=97, words=4) != INVALID and call(Bg=96, words=3, ws_bytes=0) == WORKSPACE     # ceil(Bg / 32) words
    for kw in (dict(k=0), dict(k=129), dict(k=-3), dict(products=0), dict(products=4), dict(E=96), dict(E=1088),
               dict(E=1024, products=3, k=128), dict(Bq=16 * 65535 + 1, mask_rows=1)):
        assert call(**kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_topk_workspace_bytes(4, 100, 10)
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws=0) == WORKSPACE
    # the order: invalid (the mask's refusals included) before unsupported before the workspace
    assert call(mask=0, k=129, ws=0) == INVALID and call(words=3, E=96, ws_bytes=0) == INVALID
    assert call(mask_rows=3, k=129) == INVALID and call(m=256, s=0, k=129) == INVALID
    assert call(k=129, ws=0) == UNSUPPORTED and call(E=1024, products=3, k=128, ws=0) == UNSUPPORTED
    for kw in (dict(E=1024, products=3, k=127), dict(E=1024, products=2, k=128), dict(E=768, products=3, k=128)):
        assert call(ws_bytes=0, **kw) == WORKSPACE, kw


def test_without_statistics_their_arguments_are_not_looked_at():
    lib = L.lib()
    assert _masked(lib, n_total=-1, side=7, ws_bytes=0) == WORKSPACE        # m == s == NULL ranks S
    assert _masked(lib, Bq=1, mask_rows=1, ws_bytes=0) == WORKSPACE         # Bq == 1: one mask row is both forms


def test_masked_statistics_and_pack_entries_refuse_before_touching_memory():
    lib = L.lib()

    def stats(t=256, v=256, Bt=100, Bv=7, E=64, products=2, mask=256, m=256, s=256, ws=256, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = lib.cc_dsl_col_stats_planes_workspace_bytes(Bt, Bv)
        return lib.cc_dsl_col_stats_planes_masked_f32(_p(t), _p(v), Bt, Bv, E, 1.0, products, _p(mask), _p(m), _p(s), _p(ws),
                                                      ws_bytes, None)
    for null in ("t", "v", "m", "s", "mask"):
        assert stats(**{null: 0}) == INVALID, null
    for kw in (dict(Bt=-1), dict(Bv=0), dict(E=0)):
        assert stats(**kw) == INVALID, kw
    for kw in (dict(products=0), dict(products=4), dict(E=96), dict(E=1088), dict(Bv=16 * 65535 + 1)):
        assert stats(**kw) == UNSUPPORTED, kw
    assert stats(ws=0) == WORKSPACE and stats(ws_bytes=lib.cc_dsl_col_stats_planes_workspace_bytes(100, 7) - 1) == WORKSPACE
    assert stats(mask=0, E=96, ws=0) == INVALID and stats(E=96, ws=0) == UNSUPPORTED

    pack = lambda f=256, R=2, n=100, out=256, W=4: lib.cc_pack_row_mask_u8(_p(f), R, n, _p(out), W, None)
    for kw in (dict(f=0), dict(out=0), dict(R=0), dict(R=-1), dict(n=0), dict(n=-3), dict(W=3), dict(n=129, W=4)):
        assert pack(**kw) == INVALID, kw


def test_the_workspace_is_the_plain_ops():
    lib = L.lib()
    for Bq, Bg, k in ((1, 1, 1), (16, 4099, 10), (17, 4099, 128), (16, 200003, 10)):
        w = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
        words = (Bg + 31) // 32
        for extra in (dict(), dict(mask_rows=Bq), dict(m=256, s=256), dict(head=256)):
            assert _masked(lib, Bq=Bq, Bg=Bg, k=k, words=words, ws_bytes=w - 1, **extra) == WORKSPACE
    assert lib.cc_similarity_topk_slices(16, 4099, 10) == 8                # (the GPU tests' several-slices shape)


# ------------------------------------------------------------------------------------------------ the ops
def _words(*shape):
    return torch.empty(*shape, device="meta", dtype=torch.int32)


def test_fake_kernels_give_shapes_on_the_meta_device():
    for name in ("similarity_topk_masked", "dsl_col_stats_planes_masked", "pack_row_mask"):
        assert name in torch_ops.OPS
    op = torch.ops.centerclip
    q, g = _meta(40), _meta(1000)
    head = torch.empty(1000, device="meta", dtype=torch.int32)
    stat = torch.empty(1000, device="meta")
    for scores, ids in (op.similarity_topk_masked(q, g, 900, 20.0, 2, 17, _words(29)),
                        op.similarity_topk_masked(q, g, 900, 20.0, 2, 17, _words(40, 32)),
                        op.similarity_topk_masked(q, g, 900, 20.0, 2, 17, _words(29), stat, stat, 1, 900),
                        op.similarity_topk_masked(q, g, 900, 20.0, 2, 17, _words(40, 29), stat[:40], stat[:40], 0, 900, head),
                        op.similarity_topk_masked(q, g, 900, 20.0, 2, 17, _words(29), group_head=head)):
        assert scores.shape == (40, 17) and scores.dtype == torch.float32 and scores.device.type == "meta"
        assert ids.shape == (40, 17) and ids.dtype == torch.int64
    m, s = op.dsl_col_stats_planes_masked(g, q, 900, 40, 20.0, 2, _words(29))
    assert m.shape == s.shape == (40,) and m.dtype == s.dtype == torch.float32 and m.device.type == "meta"
    for flags, shape in ((torch.empty(3, 1000, device="meta", dtype=torch.bool), (3, 32)),
                         (torch.empty(65, device="meta", dtype=torch.uint8), (1, 3))):
        out = op.pack_row_mask(flags)
        assert out.shape == shape and out.dtype == torch.int32 and out.device.type == "meta"
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        op.similarity_topk_masked(h(2), h(8), 8, 1.0, 2, 3, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        op.dsl_col_stats_planes_masked(h(8), h(2), 8, 2, 1.0, 2, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        op.pack_row_mask(torch.zeros(8, dtype=torch.bool))


def test_ops_refuse_masks_that_do_not_fit():
    op = torch.ops.centerclip
    q, g = _meta(4), _meta(100)
    stat = torch.empty(100, device="meta")
    head = torch.empty(100, device="meta", dtype=torch.int32)
    call = lambda q=q, g=g, n=100, mask=_words(4), m=None, s=None, side=1, head=None: op.similarity_topk_masked(
        q, g, n, 1.0, 2, 5, mask, m, s, side, 100, head)
    call()
    call(mask=_words(4, 4))
    call(mask=_words(4, 9), m=stat, s=stat, head=head)
    for kw in (dict(mask=torch.empty(4, device="meta", dtype=torch.int64)),                 # not int32
               dict(mask=torch.empty(4, device="meta", dtype=torch.bool)),
               dict(mask=_words(8)[::2]), dict(mask=_words(4, 8)[:, ::2]),                  # not contiguous
               dict(mask=_words(3)), dict(mask=_words(4, 3)),                               # too few words
               dict(mask=_words(3, 4)), dict(mask=_words(5, 4)), dict(mask=_words(1, 4, 4)),   # mask rows not 1 or Bq
               dict(mask=torch.zeros(4, dtype=torch.int32)),                                # not on the planes' device
               dict(m=stat), dict(s=stat),                                                  # exactly one of m / s
               dict(m=stat[:99], s=stat), dict(m=stat[:3], s=stat[:3], side=0),
               dict(head=torch.empty(99, device="meta", dtype=torch.int32)),
               dict(n=101), dict(g=_meta(100, 384)), dict(g=_meta(100, dtype=torch.float32))):
        with pytest.raises(ValueError):
            call(**kw)
    stats = lambda t=g, v=q, nt=100, nv=4, mask=_words(4): op.dsl_col_stats_planes_masked(t, v, nt, nv, 1.0, 2, mask)
    stats()
    for kw in (dict(mask=_words(3)), dict(mask=_words(1, 4)), dict(mask=torch.empty(4, device="meta", dtype=torch.int64)),
               dict(mask=_words(8)[::2]), dict(mask=torch.zeros(4, dtype=torch.int32)), dict(nt=101), dict(nv=5)):
        with pytest.raises(ValueError):
            stats(**kw)
    for flags in (torch.empty(8, device="meta", dtype=torch.int32), torch.empty(2, 2, 8, device="meta", dtype=torch.bool),
                  torch.empty(3, 0, device="meta", dtype=torch.bool)):
        with pytest.raises(ValueError):
            op.pack_row_mask(flags)


# ------------------------------------------------------------------------------------------------ FeatureGallery
def _rows(n):
    return torch.arange(n, dtype=torch.float16)[:, None].expand(n, 192).contiguous()       # row i holds i: rows can be told apart


def _live_bitmap(gal):
    return pack_bits(np.ones(gal.span, dtype=bool) if gal._live is None else gal._live)


def test_remove_keeps_positions_and_refusals_change_nothing(model):
    gal = _bare(model)
    assert len(gal) == 0 and gal.span == 0 and gal._live is None
    gal._append(_rows(70))
    assert len(gal) == gal.span == 70 and set(gal.state_dict()) == {"rows", "count", "E", "side", "products"}
    gal.remove(3)
    gal.remove([0, 69, 33])
    gal.remove(torch.tensor([31, 32]))
    gal.remove([])
    want = np.ones(70, dtype=bool)
    want[[3, 0, 69, 33, 31, 32]] = False
    assert len(gal) == 64 and gal.span == 70 and np.array_equal(gal._live, want)
    assert gal._live_dev.dtype == torch.int32 and gal._live_dev[:3].tolist() == pack_bits(want).tolist() == _live_bitmap(gal).tolist()
    before = (gal._live.copy(), gal._live_dev.clone(), len(gal))
    for bad in (70, -1, [5, 70], [5, 5], 3, [4, 0], torch.tensor([31]), [1.5], [[1, 2]], "ab",
                torch.tensor([1], dtype=torch.int32), torch.zeros(1, dtype=torch.long, device="meta")):
        with pytest.raises(ValueError):
            gal.remove(bad)
    assert np.array_equal(gal._live, before[0]) and torch.equal(gal._live_dev, before[1]) and len(gal) == before[2]
    # rows added later get new positions behind span; the holes stay
    assert gal._append(_rows(30)).tolist() == list(range(70, 100))
    want = np.concatenate((want, np.ones(30, dtype=bool)))
    assert len(gal) == 94 and gal.span == 100 and np.array_equal(gal._live, want)
    assert gal._live_dev[:4].tolist() == pack_bits(want).tolist() and gal._live_dev.shape[0] >= -(-gal._rows.shape[0] // 32)
    gal.remove(99)
    want[99] = False
    assert gal._live_words().tolist() == pack_bits(want).tolist()
    # the state: one key more; clear() forgets the removals
    state = gal.state_dict()
    assert set(state) == {"rows", "count", "E", "side", "products", "live"} and state["count"] == 100
    assert state["live"].dtype == torch.bool and state["live"].device.type == "cpu" and state["live"].tolist() == want.tolist()
    with pytest.raises(ValueError):
        gal.row_mask(positions=[100])
    assert gal.row_mask().tolist() == pack_bits(np.ones(100, dtype=bool)).tolist()
    pick = np.zeros(100, dtype=bool)
    pick[[0, 31, 32, 64, 99]] = True
    assert gal.row_mask(positions=[99, 0, 31, 32, 64]).tolist() == pack_bits(pick).tolist()
    with pytest.raises(ValueError, match="grouped=True"):
        gal.row_mask(groups=[1])
    with pytest.raises(ValueError, match="grouped=True"):
        gal.remove_groups([1])
    gal.clear()
    assert len(gal) == gal.span == 0 and gal._live is None and set(gal.state_dict()) == {"rows", "count", "E", "side", "products"}
    gal._append(_rows(5))
    assert len(gal) == 5 and gal._live is None
    # load: refusals before anything is written, then the removals come back
    for bad in (state["live"][:99], state["live"].long(), state["live"].tolist()):
        with pytest.raises(ValueError):
            gal.load_state_dict(dict(state, live=bad))
    assert len(gal) == 5 and gal.span == 5 and gal._live is None
    gal.load_state_dict(state)
    assert len(gal) == 93 and gal.span == 100 and np.array_equal(gal._live, want)
    assert gal._live_words().tolist() == pack_bits(want).tolist()
    gal.load_state_dict({k: v for k, v in state.items() if k != "live"})
    assert len(gal) == 100 and gal._live is None


def test_compact_gives_the_map_and_the_gallery_of_the_survivors(model):
    gal = _bare(model, dual_softmax=True)
    gal._append(_rows(40))
    gal._m[:40], gal._s[:40] = torch.arange(40.), torch.arange(40.) + 100
    assert gal.compact().tolist() == list(range(40)) and len(gal) == 40       # nothing removed: nothing happens
    gone = [0, 5, 6, 31, 32, 39]
    gal.remove(gone)
    keep = [i for i in range(40) if i not in gone]
    new_pos = gal.compact()
    assert new_pos.dtype == torch.int64 and new_pos.device.type == "cpu"
    assert new_pos.tolist() == [keep.index(i) if i in keep else -1 for i in range(40)]
    assert len(gal) == gal.span == 34 and gal._live is None and "live" not in gal.state_dict()
    assert gal.rows[:, 0].tolist() == keep and gal._m[:34].tolist() == keep and gal._s[:34].tolist() == [100 + i for i in keep]
    assert gal._append(_rows(2)).tolist() == [34, 35]
    gal.remove(list(range(36)))
    assert len(gal) == 0 and gal.span == 36
    assert gal.compact().tolist() == [-1] * 36 and gal.span == 0


def test_group_bookkeeping_under_removals(model):
    from centerclip_amd.search import FeatureGallery
    gal = _bare(model, "text", grouped=True)
    labels = [7] * 4 + [4] * 2 + [9] * 3 + [-5] * 2                          # heads 0 0 0 0 4 4 6 6 6 9 9
    gal._append(_rows(11), labels)
    assert gal.num_groups == 4
    before = (gal._head.clone(), gal.labels.clone(), set(gal._closed), gal._open)
    for bad in ([8], [7, 8], 12, torch.tensor([8])):
        with pytest.raises(ValueError, match="label"):
            gal.remove_groups(bad)
    for bad in (torch.zeros(1, dtype=torch.long, device="meta"), torch.tensor([7], dtype=torch.int32), [0.5], [[7]]):
        with pytest.raises(ValueError, match="labels"):                      # no device tensor (it would have to be read)
            gal.remove_groups(bad)
        with pytest.raises(ValueError, match="labels"):
            gal.row_mask(groups=bad)
    assert gal.row_mask(groups=torch.tensor([4])).tolist() == pack_bits(np.asarray(labels) == 4).tolist()
    assert len(gal) == 11 and gal._live is None and (set(gal._closed), gal._open) == before[2:]
    gal.remove([0, 6])                                                       # a head row and another group's head row
    assert gal.num_groups == 4 and len(gal) == 9
    gal.remove_groups([4])
    assert gal.num_groups == 3 and len(gal) == 7 and gal._live.tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match="label"):
        gal.remove_groups(4)                                                 # no row held carries it any more
    with pytest.raises(ValueError, match="returns"):
        gal._append(_rows(1), 4)                                             # ... but the label stays refused
    assert gal.row_mask(groups=[9, 7]).tolist() == pack_bits([1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0]).tolist()
    assert gal.row_mask(positions=[4], groups=-5).tolist() == pack_bits([0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1]).tolist()
    with pytest.raises(ValueError, match="label"):
        gal.row_mask(groups=[8])
    gal._append(_rows(1), -5)                                                # the open group still continues
    assert gal._head[11].item() == 9 and gal.num_groups == 3
    gal.remove_groups(-5)                                                    # the last group goes: the next rows start a new one
    assert gal.num_groups == 2 and gal._open is None and -5 in gal._closed
    with pytest.raises(ValueError, match="returns"):
        gal._append(_rows(1), -5)
    gal._append(_rows(2), 11)
    assert gal._head[12:14].tolist() == [12, 12] and gal.num_groups == 3 and torch.equal(gal._head[:11], before[0][:11])
    # compact(): the map, and heads / label sets as _plan_groups gives them on the surviving labels
    surviving = [7, 7, 7, 9, 9, 11, 11]
    new_pos = gal.compact()
    assert new_pos.tolist() == [-1, 0, 1, 2, -1, -1, -1, 3, 4, -1, -1, -1, 5, 6]
    fresh = _bare(model, "text", grouped=True)
    _, heads, _ = fresh._plan_groups(surviving, 0, 7)
    fresh._append(_rows(7), surviving)
    assert gal._head[:7].tolist() == heads.tolist() == [0, 0, 0, 3, 3, 5, 5] and gal.labels.tolist() == surviving
    assert gal._label_dev[:7].tolist() == surviving and (gal._closed, gal._open, gal.num_groups) == (fresh._closed, fresh._open, 3)
    assert len(gal) == gal.span == 7 and gal.rows[:, 0].tolist() == [1, 2, 3, 7, 8, 0, 1]     # (_rows(2): 0, 1)
    gal._append(_rows(1), 4)                                                 # removed labels are free again
    state_keys = set(gal.state_dict())
    assert state_keys == {"rows", "count", "E", "side", "products", "grouped", "group_head", "labels"}
    gal.remove(7)
    state = gal.state_dict()
    assert set(state) == state_keys | {"live"}
    other = _bare(model, "text", grouped=True)
    other.load_state_dict(state)
    assert len(other) == 7 and other.span == 8 and other.num_groups == 3 and other._open is None and 4 in other._closed
    gal.clear()
    assert gal.num_groups == 0 and gal._live is None and len(gal) == 0
    assert isinstance(FeatureGallery.span, property)


def test_allow_is_checked_on_the_host(model):
    gal = _bare(model)
    gal._append(_rows(70))
    for bad in ([1, 0, 1], torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64),
                torch.zeros(69, dtype=torch.bool), torch.zeros(2, 71, dtype=torch.bool), torch.zeros(3, 3, dtype=torch.int32),
                torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="allow="):
            gal._allow_words(bad, 2)
    assert gal._allow_words(None, 2) is None
    empty = _bare(model)                                                     # no position in use: a bool allow= has nothing to pack
    assert empty._allow_words(torch.zeros(0, dtype=torch.bool), 2) is None
    assert empty._allow_words(torch.zeros(2, 0, dtype=torch.bool), 2) is None
    assert empty._allow_words(torch.zeros(1, dtype=torch.int32), 2).shape == (0,)
    with pytest.raises(ValueError, match="allow="):
        empty._allow_words(torch.zeros(3, dtype=torch.bool), 2)
    wide = torch.from_numpy(pack_bits(np.ones(128, dtype=bool)))             # wider than the positions in use: cut
    assert gal._allow_words(wide, 2).tolist() == [-1, -1, -1]
    gal.remove([1, 64])
    assert gal._allow_words(None, 2).tolist() == pack_bits(gal._live).tolist()
    got = gal._allow_words(torch.from_numpy(np.stack([pack_bits(np.arange(70) < 40), pack_bits(np.arange(70) >= 40)])), 2)
    assert got.tolist() == pack_bits(np.stack([(np.arange(70) < 40), (np.arange(70) >= 40)]) & gal._live).tolist()


# ------------------------------------------------------------------------------------------------ host integer arguments
ACCEPTED = (lambda: 1, lambda: np.int64(1), lambda: [1], lambda: (1,), lambda: torch.tensor([1]), lambda: torch.tensor(1),
            lambda: [])                                                       # int, NumPy int, list, tuple, 1-D, 0-D; empty
REFUSED = (lambda: [1.5], lambda: [[1, 2]], lambda: "ab", lambda: torch.tensor([1], dtype=torch.int32),
           lambda: torch.zeros(1, 1, dtype=torch.long), lambda: torch.zeros(1, dtype=torch.long, device="meta"))


def _count(value):
    """the queries (videos) an entry is asked about: one per value of an accepted form, one for a refused form"""
    return int(value.numel()) if torch.is_tensor(value) else len(value) if isinstance(value, (list, tuple)) else 1


def _lists(value):
    if isinstance(value, (list, tuple)):
        return [_lists(v) for v in value]
    return value.tolist() if hasattr(value, "tolist") else value


def _entries():
    """The entries that read host ints through ``search._host_ints`` -> (name, read, one, none, public): ``read(g, sg, v)``
    gives what the entry made of ``v`` as nested lists - through the method that does the reading where the public one goes
    on to the encoder, which refuses CPU tensors; ``one`` / ``none``: that for the value 1 / for no value; ``public``: the
    public call of the same entry, which must refuse what ``read`` refuses before anything is encoded.  Not here, because
    they keep their own reading: ``remove`` / ``row_mask(positions=)`` / ``windows`` (``_positions``), ``remove_groups`` /
    ``row_mask(groups=)`` (``_label_list``) and the labels of ``add*(group=)`` (``_plan_groups``)."""
    from centerclip_amd.search import window_table
    ids = lambda v: torch.zeros(_count(v), 16, dtype=torch.long)
    table = lambda v: window_table([4] * _count(v), 1, 4)                    # one window per video
    clips = lambda g, v: torch.zeros(_count(v), 1, int(g.core.video_frames), 3, 8, 8)
    sizes = lambda sg: [len(g) for g in sg.shards]
    return (("rank(target=)", lambda g, sg, v: g._targets(v, _count(v), "rank"), [1], [],
             lambda g, sg, v: g.rank(ids(v), target=v)),
            ("rank_groups(target=)", lambda g, sg, v: g._group_targets(v, _count(v)), [3], [],
             lambda g, sg, v: g.rank_groups(ids(v), target=v)),
            ("add_windows(group=)", lambda g, sg, v: np.atleast_1d(g._window_groups(v, table(v), _count(v), "add_windows")), [1], [],
             lambda g, sg, v: g.add_windows(clips(g, v), [clips(g, v).shape[2]] * _count(v), clips(g, v).shape[2], group=v)),
            ("window_table(lengths=)", lambda g, sg, v: window_table(v, 1, 1), [[0, 0, 1]], [], None),
            ("ShardedGallery.remove", lambda g, sg, v: (sg.remove(v), sizes(sg))[1], [3, 4], [4, 4], None),
            ("ShardedGallery.row_mask(positions=)", lambda g, sg, v: sg.row_mask(positions=v), [[2], [0]], [[0], [0]], None),
            ("ShardedGallery.remove_groups", lambda g, sg, v: (sg.remove_groups(v), sizes(sg))[1], [3, 4], [4, 4], None),
            ("ShardedGallery.row_mask(groups=)", lambda g, sg, v: sg.row_mask(groups=v), [[8], [0]], [[0], [0]], None),
            ("ShardedGallery.rank(target=)", lambda g, sg, v: sg._row_targets(v, _count(v), "rank"), [1], [],
             lambda g, sg, v: sg.rank(ids(v), target=v)),
            ("ShardedGallery.rank_groups(target=)", lambda g, sg, v: sg._label_targets(v, _count(v), "rank_groups"), [[3], [-1]],
             [[], []], lambda g, sg, v: sg.rank_groups(ids(v), target=v)))


def _snapshot(*galleries):
    return [(len(g), g.span, {k: v.clone() if torch.is_tensor(v) else v for k, v in g.state_dict().items()}) for g in galleries]


def _same_snapshot(a, b):
    for (la, sa, da), (lb, sb, db) in zip(a, b):
        assert (la, sa, set(da)) == (lb, sb, set(db))
        assert all(torch.equal(da[k], db[k]) if torch.is_tensor(da[k]) else da[k] == db[k] for k in da)


@pytest.mark.parametrize("name,read,one,none,public", _entries(), ids=[e[0] for e in _entries()])
def test_every_host_int_argument_reads_the_same_forms(model, name, read, one, none, public):
    """One parser: every form of the value 1 that ``remove`` accepts is read as that 1 by each of these entries, the empty
    list as no value, and what ``remove`` refuses they refuse - by ``read`` and by the public call alike, nothing changed.
    ``rank(target=)`` has a second form, a device integer tensor passed through unread, so there the device LongTensor is no
    host form at all (tests/test_search_rank_host.py and test_search_sharded_host.py hold the refusals of that form)."""
    from centerclip_amd.search_sharded import ShardedGallery

    def galleries():                                 # g and shard 0: labels 0 0 0 1 - the value 1 is a position and a label
        made = [_bare(model, grouped=True) for _ in range(3)]
        for g, first in zip(made, (0, 0, 20)):
            g._append(_rows(4), [first, first, first, first + 1])
        return made[0], ShardedGallery(shards=made[1:])
    for form in ACCEPTED:
        g, sg = galleries()
        assert _lists(read(g, sg, form())) == (one if _count(form()) else none), form()
        if public is not None and (_count(form()) or "windows" not in name):       # (no video at all: add_windows refuses that first)
            with pytest.raises(L.CenterClipHipError):                        # every host check passed: CPU tensors are refused next
                public(*galleries(), form())
    g, sg = galleries()
    before = _snapshot(g, *sg.shards)
    for form in REFUSED[:-1] if name.endswith("rank(target=)") else REFUSED:  # (the last one is the device tensor)
        for call in (read, public) if public is not None else (read,):
            with pytest.raises(ValueError, match="CPU LongTensor"):
                call(g, sg, form())
    _same_snapshot(before, _snapshot(g, *sg.shards))
