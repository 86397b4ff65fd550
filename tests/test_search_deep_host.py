"""Deep lists and cursors without a GPU: every early return of cc_similarity_topk_deep_planes_f32 and their order (the checks
end before anything is read or launched, so never-dereferenced addresses do), the workspace query (one page and the cursor
buffer, whatever the number of pages), the op's fake kernel and ValueErrors, and FeatureGallery's refusals of ``after=`` and
of a k beyond 4096 on a stub."""
import re

import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_grouped_host import _bare, _meta, _p, model  # noqa: F401  (model: the fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
MAXK = 4096


def _deep(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=300, mask=0, mask_rows=1, words=4, m=0, s=0, side=1, n_total=100,
          head=0, after_scores=0, after_ids=0, scores=256, ids=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_deep_workspace_bytes(Bq, Bg, E, products, k)
    return lib.cc_similarity_topk_deep_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, k, _p(mask), mask_rows, words, _p(m),
                                                  _p(s), side, n_total, _p(head), _p(after_scores), _p(after_ids), _p(scores),
                                                  _p(ids), _p(ws), ws_bytes, None)


def test_the_header_declares_the_entries_and_the_cap():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "centerclip_hip.h")).read()
    assert re.search(r"#define\s+CC_TOPK_DEEP_MAXK\s+4096\b", text) and torch_ops.TOPK_DEEP_MAXK == MAXK
    for name in ("cc_similarity_topk_deep_planes_f32", "cc_similarity_topk_deep_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(L.lib(), name)


@pytest.mark.parametrize("extra", [dict(), dict(mask=256), dict(mask=256, mask_rows=4), dict(m=256, s=256), dict(head=256),
                                   dict(after_scores=256, after_ids=256),
                                   dict(mask=256, mask_rows=4, m=256, s=256, side=0, head=256, after_scores=256, after_ids=256)])
def test_entry_refuses_before_touching_memory(extra):
    lib = L.lib()
    call = lambda **kw: _deep(lib, **dict(extra, **kw))
    for null in ("q", "g", "scores", "ids"):
        assert call(**{null: 0}) == INVALID, null
    own = [dict(k=0), dict(k=-3), dict(m=256, s=0), dict(m=0, s=256), dict(after_scores=256, after_ids=0),
           dict(after_scores=0, after_ids=256)]
    if "mask" in extra:
        own += [dict(mask_rows=0), dict(mask_rows=2), dict(mask_rows=5), dict(mask_rows=-1), dict(words=3), dict(words=0)]
    if "m" in extra:
        own += [dict(n_total=-1), dict(side=2), dict(side=-1)]
    for kw in [dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(Bg=-5), dict(E=-64)] + own:
        assert call(**kw) == INVALID, kw
    for kw in (dict(k=MAXK + 1), dict(products=0), dict(products=4), dict(E=96), dict(E=1088), dict(Bq=16 * 65535 + 1, mask_rows=1)):
        assert call(ws_bytes=1 << 40, **kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_topk_deep_workspace_bytes(4, 100, 64, 2, 300)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws=0) == WORKSPACE
    # the order: invalid before unsupported before the workspace
    assert call(q=0, k=MAXK + 1, ws=0) == INVALID and call(after_scores=256, after_ids=0, E=96, ws_bytes=0) == INVALID
    assert call(m=256, s=0, k=MAXK + 1) == INVALID and call(k=0, products=4) == INVALID
    assert call(k=MAXK + 1, ws=0) == UNSUPPORTED and call(E=96, ws_bytes=0) == UNSUPPORTED
    # every (E, products) the plain entry supports at some k, and every k up to the cap, passes the limits
    for kw in (dict(E=1024, products=3), dict(E=1024, products=3, k=128), dict(E=1024, products=2), dict(E=768, products=3),
               dict(k=1), dict(k=128), dict(k=129), dict(k=MAXK)):
        assert call(ws_bytes=0, **kw) == WORKSPACE, kw


def test_without_a_mask_or_statistics_their_arguments_are_not_looked_at():
    lib = L.lib()
    assert _deep(lib, mask_rows=7, words=0, ws_bytes=0) == WORKSPACE       # row_mask == NULL: every row is selectable
    assert _deep(lib, n_total=-1, side=7, ws_bytes=0) == WORKSPACE         # m == s == NULL ranks S


def test_the_workspace_is_one_page_and_the_cursors():
    lib = L.lib()
    deep, plain = lib.cc_similarity_topk_deep_workspace_bytes, lib.cc_similarity_topk_workspace_bytes
    for Bq, Bg, E, products in ((1, 1, 64, 1), (4, 100, 64, 2), (16, 4099, 64, 3), (17, 200003, 512, 2), (16, 1 << 20, 768, 3),
                                (33, 4099, 1024, 3)):
        page = 127 if (E, products) == (1024, 3) else 128          # the longest list the stream's LDS holds
        want = plain(Bq, Bg, page) + -(-Bq * 8 // 256) * 256
        sizes = {k: deep(Bq, Bg, E, products, k) for k in (128, 129, 130, 256, 1000, MAXK)}
        assert sizes[129] == sizes[MAXK] == want, (Bq, Bg, E, products, sizes, want)
        assert len(set(sizes[k] for k in (129, 130, 256, 1000, MAXK))) == 1         # it does not grow with the pages
        assert sizes[128] == want                                                    # (k = 128 at page 127: two pages)
        assert deep(Bq, Bg, E, products, 10) == plain(Bq, Bg, 10) + -(-Bq * 8 // 256) * 256      # a short list: a short page
        assert _deep(lib, Bq=Bq, Bg=Bg, E=E, products=products, k=MAXK, ws_bytes=want - 1) == WORKSPACE
    # well below the matrix: 16 queries over a million rows, 4096 entries each
    assert deep(16, 1 << 20, 512, 2, MAXK) < 16 * (1 << 20) * 4 // 4
    for bad in ((0, 100, 64, 2, 300), (4, 0, 64, 2, 300), (4, 100, 96, 2, 300), (4, 100, 1088, 2, 300), (4, 100, 64, 0, 300),
                (4, 100, 64, 4, 300), (4, 100, 64, 2, 0), (4, 100, 64, 2, MAXK + 1)):
        assert deep(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the op
def _words(*shape):
    return torch.empty(*shape, device="meta", dtype=torch.int32)


def test_fake_kernel_gives_shapes_on_the_meta_device():
    assert "similarity_topk_deep" in torch_ops.OPS
    op = torch.ops.centerclip
    q, g = _meta(40), _meta(1000)
    head = torch.empty(1000, device="meta", dtype=torch.int32)
    stat = torch.empty(1000, device="meta")
    a_s, a_i = torch.empty(40, device="meta"), torch.empty(40, device="meta", dtype=torch.int64)
    for k in (1, 128, 129, 1000, MAXK):
        for scores, ids in (op.similarity_topk_deep(q, g, 900, 20.0, 2, k),
                            op.similarity_topk_deep(q, g, 900, 20.0, 2, k, _words(29)),
                            op.similarity_topk_deep(q, g, 900, 20.0, 2, k, _words(40, 32), stat, stat, 1, 900),
                            op.similarity_topk_deep(q, g, 900, 20.0, 2, k, None, stat[:40], stat[:40], 0, 900, head),
                            op.similarity_topk_deep(q, g, 900, 20.0, 2, k, after_scores=a_s, after_ids=a_i),
                            op.similarity_topk_deep(q, g, 900, 20.0, 2, k, group_head=head, after_scores=a_s, after_ids=a_i.int()),
                            op.similarity_topk_deep(q, g, 0, 20.0, 2, k)):
            assert scores.shape == (40, k) and scores.dtype == torch.float32 and scores.device.type == "meta"
            assert ids.shape == (40, k) and ids.dtype == torch.int64
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        op.similarity_topk_deep(h(2), h(8), 8, 1.0, 2, 300)
    with pytest.raises(NotImplementedError):
        op.similarity_topk_deep(h(2), h(8), 8, 1.0, 2, 300, after_scores=torch.zeros(2), after_ids=torch.zeros(2, dtype=torch.long))


def test_op_refuses_arguments_that_do_not_fit():
    op = torch.ops.centerclip
    q, g = _meta(4), _meta(100)
    stat = torch.empty(100, device="meta")
    a_s, a_i = torch.empty(4, device="meta"), torch.empty(4, device="meta", dtype=torch.int64)
    call = lambda q=q, g=g, n=100, k=300, mask=None, m=None, s=None, side=1, head=None, a_s=None, a_i=None: \
        op.similarity_topk_deep(q, g, n, 1.0, 2, k, mask, m, s, side, 100, head, a_s, a_i)
    call()
    call(a_s=a_s, a_i=a_i)
    call(mask=_words(4, 4), m=stat, s=stat, a_s=a_s, a_i=a_i.int())
    for kw in (dict(k=0), dict(k=-3), dict(k=MAXK + 1),
               dict(a_s=a_s), dict(a_i=a_i),                                                # exactly one of the pair
               dict(a_s=a_s[:3], a_i=a_i[:3]), dict(a_s=a_s, a_i=a_i[:3]), dict(a_s=a_s[:, None], a_i=a_i[:, None]),
               dict(a_s=a_s.double(), a_i=a_i), dict(a_s=a_s.half(), a_i=a_i), dict(a_s=a_s, a_i=a_s), dict(a_s=a_i, a_i=a_i),
               dict(a_s=torch.zeros(4), a_i=a_i), dict(a_s=a_s, a_i=torch.zeros(4, dtype=torch.long)),      # not on the planes' device
               dict(mask=_words(3)), dict(mask=_words(5, 4)), dict(mask=torch.zeros(4, dtype=torch.int32)),   # the masked op's checks
               dict(m=stat), dict(s=stat), dict(m=stat[:3], s=stat[:3]),
               dict(head=torch.empty(99, device="meta", dtype=torch.int32)),
               dict(n=101), dict(g=_meta(100, 384)), dict(g=_meta(100, dtype=torch.float32))):
        with pytest.raises(ValueError):
            call(**kw)


# ------------------------------------------------------------------------------------------------ FeatureGallery
def _rows(n):
    return torch.arange(n, dtype=torch.float16)[:, None].expand(n, 192).contiguous()


def test_gallery_refuses_k_and_cursors_before_anything_is_encoded(model):
    """on a stub without a device: a ValueError means the check ran before anything was encoded or launched (what comes next
    there is the refusal of CPU tensors, CenterClipHipError)"""
    seq, ids = torch.zeros(3, 1, 64), torch.zeros(3, 16, dtype=torch.long)
    vis, vmask = torch.zeros(3, 4, 64), torch.ones(3, 4, dtype=torch.long)
    plain, grouped = _bare(model), _bare(model, "text", grouped=True)
    plain._append(_rows(70))
    grouped._append(_rows(11), [7] * 4 + [4] * 2 + [9] * 3 + [-5] * 2)
    calls = [lambda **kw: plain.search(ids, **kw), lambda **kw: plain.search_features(seq, **kw),
             lambda **kw: grouped.search_groups(vis, vmask, **kw), lambda **kw: grouped.search_groups_features(vis, mask=vmask, **kw),
             lambda **kw: grouped.search(vis, vmask, **kw), lambda **kw: grouped.search_features(vis, mask=vmask, **kw)]
    sc, pos = torch.zeros(3), torch.zeros(3, dtype=torch.long)
    for call in calls:
        for k in (0, -3, MAXK + 1):
            with pytest.raises(ValueError, match="k <= 4096"):
                call(k=k)
        for bad in (sc, (sc,), (sc, pos, pos), (sc, [0, 1, 2]), ([0., 0., 0.], pos), "ab", 5,
                    (sc[:2], pos[:2]), (sc, pos[:2]), (sc[:, None], pos[:, None]), (sc[0], pos[0]),     # one pair per query
                    (sc.double(), pos), (sc.half(), pos), (sc, sc), (pos, pos), (sc, pos.short()),   # fp32 scores, int32 / int64 positions
                    (sc.to("meta"), pos), (sc, pos.to("meta")), (sc.to("meta"), pos.to("meta"))):   # on the gallery's device
            with pytest.raises(ValueError, match="after="):
                call(k=5, after=bad)
        for kw in (dict(k=1), dict(k=128), dict(k=129), dict(k=MAXK), dict(k=5, after=(sc, pos)), dict(k=300, after=(sc, pos.int()))):
            with pytest.raises(L.CenterClipHipError):                          # accepted: CPU tensors are refused next
                call(**kw)
    with pytest.raises(ValueError, match="grouped=True"):
        plain.search_groups_features(seq, k=300, after=(sc, pos))
    assert len(plain) == 70 and len(grouped) == 11


def test_an_empty_gallery_gives_the_fill_of_the_new_range(model):
    empty = _bare(model)
    q = torch.zeros(3, 192, dtype=torch.float16)
    for kw in (dict(k=1), dict(k=129), dict(k=MAXK), dict(k=7, after=(torch.zeros(3), torch.zeros(3, dtype=torch.long)))):
        scores, ids = empty._search_rows(q, **kw)
        assert scores.shape == ids.shape == (3, kw["k"]) and ids.dtype == torch.int64
        assert bool(torch.isneginf(scores).all()) and bool((ids == -1).all())
    with pytest.raises(ValueError, match="k <= 4096"):
        empty.search_features(torch.zeros(3, 1, 64), k=MAXK + 1)
