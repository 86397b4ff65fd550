"""Dual-softmax search without a GPU: every early return of cc_dsl_col_stats_planes_f32 and cc_similarity_topk_dsl_planes_f32 and
their order (the checks end before anything is read or launched, so never-dereferenced addresses do), the plan queries, the
ops' fake kernels, and FeatureGallery(dual_softmax=True)'s refusals."""
import ctypes

import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops
from test_search_host import _cpu_model

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _p(v):
    return ctypes.c_void_p(v) if v else None                               # (addresses that are never dereferenced)


def _stats(lib, text=256, video=256, Bt=100, Bv=7, E=64, products=2, m=256, s=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_dsl_col_stats_planes_workspace_bytes(Bt, Bv)
    return lib.cc_dsl_col_stats_planes_f32(_p(text), _p(video), Bt, Bv, E, 1.0, products, _p(m), _p(s), _p(ws), ws_bytes, None)


def _topk(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=10, m=256, s=256, side=1, n_total=100, scores=256, ids=256,
          ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
    return lib.cc_similarity_topk_dsl_planes_f32(_p(q), _p(g), Bq, Bg, E, 1.0, products, k, _p(m), _p(s), side, n_total,
                                                 _p(scores), _p(ids), _p(ws), ws_bytes, None)


def test_statistics_entry_refuses_before_touching_memory():
    lib = L.lib()
    for null in ("text", "video", "m", "s"):
        assert _stats(lib, **{null: 0}) == INVALID, null
    for kw in (dict(Bt=-1), dict(Bv=0), dict(Bv=-4), dict(E=0), dict(E=-64)):
        assert _stats(lib, **kw) == INVALID, kw
    for kw in (dict(products=0), dict(products=4), dict(E=96), dict(E=1088), dict(Bv=16 * 65535 + 1)):
        assert _stats(lib, **kw) == UNSUPPORTED, kw
    need = lib.cc_dsl_col_stats_planes_workspace_bytes(100, 7)
    assert need > 0
    assert _stats(lib, ws_bytes=need - 1) == WORKSPACE
    assert _stats(lib, ws=0) == WORKSPACE
    # the order: invalid before unsupported before the workspace
    assert _stats(lib, m=0, products=4, ws=0) == INVALID
    assert _stats(lib, products=4, ws=0) == UNSUPPORTED
    assert _stats(lib, E=1024, products=3, Bv=16 * 65535, ws_bytes=0) == WORKSPACE   # the widest rows pass the limits


def test_topk_entry_refuses_as_the_plain_entry_and_for_its_own_arguments():
    lib = L.lib()
    for null in ("q", "g", "scores", "ids", "m", "s"):
        assert _topk(lib, **{null: 0}) == INVALID, null
    for kw in (dict(Bq=0), dict(Bg=0), dict(E=0), dict(Bq=-5), dict(n_total=-1), dict(side=2), dict(side=-1)):
        assert _topk(lib, **kw) == INVALID, kw
    for kw in (dict(k=0), dict(k=129), dict(products=0), dict(products=4), dict(E=96), dict(E=1088),
               dict(E=1024, products=3, k=128), dict(Bq=16 * 65535 + 1)):
        assert _topk(lib, **kw) == UNSUPPORTED, kw
    need = lib.cc_similarity_topk_workspace_bytes(4, 100, 10)
    assert _topk(lib, ws_bytes=need - 1) == WORKSPACE
    assert _topk(lib, ws=0) == WORKSPACE
    assert _topk(lib, s=0, k=129, ws=0) == INVALID
    assert _topk(lib, k=129, ws=0) == UNSUPPORTED
    for kw in (dict(E=1024, products=3, k=127), dict(E=1024, products=2, k=128), dict(side=0), dict(n_total=0)):
        assert _topk(lib, ws_bytes=0, **kw) == WORKSPACE, kw


def test_workspaces_hold_partial_results_only():
    lib = L.lib()
    assert lib.cc_dsl_col_stats_planes_slices(0) == 0 and lib.cc_dsl_col_stats_planes_workspace_bytes(0, 5) == 0
    assert lib.cc_dsl_col_stats_planes_workspace_bytes(5, 0) == 0
    last = 0
    for Bt in (1, 15, 16, 17, 511, 512, 1000, 4099, 10000, 200003, 1 << 20, 1 << 24):
        slices = lib.cc_dsl_col_stats_planes_slices(Bt)
        assert slices >= max(1, last) and slices * 16 <= max(Bt, 16), Bt      # monotone in Bt; never an empty slice
        last = slices
        for Bv in (1, 16, 17, 200003):
            w = lib.cc_dsl_col_stats_planes_workspace_bytes(Bt, Bv)
            assert slices * Bv * 8 <= w < slices * Bv * 8 + 256, (Bt, Bv)   # one (m, s) pair per (slice, video row)
    assert lib.cc_dsl_col_stats_planes_slices(4099) >= 2                   # (the GPU tests' several-slices shape)
    matrix = 16 * (1 << 20) * 4
    assert lib.cc_dsl_col_stats_planes_workspace_bytes(1 << 20, 16) < matrix // 256
    # the top-k lists are the plain op's: positive, monotone in k, Bq * slices * k pairs
    for Bq, Bg in ((1, 1), (16, 4099), (33, 200003), (16, 1 << 20)):
        last = 0
        for k in (1, 10, 64, 65, 128):
            w = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
            assert w > 0 and w >= last and w < Bq * lib.cc_similarity_topk_slices(Bq, Bg, k) * k * 8 + 256
            last = w
    assert lib.cc_similarity_topk_workspace_bytes(16, 1 << 20, 128) < matrix // 4


def test_fake_kernels_give_shapes_on_the_meta_device():
    assert "dsl_col_stats_planes" in torch_ops.OPS and "similarity_topk_dsl" in torch_ops.OPS
    t = torch.empty(1000, 3 * 64, device="meta", dtype=torch.float16)
    v = torch.empty(40, 3 * 64, device="meta", dtype=torch.float16)
    m, s = torch.ops.centerclip.dsl_col_stats_planes(t, v, 900, 33, 20.0, 2)
    assert m.shape == s.shape == (33,) and m.dtype == s.dtype == torch.float32 and m.device.type == "meta"
    stat = torch.empty(1000, device="meta")
    scores, ids = torch.ops.centerclip.similarity_topk_dsl(v, t, 900, 20.0, 2, 17, stat, stat, 1, 900)
    assert scores.shape == (40, 17) and scores.dtype == torch.float32 and scores.device.type == "meta"
    assert ids.shape == (40, 17) and ids.dtype == torch.int64
    h = lambda n: torch.zeros(n, 192, dtype=torch.float16)
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        torch.ops.centerclip.dsl_col_stats_planes(h(8), h(2), 8, 2, 1.0, 2)
    with pytest.raises(NotImplementedError):
        torch.ops.centerclip.similarity_topk_dsl(h(2), h(8), 8, 1.0, 2, 3, torch.zeros(8), torch.ones(8), 1, 8)


def test_feature_gallery_dual_softmax_refusals():
    import centerclip_amd.search as S
    from centerclip_amd.search import FeatureGallery
    assert S.__all__ == ["FeatureGallery"]
    for model in (_cpu_model(), _cpu_model(camoe_dsl=1)):                  # accepted whatever the model's flag - on a device
        with pytest.raises(L.CenterClipHipError):
            FeatureGallery(model, dual_softmax=True)
    with pytest.raises(ValueError):
        FeatureGallery(_cpu_model(camoe_dsl=1), dual_softmax=False)
    with pytest.raises(ValueError):
        FeatureGallery(_cpu_model(), side="audio", dual_softmax=True)
    # galleries as the constructor leaves them, minus the device
    model = _cpu_model()

    def bare(side, dual_softmax):
        gal = FeatureGallery.__new__(FeatureGallery)
        gal.model = gal.core = model
        gal.side, gal.products, gal.E, gal._n = side, 2, 64, 0
        gal.device, gal.backend = torch.device("cpu"), S.HipBackend
        gal._rows = torch.zeros(0, 192, dtype=torch.float16)
        if dual_softmax:
            gal.dual_softmax, gal._bank, gal._m, gal._s = True, None, torch.zeros(0), torch.zeros(0)
        return gal
    ids, seq = torch.zeros(2, 16, dtype=torch.long), torch.zeros(2, 1, 64)
    for gal in (bare("text", True), bare("video", False), bare("text", False)):     # only a dual-softmax clip gallery has a bank
        with pytest.raises(ValueError):
            gal.set_query_bank(ids)
        with pytest.raises(ValueError):
            gal.set_query_bank_features(seq)
    gal = bare("video", True)
    with pytest.raises(L.CenterClipHipError):                              # CPU tensors are refused before anything is encoded
        gal.set_query_bank(ids)
    with pytest.raises(L.CenterClipHipError):
        gal.set_query_bank_features(seq)
    with pytest.raises(L.CenterClipHipError):
        gal.search(ids)
    gal._bank = None
    assert set(gal.state_dict()) == {"rows", "count", "E", "side", "products", "dual_softmax", "bank", "m", "s"}
    plain = bare("video", False)
    assert set(plain.state_dict()) == {"rows", "count", "E", "side", "products"}
    with pytest.raises(ValueError, match="dual_softmax"):                  # the flag is compared before anything is written
        plain.load_state_dict(gal.state_dict())
    with pytest.raises(ValueError, match="dual_softmax"):
        gal.load_state_dict(plain.state_dict())
