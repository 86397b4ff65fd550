"""Top-k search without a GPU: the argument checks of cc_similarity_topk_planes_f32 (they end before anything is read or
launched, so never-dereferenced pointers do), the plan queries (slices, workspace: memory that does not grow with the
gallery), the op's fake kernel, and FeatureGallery's refusals of CPU models and tensors."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _call(lib, q=256, g=256, Bq=4, Bg=100, E=64, products=2, k=10, scores=256, ids=256, ws=256, ws_bytes=None):
    p = lambda v: ctypes.c_void_p(v) if v else None                       # (addresses that are never dereferenced)
    if ws_bytes is None:
        ws_bytes = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
    return lib.cc_similarity_topk_planes_f32(p(q), p(g), Bq, Bg, E, 1.0, products, k, p(scores), p(ids), p(ws), ws_bytes, None)


def test_entry_refuses_before_touching_memory():
    lib = L.lib()
    assert b"unsupported" in lib.cc_status_string(UNSUPPORTED).lower()
    assert _call(lib, k=0) == UNSUPPORTED
    assert _call(lib, k=129) == UNSUPPORTED
    assert _call(lib, k=-3) == UNSUPPORTED
    assert _call(lib, products=4) == UNSUPPORTED
    assert _call(lib, products=0) == UNSUPPORTED
    assert _call(lib, E=96) == UNSUPPORTED
    assert _call(lib, E=1088) == UNSUPPORTED
    for null in ("q", "g", "scores", "ids"):
        assert _call(lib, **{null: 0}) == INVALID, null
    for name in ("Bq", "Bg", "E"):
        assert _call(lib, **{name: 0}) == INVALID, name
        assert _call(lib, **{name: -5}) == INVALID, name
    need = lib.cc_similarity_topk_workspace_bytes(4, 100, 10)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == WORKSPACE
    assert _call(lib, ws=0) == WORKSPACE
    # the one combination the streaming kernel's LDS cannot hold (the header names it); its neighbours pass these checks and
    # stop at the workspace
    assert _call(lib, E=1024, products=3, k=128) == UNSUPPORTED
    for kw in (dict(E=1024, products=3, k=127), dict(E=1024, products=2, k=128), dict(E=768, products=3, k=128)):
        assert _call(lib, ws_bytes=0, **kw) == WORKSPACE, kw


def test_workspace_does_not_grow_with_the_gallery():
    lib = L.lib()
    matrix = 16 * (1 << 20) * 4
    assert 0 < lib.cc_similarity_topk_workspace_bytes(16, 1 << 20, 10) < matrix // 4
    assert lib.cc_similarity_topk_workspace_bytes(16, 1 << 20, 128) < matrix // 4
    shapes = [(1, 1), (1, 17), (5, 1000), (16, 4099), (17, 4099), (33, 200003), (3, 200003), (16, 1 << 20), (1000, 1 << 20)]
    for Bq, Bg in shapes:
        last = 0
        for k in (1, 2, 10, 64, 65, 100, 128):
            s = lib.cc_similarity_topk_slices(Bq, Bg, k)
            assert s >= 1, (Bq, Bg, k)
            w = lib.cc_similarity_topk_workspace_bytes(Bq, Bg, k)
            assert w >= Bq * s * k * 8 and w >= last, (Bq, Bg, k)         # one 8-byte pair per (query, slice, entry)
            last = w
    assert lib.cc_similarity_topk_slices(3, 200003, 100) >= 3
    # a gallery 16 times as large: the same lists (the grid is full either way)
    assert lib.cc_similarity_topk_workspace_bytes(16, 1 << 24, 10) == lib.cc_similarity_topk_workspace_bytes(16, 1 << 20, 10)


def test_fake_kernel_gives_shapes_on_the_meta_device():
    assert "similarity_topk" in torch_ops.OPS
    q = torch.empty(5, 3 * 64, device="meta", dtype=torch.float16)
    g = torch.empty(1000, 3 * 64, device="meta", dtype=torch.float16)
    scores, ids = torch.ops.centerclip.similarity_topk(q, g, 900, 20.0, 2, 17)
    assert scores.shape == (5, 17) and scores.dtype == torch.float32 and scores.device.type == "meta"
    assert ids.shape == (5, 17) and ids.dtype == torch.int64
    with pytest.raises(NotImplementedError):                               # no CPU implementation
        torch.ops.centerclip.similarity_topk(torch.zeros(2, 192, dtype=torch.float16), torch.zeros(8, 192, dtype=torch.float16),
                                             8, 1.0, 2, 3)


def _cpu_model(**extra):
    from centerclip_amd.clip4clip import CLIP4Clip
    g2 = np.load(os.path.join(HERE, "golden", "r2_golden.npz"))
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    T = int(g2["s1_cfg"][11])
    a = Namespace(cluster_inter=0, deep_cluster=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T, T, T],
                  cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                  minkowski_norm_p=2.0, aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True,
                  sim_header='meanP', linear_patch='2d', pre_visual_pooling=0, **extra)
    return CLIP4Clip.from_state_dict(sd, a).eval()


def test_feature_gallery_refuses_cpu_models_and_tensors():
    import centerclip_amd.search as S
    from centerclip_amd.search import FeatureGallery
    assert S.__all__ == ["FeatureGallery"]
    model = _cpu_model()
    with pytest.raises(L.CenterClipHipError):
        FeatureGallery(model)
    with pytest.raises(ValueError):
        FeatureGallery(model, side="audio")
    with pytest.raises(ValueError):
        FeatureGallery(model, products=4)
    with pytest.raises(ValueError):
        FeatureGallery(_cpu_model(camoe_dsl=1))
    # a gallery as its constructor leaves it, minus the device: CPU tensors are refused before anything is encoded
    gal = FeatureGallery.__new__(FeatureGallery)
    gal.model = gal.core = model
    gal.side, gal.products, gal.E, gal._n = "video", 2, 64, 0
    gal.device = torch.device("cpu")
    gal.backend = S.HipBackend
    gal._rows = torch.zeros(0, 192, dtype=torch.float16)
    for call in (lambda: gal.add(torch.zeros(1, 1, 4, 3, 64, 64), torch.ones(1, 1, 4, dtype=torch.long)),
                 lambda: gal.add_features(torch.zeros(2, 4, 64), torch.ones(2, 4, dtype=torch.long)),
                 lambda: gal.search(torch.zeros(2, 16, dtype=torch.long)),
                 lambda: gal.search_features(torch.zeros(2, 1, 64), k=3),
                 lambda: gal.similarity(torch.zeros(2, 16, dtype=torch.long))):
        with pytest.raises(L.CenterClipHipError):
            call()
    assert len(gal) == 0
