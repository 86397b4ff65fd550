"""Top-k search on the MI355X (``-m gpu``): torch.ops.centerclip.similarity_topk against the matrix op it must reproduce, and
FeatureGallery on the small model of tests/golden/r2_golden.npz.

The reference of every exactness check is the existing op on the same rows:
    S = scaled_dot_planes(query planes, gallery copy padded to padded_video_rows(n) with zero rows, n, mult, products)
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
and the assertions are exact: the ids equal `order`, the scores are bit-equal to S gathered there, the fill beyond n is
(-inf, -1).  Planes come from normalize_rows_planes on seeded randn rows unless a test builds its rows on purpose."""
import io
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from centerclip_amd import _lib as L
from centerclip_amd import torch_ops as T
from oracle.recipes import dyadic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
MULT = math.exp(4.6052)
op = torch.ops.centerclip


def _planes(rows, video_side):
    return op.normalize_rows_planes(rows.to(DEV).float().contiguous(), video_side)


def _randn_planes(seed, Bq, rows, E):
    g = torch.Generator().manual_seed(seed)
    return _planes(torch.randn(Bq, E, generator=g), False), _planes(torch.randn(rows, E, generator=g), True)


def _matrix(q, gal, n, mult, products):
    pad = torch.zeros(max(n, T.padded_video_rows(n)), gal.shape[1], device=DEV, dtype=torch.float16)
    pad[:n] = gal[:n]
    return op.scaled_dot_planes(q, pad, n, mult, products)


def _assert_topk(scores, ids, S, k):
    """scores / ids [Bq, k] against the matrix S [Bq, n] (device or numpy)"""
    Sn = S.cpu().numpy() if torch.is_tensor(S) else S
    n = Sn.shape[1]
    order = np.argsort(-Sn, axis=1, kind="stable")[:, :k]
    kk = min(k, n)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and tuple(ids.shape) == tuple(scores.shape) == (Sn.shape[0], k)
    got_ids, got = ids.cpu().numpy(), scores.cpu().numpy()
    assert np.array_equal(got_ids[:, :kk], order), "ids differ from the stable descending sort"
    want = np.take_along_axis(Sn, order, 1)
    assert np.array_equal(got[:, :kk].view(np.uint32), want.view(np.uint32)), "scores are not the matrix op's bits"
    assert (got_ids[:, kk:] == -1).all() and np.isneginf(got[:, kk:]).all()


def _check(q, gal, n, products, k, mult=MULT):
    S = _matrix(q, gal, n, mult, products)
    scores, ids = op.similarity_topk(q, gal, n, mult, products, k)
    _assert_topk(scores, ids, S, k)
    return scores, ids, S


# ------------------------------------------------------------------------------------------------ 1. shapes
BQS, NS, KS, PRODUCTS = (1, 5, 16, 17, 33), (1, 15, 16, 17, 255, 256, 257, 1000, 4099), (1, 10, 64, 65, 128), (1, 2, 3)


def _sweep():
    """A seeded subset of the product: every axis is dealt out in a shuffled cycle, so 12 cases show every value of every
    axis; two more make sure k > n is met from both sides of a tile."""
    rng = np.random.default_rng(20260)
    cols = [[axis[i] for i in np.resize(rng.permutation(len(axis)), 12)] for axis in (BQS, NS, KS, PRODUCTS)]
    cases = list(zip(*cols)) + [(17, 15, 65, 2), (1, 1, 128, 3)]
    for axis, col in zip((BQS, NS, KS, PRODUCTS), zip(*cases)):
        assert set(axis) == set(col)
    assert any(k > n for _, n, k, _ in cases)
    return [tuple(int(v) for v in c) for c in cases]


@pytest.mark.parametrize("Bq,n,k,products", _sweep())
def test_shape_sweep_e64(Bq, n, k, products):
    q, gal = _randn_planes(1000 * Bq + n + k, Bq, n + 37, 64)            # 37 non-zero rows behind n: they must not appear
    _check(q, gal, n, products, k)


@pytest.mark.parametrize("E,Bq,n,k,products", [(512, 16, 3001, 100, 2), (768, 7, 2000, 128, 3)])
def test_wide_rows(E, Bq, n, k, products):
    q, gal = _randn_planes(E + n, Bq, n + 5, E)
    _check(q, gal, n, products, k)


def test_library_refuses_what_the_header_says():
    q, gal = _randn_planes(3, 2, 40, 1024)
    with pytest.raises(L.CenterClipHipError, match="cc_similarity_topk_planes_f32"):
        op.similarity_topk(q, gal, 40, MULT, 3, 128)                       # the one (E, products, k) beyond the LDS
    with pytest.raises(L.CenterClipHipError):
        op.similarity_topk(q, gal, 40, MULT, 3, 129)
    with pytest.raises(ValueError):
        op.similarity_topk(q, gal, 41, MULT, 3, 5)                         # more rows than the buffer holds
    _check(q, gal, 40, 3, 127)


# ------------------------------------------------------------------------------------------------ 2. ties
def test_identical_gallery_rows_come_in_id_order():
    g = torch.Generator().manual_seed(11)
    q = _planes(torch.randn(5, 64, generator=g), False)
    gal = _planes(torch.randn(1, 64, generator=g).expand(4099, 64), True)
    for k in (10, 128):
        _, ids, _ = _check(q, gal, 4099, 2, k)
        assert torch.equal(ids.cpu(), torch.arange(k).expand(5, k))


def test_duplicates_of_the_best_row_in_every_slice():
    n, k, Bq = 4099, 64, 3
    slices = L.lib().cc_similarity_topk_slices(Bq, n, k)
    assert slices >= 2
    q, gal = _randn_planes(12, Bq, n, 64)
    best = int(_matrix(q, gal, n, MULT, 3)[0].argmax())
    at = sorted({0, n - 1, best} | {n * (2 * s + 1) // (2 * slices) for s in range(slices)})     # the middle of every slice
    gal[at] = gal[best].clone()
    _, ids, S = _check(q, gal, n, 3, k)
    assert len(at) >= slices + 2 and ids[0, :len(at)].tolist() == at                              # equal scores: ascending ids
    assert len(set(S[0, at].tolist())) == 1


def test_seven_distinct_rows_repeated():
    n = 4099
    g = torch.Generator().manual_seed(13)
    base = torch.randn(7, 64, generator=g)
    pick = torch.from_numpy(np.random.default_rng(13).integers(0, 7, size=n))
    q = _planes(torch.randn(17, 64, generator=g), False)
    gal = _planes(base[pick], True)
    for k, products in ((1, 1), (65, 2), (128, 3)):
        _check(q, gal, n, products, k)


# ------------------------------------------------------------------------------------------------ 3. insertion extremes
@pytest.mark.parametrize("direction", ["increasing", "decreasing"])
def test_every_column_a_new_best_or_none(direction):
    """Planar unit vectors at increasing angles: against the query (1, 0, ...) the scores fall with the column id, so only
    the first k columns ever enter a list; reversed they rise and EVERY column is inserted.  fp16 plane rounding makes
    neighbours tie - the comparison is against S, so the tie rule covers them."""
    n, k = 1000, 64
    theta = torch.arange(n, dtype=torch.float64) * (math.pi / 2 / n)
    if direction == "increasing":
        theta = theta.flip(0)
    rows = torch.zeros(n, 64, dtype=torch.float64)
    rows[:, 0], rows[:, 1] = torch.cos(theta), torch.sin(theta)
    qr = torch.zeros(3, 64)
    qr[0, 0] = 1.0
    qr[1, 1] = 1.0                                                        # (the other direction in the same launch)
    qr[2, 0] = qr[2, 1] = 1.0
    q, gal = _planes(qr, False), _planes(rows.float(), True)
    for products in (1, 3):
        _, ids, S = _check(q, gal, n, products, k)
    s0 = S[0].cpu().numpy()
    assert (np.diff(s0) >= 0).all() if direction == "increasing" else (np.diff(s0) <= 0).all()
    assert len(np.unique(s0)) > n // 2


# ------------------------------------------------------------------------------------------------ 4. many slices, capture
def test_many_slices():
    Bq, n, k = 3, 200003, 100
    assert L.lib().cc_similarity_topk_slices(Bq, n, k) >= 3
    g = torch.Generator(device=DEV).manual_seed(14)
    gal = op.normalize_rows_planes(torch.randn(n + 5, 64, device=DEV, generator=g), True)
    q = op.normalize_rows_planes(torch.randn(Bq, 64, device=DEV, generator=g), False)
    _check(q, gal, n, 2, k)


def test_graph_capture_and_replay():
    Bq, n, k = 5, 4099, 10
    q, gal = _randn_planes(15, Bq, n, 64)
    q2, _ = _randn_planes(16, Bq, 1, 64)
    qbuf = q.clone()
    op.similarity_topk(qbuf, gal, n, MULT, 2, k)                           # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores, ids = op.similarity_topk(qbuf, gal, n, MULT, 2, k)
    for new in (q2, q):
        qbuf.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want_scores, want_ids = op.similarity_topk(new, gal, n, MULT, 2, k)
        assert torch.equal(ids, want_ids) and torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
        _assert_topk(scores, ids, _matrix(new, gal, n, MULT, 2), k)


# ------------------------------------------------------------------------------------------------ 5. FeatureGallery
@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(HERE, "golden", "r2_golden.npz"))


def _state(g2):
    return {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
            for k in g2.files if k.startswith("s1_sd/")}


def _eval_model(g2, cluster_inter, sd=None, **extra):
    """tests/test_dsl_gpu.py::_eval_model"""
    from centerclip_amd.clip4clip import CLIP4Clip
    cfg = g2["s1_cfg"]
    Tf, T_new = int(cfg[11]), int(cfg[12])
    kw = dict(cluster_inter=cluster_inter, deep_cluster=0, cluster_algo='kmediods++', max_frames=Tf,
              target_frames_blocks=[4, T_new, T_new] if cluster_inter else [Tf, Tf, Tf], cluster_num_blocks=[16, 6, 6],
              cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100, minkowski_norm_p=2.0,
              aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True, sim_header='meanP',
              linear_patch='2d', pre_visual_pooling=0)
    kw.update(extra)
    return CLIP4Clip.from_state_dict(_state(g2) if sd is None else sd, Namespace(**kw)).to(DEV).eval()


N_CLIPS, BATCHES = 12, (5, 3, 4)


def _dataset(cfg):
    """12 clips with a caption each, in the loader's shapes: video [n, 1, T, 3, RES, RES], video_mask [n, 1, T] (zeros in
    some), input_ids [n, 1, CTX]"""
    RES, CTX, VOCAB, Tf = int(cfg[1]), int(cfg[5]), int(cfg[6]), int(cfg[11])
    rng = np.random.default_rng(77)
    video = dyadic(78, (N_CLIPS, 1, Tf, 3, RES, RES)) * np.float32(1.5)
    vmask = np.ones((N_CLIPS, 1, Tf), dtype=np.int64)
    vmask[1, 0, Tf - 1:] = 0
    vmask[7, 0, Tf - 2:] = 0
    ids = np.zeros((N_CLIPS, 1, CTX), dtype=np.int64)
    for i in range(N_CLIPS):
        ln = int(rng.integers(4, CTX + 1))
        ids[i, 0, 0], ids[i, 0, ln - 1] = VOCAB - 2, VOCAB - 1
        ids[i, 0, 1:ln - 1] = rng.integers(1, VOCAB - 2, size=ln - 2)
    return tuple(torch.from_numpy(a).to(DEV) for a in (video, vmask, ids))


def _split(t):
    return torch.split(t, list(BATCHES))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else
                                                                    a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                    b.view(torch.int16) if b.dtype == torch.float16 else
                                                                    b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("cluster_inter", [0, 1])
def test_feature_gallery_on_the_small_model(g2, cluster_inter):
    from centerclip_amd import eval as E
    from centerclip_amd.search import FeatureGallery
    model = _eval_model(g2, cluster_inter)
    video, vmask, ids = _dataset(g2["s1_cfg"])
    gal = FeatureGallery(model, capacity=4)
    assert len(gal) == 0 and gal.products == E.HipBackend.similarity_products
    s, i = gal.search(ids[:2], k=3)                                        # an empty gallery: the fill alone
    assert bool((i == -1).all()) and bool(torch.isneginf(s).all())
    pos = [gal.add(v, m) for v, m in zip(_split(video), _split(vmask))]
    assert torch.equal(torch.cat(pos), torch.arange(N_CLIPS)) and len(gal) == N_CLIPS
    assert gal.rows.shape == (N_CLIPS, 3 * int(g2["s1_cfg"][0])) and not model.training
    one = FeatureGallery(model)
    one.add(video, vmask)
    assert _bits(gal.rows, one.rows)                                       # growth 4 -> 8 -> 16 kept every row
    # the matrix: eval's, from the same per-batch features
    with torch.no_grad():
        seq_list = [model(input_ids=ids)['sequence_output']]
        vis_list = [model(video=v, video_mask=m)['visual_output'] for v, m in zip(_split(video), _split(vmask))]
        want = E._similarity_matrix(model, None, [(m,) for m in _split(vmask)], seq_list, vis_list)
    S = gal.similarity(ids)
    assert want.shape == (N_CLIPS, N_CLIPS) and _bits(S, want)
    assert _bits(gal.similarity_features(seq_list[0]), want)
    for k in (1, 5, 20):                                                   # 20 > 12 clips: the fill
        scores, idx = gal.search(ids, k=k)
        _assert_topk(scores, idx, S, k)
        s2, i2 = gal.search_features(seq_list[0], k=k)
        assert _bits(s2, scores) and torch.equal(i2, idx)
    # products on request
    g3 = FeatureGallery(model, products=3)
    g3.add_features(torch.cat(vis_list), vmask)
    assert _bits(g3.rows, gal.rows)
    s3, i3 = g3.search(ids, k=5)
    _assert_topk(s3, i3, g3.similarity(ids), 5)
    assert not _bits(g3.similarity(ids), S)
    # captions as the gallery, clips as the queries: rows of the transposed matrix
    tg = FeatureGallery(model, side="text", capacity=4)
    for b in _split(ids):
        tg.add(b)
    feats = torch.cat(vis_list)
    assert _bits(tg.similarity_features(feats, vmask), want.t().contiguous())
    scores, idx = tg.search_features(feats, k=7, mask=vmask)
    _assert_topk(scores, idx, want.t().contiguous(), 7)
    St = tg.similarity(video, vmask)                                       # (the clips encoded by the gallery itself)
    scores, idx = tg.search(video, vmask, k=7)
    _assert_topk(scores, idx, St, 7)
    # save / load
    buf = io.BytesIO()
    torch.save(gal.state_dict(), buf)
    buf.seek(0)
    fresh = FeatureGallery(model, products=3)
    fresh.load_state_dict(torch.load(buf))
    assert len(fresh) == N_CLIPS and fresh.products == gal.products and _bits(fresh.rows, gal.rows)
    a, b = fresh.search(ids, k=5), gal.search(ids, k=5)
    assert _bits(a[0], b[0]) and torch.equal(a[1], b[1]) and _bits(fresh.similarity(ids), S)
    with pytest.raises(ValueError):
        tg.load_state_dict(gal.state_dict())                               # side
    bad = dict(gal.state_dict(), E=128)
    with pytest.raises(ValueError):
        fresh.load_state_dict(bad)
    assert len(tg) == N_CLIPS and _bits(tg.similarity(video, vmask), St) and len(fresh) == N_CLIPS
    gal.clear()
    assert len(gal) == 0
    with pytest.raises(L.CenterClipHipError):
        one.search(ids.cpu())


def test_feature_gallery_refuses_the_dual_softmax(g2):
    from centerclip_amd.search import FeatureGallery
    with pytest.raises(ValueError, match="camoe_dsl"):
        FeatureGallery(_eval_model(g2, 0, camoe_dsl=1))


def test_feature_gallery_runs_the_seqtransf_head(g2):
    """embed_dim = transformer_width (128), as the head needs: the small model with square projections"""
    from centerclip_amd import eval as E
    from centerclip_amd.search import FeatureGallery
    sd = _state(g2)
    g = torch.Generator().manual_seed(5)
    sd["text_projection"] = torch.randn(128, 128, generator=g) * 0.05
    sd["visual.proj"] = torch.randn(sd["visual.proj"].shape[0], 128, generator=g) * 0.05
    model = _eval_model(g2, 0, sd=sd, sim_header='seqTransf', cross_num_hidden_layers=2)
    Tf = int(g2["s1_cfg"][11])
    vis = torch.randn(6, Tf, 128, generator=g).to(DEV)
    mask = torch.ones(6, 1, Tf, dtype=torch.long, device=DEV)
    mask[2, 0, 2:] = 0
    gal = FeatureGallery(model)
    assert gal.E == 128
    gal.add_features(vis, mask)
    with torch.no_grad():
        want = E._video_operand(model, vis, mask, E.HipBackend)
        plain = E.HipBackend.video_operand(vis, mask.view(6, Tf))
    assert _bits(gal.rows, want) and not _bits(want, plain)
    seq = torch.randn(3, 1, 128, generator=g).to(DEV)
    scores, idx = gal.search_features(seq, k=4)
    _assert_topk(scores, idx, gal.similarity_features(seq), 4)
