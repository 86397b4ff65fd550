"""Parity of the HIP CLIP forward / similarity path (through the C ABI) against the oracle and the
fixtures captured from the reference.  Needs a real MI355X (``-m gpu``).

Tolerances (north star: "within 1e-3 fp32 for embeddings/similarities"):
  * single ops, fp32 outputs ............ 2e-4 relative to the tensor's max magnitude
  * single ops, fp16 outputs ............ 2e-3 relative (one fp16 rounding = 4.9e-4)
  * L2-normalised embeddings, cosine similarities ... max|delta| <= 1e-3 absolute, asserted
    GIVEN IDENTICAL MEDOID SETS (raw 512-d features have norm ~22, so the absolute
    1e-3 contract is stated on normalised embeddings; raw features are checked at 1e-3 relative).
  * fp32-only paths (pooling, similarity GEMM, metrics) ... 2e-5 absolute.
"""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import clip_oracle as clo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_golden.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def golden_state_dict(g):
    return {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k])
            for k in g.files if k.startswith("sd/")}


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------- single ops
@pytest.mark.parametrize("M,N,K", [(9600, 2304, 768), (2400, 768, 3072), (100, 128, 64), (513, 3072, 768), (77, 512, 2048)])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 8, 10])
def test_linear_f16_epilogues(M, N, K, tile):
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=gen)).half()
    w = (torch.randn(N, K, generator=gen) * K ** -0.5).half()
    bias = torch.randn(N, generator=gen)
    ref = a.double() @ w.double().t() + bias.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    if (tile in (5, 10) and N % 256) or (tile in (1, 3, 6) and N % 128) or (tile == 8 and K % 128):
        with pytest.raises(RuntimeError, match="invalid"):      # a forced tile that does not divide N is refused
            ops.linear_f16(ad, wd, bd, "f32", tile=tile)
        return
    y = ops.linear_f16(ad, wd, bd, "f32", tile=tile).cpu()
    assert relerr(y, ref) < 2e-4
    y = ops.linear_f16(ad, wd, None, "f32", tile=tile).cpu()
    assert relerr(y, ref - bias.double()) < 2e-4
    y = ops.linear_f16(ad, wd, bd, "f16", tile=tile).float().cpu()
    assert relerr(y, ref) < 2e-3
    y = ops.linear_f16(ad, wd, bd, "f16_gelu", tile=tile).float().cpu()
    assert relerr(y, ref * torch.sigmoid(1.702 * ref)) < 2e-3
    resid = torch.randn(M, N, generator=gen)
    out = resid.to(DEV).clone()
    ops.linear_f16(ad, wd, bd, "f32_resid", out=out, tile=tile)
    assert relerr(out.cpu(), ref + resid.double()) < 2e-4


@pytest.mark.parametrize("M,N,K", [(9600, 2304, 768), (300, 192, 64), (1000, 1536, 512), (257, 768, 3072)])
def test_linear_f16_tile_256x192(M, N, K):
    """tile 7 (256 x 192, 48-column wave tiles) exists for the fp16-output epilogues and the plain fp32 one (the similarity
    GEMM of similarity.hip); the auto choice picks it for
    in_proj at M = 9,600 and must agree with the forced 256 x 256 / 128 x 128 results bit for bit (same k order)."""
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(7 * M + N + K)
    a = (torch.randn(M, K, generator=gen)).half()
    w = (torch.randn(N, K, generator=gen) * K ** -0.5).half()
    bias = torch.randn(N, generator=gen)
    ref = a.double() @ w.double().t() + bias.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    y = ops.linear_f16(ad, wd, bd, "f16", tile=7)
    assert relerr(y.float().cpu(), ref) < 2e-3
    assert torch.equal(y, ops.linear_f16(ad, wd, bd, "f16", tile=4))
    assert torch.equal(y, ops.linear_f16(ad, wd, bd, "f16", tile=0))
    y = ops.linear_f16(ad, wd, bd, "f16_gelu", tile=7)
    assert relerr(y.float().cpu(), ref * torch.sigmoid(1.702 * ref)) < 2e-3
    assert torch.equal(y, ops.linear_f16(ad, wd, bd, "f16_gelu", tile=4))
    y32 = ops.linear_f16(ad, wd, bd, "f32", out=torch.zeros(M, N, device=DEV), tile=7)      # 12 of 16 lane slots per row
    assert torch.equal(y32, ops.linear_f16(ad, wd, bd, "f32", out=torch.zeros(M, N, device=DEV), tile=4))
    assert relerr(y32.cpu(), ref) < 2e-5
    with pytest.raises(RuntimeError, match="invalid"):
        ops.linear_f16(ad, wd, bd, "f32_resid", out=torch.zeros(M, N, device=DEV), tile=7)
    with pytest.raises(RuntimeError, match="invalid"):
        ops.linear_f16(ad[:, :64].contiguous(), wd[:128, :64].contiguous(), None, "f16", tile=7)     # 128 % 192
    # folded LayerNorm through the same tile
    h = torch.randn(M, K, generator=gen) * 2 + 0.3
    gamma, beta = torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.2
    w2 = torch.randn(N, K, generator=gen) * K ** -0.5
    pre = F.layer_norm(h.double(), (K,), gamma.double(), beta.double(), 1e-5) @ w2.double().t() + bias.double()
    h16, st1, _ = ops.row_stats(h.to(DEV))
    wf, c1, c2 = ops.fold_layernorm_linear(w2.to(DEV), bd, gamma.to(DEV), beta.to(DEV))
    y7 = ops.linear_ln_f16(h16, wf, c1, c2, st1, 1, gelu=False, tile=7)
    assert relerr(y7.float().cpu(), pre) < 3e-3
    assert torch.equal(y7, ops.linear_ln_f16(h16, wf, c1, c2, st1, 1, gelu=False, tile=4))
    y7 = ops.linear_ln_f16(h16, wf, c1, c2, st1, 1, gelu=True, tile=7)
    assert torch.equal(y7, ops.linear_ln_f16(h16, wf, c1, c2, st1, 1, gelu=True, tile=4))


@pytest.mark.parametrize("M,W,tile", [(9600, 768, 0), (2400, 768, 0), (512, 512, 0), (300, 768, 1), (300, 768, 4)])
def test_folded_layernorm_chain(M, W, tile):
    """residual linear (+fp16 copy + per-tile partial sums) -> LayerNorm-folded linear, against
    h += a W^T + b;  y = QuickGELU(LN(h) W2^T + b2) in float64."""
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(M + W)
    a = torch.randn(M, W, generator=gen).half()
    w1 = (torch.randn(W, W, generator=gen) * W ** -0.5).half()
    b1 = torch.randn(W, generator=gen) * 0.1
    h0 = torch.randn(M, W, generator=gen) * 2 + 0.3
    gamma, beta = torch.rand(W, generator=gen) + 0.5, torch.randn(W, generator=gen) * 0.2
    w2 = torch.randn(4 * W, W, generator=gen) * W ** -0.5
    b2 = torch.randn(4 * W, generator=gen) * 0.1
    href = h0.double() + a.double() @ w1.double().t() + b1.double()
    xn = F.layer_norm(href, (W,), gamma.double(), beta.double(), 1e-5)
    pre = xn @ w2.double().t() + b2.double()
    yref = pre * torch.sigmoid(1.702 * pre)
    h = h0.to(DEV).clone()
    h16, stats, slots, _ = ops.linear_resid_stats_f16(a.to(DEV), w1.to(DEV), b1.to(DEV), h, tile=tile)
    assert relerr(h.cpu(), href) < 2e-4 and torch.equal(h16, h.half())
    s = stats.sum(1).double().cpu()
    np.testing.assert_allclose(s[:, 0].numpy(), h16.double().sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[:, 1].numpy(), (h16.double() ** 2).sum(-1).cpu().numpy(), rtol=1e-5)
    wf, c1, c2 = ops.fold_layernorm_linear(w2.to(DEV), b2.to(DEV), gamma.to(DEV), beta.to(DEV))
    y = ops.linear_ln_f16(h16, wf, c1, c2, stats.contiguous(), slots, gelu=True).float().cpu()
    assert relerr(y, yref) < 3e-3
    pre_hip = ops.linear_ln_f16(h16, wf, c1, c2, stats.contiguous(), slots, gelu=False).float().cpu()
    assert relerr(pre_hip, pre) < 3e-3
    # one-slot statistics from cc_row_stats_f16 give the same result
    h16b, st1, _ = ops.row_stats(h)
    y1 = ops.linear_ln_f16(h16b, wf, c1, c2, st1, 1, gelu=True).float().cpu()
    assert float((y1 - y).abs().max()) <= 4e-3 * float(yref.abs().max())


def test_linear_detects_transposed_operands():
    """asymmetric A=I check (a symmetric B would hide a row/col swap)."""
    from centerclip_amd import ops
    K = N = 128
    a = torch.eye(64, K).half()
    w = (torch.arange(N * K).reshape(N, K) % 17).half()
    y = ops.linear_f16(a.to(DEV), w.to(DEV), None, "f32").cpu()
    assert torch.equal(y, w.float().t()[:64])


@pytest.mark.parametrize("rows,W", [(9600, 768), (37, 512), (5, 128), (1, 1024)])
def test_layernorm(rows, W):
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, W, generator=gen) * 3 + 0.5
    w, b = torch.randn(W, generator=gen), torch.randn(W, generator=gen)
    ref = F.layer_norm(x.double(), (W,), w.double(), b.double(), 1e-5)
    y = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV)).cpu()
    assert float((y.double() - ref).abs().max()) < 2e-5
    y16 = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out_f16=True).float().cpu()
    assert relerr(y16, ref) < 2e-3


@pytest.mark.parametrize("nseq,L,heads,causal", [(24, 50, 12, False), (3, 197, 12, False), (5, 101, 2, False),
                                                 (4, 161, 2, False), (16, 32, 8, True), (3, 77, 8, True), (2, 1, 2, False),
                                                 (2, 7, 2, True)])
def test_attention(nseq, L, heads, causal):
    from centerclip_amd import ops
    W = heads * 64
    gen = torch.Generator().manual_seed(L * 7 + heads)
    qkv = (torch.randn(nseq * L, 3 * W, generator=gen) * 1.5).half()
    q, k, v = qkv.double().view(nseq, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-2, -1) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(nseq * L, W)
    y = ops.attention_f16(qkv.to(DEV), nseq, L, heads, causal).float().cpu()
    assert float((y.double() - ref).abs().max()) < 4e-3 * float(ref.abs().max())


def _attention_sweep():
    rng = np.random.default_rng(20260930)
    edge_l = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 50, 55, 56, 57, 63, 64, 65, 100, 128, 129, 197, 255, 256]
    return [(int(rng.integers(1, 9)), int(L), int(rng.integers(1, 5)), bool(rng.integers(0, 2))) for L in edge_l]


@pytest.mark.parametrize("nseq,L,heads,causal", _attention_sweep())
def test_attention_length_sweep(nseq, L, heads, causal):
    """Sequence lengths around the 16-row query tiles, the 56-token switch between the wave and the workgroup kernel and
    the 256-token limit, with and without the causal mask."""
    test_attention(nseq, L, heads, causal)


def _gemm_sweep():
    rng = np.random.default_rng(20261001)
    out = []
    for c in range(28):
        M = int(rng.choice([1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 1000, 2400]))
        N = int(rng.integers(1, 17)) * 64
        K = int(rng.integers(1, 17)) * 64
        epi = str(rng.choice(["f16", "f16_gelu", "f32", "f32_resid"]))
        tiles = [t for t in (1, 2, 3, 4, 5, 6, 7, 8) if N % {1: 128, 2: 64, 3: 128, 4: 64, 5: 256, 6: 128, 7: 192, 8: 64}[t] == 0
                 and (t != 7 or epi.startswith("f16")) and (t != 8 or K % 128 == 0)]
        out.append((c, M, N, K, epi, int(rng.choice(tiles))))
    # tile 10 (128 x 256, 8 waves) joins the forced tiles: cases of its own, drawn behind the ones above so that those keep
    # their shapes
    for c, epi in enumerate(["f16", "f16_gelu", "f32", "f32_resid"], start=28):
        M = int(rng.choice([1, 127, 128, 129, 257, 300, 513, 2400]))
        out.append((c, M, int(rng.integers(1, 5)) * 256, int(rng.integers(1, 17)) * 64, epi, 10))
    return out


@pytest.mark.parametrize("c,M,N,K,epi,tile", _gemm_sweep())
def test_linear_f16_shape_sweep(c, M, N, K, epi, tile):
    """Seeded sweep over (M, N, K, epilogue, tile): ragged last row tiles, single-tile problems, every tile shape the
    dispatcher can be forced to; the automatic choice must give the forced tile's result (same k order) bit for bit."""
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(9000 + c)
    a = torch.randn(M, K, generator=gen).half()
    w = (torch.randn(N, K, generator=gen) * K ** -0.5).half()
    bias = torch.randn(N, generator=gen)
    ref = a.double() @ w.double().t() + bias.double()
    resid = torch.randn(M, N, generator=gen)
    outs = []
    for t in (tile, 0):
        if epi == "f32_resid":
            out = resid.to(DEV).clone()
            ops.linear_f16(a.to(DEV), w.to(DEV), bias.to(DEV), epi, out=out, tile=t)
            want, tol = ref + resid.double(), 2e-4
        else:
            out = ops.linear_f16(a.to(DEV), w.to(DEV), bias.to(DEV), epi, tile=t)
            want = ref * torch.sigmoid(1.702 * ref) if epi == "f16_gelu" else ref
            tol = 2e-4 if epi == "f32" else 2e-3
        assert relerr(out.float().cpu(), want) < tol, (M, N, K, epi, t)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), (M, N, K, epi, tile)


# ------------------------------------------------------------------------------- small model vs reference goldens
def small_model(g, cluster):
    from centerclip_amd.clip import build_clip_model
    T = int(g["cfg"][11])
    args = Namespace(cluster_inter=int(cluster), cluster_algo='kmediods++', max_frames=T,
                     target_frames_blocks=[4, 2, 2], cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean',
                     cluster_threshold=1e-6, cluster_iter_limit=100, minkowski_norm_p=2.0,
                     pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False)
    model, cfg = build_clip_model(golden_state_dict(g), args=args)
    return model.to(DEV), T


def nrm(x):
    return x / x.norm(dim=-1, keepdim=True)


def test_small_visual_forward_given_reference_medoids(g):
    model, T = small_model(g, cluster=True)
    video = torch.from_numpy(g["video"]).to(DEV)
    feat, hidden = model.visual.encode(video, T, want_hidden=True, forced_medoids=torch.from_numpy(g["v_medoids"]))
    ref, refh = torch.from_numpy(g["v_feat"]), torch.from_numpy(g["v_hidden"])
    assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3
    assert relerr(feat.cpu(), ref) <= 1e-3
    assert relerr(hidden.cpu(), refh) <= 1e-3
    # reference-shaped API: encode_image -> (features, cluster_loss)
    f2, closs = model.encode_image(video, video_frame=T)
    assert f2.shape == ref.shape and float(closs) == 0.0


def test_small_visual_forward_own_medoids_close_or_reported(g):
    """End to end with the HIP k-medoids: medoid sets on generic floats are not a bit-exact target
    (P3); report agreement and check the embedding only where the sets agree."""
    model, T = small_model(g, cluster=True)
    video = torch.from_numpy(g["video"]).to(DEV)
    feat, _ = model.visual.encode(video, T, want_medoids=True)
    med = model.visual.last_medoids.cpu().numpy()
    same = np.array_equal(med, g["v_medoids"])
    print(f"[small ViT] own medoids identical to the reference's: {same}")
    if same:
        assert float((nrm(feat.cpu()) - nrm(torch.from_numpy(g["v_feat"]))).abs().max()) <= 1e-3


def test_small_visual_forward_without_cluster(g):
    model, T = small_model(g, cluster=False)
    feat, _ = model.encode_image(torch.from_numpy(g["video"]).to(DEV), video_frame=T)
    ref = torch.from_numpy(g["v_feat_nocluster"])
    assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3
    assert relerr(feat.cpu(), ref) <= 1e-3


def test_small_text_forward(g):
    model, _ = small_model(g, cluster=False)
    feat = model.encode_text(torch.from_numpy(g["t_ids"]).to(DEV))
    ref = torch.from_numpy(g["t_feat"])
    assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3
    assert relerr(feat.cpu(), ref) <= 1e-3


def test_paired_towers_equal_separate_encodes(g):
    """cc_clip_encode (text blocks riding in the ViT's launches) gives bit-identical features to
    cc_vit_encode + cc_text_encode: same kernels, same per-problem arithmetic, different grids."""
    model, T = small_model(g, cluster=True)
    video = torch.from_numpy(g["video"]).to(DEV)
    ids = torch.from_numpy(g["t_ids"]).to(DEV)
    v1, _ = model.encode_image(video, video_frame=T)
    t1 = model.encode_text(ids)
    v2, t2 = model.encode_pair(video, ids, video_frame=T)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)


def test_loose_similarity_and_mask(g):
    from centerclip_amd import ops
    seq, vis = torch.from_numpy(g["s_seq"]).to(DEV), torch.from_numpy(g["s_vis"]).to(DEV)
    m3 = torch.from_numpy(g["s_mask3"]).to(DEV)
    logits, pooled = ops.loose_similarity(seq.squeeze(1), vis, m3, float(g["s_logit_scale"]), return_pooled=True)
    np.testing.assert_allclose(logits.cpu().numpy(), g["s_logits"], rtol=0, atol=2e-5)
    ref_pool = clo.mean_pool_visual(torch.from_numpy(g["s_vis"]), torch.from_numpy(g["s_mask3"]))
    np.testing.assert_allclose(pooled.cpu().numpy(), ref_pool.numpy(), rtol=0, atol=2e-6)


def test_clip4clip_module_eval_path(g):
    """CLIP4Clip.forward -> get_similarity_logits with the reference's calling convention (main.py:430-449,518)."""
    from centerclip_amd.clip4clip import CLIP4Clip
    T = int(g["cfg"][11])
    cfg = Namespace(cluster_inter=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 4, 4],
                    cluster_num_blocks=[16, 16, 16], cluster_distance='euclidean', cluster_threshold=1e-6,
                    cluster_iter_limit=100, minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None,
                    pre_norm=False, loose_type=True, sim_header='meanP', linear_patch='2d')
    sd = golden_state_dict(g)
    model = CLIP4Clip.from_state_dict(sd, cfg).to(DEV).eval()
    B = 2
    video = torch.from_numpy(g["video"]).view(B, 1, T, 3, 64, 64).to(DEV)
    vmask = torch.ones(B, 1, T, dtype=torch.long, device=DEV)
    vmask[1, 0, 2:] = 0
    ids = torch.from_numpy(g["t_ids"]).to(DEV)
    amask = (ids > 0).long()
    out = model(ids, torch.zeros_like(ids), amask, video, vmask)
    assert out["sequence_output"].shape == (3, 1, 64) and out["visual_output"].shape == (B, T, 64)
    logits, extra = model.get_similarity_logits(out["sequence_output"], out["visual_output"], amask, vmask)
    assert extra == () and logits.shape == (3, B)
    vfeat = clo.visual_forward(sd, torch.from_numpy(g["video"]), T).view(B, T, 64)
    tfeat = clo.text_forward(sd, torch.from_numpy(g["t_ids"])).view(3, 1, 64)
    ref = clo.loose_similarity(tfeat, vfeat, vmask.view(B, T).cpu(), float(sd["logit_scale"]))
    scale = float(torch.tensor(float(sd["logit_scale"])).exp())
    assert float((logits.cpu() - ref).abs().max()) <= 1e-3 * scale          # cosine similarities within 1e-3


# ------------------------------------------------------------------------------- full-size ViT-B/32 vs fp32 oracle
def test_vitb32_full_size_against_fp32_oracle():
    """ViT-B/32, 12 frames -> 3 segments at block 7, K=49 (MSR-VTT shaped, one clip), random weights with
    CLIP's init statistics rounded through fp16.  HIP (fp16 MFMA operands) vs the plain fp32 CPU oracle
    given the HIP path's own medoid ids."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(0)
    args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=12,
                     target_frames_blocks=[12] * 6 + [3] * 6, cluster_num_blocks=[49] * 12,
                     cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False)
    model = CLIP(512, 224, 12, 768, 32, 77, 49408, 512, 8, 12, video_frames=12, args=args)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    video = torch.randn(12, 3, 224, 224)
    feat, _ = model.visual.encode(video.to(DEV), 12, want_medoids=True)
    med = model.visual.last_medoids.cpu()
    assert med.shape == (3, 49) and bool((med[:, 1:] > med[:, :-1]).all())
    ref = clo.visual_forward(sd, video, 12, cluster_plan={6: (3, 49)}, forced_medoids={6: med})
    d = float((nrm(feat.cpu()) - nrm(ref)).abs().max())
    print(f"[ViT-B/32 full] max|delta| normalised embedding = {d:.2e}; raw rel = {relerr(feat.cpu(), ref):.2e}")
    assert d <= 1e-3
    ids = torch.zeros(4, 32, dtype=torch.long)
    for b in range(4):
        ln = 6 + 5 * b
        ids[b, 0], ids[b, ln - 1] = 49406, 49407
        ids[b, 1:ln - 1] = torch.randint(1, 49405, (ln - 2,))
    tfeat = model.encode_text(ids.to(DEV)).cpu()
    tref = clo.text_forward(sd, ids)
    dt = float((nrm(tfeat) - nrm(tref)).abs().max())
    print(f"[text full] max|delta| normalised embedding = {dt:.2e}")
    assert dt <= 1e-3
    sim = nrm(tfeat) @ nrm(feat.cpu()).t()
    simref = nrm(tref) @ nrm(ref).t()
    assert float((sim - simref).abs().max()) <= 1e-3


def test_vitb32_activitynet_shape_against_fp32_oracle():
    """BASELINE.json configs[3] shape, one clip: ViT-B/32, 64 frames -> 8 segments at block 7, K=49: 8 problems of
    N = 392 tokens (the distance matrix does not fit LDS: the global-memory form of the selection kernel).  HIP vs
    the fp32 CPU oracle given the HIP path's own medoid ids; the ids themselves obey the structural contract."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(1)
    args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=64,
                     target_frames_blocks=[64] * 6 + [8] * 6, cluster_num_blocks=[49] * 12,
                     cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False)
    model = CLIP(512, 224, 12, 768, 32, 77, 49408, 512, 8, 12, video_frames=64, args=args)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    video = torch.randn(64, 3, 224, 224)
    feat, _ = model.visual.encode(video.to(DEV), 64, want_medoids=True)
    med = model.visual.last_medoids.cpu()
    assert feat.shape == (8, 512) and med.shape == (8, 49)
    assert bool((med[:, 1:] > med[:, :-1]).all()) and int(med.min()) >= 0 and int(med.max()) < 8 * 49
    ref = clo.visual_forward(sd, video, 64, cluster_plan={6: (8, 49)}, forced_medoids={6: med})
    d = float((nrm(feat.cpu()) - nrm(ref)).abs().max())
    print(f"[ViT-B/32 64f] max|delta| normalised embedding = {d:.2e}")
    assert d <= 1e-3


def _model_sweep():
    rng = np.random.default_rng(20261003)
    out = []
    for c in range(8):
        heads = int(rng.integers(1, 4))
        layers = int(rng.integers(2, 5))
        patch, res = (16, 64) if rng.integers(0, 2) else (32, 96)
        n = (res // patch) ** 2
        T_new = int(rng.choice([1, 2, 3]))
        fd = int(rng.choice([1, 2, 4]))
        K = int(rng.integers(1, min(fd * n, 12) + 1))
        if fd == 1 and K >= n:
            K = n - 1
        cblock = int(rng.integers(2, layers + 1))            # 1-based block whose input is clustered (block 1 cannot be:
        #                                                      its 'tokens before' is cluster_num_blocks[0] itself, cluster.py:26-27)
        theads = int(rng.integers(1, 3))
        out.append((c, heads, layers, patch, res, T_new * fd, T_new, K, cblock, theads, int(rng.integers(2, 5)),
                    int(rng.integers(4, 21)), int(rng.integers(1, 4))))
    return out


@pytest.mark.parametrize("c,heads,layers,patch,res,T,T_new,K,cblock,theads,tlayers,Lt,B", _model_sweep())
def test_small_model_sweep_against_fp32_oracle(c, heads, layers, patch, res, T, T_new, K, cblock, theads, tlayers, Lt, B):
    """Seeded sweep over tiny CLIP configurations (widths 64-192, 2-4 blocks, 16- and 32-pixel patches, the cluster block
    anywhere, text towers shorter and longer than the visual one so the paired launches run out on either side): both
    towers through the fused forward vs the plain fp32 oracle given the HIP path's own medoids, <= 1e-3 on the
    normalised embeddings."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(100 + c)
    W, Wt, n = heads * 64, theads * 64, (res // patch) ** 2
    args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T,
                     target_frames_blocks=[T] * (cblock - 1) + [T_new] * (layers - cblock + 1),
                     cluster_num_blocks=[n] * (cblock - 1) + [K] * (layers - cblock + 1),
                     cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/%d' % patch, aggregation=None, pre_norm=False)
    model = CLIP(64, res, layers, W, patch, 24, 1000, Wt, theads, tlayers, video_frames=T, args=args)
    with torch.no_grad():
        for prm in model.parameters():
            prm.copy_(prm.half().float())
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    video = torch.randn(B * T, 3, res, res)
    feat, _ = model.visual.encode(video.to(DEV), T, want_medoids=True)
    med = model.visual.last_medoids.cpu()
    assert feat.shape == (B * T_new, 64) and med.shape == (B * T_new, K)
    ref = clo.visual_forward(sd, video, T, cluster_plan={cblock - 1: (T_new, K)}, forced_medoids={cblock - 1: med})
    assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3
    ids = torch.zeros(B, Lt, dtype=torch.long)
    for b in range(B):
        ln = min(Lt, 3 + b)
        ids[b, 0], ids[b, ln - 1] = 998, 999
        ids[b, 1:ln - 1] = torch.randint(1, 997, (max(ln - 2, 0),))
    tfeat = model.encode_text(ids.to(DEV)).cpu()
    assert float((nrm(tfeat) - nrm(clo.text_forward(sd, ids))).abs().max()) <= 1e-3
    # the paired encode of both towers gives the separate encodes' values
    both_v, both_t = model.encode_pair(video.to(DEV), ids.to(DEV), video_frame=T)
    assert torch.equal(both_v.cpu(), feat.cpu()) and torch.equal(both_t.cpu(), tfeat)


def test_vitb16_shape_against_fp32_oracle():
    """BASELINE.json configs[4] shape, one clip: ViT-B/16 (196 tokens per frame, L = 197: the long-sequence attention
    kernel), 12 frames -> 4 segments at block 7, K = 100: 4 problems of N = 588 tokens.  HIP vs the fp32 CPU oracle given
    the HIP path's own medoid ids."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(2)
    args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=12,
                     target_frames_blocks=[12] * 6 + [4] * 6, cluster_num_blocks=[100] * 12,
                     cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/16', aggregation=None, pre_norm=False)
    model = CLIP(512, 224, 12, 768, 16, 77, 49408, 512, 8, 12, video_frames=12, args=args)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.half().float())
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    video = torch.randn(12, 3, 224, 224)
    feat, _ = model.visual.encode(video.to(DEV), 12, want_medoids=True)
    med = model.visual.last_medoids.cpu()
    assert feat.shape == (4, 512) and med.shape == (4, 100)
    assert bool((med[:, 1:] > med[:, :-1]).all()) and int(med.min()) >= 0 and int(med.max()) < 3 * 196
    ref = clo.visual_forward(sd, video, 12, cluster_plan={6: (4, 100)}, forced_medoids={6: med})
    d = float((nrm(feat.cpu()) - nrm(ref)).abs().max())
    print(f"[ViT-B/16 12f] max|delta| normalised embedding = {d:.2e}")
    assert d <= 1e-3


def _similarity_sweep():
    rng = np.random.default_rng(20261002)
    return [(c, int(rng.integers(1, 130)), int(rng.integers(1, 130)), int(rng.integers(1, 9)), int(rng.choice([64, 128, 512, 1024])))
            for c in range(16)]


@pytest.mark.parametrize("c,Bt,Bv,Tn,E", _similarity_sweep())
def test_similarity_and_rank_shape_sweep(c, Bt, Bv, Tn, E):
    """Seeded sweep over (Bt, Bv, T_new, E): both forms of the meanP similarity (one-launch tail for Bt x Bv <= 4096, pooled
    + exact-fp32 MFMA GEMM above) against the oracle within 1e-3 of the logit scale, random masks with fully masked clips;
    then the rank counts of the result against a NumPy count, exactly."""
    from centerclip_amd import ops
    from centerclip_amd.metrics import rank_counts
    gen = torch.Generator().manual_seed(9100 + c)
    text, vis = torch.randn(Bt, E, generator=gen), torch.randn(Bv, Tn, E, generator=gen)
    mask = (torch.rand(Bv, Tn, generator=gen) > 0.25).long()
    if Bv > 2:
        mask[1] = 0
    logits = ops.loose_similarity(text.to(DEV), vis.to(DEV), mask.to(DEV), 1.3)
    ref = clo.loose_similarity(text.view(Bt, 1, E), vis, mask, 1.3)
    got = logits.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert float((got[ok] - ref[ok]).abs().max()) <= 1e-3 * float(torch.tensor(1.3).exp())
    sim = torch.nan_to_num(logits, nan=-1e30)
    R = min(Bt, Bv)
    counts = rank_counts(sim[:R].contiguous()).cpu().numpy()
    sn = sim[:R].cpu().numpy()
    d = sn[np.arange(R), np.arange(R)]
    assert np.array_equal(counts[:, 0], (sn > d[:, None]).sum(1)) and np.array_equal(counts[:, 1], (sn == d[:, None]).sum(1))


def test_n1_retrieval_metrics_match_reference(g):
    """compute_metrics on the device (2 ints per row) == utils/metrics.py:11-26 incl. its tie behaviour."""
    from centerclip_amd.metrics import compute_metrics
    sim = torch.from_numpy(g["n1_sim"]).to(DEV)
    t2v, v2t = compute_metrics(sim), compute_metrics(sim.T)
    for got, ref, cols in ((t2v, g["n1_t2v"], g["n1_t2v_cols"]), (v2t, g["n1_v2t"], None)):
        np.testing.assert_allclose([got["R1"], got["R5"], got["R10"], got["MR"], got["MeanR"]], ref, rtol=0, atol=1e-12)
        if cols is not None:
            assert got["cols"] == [int(c) for c in cols]
    assert len(t2v["cols"]) == 41            # the tie with the diagonal yields an extra entry, as in the reference


def test_n1_multi_sentence_metrics_match_reference():
    """tensor_text_to_video_metrics / tensor_video_to_text_sim (utils/metrics.py:38-76) on the device == the
    reference's numbers on a ragged 12-video / 33-sentence problem (fixture from the reference itself)."""
    from centerclip_amd.metrics import compute_metrics, tensor_text_to_video_metrics, tensor_video_to_text_sim
    gm = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics_multi_golden.npz"))
    sim3 = torch.from_numpy(gm["sim3"]).to(DEV)
    tv = tensor_text_to_video_metrics(sim3)
    np.testing.assert_allclose([tv["R1"], tv["R5"], tv["R10"], tv["MedianR"], tv["MeanR"], tv["Std_Rank"]], gm["tv"],
                               rtol=0, atol=1e-12)
    v2t = tensor_video_to_text_sim(sim3)
    assert np.array_equal(v2t.cpu().numpy(), gm["v2t_sim"])
    vt = compute_metrics(v2t)
    np.testing.assert_allclose([vt["R1"], vt["R5"], vt["R10"], vt["MR"], vt["MeanR"]], gm["vt"], rtol=0, atol=1e-12)


def test_edge_similarity_shapes_and_masks():
    """1 x 1 logits, a fully masked clip (denominator 0 -> 1, clip4clip.py:313) and a mask given as int64."""
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(3)
    for Bt, Bv, Tn, E in ((1, 1, 1, 64), (3, 2, 5, 512), (65, 67, 3, 512)):
        t = torch.randn(Bt, 1, E, generator=gen)
        v = torch.randn(Bv, Tn, E, generator=gen)
        m = (torch.rand(Bv, Tn, generator=gen) > 0.4).long()
        m[0] = 0
        ref = clo.loose_similarity(t, v, m, 0.7)
        got = ops.loose_similarity(t.squeeze(1).to(DEV), v.to(DEV), m.to(DEV), 0.7).cpu()
        assert got.shape == (Bt, Bv)
        # a fully masked clip pools to 0 -> 0/0 = NaN in both implementations (clip 0 always, others by chance)
        dead = m.sum(1) == 0
        assert bool(dead[0]) and bool(torch.isnan(ref[:, dead]).all()) and bool(torch.isnan(got[:, dead]).all())
        assert bool(torch.isfinite(ref[:, ~dead]).all())
        np.testing.assert_allclose(got[:, ~dead].numpy(), ref[:, ~dead].numpy(), rtol=0, atol=3e-5)


@pytest.mark.parametrize("Bt,Bv", [(5, 7), (80, 70)])          # one-launch tail / pooled + MFMA path
def test_similarity_takes_the_segment_mask_as_a_strided_view(Bt, Bv):
    """The mask after clustering is every fd-th column of the frame mask (clip4clip.py:436-447): the similarity entry reads it
    through strides - same logits as with a gathered copy, and the NaN pattern of fully masked clips is kept."""
    from centerclip_amd import ops
    gen = torch.Generator().manual_seed(Bt * 100 + Bv)
    T, Tn, E = 12, 3, 512
    text = torch.randn(Bt, E, generator=gen).to(DEV)
    vis = torch.randn(Bv, Tn, E, generator=gen).to(DEV)
    frame_mask = (torch.rand(Bv, T, generator=gen) > 0.3).long()
    frame_mask[0] = 0                                             # a fully masked clip
    frame_mask = frame_mask.to(DEV)
    view = frame_mask[:, T // Tn - 1::T // Tn]
    assert not view.is_contiguous() and view.shape == (Bv, Tn)
    a = ops.loose_similarity(text, vis, view, 0.7)
    b = ops.loose_similarity(text, vis, view.contiguous(), 0.7)
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    ref = clo.loose_similarity(text.cpu().view(Bt, 1, E), vis.cpu(), view.cpu().contiguous(), 0.7)
    ok = ~torch.isnan(ref)
    assert float((a.cpu()[ok] - ref[ok]).abs().max()) <= 1e-3 * float(torch.tensor(0.7).exp())


def test_n3_uint8_frames_bit_identical_to_loader_path(g):
    """N3: uint8 frames (CHW and the decoder's HWC) through the fused normalise + patch gather give the same
    bits as the reference pipeline loader_normalize -> encode_image, and match the oracle forward."""
    model, T = small_model(g, cluster=True)
    res = int(g["video"].shape[-1])
    rng = np.random.default_rng(11)
    u_hwc = torch.from_numpy(rng.integers(0, 256, size=(g["video"].shape[0], res, res, 3), dtype=np.uint8))
    u_chw = u_hwc.permute(0, 3, 1, 2).contiguous()
    x = clo.loader_normalize(u_hwc, channels_last=True)
    f_ref, _ = model.visual.encode(x.to(DEV), T)
    f_chw, _ = model.visual.encode(u_chw.to(DEV), T)
    f_hwc, _ = model.visual.encode(u_hwc.to(DEV), T)
    assert torch.equal(f_chw, f_ref) and torch.equal(f_hwc, f_ref)
    # both towers in one enqueue, uint8 video in the reference's 6-d batch layout
    ids = torch.from_numpy(g["t_ids"]).to(DEV)
    v1, t1 = model.encode_pair(x.to(DEV), ids, video_frame=T)
    v2, t2 = model.encode_pair(u_hwc.to(DEV), ids, video_frame=T)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    med = model.visual.encode(u_chw.to(DEV), T, want_medoids=True) and model.visual.last_medoids
    ref = clo.visual_forward(golden_state_dict(g), x, T, cluster_plan={1: (2, 6)}, forced_medoids={1: med.cpu()})
    f_forced, _ = model.visual.encode(u_chw.to(DEV), T, forced_medoids=med)
    assert float((nrm(f_forced.cpu()) - nrm(ref)).abs().max()) <= 1e-3
    with pytest.raises(ValueError):
        model.visual.encode(torch.zeros(4, 5, 64, 64, dtype=torch.uint8, device=DEV), T)


def test_forced_medoids_with_two_cluster_blocks(g):
    """Round 5: the "given identical medoid sets" hook for plans with MORE than one cluster block (4 -> 2 frames with K = 8 in
    block 1, 2 -> 1 with K = 4 in block 2): the id tensors of the blocks back to back; features and hidden state vs the fp32
    oracle given the same ids (clip.py:236-242 twice)."""
    from centerclip_amd.clip import build_clip_model
    T = int(g["cfg"][11])
    args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[2, 1, 1],
                     cluster_num_blocks=[8, 4, 4], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False)
    model, _ = build_clip_model(golden_state_dict(g), args=args)
    model = model.to(DEV)
    video = torch.from_numpy(g["video"])
    B = video.shape[0] // T
    n = (video.shape[-1] // int(golden_state_dict(g)["visual.conv1.weight"].shape[-1])) ** 2
    gen = torch.Generator().manual_seed(5)
    m0 = torch.stack([torch.randperm((T // 2) * n, generator=gen)[:8].sort().values for _ in range(B * 2)])
    m1 = torch.stack([torch.randperm(2 * 8, generator=gen)[:4].sort().values for _ in range(B * 1)])
    feat, hidden = model.visual.encode(video.to(DEV), T, want_hidden=True, forced_medoids=[m0, m1])
    ref, refh = clo.visual_forward(golden_state_dict(g), video, T, cluster_plan={0: (2, 8), 1: (1, 4)},
                                   forced_medoids={0: m0, 1: m1}, return_hidden=True)
    assert feat.shape == ref.shape == (B, ref.shape[1]) and hidden.shape == refh.shape
    assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3 and relerr(hidden.cpu(), refh) <= 1e-3
    own, _ = model.visual.encode(video.to(DEV), T)                 # (and the plan runs with its own k-medoids in both blocks)
    assert own.shape == feat.shape and bool(torch.isfinite(own).all())


@pytest.mark.parametrize("algo,agg", [("pooling", None), ("sparse_sampling", None), ("kmediods++", "mean")])
def test_n2_variants_inside_the_fused_forward(g, algo, agg):
    """The per-block cc_cluster_variant array of cc_vit_model: 'pooling' and eval-mode 'sparse_sampling' (no
    data-dependent selection) agree with the oracle forward; aggregation='mean' runs and is deterministic (its
    arithmetic is pinned at the operator level in test_cluster_gpu.py)."""
    from centerclip_amd.clip import build_clip_model
    T = int(g["cfg"][11])
    n = (int(g["video"].shape[-1]) // int(g["cfg"][2])) ** 2
    K = n if algo == "pooling" else 6
    args = Namespace(cluster_inter=1, cluster_algo=algo, max_frames=T, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[n, K, K], cluster_distance='euclidean', cluster_threshold=1e-6,
                     cluster_iter_limit=100, minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=agg,
                     pre_norm=False)
    model, _ = build_clip_model(golden_state_dict(g), args=args)
    model = model.to(DEV).eval()
    video = torch.from_numpy(g["video"])
    feat, hidden = model.visual.encode(video.to(DEV), T, want_hidden=True)
    feat2, _ = model.visual.encode(video.to(DEV), T)
    feat3, _ = model.visual.encode(video.to(DEV), T)
    # deterministic; with the hidden state requested the last block computes every row instead of the CLS rows only (other
    # GEMM tiles: agreement to rounding, tests/test_r2_gpu.py::test_last_block_runs_on_the_rows_the_heads_read)
    assert torch.equal(feat2, feat3) and bool(torch.isfinite(feat).all())
    assert float((feat - feat2).abs().max() / feat.abs().max()) < 2e-4
    assert hidden.shape == (video.shape[0] // T * 2, 1 + K, int(g["cfg"][3]))
    if agg is None:
        ref = clo.visual_forward(golden_state_dict(g), video, T, cluster_plan={1: (2, K)},
                                 cluster_cfg=dict(algorithm=algo, aggregation=None))
        assert float((nrm(feat.cpu()) - nrm(ref)).abs().max()) <= 1e-3


def test_forward_is_deterministic(g):
    model, T = small_model(g, cluster=True)
    video = torch.from_numpy(g["video"]).to(DEV)
    ids = torch.from_numpy(g["t_ids"]).to(DEV)
    a = model.encode_pair(video, ids, video_frame=T)
    b = model.encode_pair(video, ids, video_frame=T)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
