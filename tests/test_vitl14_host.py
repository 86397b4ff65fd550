"""ViT-L/14 on the host: the geometry build_clip_model reads from a state dict with a 14 x 14 conv1 and a 257-row positional
embedding, the checkpoint names, the conv1 weight packed with zero columns up to a multiple of 64, the fake kernels' shapes,
the argument checks of the entry points that need no GPU.  No GPU needed."""
import ctypes

import pytest
import torch


def _tiny_l14_sd(width=128, layers=2, embed=64, text_width=64, text_layers=1, vocab=100):
    """A synthetic state dict with ViT-L/14's geometry keys at a small width: conv1 [W, 3, 14, 14], 257 position rows."""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g) * 0.02
    sd = {"visual.conv1.weight": r(width, 3, 14, 14), "visual.class_embedding": r(width),
          "visual.positional_embedding": r(257, width), "visual.ln_pre.weight": torch.ones(width),
          "visual.ln_pre.bias": torch.zeros(width), "visual.ln_post.weight": torch.ones(width),
          "visual.ln_post.bias": torch.zeros(width), "visual.proj": r(width, embed),
          "text_projection": r(text_width, embed), "positional_embedding": r(77, text_width),
          "token_embedding.weight": r(vocab, text_width), "ln_final.weight": torch.ones(text_width),
          "ln_final.bias": torch.zeros(text_width), "logit_scale": torch.tensor(2.0)}
    for prefix, n, w in (("visual.transformer.resblocks.", layers, width), ("transformer.resblocks.", text_layers, text_width)):
        for i in range(n):
            b = prefix + "%d." % i
            sd.update({b + "attn.in_proj_weight": r(3 * w, w), b + "attn.in_proj_bias": r(3 * w),
                       b + "attn.out_proj.weight": r(w, w), b + "attn.out_proj.bias": r(w),
                       b + "ln_1.weight": torch.ones(w), b + "ln_1.bias": torch.zeros(w),
                       b + "mlp.c_fc.weight": r(4 * w, w), b + "mlp.c_fc.bias": r(4 * w),
                       b + "mlp.c_proj.weight": r(w, 4 * w), b + "mlp.c_proj.bias": r(w),
                       b + "ln_2.weight": torch.ones(w), b + "ln_2.bias": torch.zeros(w)})
    return sd


def test_geometry_is_read_from_the_state_dict():
    from centerclip_amd.clip import build_clip_model
    sd = _tiny_l14_sd()
    model, cfg = build_clip_model(dict(sd), args=None)
    assert cfg["vision_patch_size"] == 14 and cfg["image_resolution"] == 224 and cfg["vision_width"] == 128
    assert cfg["vision_layers"] == 2 and cfg["embed_dim"] == 64 and cfg["transformer_width"] == 64 and cfg["transformer_layers"] == 1
    vis = model.visual
    assert (vis.patch_size, vis.input_resolution, vis.heads, vis.width) == (14, 224, 2, 128)
    assert vis.positional_embedding.shape == (257, 128) and vis.final_shape(3) == (3, 257)
    assert torch.equal(vis.conv1.weight, sd["visual.conv1.weight"])
    # the real checkpoint's geometry, shapes only (no parameters are allocated for the check)
    full = {"visual.conv1.weight": torch.empty(1024, 3, 14, 14, device="meta"),
            "visual.positional_embedding": torch.empty(257, 1024, device="meta")}
    assert full["visual.conv1.weight"].shape[0] // 64 == 16 and round((257 - 1) ** 0.5) * 14 == 224
    assert round((577 - 1) ** 0.5) * 14 == 336                       # ViT-L/14@336px: 577 position rows


def test_checkpoint_names(tmp_path):
    from centerclip_amd import clip
    assert clip._PT_NAME["ViT-L/14"] == "ViT-L-14.pt" and clip._PT_NAME["ViT-L/14@336px"] == "ViT-L-14-336px.pt"
    assert clip._PT_NAME["ViT-B/32"] == "ViT-B-32.pt" and clip._PT_NAME["ViT-B/16"] == "ViT-B-16.pt"
    for name, fn in (("ViT-L/14", "ViT-L-14.pt"), ("ViT-L/14@336px", "ViT-L-14-336px.pt")):
        with pytest.raises(FileNotFoundError, match=fn.replace(".", r"\.")):
            clip.load_clip_state_dict(name, str(tmp_path))
    sd = {"visual.proj": torch.zeros(2, 2)}
    torch.save(sd, str(tmp_path / "ViT-L-14.pt"))
    assert set(clip.load_clip_state_dict("ViT-L/14", str(tmp_path))) == {"visual.proj"}
    with pytest.raises(NotImplementedError):
        clip.load_clip_state_dict("RN50", str(tmp_path))


def test_split_size_rule():
    """cluster.py:15-63: split_size 4 for 'ViT-B/16', 16 for every other name - 'ViT-L/14' included."""
    from argparse import Namespace
    from centerclip_amd.cluster import get_cluster_inter
    for name, split in (("ViT-B/16", 4), ("ViT-B/32", 16), ("ViT-L/14", 16), ("ViT-L/14@336px", 16)):
        args = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=4, target_frames_blocks=[2, 2],
                         cluster_num_blocks=[64, 64], cluster_distance='euclidean', cluster_threshold=1e-6,
                         cluster_iter_limit=100, minkowski_norm_p=2.0, pretrained_clip_name=name, aggregation=None, pre_norm=False)
        assert get_cluster_inter(128, 1, args).split_size == split


@pytest.mark.parametrize("p,cols", [(14, 640), (32, 3072), (16, 768), (8, 192), (7, 192), (12, 448)])
def test_packed_conv1_weight(p, cols):
    """[W, 3, p, p] -> [W, roundup(3 p^2, 64)] fp16: the oracle's reshape (clip_oracle._visual_forward_native: weight.reshape(W, -1),
    columns (c, kh, kw)) in the first 3 p^2 columns, exact zeros behind."""
    from centerclip_amd.clip import pack_conv1_weight
    from centerclip_amd.torch_ops import patch_cols
    w = torch.randn(6, 3, p, p, generator=torch.Generator().manual_seed(p))
    packed = pack_conv1_weight(w)
    assert patch_cols(p) == cols and packed.shape == (6, cols) and packed.dtype == torch.float16 and packed.is_contiguous()
    assert torch.equal(packed[:, :3 * p * p], w.reshape(6, -1).half())
    assert not packed[:, 3 * p * p:].any()
    assert packed[2, 1 * p * p + 3 * p + 5] == w[2, 1, 3, 5].half()


def test_fake_kernel_shapes():
    """Meta-device calls of the ops whose shapes the geometry changes: the padded patch matrix and the attention output."""
    from centerclip_amd import torch_ops  # noqa: F401
    f32 = torch.empty(3, 3, 224, 224, device="meta")
    u8 = torch.empty(3, 224, 224, 3, device="meta", dtype=torch.uint8)
    for fr in (f32, u8):
        a = torch.ops.centerclip.patch_gather(fr, 224, 14)
        assert a.shape == (3 * 256, 640) and a.dtype == torch.float16
    assert torch.ops.centerclip.patch_gather(f32, 224, 32).shape == (3 * 49, 3072)
    assert torch.ops.centerclip.patch_gather(f32, 224, 16).shape == (3 * 196, 768)
    qkv = torch.empty(2 * 577, 3 * 128, device="meta", dtype=torch.float16)
    out = torch.ops.centerclip.attention_f16(qkv, 2, 577, 2, False, 577, 1)
    assert out.shape == (2 * 577, 128) and out.dtype == torch.float16


def test_entry_points_refuse_before_touching_memory():
    """Argument checks that end before any launch: NULL frames, a patch that does not divide the resolution, sequence lengths
    above the kernels' ranges (641 forward, 321 backward)."""
    from centerclip_amd import _lib as L
    from centerclip_amd._lib_clip import Frames
    lib = L.lib()
    INVALID, UNSUPPORTED = -1, lib.cc_attention_f16(ctypes.c_void_p(256), ctypes.c_void_p(256), 1, 100000, 1, 64, 0, None)
    assert UNSUPPORTED != 0 and UNSUPPORTED != INVALID
    assert b"unsupported" in lib.cc_status_string(UNSUPPORTED).lower()
    fr = Frames()
    assert lib.cc_patch_gather_any_f16(None, 2, 28, 14, None, None) == INVALID
    assert lib.cc_patch_gather_any_f16(ctypes.byref(fr), 2, 28, 14, None, None) == INVALID       # no frames, no output
    fr.data = 256                                                                                   # never dereferenced
    assert lib.cc_patch_gather_any_f16(ctypes.byref(fr), 2, 30, 14, ctypes.c_void_p(256), None) == INVALID   # 30 % 14
    p = ctypes.c_void_p(256)
    assert lib.cc_attention_f16(p, p, 2, 641, 2, 128, 0, None) == UNSUPPORTED
    assert lib.cc_attention_strided_f16(p, p, 2, 641, 2, 128, 0, 641, 1, None) == UNSUPPORTED
    assert lib.cc_attention_backward_f16(p, p, p, 2, 321, 2, 128, 0, None, p, 1 << 30, None) == UNSUPPORTED
    assert lib.cc_attention_backward_workspace_bytes(2, 320, 2) == 2 * 320 * 2 * 2 * 4


def test_training_refuses_more_than_320_tokens():
    from centerclip_amd.train import block as tb
    assert tb.MAX_TRAIN_TOKENS == 320
