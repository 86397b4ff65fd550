"""The exact GELU (OpenCLIP-format checkpoints) on the host: the two new entry points are exported and declared, the model
structs carry an ``activation`` field that a zero fill leaves at QuickGELU, ``quick_gelu=False`` reaches both towers' blocks and
not the seqTransf head, the new op has a fake kernel, an OpenCLIP-style file loads, head widths other than 64 are refused and
an unknown activation id is CC_ERR_INVALID before any pointer is read.  No GPU needed."""
import ctypes
import os
import re
from argparse import Namespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC_ERR_INVALID = -1


def _tiny_openai_sd(width=128, layers=2, embed=64, text_width=64, text_layers=1, vocab=100, patch=16, grid=2):
    """A synthetic state dict under the OpenAI / OpenCLIP key names."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g) * 0.02
    sd = {"visual.conv1.weight": r(width, 3, patch, patch), "visual.class_embedding": r(width),
          "visual.positional_embedding": r(grid * grid + 1, width), "visual.ln_pre.weight": torch.ones(width),
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


def test_new_entry_points_are_exported_and_declared():
    from centerclip_amd import _lib as L
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    for name in ("cc_gelu_f16", "cc_gelu_backward_f16"):
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define\s+CC_ACT_QUICK_GELU\s+0\b", header) and re.search(r"#define\s+CC_ACT_GELU\s+1\b", header)
    # ragged sizes and NULL operands are refused before a launch (no GPU is touched)
    p = ctypes.c_void_p(256)
    assert lib.cc_gelu_f16(p, p, 6, None) == CC_ERR_INVALID and lib.cc_gelu_f16(None, p, 8, None) == CC_ERR_INVALID
    assert lib.cc_gelu_backward_f16(p, p, p, 6, None, None) == CC_ERR_INVALID


def test_existing_epilogue_ids_keep_their_values_and_the_new_ones_follow():
    from centerclip_amd._lib_clip import EPI
    assert EPI == {"f16": 0, "f16_gelu": 1, "f32_resid": 2, "f32": 4, "f16_gelu_erf": 9}
    src = open(os.path.join(ROOT, "centerclip_amd", "csrc", "cc_kernels.h")).read()
    ids = dict((k, int(v)) for k, v in re.findall(r"\b(EPI_\w+)\s*=\s*(\d+)", src))
    assert ids == dict(EPI_F16=0, EPI_F16_GELU=1, EPI_F32_RESID=2, EPI_F32_PATCH=3, EPI_F32=4, EPI_F16_LN=5, EPI_F16_GELU_LN=6,
                       EPI_F32_RESID_STATS=7, EPI_ATTN_LN=8, EPI_F16_GELU_ERF=9, EPI_F16_GELU_ERF_LN=10)
    from centerclip_amd import _lib as L
    lib = L.lib()
    # the new ids take the tiles of their QuickGELU counterparts, whatever the shape
    for M, N, K in ((9600, 3072, 768), (2400, 3072, 768), (300, 768, 64), (48, 512, 192), (25600, 3072, 768), (520, 2048, 512)):
        assert lib.cc_linear_tile_for(M, N, K, 9) == lib.cc_linear_tile_for(M, N, K, 1) > 0
        assert lib.cc_linear_tile_for(M, N, K, 10) == lib.cc_linear_tile_for(M, N, K, 6) > 0
    assert lib.cc_linear_tile_for(300, 768, 64, 8) == CC_ERR_INVALID and lib.cc_linear_tile_for(300, 768, 64, 11) == CC_ERR_INVALID


def test_zeroed_model_structs_are_the_reference_model():
    from centerclip_amd._lib_clip import VitModel, TextModel, ACT_QUICK_GELU, ACT_GELU
    assert (ACT_QUICK_GELU, ACT_GELU) == (0, 1)
    for cls in (VitModel, TextModel):
        assert cls().activation == 0
        assert cls._fields_[-1] == ("activation", ctypes.c_int32)            # appended: earlier offsets are unchanged
        assert ctypes.sizeof(cls) % 8 == 0


def test_quick_gelu_false_reaches_both_towers_and_not_the_head():
    from centerclip_amd.clip import CLIP, build_clip_model
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd._lib_clip import ACT_GELU, ACT_QUICK_GELU
    m = CLIP(64, 32, 2, 128, 16, 77, 100, 64, 1, 1, args=None, quick_gelu=False)
    blocks = list(m.visual.transformer.resblocks) + list(m.transformer.resblocks)
    assert len(blocks) == 3 and not any(b.quick_gelu for b in blocks) and m.quick_gelu is False
    assert m.visual.transformer.activation == ACT_GELU and m.transformer.activation == ACT_GELU
    d = CLIP(64, 32, 2, 128, 16, 77, 100, 64, 1, 1, args=None)
    assert all(b.quick_gelu for b in list(d.visual.transformer.resblocks) + list(d.transformer.resblocks))
    assert d.transformer.activation == ACT_QUICK_GELU
    assert set(m.state_dict()) == set(d.state_dict())                       # a construction argument, not state
    sd = _tiny_openai_sd(text_width=64, embed=64)
    model, _ = build_clip_model(dict(sd), args=None, quick_gelu=False)
    assert not model.visual.transformer.resblocks[0].quick_gelu and not model.transformer.resblocks[0].quick_gelu
    cfg = Namespace(cluster_inter=0, cluster_algo=None, max_frames=4, target_frames_blocks=[4] * 12, cluster_num_blocks=[4] * 12,
                    cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100, minkowski_norm_p=2.0,
                    pretrained_clip_name='ViT-B/16', aggregation=None, pre_norm=False, loose_type=True, sim_header='seqTransf',
                    linear_patch='2d', cross_num_hidden_layers=2, quick_gelu=0)
    c4c = CLIP4Clip(dict(sd), cfg)
    assert not any(b.quick_gelu for b in c4c.clip.visual.transformer.resblocks)
    assert not any(b.quick_gelu for b in c4c.clip.transformer.resblocks)
    assert len(c4c.transformerClip.resblocks) == 2 and all(b.quick_gelu for b in c4c.transformerClip.resblocks)
    cfg.quick_gelu = 1
    assert all(b.quick_gelu for b in CLIP4Clip(dict(sd), cfg).clip.visual.transformer.resblocks)
    del cfg.quick_gelu                                                       # the default is the reference's model
    assert all(b.quick_gelu for b in CLIP4Clip(dict(sd), cfg).clip.transformer.resblocks)


def test_fake_kernels_of_the_new_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from centerclip_amd import torch_ops
    assert "linear_ln_act_f16" in torch_ops.OPS
    assert torch.ops.centerclip.linear_ln_act_f16.default._schema.name == "centerclip::linear_ln_act_f16"
    # the schema existing callers use positionally is unchanged
    assert "bool gelu" in str(torch.ops.centerclip.linear_ln_f16.default._schema)
    with FakeTensorMode():
        h16 = torch.empty(100, 64, device="cuda", dtype=torch.float16)
        w = torch.empty(256, 64, device="cuda", dtype=torch.float16)
        c = torch.empty(256, device="cuda")
        st = torch.empty(100, 1, 2, device="cuda")
        for act in (0, 1, 2):
            y = torch.ops.centerclip.linear_ln_act_f16(h16, w, c, c, st, 1, act, 1e-5, 0)
            assert y.shape == (100, 256) and y.dtype == torch.float16 and y.device.type == "cuda"
        y = torch.ops.centerclip.linear_f16(h16, w, None, "f16_gelu_erf", 0)
        assert y.shape == (100, 256) and y.dtype == torch.float16


def test_openclip_style_file_loads(tmp_path):
    """{'state_dict': {'module.<key>': ...}} with an attn_mask buffer and a logit_bias: unwrapped, stripped, the two dropped."""
    from centerclip_amd import clip
    sd = _tiny_openai_sd()
    wrapped = {"module." + k: v for k, v in sd.items()}
    wrapped["module.attn_mask"] = torch.full((77, 77), float("-inf")).triu_(1)
    wrapped["module.logit_bias"] = torch.tensor(-10.0)
    path = str(tmp_path / "open_clip_pytorch_model.bin")
    torch.save({"state_dict": wrapped, "epoch": 3}, path)
    got = clip.load_clip_state_dict(path)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    plain = str(tmp_path / "plain.pt")
    torch.save(sd, plain)
    assert set(clip.load_clip_state_dict(plain)) == set(sd)
    model, cfg = clip.build_clip_model(got, args=None, quick_gelu=False)
    assert cfg["vision_width"] == 128 and cfg["vision_patch_size"] == 16 and cfg["image_resolution"] == 32
    assert torch.equal(model.visual.conv1.weight, sd["visual.conv1.weight"])
    assert torch.equal(model.transformer.resblocks[0].mlp["c_fc"].weight, sd["transformer.resblocks.0.mlp.c_fc.weight"])
    # the rest of the function stays: unknown names that are no file raise as before
    with pytest.raises(NotImplementedError):
        clip.load_clip_state_dict("RN50", str(tmp_path))
    with pytest.raises(NotImplementedError):
        clip.load_clip_state_dict(str(tmp_path / "missing.bin"))
    with pytest.raises(FileNotFoundError):
        clip.load_clip_state_dict("ViT-B/32", str(tmp_path))


def test_head_widths_other_than_64_are_refused():
    from centerclip_amd.clip import build_clip_model
    sd = _tiny_openai_sd(width=320, layers=1)                              # ViT-H-like: 320 / 80 = 4 heads
    with pytest.raises(NotImplementedError, match="vision_heads"):
        build_clip_model(dict(sd), args=None, vision_heads=4)
    with pytest.raises(NotImplementedError, match="text_heads"):
        build_clip_model(dict(sd), args=None, text_heads=2)
    model, cfg = build_clip_model(dict(sd), args=None, vision_heads=5, text_heads=1)
    assert model.visual.heads == 5 and cfg["transformer_heads"] == 1


def test_unknown_activation_is_refused_before_touching_memory():
    """activation = 7 in an otherwise plausible model whose pointers are all 256: every fused entry returns CC_ERR_INVALID."""
    from centerclip_amd import _lib as L
    from centerclip_amd._lib_clip import BlockWeights, Frames, TextModel, VitModel
    lib = L.lib()
    p = ctypes.c_void_p(256)
    vm = VitModel(layers=2, width=128, heads=2, patch=16, resolution=32, embed_dim=64)
    tm = TextModel(layers=1, width=64, heads=1, context_length=77, vocab_size=100, embed_dim=64)
    for m in (vm, tm):
        m.blocks = ctypes.cast(p, ctypes.POINTER(BlockWeights))            # a HOST array: reading it would fault
    fr = Frames()
    fr.data = 256
    ws = 1 << 30

    def calls():
        return dict(
            vit_encode=lib.cc_vit_encode(ctypes.byref(vm), p, 1, 1, p, None, None, None, p, ws, None),
            vit_encode_frames=lib.cc_vit_encode_frames(ctypes.byref(vm), ctypes.byref(fr), 1, 1, p, None, None, None, p, ws, None),
            vit_prefix=lib.cc_vit_encode_prefix_frames(ctypes.byref(vm), ctypes.byref(fr), 1, 1, 1, p, None, p, ws, None),
            text_encode=lib.cc_text_encode(ctypes.byref(tm), p, 1, 8, p, p, ws, None),
            text_hidden=lib.cc_text_encode_hidden(ctypes.byref(tm), p, 1, 8, p, p, p, ws, None),
            text_prefix=lib.cc_text_encode_prefix(ctypes.byref(tm), p, 1, 8, 1, p, p, ws, None),
            clip_encode=lib.cc_clip_encode(ctypes.byref(vm), p, 1, 1, p, None, ctypes.byref(tm), p, 1, 8, p, p, ws, None),
            clip_frames=lib.cc_clip_encode_frames(ctypes.byref(vm), ctypes.byref(fr), 1, 1, p, None, None, ctypes.byref(tm), p, 1, 8,
                                                  p, p, ws, None))
    vm.activation = tm.activation = 7
    assert set(calls().values()) == {CC_ERR_INVALID}, calls()
    vm.activation, tm.activation = -1, 2
    assert set(calls().values()) == {CC_ERR_INVALID}, calls()
    vm.activation, tm.activation = 1, 7                                      # one bad tower refuses the pair
    assert lib.cc_clip_encode(ctypes.byref(vm), p, 1, 1, p, None, ctypes.byref(tm), p, 1, 8, p, p, ws, None) == CC_ERR_INVALID
    assert lib.cc_clip_encode_frames(ctypes.byref(vm), ctypes.byref(fr), 1, 1, p, None, None, ctypes.byref(tm), p, 1, 8, p, p, ws,
                                     None) == CC_ERR_INVALID
    # cc_linear_ln_f16's gelu argument: 0, 1, 2 only
    assert lib.cc_linear_ln_f16(p, p, p, p, p, 1, 1e-5, p, 64, 64, 64, 3, 0, None) == CC_ERR_INVALID
    assert lib.cc_linear_ln_f16(p, p, p, p, p, 1, 1e-5, p, 64, 64, 64, -1, 0, None) == CC_ERR_INVALID
