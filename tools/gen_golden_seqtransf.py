"""Fixture tests/golden/seqtransf_golden.npz for tests/test_seqtransf_host.py, captured from the reference (dev container
only: it imports the reference's modules/clip4clip.py, module_cross.py and losses.py).

The head is the small model of clip_golden.npz: width 128, 2 heads of 64, transformerClip with cross_num_hidden_layers = 2,
whose blocks come from the text transformer by the reference's initialisation trick.  The frame position table has 77 rows
(seeded; the small model's own context is 16 rows, too short for T = 64 / 77).

  pos                              [77, 128]   frame_position_embeddings.weight of every case
  init/names                       json        the names from_pretrained's initialisation trick adds (no fine-tuned head)
  init/<name>/{head,sketch}        their values: first 256 entries and 16 projections as below (the small model has a
                                   16-row positional_embedding)
  c/<T>/vis, c/<T>/mask, c/<T>/seq [B, T, D], [B, T] int64 (padded: a prefix of live frames, at least one), [B, 1, D]
  c/<T>/logits32                   _loose_similarity's logits, fp32
  c/<T>/head64, c/<T>/logits64     the head's output (x + visual_output, clip4clip.py:349) and the logits with the reference
                                   run in float64 (.double(); its LayerNorm then computes in float64 too)
  c/<T>/loss64                     symmetric CrossEn of logits64
  c/<T>/g64/<name>                 float64 gradient of that loss for visual_output ('vis'), the position table and every
                                   head parameter, when it has at most 4096 entries
  c/<T>/g64/<name>/{amax,norm,head,sketch}   larger tensors, summarised to keep the file small: largest magnitude, 2-norm,
                                   first 256 entries (flattened) and 16 projections <r_i, g>, r_i = sketch_vectors(name, numel)
  a/<L>/{qkv,mask,out}             block 0's attention (ResidualAttentionBlock.attention, out_proj included) of 2 sequences
                                   of L tokens, sequence 0 fully masked, sequence 1 half; qkv = its in_proj rows [2 * L, 384]
                                   (sequence-major), out [2 * L, 128] - L in {3, 12}

    python tools/gen_golden_seqtransf.py
"""
import json
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
TS = (1, 3, 12, 64, 77)
B = {1: 4, 3: 4, 12: 4, 64: 2, 77: 2}      # clips per case (the fixture stays under 1 MiB)
LAYERS = 2
SKETCH = 16
FULL = 4096


def sketch_vectors(name, numel):
    """[SKETCH, numel] float64 standard normal vectors, seeded by the parameter's name."""
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal((SKETCH, numel))


def init_trick(rc4c, sd, g):
    """Run the reference's from_pretrained on the small model with the checkpoint loader and init_preweight stubbed: ->
    the state dict it would load (the initialisation trick's entries included)."""
    from gen_golden_clip import ref_args
    captured = {}
    E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, Bc, T = (int(v) for v in g["cfg"])
    args = ref_args(T, [T, T, T], [16, 16, 16], cluster_inter=0, sim_header="seqTransf", loose_type=True,
                    cross_num_hidden_layers=LAYERS, pretrained_dir="", temperature_new=0.0, linear_patch='2d',
                    max_words=CTX, time_embedding=None, freeze_clip=0, new_added_modules=[None], camoe_dsl=False,
                    local_rank=0)
    orig_load, orig_init = rc4c.load_clip_state_dict, rc4c.CLIP4Clip.init_preweight
    rc4c.load_clip_state_dict = lambda *a, **k: {k_: v.clone() for k_, v in sd.items()}
    rc4c.CLIP4Clip.init_preweight = classmethod(lambda cls, model, state_dict, task_config=None: captured.update(state_dict) or model)
    try:
        rc4c.CLIP4Clip.from_pretrained("cross-base", state_dict=None, task_config=args)
    finally:
        rc4c.load_clip_state_dict, rc4c.CLIP4Clip.init_preweight = orig_load, orig_init
    return {k: v for k, v in captured.items() if not k.startswith("clip.")}


def head_module(rcross, init, pos, dtype):
    m = types.SimpleNamespace()
    m.frame_position_embeddings = torch.nn.Embedding(pos.shape[0], pos.shape[1])
    m.transformerClip = rcross.Transformer(width=pos.shape[1], layers=LAYERS, heads=pos.shape[1] // 64)
    with torch.no_grad():
        m.frame_position_embeddings.weight.copy_(torch.from_numpy(pos))
        m.transformerClip.load_state_dict({k[len("transformerClip."):]: v for k, v in init.items()
                                           if k.startswith("transformerClip.")})
    m.frame_position_embeddings.to(dtype)
    m.transformerClip.to(dtype)
    return m


def run_case(rc4c, rlosses, m, vis, mask, seq, logit_scale, dtype, grads, mask_dtype=torch.long):
    fake = types.SimpleNamespace(sim_header="seqTransf", training=False, pre_visual_pooling=0,
                                 frame_position_embeddings=m.frame_position_embeddings, transformerClip=m.transformerClip,
                                 clip=types.SimpleNamespace(logit_scale=logit_scale.to(dtype)))
    fake._mean_pooling_for_similarity_visual = types.MethodType(rc4c.CLIP4Clip._mean_pooling_for_similarity_visual, fake)
    captured = {}
    hook = m.transformerClip.register_forward_hook(lambda mod, inp, out: captured.update(x=out))
    v = torch.from_numpy(vis).to(dtype).requires_grad_(grads)
    try:
        logits = rc4c.CLIP4Clip._loose_similarity(fake, torch.from_numpy(seq).to(dtype), v,
                                                  torch.ones(seq.shape[0], 1, dtype=torch.long), torch.from_numpy(mask).to(mask_dtype))
    finally:
        hook.remove()
    head = captured["x"].permute(1, 0, 2) + v
    out = dict(head=head.detach().numpy(), logits=logits.detach().numpy())
    if grads:
        ce = rlosses.CrossEn()
        loss = (ce(logits) + ce(logits.T)) / 2
        params = [("frame_position_embeddings.weight", m.frame_position_embeddings.weight)] + \
                 [("transformerClip." + k, p) for k, p in m.transformerClip.named_parameters()]
        gs = torch.autograd.grad(loss, [v] + [p for _, p in params])
        out["loss"] = np.float64(loss.item())
        out["g"] = [("vis", gs[0].numpy())] + [(k, g_.numpy()) for (k, _), g_ in zip(params, gs[1:])]
    return out


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden_clip import _import_reference
    rclip, rc4c, _, _ = _import_reference()
    import modules.module_cross as rcross
    import modules.losses as rlosses
    g = np.load(os.path.join(GOLD, "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
          if k.startswith("sd/")}
    init = init_trick(rc4c, sd, g)
    out = {"init/names": np.array(json.dumps(sorted(init)))}
    for k, v in init.items():
        f = v.numpy().astype(np.float64).reshape(-1)
        out.update({"init/" + k + "/head": f[:256].copy(), "init/" + k + "/sketch": sketch_vectors(k, f.size) @ f})
    rng = np.random.default_rng(77)
    D = sd["ln_final.weight"].shape[0]
    pos = (0.02 * rng.standard_normal((77, D))).astype(np.float32)
    out["pos"] = pos
    m32, m64 = head_module(rcross, init, pos, torch.float32), head_module(rcross, init, pos, torch.float64)
    logit_scale = sd["logit_scale"].float()
    for T in TS:
        vis = rng.standard_normal((B[T], T, D)).astype(np.float32)
        seq = rng.standard_normal((B[T], 1, D)).astype(np.float32)
        live = rng.integers(1, T + 1, size=B[T])
        live[0] = T                                     # one clip without padding
        mask = (np.arange(T)[None, :] < live[:, None]).astype(np.int64)
        assert (mask.sum(1) >= 1).all(), "every video needs a live frame (the reference's pooled feature is NaN otherwise)"
        r32 = run_case(rc4c, rlosses, m32, vis, mask, seq, logit_scale, torch.float32, False)
        # (the reference's LayerNorm casts its input to fp32, clip.py:186-189: for the float64 run it computes in the input's
        #  dtype instead - nn.LayerNorm.forward itself)
        ln_fwd = rclip.LayerNorm.forward
        rclip.LayerNorm.forward = torch.nn.LayerNorm.forward
        try:
            r64 = run_case(rc4c, rlosses, m64, vis, mask, seq, logit_scale, torch.float64, True, torch.float64)
        finally:
            rclip.LayerNorm.forward = ln_fwd
        c = "c/%d/" % T
        out.update({c + "vis": vis, c + "mask": mask, c + "seq": seq, c + "logits32": r32["logits"],
                    c + "head64": r64["head"], c + "logits64": r64["logits"], c + "loss64": r64["loss"]})
        for name, gr in r64["g"]:
            if gr.size <= FULL:
                out[c + "g64/" + name] = gr
            else:
                f = gr.reshape(-1)
                out.update({c + "g64/" + name + "/amax": np.float64(np.abs(f).max()),
                            c + "g64/" + name + "/norm": np.float64(np.linalg.norm(f)),
                            c + "g64/" + name + "/head": f[:256].copy(),
                            c + "g64/" + name + "/sketch": sketch_vectors(name, f.size) @ f})
        print("T", T, "live", live.tolist(), "loss64", r64["loss"], flush=True)
    # the attention alone, with a fully masked sequence (nn.MultiheadAttention in fp32, as module_cross calls it)
    blk = m32.transformerClip.resblocks[0]
    for Lk in (3, 12):
        x = torch.from_numpy(rng.standard_normal((Lk, 2, D)).astype(np.float32))
        mask = np.ones((2, Lk), dtype=np.int64)
        mask[0] = 0
        mask[1, Lk // 2:] = 0
        ext = ((1.0 - torch.from_numpy(mask).float().unsqueeze(1)) * -1000000.0).expand(-1, Lk, -1)
        with torch.no_grad():
            o = blk.attention(x, ext)                                         # [Lk, 2, D]
            qkv = torch.nn.functional.linear(x, blk.attn.in_proj_weight, blk.attn.in_proj_bias)
        a = "a/%d/" % Lk
        out[a + "qkv"] = qkv.permute(1, 0, 2).reshape(2 * Lk, 3 * D).numpy()
        out[a + "mask"] = mask
        out[a + "out"] = o.permute(1, 0, 2).reshape(2 * Lk, D).numpy()
    path = os.path.join(GOLD, "seqtransf_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
