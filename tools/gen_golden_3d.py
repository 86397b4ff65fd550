"""Fixtures tests/golden/train3d_sd_golden.npz, train3d_golden.npz and train3d_t1_golden.npz for tests/test_train3d_host.py / test_train3d_gpu.py,
captured from the reference (dev container only: it imports the reference's modules/clip.py, clip4clip.py and losses.py with
the stub modules of oracle/gen_golden_clip.py).

The model is the reference's CLIP with linear_patch='3d' at the smallest shape with more than one patch per side: resolution
32, patch 8 (4 x 4 patches, conv2.weight [64, 3, 3, 8, 8] = 576 columns), width 64 (one head), 2 visual blocks and 1 text
block, no cluster module.  Weights are random (conv2 with nn.Conv3d's own initialisation: all three taps live), LayerNorm and
bias terms perturbed, every tensor rounded to a coarse power-of-two grid (fp16-representable, and the file compresses).  One
training step - encode_image, encode_text, the meanP similarity, the symmetric CrossEn of clip4clip.py:245-262, evaluated as
oracle/gen_golden_r4.py does - runs in float64 (the reference's LayerNorm computes in fp32 whatever comes in, clip.py:186-189:
for this run it computes in the input's dtype), and torch.autograd gives the gradient of every parameter.

  train3d_sd_golden.npz    cfg [E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T], sd/<name> the state dict (fp16: exact)
  train3d_golden.npz       cfg, video [B * T, 3, RES, RES] (fp16 values), ids [B, CTX]: two clips of T = 3 frames
  train3d_t1_golden.npz    the same model, two clips of T = 1 frame: both temporal neighbours of every frame are padding
  both cases: loss, vfeat, tfeat float64; no_grad json: the parameters that received no gradient (visual.conv1.weight);
        g64/<name>         the float64 gradient of a parameter with at most 4096 entries
        g64/<name>/f32     a larger one: the float64 gradient rounded to float32 (6e-8 of an entry; the full float64 gradients
                           of the 213,000 parameters would be 1.7 MB per case, above the size a committed file may have)

    python tools/gen_golden_3d.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

E, RES, P, VW, VL = 64, 32, 8, 64, 2
CTX, VOCAB, TW, TH, TL = 8, 64, 64, 1, 1
B = 2
FULL = 4096


def coarse(p_):
    """Round to multiples of 2^floor(log2(std)) / 8: about fifty levels over +-3 sigma, exact in fp16."""
    std = float(p_.std()) if p_.numel() > 1 else max(abs(float(p_)), 1e-3)
    step = 2.0 ** (np.floor(np.log2(max(std, 1e-4))) - 3)
    return torch.round(p_ / step) * step


def run_case(rclip, rc4c, rlosses, model, video, ids, T):
    for p_ in model.parameters():
        p_.grad = None
    vfeat, _ = model.encode_image(video.double(), video_frame=T)
    tfeat = model.encode_text(ids)
    fake = types.SimpleNamespace(sim_header="meanP", training=False, pre_visual_pooling=0,
                                 clip=types.SimpleNamespace(logit_scale=model.logit_scale))
    fake._mean_pooling_for_similarity_visual = types.MethodType(rc4c.CLIP4Clip._mean_pooling_for_similarity_visual, fake)
    vis, seq = vfeat.view(B, -1, E), tfeat.view(B, 1, E)
    vmask = torch.ones(B, vis.shape[1], dtype=torch.long)
    sim = rc4c.CLIP4Clip._loose_similarity(fake, seq, vis, torch.ones(B, CTX, dtype=torch.long), vmask)
    ce = rlosses.CrossEn()
    loss = (ce(sim) + ce(sim.T)) / 2
    loss.backward()
    assert loss.dtype == torch.float64 and vfeat.dtype == torch.float64
    out = {"loss": np.float64(loss.item()), "vfeat": vfeat.detach().numpy(), "tfeat": tfeat.detach().numpy()}
    none = []
    for k, p_ in model.named_parameters():
        if p_.grad is None:
            none.append(k)
        elif p_.numel() <= FULL:
            out["g64/" + k] = p_.grad.numpy().copy()
        else:
            out["g64/" + k + "/f32"] = p_.grad.numpy().astype(np.float32)
    out["no_grad"] = np.array(json.dumps(sorted(none)))
    print("T", T, "loss", float(loss), "no gradient:", none, flush=True)
    return out


def main():
    from gen_golden_clip import _import_reference, ref_args
    rclip, rc4c, _, _ = _import_reference()
    import modules.losses as rlosses
    torch.manual_seed(3003)
    T = 3
    args = ref_args(T, [T] * VL, [16] * VL, cluster_inter=0)
    model = rclip.CLIP(E, RES, VL, VW, P, CTX, VOCAB, TW, TH, TL, linear_patch='3d', video_frames=T, args=args).float().train()
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("bias") or "ln_" in n_:
                p_.add_(0.05 * torch.randn_like(p_))
            p_.copy_(coarse(p_))
            assert torch.equal(p_.half().float(), p_), n_
    out = {"cfg": np.array([E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T], dtype=np.int64)}
    for k, v in model.state_dict().items():
        out["sd/" + k] = v.numpy().astype(np.float16) if v.is_floating_point() else v.numpy()
    ids = torch.zeros(B, CTX, dtype=torch.long)
    for b, ln in enumerate((5, 8)):
        ids[b, 0] = VOCAB - 2
        ids[b, 1:ln - 1] = torch.randint(1, VOCAB - 2, (ln - 2,))
        ids[b, ln - 1] = VOCAB - 1                         # EOT = largest id
    path = os.path.join(GOLD, "train3d_sd_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    ln_fwd = rclip.LayerNorm.forward
    rclip.LayerNorm.forward = torch.nn.LayerNorm.forward
    try:
        model = model.double()
        for T_, name in ((3, "train3d_golden.npz"), (1, "train3d_t1_golden.npz")):
            video = torch.randn(B * T_, 3, RES, RES).half()
            res = run_case(rclip, rc4c, rlosses, model, video.float(), ids, T_)
            res.update({"video": video.numpy(), "ids": ids.numpy()})
            res["cfg"] = np.array([E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T_], dtype=np.int64)
            path = os.path.join(GOLD, name)
            np.savez_compressed(path, **res)
            print("wrote", path, os.path.getsize(path), "bytes")
    finally:
        rclip.LayerNorm.forward = ln_fwd


if __name__ == "__main__":
    main()
