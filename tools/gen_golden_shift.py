"""Fixture tests/golden/shift_golden.npz for tests/test_shift_host.py / tests/test_shift_gpu.py, captured from the reference
(dev container only: it imports the reference's modules/cluster/shift.py and modules/clip.py).

  k/<case>/cfg                     [4]        nt, L, W, segment of a kernel case (NLD input [nt, L, W])
  k/<case>/x                       [nt, L, W] seeded input
  k/<case>/temporal, k/<case>/token          temporal_shift_wo_cls / token_shift (fold_div 8) of x
  plans                            json       {plan: [target_frames_blocks, cluster_num_blocks]} at max_frames = T
  e/<algo>/<plan>/v_feat           [B*T, E]   CLIP.encode_image of the small model of clip_golden.npz (video_frame = T)
  e/<algo>/<plan>/logits           [B, B]     meanP loose similarity logits (CLIP4Clip._loose_similarity, eval) of its
                                              features against encode_text of the first B captions
  t/<algo>/loss, t/<algo>/vfeat, t/<algo>/tfeat    one training step (gen_train_grads of oracle/gen_golden_r4.py: meanP,
                                              symmetric CrossEn) with every block shifting (plan 'all')
  t/<algo>/g/<param>/{norm,amax,head,sketch}     torch.autograd's gradient of every parameter, summarised to stay small:
                                              its 2-norm, largest magnitude, first 256 entries (flattened) and 16 random
                                              projections <r_i, g> with r_i = sketch_vectors(param, numel) below

    python tools/gen_golden_shift.py
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

KERNEL_CASES = {                      # nt, L, W, segment
    "w128": (8, 5, 128, 4),           # two segments
    "w100": (12, 3, 100, 3),          # W % 8 != 0 (fold 12), four segments
    "w7": (6, 4, 7, 6),               # W < 8: fold 0, a copy
    "w36": (10, 7, 36, 5),            # fold 4, two segments
    "seg1": (4, 3, 64, 1),            # one frame per segment: every shifted channel is zero
}
PLANS = {"all": ([2, 2, 2], [16, 15, 14]),    # every block fires (frames or tokens decrease)
         "last": ([4, 4, 4], [16, 16, 15])}   # only block 3 fires
ALGOS = ("token_shift", "temporal_shift")
SKETCH = 16


def sketch_vectors(name, numel):
    """[SKETCH, numel] float64 standard normal vectors, seeded by the parameter's name."""
    return np.random.default_rng(zlib.crc32(name.encode())).standard_normal((SKETCH, numel))


def summarise(name, g):
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return dict(norm=np.float64(np.linalg.norm(g)), amax=np.float64(np.abs(g).max()), head=g[:256].astype(np.float32),
                sketch=sketch_vectors(name, g.size) @ g)


def small_model(rclip, algo, plan, train=False):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden_clip import ref_args
    g = np.load(os.path.join(GOLD, "clip_golden.npz"))
    E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T = (int(v) for v in g["cfg"])
    frames, tokens = PLANS[plan]
    model = rclip.CLIP(E, RES, VL, VW, P, CTX, VOCAB, TW, TH, TL, linear_patch='2d', video_frames=T,
                       args=ref_args(T, frames, tokens, cluster_algo=algo)).float()
    model.load_state_dict({k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k])
                           for k in g.files if k.startswith("sd/")})
    return (model.train() if train else model.eval()), g


def loose_logits(rc4c, model, seq, vis, CTX):
    fake = types.SimpleNamespace(sim_header="meanP", training=False, pre_visual_pooling=0,
                                 clip=types.SimpleNamespace(logit_scale=model.logit_scale))
    fake._mean_pooling_for_similarity_visual = types.MethodType(rc4c.CLIP4Clip._mean_pooling_for_similarity_visual, fake)
    B = seq.shape[0]
    vmask = torch.ones(B, vis.shape[1], dtype=torch.long)
    return rc4c.CLIP4Clip._loose_similarity(fake, seq, vis, torch.ones(B, CTX, dtype=torch.long), vmask)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from gen_golden_clip import _import_reference
    rclip, rc4c, _, _ = _import_reference()
    import modules.cluster.shift as rshift
    import modules.losses as rlosses
    out = {"plans": np.array(json.dumps(PLANS))}
    rng = np.random.default_rng(2024)
    for case, (nt, L, W, seg) in KERNEL_CASES.items():
        x = rng.standard_normal((nt, L, W)).astype(np.float32)
        xt = torch.from_numpy(x)
        out[f"k/{case}/cfg"] = np.array([nt, L, W, seg], dtype=np.int64)
        out[f"k/{case}/x"] = x
        out[f"k/{case}/temporal"] = rshift.temporal_shift_wo_cls(xt.clone(), seg, fold_div=8).numpy()
        out[f"k/{case}/token"] = rshift.token_shift(xt.clone(), seg, fold_div=8).numpy()
    for algo in ALGOS:
        for plan in PLANS:
            model, g = small_model(rclip, algo, plan)
            E, CTX, B, T = int(g["cfg"][0]), int(g["cfg"][5]), int(g["cfg"][10]), int(g["cfg"][11])
            video, ids = torch.from_numpy(g["video"]), torch.from_numpy(g["t_ids"])[:B]
            with torch.no_grad():
                vfeat, _ = model.encode_image(video, video_frame=T)
                tfeat = model.encode_text(ids)
                logits = loose_logits(rc4c, model, tfeat.view(B, 1, E), vfeat.view(B, -1, E), CTX)
            out[f"e/{algo}/{plan}/v_feat"] = vfeat.numpy()
            out[f"e/{algo}/{plan}/logits"] = logits.numpy()
            print(algo, plan, tuple(vfeat.shape), flush=True)
        # one training step, every block shifting
        model, g = small_model(rclip, algo, "all", train=True)
        video, ids = torch.from_numpy(g["video"]), torch.from_numpy(g["t_ids"])[:B]
        vfeat, _ = model.encode_image(video, video_frame=T)
        tfeat = model.encode_text(ids)
        sim = loose_logits(rc4c, model, tfeat.view(B, 1, E), vfeat.view(B, -1, E), CTX)
        ce = rlosses.CrossEn()
        loss = (ce(sim) + ce(sim.T)) / 2
        loss.backward()
        out[f"t/{algo}/loss"] = np.float32(loss.item())
        out[f"t/{algo}/vfeat"], out[f"t/{algo}/tfeat"] = vfeat.detach().numpy(), tfeat.detach().numpy()
        n = 0
        for k, p_ in model.named_parameters():
            if p_.grad is not None:
                for field, v in summarise(k, p_.grad.numpy()).items():
                    out[f"t/{algo}/g/{k}/{field}"] = v
                n += 1
        print(algo, "train grads:", n, "tensors, loss", float(loss), flush=True)
    path = os.path.join(GOLD, "shift_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
