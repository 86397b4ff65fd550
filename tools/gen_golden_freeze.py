"""tests/golden/freeze_golden.json: the parameters the REFERENCE freezes (dev container only: imports the read-only reference).

One entry per (freeze_layer_num, linear_patch, sim_header), key "<k>|<patch>|<head>": the sorted names of the parameters with
requires_grad == False after the reference's own CLIP4Clip.freeze_cip_layers(k) (modules/clip4clip.py:449-471) on the small
model of clip_golden.npz.  The function reads ``self.clip`` and ``self.linear_patch`` only, so it is called unbound on a
holder module that carries the reference's CLIP under ``clip`` and - for seqTransf - a frame_position_embeddings table and a
transformerClip stack under the reference's names (the head is outside ``clip.``: the entries show that it never freezes).
Names and nothing else are stored.

    python tools/gen_golden_freeze.py   ->  tests/golden/freeze_golden.json
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LAYER_NUMS = (-1, 0, 1, 2, 3, 6, 11, 12)      # the issue's six values, plus 2 and 3 for the GPU test on the 3-block fixture model


def main():
    from gen_golden_clip import _import_reference, ref_args
    rclip, rc4c, _, _ = _import_reference()
    g = np.load(os.path.join(GOLD, "clip_golden.npz"))
    E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T = (int(v) for v in g["cfg"])
    out = {}
    for patch in ("2d", "3d"):
        for head in ("meanP", "seqTransf"):
            for k in LAYER_NUMS:
                holder = torch.nn.Module()
                holder.clip = rclip.CLIP(E, RES, VL, VW, P, CTX, VOCAB, TW, TH, TL, linear_patch=patch, video_frames=T,
                                         args=ref_args(T, [4, 2, 2], [16, 6, 6])).float()
                holder.linear_patch = patch
                if head == "seqTransf":
                    holder.frame_position_embeddings = torch.nn.Embedding(CTX, TW)
                    holder.transformerClip = rclip.Transformer(TW, 1, TH)
                rc4c.CLIP4Clip.freeze_cip_layers(holder, k)
                out["%d|%s|%s" % (k, patch, head)] = sorted(n for n, p_ in holder.named_parameters() if not p_.requires_grad)
                print(k, patch, head, len(out["%d|%s|%s" % (k, patch, head)]), flush=True)
    for bad in (13, -2):
        try:
            rc4c.CLIP4Clip.freeze_cip_layers(holder, bad)
            raise SystemExit("the reference accepted freeze_layer_num=%d" % bad)
        except AssertionError:
            pass
    with open(os.path.join(GOLD, "freeze_golden.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
