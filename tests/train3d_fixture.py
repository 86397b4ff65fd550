"""Loader of tests/golden/train3d_sd_golden.npz / train3d_golden.npz / train3d_t1_golden.npz (tools/gen_golden_3d.py) for the linear_patch='3d'
training tests: the reference's small '3d' CLIP, one training step in float64."""
import json
import os
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {3: "train3d_golden.npz", 1: "train3d_t1_golden.npz"}


def load(T):
    return np.load(os.path.join(HERE, "golden", FILES[T]))


def state_dict():
    g = np.load(os.path.join(HERE, "golden", "train3d_sd_golden.npz"))
    return {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
            if k.startswith("sd/")}


def cfg(T, layers, **kw):
    """The task config of the fixture model: no cluster module, T frames per clip."""
    a = Namespace(cluster_inter=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T] * layers,
                  cluster_num_blocks=[16] * layers, cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                  minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                  sim_header='meanP', linear_patch='3d')
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def model(T, **kw):
    from centerclip_amd.clip4clip import CLIP4Clip
    g = load(3)
    return CLIP4Clip.from_state_dict(state_dict(), cfg(T, int(g["cfg"][4]), **kw)).float()


def no_grad_names(g):
    return set(json.loads(str(g["no_grad"])))


def gradients(g):
    """name -> the reference's float64 gradient (tensors above 4096 entries: rounded to float32 in the file)."""
    out = {}
    for k in g.files:
        if k.startswith("g64/"):
            name = k[4:-4] if k.endswith("/f32") else k[4:]
            out[name] = torch.from_numpy(g[k].astype(np.float64))
    return out


def batch(g):
    """(input_ids, input_mask, segment_ids, video, video_mask) as the dataloaders yield it."""
    E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T = (int(v) for v in g["cfg"])
    ids = torch.from_numpy(g["ids"])
    video = torch.from_numpy(g["video"].astype(np.float32)).view(B, 1, T, 3, RES, RES)
    return ids, (ids > 0).long(), torch.zeros_like(ids), video, torch.ones(B, 1, T, dtype=torch.long)
