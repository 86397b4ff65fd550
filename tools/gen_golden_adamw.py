"""Fixture tests/golden/adamw_golden.npz for tests/test_adamw_host.py, captured from the reference (dev container only: it
imports the reference's utils/lr_scheduler.py and utils/optimization.py).

  sched/<case>/lr, sched/<case>/wd   [steps, 4]  lr and weight_decay of four parameter groups (lr_mult / decay_mult of the
                                                 reference's AdamW groups at coef_lr = 0.1) after scheduler(opt, global_step=T),
                                                 T = 0 .. steps - 1 (epoch = T // 10 for mode 'step')
  sched/<case>/cfg                   json        the lr_scheduler arguments
  sched_group_mults                  [4, 2]      (lr_mult, decay_mult) of the four groups
  groups_args                        json        lr, wd, new_added_modules, coef_lr of the grouping below
  groups                             json        prep_optim_params_groups(Namespace(optim='AdamW', ...)) of the reference on
                                                 the small CLIP4Clip of clip_golden.npz: per group the parameter names and
                                                 every key except 'params'

    python tools/gen_golden_adamw.py
"""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

GROUP_MULTS = [(0.1, 1), (0.1, 0.0), (1.0, 1.0), (1.0, 0.0)]
ALL_ITERS, STEPS = 57, 58
SCHED_CASES = {
    "cos": dict(mode='cos', init_lr=1e-3, all_iters=ALL_ITERS, slow_start_iters=0.1 * ALL_ITERS, end_lr=1e-5, weight_decay=0.2),
    "cos_nowarm": dict(mode='cos', init_lr=2e-4, all_iters=ALL_ITERS, weight_decay=0.05),
    "poly": dict(mode='poly', init_lr=1e-3, all_iters=ALL_ITERS, slow_start_iters=6, slow_start_lr=1e-6, end_lr=1e-5,
                 weight_decay=0.2),
    "HTD": dict(mode='HTD', init_lr=1e-3, all_iters=ALL_ITERS, slow_start_iters=0.1 * ALL_ITERS, end_lr=1e-5, weight_decay=0.1),
    "step": dict(mode='step', init_lr=1e-3, all_iters=ALL_ITERS, lr_step=2, lr_step_multiplier=0.5, end_lr=1e-5, weight_decay=0.2),
    "step_milestones": dict(mode='step', init_lr=1e-3, all_iters=ALL_ITERS, lr_milestones=[1, 3, 4], slow_start_iters=4,
                            weight_decay=0.2),
}
NEW_ADDED = ["ln_final", "text_projection", "visual.proj"]


def small_clip4clip():
    """The small CLIP4Clip of tests/golden/clip_golden.npz (its parameter names are what the grouping sees)."""
    from centerclip_amd.clip4clip import CLIP4Clip
    g = np.load(os.path.join(GOLD, "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
          if k.startswith("sd/")}
    T = int(g["cfg"][11])
    cfg = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                    cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                    minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                    sim_header='meanP', linear_patch='2d')
    return CLIP4Clip.from_state_dict(sd, cfg)


def group_args():
    return Namespace(optim='AdamW', lr=1e-4, wd=0.2, new_added_modules=NEW_ADDED)


def main():
    from oracle.gen_golden_clip import _import_reference, REF
    _import_reference()                                   # (stubs the reference's download / tokenizer dependencies)
    saved = list(sys.path)
    sys.path[:] = [REF] + sys.path
    try:
        from utils.lr_scheduler import lr_scheduler as ref_sched
        from utils.optimization import prep_optim_params_groups as ref_groups
    finally:
        sys.path[:] = saved
    out = {}

    class _Opt:
        def __init__(self):
            self.param_groups = [{'lr': 0.0, 'weight_decay': 0.0, 'lr_mult': lm, 'decay_mult': dm} for lm, dm in GROUP_MULTS]

    for name, kw in SCHED_CASES.items():
        s, opt = ref_sched(**kw), _Opt()
        lr, wd = np.zeros((STEPS, 4)), np.zeros((STEPS, 4))
        for T in range(STEPS):
            s(opt, epoch=T // 10, global_step=T)
            lr[T] = [g['lr'] for g in opt.param_groups]
            wd[T] = [g['weight_decay'] for g in opt.param_groups]
        out["sched/%s/lr" % name], out["sched/%s/wd" % name] = lr, wd
        out["sched/%s/cfg" % name] = np.array(json.dumps(kw))

    out["sched_group_mults"] = np.array(GROUP_MULTS, dtype=np.float64)
    out["groups_args"] = np.array(json.dumps(dict(vars(group_args()), coef_lr=0.1)))
    model = small_clip4clip()
    names = {id(p): n for n, p in model.named_parameters()}
    groups = ref_groups(group_args(), model, coef_lr=0.1)
    out["groups"] = np.array(json.dumps([dict({k: v for k, v in g.items() if k != 'params'},
                                              names=[names[id(p)] for p in g['params']]) for g in groups]))
    path = os.path.join(GOLD, "adamw_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, sorted(out))


if __name__ == "__main__":
    main()
