"""Worker of tests/test_dsl_gpu.py::test_two_ranks_on_one_gpu_sharded_dsl_equals_single_process - run by torch.distributed.run
with two processes that share cuda:0, collectives over gloo.  Every rank: eval_epoch(shard=True, camoe_dsl=True) on the ev_*
loaders (batches dealt round robin; single- and multi-sentence protocols), and on ONE batch holding the whole dataset, so that
rank 1 receives no row; rank 0 alone: the single-process call.  Same R@1 and metric strings, and they are not the flag-off
ones.  Prints DSL_WORKER_OK world=2 on rank 0."""
import os
import sys
from argparse import Namespace

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Loader(list):
    pass


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.eval import eval_epoch
    from oracle.recipes import EVAL_CASES, eval_case_batches
    g2 = np.load(os.path.join(ROOT, "tests", "golden", "r2_golden.npz"))
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    cfg = g2["s1_cfg"]
    T = int(cfg[11])
    a = Namespace(cluster_inter=0, deep_cluster=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T, T, T],
                  cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                  minkowski_norm_p=2.0, aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True,
                  sim_header='meanP', linear_patch='2d', pre_visual_pooling=0, camoe_dsl=1)
    model = CLIP4Clip.from_state_dict(sd, a).to(dev).eval()
    assert model.camoe_dsl
    for name in sorted(EVAL_CASES):
        for whole in (False, True):
            case = dict(EVAL_CASES[name], batch=64) if whole else EVAL_CASES[name]
            batches, attrs = eval_case_batches(case, cfg)
            assert not whole or len(batches) == 1
            loader = _Loader(batches)
            loader.dataset = Namespace(**attrs)
            got = eval_epoch(model, loader, dev, shard=True)                       # (the flag from the model)
            box = [(eval_epoch(model, loader, dev), eval_epoch(model, loader, dev, camoe_dsl=False)) if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            want, plain = box[0]
            assert abs(got[0] - want[0]) < 1e-9 and list(got[2]) == list(want[2]), (name, whole, got, want)
            assert list(plain[2]) != list(want[2]), (name, whole)
    torch.cuda.synchronize()
    dist.barrier()
    if rank == 0:
        print("DSL_WORKER_OK world=%d" % world, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
