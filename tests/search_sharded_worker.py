"""Worker of tests/test_search_sharded_gpu.py::test_two_ranks_on_one_gpu_equal_the_concatenated_gallery - run by
torch.distributed.run with two processes that share cuda:0, collectives over gloo.  Every rank holds one shard of a grouped
gallery (an uneven share of the same rows; in the second case rank 1 holds nothing) behind ShardedGallery(local=...,
distributed=True) and runs search, a cursor page, search_groups, rank, rank_groups and validate(); rank 0 also builds the
concatenated FeatureGallery and broadcasts its results as objects; every rank asserts its own results equal them (scores by
their bits).  Prints SHARDED_WORKER_OK world=2 on rank 0."""
import os
import sys
from argparse import Namespace

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_Q, K = 5, 12


def _cpu(result):
    return tuple(t.cpu() for t in result)


def _same(got, want, what):
    for a, b in zip(_cpu(got), want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.search import FeatureGallery
    from centerclip_amd.search_sharded import ShardedGallery
    g2 = np.load(os.path.join(ROOT, "tests", "golden", "r2_golden.npz"))
    sd = {k[6:]: torch.from_numpy(g2[k].astype(np.float32) if g2[k].dtype == np.float16 else g2[k])
          for k in g2.files if k.startswith("s1_sd/")}
    cfg = g2["s1_cfg"]
    E, T = int(cfg[0]), int(cfg[11])
    a = Namespace(cluster_inter=0, deep_cluster=0, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[T, T, T],
                  cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                  minkowski_norm_p=2.0, aggregation=None, pretrained_clip_name='ViT-B/32', pre_norm=False, loose_type=True,
                  sim_header='meanP', linear_patch='2d', pre_visual_pooling=0)
    model = CLIP4Clip.from_state_dict(sd, a).to(dev).eval()
    gen = torch.Generator().manual_seed(2)                                     # the same rows and queries on both ranks
    pool, seq = torch.randn(8, E, generator=gen).to(dev), torch.randn(N_Q, 1, E, generator=gen).to(dev)
    for case, shares in enumerate(((37, 13), (50, 0))):
        rng = np.random.default_rng(case)
        total = sum(shares)
        rows = pool[torch.from_numpy(rng.integers(0, 8, size=total)).to(dev)]  # duplicates fall on both shards
        labels = np.concatenate([1000 * (r + 1) + np.cumsum(rng.random(n) < 0.45) for r, n in enumerate(shares)]).astype(np.int64)
        base = np.concatenate(([0], np.cumsum(shares)))
        local = FeatureGallery(model, grouped=True)
        sg = ShardedGallery(local=local, distributed=True)
        assert (sg.S, sg.first) == (world, rank)
        if shares[rank]:
            ids = sg.add_features(rows[base[rank]:base[rank + 1]], group=labels[base[rank]:base[rank + 1]].tolist())
            assert ids.tolist() == [(rank << 32) | p for p in range(shares[rank])]
        assert len(sg) == shares[rank] and sg.global_len() == total
        sg.validate()
        gone = rng.choice(total, size=6, replace=False)                        # some rows leave, on whichever rank holds them
        shard_of = np.searchsorted(base[1:], gone, side="right")
        sg.remove([(int(s) << 32) | int(p - base[s]) for s, p in zip(shard_of, gone)])
        target = rng.integers(0, total, size=N_Q)
        target[0] = gone[0]                                                    # a removed target keeps its score
        t_shard = np.searchsorted(base[1:], target, side="right")
        t_ids = [(int(s) << 32) | int(p - base[s]) for s, p in zip(t_shard, target)]
        t_labels = labels[target].tolist()
        got = {"search": sg.search_features(seq, k=K)}
        got["page"] = sg.search_features(seq, k=K, after=(got["search"][0][:, -1].contiguous(), got["search"][1][:, -1].contiguous()))
        got["deep"] = sg.search_features(seq, k=150)
        got["groups"] = sg.search_groups_features(seq, k=K)
        got["rank"] = sg.rank_features(seq, t_ids)
        got["rank_groups"] = sg.rank_groups_features(seq, t_labels)
        got["outside"] = sg.rank_features(seq, [(5 << 32) | 1] * N_Q)
        box = [None]
        if rank == 0:
            cat = FeatureGallery(model, grouped=True)
            cat.add_features(rows, group=labels.tolist())
            cat.remove(gone)
            want = {"search": cat.search_features(seq, k=K)}
            want["page"] = cat.search_features(seq, k=K, after=(want["search"][0][:, -1].contiguous(), want["search"][1][:, -1].contiguous()))
            want["deep"] = cat.search_features(seq, k=150)
            want["groups"] = cat.search_groups_features(seq, k=K)
            want["rank"] = cat.rank_features(seq, target.tolist())
            want["rank_groups"] = cat.rank_groups_features(seq, t_labels)
            box = [{name: _cpu(res) for name, res in want.items()}]
        dist.broadcast_object_list(box, src=0)
        want = box[0]
        flat = torch.from_numpy(base[:-1])
        for name in ("search", "page", "deep", "groups"):
            res = _cpu(got[name])
            shard, pos = ShardedGallery.split(res[-1])
            res = res[:-1] + (torch.where(res[-1] < 0, -1, flat[shard.clamp(min=0)] + pos),)
            _same(res, want[name], (case, name))
        _same(got["rank"], want["rank"], (case, "rank"))
        _same(got["rank_groups"], want["rank_groups"], (case, "rank_groups"))
        assert bool(torch.isfinite(got["rank"][1]).all()) and int(got["outside"][2].sum()) == 0
        assert bool(torch.isneginf(got["outside"][1]).all())
        if case == 0:                                                          # a group on two shards: every rank raises alike
            if rank == 1:
                local.add_features(rows[:1], group=[int(labels[0])])
            try:
                sg.validate()
            except ValueError as e:
                assert "shards 0 and 1" in str(e), e
            else:
                raise AssertionError("validate() accepted a group on two shards")
    torch.cuda.synchronize()
    dist.barrier()
    if rank == 0:
        print("SHARDED_WORKER_OK world=%d" % world, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
