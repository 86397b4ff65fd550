"""A gallery split in shards on one device: ``ShardedGallery(shards=[...])`` over S ``FeatureGallery`` objects against the
concatenated gallery - one ``FeatureGallery`` holding the same rows in shard order.  ``search``, a cursor page and ``rank`` are
checked for equality (scores by their bits, ids after mapping (shard, position) -> concatenated position); then the merge op
``torch.ops.centerclip.similarity_topk_merge`` is timed next to ``torch.cat`` + two stable ``torch.sort`` passes over the same
lists at (S, k, Bq) = (8, 128, 64) and (8, 4096, 64).  The process-group form (``ShardedGallery(local=g, distributed=True)``,
one shard per rank) runs the same merge path; it was never run on multi-GPU hardware.

    python examples/search_sharded.py [--shards 8] [--rows 20000] [--queries 16] [--k 200]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from centerclip_amd.clip4clip import CLIP4Clip              # noqa: E402
from centerclip_amd.search import FeatureGallery            # noqa: E402
from centerclip_amd.search_sharded import ShardedGallery    # noqa: E402
import bench                                                # noqa: E402  (cfg-2 task config, random ViT-B/32 state dict)
from search_synthetic import timed                          # noqa: E402


def check_part(model, device, S, rows, queries, k):
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    pool = torch.randn(max(rows // 4, 1), E, device=device, generator=g)                 # every row four times: ties cross shards
    feats = pool[torch.randint(0, pool.shape[0], (rows,), device=device, generator=g)]
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    cuts = np.sort(np.random.default_rng(1).integers(0, rows + 1, size=S - 1))
    base = np.concatenate(([0], cuts, [rows]))                                          # uneven shards, some possibly empty
    shards, cat = [FeatureGallery(model) for _ in range(S)], FeatureGallery(model)
    sharded = ShardedGallery(shards=shards)
    for i in range(S):
        if base[i + 1] > base[i]:
            sharded.add_features(feats[base[i]:base[i + 1]], shard=i)
    cat.add_features(feats)
    print("%d rows in %d shards of %s rows" % (rows, S, [int(n) for n in np.diff(base)]))
    first = torch.from_numpy(base[:-1]).to(device)

    def flat(ids):
        shard, pos = ShardedGallery.split(ids)
        return torch.where(ids < 0, -1, first[shard.clamp(min=0)] + pos)

    def same(got, want):
        return bool(torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(flat(got[1]), want[1]))

    got, want = sharded.search_features(seq, k=k), cat.search_features(seq, k=k)
    print("search(k=%d) equals the concatenated gallery's, bit for bit: %s" % (k, same(got, want)))
    page = sharded.search_features(seq, k=k, after=(got[0][:, -1].contiguous(), got[1][:, -1].contiguous()))
    both = cat.search_features(seq, k=2 * k)
    print("the cursor page is columns [%d, %d) of search(k=%d): %s" % (k, 2 * k, 2 * k, same(page, [t[:, k:].contiguous() for t in both])))
    target = torch.randint(0, rows, (queries,), generator=torch.Generator().manual_seed(2))
    shard = np.searchsorted(base[1:], target.numpy(), side="right")
    ids = [(int(s) << 32) | int(p - base[s]) for s, p in zip(shard, target.tolist())]
    r, c = sharded.rank_features(seq, ids), cat.rank_features(seq, target)
    ok = torch.equal(r[0], c[0]) and torch.equal(r[1].view(torch.int32), c[1].view(torch.int32)) and torch.equal(r[2], c[2])
    print("rank equals the concatenated gallery's (ranks %s ...): %s" % (r[0][:4].tolist(), bool(ok)))
    return same(got, want) and bool(ok)


def time_merge(device, S, k, Bq, reps, warmup):
    """valid lists (descending, ties by smaller id, a fill tail) -> the merge op next to cat + two stable sorts"""
    g = torch.Generator(device=device).manual_seed(k)
    scores = torch.randint(0, 4 * k, (S, Bq, k), device=device, generator=g).float().sort(dim=2, descending=True).values
    ids = torch.arange(k, device=device, dtype=torch.int32).expand(S, Bq, k).contiguous()  # ascending: ties by smaller id
    ids[:, :, k - k // 8:] = -1                                                             # the last eighth of every list is fill
    shard = torch.arange(S, device=device)[:, None, None].expand(S, Bq, k)

    def merge():
        return torch.ops.centerclip.similarity_topk_merge(scores, ids)

    def cat_sort():
        s = torch.where(ids < 0, float("-inf"), scores + 0.0).permute(1, 0, 2).reshape(Bq, S * k)
        gid = torch.where(ids < 0, torch.iinfo(torch.int64).max, (shard << 32) | ids.long()).permute(1, 0, 2).reshape(Bq, S * k)
        gid, order = torch.sort(gid, dim=1, stable=True)                                 # by (shard, id) ...
        s, order = torch.sort(s.gather(1, order), dim=1, descending=True, stable=True)   # ... then, stably, by score
        return s[:, :k], gid.gather(1, order)[:, :k]
    a, b = merge(), cat_sort()
    valid = a[1] >= 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][valid], b[1][valid]), "the two paths disagree"
    t = timed([("similarity_topk_merge", merge), ("torch.cat + two stable sorts", cat_sort)], warmup, reps)
    med = {name: statistics.median(v) for name, v in t.items()}
    print("merge at (S, k, Bq) = (%d, %d, %d): similarity_topk_merge %.3f ms, cat + two stable sorts %.3f ms, ratio %.2f"
          % (S, k, Bq, med["similarity_topk_merge"], med["torch.cat + two stable sorts"],
             med["torch.cat + two stable sorts"] / med["similarity_topk_merge"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    c = bench.CFG2
    model = CLIP4Clip.from_state_dict(bench.random_state_dict(c, seed=0), bench.task_config(c)).to(device).eval()
    ok = check_part(model, device, a.shards, a.rows, a.queries, a.k)
    print("agreement: %s" % ok)
    for S, k, Bq in ((8, 128, 64), (8, 4096, 64)):
        time_merge(device, S, k, Bq, a.reps, a.warmup)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
