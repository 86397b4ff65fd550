"""Retrieval with a cached gallery on synthetic data: encode clips once, keep their similarity operands on the device, ask for
the k best clips of a caption.

    gallery = FeatureGallery(model); gallery.add(video, video_mask) ...; scores, ids = gallery.search(input_ids, k=10)

Random-init CLIP weights (no checkpoint / dataset access here), clips added in uneven batches.  The second part times the
search against the matrix path (the [Nq, N] matrix of eval_epoch + torch.topk) on a large gallery of random unit rows:
device events around every call, the two paths alternating, after a warm-up.

    python examples/search_synthetic.py [--clips 40] [--k 5] [--time-rows 200000] [--time-queries 16] [--time-k 10] [--reps 50]
    python examples/search_synthetic.py --clips 0 --time-rows 200000     (the timing alone)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from centerclip_amd import _lib as L                        # noqa: E402
from centerclip_amd import torch_ops as T                   # noqa: E402
from centerclip_amd.clip4clip import CLIP4Clip              # noqa: E402
from centerclip_amd.search import FeatureGallery            # noqa: E402
import bench                                                # noqa: E402  (cfg-2 task config, random ViT-B/32 state dict)
from eval_synthetic import SyntheticRetrieval               # noqa: E402


def uneven(n, sizes=(16, 7, 11, 3)):
    """n items cut into batches of cycling, unequal sizes"""
    out, i = [], 0
    while n > 0:
        out.append(min(n, sizes[i % len(sizes)]))
        n -= out[-1]
        i += 1
    return out


def timed(fns, warmup, reps):
    """[(name, fn)] -> {name: per-call device milliseconds, one per repetition}; the functions alternate inside a repetition"""
    for _ in range(warmup):
        for _, fn in fns:
            fn()
    events = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            events[name].append((start, stop))
    torch.cuda.synchronize()
    return {name: [a.elapsed_time(b) for a, b in ev] for name, ev in events.items()}


def time_search(model, device, rows, queries, k, reps, warmup):
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    gallery = FeatureGallery(model, capacity=rows)
    for b in uneven(rows, (rows // 2, rows // 3, rows)):                     # pooled clip features "cached elsewhere"
        gallery.add_features(torch.randn(b, E, device=device, generator=g))
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    products, mult = gallery.products, T.logit_multiplier(model._logit_scale_value())
    q = gallery.backend.text_operand(seq.reshape(queries, -1))
    padded = torch.zeros(T.padded_video_rows(rows), 3 * E, device=device, dtype=torch.float16)
    padded[:rows] = gallery.rows

    def matrix_op():
        return torch.topk(torch.ops.centerclip.scaled_dot_planes(q, padded, rows, mult, products), k, dim=1)

    def matrix_api():
        return torch.topk(gallery.similarity_features(seq), k, dim=1)

    fns = [("search_features", lambda: gallery.search_features(seq, k=k)),
           ("similarity_features + topk (pads a copy per call)", matrix_api),
           ("similarity_topk op", lambda: torch.ops.centerclip.similarity_topk(q, gallery.rows, rows, mult, products, k)),
           ("scaled_dot_planes op on a padded copy + topk", matrix_op)]
    a, b = fns[2][1](), matrix_op()
    assert torch.equal(a[0], b[0]), "the two paths disagree on the scores"
    times = timed(fns, warmup, reps)
    read = rows * products * E * 2
    print("\n%d queries x %d gallery rows, E = %d, products = %d, k = %d: %d repetitions after %d warm-up rounds, device events"
          % (queries, rows, E, products, k, reps, warmup))
    for name, ms in times.items():
        print("  %-52s median %8.1f us   min %8.1f   max %8.1f" % (name, 1e3 * statistics.median(ms), 1e3 * min(ms), 1e3 * max(ms)))
    print("  the streaming kernel reads %d bytes of plane rows (%.0f MB); the matrix has %d bytes; search workspace %d bytes"
          % (read, read / 1e6, queries * rows * 4, L.lib().cc_similarity_topk_workspace_bytes(queries, rows, k)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=40, help="clips encoded into the gallery (0: skip the model part)")
    ap.add_argument("--captions", type=int, default=4)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--time-rows", type=int, default=200000, help="gallery rows of the timing part (0: skip it)")
    ap.add_argument("--time-queries", type=int, default=16)
    ap.add_argument("--time-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    c = bench.CFG2
    model = CLIP4Clip.from_state_dict(bench.random_state_dict(c, seed=0), bench.task_config(c)).to(device).eval()
    if a.clips:
        data = SyntheticRetrieval(a.clips)
        gallery = FeatureGallery(model)
        start = 0
        for b in uneven(a.clips):
            pos = gallery.add(data.video[start:start + b].to(device), data.vmask[start:start + b].to(device))
            print("added clips %d..%d as positions %d..%d" % (start, start + b - 1, int(pos[0]), int(pos[-1])))
            start += b
        ids = data.ids[:a.captions].to(device)
        scores, found = gallery.search(ids, k=a.k)
        for i in range(ids.shape[0]):
            print("caption %d: clips %s  scores %s" % (i, found[i].tolist(), ["%.4f" % s for s in scores[i].tolist()]))
        full = torch.topk(gallery.similarity(ids), min(a.k, len(gallery)), dim=1)
        print("same scores as the matrix path: %s" % bool(torch.equal(full.values, scores[:, :full.values.shape[1]])))
    if a.time_rows:
        time_search(model, device, a.time_rows, a.time_queries, a.time_k, a.reps, a.warmup)


if __name__ == "__main__":
    main()
