"""Retrieval with a cached gallery on synthetic data: encode clips once, keep their similarity operands on the device, ask for
the k best clips of a caption.

    gallery = FeatureGallery(model); gallery.add(video, video_mask) ...; scores, ids = gallery.search(input_ids, k=10)

Random-init CLIP weights (no checkpoint / dataset access here), clips added in uneven batches.  The second part times the
search against the matrix path (the [Nq, N] matrix of eval_epoch + torch.topk) on a large gallery of random unit rows:
device events around every call, the two paths alternating, after a warm-up.

    python examples/search_synthetic.py [--clips 40] [--k 5] [--time-rows 200000] [--time-queries 16] [--time-k 10] [--reps 50]
    python examples/search_synthetic.py --clips 0 --time-rows 200000     (the timing alone)

--camoe_dsl 1 does the same under the CAMoE dual softmax (FeatureGallery(dual_softmax=True)): a clip gallery with the captions
as its bank, a caption gallery asked with clips, and the timing of similarity_topk_dsl against the plain op and of the
statistics pass (dsl_col_stats_planes) against the matrix op in blocks + dsl_col_stats.

    python examples/search_synthetic.py --camoe_dsl 1 [--time-bank 1000]

--groups G ranks groups of rows, each by its best row (FeatureGallery(grouped=True): the sentences of a video, the windows of a
long video): clips added in groups of 1..G rows and asked with search_groups, then the timing of search_groups_features
against plain search_features on the same gallery and against what there was before - similarity_features, a per-group
maximum, torch.topk - with groups of 1 row and of 1..G rows.

    python examples/search_synthetic.py --groups 40

--remove FRACTION / --subset FRACTION take clips out of the gallery (remove, then compact) and search within a subset
(allow= with a mask from row_mask or a device bool tensor), each checked against masking the matrix + torch.topk; the timing
is similarity_topk_masked with an all-ones mask, one contiguous 1/16 of the rows, random halves (one mask, one per query) and
the masked statistics pass against the unmasked ops - and, with --baseline-lib PATH, against another build's unmasked op.

    python examples/search_synthetic.py --remove 0.25 --subset 0.3 [--baseline-lib other/libcenterclip_hip.so]

--rank 1 asks where a known clip stands (FeatureGallery.rank: R@k, MdR, MnR without the matrix): every caption's own clip
against the matrix + rank_counts_cols, the cross-check with search (its entry at the rank is the target, same score bits), and
the timing of similarity_rank next to similarity_topk at --time-k and to the matrix op + rank_counts_cols, of its masked,
grouped and dual-softmax forms next to their top-k counterparts, and of the evaluation-size shape against the matrix path.

    python examples/search_synthetic.py --rank 1

--deep K asks for lists beyond 128 entries and walks one with a cursor (search*(k=K), after=): on a small gallery with removed
rows and runs of equal scores the list of K and three calls that continue each other are checked against the matrix + a
stable sort, rows and groups; the timing is the deep call next to the same gallery's search(k=128) - one page of it - and to
similarity() + torch.topk(k=K), and, with --baseline-lib PATH, to another build's k = 128 entry.

    python examples/search_synthetic.py --deep 1000 [--baseline-lib other/libcenterclip_hip.so]

--windows W1,W2,... (frames, multiples of the model's frames per segment) asks "which video, and where in it": two synthetic
videos of 10 x T frames go into a grouped gallery with FeatureGallery.add_windows - every frame encoded once, every window of
every scale one row, a video one group - search_groups names the video and windows() the frames of its best window; then
add_windows is timed against pushing the frames of every window through the encoder (the windows' frames cut out, laid end
to end as clips of T frames: the encoder work of adding every window on its own), host clock around a synchronised call.

    python examples/search_synthetic.py --windows 8,16 [--reps 5]
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


def report(title, times):
    print("\n" + title)
    for name, ms in times.items():
        print("  %-64s median %9.1f us   min %9.1f   max %9.1f" % (name, 1e3 * statistics.median(ms), 1e3 * min(ms), 1e3 * max(ms)))


def time_dsl(model, device, rows, queries, k, bank, reps, warmup):
    """similarity_topk_dsl against similarity_topk on `queries` x `rows`, and the statistics pass at rows x bank (a clip
    gallery's add) and queries x rows (a caption gallery's search) against the matrix op + dsl_col_stats"""
    op = torch.ops.centerclip
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    unit = lambda n, video_side: op.normalize_rows_planes(torch.randn(n, E, device=device, generator=g), video_side)
    gallery = FeatureGallery(model)
    products, mult = gallery.products, T.logit_multiplier(model._logit_scale_value())
    clips, captions = unit(rows, True), unit(rows, False)                     # a clip gallery, a caption gallery
    text_q, clip_q, bank_rows = unit(queries, False), unit(queries, True), unit(bank, False)
    m_g, s_g = op.dsl_col_stats_planes(bank_rows, clips, bank, rows, mult, products)
    m_q, s_q = op.dsl_col_stats_planes(captions, clip_q, rows, queries, mult, products)
    fns = [("similarity_topk (plain)", lambda: op.similarity_topk(text_q, clips, rows, mult, products, k)),
           ("similarity_topk_dsl, statistics per gallery row", lambda: op.similarity_topk_dsl(text_q, clips, rows, mult, products, k,
                                                                                            m_g, s_g, 1, bank)),
           ("similarity_topk_dsl, statistics per query row", lambda: op.similarity_topk_dsl(clip_q, captions, rows, mult, products,
                                                                                          k, m_q, s_q, 0, rows))]
    report("%d queries x %d gallery rows, E = %d, products = %d, k = %d: %d repetitions after %d warm-up rounds, device events"
           % (queries, rows, E, products, k, reps, warmup), timed(fns, warmup, reps))

    def blocks(text, video, n_video, block):
        """what a user had before: the matrix op on zero-padded blocks of the video rows, then the column statistics"""
        ms, ss = [], []
        for at in range(0, n_video, block):
            b = min(block, n_video - at)
            padded = torch.zeros(max(b, T.padded_video_rows(b)), 3 * E, device=device, dtype=torch.float16)
            padded[:b] = video[at:at + b]
            mb, sb = op.dsl_col_stats(op.scaled_dot_planes(text, padded, b, mult, products))
            ms.append(mb)
            ss.append(sb)
        return torch.cat(ms), torch.cat(ss)
    for title, text, video, nt, nv, block in (("a clip gallery's add", bank_rows, clips, bank, rows, 16384),
                                              ("a caption gallery's search", captions, clip_q, rows, queries, queries)):
        a, b = op.dsl_col_stats_planes(text, video, nt, nv, mult, products), blocks(text, video, nv, block)
        assert torch.equal(a[0], b[0]), "the two paths disagree on the maxima"
        fns = [("dsl_col_stats_planes", lambda: op.dsl_col_stats_planes(text, video, nt, nv, mult, products)),
               ("scaled_dot_planes on padded blocks of %d + dsl_col_stats" % block, lambda: blocks(text, video, nv, block))]
        report("statistics of %d video rows over %d text rows (%s): workspace %d bytes, the matrix %d bytes"
               % (nv, nt, title, L.lib().cc_dsl_col_stats_planes_workspace_bytes(nt, nv), nt * nv * 4), timed(fns, warmup, reps))


def dsl_part(model, device, a):
    """both sides under the dual softmax on encoded synthetic clips: the captions are the bank of the clip gallery"""
    data = SyntheticRetrieval(a.clips)
    ids = data.ids.to(device)
    gallery = FeatureGallery(model, dual_softmax=True)
    start = 0
    for b in uneven(a.clips):                                                # (clips before the bank or after it: the same bits)
        gallery.add(data.video[start:start + b].to(device), data.vmask[start:start + b].to(device))
        start += b
    gallery.set_query_bank(ids)
    scores, found = gallery.search(ids[:a.captions], k=a.k)
    for i in range(scores.shape[0]):
        print("caption %d: clips %s  dual-softmax scores %s" % (i, found[i].tolist(), ["%.4f" % s for s in scores[i].tolist()]))
    D = gallery.similarity(ids)
    full = torch.topk(D[:a.captions], min(a.k, len(gallery)), dim=1)
    print("same scores as dsl_apply_ on the matrix: %s" % bool(torch.equal(full.values, scores[:, :full.values.shape[1]])))
    captions = FeatureGallery(model, side="text", dual_softmax=True)
    captions.add(ids)
    video, vmask = data.video[:a.captions].to(device), data.vmask[:a.captions].to(device)
    scores, found = captions.search(video, vmask, k=a.k)
    for i in range(scores.shape[0]):
        print("clip %d: captions %s  dual-softmax scores %s" % (i, found[i].tolist(), ["%.4f" % s for s in scores[i].tolist()]))
    full = torch.topk(captions.similarity(video, vmask), min(a.k, len(captions)), dim=1)
    print("same scores as dsl_apply_ on the matrix: %s" % bool(torch.equal(full.values, scores[:, :full.values.shape[1]])))


def group_labels(rows, largest, seed=2):
    """one label per row: groups of 1..largest adjacent rows (seeded), labelled 0, 1, ... in row order -> CPU LongTensor"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, largest + 1, (rows,), generator=g)            # (more than enough groups)
    return torch.repeat_interleave(torch.arange(rows), sizes)[:rows].contiguous()


def time_groups(model, device, rows, queries, k, largest, reps, warmup):
    """search_groups_features against search_features on the same gallery and against the matrix path a user had before"""
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    feats = torch.randn(rows, E, device=device, generator=g)
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    for largest_here in sorted({1, largest}):
        labels = group_labels(rows, largest_here)
        gallery = FeatureGallery(model, capacity=rows, grouped=True)
        start = 0
        for b in uneven(rows, (rows // 2, rows // 3, rows)):                 # (batches that split groups)
            gallery.add_features(feats[start:start + b], group=labels[start:start + b])
            start += b
        n_groups = gallery.num_groups
        index = labels.to(device).expand(queries, rows)                      # (labels 0, 1, ...: the column of a group's maximum)

        def matrix_path():
            sim = gallery.similarity_features(seq)
            best = torch.full((queries, n_groups), float("-inf"), device=device).scatter_reduce_(1, index, sim, "amax")
            return torch.topk(best, min(k, n_groups), dim=1)

        fns = [("search_groups_features", lambda: gallery.search_groups_features(seq, k=k)),
               ("search_features (rows, not groups)", lambda: gallery.search_features(seq, k=k)),
               ("similarity_features + per-group max (scatter_reduce amax) + topk", matrix_path)]
        a, b = fns[0][1](), matrix_path()
        kk = b.values.shape[1]
        assert torch.equal(a[0][:, :kk], b.values), "the two paths disagree on the scores"
        report("%d queries x %d gallery rows in %d groups of 1..%d rows, E = %d, products = %d, k = %d: %d repetitions after %d "
               "warm-up rounds, device events" % (queries, rows, n_groups, largest_here, E, gallery.products, k, reps, warmup),
               timed(fns, warmup, reps))
        print("  search workspace %d bytes; the matrix has %d bytes, the per-group maxima %d more"
              % (L.lib().cc_similarity_topk_workspace_bytes(queries, rows, k), queries * rows * 4, queries * n_groups * 4))


def groups_part(model, device, a):
    """clips in groups of 1..G windows: the k best groups of every caption, each by its best window"""
    data = SyntheticRetrieval(a.clips)
    labels = 100 + group_labels(a.clips, a.groups)                           # (labels are any int64, not positions)
    gallery = FeatureGallery(model, grouped=True)
    start = 0
    for b in uneven(a.clips):
        gallery.add(data.video[start:start + b].to(device), data.vmask[start:start + b].to(device), group=labels[start:start + b])
        start += b
    print("%d clips in %d groups" % (len(gallery), gallery.num_groups))
    ids = data.ids[:a.captions].to(device)
    scores, groups, pos = gallery.search_groups(ids, k=a.k)
    for i in range(ids.shape[0]):
        print("caption %d: groups %s  by their clips %s  scores %s"
              % (i, groups[i].tolist(), pos[i].tolist(), ["%.4f" % s for s in scores[i].tolist()]))
    sim = gallery.similarity(ids)
    on_device = labels.to(device)
    want = torch.stack([sim[:, on_device == lab].max(dim=1).values for lab in labels.unique().tolist()], 1)
    full = torch.topk(want, min(a.k, gallery.num_groups), dim=1)
    print("same scores as the per-group maximum of the matrix: %s" % bool(torch.equal(full.values, scores[:, :full.values.shape[1]])))


def masked_part(model, device, a):
    """take clips out, search within a subset, close the holes - each against the matrix path on the same rows"""
    data = SyntheticRetrieval(a.clips)
    gallery = FeatureGallery(model)
    gallery.add(data.video.to(device), data.vmask.to(device))
    ids = data.ids[:a.captions].to(device)
    g = torch.Generator().manual_seed(3)
    order = torch.randperm(a.clips, generator=g)
    gone = order[:int(a.remove * a.clips)].sort().values
    subset = order[:max(1, int(a.subset * a.clips))].sort().values if a.subset else None      # (overlaps the removed ones)

    def check(title, got, sim, selectable):
        sim = sim.masked_fill(~selectable.to(device)[None, :], float("-inf"))
        full = torch.topk(sim, min(a.k, int(selectable.sum())), dim=1)
        print("%s: same scores as masking the matrix + topk: %s" % (title, bool(torch.equal(full.values, got[0][:, :full.values.shape[1]]))))
    sim = gallery.similarity(ids)
    live = torch.ones(a.clips, dtype=torch.bool)
    if gone.numel():
        gallery.remove(gone)
        live[gone] = False
        scores, found = gallery.search(ids, k=a.k)
        print("removed %d of %d clips: %d held, span %d" % (gone.numel(), a.clips, len(gallery), gallery.span))
        for i in range(ids.shape[0]):
            print("caption %d: clips %s  scores %s" % (i, found[i].tolist(), ["%.4f" % s for s in scores[i].tolist()]))
        check("after remove", (scores, found), sim, live)
    if subset is not None:
        mask = gallery.row_mask(positions=subset)                            # built once, passed to any number of searches
        allowed = torch.zeros(a.clips, dtype=torch.bool)
        allowed[subset] = True
        check("allow= a subset of %d" % subset.numel(), gallery.search(ids, k=a.k, allow=mask), sim, allowed & live)
        check("allow= the same subset as a device bool tensor", gallery.search(ids, k=a.k, allow=allowed.to(device)), sim, allowed & live)
    new_pos = gallery.compact()
    fresh = FeatureGallery(model)
    fresh.add(data.video[live].to(device), data.vmask[live].to(device))
    same = torch.equal(gallery.rows.view(torch.int16), fresh.rows.view(torch.int16))
    print("compact(): %d rows, new positions of the first clips %s; the gallery of the survivors bit for bit: %s"
          % (len(gallery), new_pos[:8].tolist(), same))


def time_masked(model, device, rows, queries, k, reps, warmup, baseline_lib):
    """The masked top-k entry at the shapes DESIGN.md records - all ones, one contiguous 1/16 of the rows, random halves (one
    mask and one per query) - against the unmasked entry of this build and, with --baseline-lib, of another build of the
    library (same buffers, same stream); then the masked statistics op against the unmasked one."""
    import ctypes
    op = torch.ops.centerclip
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    unit = lambda n, video_side: op.normalize_rows_planes(torch.randn(n, E, device=device, generator=g), video_side)
    products, mult = FeatureGallery(model).products, T.logit_multiplier(model._logit_scale_value())
    clips, text_q, captions, clip_q = unit(rows, True), unit(queries, False), unit(rows, False), unit(queries, True)
    flags = lambda *shape: torch.rand(*shape, device=device, generator=g) < 0.5
    ones = op.pack_row_mask(torch.ones(rows, dtype=torch.bool, device=device))[0]
    block = torch.zeros(rows, dtype=torch.bool, device=device)
    block[rows // 2:rows // 2 + rows // 16] = True
    sixteenth, half, per_query = op.pack_row_mask(block)[0], op.pack_row_mask(flags(rows))[0], op.pack_row_mask(flags(queries, rows))
    # the library's entries called directly on buffers allocated once (no allocation, no int64 copy of the ids, a few
    # microseconds of host work a call): behind the ops' host work a 1/16 search would hide
    scores = torch.empty(queries, k, device=device)
    found = torch.empty(queries, k, device=device, dtype=torch.int32)
    ws = L.workspace(L.lib().cc_similarity_topk_workspace_bytes(queries, rows, k), device)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32

    def plain_of(lib):
        lib.cc_similarity_topk_planes_f32.argtypes = [vp, vp, i32, i32, i32, ctypes.c_float, i32, i32, vp, vp, vp, ctypes.c_size_t, vp]
        return lambda: L.check(lib.cc_similarity_topk_planes_f32(L.ptr(text_q), L.ptr(clips), queries, rows, E, mult, products, k,
                                                                 L.ptr(scores), L.ptr(found), L.ptr(ws), ws.numel(),
                                                                 L.stream_ptr(device)), "cc_similarity_topk_planes_f32")

    def masked(mask):
        return lambda: L.check(L.lib().cc_similarity_topk_masked_planes_f32(
            L.ptr(text_q), L.ptr(clips), queries, rows, E, mult, products, k, L.ptr(mask), 1 if mask.dim() == 1 else queries,
            mask.shape[-1], None, None, 1, 0, None, L.ptr(scores), L.ptr(found), L.ptr(ws), ws.numel(), L.stream_ptr(device)),
            "cc_similarity_topk_masked_planes_f32")
    want = op.similarity_topk(text_q, clips, rows, mult, products, k)
    fns = [("cc_similarity_topk_planes_f32 (this build)", plain_of(L.lib()))]
    if baseline_lib:
        fns.append(("cc_similarity_topk_planes_f32 (--baseline-lib)", plain_of(ctypes.CDLL(baseline_lib))))
    fns += [("cc_similarity_topk_masked_planes_f32, all ones", masked(ones))]
    for _, fn in fns:                                                        # both builds, and the all-ones mask: the op's result
        scores.zero_()
        fn()
        assert torch.equal(scores, want[0]) and torch.equal(found.long(), want[1]), "the paths disagree"
    fns += [("... one contiguous 1/16 of the rows", masked(sixteenth)),
            ("... random p = 0.5 (every tile live)", masked(half)),
            ("... one mask per query, p = 0.5", masked(per_query))]
    report("%d queries x %d gallery rows, E = %d, products = %d, k = %d: %d repetitions after %d warm-up rounds, device events"
           % (queries, rows, E, products, k, reps, warmup), timed(fns, warmup, reps))
    fns = [("dsl_col_stats_planes", lambda: op.dsl_col_stats_planes(captions, clip_q, rows, queries, mult, products)),
           ("dsl_col_stats_planes_masked, random p = 0.5", lambda: op.dsl_col_stats_planes_masked(captions, clip_q, rows, queries, mult,
                                                                                                 products, half)),
           ("dsl_col_stats_planes_masked, one contiguous 1/16", lambda: op.dsl_col_stats_planes_masked(captions, clip_q, rows, queries,
                                                                                                      mult, products, sixteenth))]
    report("statistics of %d video rows over %d text rows" % (queries, rows), timed(fns, warmup, reps))


def rank_part(model, device, a):
    """where every caption's own clip stands: rank against the matrix + rank_counts_cols, and against search's own order"""
    data = SyntheticRetrieval(a.clips)
    gallery = FeatureGallery(model)
    gallery.add(data.video.to(device), data.vmask.to(device))
    ids = data.ids.to(device)
    truth = torch.arange(a.clips)                                            # caption i describes clip i
    ranks, scores, counts = gallery.rank(ids, target=truth)
    for i in range(min(a.captions, a.clips)):
        print("caption %d: its clip stands at place %d (score %.4f; %d clips above, %d equal)"
              % (i, int(ranks[i]), float(scores[i]), int(counts[i, 0]), int(counts[i, 1])))
    sim = gallery.similarity(ids)
    want = torch.ops.centerclip.rank_counts_cols(sim, truth.to(device, torch.int32))
    print("same counts as rank_counts_cols on the matrix: %s; same score bits: %s"
          % (bool(torch.equal(counts, want)), bool(torch.equal(scores, sim.diagonal().contiguous()))))
    r = ranks.cpu().numpy()
    print("R@1 %.1f  R@5 %.1f  R@10 %.1f  MdR %.1f  MnR %.1f  (no matrix)"
          % tuple([100.0 * float((r < k).mean()) for k in (1, 5, 10)] + [float(statistics.median(r + 1)), float(r.mean() + 1)]))
    # against the search: for every caption whose rank is below k, search's entry at that rank is the target, same score bits.
    # Half the targets are taken from search's own result at seeded places, so at least half the captions are checked.
    k = min(a.k, a.clips)
    found_scores, found = gallery.search(ids, k=k)
    g = torch.Generator().manual_seed(4)
    at = torch.randint(0, k, (a.clips,), generator=g)
    target = torch.randint(0, a.clips, (a.clips,), generator=g)
    target[::2] = found.cpu()[torch.arange(a.clips), at][::2]
    ranks, scores, _ = gallery.rank(ids, target=target)
    inside = (ranks.cpu() < k).nonzero().flatten()
    place = ranks.cpu()[inside]
    assert inside.numel() >= a.clips // 2, "the cross-check with the search ran (nearly) empty"
    same = torch.equal(found.cpu()[inside, place], target[inside]) and torch.equal(found_scores.cpu()[inside, place], scores.cpu()[inside])
    print("search(k=%d) holds the target at its rank with the same score for all %d of %d captions ranked below k: %s"
          % (k, inside.numel(), a.clips, same))


def time_rank(model, device, rows, queries, k, largest, bank, reps, warmup):
    """similarity_rank next to the top-k op at k (untouched: the yardstick) and to the matrix op + rank_counts_cols on a ready
    padded copy; rank_features next to similarity_features + counts; the masked, grouped and dual-softmax forms next to their
    top-k counterparts; then the evaluation-size shape (10,000 captions x 1,000 clips, both directions) against the matrix"""
    op = torch.ops.centerclip
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    gallery = FeatureGallery(model, capacity=rows)
    for b in uneven(rows, (rows // 2, rows // 3, rows)):
        gallery.add_features(torch.randn(b, E, device=device, generator=g))
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    products, mult = gallery.products, T.logit_multiplier(model._logit_scale_value())
    q, clips = gallery.backend.text_operand(seq.reshape(queries, -1)), gallery.rows
    padded = torch.zeros(T.padded_video_rows(rows), 3 * E, device=device, dtype=torch.float16)
    padded[:rows] = clips
    target = torch.randint(0, rows, (queries,), device=device, generator=g)
    target32 = target.to(torch.int32)

    def matrix_op():
        return op.rank_counts_cols(op.scaled_dot_planes(q, padded, rows, mult, products), target32)

    def matrix_api():
        return op.rank_counts_cols(gallery.similarity_features(seq), target32)

    fns = [("similarity_rank op", lambda: op.similarity_rank(q, clips, rows, mult, products, target32)),
           ("similarity_topk op, k = %d (the yardstick)" % k, lambda: op.similarity_topk(q, clips, rows, mult, products, k)),
           ("scaled_dot_planes op on a padded copy + rank_counts_cols", matrix_op),
           ("rank_features", lambda: gallery.rank_features(seq, target)),
           ("similarity_features + rank_counts_cols (pads a copy per call)", matrix_api)]
    assert torch.equal(fns[0][1]()[0], matrix_op()), "the two paths disagree on the counts"
    title = "%d queries x %d gallery rows, E = %d, products = %d: %d repetitions after %d warm-up rounds, device events"
    report(title % (queries, rows, E, products, reps, warmup), timed(fns, warmup, reps))
    print("  rank workspace %d bytes; the matrix has %d bytes" % (L.lib().cc_similarity_rank_workspace_bytes(queries, rows),
                                                                   queries * rows * 4))
    # the forms: one mask (random half), one per query, groups of 1..largest rows, the dual softmax per gallery / query row
    flags = lambda *shape: torch.rand(*shape, device=device, generator=g) < 0.5
    half, per_query = op.pack_row_mask(flags(rows))[0], op.pack_row_mask(flags(queries, rows))
    labels = group_labels(rows, largest)
    first = torch.cat([torch.ones(1, dtype=torch.bool), labels[1:] != labels[:-1]])
    head = torch.cummax(torch.where(first, torch.arange(rows), torch.zeros(rows, dtype=torch.long)), 0).values.to(device, torch.int32)
    unit = lambda n, video_side: op.normalize_rows_planes(torch.randn(n, E, device=device, generator=g), video_side)
    bank_rows, captions, clip_q = unit(bank, False), unit(rows, False), unit(queries, True)
    m_g, s_g = op.dsl_col_stats_planes(bank_rows, clips, bank, rows, mult, products)
    m_q, s_q = op.dsl_col_stats_planes(captions, clip_q, rows, queries, mult, products)
    pair = lambda name, rank, topk: [("similarity_rank, " + name, rank), ("similarity_topk (k = %d), " % k + name, topk)]
    fns = (pair("one mask, p = 0.5", lambda: op.similarity_rank(q, clips, rows, mult, products, target32, half),
                lambda: op.similarity_topk_masked(q, clips, rows, mult, products, k, half))
           + pair("one mask per query, p = 0.5", lambda: op.similarity_rank(q, clips, rows, mult, products, target32, per_query),
                  lambda: op.similarity_topk_masked(q, clips, rows, mult, products, k, per_query))
           + pair("groups of 1..%d rows" % largest, lambda: op.similarity_rank(q, clips, rows, mult, products, target32, group_head=head),
                  lambda: op.similarity_topk_grouped(q, clips, rows, mult, products, k, head))
           + pair("dual softmax per gallery row", lambda: op.similarity_rank(q, clips, rows, mult, products, target32, None, m_g, s_g, 1, bank),
                  lambda: op.similarity_topk_dsl(q, clips, rows, mult, products, k, m_g, s_g, 1, bank))
           + pair("dual softmax per query row", lambda: op.similarity_rank(clip_q, captions, rows, mult, products, target32, None, m_q, s_q, 0, rows),
                  lambda: op.similarity_topk_dsl(clip_q, captions, rows, mult, products, k, m_q, s_q, 0, rows)))
    report("the forms, same shape", timed(fns, warmup, reps))
    # the evaluation-size shape: the device work of both directions' counts, with and without the matrix
    nt, nv = 10000, 1000
    text, video = unit(nt, False), unit(nv, True)
    vpad = torch.zeros(T.padded_video_rows(nv), 3 * E, device=device, dtype=torch.float16)
    vpad[:nv] = video
    gt = torch.randint(0, nv, (nt,), device=device, generator=g)
    gt32, first_text = gt.to(torch.int32), torch.arange(nv, device=device, dtype=torch.int32) * (nt // nv)

    def with_matrix():
        sim = op.scaled_dot_planes(text, vpad, nv, mult, products)
        ref = sim[first_text.long(), torch.arange(nv, device=device)]
        return op.rank_counts_cols(sim, gt32), op.rank_counts_ref(sim, ref.contiguous(), True)

    def without():
        return (op.similarity_rank(text, video, nv, mult, products, gt32)[0],
                op.similarity_rank(video, text, nt, mult, products, first_text)[0])
    a, b = with_matrix(), without()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1][:, :2]), "the two paths disagree on the counts"
    report("evaluation size: %d captions x %d clips, text->video and video->text counts" % (nt, nv),
           timed([("scaled_dot_planes + rank_counts_cols + rank_counts_ref (the matrix path)", with_matrix),
                  ("similarity_rank x 2 (no matrix)", without)], warmup, reps))


def deep_part(model, device, k, rows=5000, queries=6):
    """a list of k entries and a three-step cursor walk over it, against the matrix + a stable sort, rows and groups"""
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(5)
    feats = torch.randn(rows, E, device=device, generator=g)
    feats[1::7] = feats[0]                                                   # (runs of equal scores across the page edges)
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    labels = group_labels(rows, 5)
    gallery = FeatureGallery(model, grouped=True)
    gallery.add_features(feats, group=labels)
    gallery.remove(list(range(3, rows, 11)))
    sim = gallery.similarity_features(seq)                                   # (-inf in the removed columns)
    held = len(gallery)
    order = torch.sort(sim, dim=1, descending=True, stable=True)
    kk = min(k, held)
    scores, found = gallery.search_features(seq, k=k)
    same = torch.equal(found[:, :kk], order.indices[:, :kk]) and torch.equal(scores[:, :kk], order.values[:, :kk])
    print("search_features(k=%d) over %d rows held: the first %d entries of the matrix row's stable sort, same bits: %s; the fill "
          "behind them: %s" % (k, held, kk, same, bool((found[:, kk:] == -1).all())))
    steps, walk, after = (k // 3, k // 3, k - 2 * (k // 3)), [], None
    for step in steps:
        walk.append(gallery.search_features(seq, k=step, after=after))
        after = (walk[-1][0][:, -1], walk[-1][1][:, -1])
    same = torch.equal(torch.cat([w[1] for w in walk], 1), found) and torch.equal(torch.cat([w[0] for w in walk], 1), scores)
    print("three calls of k = %s, each after= the last column of the one before: the columns of the one call: %s" % (list(steps), same))
    # groups: the matrix, the per-group maximum, the stable sort - a group by its best row
    on_device = labels.to(device)
    best = torch.full((queries, int(labels.max()) + 1), float("-inf"), device=device).scatter_reduce_(
        1, on_device.expand(queries, rows), sim, "amax")
    want = torch.sort(best, dim=1, descending=True, stable=True)
    n_groups = int((want.values[0] > float("-inf")).sum())
    kg = min(k, n_groups)
    gs, gl, gp = gallery.search_groups_features(seq, k=k)
    walk, after = [], None
    for step in steps:
        walk.append(gallery.search_groups_features(seq, k=step, after=after))
        after = (walk[-1][0][:, -1], walk[-1][2][:, -1])
    same = torch.equal(gs[:, :kg], want.values[:, :kg]) and all(len(set(r[:kg])) == kg for r in gl.tolist())
    print("search_groups_features(k=%d) over %d groups: the per-group maxima in stable order, no group twice: %s; the cursor walk "
          "gives its columns: %s" % (k, n_groups, same, torch.equal(torch.cat([w[2] for w in walk], 1), gp)
                                     and torch.equal(torch.cat([w[0] for w in walk], 1), gs)))


def time_deep(model, device, rows, queries, k, reps, warmup, baseline_lib):
    """the deep call next to the same gallery's search(k=128) - one page, the yardstick; with --baseline-lib another build's
    k = 128 entry on the same buffers - and to similarity() + torch.topk(k), the only way to such a list before"""
    import ctypes
    E = int(model.clip_config['embed_dim'])
    g = torch.Generator(device=device).manual_seed(1)
    gallery = FeatureGallery(model, capacity=rows)
    for b in uneven(rows, (rows // 2, rows // 3, rows)):
        gallery.add_features(torch.randn(b, E, device=device, generator=g))
    seq = torch.randn(queries, 1, E, device=device, generator=g)
    products, mult = gallery.products, T.logit_multiplier(model._logit_scale_value())
    q = gallery.backend.text_operand(seq.reshape(queries, -1))
    op, lib = torch.ops.centerclip, L.lib()
    a, b = gallery.search_features(seq, k=k), torch.topk(gallery.similarity_features(seq), k, dim=1)
    assert torch.equal(a[0], b.values), "the two paths disagree on the scores"
    page = gallery.search_features(seq, k=128)
    assert torch.equal(a[0][:, :128], page[0]) and torch.equal(a[1][:, :128], page[1]), "the first page is not search(k=128)"
    scores = torch.empty(queries, 128, device=device)
    found = torch.empty(queries, 128, device=device, dtype=torch.int32)
    ws = L.workspace(lib.cc_similarity_topk_workspace_bytes(queries, rows, 128), device)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32

    def plain_of(build):
        build.cc_similarity_topk_planes_f32.argtypes = [vp, vp, i32, i32, i32, ctypes.c_float, i32, i32, vp, vp, vp, ctypes.c_size_t, vp]
        return lambda: L.check(build.cc_similarity_topk_planes_f32(L.ptr(q), L.ptr(gallery.rows), queries, rows, E, mult, products, 128,
                                                                   L.ptr(scores), L.ptr(found), L.ptr(ws), ws.numel(),
                                                                   L.stream_ptr(device)), "cc_similarity_topk_planes_f32")
    fns = [("search_features(k=%d): %d pages" % (k, -(-k // 128)), lambda: gallery.search_features(seq, k=k)),
           ("search_features(k=128): one page, the yardstick", lambda: gallery.search_features(seq, k=128)),
           ("similarity_topk_deep op, k = %d" % k, lambda: op.similarity_topk_deep(q, gallery.rows, rows, mult, products, k)),
           ("cc_similarity_topk_planes_f32, k = 128 (this build)", plain_of(lib))]
    if baseline_lib:
        fns.append(("cc_similarity_topk_planes_f32, k = 128 (--baseline-lib)", plain_of(ctypes.CDLL(baseline_lib))))
    for _, fn in fns[3:]:
        scores.zero_()
        fn()
        assert torch.equal(scores, page[0]) and torch.equal(found.long(), page[1]), "the builds disagree"
    fns.append(("similarity_features + torch.topk(k=%d) (the matrix)" % k, lambda: torch.topk(gallery.similarity_features(seq), k, dim=1)))
    report("%d queries x %d gallery rows, E = %d, products = %d: %d repetitions after %d warm-up rounds, device events"
           % (queries, rows, E, products, reps, warmup), timed(fns, warmup, reps))
    print("  deep workspace %d bytes (one page and the cursors, whatever k); the matrix has %d bytes"
          % (lib.cc_similarity_topk_deep_workspace_bytes(queries, rows, E, products, k), queries * rows * 4))


def windows_part(model, device, a):
    """long videos as groups of sliding windows: one encode, every window's row in one launch, the frames it stands for"""
    import time
    scales = [int(w) for w in a.windows.split(",")]
    T_clip, videos = int(model.video_frames), 2
    F = 10 * T_clip
    g = torch.Generator().manual_seed(6)
    video = torch.randn(videos, 1, F, 3, 224, 224, generator=g).to(device)
    lengths = [F, F - T_clip // 2]                                           # (the second one ends inside its last clip)
    gallery = FeatureGallery(model, grouped=True)
    pos, windows = gallery.add_windows(video, lengths, scales, group=[100, 101])
    print("%d videos of %d frames, windows of %s frames: %d rows in %d groups, every frame encoded once"
          % (videos, F, scales, len(gallery), gallery.num_groups))
    ids = SyntheticRetrieval(a.captions).ids.to(device)
    scores, groups, best = gallery.search_groups(ids, k=1)
    frames = gallery.windows(best.cpu().reshape(-1))
    for i in range(ids.shape[0]):
        print("caption %d: video %d, frames [%d, %d)  score %.4f" % (i, int(groups[i, 0]), int(frames[i, 0]), int(frames[i, 1]),
                                                                      float(scores[i, 0])))
    # the encoder work of adding every window on its own: the windows' frames, end to end, as clips of T frames
    index = torch.cat([v * F + torch.arange(lo, hi) for v, lo, hi in windows.tolist()])
    index = torch.cat([index, index[:(-index.numel()) % T_clip]])            # (whole clips)
    flat = video.reshape((videos * F,) + tuple(video.shape[3:]))

    def one_encode():
        gallery.clear()
        gallery.add_windows(video, lengths, scales, group=[100, 101])

    def every_window():
        plain = FeatureGallery(model)
        clips = flat[index.to(device)].reshape((-1, 1, T_clip) + tuple(flat.shape[1:]))
        for at in range(0, clips.shape[0], 64):
            part = clips[at:at + 64]
            plain.add(part, torch.ones(part.shape[0], 1, T_clip, dtype=torch.long, device=device))

    print("\n%d frames in the videos, %d frames in their %d windows: %d repetitions after one warm-up, host clock, synchronised"
          % (videos * F, index.numel(), windows.shape[0], a.reps))
    for name, fn in (("add_windows (one encode, one pooling launch)", one_encode),
                     ("the frames of every window through the encoder", every_window)):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            start = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - start))
        print("  %-52s median %8.1f ms   min %8.1f   max %8.1f" % (name, statistics.median(ms), min(ms), max(ms)))


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
    ap.add_argument("--camoe_dsl", type=int, default=0, help="1: the dual softmax (FeatureGallery(dual_softmax=True))")
    ap.add_argument("--time-bank", type=int, default=1000, help="--camoe_dsl 1: captions in the bank of the timed clip gallery")
    ap.add_argument("--groups", type=int, default=0, help="G > 0: grouped search (FeatureGallery(grouped=True)), groups of 1..G rows")
    ap.add_argument("--remove", type=float, default=0.0, help="FRACTION > 0: remove that share of the clips, search, compact()")
    ap.add_argument("--subset", type=float, default=0.0, help="FRACTION > 0: search within that share of the clips (allow=)")
    ap.add_argument("--baseline-lib", default="", help="--remove / --subset: another build of the library to time the unmasked op of")
    ap.add_argument("--rank", type=int, default=0, help="1: the rank of a known clip (FeatureGallery.rank), checked and timed")
    ap.add_argument("--deep", type=int, default=0, help="K > 128: a list of K entries and a cursor walk, checked and timed")
    ap.add_argument("--windows", default="", help="W1,W2,...: windows of long videos (FeatureGallery.add_windows), frames per scale")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    c = bench.CFG2
    model = CLIP4Clip.from_state_dict(bench.random_state_dict(c, seed=0), bench.task_config(c)).to(device).eval()
    if a.windows:
        windows_part(model, device, a)
        return
    if a.deep:
        if a.clips:
            deep_part(model, device, a.deep)
        if a.time_rows:
            time_deep(model, device, a.time_rows, a.time_queries, a.deep, a.reps, a.warmup, a.baseline_lib)
        return
    if a.rank:
        if a.clips:
            rank_part(model, device, a)
        if a.time_rows:
            time_rank(model, device, a.time_rows, a.time_queries, a.time_k, a.groups or 40, a.time_bank, a.reps, a.warmup)
        return
    if a.remove or a.subset:
        if a.clips:
            masked_part(model, device, a)
        if a.time_rows:
            time_masked(model, device, a.time_rows, a.time_queries, a.time_k, a.reps, a.warmup, a.baseline_lib)
        return
    if a.camoe_dsl:
        if a.clips:
            dsl_part(model, device, a)
        if a.time_rows:
            time_dsl(model, device, a.time_rows, a.time_queries, a.time_k, a.time_bank, a.reps, a.warmup)
        return
    if a.groups:
        if a.clips:
            groups_part(model, device, a)
        if a.time_rows:
            time_groups(model, device, a.time_rows, a.time_queries, a.time_k, a.groups, a.reps, a.warmup)
        return
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
