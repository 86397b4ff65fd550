"""Time of one ragged-batch collate call next to the per-clip way of doing the same (DESIGN.md "Ragged clip batches"): B = 16 clips
of T = 12 frames -> 224 px, the sizes cycling through 224x298, 224x398, 398x224 and 240x320, with resize=False and resize=True.

  * collate:  ClipCollate(224, 12, resize)(packed) - table build on the host, one small upload, at most two launches;
  * per clip: B calls of resize_center_crop on the same bytes (views of the packed buffer) + one torch.stack, plans warmed.

Both are timed eagerly, as a loader would call them: device events around REPS calls in a row (the span on the device, host
gaps included where the host is the limit), five rounds, the two ways alternating; the median round is reported with the
spread, next to the launches each way makes (counted from the plans' geometry; torch.stack is one more).  The outputs are
compared first: byte equality.

    python tools/collate_times.py [--out profiles/collate_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centerclip_amd.preprocess import ClipCollate, pack_clips, resize_center_crop     # noqa: E402

SIZES = ((224, 298), (224, 398), (398, 224), (240, 320))
B, T, N_PX, REPS, ROUNDS = 16, 12, 224, 20, 5


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    clips = [torch.randint(0, 256, (T,) + SIZES[b % len(SIZES)] + (3,), dtype=torch.uint8, generator=gen) for b in range(B)]
    packed = pack_clips(clips).to(device)
    views = [packed.clip(b) for b in range(B)]
    lines = ["ragged collate, %d clips x %d frames -> %d px, sizes %s, %s; %d rounds of %d calls, device events"
             % (B, T, N_PX, " ".join("%dx%d" % s for s in SIZES), torch.cuda.get_device_name(0), ROUNDS, REPS)]
    for resize in (False, True):
        collate = ClipCollate(N_PX, max_frames=T, resize=resize)

        def one():
            return collate(packed)

        def loop():
            return torch.stack([resize_center_crop(v, N_PX, resize) for v in views]).unsqueeze(1)
        assert torch.equal(one(), loop()), "the collate call and the per-clip loop differ"
        both = [bool(collate.plan(H, W)[11] and collate.plan(H, W)[12]) for H, W in SIZES]
        n_collate = 2 if any(both) else 1
        n_loop = sum(2 if both[b % len(SIZES)] else 1 for b in range(B)) + 1
        for fn in (one, loop):                                   # every shape and both workspaces warm
            event_ms(fn, 5)
        t_one, t_loop = [], []
        for _ in range(ROUNDS):
            t_one.append(event_ms(one, REPS))
            t_loop.append(event_ms(loop, REPS))
        lines.append("resize=%-5s  collate %.3f ms (min %.3f max %.3f), %d launches + 1 upload | per clip + stack %.3f ms (min %.3f "
                     "max %.3f), %d launches" % (resize, statistics.median(t_one), min(t_one), max(t_one), n_collate,
                                                 statistics.median(t_loop), min(t_loop), max(t_loop), n_loop))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
