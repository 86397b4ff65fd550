"""GPU time of the train-time augmentation launch (preprocess.TrainFrameTransform.apply on a device box table) for 16 clips x 12
frames 240 x 320 -> 224, next to preprocess.FrameTransform's centre crop of the same frames in the same session: device events
around one eager call into a reused output buffer, median of 50 after 10 warm-up calls (profiles/augment_times.txt; DESIGN.md
section 7, "Train-time augmentation").  Recorded, not asserted.

    python tools/augment_times.py [--out profiles/augment_times.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centerclip_amd.preprocess import FrameTransform, TrainFrameTransform  # noqa: E402

B, T, H, W, N_PX = 16, 12, 240, 320, 224


def timed(fn, reps=50):
    """-> (median, min, max) in microseconds"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_times.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    video = torch.randint(0, 256, (B, 1, T, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.empty(B, 1, T, N_PX, N_PX, 3, dtype=torch.uint8, device=dev)
    lines = ["train-time augmentation, %d frames (%d clips x %d) %dx%d -> %d (%.1f MB in, %.1f MB out), one MI355X; device events "
             "around one eager call, median (min - max) of 50" % (B * T, B, T, H, W, N_PX, video.numel() / 1e6, out.numel() / 1e6)]
    fmt = "%-72s %6.1f us (%.1f - %.1f)"
    for crop, interp in (("multiscale", "bilinear"), ("multiscale", "bicubic"), ("random_resized", "bicubic"),
                         ("random_resized", "bilinear")):
        t = TrainFrameTransform(N_PX, crop=crop, interpolation=interp, flip=True, seed=0)
        boxes = t.sample(B, H, W).to(dev)
        lines.append(fmt % (("TrainFrameTransform.apply, %s boxes + flips, %s:" % (crop, interp),)
                            + timed(lambda: t.apply(video, boxes, out=out))))
    ft = FrameTransform(N_PX)
    lines.append(fmt % (("FrameTransform: resize + centre crop (two launches):",) + timed(lambda: ft(video, out=out))))
    ft0 = FrameTransform(N_PX, resize=False)
    lines.append(fmt % (("FrameTransform(resize=False): the centre crop alone (a strided copy):",) + timed(lambda: ft0(video, out=out))))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
