"""Times of the device frame transform next to what it has to hide under (DESIGN.md "Resize and centre crop"): for 192 frames
(16 clips x 12) at 240x320 and 360x640 -> 224,

  * the transform itself, from the events of its own dispatches (20 launches in one hipGraph, as bench_common.graph_time_ms),
    with its HBM traffic (source rows read + intermediate written and read + output written) over the HBM peak;
  * the host -> device copy of the same raw batch from pinned memory;
  * the cfg-2 forward step on resident uint8 frames of the model's resolution;
  * the evaluation step fed through DeviceFeeder from pinned host batches, raw frames + transform against ready frames.

    python tools/resize_times.py [--out profiles/resize_times.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_common as bc                                    # noqa: E402
from centerclip_amd import _lib as L                         # noqa: E402
from centerclip_amd.clip4clip import CLIP4Clip               # noqa: E402
from centerclip_amd.feeder import DeviceFeeder               # noqa: E402
from centerclip_amd.preprocess import FrameTransform         # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, MI355X


def fed_step_ms(model, batches, device, transform, steps):
    """Wall time per batch of `steps` forward steps fed by a DeviceFeeder from pinned host batches (ends in a synchronise)."""
    feeder = DeviceFeeder(device, depth=2, frame_transform=transform, video_index=3)

    def run(n):
        with torch.no_grad():
            for _, (ids, mask, seg, video, vmask) in feeder(batches[i % len(batches)] for i in range(n)):
                model(ids, seg, mask, video, vmask)
        torch.cuda.synchronize()
    run(4)
    t0 = time.perf_counter()
    run(steps)
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    c = bc.CFG2
    B, T, res = c["B"], c["T"], c["res"]
    lines = ["device frame transform, %d frames (%d clips x %d) -> %d, %s" % (B * T, B, T, res, torch.cuda.get_device_name(0))]
    model = CLIP4Clip.from_state_dict(bc.random_state_dict(c, seed=0), bc.task_config(c)).to(device).eval()
    ids, amask, _, vmask = bc.synthetic_batch(c, device, seed=1)
    seg = torch.zeros_like(ids)
    gen = torch.Generator().manual_seed(2)
    ready = torch.randint(0, 256, (B, 1, T, res, res, 3), dtype=torch.uint8, generator=gen)
    ready_dev = ready.to(device)
    with torch.no_grad():
        step = bc.graph_time_ms(lambda: model(ids, seg, amask, ready_dev, vmask), launches=4)
    lines.append("cfg-2 forward step, resident uint8 frames: %.3f ms" % step)
    host_ready = [tuple(t.cpu().pin_memory() for t in (ids, amask, seg, ready, vmask))]
    base = fed_step_ms(model, host_ready, device, None, a.steps)
    lines.append("cfg-2 step fed by DeviceFeeder, ready %dx%d frames from pinned memory: %.3f ms per batch" % (res, res, base))
    lib = L.lib()
    for (H, W) in ((240, 320), (360, 640)):
        raw = torch.randint(0, 256, (B, 1, T, H, W, 3), dtype=torch.uint8, generator=gen).pin_memory()
        raw_dev = raw.to(device)
        t = FrameTransform(res)
        t(raw_dev)
        ms = bc.graph_time_ms(lambda: t(raw_dev), launches=20)
        plan = t.plan(H, W, device).cpu()
        rows = int(plan[10] - plan[9])
        mid = lib.cc_resize_crop_workspace_bytes(B * T, H, W, res, 1)
        moved = B * T * 3 * (rows * W + res * res) + 2 * mid
        dst = torch.empty_like(raw_dev)
        copy = bc.event_time_ms(lambda: dst.copy_(raw, non_blocking=True), 20)
        fed = fed_step_ms(model, [tuple(host_ready[0][:3]) + (raw,) + tuple(host_ready[0][4:])], device, t, a.steps)
        lines.append("%dx%d: transform %.3f ms (%.1f MB moved: %.3f ms at the HBM peak, %.0f %% of it); H2D copy of the raw batch "
                     "(%.1f MB) %.3f ms; cfg-2 step fed by DeviceFeeder with the transform on the copy stream: %.3f ms per batch "
                     "(ready frames: %.3f)" % (H, W, ms, moved / 1e6, moved / HBM_PEAK * 1e3, 100 * moved / HBM_PEAK * 1e3 / ms,
                                               raw.numel() / 1e6, copy, fed, base))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
