"""Times of the frame transform on 4:2:0 sources (DESIGN.md "YUV 4:2:0 sources"): 192 frames (16 clips x 12) of 360x640 and
1080x1920 -> 224, NV12 and I420,

  * fused:     YuvFrameTransform(224)(yuv) - the conversion inside the first resampling pass;
  * two-step:  yuv420_to_rgb(yuv), then FrameTransform(224) on its output;
  * rgb:       FrameTransform(224) on frames converted beforehand (the conversion not timed) - the yardstick: what the loader
               pays once a CPU (or another kernel) has produced RGB.  With --baseline-lib PATH (a build of another commit's
               library, e.g. the parent's) also that library's cc_resize_crop_u8 on the same frames, same plan, same workspace.

Each is timed eagerly with device events around REPS calls in a row, ROUNDS rounds, the ways alternating within a round; the
median round is reported with the spread (min - max), next to the source bytes a call reads at least (the rows the window's
taps touch).  The outputs are compared first: byte equality.

    python tools/yuv_times.py [--baseline-lib PATH] [--out profiles/yuv_times.txt]

--formats (DESIGN.md "YUV sources in general", profiles/yuv_formats.txt): 1080x1920 only; fused "p010", "i420p10" and "i444" each
against yuv_to_rgb + FrameTransform, and fused "nv12" / "i420" - with --baseline-lib also that library's cc_resize_crop_yuv420_u8
on the same frames, plan and workspace, alternating with this build's call inside every round.

    python tools/yuv_times.py --formats [--baseline-lib PATH] [--out profiles/yuv_formats.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from centerclip_amd import _lib as L                                                   # noqa: E402
from centerclip_amd import torch_ops as T                                              # noqa: E402
from centerclip_amd.preprocess import FrameTransform, YuvFrameTransform, yuv420_to_rgb, yuv_to_rgb  # noqa: E402

SIZES = ((360, 640), (1080, 1920))
B, FRAMES, N_PX, REPS, ROUNDS = 16, 12, 224, 10, 7


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def baseline_call(path, rgb, out):
    """cc_resize_crop_u8 of the library at ``path`` on [F, H, W, 3] frames, with this build's plan and workspace"""
    lib = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.cc_resize_crop_u8.argtypes = [vp, i32, i32, i32, i32, vp, i32, i32, vp, i32, vp, ctypes.c_size_t, vp]
    lib.cc_resize_crop_u8.restype = ctypes.c_int
    F, H, W, _ = rgb.shape
    plan = T.resize_plan(H, W, N_PX, True, rgb.device)
    nws = L.lib().cc_resize_crop_workspace_bytes(F, H, W, N_PX, 1)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=rgb.device)

    def call():
        L.check(lib.cc_resize_crop_u8(L.ptr(rgb), 2, F, H, W, L.ptr(plan), N_PX, 1, L.ptr(out), 2, L.ptr(ws), nws,
                                      L.stream_ptr(rgb.device)), "baseline cc_resize_crop_u8")
    return call


def baseline_yuv420_call(path, yuv, kind, out):
    """cc_resize_crop_yuv420_u8 of the library at ``path`` on tight [F, 3H/2, W] frames, with this build's plan and workspace"""
    lib = ctypes.CDLL(path)
    vp, i32, lay = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(L.Yuv420Layout)
    lib.cc_resize_crop_yuv420_u8.argtypes = [vp, ctypes.c_size_t, lay, i32, i32, i32, vp, i32, i32, vp, i32, vp, ctypes.c_size_t, vp]
    lib.cc_resize_crop_yuv420_u8.restype = ctypes.c_int
    F, H, W = yuv.shape[0], yuv.shape[1] // 3 * 2, yuv.shape[2]
    layout = L.Yuv420Layout(*T.yuv420_tight_layout(kind, H, W, "bt601", False))
    plan = T.resize_plan(H, W, N_PX, True, yuv.device)
    nws = L.lib().cc_resize_crop_workspace_bytes(F, H, W, N_PX, 1)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=yuv.device)

    def call():
        L.check(lib.cc_resize_crop_yuv420_u8(L.ptr(yuv), yuv.numel(), ctypes.byref(layout), F, H, W, L.ptr(plan), N_PX, 1, L.ptr(out),
                                             2, L.ptr(ws), nws, L.stream_ptr(yuv.device)), "baseline cc_resize_crop_yuv420_u8")
    return call


def time_ways(ways):
    """-> {name: [ms per call of every round]}, the ways alternating within a round"""
    for fn in ways.values():                                         # warm: plans, workspaces, code objects
        fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in ways}
    for r in range(ROUNDS):
        order = list(ways) if r % 2 == 0 else list(ways)[::-1]
        for name in order:
            rounds[name].append(event_ms(ways[name], REPS))
    return rounds


def formats(a, device):
    """The --formats measurement -> lines"""
    H, W = SIZES[-1]
    gen = torch.Generator().manual_seed(0)
    F = B * FRAMES
    lines = ["frame transform on YUV sources, %d frames (%d clips x %d) of %dx%d -> %d px, %s; %d rounds of %d calls, device events, "
             "median (min - max) ms per call" % (F, B, FRAMES, H, W, N_PX, torch.cuda.get_device_name(0), ROUNDS, REPS)]
    rgb_t = FrameTransform(N_PX)
    for name in ("nv12", "i420", "p010", "i420p10", "i444"):
        _, sub_x, sub_y, depth, shift, _ = T.YUV_FORMATS[name]
        den = 1 << (sub_x + sub_y)
        shape = (F, H * (den + 2) // den, W)
        if depth == 8:
            yuv = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen).to(device)
        else:
            words = torch.randint(0, 1 << depth, shape, dtype=torch.int32, generator=gen) << shift
            yuv = torch.from_numpy(words.numpy().astype("uint16")).to(device)
        fused_t = YuvFrameTransform(N_PX, layout=name)
        ways = {"fused": lambda: fused_t(yuv), "two-step": lambda: rgb_t(yuv_to_rgb(yuv, name))}
        want = ways["two-step"]()
        assert torch.equal(ways["fused"](), want), "the ways differ"
        if a.baseline_lib and name in T.YUV_KINDS:
            out = torch.empty_like(want)
            ways["fused, baseline library"] = baseline_yuv420_call(a.baseline_lib, yuv, name, out)
            ways["fused, baseline library"]()
            assert torch.equal(out, want), "the baseline library gives other bytes"
        lines.append("%s (%.1f MB of source per call, whole frames):" % (name, yuv.numel() * yuv.element_size() / 1e6))
        for way, ms in time_ways(ways).items():
            lines.append("  %-24s %.3f (%.3f - %.3f)" % (way, statistics.median(ms), min(ms), max(ms)))
        del yuv, want
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--formats", action="store_true")
    a = ap.parse_args()
    if a.formats:
        text = "\n".join(formats(a, torch.device("cuda:0")))
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    device = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    F = B * FRAMES
    lines = ["frame transform on 4:2:0 sources, %d frames (%d clips x %d) -> %d px, %s; %d rounds of %d calls, device events, "
             "median (min - max) ms per call" % (F, B, FRAMES, N_PX, torch.cuda.get_device_name(0), ROUNDS, REPS)]
    for H, W in SIZES:
        for kind in ("nv12", "i420"):
            yuv = torch.randint(0, 256, (F, H * 3 // 2, W), dtype=torch.uint8, generator=gen).to(device)
            fused_t, rgb_t = YuvFrameTransform(N_PX, layout=kind), FrameTransform(N_PX)
            rgb = yuv420_to_rgb(yuv, layout=kind)
            ways = {"fused": lambda: fused_t(yuv), "two-step": lambda: rgb_t(yuv420_to_rgb(yuv, layout=kind)),
                    "rgb": lambda: rgb_t(rgb)}
            want = ways["rgb"]()
            assert torch.equal(ways["fused"](), want) and torch.equal(ways["two-step"](), want), "the ways differ"
            if a.baseline_lib:
                out = torch.empty_like(want)
                ways["rgb, baseline library"] = baseline_call(a.baseline_lib, rgb, out)
                ways["rgb, baseline library"]()
                assert torch.equal(out, want), "the baseline library gives other bytes"
            rounds = time_ways(ways)
            plan = rgb_t.plan(H, W, device).cpu()
            rows = int(plan[10] - plan[9])
            lines.append("%dx%d %s (window rows %d of %d; source bytes of those rows: 4:2:0 %.1f MB, RGB %.1f MB):"
                         % (H, W, kind, rows, H, F * rows * W * 1.5 / 1e6, F * rows * W * 3 / 1e6))
            for name, ms in rounds.items():
                lines.append("  %-22s %.3f (%.3f - %.3f)" % (name, statistics.median(ms), min(ms), max(ms)))
            del yuv, rgb, want
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
