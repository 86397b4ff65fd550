"""Times of the camoe_dsl paths on the MI355X (written to profiles/dsl_times.txt).

  python tools/dsl_times.py eval                       stats + apply at 10,000 x 1,000 against the eager torch expression
  python tools/dsl_times.py train [--parent DIR]       the captured cfg-2 step with camoe_dsl=1 against the step without it,
                                                       one fresh process per line, the variants alternating; --parent: a
                                                       checkout of the parent commit with its own build of the library

Evaluation: device events around windows of REPS calls (a single call of ~20 us would measure the event pair), the two
variants alternating window by window in one process; median (min, max) over the windows.  Bytes: the two passes touch the
matrix three times (read for the statistics, read and write for the rewrite) = 120 MB at 10k x 1k.
Training: GraphedTrainStep (AdamW + lr_scheduler('cos') + clip 1.0, random ViT-B/32 weights, batch 16), host clock around
synchronised windows of 10 replays.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stat(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def eval_times(rows=10000, cols=1000, reps=50, windows=9):
    import torch
    sys.path.insert(0, ROOT)
    from centerclip_amd import torch_ops  # noqa: F401
    op = torch.ops.centerclip
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    base = (torch.randn(rows, cols, generator=g) * 3.0 + 20.0).to(dev)          # logits of unit rows at exp(logit_scale) ~ 100
    work = base.clone()

    def ours():
        m, s = op.dsl_col_stats(work)
        op.dsl_apply_(work, m, s, rows)

    def eager():
        return base * torch.softmax(base, dim=0) * len(base)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps * 1e3                                    # us per call
    for fn in (ours, eager):                                                     # warm-up: code objects, workspaces, allocator
        for _ in range(5):
            fn()
    work.copy_(base)
    ours()
    err = float((work - eager()).abs().max() / eager().abs().max())
    t_ours, t_eager = [], []
    for _ in range(windows):
        work.copy_(base)                                                         # (repeated rewrites of one buffer drift to inf / NaN; the time does not depend on the values)
        t_ours.append(window(ours))
        t_eager.append(window(eager))
    mo, me = _stat(t_ours), _stat(t_eager)
    nbytes = 3 * rows * cols * 4
    print("EVAL %d x %d, windows of %d calls, %d windows alternating (device events)" % (rows, cols, reps, windows))
    print("EVAL cc_dsl_col_stats_f32 + cc_dsl_apply_f32: %.1f us (min %.1f max %.1f) = %.2f TB/s over %.0f MB"
          % (mo[0], mo[1], mo[2], nbytes / mo[0] / 1e6, nbytes / 1e6))
    print("EVAL eager torch sim * softmax(sim, 0) * len(sim): %.1f us (min %.1f max %.1f)" % me)
    print("EVAL ratio eager / kernels = %.2f; max |difference| / max |D| = %.1e" % (me[0] / mo[0], err))


def train_child(flag, windows=7, reps=10):
    """One process: the captured step of the tree this file's --tree names."""
    import torch
    from argparse import Namespace
    import bench
    from centerclip_amd.clip4clip import CLIP4Clip
    from centerclip_amd.train import AdamW, GraphedTrainStep, lr_scheduler, prep_optim_params_groups
    sys.path.insert(0, os.path.join(os.getcwd(), "examples"))
    from eval_synthetic import SyntheticRetrieval
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    c = bench.CFG2
    args = bench.task_config(c)
    if flag:
        args.camoe_dsl = 1
    model = CLIP4Clip.from_state_dict(bench.random_state_dict(c, seed=0), args).float().to(dev)
    targs = Namespace(lr=1e-7, wd=0.2, new_added_modules=["Cross", "cluster_embed"], gradient_accumulation_steps=1,
                      clip_grad_norm=1.0, optim="AdamW")
    opt = AdamW(prep_optim_params_groups(targs, model, coef_lr=1e-3), lr=targs.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2,
                capturable=True)
    sched = lr_scheduler('cos', init_lr=targs.lr, all_iters=1000, slow_start_iters=100, weight_decay=0.2)
    stepper = GraphedTrainStep(model, opt, scheduler=sched, clip_grad_norm=1.0)
    batch = next(iter(torch.utils.data.DataLoader(SyntheticRetrieval(16), batch_size=16, shuffle=False)))
    for _ in range(4):
        loss = stepper(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        t0 = time.time()
        for _ in range(reps):
            loss = stepper(batch)
        torch.cuda.synchronize()
        ts.append((time.time() - t0) / reps * 1e3)
    med, lo, hi = _stat(ts)
    print("median %.3f ms min %.3f max %.3f loss %.4f windows %s" % (med, lo, hi, float(loss), ["%.3f" % t for t in ts]), flush=True)


def train_times(parent, rounds):
    variants = [("this camoe_dsl=1", ROOT, 1), ("this camoe_dsl=0", ROOT, 0)]
    if parent:
        variants.append(("parent", os.path.abspath(parent), 0))
    print("TRAIN captured cfg-2 step, batch 16: one fresh process per line, %d rounds, variants alternating" % rounds)
    for _ in range(rounds):
        for name, tree, flag in variants:
            env = dict(os.environ, PYTHONPATH=tree)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "train-child", "--flag", str(flag)], cwd=tree, env=env,
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:                           # stop: nothing more is started on the device after a failure
                print("STEP %s FAILED (%d)\n%s" % (name, r.returncode, r.stderr[-2000:]))
                sys.exit(1)
            print("STEP %s %s" % (name, r.stdout.strip().splitlines()[-1]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["eval", "train", "train-child"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flag", type=int, default=0)
    a = ap.parse_args()
    if a.what == "eval":
        eval_times()
    elif a.what == "train":
        train_times(a.parent, a.rounds)
    else:
        train_child(a.flag)
