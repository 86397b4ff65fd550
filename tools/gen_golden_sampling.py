"""Fixture tests/golden/sampling_golden.npz for tests/test_collate_host.py, recorded from the reference (dev container only: it
loads the reference's dataloaders/sampling.py by path; the module needs NumPy alone).

For every (clip_length, num_frames) in CASES:
  uniform/<c>_<n>_<twice>                 uniform_sampling(c, n, twice_sample=bool(twice))
  segments/<c>_<n>_<shift>_<seed>         multi_segments_sampling(c, n, random_shift=bool(shift)) after numpy.random.seed(seed)
and with data_length=2 for DATA2 and data_length=3 for DATA3 (num_frames = clip_length + 1 with three frames per offset: the
one place where the reference's np.random.choice branch is reached - (n - d + 1) // c == 0 and n > c need d >= 3):
  uniform2/<c>_<n>_<twice>, segments2/<c>_<n>_<shift>_<seed>, uniform3/..., segments3/...

Only these index arrays are committed.

    python tools/gen_golden_sampling.py [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "sampling_golden.npz")

CASES = ((12, 300), (12, 24), (12, 17), (12, 13), (12, 12), (12, 5), (12, 1), (4, 9))      # (clip_length, num_frames)
DATA2 = ((4, 5), (4, 6))
DATA3 = ((4, 5),)
SEEDS = (0, 1, 2, 3, 4)


def load(reference):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_sampling", os.path.join(reference, "dataloaders", "sampling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(rs):
    out = {}
    for tag, cases, kw in (("", CASES, {}), ("2", DATA2, dict(data_length=2)), ("3", DATA3, dict(data_length=3))):
        for c, n in cases:
            for twice in (0, 1):
                out["uniform%s/%d_%d_%d" % (tag, c, n, twice)] = np.asarray(rs.uniform_sampling(c, n, twice_sample=bool(twice), **kw))
            for shift in (0, 1):
                for seed in SEEDS:
                    np.random.seed(seed)
                    out["segments%s/%d_%d_%d_%d" % (tag, c, n, shift, seed)] = np.asarray(
                        rs.multi_segments_sampling(c, n, random_shift=bool(shift), **kw))
    return {k: v.astype(np.int64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference's checkout (default: where oracle/ looks for it)")
    a = ap.parse_args()
    if a.reference is None:
        from oracle.gen_golden_clip import REF
        a.reference = REF
    out = record(load(a.reference))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
