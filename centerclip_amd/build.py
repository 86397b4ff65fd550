"""Build libcenterclip_hip.so in-tree with hipcc for gfx950 (no torch extension machinery:
the product boundary is a plain C ABI, include/centerclip_hip.h).

    python -m centerclip_amd.build [--force]
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "lib", "libcenterclip_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"] + os.environ.get("CC_EXTRA_FLAGS", "").split()      # e.g. -DCC_DEV_KNOBS for A/B builds
# the cluster / similarity paths promise IEEE single operations in source order (no fma contraction); preprocess.hip the same
# for the double operations of its host-side coefficient tables, augment.hip for the fp32 weights and sums its error bound counts
STRICT = {"cluster.hip": ["-ffp-contract=off"], "similarity.hip": ["-ffp-contract=off"], "dsl.hip": ["-ffp-contract=off"],
          "preprocess.hip": ["-ffp-contract=off"], "search.hip": ["-ffp-contract=off"], "augment.hip": ["-ffp-contract=off"]}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(PKG, "..", "include", "centerclip_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not _stale():
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    objs = []
    procs = []
    for src in sources():
        obj = os.path.join(PKG, "lib", os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        cmd = [HIPCC] + FLAGS + STRICT.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
