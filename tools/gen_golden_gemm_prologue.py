"""Fixture tests/golden/gemm_rows_prologue.npz for tests/test_gemm_prologue_gpu.py: the outputs of the few-rows kernel
(cc_linear_rows_pair_f16: LayerNorm-folded QuickGELU and residual + statistics with a centring shift, rows by row_map and by
row_step, M = 1, 16, 48, 64, 65) as bit patterns, whole output buffers with their sentinel rows.  The problems are the ones
the test builds (rows_case there, seeded numpy streams); run this on the commit whose outputs are to be kept - the library
that computes them is the one the package loads (CENTERCLIP_HIP_LIB names another build).  Needs a GPU.

    python tools/gen_golden_gemm_prologue.py [out.npz]
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    spec = importlib.util.spec_from_file_location("test_gemm_prologue_gpu", os.path.join(ROOT, "tests", "test_gemm_prologue_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path, n = mod.write_golden(*sys.argv[1:2])
    print("wrote", path, n, "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
