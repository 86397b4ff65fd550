"""CPU-only: the host decisions of the token-cluster entries (csrc/cluster.hip) that need no device - the workspace sizes
over a table, against values recorded from the library before its host path was restructured
(tests/golden/cluster_host_ws.json, tools/gen_golden_cluster_host.py), and the status of every early return that precedes
the first HIP call.  No case here reaches a launch: each one fails a check in front of it."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_host_ws.json")

PS, NS, WS, KS = (1, 48, 64), (8, 196, 197, 202, 392, 784, 833, 1568), (16, 768), (1, 49, 160)
SIM_SHAPES = ((1, 1, 512), (16, 16, 512), (128, 1000, 512), (33, 7, 768))          # (Bt, Bv, E)
DSL_SHAPES = ((1, 1), (16, 16), (128, 1000), (1000, 33))                           # (rows, cols)
CTR_SHAPES = ((1, 1, 512), (16, 12, 512), (128, 3, 512), (33, 7, 768))             # (n, Tn, E)


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import build
    build.build(verbose=False)
    from centerclip_amd import _lib as L
    return L.lib()


def workspace_table(lib):
    """The values the golden file records, as {name: {key: bytes}}; shared with tools/gen_golden_cluster_host.py."""
    t = {"cluster": {}, "spectral": {}, "embedding": {}, "similarity": {}, "dsl_col_stats": {}, "contrastive_grad": {},
         "contrastive_grad_dsl": {}}
    for P in PS:
        for N in NS:
            t["embedding"]["%d,%d" % (P, N)] = lib.cc_spectral_embedding_workspace_bytes(P, N)
            for W in WS:
                for pre in (0, 1):
                    t["cluster"]["%d,%d,%d,%d" % (P, N, W, pre)] = lib.cc_cluster_workspace_bytes(P, N, W, pre)
            for K in KS:
                t["spectral"]["%d,%d,%d" % (P, N, K)] = lib.cc_spectral_workspace_bytes(P, N, K)
    for s in SIM_SHAPES:
        t["similarity"]["%d,%d,%d" % s] = lib.cc_similarity_workspace_bytes(*s)
    for s in DSL_SHAPES:
        t["dsl_col_stats"]["%d,%d" % s] = lib.cc_dsl_col_stats_workspace_bytes(*s)
    for s in CTR_SHAPES:                         # what the two workspace carvers of similarity.hip size
        t["contrastive_grad"]["%d,%d,%d" % s] = lib.cc_contrastive_grad_workspace_bytes(*s)
        t["contrastive_grad_dsl"]["%d,%d,%d" % s] = lib.cc_contrastive_grad_dsl_workspace_bytes(*s)
    return t


def test_workspace_sizes_match_the_recorded_table(lib):
    want = json.load(open(GOLDEN))
    got = workspace_table(lib)
    assert sorted(got) == sorted(want)
    assert len(want["cluster"]) == 96 and len(want["spectral"]) == 72 and len(want["embedding"]) == 24
    for name in want:
        assert got[name] == want[name], name
    assert all(v > 0 for v in want["cluster"].values())


# ---- early returns.  Pointers that are only tested against NULL point into this host buffer; nothing dereferences them.
_BUF = (ctypes.c_char * 4096)()
PTR = ctypes.c_void_p(ctypes.addressof(_BUF))
NAN = float("nan")


def _lay(N=8, W=16):
    from centerclip_amd import _lib as L
    return ctypes.byref(L.TokenLayout(1, 1, 1, N, N * W, 0, 0, W))


def _var(algorithm=0, aggregation=0, fixed_ids=None):
    from centerclip_amd import _lib as L
    v = L.ClusterVariant()
    v.algorithm, v.aggregation, v.fixed_ids = algorithm, aggregation, fixed_ids
    v.spectral_sigma = 1.0
    return ctypes.byref(v)


def _kmedoids(lib, x=PTR, N=8, K=2, metric=0, p=2.0, thr=1e-6, ws=None):
    return lib.cc_batch_kmedoids_f32(x, _lay(N), 16, K, metric, p, thr, 10, 1, 1, 0, PTR, None, None, ws, 0, None)


def _pairwise(lib, metric=0, p=2.0):
    return lib.cc_pairwise_distance_f32(PTR, _lay(), 16, metric, p, 0, 0, 0, PTR, None, None, 0, None)


def _cross(lib, N1=8, N2=8, p=2.0, all_negative=0, self_nearest=0):
    return lib.cc_pairwise_distance_cross_f32(PTR, PTR, 1, N1, N2, 16, 0, p, all_negative, self_nearest, PTR, None, 0, None)


# token ops: B = 1, T frames of 1 + n = 9 tokens, W floats each, frame-major
def _gather(lib, T=4, T_new=2, W=16, in_tok=None):
    return lib.cc_token_gather_f32(PTR, W if in_tok is None else in_tok, 9 * W, 1, T, T_new, 8, W, 3, PTR, PTR, W, 4 * W, None)


def _apply(lib, aggregation, medoids, assign):
    return lib.cc_token_apply_selection_f32(PTR, 16, 9 * 16, 1, 4, 2, 8, 16, 3, _var(0, aggregation), medoids, assign, PTR,
                                            16, 4 * 16, None)


def _variant(lib, var, K=3, ws=None, ws_bytes=0):
    return lib.cc_token_cluster_variant_f32(PTR, 16, 9 * 16, 1, 4, 2, 8, 16, K, 0, 2.0, 1e-6, 10, 1, 0, var, PTR, 16,
                                            (1 + K) * 16, None, None, None, ws, ws_bytes, None)


def _backward(lib, var, K=3, medoids=PTR, assign=None, x=PTR, g_mult=None):
    return lib.cc_token_cluster_backward_f32(PTR, 16, (1 + K) * 16, 1, 4, 2, 8, 16, K, var, medoids, assign, x, 16, 9 * 16, PTR,
                                             16, 9 * 16, None, g_mult, None)


def _laplacian(lib, sigma=1.0, mode=0, knn_k=0):
    return lib.cc_spectral_graph_laplacian_f32(PTR, _lay(), 16, sigma, mode, knn_k, 0, None, PTR, None, None, None, 0, None)


def _solver(lib, N=16, K=4, ldq=4, solver=0):
    return lib.cc_spectral_embedding_solver_f32(PTR, 1, N, K, 0, PTR, ldq, None, None, solver, None, 0, None)


EARLY_RETURNS = [
    ("kmedoids: NaN threshold", lambda l: _kmedoids(l, thr=NAN), -1),
    ("kmedoids: x null", lambda l: _kmedoids(l, x=None), -1),
    ("kmedoids: K > N", lambda l: _kmedoids(l, K=9), -1),
    ("kmedoids: metric 2", lambda l: _kmedoids(l, metric=2), -2),
    ("kmedoids: euclidean, norm_p 0", lambda l: _kmedoids(l, p=0.0), -2),
    ("kmedoids: N = 8192", lambda l: _kmedoids(l, N=8192), -2),
    ("kmedoids: ws null", lambda l: _kmedoids(l), -3),
    # the order of the checks: NaN threshold in front of everything, K in front of the metric, the metric in front of ws
    ("kmedoids: NaN threshold and x null", lambda l: _kmedoids(l, thr=NAN, x=None), -1),
    ("kmedoids: K > N and metric 2", lambda l: _kmedoids(l, K=9, metric=2), -1),
    ("kmedoids: N = 8192, metric 2, ws null", lambda l: _kmedoids(l, N=8192, metric=2), -2),
    ("from_dist: N = 8192", lambda l: l.cc_kmedoids_from_dist_f32(PTR, PTR, 1, 8192, 2, 10, 1, PTR, None, None, None, 0, None), -2),
    ("from_dist: K > N", lambda l: l.cc_kmedoids_from_dist_f32(PTR, PTR, 1, 8, 9, 10, 1, PTR, None, None, None, 0, None), -1),
    ("pairwise: metric 2", lambda l: _pairwise(l, metric=2), -2),
    ("pairwise: euclidean, p 0", lambda l: _pairwise(l, p=0.0), -2),
    ("pairwise: ws null", lambda l: _pairwise(l), -3),
    ("cross: p 0", lambda l: _cross(l, p=0.0), -1),
    ("cross: self_nearest, N2 > N1", lambda l: _cross(l, N1=4, N2=8, self_nearest=1), -1),
    ("cross: all_negative, ws null", lambda l: _cross(l, all_negative=1), -3),
    ("gather: T 3, T_new 2", lambda l: _gather(l, T=3), -1),
    ("gather: W 30", lambda l: _gather(l, W=30), -1),
    ("gather: a stride of 6", lambda l: _gather(l, in_tok=6), -1),
    ("apply_selection: mean without assign", lambda l: _apply(l, 1, PTR, None), -1),
    ("apply_selection: medoid without medoids", lambda l: _apply(l, 0, None, PTR), -1),
    ("variant: var null", lambda l: _variant(l, None), -1),
    ("variant: algorithm 4", lambda l: _variant(l, _var(4)), -1),
    ("variant: algorithm 5", lambda l: _variant(l, _var(5)), -1),
    ("variant: algorithm 7", lambda l: _variant(l, _var(7)), -1),
    ("variant: aggregation 2", lambda l: _variant(l, _var(0, 2)), -1),
    ("variant: K > N", lambda l: _variant(l, _var(0), K=17), -1),
    ("variant: sparse sampling without fixed_ids", lambda l: _variant(l, _var(2)), -1),
    ("variant: k-medoids, ws null", lambda l: _variant(l, _var(0)), -3),
    ("variant: K > N in front of ws null", lambda l: _variant(l, _var(3), K=17), -1),
    ("variant: spectral, ws_bytes = the k-medoids size only",
     lambda l: _variant(l, _var(3), ws=PTR, ws_bytes=l.cc_cluster_workspace_bytes(2, 16, 16, 0)), -3),
    ("backward: algorithm 3", lambda l: _backward(l, _var(3)), -2),
    ("backward: pooling, K != n", lambda l: _backward(l, _var(1)), -1),
    ("backward: sparse sampling without fixed_ids", lambda l: _backward(l, _var(2)), -1),
    ("backward: mean without assign", lambda l: _backward(l, _var(0, 1)), -1),
    ("backward: grad_cls_mult without x", lambda l: _backward(l, _var(0), x=None, g_mult=PTR), -1),
    ("laplacian: sigma 0", lambda l: _laplacian(l, sigma=0.0), -1),
    ("laplacian: mode 2", lambda l: _laplacian(l, mode=2), -2),
    ("laplacian: KNN, knn_k 0", lambda l: _laplacian(l, mode=1), -1),
    ("laplacian: ws null", lambda l: _laplacian(l), -3),
    ("solver: solver 2", lambda l: _solver(l, solver=2), -1),
    ("solver: ldq < K", lambda l: _solver(l, ldq=3), -1),
    ("solver: N 700, CC_EIG_JACOBI", lambda l: _solver(l, N=700, solver=1), -2),
    ("solver: N 900, auto", lambda l: _solver(l, N=900), -2),
]


@pytest.mark.parametrize("what,call,want", EARLY_RETURNS, ids=[c[0] for c in EARLY_RETURNS])
def test_early_return_status(lib, what, call, want):
    assert call(lib) == want, what
