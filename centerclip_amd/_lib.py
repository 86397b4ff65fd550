"""ctypes binding of libcenterclip_hip.so (C ABI: include/centerclip_hip.h).

The HIP library IS the product path: there is no CPU or eager-PyTorch fallback.  If the
shared library is missing or a tensor is not on a ROCm device, calls fail loudly.
"""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libcenterclip_hip.so")

CC_OK = 0
METRIC_IDS = {"euclidean": 0, "cosine": 1}


class CenterClipHipError(RuntimeError):
    pass


class TokenLayout(ctypes.Structure):
    """struct cc_token_layout"""
    _fields_ = [("B", ctypes.c_int32), ("S", ctypes.c_int32), ("fd", ctypes.c_int32), ("n", ctypes.c_int32),
                ("stride_b", ctypes.c_int64), ("stride_s", ctypes.c_int64),
                ("stride_f", ctypes.c_int64), ("stride_i", ctypes.c_int64)]


class Yuv420Layout(ctypes.Structure):
    """struct cc_yuv420_layout: byte offsets of an 8-bit 4:2:0 source - Y(y, x) at y * y_pitch + x, Cb(cy, cx) at u_offset +
    cy * c_pitch + cx * c_step, Cr the same from v_offset, frame f at f * frame_stride; matrix 0 BT.601 / 1 BT.709, range 0 limited /
    1 full."""
    _fields_ = [("frame_stride", ctypes.c_int64), ("y_pitch", ctypes.c_int64), ("u_offset", ctypes.c_int64),
                ("v_offset", ctypes.c_int64), ("c_pitch", ctypes.c_int64), ("c_step", ctypes.c_int32),
                ("matrix", ctypes.c_int32), ("range", ctypes.c_int32)]


class YuvLayout(ctypes.Structure):
    """struct cc_yuv_layout: the general descriptor - the five byte positions of cc_yuv420_layout, then c_step (bytes between two
    samples of one chroma plane in a row), sub_x / sub_y (log2 of the chroma subsampling, 0 or 1), depth (8, 10, 12, 16), shift
    (a sample is word >> shift), matrix, range."""
    _fields_ = [("frame_stride", ctypes.c_int64), ("y_pitch", ctypes.c_int64), ("u_offset", ctypes.c_int64),
                ("v_offset", ctypes.c_int64), ("c_pitch", ctypes.c_int64), ("c_step", ctypes.c_int32),
                ("sub_x", ctypes.c_int32), ("sub_y", ctypes.c_int32), ("depth", ctypes.c_int32), ("shift", ctypes.c_int32),
                ("matrix", ctypes.c_int32), ("range", ctypes.c_int32)]


_lib = None


class ClusterVariant(ctypes.Structure):
    """cc_cluster_variant (include/centerclip_hip.h): algorithm 0 kmedoids / 1 pooling / 2 sparse_sampling / 3 spectral /
    4 temporal_shift / 5 token_shift, aggregation 0 medoid / 1 mean."""
    _fields_ = [("algorithm", ctypes.c_int32), ("aggregation", ctypes.c_int32), ("cluster_embed", ctypes.c_void_p),
                ("cls_multiplier", ctypes.c_void_p), ("fixed_ids", ctypes.c_void_p),
                ("spectral_sigma", ctypes.c_float), ("spectral_graph_mode", ctypes.c_int32),
                ("spectral_knn_k", ctypes.c_int32), ("spectral_correct_sign", ctypes.c_int32),
                ("spectral_graph", ctypes.c_void_p), ("mean_residual", ctypes.c_int32),
                ("shift_fold_div", ctypes.c_int32), ("shift_segment", ctypes.c_int32)]


class LinearProblem(ctypes.Structure):
    """cc_linear_problem (include/centerclip_hip.h): one problem of cc_linear_pair_f16 / cc_linear_rows_pair_f16 /
    cc_inproj_attention_pair_f16; the layout is checked against cc_linear_problem_size()."""
    _fields_ = [("a", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("c", ctypes.c_void_p),
                ("resid", ctypes.c_void_p), ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("ldc", ctypes.c_int32), ("ln_stats", ctypes.c_void_p), ("ln_slots", ctypes.c_int32),
                ("ln_c1", ctypes.c_void_p), ("ln_eps", ctypes.c_float), ("stats_out", ctypes.c_void_p),
                ("c16", ctypes.c_void_p), ("shift_in", ctypes.c_void_p), ("shift_stats", ctypes.c_void_p),
                ("shift_slots", ctypes.c_int32), ("shift_out", ctypes.c_void_p), ("m_dev", ctypes.c_void_p),
                ("row_step", ctypes.c_int32), ("row_map", ctypes.c_void_p), ("pos", ctypes.c_void_p),
                ("patch_n", ctypes.c_int32), ("att_L", ctypes.c_int32), ("att_nseq", ctypes.c_int32),
                ("att_causal", ctypes.c_int32), ("att_seq_off", ctypes.c_void_p), ("att_seq_len", ctypes.c_void_p)]


def _declare(lib):
    c = ctypes
    vp, i32, i64, f32, sz = c.c_void_p, c.c_int32, c.c_int64, c.c_float, c.c_size_t
    lay = c.POINTER(TokenLayout)
    lib.cc_version.restype = c.c_char_p
    lib.cc_status_string.restype = c.c_char_p
    lib.cc_status_string.argtypes = [c.c_int]
    lib.cc_cluster_workspace_bytes.restype = sz
    lib.cc_cluster_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.cc_token_norms_f32.argtypes = [vp, lay, i32, vp, vp, sz, vp]
    lib.cc_pairwise_distance_f32.argtypes = [vp, lay, i32, i32, f32, i32, i32, i32, vp, vp, vp, sz, vp]
    lib.cc_pairwise_distance_cross_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, i32, i32, vp, vp, sz, vp]
    lib.cc_pairwise_distance_cross_f32.restype = c.c_int
    lib.cc_kmedoids_from_dist_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.cc_batch_kmedoids_f32.argtypes = [vp, lay, i32, i32, i32, f32, f32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.cc_token_cluster_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, f32, f32, i32, i32, i32,
                                         vp, i64, i64, vp, vp, vp, vp, sz, vp]
    lib.cc_token_cluster_variant_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, f32, f32, i32, i32, i32,
                                                 c.POINTER(ClusterVariant), vp, i64, i64, vp, vp, vp, vp, sz, vp]
    lib.cc_token_aggregate_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, vp, c.POINTER(ClusterVariant), vp,
                                           i64, i64, vp]
    lib.cc_token_apply_selection_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, c.POINTER(ClusterVariant), vp, vp,
                                                 vp, i64, i64, vp]
    lib.cc_token_apply_selection_f32.restype = c.c_int
    lib.cc_token_cluster_backward_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, c.POINTER(ClusterVariant), vp, vp,
                                                  vp, i64, i64, vp, i64, i64, vp, vp, vp]
    lib.cc_token_cluster_backward_f32.restype = c.c_int
    lib.cc_token_shift_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp, i64, i64, vp]
    lib.cc_token_shift_f32.restype = c.c_int
    lib.cc_token_shift_rows_f32.argtypes = [vp, i64, i64, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    lib.cc_token_shift_rows_f32.restype = c.c_int
    lib.cc_token_shift_rows_lds_bytes.argtypes = [i32, i32, i32]
    lib.cc_token_shift_rows_lds_bytes.restype = sz
    lib.cc_spectral_laplacian_f32.argtypes = [vp, lay, i32, f32, vp, vp, vp, vp, vp, sz, vp]
    lib.cc_svd_sign_flip_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.cc_spectral_graph_laplacian_f32.argtypes = [vp, lay, i32, f32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.cc_spectral_graph_laplacian_f32.restype = c.c_int
    lib.cc_spectral_embedding_workspace_bytes.argtypes = [i32, i32]
    lib.cc_spectral_embedding_workspace_bytes.restype = sz
    lib.cc_spectral_workspace_bytes.argtypes = [i32, i32, i32]
    lib.cc_spectral_workspace_bytes.restype = sz
    lib.cc_spectral_embedding_f32.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, sz, vp]
    lib.cc_spectral_embedding_solver_f32.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp, sz, vp]
    lib.cc_spectral_embedding_solver_f32.restype = c.c_int
    lib.cc_spectral_embedding_f32.restype = c.c_int
    lib.cc_spectral_laplacian_f32.restype = c.c_int
    lib.cc_svd_sign_flip_f32.restype = c.c_int
    prob = c.POINTER(LinearProblem)
    lib.cc_linear_problem_size.argtypes = []
    lib.cc_linear_problem_size.restype = sz
    lib.cc_linear_pair_f16.argtypes = [prob, prob, i32, i32, c.POINTER(i32), vp]
    lib.cc_linear_pair_f16.restype = c.c_int
    lib.cc_linear_rows_pair_f16.argtypes = [prob, prob, i32, c.POINTER(i32), vp]
    lib.cc_linear_rows_pair_f16.restype = c.c_int
    lib.cc_inproj_attention_pair_f16.argtypes = [prob, prob, vp]
    lib.cc_inproj_attention_pair_f16.restype = c.c_int
    lib.cc_similarity_topk_slices.argtypes = [i32, i32, i32]
    lib.cc_similarity_topk_slices.restype = i32
    lib.cc_similarity_topk_workspace_bytes.argtypes = [i32, i32, i32]
    lib.cc_similarity_topk_workspace_bytes.restype = sz
    lib.cc_similarity_topk_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, vp, vp, sz, vp]
    lib.cc_similarity_topk_planes_f32.restype = c.c_int
    lib.cc_dsl_col_stats_planes_slices.argtypes = [i32]
    lib.cc_dsl_col_stats_planes_slices.restype = i32
    lib.cc_dsl_col_stats_planes_workspace_bytes.argtypes = [i32, i32]
    lib.cc_dsl_col_stats_planes_workspace_bytes.restype = sz
    lib.cc_dsl_col_stats_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, sz, vp]
    lib.cc_dsl_col_stats_planes_f32.restype = c.c_int
    lib.cc_similarity_topk_dsl_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, vp, i32, i32, vp, vp, vp, sz, vp]
    lib.cc_similarity_topk_dsl_planes_f32.restype = c.c_int
    lib.cc_similarity_topk_grouped_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.cc_similarity_topk_grouped_planes_f32.restype = c.c_int
    lib.cc_similarity_topk_grouped_dsl_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp,
                                                              sz, vp]
    lib.cc_similarity_topk_grouped_dsl_planes_f32.restype = c.c_int
    lib.cc_similarity_topk_masked_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, i32, i32, vp, vp, i32, i32, vp,
                                                         vp, vp, vp, sz, vp]
    lib.cc_similarity_topk_masked_planes_f32.restype = c.c_int
    lib.cc_similarity_topk_deep_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.cc_similarity_topk_deep_workspace_bytes.restype = sz
    lib.cc_similarity_topk_deep_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, i32, i32, vp, vp, i32, i32, vp, vp,
                                                       vp, vp, vp, vp, sz, vp]
    lib.cc_similarity_topk_deep_planes_f32.restype = c.c_int
    lib.cc_dsl_col_stats_planes_masked_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, vp, sz, vp]
    lib.cc_dsl_col_stats_planes_masked_f32.restype = c.c_int
    lib.cc_pack_row_mask_u8.argtypes = [vp, i32, i32, vp, i32, vp]
    lib.cc_pack_row_mask_u8.restype = c.c_int
    lib.cc_similarity_rank_workspace_bytes.argtypes = [i32, i32]
    lib.cc_similarity_rank_workspace_bytes.restype = sz
    lib.cc_similarity_rank_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp,
                                                  vp, sz, vp]
    lib.cc_similarity_rank_planes_f32.restype = c.c_int
    lib.cc_topk_merge_lists_f32.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.cc_topk_merge_lists_f32.restype = c.c_int
    lib.cc_similarity_target_score_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp,
                                                          vp]
    lib.cc_similarity_target_score_planes_f32.restype = c.c_int
    lib.cc_similarity_count_workspace_bytes.argtypes = [i32, i32]
    lib.cc_similarity_count_workspace_bytes.restype = sz
    lib.cc_similarity_count_planes_f32.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp,
                                                   sz, vp]
    lib.cc_similarity_count_planes_f32.restype = c.c_int
    for name in ("cc_token_norms_f32", "cc_pairwise_distance_f32", "cc_kmedoids_from_dist_f32",
                 "cc_batch_kmedoids_f32", "cc_token_cluster_f32", "cc_token_cluster_variant_f32",
                 "cc_token_aggregate_f32"):
        getattr(lib, name).restype = c.c_int
    return lib


def _declare_optional(lib):
    """Entry points added by later translation units (transformer / similarity kernels)."""
    try:
        from . import _lib_clip
        _lib_clip.declare(lib)
    except ImportError:
        pass


def lib():
    """Load the shared library once; raise if it has not been built (python -m centerclip_amd.build)."""
    global _lib
    if _lib is None:
        path = os.environ.get("CENTERCLIP_HIP_LIB", LIB_PATH)    # dev aid: A/B two builds in one GPU session
        if not os.path.exists(path):
            raise CenterClipHipError(
                "libcenterclip_hip.so not found at %s - build it with `python -m centerclip_amd.build` "
                "(the HIP library is the only execution path; there is no CPU fallback)" % path)
        handle = ctypes.CDLL(path)
        _declare(handle)
        _declare_optional(handle)
        _lib = handle
    return _lib


def check(status, what):
    if status != CC_OK:
        raise CenterClipHipError("%s failed: %s (%d)" % (what, lib().cc_status_string(status).decode(), status))


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CenterClipHipError("centerclip_amd runs on MI355X only: got a %s tensor (no CPU fallback)" % t.device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_workspaces = {}
_retired = []      # outgrown workspaces stay allocated: a hipGraph captured earlier may still hold their addresses


def workspace(nbytes, device):
    """Caller-owned scratch for the C ABI: one growing uint8 buffer per (device, stream).  A buffer that is outgrown is
    retired, never freed - a captured hipGraph replays with the addresses it was captured with, and the caching
    allocator must not hand that memory to another tensor (growth is geometric, so the retired total stays below the
    live buffer's size)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired.append(buf)
        grow = 0 if buf is None else buf.numel() * 3 // 2
        buf = torch.empty(max(int(nbytes), grow, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf
