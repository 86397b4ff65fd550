"""``torch.library`` registration of the C-ABI entry points (namespace ``centerclip``): the boundary the north star
names - "called from Python via PyTorch-ROCm custom ops that keep the modules/clip.py and modules/clip4clip.py forward
signatures" (SURVEY.md §8b).  Every op

  * has a schema in the dispatcher (``torch.ops.centerclip.<name>``), so it is visible to torch.compile / export /
    profilers like any ATen op;
  * has a CUDA(=ROCm) implementation that only enqueues kernels of libcenterclip_hip.so on the current stream through
    the ctypes binding (no CPU implementation is registered: a CPU tensor fails in the dispatcher, loudly);
  * has a fake (meta) kernel giving output shapes / dtypes without touching the device.

The module mirrors (clip.py, clip4clip.py, cluster/*, metrics.py) and ops.py call these ops; nothing else in the package
calls the ctypes layer for compute.  The encoders take their weights through an integer *model handle*
(``register_model``): the C structs hold raw device pointers, which a dispatcher schema cannot carry.
"""
import ctypes
import math
from typing import List, Optional, Tuple

import torch
from torch.library import custom_op

from . import _lib as L
from ._lib_clip import EPI

NS = "centerclip"
LN_MAX_SLOTS = 32

# ------------------------------------------------------------------------------------------ model handles
_MODELS = {}
_next_handle = [1]


def register_model(struct, meta, keep):
    """Park a packed cc_vit_model / cc_text_model (+ the tensors its pointers refer to) -> int handle."""
    h = _next_handle[0]
    _next_handle[0] += 1
    _MODELS[h] = (struct, meta, keep)
    return h


def release_model(handle):
    _MODELS.pop(handle, None)


def _model(handle):
    try:
        return _MODELS[handle]
    except KeyError:
        raise L.CenterClipHipError("unknown centerclip model handle %r" % (handle,))


def _st(t):
    return L.stream_ptr(t.device)


def _e(*shape, like, dtype):
    return torch.empty(shape, device=like.device, dtype=dtype)


# ------------------------------------------------------------------------------------------ Linear / LN / attention
@custom_op(NS + "::linear_f16", mutates_args=(), device_types="cuda")
def linear_f16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epilogue: str, tile: int) -> torch.Tensor:
    M, K = a.shape
    N = w.shape[0]
    out = _e(M, N, like=a, dtype=torch.float16 if epilogue.startswith("f16") else torch.float32)
    L.check(L.lib().cc_linear_f16(L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(out), M, N, K, N, EPI[epilogue], tile, _st(a)),
            "cc_linear_f16")
    return out


@linear_f16.register_fake
def _(a, w, bias, epilogue, tile):
    return a.new_empty((a.shape[0], w.shape[0]), dtype=torch.float16 if epilogue.startswith("f16") else torch.float32)


@custom_op(NS + "::linear_f16_out", mutates_args=("out",), device_types="cuda")
def linear_f16_out(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epilogue: str,
                   tile: int) -> None:
    """epilogue 'f32_resid': out += a w^T + b in place; the other epilogues overwrite ``out`` (row stride honoured)."""
    M, K = a.shape
    L.check(L.lib().cc_linear_f16(L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(out), M, w.shape[0], K, out.stride(0),
                                  EPI[epilogue], tile, _st(a)), "cc_linear_f16")


@linear_f16_out.register_fake
def _(a, w, bias, out, epilogue, tile):
    return None


@custom_op(NS + "::layernorm", mutates_args=(), device_types="cuda")
def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, out_f16: bool) -> torch.Tensor:
    W = x.shape[-1]
    rows = x.numel() // W
    out = torch.empty(x.shape, device=x.device, dtype=torch.float16 if out_f16 else torch.float32)
    L.check(L.lib().cc_layernorm_f32(L.ptr(x), W, L.ptr(weight), L.ptr(bias), L.ptr(out), W, rows, W, float(eps),
                                     int(out_f16), _st(x)), "cc_layernorm_f32")
    return out


@layernorm.register_fake
def _(x, weight, bias, eps, out_f16):
    return x.new_empty(x.shape, dtype=torch.float16 if out_f16 else torch.float32)


@custom_op(NS + "::attention_f16", mutates_args=(), device_types="cuda")
def attention_f16(qkv: torch.Tensor, nseq: int, L_tok: int, heads: int, causal: bool, seq_rows: int,
                  tok_rows: int) -> torch.Tensor:
    W = qkv.shape[1] // 3
    out = _e(nseq * L_tok, W, like=qkv, dtype=torch.float16)
    L.check(L.lib().cc_attention_strided_f16(L.ptr(qkv), L.ptr(out), nseq, L_tok, heads, W, int(causal), seq_rows, tok_rows,
                                             _st(qkv)), "cc_attention_strided_f16")
    return out


@attention_f16.register_fake
def _(qkv, nseq, L_tok, heads, causal, seq_rows, tok_rows):
    return qkv.new_empty((nseq * L_tok, qkv.shape[1] // 3))


# ------------------------------------------------------------------------------------------ sim_header 'seqTransf'
def _mask_i64(mask):
    if mask.dtype != torch.long or mask.dim() != 2:
        raise ValueError("the key mask must be an int64 [nseq, L] tensor (any strides)")
    return mask


@custom_op(NS + "::key_masked_attention", mutates_args=(), device_types="cuda")
def key_masked_attention(qkv: torch.Tensor, mask: torch.Tensor, nseq: int, L_tok: int, heads: int) -> torch.Tensor:
    """softmax(q k^T / 8 + (1 - mask[key]) * -1e6) v per head (module_cross.py:102-104) of frame-major qkv [nseq * L, 3W] fp16;
    mask [nseq, L] int64, any strides -> [nseq * L, W] fp16."""
    W = qkv.shape[1] // 3
    _mask_i64(mask)
    out = _e(nseq * L_tok, W, like=qkv, dtype=torch.float16)
    L.check(L.lib().cc_key_masked_attention_f16(L.ptr(qkv), L.ptr(out), nseq, L_tok, heads, W, L.ptr(mask), mask.stride(0),
                                                mask.stride(1), _st(qkv)), "cc_key_masked_attention_f16")
    return out


@key_masked_attention.register_fake
def _(qkv, mask, nseq, L_tok, heads):
    return qkv.new_empty((nseq * L_tok, qkv.shape[1] // 3))


@custom_op(NS + "::key_masked_attention_backward", mutates_args=("amax",), device_types="cuda")
def key_masked_attention_backward(qkv: torch.Tensor, mask: torch.Tensor, d_out: torch.Tensor, nseq: int, L_tok: int, heads: int,
                                  amax: Optional[torch.Tensor]) -> torch.Tensor:
    """d_out [nseq * L, W] fp32 -> d_qkv [nseq * L, 3W] fp32; amax (optional, one device float): max(it, largest |d_qkv|)."""
    W = qkv.shape[1] // 3
    _mask_i64(mask)
    d_qkv = _e(nseq * L_tok, 3 * W, like=qkv, dtype=torch.float32)
    L.check(L.lib().cc_key_masked_attention_backward_f16(L.ptr(qkv), L.ptr(mask), mask.stride(0), mask.stride(1), L.ptr(d_out),
                                                         L.ptr(d_qkv), nseq, L_tok, heads, W, L.ptr(amax), _st(qkv)),
            "cc_key_masked_attention_backward_f16")
    return d_qkv


@key_masked_attention_backward.register_fake
def _(qkv, mask, d_out, nseq, L_tok, heads, amax):
    return qkv.new_empty((nseq * L_tok, qkv.shape[1]), dtype=torch.float32)


SEQTRANSF_BLOCK_FIELDS = ("ln_1_weight", "ln_1_bias", "in_proj_weight_f16", "in_proj_bias", "out_proj_weight_f16", "out_proj_bias",
                          "ln_2_weight", "ln_2_bias", "c_fc_weight_f16", "c_fc_bias", "c_proj_weight_f16", "c_proj_bias")


@custom_op(NS + "::seqtransf_forward", mutates_args=(), device_types="cuda")
def seqtransf_forward(feat: torch.Tensor, mask: torch.Tensor, pos: torch.Tensor, weights: List[torch.Tensor],
                      heads: int) -> torch.Tensor:
    """The seqTransf head (clip4clip.py:335-349): feat [B, T, D] fp32 + pos[0:T] -> blocks with the key mask [B, T] int64 (any
    strides) -> + feat.  ``weights``: per block the 12 tensors of SEQTRANSF_BLOCK_FIELDS (fp16 for *_f16, fp32 otherwise)."""
    from ._lib_clip import BlockWeights
    B, T, D = feat.shape
    _mask_i64(mask)
    nf = len(SEQTRANSF_BLOCK_FIELDS)
    if len(weights) % nf:
        raise ValueError("seqtransf_forward: %d weight tensors per block" % nf)
    layers = len(weights) // nf
    arr = (BlockWeights * max(layers, 1))()
    for i in range(layers):
        for k, name in enumerate(SEQTRANSF_BLOCK_FIELDS):
            setattr(arr[i], name, L.ptr(weights[i * nf + k]))
    out = torch.empty_like(feat)
    lib = L.lib()
    ws = L.workspace(lib.cc_seqtransf_workspace_bytes(B, T, D), feat.device)
    L.check(lib.cc_seqtransf_forward_f32(L.ptr(feat), L.ptr(mask), mask.stride(0), mask.stride(1), L.ptr(pos), arr, layers, B, T, D,
                                         heads, L.ptr(out), L.ptr(ws), ws.numel(), _st(feat)), "cc_seqtransf_forward_f32")
    return out


@seqtransf_forward.register_fake
def _(feat, mask, pos, weights, heads):
    return torch.empty_like(feat)


@custom_op(NS + "::fold_layernorm_linear", mutates_args=(), device_types="cuda")
def fold_layernorm_linear(weight: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor,
                          beta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    N, K = weight.shape
    wf = _e(N, K, like=weight, dtype=torch.float16)
    c1 = _e(N, like=weight, dtype=torch.float32)
    c2 = _e(N, like=weight, dtype=torch.float32)
    L.check(L.lib().cc_fold_layernorm_linear_f32(L.ptr(weight), L.ptr(bias), L.ptr(gamma), L.ptr(beta), N, K, L.ptr(wf),
                                                 L.ptr(c1), L.ptr(c2), _st(weight)), "cc_fold_layernorm_linear_f32")
    return wf, c1, c2


@fold_layernorm_linear.register_fake
def _(weight, bias, gamma, beta):
    N, K = weight.shape
    return weight.new_empty((N, K), dtype=torch.float16), weight.new_empty((N,)), weight.new_empty((N,))


@custom_op(NS + "::row_stats", mutates_args=(), device_types="cuda")
def row_stats(h: torch.Tensor, centre: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    M, W = h.shape
    h16 = _e(M, W, like=h, dtype=torch.float16)
    stats = _e(M, 2, like=h, dtype=torch.float32)
    shift = _e(M if centre else 0, like=h, dtype=torch.float32)
    L.check(L.lib().cc_row_stats_f16(L.ptr(h), L.ptr(h16), L.ptr(stats), L.ptr(shift) if centre else None, M, W, _st(h)),
            "cc_row_stats_f16")
    return h16, stats, shift


@row_stats.register_fake
def _(h, centre):
    M, W = h.shape
    return h.new_empty((M, W), dtype=torch.float16), h.new_empty((M, 2)), h.new_empty((M if centre else 0,))


@custom_op(NS + "::linear_ln_f16", mutates_args=(), device_types="cuda")
def linear_ln_f16(h16: torch.Tensor, w_ln: torch.Tensor, c1: torch.Tensor, c2: torch.Tensor, stats: torch.Tensor,
                  slots: int, gelu: bool, eps: float, tile: int) -> torch.Tensor:
    M, K = h16.shape
    N = w_ln.shape[0]
    out = _e(M, N, like=h16, dtype=torch.float16)
    L.check(L.lib().cc_linear_ln_f16(L.ptr(h16), L.ptr(w_ln), L.ptr(c1), L.ptr(c2), L.ptr(stats), int(slots), float(eps),
                                     L.ptr(out), M, N, K, int(gelu), tile, _st(h16)), "cc_linear_ln_f16")
    return out


@linear_ln_f16.register_fake
def _(h16, w_ln, c1, c2, stats, slots, gelu, eps, tile):
    return h16.new_empty((h16.shape[0], w_ln.shape[0]))


@custom_op(NS + "::linear_ln_act_f16", mutates_args=(), device_types="cuda")
def linear_ln_act_f16(h16: torch.Tensor, w_ln: torch.Tensor, c1: torch.Tensor, c2: torch.Tensor, stats: torch.Tensor,
                      slots: int, act: int, eps: float, tile: int) -> torch.Tensor:
    """linear_ln_f16 with the activation by number: 0 none, 1 QuickGELU, 2 the exact GELU (cc_linear_ln_f16's ``gelu``)."""
    M, K = h16.shape
    N = w_ln.shape[0]
    out = _e(M, N, like=h16, dtype=torch.float16)
    L.check(L.lib().cc_linear_ln_f16(L.ptr(h16), L.ptr(w_ln), L.ptr(c1), L.ptr(c2), L.ptr(stats), int(slots), float(eps),
                                     L.ptr(out), M, N, K, int(act), tile, _st(h16)), "cc_linear_ln_f16")
    return out


@linear_ln_act_f16.register_fake
def _(h16, w_ln, c1, c2, stats, slots, act, eps, tile):
    return h16.new_empty((h16.shape[0], w_ln.shape[0]))


@custom_op(NS + "::inproj_attention_f16", mutates_args=(), device_types="cuda")
def inproj_attention_f16(h16: torch.Tensor, w_ln: torch.Tensor, c1: torch.Tensor, c2: torch.Tensor, stats: torch.Tensor,
                         slots: int, eps: float, nseq: int, L_tok: int, heads: int, causal: bool,
                         seq_off: Optional[torch.Tensor], seq_len: Optional[torch.Tensor]) -> torch.Tensor:
    """LN-folded in_proj + attention in one launch (frame-major rows); -> att [nseq * L_tok, W] fp16."""
    M, W = h16.shape
    out = torch.zeros(M, W, device=h16.device, dtype=torch.float16) if seq_off is not None else _e(M, W, like=h16, dtype=torch.float16)
    L.check(L.lib().cc_inproj_attention_f16(L.ptr(h16), L.ptr(w_ln), L.ptr(c1), L.ptr(c2), L.ptr(stats), int(slots), float(eps),
                                            L.ptr(out), nseq, L_tok, heads, int(causal), L.ptr(seq_off), L.ptr(seq_len), None,
                                            _st(h16)), "cc_inproj_attention_f16")
    return out


@inproj_attention_f16.register_fake
def _(h16, w_ln, c1, c2, stats, slots, eps, nseq, L_tok, heads, causal, seq_off, seq_len):
    return h16.new_empty(h16.shape)


@custom_op(NS + "::linear_resid_stats_f16", mutates_args=("h", "h16", "stats", "shift_out"), device_types="cuda")
def linear_resid_stats_f16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], h: torch.Tensor,
                           h16: torch.Tensor, stats: torch.Tensor, shift_in: Optional[torch.Tensor],
                           stats_in: Optional[torch.Tensor], slots_in: int, shift_out: Optional[torch.Tensor],
                           tile: int) -> None:
    """h += a w^T + b; h16 = fp16(h - c_row); stats (flat, >= M * resid_stats_slots * 2 floats) <- partial sums."""
    M, K = a.shape
    N = w.shape[0]
    slots = ctypes.c_int32(0)
    L.check(L.lib().cc_linear_resid_stats_f16(L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(h), L.ptr(h16), L.ptr(stats),
                                              ctypes.byref(slots), L.ptr(shift_in), L.ptr(stats_in), int(slots_in),
                                              L.ptr(shift_out), M, N, K, tile, _st(a)), "cc_linear_resid_stats_f16")


@linear_resid_stats_f16.register_fake
def _(a, w, bias, h, h16, stats, shift_in, stats_in, slots_in, shift_out, tile):
    return None


def resid_stats_slots(M, N, K, tile=0):
    """Partial-sum slots per row the residual Linear writes for this shape (a host-side query of the tile choice)."""
    n = L.lib().cc_linear_resid_stats_slots(int(M), int(N), int(K), int(tile))
    if n <= 0:
        raise L.CenterClipHipError("cc_linear_resid_stats_slots(%d, %d, %d, %d): unsupported shape / tile" % (M, N, K, tile))
    return n


@custom_op(NS + "::head_project", mutates_args=(), device_types="cuda")
def head_project(h: torch.Tensor, row_mul: int, row_idx: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                 proj: torch.Tensor, R: int) -> torch.Tensor:
    W, E = proj.shape
    out = _e(R, E, like=h, dtype=torch.float32)
    L.check(L.lib().cc_head_project_f32(L.ptr(h), row_mul, L.ptr(row_idx), L.ptr(gamma), L.ptr(beta), L.ptr(proj),
                                        L.ptr(out), R, W, E, _st(h)), "cc_head_project_f32")
    return out


@head_project.register_fake
def _(h, row_mul, row_idx, gamma, beta, proj, R):
    return h.new_empty((R, proj.shape[1]))


# ------------------------------------------------------------------------------------------ token cluster
def _variant(algorithm, aggregation, cluster_embed, cls_mult, fixed_ids, spectral=None):
    var = L.ClusterVariant()
    var.algorithm, var.aggregation = int(algorithm), int(aggregation)
    var.cluster_embed = cluster_embed.data_ptr() if cluster_embed is not None else None
    var.cls_multiplier = cls_mult.data_ptr() if cls_mult is not None else None
    var.fixed_ids = fixed_ids.data_ptr() if fixed_ids is not None else None
    if spectral is not None:                       # (sigma, graph mode, knn_k, correct_sign, graph [N,N] uint8 | None)
        sigma, mode, knn_k, sign, graph = spectral
        var.spectral_sigma, var.spectral_graph_mode, var.spectral_knn_k = float(sigma), int(mode), int(knn_k)
        var.spectral_correct_sign = int(bool(sign))
        var.spectral_graph = graph.data_ptr() if graph is not None else None
    return var


def _cluster_ws(lib, P, N, W, pre_norm, K, algorithm, device):
    need = lib.cc_cluster_workspace_bytes(P, N, W, int(pre_norm))
    if algorithm == 3:
        need += lib.cc_spectral_workspace_bytes(P, N, K)
    return L.workspace(need, device)


def _cluster_strides(shape, frame_major):
    if frame_major:
        BT, Lt, W = shape
        return BT, Lt, W, W, Lt * W
    Lt, BT, W = shape
    return BT, Lt, W, BT * W, W


def _token_cluster(x, frame_major, T, T_new, K, kmedoids, variant, spectral, *, want_medoids, want_assign):
    """The one cc_token_cluster_variant_f32 call of token_cluster / token_cluster_train -> (out, medoids, assign).
    kmedoids = (metric, norm_p, threshold, iter_limit, split_size, pre_norm); variant = (algorithm, aggregation,
    cluster_embed, cls_mult, fixed_ids); spectral = the spectral_* arguments.  The selection outputs only exist for the
    algorithms that select (0 k-medoids, 3 spectral) and are empty when not wanted."""
    metric, norm_p, threshold, iter_limit, split_size, pre_norm = kmedoids
    algorithm = variant[0]
    BT, Lt, W, tok, frame = _cluster_strides(x.shape, frame_major)
    B, n = BT // T, Lt - 1
    oshape = (B * T_new, 1 + K, W) if frame_major else (1 + K, B * T_new, W)
    out = _e(*oshape, like=x, dtype=torch.float32)
    _, _, _, o_tok, o_frame = _cluster_strides(oshape, frame_major)
    kmed = algorithm in (0, 3)
    N = (T // T_new) * n
    med = _e(B * T_new if (want_medoids and kmed) else 0, K, like=x, dtype=torch.long)
    assign = _e(B * T_new if (want_assign and kmed) else 0, N, like=x, dtype=torch.long)
    var = _variant(*variant, spectral if algorithm == 3 else None)
    lib = L.lib()
    ws = _cluster_ws(lib, B * T_new, N, W, pre_norm, K, algorithm, x.device)
    L.check(lib.cc_token_cluster_variant_f32(L.ptr(x), tok, frame, B, T, T_new, n, W, K, metric, float(norm_p),
                                             float(threshold), int(iter_limit), int(split_size), int(pre_norm),
                                             ctypes.byref(var), L.ptr(out), o_tok, o_frame,
                                             L.ptr(med) if med.numel() else None, L.ptr(assign) if assign.numel() else None,
                                             None, L.ptr(ws), ws.numel(), _st(x)), "cc_token_cluster_variant_f32")
    return out, med, assign


@custom_op(NS + "::token_cluster", mutates_args=(), device_types="cuda")
def token_cluster(x: torch.Tensor, frame_major: bool, T: int, T_new: int, K: int, metric: int, norm_p: float,
                  threshold: float, iter_limit: int, split_size: int, pre_norm: bool, algorithm: int, aggregation: int,
                  cluster_embed: Optional[torch.Tensor], cls_mult: Optional[torch.Tensor], fixed_ids: Optional[torch.Tensor],
                  want_medoids: bool, spectral_sigma: float = 0.0, spectral_mode: int = 0, spectral_knn_k: int = 0,
                  spectral_sign: bool = False, spectral_graph: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """TokenClusterInter.forward (modules/cluster/cluster.py:206-352).  x contiguous fp32: [1+n, B*T, W] (LND, the
    reference's layout) or [B*T, 1+n, W] (frame_major) -> same layout with T_new segments of 1+K tokens; medoids
    [T_new*B, K] int64 (empty unless want_medoids and algorithm 0 / 3).  algorithm 3 = 'spectral' (the spectral_* arguments:
    sigma, graph mode 0 HeatKernel / 1 KNN, knn_k, sign correction, optional [N,N] uint8 spatial-temporal mask)."""
    out, med, _ = _token_cluster(x, frame_major, T, T_new, K, (metric, norm_p, threshold, iter_limit, split_size, pre_norm),
                                 (algorithm, aggregation, cluster_embed, cls_mult, fixed_ids),
                                 (spectral_sigma, spectral_mode, spectral_knn_k, spectral_sign, spectral_graph),
                                 want_medoids=want_medoids, want_assign=False)
    return out, med


@token_cluster.register_fake
def _(x, frame_major, T, T_new, K, metric, norm_p, threshold, iter_limit, split_size, pre_norm, algorithm, aggregation,
      cluster_embed, cls_mult, fixed_ids, want_medoids, spectral_sigma=0.0, spectral_mode=0, spectral_knn_k=0,
      spectral_sign=False, spectral_graph=None):
    if frame_major:
        BT, Lt, W = x.shape
        out = x.new_empty((BT // T * T_new, 1 + K, W))
    else:
        Lt, BT, W = x.shape
        out = x.new_empty((1 + K, BT // T * T_new, W))
    rows = BT // T * T_new if (want_medoids and algorithm in (0, 3)) else 0
    return out, x.new_empty((rows, K), dtype=torch.long)


@custom_op(NS + "::token_cluster_train", mutates_args=(), device_types="cuda")
def token_cluster_train(x: torch.Tensor, frame_major: bool, T: int, T_new: int, K: int, metric: int, norm_p: float,
                        threshold: float, iter_limit: int, split_size: int, pre_norm: bool, algorithm: int, aggregation: int,
                        cluster_embed: Optional[torch.Tensor], cls_mult: Optional[torch.Tensor],
                        fixed_ids: Optional[torch.Tensor], spectral_sigma: float = 0.0, spectral_mode: int = 0,
                        spectral_knn_k: int = 0, spectral_sign: bool = False,
                        spectral_graph: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """token_cluster that also returns what its backward needs: medoids [T_new*B, K] and assign [T_new*B, fd*n] (both
    empty for 'pooling' / 'sparse_sampling').  Differentiable with respect to x, cluster_embed and cls_mult
    (torch.ops.centerclip.token_cluster_backward); the selection is a constant of the backward pass, as in the reference,
    whose k-medoids runs under no_grad (fast_kmeans.py:13,44)."""
    return _token_cluster(x, frame_major, T, T_new, K, (metric, norm_p, threshold, iter_limit, split_size, pre_norm),
                          (algorithm, aggregation, cluster_embed, cls_mult, fixed_ids),
                          (spectral_sigma, spectral_mode, spectral_knn_k, spectral_sign, spectral_graph),
                          want_medoids=True, want_assign=True)


@token_cluster_train.register_fake
def _(x, frame_major, T, T_new, K, metric, norm_p, threshold, iter_limit, split_size, pre_norm, algorithm, aggregation,
      cluster_embed, cls_mult, fixed_ids, spectral_sigma=0.0, spectral_mode=0, spectral_knn_k=0, spectral_sign=False,
      spectral_graph=None):
    BT, Lt, W, _, _ = _cluster_strides(x.shape, frame_major)
    B, n = BT // T, Lt - 1
    out = x.new_empty((B * T_new, 1 + K, W) if frame_major else (1 + K, B * T_new, W))
    rows = B * T_new if algorithm in (0, 3) else 0
    return out, x.new_empty((rows, K), dtype=torch.long), x.new_empty((rows, (T // T_new) * n), dtype=torch.long)


@custom_op(NS + "::token_apply_selection", mutates_args=(), device_types="cuda")
def token_apply_selection(x: torch.Tensor, frame_major: bool, T: int, T_new: int, K: int, aggregation: int,
                          medoids: torch.Tensor, assign: torch.Tensor, cluster_embed: Optional[torch.Tensor],
                          cls_mult: Optional[torch.Tensor]) -> torch.Tensor:
    """The gather / aggregation half of TokenClusterInter.forward (cluster.py:287-310) for a selection made elsewhere
    (cluster_algo 'spectral'): medoids [T_new*B, K] or, for cluster means, assign [T_new*B, fd*n]."""
    BT, Lt, W, tok, frame = _cluster_strides(x.shape, frame_major)
    B, n = BT // T, Lt - 1
    oshape = (B * T_new, 1 + K, W) if frame_major else (1 + K, B * T_new, W)
    out = _e(*oshape, like=x, dtype=torch.float32)
    _, _, _, o_tok, o_frame = _cluster_strides(oshape, frame_major)
    var = _variant(0, aggregation, cluster_embed, cls_mult, None)
    L.check(L.lib().cc_token_apply_selection_f32(L.ptr(x), tok, frame, B, T, T_new, n, W, K, ctypes.byref(var),
                                                 L.ptr(medoids) if medoids.numel() else None,
                                                 L.ptr(assign) if assign.numel() else None, L.ptr(out), o_tok, o_frame,
                                                 _st(x)), "cc_token_apply_selection_f32")
    return out


@token_apply_selection.register_fake
def _(x, frame_major, T, T_new, K, aggregation, medoids, assign, cluster_embed, cls_mult):
    BT, Lt, W, _, _ = _cluster_strides(x.shape, frame_major)
    B = BT // T
    return x.new_empty((B * T_new, 1 + K, W) if frame_major else (1 + K, B * T_new, W))


@custom_op(NS + "::token_cluster_backward", mutates_args=(), device_types="cuda")
def token_cluster_backward(grad_out: torch.Tensor, x: torch.Tensor, frame_major: bool, T: int, T_new: int, K: int,
                           algorithm: int, aggregation: int, medoids: torch.Tensor, assign: torch.Tensor,
                           cls_mult: Optional[torch.Tensor], fixed_ids: Optional[torch.Tensor], want_embed: bool,
                           want_mult: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradient of token_cluster_train for a fixed selection (cc_token_cluster_backward_f32): -> (grad_x like x,
    grad_cluster_embed [K, W] or empty, grad_cls_mult [T] or empty)."""
    BT, Lt, W, tok, frame = _cluster_strides(x.shape, frame_major)
    B, n = BT // T, Lt - 1
    _, _, _, g_tok, g_frame = _cluster_strides(grad_out.shape, frame_major)
    gx = torch.empty_like(x)
    g_embed = _e(K if want_embed else 0, W, like=x, dtype=torch.float32)
    g_mult = _e(T if want_mult else 0, like=x, dtype=torch.float32)
    var = _variant(algorithm, aggregation, None, cls_mult, fixed_ids)
    L.check(L.lib().cc_token_cluster_backward_f32(L.ptr(grad_out), g_tok, g_frame, B, T, T_new, n, W, K, ctypes.byref(var),
                                                  L.ptr(medoids) if medoids.numel() else None,
                                                  L.ptr(assign) if assign.numel() else None, L.ptr(x), tok, frame,
                                                  L.ptr(gx), tok, frame, L.ptr(g_embed) if want_embed else None,
                                                  L.ptr(g_mult) if want_mult else None, _st(x)),
            "cc_token_cluster_backward_f32")
    return gx, g_embed, g_mult


@token_cluster_backward.register_fake
def _(grad_out, x, frame_major, T, T_new, K, algorithm, aggregation, medoids, assign, cls_mult, fixed_ids, want_embed,
      want_mult):
    W = x.shape[-1]
    return torch.empty_like(x), x.new_empty((K if want_embed else 0, W)), x.new_empty((T if want_mult else 0,))


def _token_cluster_setup(ctx, inputs, output):
    (x, frame_major, T, T_new, K, _m, _p, _t, _i, _s, _pn, algorithm, aggregation, cluster_embed, cls_mult, fixed_ids) = inputs[:16]
    algorithm = 0 if algorithm == 3 else algorithm          # spectral: the backward is that of the gather / cluster means
    _, med, assign = output
    ctx.cfg = (frame_major, T, T_new, K, algorithm, aggregation)
    ctx.has = (cluster_embed is not None, cls_mult is not None, fixed_ids is not None)
    ctx.save_for_backward(x, med, assign, *(t for t in (cls_mult, fixed_ids) if t is not None))


def _token_cluster_bwd(ctx, grad_out, _gmed, _gassign):
    frame_major, T, T_new, K, algorithm, aggregation = ctx.cfg
    has_embed, has_mult, has_ids = ctx.has
    saved = list(ctx.saved_tensors)
    x, med, assign = saved[:3]
    rest = saved[3:]
    cls_mult = rest.pop(0) if has_mult else None
    fixed_ids = rest.pop(0) if has_ids else None
    want_embed = has_embed and ctx.needs_input_grad[13]
    want_mult = has_mult and ctx.needs_input_grad[14]
    gx, ge, gm = torch.ops.centerclip.token_cluster_backward(grad_out.contiguous().float(), x, frame_major, T, T_new, K,
                                                             algorithm, aggregation, med, assign, cls_mult, fixed_ids,
                                                             want_embed, want_mult)
    return (gx,) + (None,) * 12 + (ge if want_embed else None, gm if want_mult else None) + (None,) * 6


token_cluster_train.register_autograd(_token_cluster_bwd, setup_context=_token_cluster_setup)


SHIFT_MODES = {'temporal_shift': 4, 'token_shift': 5}      # CC_CLUSTER_TEMPORAL_SHIFT / CC_CLUSTER_TOKEN_SHIFT


@custom_op(NS + "::token_shift", mutates_args=(), device_types="cuda")
def token_shift(x: torch.Tensor, frame_major: bool, segment: int, fold_div: int, mode: int, adjoint: bool) -> torch.Tensor:
    """temporal_shift_wo_cls / token_shift (modules/cluster/shift.py) of x [L, F, W] (LND) or [F, L, W] (frame_major) over
    segments of ``segment`` consecutive frames; adjoint=True applies the transpose (the backward).  Bit exact."""
    x = x.contiguous()
    F, Lt, W, ts, fs = _cluster_strides(x.shape, frame_major)
    out = torch.empty_like(x)
    L.check(L.lib().cc_token_shift_f32(L.ptr(x), ts, fs, F, Lt, W, int(segment), int(fold_div), int(mode), int(bool(adjoint)),
                                       L.ptr(out), ts, fs, _st(x)), "cc_token_shift_f32")
    return out


@token_shift.register_fake
def _(x, frame_major, segment, fold_div, mode, adjoint):
    return torch.empty_like(x)


@custom_op(NS + "::token_shift_rows", mutates_args=("h", "h16", "stats", "shift"), device_types="cuda")
def token_shift_rows(h: torch.Tensor, tok_rows: int, frame_rows: int, F: int, L_tok: int, segment: int, fold_div: int,
                     mode: int, h16: torch.Tensor, stats: torch.Tensor, slots: int, shift: torch.Tensor) -> None:
    """The shift in place on the contiguous fp32 rows h [M, W] (row of frame f, token j = f * frame_rows + j * tok_rows), with
    the fp16 copy h16, the statistics (slot 0 of stats [M, slots, 2], zeros in the others) and the centre ``shift`` [M] of
    every row it rewrites (cc_token_shift_rows_f32: what the next LayerNorm-folded GEMM reads)."""
    M, W = h.shape
    L.check(L.lib().cc_token_shift_rows_f32(L.ptr(h), int(tok_rows), int(frame_rows), int(F), int(L_tok), W, int(segment),
                                            int(fold_div), int(mode), L.ptr(h16), L.ptr(stats), int(slots), L.ptr(shift), _st(h)),
            "cc_token_shift_rows_f32")


@token_shift_rows.register_fake
def _(h, tok_rows, frame_rows, F, L_tok, segment, fold_div, mode, h16, stats, slots, shift):
    return None


@custom_op(NS + "::batch_kmedoids", mutates_args=(), device_types="cuda")
def batch_kmedoids(x: torch.Tensor, K: int, metric: int, norm_p: float, threshold: float, iter_limit: int, id_sort: bool,
                   split_size: int, pre_norm: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """batch_fast_kmedoids_with_split (modules/cluster/fast_kmeans.py:14-97): x [P,N,W] -> (assign [P,N] int64,
    medoids [P,K] int64, iterations [P] int32)."""
    P, N, W = x.shape
    lay = L.TokenLayout(P, 1, 1, N, N * W, 0, 0, W)
    lib = L.lib()
    medoids = _e(P, K, like=x, dtype=torch.long)
    assign = _e(P, N, like=x, dtype=torch.long)
    iters = _e(P, like=x, dtype=torch.int32)
    ws = L.workspace(lib.cc_cluster_workspace_bytes(P, N, W, int(pre_norm)), x.device)
    L.check(lib.cc_batch_kmedoids_f32(L.ptr(x), ctypes.byref(lay), W, int(K), metric, float(norm_p), float(threshold),
                                      int(iter_limit), int(id_sort), int(split_size), int(pre_norm), L.ptr(medoids),
                                      L.ptr(assign), L.ptr(iters), L.ptr(ws), ws.numel(), _st(x)), "cc_batch_kmedoids_f32")
    return assign, medoids, iters


@batch_kmedoids.register_fake
def _(x, K, metric, norm_p, threshold, iter_limit, id_sort, split_size, pre_norm):
    P, N, W = x.shape
    return (x.new_empty((P, N), dtype=torch.long), x.new_empty((P, K), dtype=torch.long),
            x.new_empty((P,), dtype=torch.int32))


@custom_op(NS + "::kmedoids_from_dist", mutates_args=(), device_types="cuda")
def kmedoids_from_dist(dist: torch.Tensor, norms: torch.Tensor, K: int, iter_limit: int,
                       id_sort: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    P, N, _ = dist.shape
    medoids = _e(P, K, like=dist, dtype=torch.long)
    assign = _e(P, N, like=dist, dtype=torch.long)
    iters = _e(P, like=dist, dtype=torch.int32)
    L.check(L.lib().cc_kmedoids_from_dist_f32(L.ptr(dist), L.ptr(norms), P, N, int(K), int(iter_limit), int(id_sort),
                                              L.ptr(medoids), L.ptr(assign), L.ptr(iters), None, 0, _st(dist)),
            "cc_kmedoids_from_dist_f32")
    return assign, medoids, iters


@kmedoids_from_dist.register_fake
def _(dist, norms, K, iter_limit, id_sort):
    P, N, _ = dist.shape
    return (dist.new_empty((P, N), dtype=torch.long), dist.new_empty((P, K), dtype=torch.long),
            dist.new_empty((P,), dtype=torch.int32))


@custom_op(NS + "::pairwise_distance", mutates_args=(), device_types="cuda")
def pairwise_distance(x: torch.Tensor, metric: int, p: float, all_negative: bool, self_nearest: bool) -> torch.Tensor:
    """pairwise_distance(x, x, ...) (modules/cluster/cluster_utils.py:8-43): x [P,N,W] -> [P,N,N]."""
    P, N, W = x.shape
    lay = L.TokenLayout(P, 1, 1, N, N * W, 0, 0, W)
    dist = _e(P, N, N, like=x, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_cluster_workspace_bytes(P, N, W, 0), x.device)
    L.check(lib.cc_pairwise_distance_f32(L.ptr(x), ctypes.byref(lay), W, metric, float(p), int(all_negative),
                                         int(self_nearest), P, L.ptr(dist), None, L.ptr(ws), ws.numel(), _st(x)),
            "cc_pairwise_distance_f32")
    return dist


@pairwise_distance.register_fake
def _(x, metric, p, all_negative, self_nearest):
    P, N, W = x.shape
    return x.new_empty((P, N, N))


@custom_op(NS + "::pairwise_distance_cross", mutates_args=(), device_types="cuda")
def pairwise_distance_cross(x1: torch.Tensor, x2: torch.Tensor, metric: int, p: float, all_negative: bool,
                            self_nearest: bool) -> torch.Tensor:
    """pairwise_distance(data1, data2, ...) for two different sets (cluster_utils.py:8-43): [P,N1,W], [P,N2,W] -> [P,N1,N2]."""
    P, N1, W = x1.shape
    N2 = x2.shape[1]
    dist = _e(P, N1, N2, like=x1, dtype=torch.float32)
    ws = L.workspace(256, x1.device)
    L.check(L.lib().cc_pairwise_distance_cross_f32(L.ptr(x1), L.ptr(x2), P, N1, N2, W, metric, float(p), int(all_negative),
                                                   int(self_nearest), L.ptr(dist), L.ptr(ws), ws.numel(), _st(x1)),
            "cc_pairwise_distance_cross_f32")
    return dist


@pairwise_distance_cross.register_fake
def _(x1, x2, metric, p, all_negative, self_nearest):
    return x1.new_empty((x1.shape[0], x1.shape[1], x2.shape[1]))


@custom_op(NS + "::token_norms", mutates_args=(), device_types="cuda")
def token_norms(x: torch.Tensor) -> torch.Tensor:
    P, N, W = x.shape
    lay = L.TokenLayout(P, 1, 1, N, N * W, 0, 0, W)
    norms = _e(P, N, like=x, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_cluster_workspace_bytes(P, N, W, 0), x.device)
    L.check(lib.cc_token_norms_f32(L.ptr(x), ctypes.byref(lay), W, L.ptr(norms), L.ptr(ws), ws.numel(), _st(x)),
            "cc_token_norms_f32")
    return norms


@token_norms.register_fake
def _(x):
    return x.new_empty(x.shape[:2])


@custom_op(NS + "::spectral_laplacian", mutates_args=(), device_types="cuda")
def spectral_laplacian(x: torch.Tensor, sigma: float, graph: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Normalised graph Laplacian of the heat-kernel affinity (modules/cluster/spectral.py:42-52,79-107): x [P,N,W] fp32,
    graph [N,N] uint8 or None -> (L_sym [P,N,N], W [P,N,N])."""
    P, N, Wd = x.shape
    lay = L.TokenLayout(P, 1, 1, N, N * Wd, 0, 0, Wd)
    lap = _e(P, N, N, like=x, dtype=torch.float32)
    aff = _e(P, N, N, like=x, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_cluster_workspace_bytes(P, N, Wd, 0), x.device)
    L.check(lib.cc_spectral_laplacian_f32(L.ptr(x), ctypes.byref(lay), Wd, float(sigma), L.ptr(graph), L.ptr(lap), L.ptr(aff),
                                          None, L.ptr(ws), ws.numel(), _st(x)), "cc_spectral_laplacian_f32")
    return lap, aff


@spectral_laplacian.register_fake
def _(x, sigma, graph):
    P, N, _W = x.shape
    return x.new_empty((P, N, N)), x.new_empty((P, N, N))


@custom_op(NS + "::spectral_graph_laplacian", mutates_args=(), device_types="cuda")
def spectral_graph_laplacian(x: torch.Tensor, frame_major: bool, T: int, T_new: int, sigma: float, mode: int, knn_k: int,
                             mutual: bool, graph: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """constructW + normalised Laplacian (spectral.py:42-52,79-107) for the heat-kernel (mode 0) and the KNN graph (mode 1).
    x: [P,N,W] (T = T_new = 0), or the activations of TokenClusterInter ([1+n, B*T, W] LND / [B*T, 1+n, W] frame-major) whose
    patch tokens are regrouped into T_new segments per clip through strides (problem p = s*B + b, cluster.py:247-250).
    -> (L_sym [P,N,N], W [P,N,N])."""
    if T == 0:
        P, N, Wd = x.shape
        lay = L.TokenLayout(P, 1, 1, N, N * Wd, 0, 0, Wd)
        base = x
    else:
        BT, Lt, Wd, tok, frame = _cluster_strides(x.shape, frame_major)
        B, n, fd = BT // T, Lt - 1, T // T_new
        P, N = B * T_new, fd * n
        lay = L.TokenLayout(B, T_new, fd, n, T * frame, fd * frame, frame, tok)
        base = x.reshape(-1)[tok:]                       # first patch token of frame 0 (the CLS token is skipped)
    lap = _e(P, N, N, like=x, dtype=torch.float32)
    aff = _e(P, N, N, like=x, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_cluster_workspace_bytes(P, N, Wd, 0), x.device)
    L.check(lib.cc_spectral_graph_laplacian_f32(L.ptr(base), ctypes.byref(lay), Wd, float(sigma), int(mode), int(knn_k),
                                                int(mutual), L.ptr(graph), L.ptr(lap), L.ptr(aff), None, L.ptr(ws), ws.numel(),
                                                _st(x)), "cc_spectral_graph_laplacian_f32")
    return lap, aff


@spectral_graph_laplacian.register_fake
def _(x, frame_major, T, T_new, sigma, mode, knn_k, mutual, graph):
    if T == 0:
        P, N, _W = x.shape
    else:
        BT, Lt, _W, _, _ = _cluster_strides(x.shape, frame_major)
        P, N = BT // T * T_new, (T // T_new) * (Lt - 1)
    return x.new_empty((P, N, N)), x.new_empty((P, N, N))


@custom_op(NS + "::spectral_embedding", mutates_args=(), device_types="cuda")
def spectral_embedding(laplacian: torch.Tensor, K: int, correct_sign: bool, solver: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The decomposition of batch_spectral_clustering (spectral.py:54-61, cc_spectral_embedding_solver_f32): laplacian [P,N,N]
    -> (Q [P,N,K4] with K4 = K rounded up to 4 and zero padding columns - the k-medoids kernels read 16-byte pieces -,
    eigenvalues [P,K] in the reference's order, sweeps [P]).  solver: 0 = CC_EIG_AUTO, 1 = CC_EIG_JACOBI."""
    P, N, _ = laplacian.shape
    K4 = (K + 3) // 4 * 4
    Q = _e(P, N, K4, like=laplacian, dtype=torch.float32)
    ev = _e(P, K, like=laplacian, dtype=torch.float32)
    sw = _e(P, like=laplacian, dtype=torch.int32)
    lib = L.lib()
    ws = L.workspace(lib.cc_spectral_embedding_workspace_bytes(P, N), laplacian.device)
    L.check(lib.cc_spectral_embedding_solver_f32(L.ptr(laplacian), P, N, int(K), int(correct_sign), L.ptr(Q), K4, L.ptr(ev),
                                                 L.ptr(sw), int(solver), L.ptr(ws), ws.numel(), _st(laplacian)),
            "cc_spectral_embedding_solver_f32")
    return Q, ev, sw


@spectral_embedding.register_fake
def _(laplacian, K, correct_sign, solver=0):
    P, N, _ = laplacian.shape
    return (laplacian.new_empty((P, N, (K + 3) // 4 * 4)), laplacian.new_empty((P, K)),
            laplacian.new_empty((P,), dtype=torch.int32))


@custom_op(NS + "::svd_sign_flip", mutates_args=(), device_types="cuda")
def svd_sign_flip(U: torch.Tensor, S: torch.Tensor, VT: torch.Tensor) -> torch.Tensor:
    """batch_sign_flip_rasmus_bro (spectral.py:110-137): U [P,M,K], S [P,K], VT [P,K,N] -> sign-corrected copy of U."""
    P, M, K = U.shape
    out = U.clone()
    L.check(L.lib().cc_svd_sign_flip_f32(L.ptr(out), L.ptr(S), L.ptr(VT), P, M, K, VT.shape[2], _st(U)),
            "cc_svd_sign_flip_f32")
    return out


@svd_sign_flip.register_fake
def _(U, S, VT):
    return torch.empty_like(U)


# ------------------------------------------------------------------------------------------ encoders
def _check_forced_medoids(lib, m, B: int, forced_medoids: Optional[torch.Tensor]) -> None:
    """The C entry points take forced_medoids as a bare pointer: the id tensors of ALL cluster blocks back to back.  A
    buffer of any other length (e.g. the ids of the last block only, as rounds 1-4 took them) would be read past its end."""
    if forced_medoids is None:
        return
    want = int(lib.cc_vit_forced_medoids_count(ctypes.byref(m), B))
    if (forced_medoids.dtype != torch.long or not forced_medoids.is_contiguous() or forced_medoids.numel() != want):
        raise ValueError(f"forced_medoids: {want} contiguous int64 ids expected (every cluster block's [B*T_new, K] ids "
                         f"back to back), got {forced_medoids.numel()} of {forced_medoids.dtype}")


@custom_op(NS + "::vit_encode", mutates_args=(), device_types="cuda")
def vit_encode(frames: torch.Tensor, handle: int, B: int, T: int, want_hidden: bool, want_medoids: bool,
               forced_medoids: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CLIP.encode_image / VisualTransformer.forward (modules/clip.py:460-469,304-349): frames [B*T,3,H,W] fp32 or
    uint8 ([B*T,3,H,W] / [B*T,H,W,3]) -> (features [B*T_final, E], hidden [B*T_final, L_final, W] before ln_post or
    empty, medoids of the last k-medoids block or empty)."""
    from .clip import frames_descriptor
    m, meta, _keep = _model(handle)
    fr, frames = frames_descriptor(frames)
    frames_out, ltok, med_shape = meta["final"](T)
    lib = L.lib()
    feats = _e(B * frames_out, meta["embed_dim"], like=frames, dtype=torch.float32)
    hidden = _e(B * frames_out if want_hidden else 0, ltok, meta["width"], like=frames, dtype=torch.float32)
    med = torch.empty((B * med_shape[0], med_shape[1]) if (want_medoids and med_shape) else (0, 0), device=frames.device,
                      dtype=torch.long)
    _check_forced_medoids(lib, m, B, forced_medoids)
    ws = L.workspace(lib.cc_vit_workspace_bytes(ctypes.byref(m), B, T), frames.device)
    L.check(lib.cc_vit_encode_frames(ctypes.byref(m), ctypes.byref(fr), B, T, L.ptr(feats),
                                     L.ptr(hidden) if want_hidden else None, L.ptr(med) if med.numel() else None,
                                     L.ptr(forced_medoids), L.ptr(ws), ws.numel(), _st(frames)), "cc_vit_encode_frames")
    return feats, hidden, med


@vit_encode.register_fake
def _(frames, handle, B, T, want_hidden, want_medoids, forced_medoids):
    _m, meta, _keep = _model(handle)
    frames_out, ltok, med_shape = meta["final"](T)
    feats = frames.new_empty((B * frames_out, meta["embed_dim"]), dtype=torch.float32)
    hidden = frames.new_empty((B * frames_out if want_hidden else 0, ltok, meta["width"]), dtype=torch.float32)
    med = frames.new_empty((B * med_shape[0], med_shape[1]) if (want_medoids and med_shape) else (0, 0), dtype=torch.long)
    return feats, hidden, med


@custom_op(NS + "::text_encode", mutates_args=(), device_types="cuda")
def text_encode(ids: torch.Tensor, handle: int, want_hidden: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """CLIP.encode_text (modules/clip.py:471-496): ids [B, n_ctx] int64 -> (features [B, E], hidden [B, n_ctx, W]
    before ln_final, or empty)."""
    m, meta, _keep = _model(handle)
    Bt, Lt = ids.shape
    lib = L.lib()
    out = _e(Bt, meta["embed_dim"], like=ids, dtype=torch.float32)
    hidden = _e(Bt if want_hidden else 0, Lt, meta["width"], like=ids, dtype=torch.float32)
    ws = L.workspace(lib.cc_text_workspace_bytes(ctypes.byref(m), Bt, Lt), ids.device)
    L.check(lib.cc_text_encode_hidden(ctypes.byref(m), L.ptr(ids), Bt, Lt, L.ptr(out), L.ptr(hidden) if want_hidden else None,
                                      L.ptr(ws), ws.numel(), _st(ids)), "cc_text_encode_hidden")
    return out, hidden


@text_encode.register_fake
def _(ids, handle, want_hidden):
    _m, meta, _keep = _model(handle)
    Bt, Lt = ids.shape
    return (ids.new_empty((Bt, meta["embed_dim"]), dtype=torch.float32),
            ids.new_empty((Bt if want_hidden else 0, Lt, meta["width"]), dtype=torch.float32))


@custom_op(NS + "::vit_encode_prefix", mutates_args=(), device_types="cuda")
def vit_encode_prefix(frames: torch.Tensor, handle: int, B: int, T: int, n_blocks: int,
                      forced_medoids: Optional[torch.Tensor]) -> torch.Tensor:
    """The frozen prefix of the visual tower in training (cc_vit_encode_prefix_frames): frames as vit_encode -> the residual
    stream behind n_blocks blocks, [B*T_n, L_n, W] fp32 frame-major, in one enqueue.  forced_medoids: the ids of the cluster
    blocks among the first n_blocks, back to back.  The handle's meta["prefix"](T, n_blocks) gives (T_n, L_n, id count per clip)."""
    from .clip import frames_descriptor
    m, meta, _keep = _model(handle)
    fr, frames = frames_descriptor(frames)
    frames_out, ltok, ids_per_clip = meta["prefix"](T, n_blocks)
    if forced_medoids is not None and (forced_medoids.dtype != torch.long or not forced_medoids.is_contiguous()
                                       or forced_medoids.numel() != B * ids_per_clip):
        raise ValueError(f"forced_medoids: {B * ids_per_clip} contiguous int64 ids expected (the cluster blocks among the first "
                         f"{n_blocks} blocks, back to back), got {forced_medoids.numel()} of {forced_medoids.dtype}")
    lib = L.lib()
    hidden = _e(B * frames_out, ltok, meta["width"], like=frames, dtype=torch.float32)
    ws = L.workspace(lib.cc_vit_workspace_bytes(ctypes.byref(m), B, T), frames.device)
    L.check(lib.cc_vit_encode_prefix_frames(ctypes.byref(m), ctypes.byref(fr), B, T, int(n_blocks), L.ptr(hidden),
                                            L.ptr(forced_medoids), L.ptr(ws), ws.numel(), _st(frames)),
            "cc_vit_encode_prefix_frames")
    return hidden


@vit_encode_prefix.register_fake
def _(frames, handle, B, T, n_blocks, forced_medoids):
    _m, meta, _keep = _model(handle)
    frames_out, ltok, _ids = meta["prefix"](T, n_blocks)
    return frames.new_empty((B * frames_out, ltok, meta["width"]), dtype=torch.float32)


@custom_op(NS + "::text_encode_prefix", mutates_args=(), device_types="cuda")
def text_encode_prefix(ids: torch.Tensor, handle: int, n_blocks: int) -> torch.Tensor:
    """The frozen prefix of the text tower in training (cc_text_encode_prefix): ids [B, n_ctx] int64 -> the residual stream
    behind n_blocks blocks, [B, n_ctx, W] fp32, every row."""
    m, meta, _keep = _model(handle)
    Bt, Lt = ids.shape
    lib = L.lib()
    hidden = _e(Bt, Lt, meta["width"], like=ids, dtype=torch.float32)
    ws = L.workspace(lib.cc_text_workspace_bytes(ctypes.byref(m), Bt, Lt), ids.device)
    L.check(lib.cc_text_encode_prefix(ctypes.byref(m), L.ptr(ids), Bt, Lt, int(n_blocks), L.ptr(hidden), L.ptr(ws), ws.numel(),
                                      _st(ids)), "cc_text_encode_prefix")
    return hidden


@text_encode_prefix.register_fake
def _(ids, handle, n_blocks):
    _m, meta, _keep = _model(handle)
    return ids.new_empty((ids.shape[0], ids.shape[1], meta["width"]), dtype=torch.float32)


def patch_cols(patch):
    """Columns of the patch matrix and of the packed conv1 weight: 3 p^2 rounded up to a multiple of 64 (the GEMMs' k-step)."""
    return -(-3 * patch * patch // 64) * 64


@custom_op(NS + "::patch_gather", mutates_args=(), device_types="cuda")
def patch_gather(frames: torch.Tensor, resolution: int, patch: int) -> torch.Tensor:
    """The encoders' patch gather on its own (cc_patch_gather_any_f16): frames [F,3,H,W] fp32 (normalised) or uint8
    ([F,3,H,W] / [F,H,W,3], the loader's u8/255 -> (x - mean)/std inside) -> the fp16 patch matrix [F * g * g, patch_cols(p)],
    columns (c, kh, kw); patch_cols(p) = 3 p^2 for p % 8 == 0, else rounded up to a multiple of 64 with zero columns behind."""
    from .clip import frames_descriptor
    fr, frames = frames_descriptor(frames)
    F, g = frames.shape[0], resolution // patch
    out = _e(F * g * g, patch_cols(patch), like=frames, dtype=torch.float16)
    L.check(L.lib().cc_patch_gather_any_f16(ctypes.byref(fr), F, int(resolution), int(patch), L.ptr(out), _st(frames)),
            "cc_patch_gather_any_f16")
    return out


@patch_gather.register_fake
def _(frames, resolution, patch):
    g = resolution // patch
    return frames.new_empty((frames.shape[0] * g * g, patch_cols(patch)), dtype=torch.float16)


@custom_op(NS + "::patch_gather3d", mutates_args=(), device_types="cuda")
def patch_gather3d(frames: torch.Tensor, T: int, resolution: int, patch: int) -> torch.Tensor:
    """The patch gather of linear_patch '3d' on its own (cc_patch_gather3d_f16): frames as patch_gather, clips of T frames ->
    the fp16 patch matrix [F * g * g, 9 * p * p], columns (c, kt, kh, kw) as conv2.weight.view(width, -1) has them; tap kt of
    frame f is frame f + kt - 1 of the same clip, zeros outside the clip (Conv3d padding (1, 0, 0), modules/clip.py:313-317)."""
    from .clip import frames_descriptor
    fr, frames = frames_descriptor(frames)
    F, g = frames.shape[0], resolution // patch
    out = _e(F * g * g, 9 * patch * patch, like=frames, dtype=torch.float16)
    L.check(L.lib().cc_patch_gather3d_f16(ctypes.byref(fr), F, int(T), int(resolution), int(patch), L.ptr(out), _st(frames)),
            "cc_patch_gather3d_f16")
    return out


@patch_gather3d.register_fake
def _(frames, T, resolution, patch):
    g = resolution // patch
    return frames.new_empty((frames.shape[0] * g * g, 9 * patch * patch), dtype=torch.float16)


def _raw_frames_geometry(shape):
    """uint8 frames [..., H, W, 3] or [..., 3, H, W] (at least one leading dimension) -> (channels_first, H, W); [.., 3, H, W]
    wins where both read, as in clip.frames_descriptor."""
    if len(shape) < 4 or (shape[-3] != 3 and shape[-1] != 3):
        raise ValueError("uint8 frames must be [..., H, W, 3] or [..., 3, H, W] with a leading frame dimension, got %s"
                         % (tuple(shape),))
    if shape[-3] == 3:
        return True, int(shape[-2]), int(shape[-1])
    return False, int(shape[-3]), int(shape[-2])


_RESIZE_PLANS = {}


def resize_plan(H, W, n_px, resize, device):
    """The device copy of the plan of cc_resize_crop_u8 for (H, W, n_px, resize), built on the host and uploaded ONCE per device.
    The upload cannot be part of a stream capture: a size that was not seen before the capture is refused there."""
    device = torch.device(device)
    key = (int(H), int(W), int(n_px), int(bool(resize)), device.type, device.index if device.index is not None
           else torch.cuda.current_device())
    plan = _RESIZE_PLANS.get(key)
    if plan is None:
        if torch.cuda.is_current_stream_capturing():
            raise L.CenterClipHipError("resize_center_crop: no plan for %dx%d -> %d frames yet and the stream is being captured "
                                       "(the plan is uploaded once, outside any capture: run this size eagerly first)"
                                       % (H, W, n_px))
        lib = L.lib()
        nbytes = lib.cc_resize_plan_bytes(*key[:4])
        host = torch.empty(max(nbytes // 4, 1), dtype=torch.int32)
        L.check(lib.cc_resize_plan_build(*key[:4], ctypes.c_void_p(host.data_ptr())), "cc_resize_plan_build")
        plan = host.to(device)
        _RESIZE_PLANS[key] = plan
    return plan


# ------------------------------------------------------------------------------------------ frame ops
# Four operations - resize + centre crop, resized crop + flip and the two ragged collates - and a conversion, on three kinds of
# source.  A *source* (RGB, YUV420, YUV below) holds what differs between the kinds: how an op's arguments give the frames and
# the C entry's source arguments, what is checked about them, the shape of the result, what ``out`` may be and the names of the
# C entries.  An *operation* is written once, ``body(S, name, out, *args) -> (src, the result's shape, launch)``: every check,
# then the launch as a closure.  ``_frame_ops`` registers a body for a source; the allocating op, its ``_out`` twin and both
# fake kernels run that one body - the fake ones drop the launch - so a fake kernel checks exactly what its real kernel does.
COLLATE_ROW, COLLATE_BOX_ROW, COLLATE_MAX_PLANES = 6, 10, 4096      # CC_COLLATE_ROW / _BOX_ROW / _MAX_PLANES of the header
YUV_KINDS = {"i420": 0, "nv12": 1}                  # CC_YUV420_I420 / CC_YUV420_NV12
YUV_MATRICES = {"bt601": 0, "bt709": 1}             # CC_YUV_BT601 / CC_YUV_BT709
# YUV_FORMATS is THE table of what a name means; nothing else branches on names.
YUV_FORMATS = {                                     # name: (CC_YUV_* code, sub_x, sub_y, depth, shift, interleaved)
    "i420": (0, 1, 1, 8, 0, False), "nv12": (1, 1, 1, 8, 0, True), "i422": (2, 1, 0, 8, 0, False), "i444": (3, 0, 0, 8, 0, False),
    "i420p10": (4, 1, 1, 10, 0, False), "i422p10": (5, 1, 0, 10, 0, False), "i444p10": (6, 0, 0, 10, 0, False),
    "p010": (7, 1, 1, 10, 6, True), "i420p12": (8, 1, 1, 12, 0, False), "p012": (9, 1, 1, 12, 4, True),
    "p016": (10, 1, 1, 16, 0, True), "i444p16": (11, 0, 0, 16, 0, False)}
_YUV_WORDS = (torch.uint16, torch.int16)


def _pixels(n_rows, n_cols, chw):
    return (3, n_rows, n_cols) if chw else (n_rows, n_cols, 3)


def _fmt(chw):
    return 1 if chw else 2                          # cc_frames formats: uint8 CHW / uint8 HWC


def _resize_crop_shape(shape, n_px):
    chw, _, _ = _raw_frames_geometry(shape)
    return tuple(shape[:-3]) + _pixels(n_px, n_px, chw)


def _frames_out_check(name, out, shape):
    """The out-buffer rule of the YUV ops and of every collate: the result's frames under any leading dimensions (DeviceFeeder
    hands in its [B, 1, T, ...] slots)."""
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() < 3 or tuple(out.shape[-3:]) != shape[-3:] \
            or out.numel() != math.prod(shape):
        raise ValueError("%s: out must be contiguous uint8 frames [..., %s] with %d frames in all, got %s %s"
                         % (name, ", ".join(map(str, shape[-3:])), math.prod(shape[:-3]), out.dtype, tuple(out.shape)))


class _RgbSource:
    """uint8 RGB frames [..., H, W, 3] or [..., 3, H, W]: layout and leading dimensions are the tensor's, the result keeps both
    and ``out`` has exactly the result's shape.  Packed clips (the collates) say their layout with ``chw``."""
    schema = dict(frames="Tensor frames", chw="", colour="")
    entries = dict(resize_crop="cc_resize_crop_u8", crop_flip="cc_resized_crop_flip_u8", collate="cc_collate_resize_crop_u8",
                   collate_crop_flip="cc_collate_crop_flip_u8")

    def frames(self, name, frames, *rest):
        """An op's arguments -> (src, F, H, W, chw, the result's leading dimensions, layout, the op's own arguments)."""
        if frames.dtype != torch.uint8:
            raise ValueError("%s takes uint8 frames, got %s" % (name, frames.dtype))
        chw, H, W = _raw_frames_geometry(frames.shape)
        lead = tuple(frames.shape[:-3])
        return frames, math.prod(lead), H, W, chw, lead, None, rest

    def c_frames(self, src, F, H, W, chw, layout):
        """-> the source arguments every frame entry of this source begins with."""
        return L.ptr(src), _fmt(chw), F, H, W

    def out_check(self, name, out, shape):
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("%s: out must be a contiguous uint8 %s, got %s %s" % (name, shape, out.dtype, tuple(out.shape)))

    def colour(self, name, chw):
        """A collate's arguments behind ``resize`` / ``n_px`` -> (chw of the result, the C arguments between src_bytes and the clip
        table)."""
        return chw, (_fmt(chw),)


class _YuvSource:
    """Decoder planes as ANY contiguous tensor - its bytes are what the layout's offsets count in - with the geometry spelled
    out: F frames of H x W and ``layout``, the integers of the C descriptor ``struct`` in the order of its fields, all positions
    in BYTES.  uint8, or uint16 / int16 words with the same bits where the descriptor has a depth and it is over 8.  The result
    is [F, ...] in the layout ``chw`` asks for and ``out`` is any buffer of those frames.  Packed clips (the collates) are tight
    frames of one format, named by a code below ``n_codes``; there ``chw`` is the OUTPUT's layout."""
    out_check = staticmethod(_frames_out_check)

    def __init__(self, struct, layout_doc, code_arg, codes_doc, n_codes, entries):
        self.struct, self.layout_doc, self.codes_doc, self.n_codes, self.entries = struct, layout_doc, codes_doc, n_codes, entries
        self.fields = [field for field, _ in struct._fields_]
        self.depth_at = self.fields.index("depth") if "depth" in self.fields else None
        self.schema = dict(frames="Tensor src, SymInt F, SymInt H, SymInt W, SymInt[] layout", chw=", bool chw",
                           colour="SymInt %s, SymInt matrix, bool full_range, " % code_arg)

    def frames(self, name, src, F, H, W, layout, *rest):
        if len(layout) != len(self.fields):
            raise ValueError("%s: layout is the %s (%s), got %d values" % (name, self.layout_doc, ", ".join(self.fields), len(layout)))
        depth = 8 if self.depth_at is None else layout[self.depth_at]
        if src.dtype != torch.uint8 and not (src.dtype in _YUV_WORDS and depth > 8):
            raise ValueError("%s takes the decoder's planes as uint8 bytes or, for samples of more than 8 bits, uint16 / int16 words, "
                             "got %s at depth %d" % (name, src.dtype, depth))
        if F < 0 or H < 1 or W < 1:
            raise ValueError("%s: F >= 0 frames of H, W >= 1, got %d x %d x %d" % (name, F, H, W))
        return src, F, H, W, rest[-1], (F,), layout, rest[:-1]

    def c_frames(self, src, F, H, W, chw, layout):
        return L.ptr(src), src.numel() * src.element_size(), ctypes.byref(self.struct(*(int(v) for v in layout))), F, H, W

    def colour(self, name, code, matrix, full_range, chw):
        if not 0 <= code < self.n_codes or matrix not in (0, 1):
            raise ValueError("%s: %s and matrix 0 (BT.601) / 1 (BT.709), got %d, %d" % (name, self.codes_doc, code, matrix))
        return chw, (int(code), int(matrix), int(full_range))


RGB = _RgbSource()
# YUV 4:2:0 sources (include/centerclip_hip.h, "YUV 4:2:0 sources"): 8-bit samples, ``layout`` the eight integers of
# cc_yuv420_layout.  preprocess.py builds the tight layouts of a decoder's [..., 3H/2, W] arrays; a pitched or odd-sized surface
# is described by hand.  These ops keep the C entries of their own: the header folds them onto the general path.
YUV420 = _YuvSource(L.Yuv420Layout, "eight integers of cc_yuv420_layout", "kind", "kind 0 (tight I420) / 1 (tight NV12)", 2,
                    dict(to_rgb="cc_yuv420_to_rgb_u8", resize_crop="cc_resize_crop_yuv420_u8",
                         crop_flip="cc_resized_crop_flip_yuv420_u8", collate="cc_collate_resize_crop_yuv420_u8",
                         collate_crop_flip="cc_collate_crop_flip_yuv420_u8"))
# YUV sources in general (include/centerclip_hip.h, "YUV sources in general"): 4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar,
# samples of 8 bits or of 10 / 12 / 16 bits in 16-bit words; ``layout`` the twelve integers of cc_yuv_layout.
YUV = _YuvSource(L.YuvLayout, "twelve integers of cc_yuv_layout", "fmt",
                 "format 0 .. %d (the CC_YUV_* codes of YUV_FORMATS)" % (len(YUV_FORMATS) - 1), len(YUV_FORMATS),
                 dict(to_rgb="cc_yuv_to_rgb_u8", resize_crop="cc_resize_crop_yuv_u8", crop_flip="cc_resized_crop_flip_yuv_u8",
                      collate="cc_collate_resize_crop_yuv_u8", collate_crop_flip="cc_collate_crop_flip_yuv_u8"))


def _tight_layout(S, entry, codes, name, H, W, matrix, full_range):
    if name not in codes or matrix not in YUV_MATRICES:
        raise ValueError("a tight layout is one of %s and a matrix 'bt601' or 'bt709', got %r, %r" % (sorted(codes), name, matrix))
    lay = S.struct()
    if not getattr(L.lib(), entry)(codes[name], int(H), int(W), YUV_MATRICES[matrix], int(bool(full_range)), ctypes.byref(lay)):
        raise ValueError("no tight %s layout for %s x %s frames (1 .. 8192)" % (name, H, W))
    return [getattr(lay, field) for field in S.fields]


def yuv420_tight_layout(kind, H, W, matrix, full_range):
    """-> the eight integers of cc_yuv420_layout_tight for tight ``kind`` ("i420" / "nv12") frames of H x W one behind the
    other; [0] is the bytes of a frame, H W + 2 ceil(H / 2) ceil(W / 2)."""
    return _tight_layout(YUV420, "cc_yuv420_layout_tight", YUV_KINDS, kind, H, W, matrix, full_range)


def yuv_tight_layout(name, H, W, matrix, full_range):
    """-> the twelve integers of cc_yuv_layout_tight for tight frames of the named format, H x W, one behind the other; [0] is
    the bytes of a frame."""
    return _tight_layout(YUV, "cc_yuv_layout_tight", {k: v[0] for k, v in YUV_FORMATS.items()}, name, H, W, matrix, full_range)


def _to_rgb(S, name, out, *args):
    src, F, H, W, chw, lead, layout, _ = S.frames(name, *args)

    def launch(out):
        L.require_device(src)
        if F:
            s = src.contiguous()
            fn = S.entries["to_rgb"]
            L.check(getattr(L.lib(), fn)(*S.c_frames(s, F, H, W, chw, layout), L.ptr(out), _fmt(chw), _st(s)), fn)
    return src, lead + _pixels(H, W, chw), launch


def _resize_crop(S, name, out, *args):
    src, F, H, W, chw, lead, layout, (n_px, resize) = S.frames(name, *args)
    shape = lead + _pixels(n_px, n_px, chw)
    if out is not None:
        S.out_check(name, out, shape)

    def launch(out):
        L.require_device(src, out)
        if F == 0:
            return
        s = src.contiguous()
        lib, fn = L.lib(), S.entries["resize_crop"]
        plan = resize_plan(H, W, n_px, resize, s.device)
        nws = lib.cc_resize_crop_workspace_bytes(F, H, W, int(n_px), int(resize))
        ws = L.workspace(nws, s.device) if nws else None
        L.check(getattr(lib, fn)(*S.c_frames(s, F, H, W, chw, layout), L.ptr(plan), int(n_px), int(resize), L.ptr(out), _fmt(chw),
                                 L.ptr(ws), ws.numel() if ws is not None else 0, _st(s)), fn)
    return src, shape, launch


def _crop_flip(S, name, out, *args):
    src, F, H, W, chw, lead, layout, (boxes, n_px, frames_per_clip, interp) = S.frames(name, *args)
    if frames_per_clip < 1 or interp not in (0, 1) or n_px < 1:
        raise ValueError("%s: frames_per_clip >= 1, n_px >= 1 and interp 0 (bilinear) / 1 (bicubic), got %d, %d, %d"
                         % (name, frames_per_clip, n_px, interp))
    clips = -(-F // frames_per_clip)
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (clips, 5):
        raise ValueError("%s: boxes must be int32 [%d, 5] rows (top, left, height, width, flip) for %d frames in clips of %d, got "
                         "%s %s" % (name, clips, F, frames_per_clip, boxes.dtype, tuple(boxes.shape)))
    shape = lead + _pixels(n_px, n_px, chw)
    if out is not None:
        S.out_check(name, out, shape)

    def launch(out):
        L.require_device(src, boxes, out)
        if F == 0:
            return
        s, b = src.contiguous(), boxes.contiguous()
        fn = S.entries["crop_flip"]
        L.check(getattr(L.lib(), fn)(*S.c_frames(s, F, H, W, chw, layout), int(frames_per_clip), L.ptr(b), int(n_px), int(interp),
                                     L.ptr(out), _fmt(chw), _st(s)), fn)
    return src, shape, launch


def _collate_check(name, src, rows, clips, n_px, row_ints):
    """What the two ragged-batch ops check about their tables -> n_out."""
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError("%s: the packed clips are one 1-D uint8 buffer, got %s %s" % (name, src.dtype, tuple(src.shape)))
    if rows.dtype != torch.int64 or rows.dim() != 2 or rows.shape[1] != row_ints or rows.shape[0] < 1:
        raise ValueError("%s: the frame table is int64 [n_out >= 1, %d], got %s %s" % (name, row_ints, rows.dtype, tuple(rows.shape)))
    if len(clips) == 0 or len(clips) % 4:
        raise ValueError("%s: the clip table is B >= 1 rows of (byte offset, frames, H, W), got %d values" % (name, len(clips)))
    if n_px < 1:
        raise ValueError("%s: n_px >= 1, got %d" % (name, n_px))
    return int(rows.shape[0])


def _clips_host(clips):
    return (ctypes.c_int64 * len(clips))(*clips)


def _collate(S, name, out, src, rows, plans, clips, n_px, resize, *colour):
    chw, c_colour = S.colour(name, *colour)
    n_out = _collate_check(name, src, rows, clips, n_px, COLLATE_ROW)
    if plans.dtype != torch.int32 or plans.dim() != 1:
        raise ValueError("%s: the plans are one 1-D int32 buffer, got %s %s" % (name, plans.dtype, tuple(plans.shape)))
    shape = (n_out,) + _pixels(n_px, n_px, chw)
    if out is not None:
        _frames_out_check(name, out, shape)

    def launch(out):
        L.require_device(src, rows, plans, out)
        s, r, p, table = src.contiguous(), rows.contiguous(), plans.contiguous(), _clips_host(clips)
        lib, fn = L.lib(), S.entries["collate"]
        nws = lib.cc_collate_resize_crop_workspace_bytes(table, len(clips) // 4, n_out, int(n_px), int(resize))
        ws = L.workspace(nws, s.device) if nws else None
        L.check(getattr(lib, fn)(L.ptr(s), s.numel(), *c_colour, table, len(clips) // 4, L.ptr(r), n_out, L.ptr(p), p.numel(),
                                 int(n_px), int(resize), L.ptr(out), _fmt(chw), L.ptr(ws), nws, _st(s)), fn)
    return src, shape, launch


def _collate_crop_flip(S, name, out, src, rows, clips, n_px, *colour):
    chw, c_colour = S.colour(name, *colour)
    n_out = _collate_check(name, src, rows, clips, n_px, COLLATE_BOX_ROW)
    shape = (n_out,) + _pixels(n_px, n_px, chw)
    if out is not None:
        _frames_out_check(name, out, shape)

    def launch(out):
        L.require_device(src, rows, out)
        s, r = src.contiguous(), rows.contiguous()
        fn = S.entries["collate_crop_flip"]
        L.check(getattr(L.lib(), fn)(L.ptr(s), s.numel(), *c_colour, _clips_host(clips), len(clips) // 4, L.ptr(r), n_out,
                                     int(n_px), L.ptr(out), _fmt(chw), _st(s)), fn)
    return src, shape, launch


FRAME_OPS = []                                      # every name _frame_ops registered; OPS takes them from here


def _frame_ops(S, name, body, args, doc, out_doc=None):
    """Register ``body`` for the source S as centerclip::<name> - ``args``: the schema's arguments, {frames} / {chw} / {colour}
    standing for the source's - and, with ``out_doc``, as centerclip::<name>_out with a last argument ``out`` that is written
    instead of a fresh tensor.  -> the CustomOpDef, or the pair."""
    args = args.format(**S.schema)

    def alloc(*a):
        src, shape, launch = body(S, name, None, *a)
        out = _e(*shape, like=src, dtype=torch.uint8)
        launch(out)
        return out

    def alloc_fake(*a):
        src, shape, _ = body(S, name, None, *a)
        return src.new_empty(shape, dtype=torch.uint8)

    def into(*a):
        body(S, name, a[-1], *a[:-1])[2](a[-1])

    def into_fake(*a):
        body(S, name, a[-1], *a[:-1])

    alloc.__doc__, into.__doc__ = doc, out_doc
    plain = custom_op("%s::%s" % (NS, name), alloc, mutates_args=(), device_types="cuda", schema="(%s) -> Tensor" % args)
    plain.register_fake(alloc_fake)
    FRAME_OPS.append(name)
    if out_doc is None:
        return plain
    twin = custom_op("%s::%s_out" % (NS, name), into, mutates_args=("out",), device_types="cuda",
                     schema="(%s, Tensor(a%d!) out) -> ()" % (args, args.count(",") + 1))
    twin.register_fake(into_fake)
    FRAME_OPS.append(name + "_out")
    return plain, twin


_TO_RGB = (_to_rgb, "{frames}{chw}")
_RESIZE_CROP = (_resize_crop, "{frames}, SymInt n_px, bool resize{chw}")
_CROP_FLIP = (_crop_flip, "{frames}, Tensor boxes, SymInt n_px, SymInt frames_per_clip, SymInt interp{chw}")
_COLLATE = (_collate, "Tensor src, Tensor rows, Tensor plans, SymInt[] clips, SymInt n_px, bool resize, {colour}bool chw")
_COLLATE_CROP_FLIP = (_collate_crop_flip, "Tensor src, Tensor rows, SymInt[] clips, SymInt n_px, {colour}bool chw")

resize_center_crop, resize_center_crop_out = _frame_ops(
    RGB, "resize_center_crop", *_RESIZE_CROP,
    """The loader transform in front of the encoders (cc_resize_crop_u8): uint8 frames [..., H, W, 3] or [..., 3, H, W] of any
    size -> uint8 [..., n_px, n_px, 3] / [..., 3, n_px, n_px] (the input's layout), byte for byte Pillow's bicubic
    Resize(n_px) + CenterCrop(n_px) (dataloaders/rawvideo_util.py:16-23); resize=False: the crop alone.""",
    """resize_center_crop into a buffer of the caller's (DeviceFeeder: one per slot, so the addresses a hipGraph saw stay).""")
resized_crop_flip, resized_crop_flip_out = _frame_ops(
    RGB, "resized_crop_flip", *_CROP_FLIP,
    """Train-time augmentation (cc_resized_crop_flip_u8): uint8 frames [..., H, W, 3] or [..., 3, H, W] -> uint8
    [..., n_px, n_px, 3] / [..., 3, n_px, n_px] (the input's layout); the frames count in clips of frames_per_clip and clip i
    is cropped to boxes[i] = (top, left, height, width, flip) (int32, on the device - the kernel reads it, nothing is copied or
    read back), resized to n_px x n_px with interp 0 bilinear / 1 bicubic (F.interpolate, align_corners=False, no antialias,
    rounded to bytes) and mirrored where flip != 0.  A row outside the frame gives zeros for its clip.""",
    """resized_crop_flip into a buffer of the caller's (DeviceFeeder: one per slot, so the addresses a hipGraph saw stay).""")
collate_clips, collate_clips_out = _frame_ops(
    RGB, "collate_clips", *_COLLATE,
    """A ragged batch of decoded clips -> uniform frames (cc_collate_resize_crop_u8, at most two launches whatever the batch
    holds).  src: the packed uint8 bytes; clips: the HOST table, flat rows (byte offset, frames, H, W) - what is checked before
    any launch; rows: int64 [n_out, 6] on the device, per output frame (kind 0 zero / 1 transform, byte offset, H, W, int32 offset
    of the size's plan in ``plans``, byte offset of the frame's horizontal result in the workspace = i * the per-frame share of
    cc_collate_resize_crop_workspace_bytes).  -> uint8 [n_out, n_px, n_px, 3] ([n_out, 3, n_px, n_px] with chw), each frame byte
    for byte resize_center_crop of its source frame, zero frames zero.  preprocess.ClipCollate builds the tables.""",
    """collate_clips into a buffer of the caller's (DeviceFeeder: one per slot, so the addresses a hipGraph saw stay); every
    frame of it is written, the zero frames included.""")
collate_clips_crop_flip, collate_clips_crop_flip_out = _frame_ops(
    RGB, "collate_clips_crop_flip", *_COLLATE_CROP_FLIP,
    """The training form of collate_clips (cc_collate_crop_flip_u8, one launch): rows int64 [n_out, 10] on the device, per output
    frame (kind, byte offset, H, W, top, left, height, width, flip, interp 0 bilinear / 1 bicubic); each frame byte for byte
    resized_crop_flip of its source frame with that box, zero frames zero.""",
    """collate_clips_crop_flip into a buffer of the caller's; every frame of it is written.""")

yuv420_to_rgb = _frame_ops(
    YUV420, "yuv420_to_rgb", *_TO_RGB,
    """The conversion alone (cc_yuv420_to_rgb_u8, one launch): F frames of H x W 8-bit 4:2:0 in ``src`` as ``layout`` describes
    -> uint8 [F, H, W, 3] ([F, 3, H, W] with chw), the fixed integer conversion of the header, chroma replicated.""")
resize_center_crop_yuv420, resize_center_crop_yuv420_out = _frame_ops(
    YUV420, "resize_center_crop_yuv420", *_RESIZE_CROP,
    """resize_center_crop on a 4:2:0 source (cc_resize_crop_yuv420_u8): -> uint8 [F, n_px, n_px, 3] ([F, 3, n_px, n_px] with chw),
    bit for bit resize_center_crop(yuv420_to_rgb(src)); the first pass converts its taps, no RGB frame of H x W is stored.""",
    """resize_center_crop_yuv420 into a buffer of the caller's.""")
resized_crop_flip_yuv420, resized_crop_flip_yuv420_out = _frame_ops(
    YUV420, "resized_crop_flip_yuv420", *_CROP_FLIP,
    """resized_crop_flip on a 4:2:0 source (cc_resized_crop_flip_yuv420_u8, one launch): bit for bit
    resized_crop_flip(yuv420_to_rgb(src), boxes, ...).""",
    """resized_crop_flip_yuv420 into a buffer of the caller's.""")
collate_clips_yuv420, collate_clips_yuv420_out = _frame_ops(
    YUV420, "collate_clips_yuv420", *_COLLATE,
    """collate_clips on packed tight 4:2:0 frames (cc_collate_resize_crop_yuv420_u8): the same tables, byte offsets counting
    frames of H W + 2 ceil(H / 2) ceil(W / 2) bytes; kind 0 I420 / 1 NV12; chw: the OUTPUT's layout.""",
    """collate_clips_yuv420 into a buffer of the caller's; every frame of it is written.""")
collate_clips_crop_flip_yuv420, collate_clips_crop_flip_yuv420_out = _frame_ops(
    YUV420, "collate_clips_crop_flip_yuv420", *_COLLATE_CROP_FLIP,
    """collate_clips_crop_flip on packed tight 4:2:0 frames (cc_collate_crop_flip_yuv420_u8, one launch).""",
    """collate_clips_crop_flip_yuv420 into a buffer of the caller's; every frame of it is written.""")

yuv_to_rgb = _frame_ops(
    YUV, "yuv_to_rgb", *_TO_RGB,
    """The conversion alone (cc_yuv_to_rgb_u8, one launch): F frames of H x W in ``src`` as ``layout`` describes -> uint8
    [F, H, W, 3] ([F, 3, H, W] with chw), the fixed integer conversion of the header for the layout's depth, chroma replicated.""")
resize_center_crop_yuv, resize_center_crop_yuv_out = _frame_ops(
    YUV, "resize_center_crop_yuv", *_RESIZE_CROP,
    """resize_center_crop on a YUV source (cc_resize_crop_yuv_u8): -> uint8 [F, n_px, n_px, 3] ([F, 3, n_px, n_px] with chw), bit
    for bit resize_center_crop(yuv_to_rgb(src)); the first pass converts its taps, no RGB frame of H x W is stored.""",
    """resize_center_crop_yuv into a buffer of the caller's.""")
resized_crop_flip_yuv, resized_crop_flip_yuv_out = _frame_ops(
    YUV, "resized_crop_flip_yuv", *_CROP_FLIP,
    """resized_crop_flip on a YUV source (cc_resized_crop_flip_yuv_u8, one launch): bit for bit
    resized_crop_flip(yuv_to_rgb(src), boxes, ...).""",
    """resized_crop_flip_yuv into a buffer of the caller's.""")
collate_clips_yuv, collate_clips_yuv_out = _frame_ops(
    YUV, "collate_clips_yuv", *_COLLATE,
    """collate_clips on packed tight YUV frames of one named format (cc_collate_resize_crop_yuv_u8): the same tables, byte
    offsets counting tight frames of that format (even for 16-bit samples); fmt: the CC_YUV_* code; chw: the OUTPUT's layout.""",
    """collate_clips_yuv into a buffer of the caller's; every frame of it is written.""")
collate_clips_crop_flip_yuv, collate_clips_crop_flip_yuv_out = _frame_ops(
    YUV, "collate_clips_crop_flip_yuv", *_COLLATE_CROP_FLIP,
    """collate_clips_crop_flip on packed tight YUV frames of one named format (cc_collate_crop_flip_yuv_u8, one launch).""",
    """collate_clips_crop_flip_yuv into a buffer of the caller's; every frame of it is written.""")


@custom_op(NS + "::clip_encode_out", mutates_args=("vfeat", "tfeat", "medoids_out"), device_types="cuda")
def clip_encode_out(frames: torch.Tensor, ids: torch.Tensor, vhandle: int, thandle: int, B: int, T: int,
                    vfeat: torch.Tensor, tfeat: torch.Tensor, medoids_out: Optional[torch.Tensor],
                    forced_medoids: Optional[torch.Tensor]) -> None:
    """Both towers of one CLIP4Clip.forward call in a single enqueue (modules/clip4clip.py:199-243); the features are
    written into caller-owned contiguous buffers (e.g. slices of the packed all-gather record).  medoids_out / forced_medoids:
    the ids of the last k-medoids block, reported / imposed (test hook, see cc_vit_encode)."""
    from .clip import frames_descriptor
    vm, vmeta, _k0 = _model(vhandle)
    tm, tmeta, _k1 = _model(thandle)
    fr, frames = frames_descriptor(frames)
    Bt, Lt = ids.shape
    lib = L.lib()
    _check_forced_medoids(lib, vm, B, forced_medoids)
    # (caller-owned outputs reach the library as bare pointers)
    frames_out, _ltok, med_shape = vmeta["final"](T)
    if (vfeat.dtype != torch.float32 or not vfeat.is_contiguous() or vfeat.numel() != B * frames_out * vmeta["embed_dim"]
            or tfeat.dtype != torch.float32 or not tfeat.is_contiguous() or tfeat.numel() != Bt * tmeta["embed_dim"]):
        raise ValueError("clip_encode_out: vfeat [B * %d, %d] and tfeat [%d, %d] contiguous fp32 expected"
                         % (frames_out, vmeta["embed_dim"], Bt, tmeta["embed_dim"]))
    if medoids_out is not None and (med_shape is None or medoids_out.dtype != torch.long or not medoids_out.is_contiguous()
                                    or medoids_out.numel() != B * med_shape[0] * med_shape[1]):
        raise ValueError("clip_encode_out: medoids_out = the last k-medoids block's [B * T_new, K] int64 ids")
    ws = L.workspace(lib.cc_clip_workspace_bytes(ctypes.byref(vm), B, T, ctypes.byref(tm), Bt, Lt), frames.device)
    L.check(lib.cc_clip_encode_frames(ctypes.byref(vm), ctypes.byref(fr), B, T, L.ptr(vfeat), L.ptr(medoids_out),
                                      L.ptr(forced_medoids), ctypes.byref(tm), L.ptr(ids), Bt, Lt, L.ptr(tfeat), L.ptr(ws),
                                      ws.numel(), _st(frames)), "cc_clip_encode_frames")


@clip_encode_out.register_fake
def _(frames, ids, vhandle, thandle, B, T, vfeat, tfeat, medoids_out, forced_medoids):
    return None


@custom_op(NS + "::clip_encode", mutates_args=(), device_types="cuda")
def clip_encode(frames: torch.Tensor, ids: torch.Tensor, vhandle: int, thandle: int, B: int,
                T: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _vm, vmeta, _k0 = _model(vhandle)
    frames_out, _ltok, _med = vmeta["final"](T)
    vfeat = torch.empty(B * frames_out, vmeta["embed_dim"], device=frames.device, dtype=torch.float32)
    tfeat = torch.empty(ids.shape[0], vmeta["embed_dim"], device=frames.device, dtype=torch.float32)
    torch.ops.centerclip.clip_encode_out(frames, ids, vhandle, thandle, B, T, vfeat, tfeat, None, None)
    return vfeat, tfeat


@clip_encode.register_fake
def _(frames, ids, vhandle, thandle, B, T):
    _vm, vmeta, _k0 = _model(vhandle)
    frames_out, _ltok, _med = vmeta["final"](T)
    return (frames.new_empty((B * frames_out, vmeta["embed_dim"]), dtype=torch.float32),
            frames.new_empty((ids.shape[0], vmeta["embed_dim"]), dtype=torch.float32))


# ------------------------------------------------------------------------------------------ similarity tail / metrics
@custom_op(NS + "::loose_similarity", mutates_args=(), device_types="cuda")
def loose_similarity(text: torch.Tensor, visual: torch.Tensor, video_mask: torch.Tensor, logit_scale: float, group: int,
                     vis_group_stride: int, mask_group_stride: int, Bv: int, Tn: int,
                     want_pooled: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """CLIP4Clip._loose_similarity, meanP (modules/clip4clip.py:305-316,357-366): text [Bt,E] fp32, visual fp32 holding
    Bv videos of Tn frames (plain [Bv,Tn,E], or records of `group` videos every vis_group_stride floats), video_mask
    int64 (a strided [Bv,Tn] view, or records every mask_group_stride elements) -> (logits [Bt,Bv], pooled [Bv,E] or
    empty)."""
    Bt, E = text.shape
    lib = L.lib()
    logits = _e(Bt, Bv, like=text, dtype=torch.float32)
    pooled = _e(Bv if want_pooled else 0, E, like=text, dtype=torch.float32)
    ws = L.workspace(lib.cc_similarity_workspace_bytes(Bt, Bv, E), text.device)
    if video_mask.dim() == 2:
        mrs, mcs = video_mask.stride(0), video_mask.stride(1)
    else:                                    # flat record buffer: rows of Tn mask entries inside each record
        mrs, mcs = Tn, 1
    L.check(lib.cc_loose_similarity_grouped_f32(L.ptr(text), L.ptr(visual), L.ptr(video_mask), int(group),
                                                int(vis_group_stride), int(mask_group_stride), mrs, mcs, Bt, Bv, Tn, E,
                                                float(logit_scale), L.ptr(logits), Bv,
                                                L.ptr(pooled) if want_pooled else None, L.ptr(ws), ws.numel(), _st(text)),
            "cc_loose_similarity_grouped_f32")
    return logits, pooled


@loose_similarity.register_fake
def _(text, visual, video_mask, logit_scale, group, vis_group_stride, mask_group_stride, Bv, Tn, want_pooled):
    Bt, E = text.shape
    return text.new_empty((Bt, Bv)), text.new_empty((Bv if want_pooled else 0, E))


@custom_op(NS + "::video_pool_normalize", mutates_args=(), device_types="cuda")
def video_pool_normalize(visual: torch.Tensor, video_mask: torch.Tensor) -> torch.Tensor:
    Bv, Tn, E = visual.shape
    pooled = _e(Bv, E, like=visual, dtype=torch.float32)
    L.check(L.lib().cc_video_pool_normalize_f32(L.ptr(visual), L.ptr(video_mask), Bv, Tn, E, L.ptr(pooled), _st(visual)),
            "cc_video_pool_normalize_f32")
    return pooled


@video_pool_normalize.register_fake
def _(visual, video_mask):
    return visual.new_empty((visual.shape[0], visual.shape[2]))


@custom_op(NS + "::normalize_rows", mutates_args=(), device_types="cuda")
def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    R, E = x.shape
    out = torch.empty_like(x)
    L.check(L.lib().cc_normalize_rows_f32(L.ptr(x), L.ptr(out), R, E, _st(x)), "cc_normalize_rows_f32")
    return out


@normalize_rows.register_fake
def _(x):
    return torch.empty_like(x)


@custom_op(NS + "::normalize_rows_planes", mutates_args=(), device_types="cuda")
def normalize_rows_planes(x: torch.Tensor, video_side: bool) -> torch.Tensor:
    """rows / |row| written as the split-fp16 planes the similarity GEMM multiplies: [R, 3E] fp16 (text side [hi|hi|lo],
    video side [hi|lo|hi]) - the operand of scaled_dot_planes, produced when a batch is encoded."""
    R, E = x.shape
    planes = _e(R, 3 * E, like=x, dtype=torch.float16)
    L.check(L.lib().cc_normalize_rows_planes_f32(L.ptr(x), None, L.ptr(planes), int(video_side), R, E, _st(x)),
            "cc_normalize_rows_planes_f32")
    return planes


@normalize_rows_planes.register_fake
def _(x, video_side):
    return x.new_empty((x.shape[0], 3 * x.shape[1]), dtype=torch.float16)


@custom_op(NS + "::video_pool_normalize_planes", mutates_args=(), device_types="cuda")
def video_pool_normalize_planes(visual: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """_mean_pooling_for_similarity_visual + the final normalisation (clip4clip.py:305-316,357-360) -> video-side planes
    [Bv, 3E] fp16."""
    Bv, Tn, E = visual.shape
    planes = _e(Bv, 3 * E, like=visual, dtype=torch.float16)
    L.check(L.lib().cc_video_pool_normalize_planes_f32(L.ptr(visual), L.ptr(mask), Bv, Tn, E, None, L.ptr(planes), _st(visual)),
            "cc_video_pool_normalize_planes_f32")
    return planes


@video_pool_normalize_planes.register_fake
def _(visual, mask):
    return visual.new_empty((visual.shape[0], 3 * visual.shape[2]), dtype=torch.float16)


@custom_op(NS + "::video_window_pool_planes", mutates_args=(), device_types="cuda")
def video_window_pool_planes(visual: torch.Tensor, windows: torch.Tensor) -> torch.Tensor:
    """The windows of long videos: visual [Bv, S, E] fp32 per-segment features, windows [nW, 3] int32 on the device =
    (video, start segment, stop segment) -> video-side planes [nW, 3E] fp16, row w = video_pool_normalize_planes of the
    segments [start, stop) of that video with a mask of ones, bit for bit.  An entry outside the tensor gives a zero row."""
    Bv, S, E = visual.shape
    nW = windows.shape[0]
    if (visual.dtype != torch.float32 or not visual.is_contiguous() or windows.dtype != torch.int32 or windows.dim() != 2
            or windows.shape[1] != 3 or not windows.is_contiguous() or windows.device != visual.device):
        raise ValueError("video_window_pool_planes: visual is contiguous fp32 [Bv, S, E] and windows contiguous int32 [nW, 3] "
                         "on its device, not %s %s and %s %s on %s" % (visual.dtype, tuple(visual.shape), windows.dtype,
                                                                       tuple(windows.shape), windows.device))
    planes = _e(nW, 3 * E, like=visual, dtype=torch.float16)
    L.check(L.lib().cc_video_window_pool_planes_f32(L.ptr(visual), L.ptr(windows), Bv, S, nW, E, L.ptr(planes), _st(visual)),
            "cc_video_window_pool_planes_f32")
    return planes


@video_window_pool_planes.register_fake
def _(visual, windows):
    return visual.new_empty((windows.shape[0], 3 * visual.shape[2]), dtype=torch.float16)


@custom_op(NS + "::scaled_dot_planes", mutates_args=(), device_types="cuda")
def scaled_dot_planes(text_planes: torch.Tensor, video_planes: torch.Tensor, n_video: int, mult: float,
                      products: int = 3) -> torch.Tensor:
    """[Bt, n_video] = mult * text . video^T from the planes: the GEMM launch alone.  video_planes holds at least
    padded_video_rows(n_video) rows, zeros behind n_video.  products: 3 (default: both operands to 22 bits), 2 (the text
    side rounded to fp16) or 1 (both sides fp16) of the three fp16 products per multiply-add - see cc_scaled_dot_planes_products_f32."""
    Bt, E3 = text_planes.shape
    out = _e(Bt, int(n_video), like=text_planes, dtype=torch.float32)
    L.check(L.lib().cc_scaled_dot_planes_products_f32(L.ptr(text_planes), L.ptr(video_planes), Bt, int(n_video),
                                                      video_planes.shape[0], E3 // 3, float(mult), int(products), L.ptr(out),
                                                      int(n_video), _st(text_planes)), "cc_scaled_dot_planes_products_f32")
    return out


@scaled_dot_planes.register_fake
def _(text_planes, video_planes, n_video, mult, products=3):
    return text_planes.new_empty((text_planes.shape[0], n_video), dtype=torch.float32)


@custom_op(NS + "::similarity_topk", mutates_args=(), device_types="cuda")
def similarity_topk(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                    k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best of the first n_gallery rows of gallery_planes for every row of query_planes -> (scores [Bq, k] fp32, ids
    [Bq, k] int64): the first k entries of the stable descending sort of the row scaled_dot_planes gives for the same planes
    (same bits; equal scores by smaller id; (-inf, -1) beyond n_gallery), without that matrix.  The gallery needs no padding
    rows.  1 <= k <= 128.  cc_similarity_topk_planes_f32."""
    return _topk("similarity_topk", query_planes, gallery_planes, n_gallery, mult, products, k)


@similarity_topk.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k):
    return _topk_fake("similarity_topk", query_planes, gallery_planes, n_gallery, k)


def _check_plane_pair(name, a, b, rows_b):
    E3 = a.shape[1]
    if b.dim() != 2 or b.shape[1] != E3 or b.shape[0] < int(rows_b):
        raise ValueError("%s: planes %s do not hold %d rows of %d halfs" % (name, tuple(b.shape), int(rows_b), E3))
    if a.dtype != torch.float16 or b.dtype != torch.float16:
        raise ValueError("%s: plane rows are fp16" % name)
    return E3


@custom_op(NS + "::dsl_col_stats_planes", mutates_args=(), device_types="cuda")
def dsl_col_stats_planes(text_planes: torch.Tensor, video_planes: torch.Tensor, n_text: int, n_video: int, mult: float,
                         products: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """camoe_dsl without the matrix: (m [n_video], s [n_video]) = dsl_col_stats of the matrix scaled_dot_planes gives for the
    first n_text text rows and the first n_video video rows (m bit-equal; s in a fixed order that depends on n_text alone, so a
    video row's pair is the same bits whichever rows share the call).  Neither side needs padding rows.  n_text == 0 gives
    (-inf, 0).  cc_dsl_col_stats_planes_f32."""
    E3 = _check_plane_pair("dsl_col_stats_planes", video_planes, text_planes, n_text)
    if video_planes.dim() != 2 or video_planes.shape[0] < int(n_video):
        raise ValueError("dsl_col_stats_planes: video planes %s do not hold %d rows" % (tuple(video_planes.shape), int(n_video)))
    text_planes, video_planes = text_planes.contiguous(), video_planes.contiguous()
    m = _e(int(n_video), like=video_planes, dtype=torch.float32)
    s = _e(int(n_video), like=video_planes, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_dsl_col_stats_planes_workspace_bytes(int(n_text), int(n_video)), video_planes.device)
    L.check(lib.cc_dsl_col_stats_planes_f32(L.ptr(text_planes), L.ptr(video_planes), int(n_text), int(n_video), E3 // 3,
                                            float(mult), int(products), L.ptr(m), L.ptr(s), L.ptr(ws), ws.numel(),
                                            _st(video_planes)), "cc_dsl_col_stats_planes_f32")
    return m, s


@dsl_col_stats_planes.register_fake
def _(text_planes, video_planes, n_text, n_video, mult, products):
    return (video_planes.new_empty((n_video,), dtype=torch.float32), video_planes.new_empty((n_video,), dtype=torch.float32))


@custom_op(NS + "::similarity_topk_dsl", mutates_args=(), device_types="cuda")
def similarity_topk_dsl(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                        k: int, m: torch.Tensor, s: torch.Tensor, stats_on_gallery: int,
                        n_total: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity_topk ranking the dual softmax D = n_total * S * exp(S - m[x]) / s[x] instead of S: x is the gallery row
    (stats_on_gallery = 1: m, s hold at least n_gallery entries) or the query row (0: m, s [Bq]).  A score has the bits dsl_apply_
    writes over scaled_dot_planes' entry; order, fill and limits are similarity_topk's.  cc_similarity_topk_dsl_planes_f32."""
    return _topk("similarity_topk_dsl", query_planes, gallery_planes, n_gallery, mult, products, k, m=m, s=s,
                 stats_on_gallery=stats_on_gallery, n_total=n_total)


@similarity_topk_dsl.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k, m, s, stats_on_gallery, n_total):
    return _topk_fake("similarity_topk_dsl", query_planes, gallery_planes, n_gallery, k, m=m, s=s, stats_on_gallery=stats_on_gallery)


def _check_group_head(name, query_planes, gallery_planes, n_gallery, group_head):
    """the planes and the heads of a grouped search (the fake kernels run it too: every refusal is an op-level ValueError)"""
    E3 = _check_plane_pair(name, query_planes, gallery_planes, n_gallery)
    if (group_head.dtype != torch.int32 or group_head.dim() != 1 or not group_head.is_contiguous()
            or group_head.shape[0] < int(n_gallery)):
        raise ValueError("%s: group_head %s %s is not a contiguous int32 vector of at least %d entries"
                         % (name, tuple(group_head.shape), group_head.dtype, int(n_gallery)))
    if group_head.device != gallery_planes.device or query_planes.device != gallery_planes.device:
        raise ValueError("%s: group_head on %s, the planes on %s and %s" % (name, group_head.device, query_planes.device,
                                                                        gallery_planes.device))
    return E3


def _check_dsl_stats(name, m, s, need):
    if m.dim() != 1 or s.dim() != 1 or m.shape[0] < need or s.shape[0] < need or m.dtype != torch.float32 or s.dtype != torch.float32:
        raise ValueError("%s: m %s, s %s are not fp32 vectors of at least %d entries" % (name, tuple(m.shape), tuple(s.shape), need))


@custom_op(NS + "::similarity_topk_grouped", mutates_args=(), device_types="cuda")
def similarity_topk_grouped(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                            k: int, group_head: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity_topk over GROUPS of adjacent gallery rows, each by its best row: group_head [>= n_gallery] int32 holds the
    first row of every row's group.  -> (scores [Bq, k] fp32, ids [Bq, k] int64): of similarity_topk's row order the first k
    rows that are the first of their group to appear - entry i is the best row of the i-th best group; (-inf, -1) beyond the
    number of groups.  group_head = arange gives similarity_topk bit for bit.  cc_similarity_topk_grouped_planes_f32."""
    return _topk("similarity_topk_grouped", query_planes, gallery_planes, n_gallery, mult, products, k, group_head=group_head)


@similarity_topk_grouped.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k, group_head):
    return _topk_fake("similarity_topk_grouped", query_planes, gallery_planes, n_gallery, k, group_head=group_head)


@custom_op(NS + "::similarity_topk_grouped_dsl", mutates_args=(), device_types="cuda")
def similarity_topk_grouped_dsl(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float,
                                products: int, k: int, m: torch.Tensor, s: torch.Tensor, stats_on_gallery: int, n_total: int,
                                group_head: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity_topk_grouped ranking the dual softmax D of similarity_topk_dsl (same m, s, stats_on_gallery, n_total): a
    group's score is the largest D of its rows.  cc_similarity_topk_grouped_dsl_planes_f32."""
    return _topk("similarity_topk_grouped_dsl", query_planes, gallery_planes, n_gallery, mult, products, k, m=m, s=s,
                 stats_on_gallery=stats_on_gallery, n_total=n_total, group_head=group_head)


@similarity_topk_grouped_dsl.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k, m, s, stats_on_gallery, n_total, group_head):
    return _topk_fake("similarity_topk_grouped_dsl", query_planes, gallery_planes, n_gallery, k, m=m, s=s,
                      stats_on_gallery=stats_on_gallery, group_head=group_head)


def mask_words(n):
    """int32 words of a row mask over n rows (bit b of word w = row 32 w + b)"""
    return (int(n) + 31) // 32


def _check_row_mask(name, mask, rows, n, planes, what="row_mask"):
    """a row mask: int32, contiguous, [W] or - rows given - [rows, W] with W >= ceil(n / 32), on the planes' device"""
    shapes = "[W]" if rows is None else "[W] or [%d, W]" % rows
    if (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.dim() not in ((1,) if rows is None else (1, 2))
            or (mask.dim() == 2 and mask.shape[0] != rows) or mask.shape[-1] < mask_words(n)):
        raise ValueError("%s: %s %s %s is not a contiguous int32 mask %s of W >= %d words"
                         % (name, what, tuple(mask.shape), mask.dtype, shapes, mask_words(n)))
    if mask.device != planes.device:
        raise ValueError("%s: %s on %s, the planes on %s" % (name, what, mask.device, planes.device))


def _check_search(name, query_planes, gallery_planes, n_gallery, row_mask, m, s, stats_on_gallery, group_head):
    """the planes and the optional parts of a search request - row mask, dual-softmax statistics, group heads - for every
    top-k, rank, target-score and count op (the fake kernels run it too: every refusal is an op-level ValueError)"""
    if group_head is not None:
        E3 = _check_group_head(name, query_planes, gallery_planes, n_gallery, group_head)
    else:
        E3 = _check_plane_pair(name, query_planes, gallery_planes, n_gallery)
    if query_planes.device != gallery_planes.device:
        raise ValueError("%s: the planes on %s and %s" % (name, query_planes.device, gallery_planes.device))
    if (m is None) != (s is None):
        raise ValueError("%s: m and s come together (both for the dual softmax, neither for S)" % name)
    if m is not None:
        _check_dsl_stats(name, m, s, int(n_gallery) if stats_on_gallery else query_planes.shape[0])
    if row_mask is not None:
        _check_row_mask(name, row_mask, query_planes.shape[0], n_gallery, gallery_planes)
    return E3


TOPK_DEEP_MAXK = 4096          # CC_TOPK_DEEP_MAXK
# the optional parts the C entry of every top-k op takes, in its argument order, between k and the outputs
_TOPK_PARTS = {"similarity_topk": (), "similarity_topk_dsl": ("stats",), "similarity_topk_grouped": ("heads",),
               "similarity_topk_grouped_dsl": ("stats", "heads"), "similarity_topk_masked": ("mask", "stats", "heads"),
               "similarity_topk_deep": ("mask", "stats", "heads", "cursor")}


def _mask_args(row_mask, Bq):
    """an optional row mask -> the (pointer, mask_rows, mask_words) of the C entries"""
    if row_mask is None:
        return L.ptr(None), 0, 0
    return L.ptr(row_mask), 1 if row_mask.dim() == 1 else Bq, int(row_mask.shape[-1])


def _contiguous_stats(m, s):
    return (m, s) if m is None else (m.contiguous(), s.contiguous())


def _check_topk(name, query_planes, gallery_planes, n_gallery, k, row_mask=None, m=None, s=None, stats_on_gallery=1,
                group_head=None, after_scores=None, after_ids=None):
    """_check_search and, for similarity_topk_deep, k and the cursor: both tensors or neither, one fp32 score and one int32 /
    int64 id per query row on the planes' device"""
    E3 = _check_search(name, query_planes, gallery_planes, n_gallery, row_mask, m, s, stats_on_gallery, group_head)
    if name != "similarity_topk_deep":
        return E3
    if not 1 <= int(k) <= TOPK_DEEP_MAXK:
        raise ValueError("%s: 1 <= k <= %d, not %d" % (name, TOPK_DEEP_MAXK, int(k)))
    if (after_scores is None) != (after_ids is None):
        raise ValueError("%s: after_scores and after_ids come together" % name)
    if after_scores is not None:
        Bq = query_planes.shape[0]
        if (after_scores.dtype != torch.float32 or after_ids.dtype not in (torch.int32, torch.int64)
                or tuple(after_scores.shape) != (Bq,) or tuple(after_ids.shape) != (Bq,)
                or after_scores.device != query_planes.device or after_ids.device != query_planes.device):
            raise ValueError("%s: after_scores %s %s on %s, after_ids %s %s on %s are not one fp32 score and one int32 / int64 id "
                             "per query row (%d) on %s" % (name, tuple(after_scores.shape), after_scores.dtype, after_scores.device,
                                                          tuple(after_ids.shape), after_ids.dtype, after_ids.device, Bq,
                                                          query_planes.device))
    return E3


def _topk(name, query_planes, gallery_planes, n_gallery, mult, products, k, row_mask=None, m=None, s=None, stats_on_gallery=1,
          n_total=0, group_head=None, after_scores=None, after_ids=None):
    """The body of the six top-k ops: check, allocate scores / ids, size the workspace, call the C entry cc_<name>_planes_f32
    with the parts _TOPK_PARTS names, ids to int64."""
    Bq, deep = query_planes.shape[0], name == "similarity_topk_deep"
    E3 = _check_topk(name, query_planes, gallery_planes, n_gallery, k, row_mask, m, s, stats_on_gallery, group_head, after_scores,
                     after_ids)
    scores = _e(Bq, int(k), like=query_planes, dtype=torch.float32)
    ids = _e(Bq, int(k), like=query_planes, dtype=torch.int32)
    if deep and (Bq == 0 or int(n_gallery) == 0):           # no row: nothing to rank
        return scores.fill_(float("-inf")), ids.fill_(-1).to(torch.int64)
    query_planes, gallery_planes = query_planes.contiguous(), gallery_planes.contiguous()
    m, s = _contiguous_stats(m, s)
    if after_scores is not None:
        after_scores, after_ids = after_scores.contiguous(), after_ids.to(torch.int32).contiguous()
    parts = {"mask": _mask_args(row_mask, Bq), "stats": (L.ptr(m), L.ptr(s), int(stats_on_gallery), int(n_total)),
             "heads": (L.ptr(group_head),), "cursor": (L.ptr(after_scores), L.ptr(after_ids))}
    lib, entry = L.lib(), "cc_%s_planes_f32" % name
    if deep:
        nbytes = lib.cc_similarity_topk_deep_workspace_bytes(Bq, int(n_gallery), E3 // 3, int(products), int(k))
    else:
        nbytes = lib.cc_similarity_topk_workspace_bytes(Bq, int(n_gallery), int(k))
    ws = L.workspace(nbytes, query_planes.device)
    L.check(getattr(lib, entry)(L.ptr(query_planes), L.ptr(gallery_planes), Bq, int(n_gallery), E3 // 3, float(mult), int(products),
                                int(k), *(a for part in _TOPK_PARTS[name] for a in parts[part]), L.ptr(scores), L.ptr(ids),
                                L.ptr(ws), ws.numel(), _st(query_planes)), entry)
    return scores, ids.to(torch.int64)


def _topk_fake(name, query_planes, gallery_planes, n_gallery, k, **parts):
    _check_topk(name, query_planes, gallery_planes, n_gallery, k, **parts)
    return (query_planes.new_empty((query_planes.shape[0], k), dtype=torch.float32),
            query_planes.new_empty((query_planes.shape[0], k), dtype=torch.int64))


@custom_op(NS + "::similarity_topk_masked", mutates_args=(), device_types="cuda")
def similarity_topk_masked(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                           k: int, row_mask: torch.Tensor, m: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None,
                           stats_on_gallery: int = 1, n_total: int = 0,
                           group_head: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity_topk (m, s: similarity_topk_dsl; group_head: the grouped ops) over the gallery rows whose bit is set in
    row_mask: int32 words, bit b of word w = row 32 w + b; [W] - one mask for all queries, tiles of 16 rows without a set bit
    are not even read - or [Bq, W], one mask per query row; W >= ceil(n_gallery / 32), bits at or above n_gallery are ignored.
    The result is the unmasked op's with the other rows left out (same bits, same order, ids of the whole gallery; the fill
    starts behind the selectable rows or groups - a group is ranked by its best selectable row).
    cc_similarity_topk_masked_planes_f32."""
    return _topk("similarity_topk_masked", query_planes, gallery_planes, n_gallery, mult, products, k, row_mask, m, s, stats_on_gallery,
                 n_total, group_head)


@similarity_topk_masked.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k, row_mask, m=None, s=None, stats_on_gallery=1, n_total=0,
      group_head=None):
    return _topk_fake("similarity_topk_masked", query_planes, gallery_planes, n_gallery, k, row_mask=row_mask, m=m, s=s,
                      stats_on_gallery=stats_on_gallery, group_head=group_head)


@custom_op(NS + "::similarity_topk_deep", mutates_args=(), device_types="cuda")
def similarity_topk_deep(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                         k: int, row_mask: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                         s: Optional[torch.Tensor] = None, stats_on_gallery: int = 1, n_total: int = 0,
                         group_head: Optional[torch.Tensor] = None, after_scores: Optional[torch.Tensor] = None,
                         after_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """similarity_topk_masked (row_mask optional here) for lists beyond 128 and for cursors: 1 <= k <= 4096 -> (scores [Bq, k]
    fp32, ids [Bq, k] int64), the first k entries of the same ordering with the same bits.  after_scores [Bq] fp32 and
    after_ids [Bq] int32 / int64 (both or neither; typically scores[:, -1], ids[:, -1] of an earlier result): the list starts
    behind that entry of the ordering - k = a, then k = b after its last column, are columns [0, a) and [a, a + b) of k = a + b;
    an id < 0 (the fill) gives the fill.  Built in pages of at most 128 entries, each one pass over the gallery restricted to
    the keys below the page before; the pages hand over on the device (no host read).  n_gallery == 0 gives the fill without a
    launch.  cc_similarity_topk_deep_planes_f32."""
    return _topk("similarity_topk_deep", query_planes, gallery_planes, n_gallery, mult, products, k, row_mask, m, s, stats_on_gallery,
                 n_total, group_head, after_scores, after_ids)


@similarity_topk_deep.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, k, row_mask=None, m=None, s=None, stats_on_gallery=1, n_total=0,
      group_head=None, after_scores=None, after_ids=None):
    return _topk_fake("similarity_topk_deep", query_planes, gallery_planes, n_gallery, k, row_mask=row_mask, m=m, s=s,
                      stats_on_gallery=stats_on_gallery, group_head=group_head, after_scores=after_scores, after_ids=after_ids)


def _check_rank(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head):
    """_check_search and the targets: one int32 / int64 per query row"""
    name = "similarity_rank"
    E3 = _check_search(name, query_planes, gallery_planes, n_gallery, row_mask, m, s, stats_on_gallery, group_head)
    if (target.dtype not in (torch.int32, torch.int64) or target.dim() != 1 or target.shape[0] != query_planes.shape[0]
            or target.device != query_planes.device):
        raise ValueError("%s: target %s %s on %s is not one int32 / int64 position per query row (%d) on %s"
                         % (name, tuple(target.shape), target.dtype, target.device, query_planes.shape[0], query_planes.device))
    return E3


@custom_op(NS + "::similarity_rank", mutates_args=(), device_types="cuda")
def similarity_rank(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                    target: torch.Tensor, row_mask: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                    s: Optional[torch.Tensor] = None, stats_on_gallery: int = 1, n_total: int = 0,
                    group_head: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Where gallery row target[q] stands for query row q, without the matrix and without a list -> (counts [Bq, 3] int32,
    score [Bq] fp32): score = the target's score (the bits similarity_topk* give the pair; always computed, whatever the
    target's own mask bit says), counts = (#greater, #equal, #equal with a smaller id) over the rows row_mask leaves selectable
    (None: all) - what rank_counts_cols gives for the matrix row with gt_cols = target; the 0-based rank in similarity_topk's
    order is counts[:, 0] + counts[:, 2].  m, s, stats_on_gallery, n_total, group_head as in similarity_topk_masked; with
    group_head the target is any row of the target group, score the group's best selectable row (-inf without one) and the
    counts run over the groups with a selectable row.  A target outside [0, n_gallery): (0, 0, 0), -inf.
    cc_similarity_rank_planes_f32."""
    Bq = query_planes.shape[0]
    E3 = _check_rank(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head)
    query_planes, gallery_planes = query_planes.contiguous(), gallery_planes.contiguous()
    m, s = _contiguous_stats(m, s)
    target = target.to(torch.int32).contiguous()
    counts = _e(Bq, 3, like=query_planes, dtype=torch.int32)
    score = _e(Bq, like=query_planes, dtype=torch.float32)
    if Bq == 0:
        return counts, score
    if int(n_gallery) == 0:                                 # no row: every target is outside
        return counts.zero_(), score.fill_(float("-inf"))
    lib = L.lib()
    ws = L.workspace(lib.cc_similarity_rank_workspace_bytes(Bq, int(n_gallery)), query_planes.device)
    L.check(lib.cc_similarity_rank_planes_f32(L.ptr(query_planes), L.ptr(gallery_planes), Bq, int(n_gallery), E3 // 3, float(mult),
                                              int(products), L.ptr(target), *_mask_args(row_mask, Bq), L.ptr(m), L.ptr(s),
                                              int(stats_on_gallery),
                                              int(n_total), L.ptr(group_head), L.ptr(counts), L.ptr(score), L.ptr(ws), ws.numel(),
                                              _st(query_planes)), "cc_similarity_rank_planes_f32")
    return counts, score


@similarity_rank.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, target, row_mask=None, m=None, s=None, stats_on_gallery=1, n_total=0,
      group_head=None):
    _check_rank(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head)
    return (query_planes.new_empty((query_planes.shape[0], 3), dtype=torch.int32),
            query_planes.new_empty((query_planes.shape[0],), dtype=torch.float32))


TOPK_MERGE_MAX_LISTS = 64      # CC_TOPK_MERGE_MAX_LISTS


def _check_topk_merge(scores, ids):
    name = "similarity_topk_merge"
    if scores.dim() != 3 or tuple(ids.shape) != tuple(scores.shape) or scores.dtype != torch.float32 or ids.dtype != torch.int32:
        raise ValueError("%s: scores %s %s and ids %s %s are not fp32 / int32 lists [S, Bq, k]"
                         % (name, tuple(scores.shape), scores.dtype, tuple(ids.shape), ids.dtype))
    if scores.device != ids.device:
        raise ValueError("%s: scores on %s, ids on %s" % (name, scores.device, ids.device))
    S, _, k = scores.shape
    if not 1 <= S <= TOPK_MERGE_MAX_LISTS:
        raise ValueError("%s: 1 <= S <= %d lists, not %d" % (name, TOPK_MERGE_MAX_LISTS, S))
    if not 1 <= k <= TOPK_DEEP_MAXK:
        raise ValueError("%s: 1 <= k <= %d, not %d" % (name, TOPK_DEEP_MAXK, k))


@custom_op(NS + "::similarity_topk_merge", mutates_args=(), device_types="cuda")
def similarity_topk_merge(scores: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The lists of S shards -> the list of their concatenation.  scores fp32 / ids int32 [S, Bq, k]: per shard what
    similarity_topk* return for the same queries and the same k (descending, equal scores by smaller id, id -1 = the fill),
    1 <= S <= 64, 1 <= k <= 4096 -> (scores [Bq, k] fp32, ids [Bq, k] int64 = (shard << 32) | id, src [Bq, k] int32 =
    shard * k + index of the entry taken): larger score first (-0 == +0, the bits kept), equal scores by smaller shard, then
    smaller id; the fill (-inf, -1, -1) last.  ``src`` gathers any payload that travels with the entries (labels).  One
    launch, no host read.  Bq == 0 returns without a launch.  cc_topk_merge_lists_f32."""
    _check_topk_merge(scores, ids)
    S, Bq, k = scores.shape
    out_scores = _e(Bq, k, like=scores, dtype=torch.float32)
    out_ids = _e(Bq, k, like=scores, dtype=torch.int64)
    out_src = _e(Bq, k, like=scores, dtype=torch.int32)
    if Bq == 0:
        return out_scores, out_ids, out_src
    scores, ids = scores.contiguous(), ids.contiguous()
    L.check(L.lib().cc_topk_merge_lists_f32(L.ptr(scores), L.ptr(ids), S, Bq, k, L.ptr(out_scores), L.ptr(out_ids), L.ptr(out_src),
                                            _st(scores)), "cc_topk_merge_lists_f32")
    return out_scores, out_ids, out_src


@similarity_topk_merge.register_fake
def _(scores, ids):
    _check_topk_merge(scores, ids)
    _, Bq, k = scores.shape
    return (scores.new_empty((Bq, k), dtype=torch.float32), scores.new_empty((Bq, k), dtype=torch.int64),
            scores.new_empty((Bq, k), dtype=torch.int32))


def _check_per_query(name, what, t, dtypes, planes):
    if t.dtype not in dtypes or t.dim() != 1 or t.shape[0] != planes.shape[0] or t.device != planes.device:
        raise ValueError("%s: %s %s %s on %s is not one %s per query row (%d) on %s"
                         % (name, what, tuple(t.shape), t.dtype, t.device, " / ".join(str(d).replace("torch.", "") for d in dtypes),
                            planes.shape[0], planes.device))


def _check_target_score(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head):
    name = "similarity_target_score"
    E3 = _check_search(name, query_planes, gallery_planes, n_gallery, row_mask, m, s, stats_on_gallery, group_head)
    _check_per_query(name, "target", target, (torch.int32, torch.int64), query_planes)
    return E3


@custom_op(NS + "::similarity_target_score", mutates_args=(), device_types="cuda")
def similarity_target_score(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                            target: torch.Tensor, row_mask: Optional[torch.Tensor] = None, m: Optional[torch.Tensor] = None,
                            s: Optional[torch.Tensor] = None, stats_on_gallery: int = 1, n_total: int = 0,
                            group_head: Optional[torch.Tensor] = None) -> torch.Tensor:
    """similarity_rank's score alone: [Bq] fp32, the score of gallery row target[q] for query row q (with group_head: of the
    best selectable row of the target's group, -inf without one), the bits similarity_topk* give the pair; a target outside
    [0, n_gallery) - a row another shard holds - gives -inf.  Arguments as similarity_rank.  One launch; Bq == 0 or
    n_gallery == 0: none.  cc_similarity_target_score_planes_f32."""
    Bq = query_planes.shape[0]
    E3 = _check_target_score(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head)
    score = _e(Bq, like=query_planes, dtype=torch.float32)
    if Bq == 0:
        return score
    if int(n_gallery) == 0:                                 # no row: every target is outside
        return score.fill_(float("-inf"))
    query_planes, gallery_planes = query_planes.contiguous(), gallery_planes.contiguous()
    m, s = _contiguous_stats(m, s)
    target = target.to(torch.int32).contiguous()
    L.check(L.lib().cc_similarity_target_score_planes_f32(L.ptr(query_planes), L.ptr(gallery_planes), Bq, int(n_gallery), E3 // 3,
                                                          float(mult), int(products), L.ptr(target),
                                                          *_mask_args(row_mask, Bq), L.ptr(m), L.ptr(s),
                                                          int(stats_on_gallery), int(n_total), L.ptr(group_head), L.ptr(score),
                                                          _st(query_planes)), "cc_similarity_target_score_planes_f32")
    return score


@similarity_target_score.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, target, row_mask=None, m=None, s=None, stats_on_gallery=1,
      n_total=0, group_head=None):
    _check_target_score(query_planes, gallery_planes, n_gallery, target, row_mask, m, s, stats_on_gallery, group_head)
    return query_planes.new_empty((query_planes.shape[0],), dtype=torch.float32)


def _check_count(query_planes, gallery_planes, n_gallery, bound_scores, bound_front, row_mask, m, s, stats_on_gallery, group_head):
    name = "similarity_count"
    E3 = _check_search(name, query_planes, gallery_planes, n_gallery, row_mask, m, s, stats_on_gallery, group_head)
    _check_per_query(name, "bound_scores", bound_scores, (torch.float32,), query_planes)
    _check_per_query(name, "bound_front", bound_front, (torch.int32,), query_planes)
    return E3


@custom_op(NS + "::similarity_count", mutates_args=(), device_types="cuda")
def similarity_count(query_planes: torch.Tensor, gallery_planes: torch.Tensor, n_gallery: int, mult: float, products: int,
                     bound_scores: torch.Tensor, bound_front: torch.Tensor, row_mask: Optional[torch.Tensor] = None,
                     m: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None, stats_on_gallery: int = 1,
                     n_total: int = 0, group_head: Optional[torch.Tensor] = None) -> torch.Tensor:
    """similarity_rank's counting pass against a bound the caller holds -> counts [Bq, 3] int32: the candidates of query row q
    (the selectable rows; with group_head the groups that have one, each by its best row) with a score above bound_scores[q],
    equal to it, and equal to it at a position (the row; the group's best row) below bound_front[q].  bound_scores fp32 [Bq],
    bound_front int32 [Bq]: negative - the row counts nothing; n_gallery or more (up to 2^31 - 1) - every equal candidate is in
    front.  Plain float compares: -0 == +0, a NaN bound counts nothing.  The counts of the parts of a gallery split in two
    add up to those of the whole.  Bq == 0 or n_gallery == 0 (zeros): no launch.  cc_similarity_count_planes_f32."""
    Bq = query_planes.shape[0]
    E3 = _check_count(query_planes, gallery_planes, n_gallery, bound_scores, bound_front, row_mask, m, s, stats_on_gallery,
                      group_head)
    counts = _e(Bq, 3, like=query_planes, dtype=torch.int32)
    if Bq == 0:
        return counts
    if int(n_gallery) == 0:                                 # no row: nothing to count
        return counts.zero_()
    query_planes, gallery_planes = query_planes.contiguous(), gallery_planes.contiguous()
    m, s = _contiguous_stats(m, s)
    bound_scores, bound_front = bound_scores.contiguous(), bound_front.contiguous()
    lib = L.lib()
    ws = L.workspace(lib.cc_similarity_count_workspace_bytes(Bq, int(n_gallery)), query_planes.device)
    L.check(lib.cc_similarity_count_planes_f32(L.ptr(query_planes), L.ptr(gallery_planes), Bq, int(n_gallery), E3 // 3, float(mult),
                                               int(products), L.ptr(bound_scores), L.ptr(bound_front),
                                               *_mask_args(row_mask, Bq), L.ptr(m), L.ptr(s), int(stats_on_gallery),
                                               int(n_total), L.ptr(group_head), L.ptr(counts), L.ptr(ws), ws.numel(),
                                               _st(query_planes)), "cc_similarity_count_planes_f32")
    return counts


@similarity_count.register_fake
def _(query_planes, gallery_planes, n_gallery, mult, products, bound_scores, bound_front, row_mask=None, m=None, s=None,
      stats_on_gallery=1, n_total=0, group_head=None):
    _check_count(query_planes, gallery_planes, n_gallery, bound_scores, bound_front, row_mask, m, s, stats_on_gallery, group_head)
    return query_planes.new_empty((query_planes.shape[0], 3), dtype=torch.int32)


def _check_masked_stats(text_planes, video_planes, n_text, n_video, text_mask):
    name = "dsl_col_stats_planes_masked"
    E3 = _check_plane_pair(name, video_planes, text_planes, n_text)
    if video_planes.dim() != 2 or video_planes.shape[0] < int(n_video):
        raise ValueError("%s: video planes %s do not hold %d rows" % (name, tuple(video_planes.shape), int(n_video)))
    _check_row_mask(name, text_mask, None, n_text, text_planes, "text_mask")
    return E3


@custom_op(NS + "::dsl_col_stats_planes_masked", mutates_args=(), device_types="cuda")
def dsl_col_stats_planes_masked(text_planes: torch.Tensor, video_planes: torch.Tensor, n_text: int, n_video: int, mult: float,
                                products: int, text_mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """dsl_col_stats_planes over the text rows whose bit is set in text_mask (int32 [W], W >= ceil(n_text / 32), the format of
    similarity_topk_masked): the same tree with the other rows' terms left out - m bit-equal to the maximum over the set rows,
    all ones = the unmasked op's bits, no row set = (-inf, 0).  cc_dsl_col_stats_planes_masked_f32."""
    E3 = _check_masked_stats(text_planes, video_planes, n_text, n_video, text_mask)
    text_planes, video_planes = text_planes.contiguous(), video_planes.contiguous()
    m = _e(int(n_video), like=video_planes, dtype=torch.float32)
    s = _e(int(n_video), like=video_planes, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_dsl_col_stats_planes_workspace_bytes(int(n_text), int(n_video)), video_planes.device)
    L.check(lib.cc_dsl_col_stats_planes_masked_f32(L.ptr(text_planes), L.ptr(video_planes), int(n_text), int(n_video), E3 // 3,
                                                   float(mult), int(products), L.ptr(text_mask), L.ptr(m), L.ptr(s), L.ptr(ws),
                                                   ws.numel(), _st(video_planes)), "cc_dsl_col_stats_planes_masked_f32")
    return m, s


@dsl_col_stats_planes_masked.register_fake
def _(text_planes, video_planes, n_text, n_video, mult, products, text_mask):
    _check_masked_stats(text_planes, video_planes, n_text, n_video, text_mask)
    return (video_planes.new_empty((n_video,), dtype=torch.float32), video_planes.new_empty((n_video,), dtype=torch.float32))


def _check_flags(flags):
    if flags.dtype not in (torch.bool, torch.uint8) or flags.dim() not in (1, 2) or flags.shape[-1] < 1:
        raise ValueError("pack_row_mask: flags %s %s are not bool or uint8 [n] or [R, n], n >= 1" % (tuple(flags.shape), flags.dtype))


@custom_op(NS + "::pack_row_mask", mutates_args=(), device_types="cuda")
def pack_row_mask(flags: torch.Tensor) -> torch.Tensor:
    """bool or uint8 flags [R, n] (or [n]: one row), non-zero = selectable -> the row masks of similarity_topk_masked, int32
    [R, ceil(n / 32)]: bit b of word w = flag 32 w + b, the bits at or above n zero.  cc_pack_row_mask_u8."""
    _check_flags(flags)
    flat = flags.reshape(-1, flags.shape[-1]).contiguous()
    flat = flat.view(torch.uint8) if flat.dtype == torch.bool else flat
    R, n = flat.shape
    out = _e(R, mask_words(n), like=flat, dtype=torch.int32)
    if R:
        L.check(L.lib().cc_pack_row_mask_u8(L.ptr(flat), R, n, L.ptr(out), mask_words(n), _st(flat)), "cc_pack_row_mask_u8")
    return out


@pack_row_mask.register_fake
def _(flags):
    _check_flags(flags)
    return flags.new_empty((flags.numel() // flags.shape[-1], mask_words(flags.shape[-1])), dtype=torch.int32)


def padded_video_rows(n_video):
    """Rows a video-side plane buffer needs for n_video videos (whole GEMM tiles; the rows behind n_video must be zero)."""
    return int(L.lib().cc_similarity_padded_rows(int(n_video)))


@custom_op(NS + "::scaled_dot_nt", mutates_args=(), device_types="cuda")
def scaled_dot_nt(a: torch.Tensor, b: torch.Tensor, mult: float) -> torch.Tensor:
    Bt, E = a.shape
    Bv = b.shape[0]
    out = _e(Bt, Bv, like=a, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_similarity_workspace_bytes(Bt, Bv, E), a.device)
    L.check(lib.cc_scaled_dot_nt_f32(L.ptr(a), L.ptr(b), Bt, Bv, E, float(mult), L.ptr(out), Bv, L.ptr(ws), ws.numel(),
                                     _st(a)), "cc_scaled_dot_nt_f32")
    return out


@scaled_dot_nt.register_fake
def _(a, b, mult):
    return a.new_empty((a.shape[0], b.shape[0]))


@custom_op(NS + "::scaled_dot_nt_out", mutates_args=("out",), device_types="cuda")
def scaled_dot_nt_out(a: torch.Tensor, b: torch.Tensor, mult: float, out: torch.Tensor) -> None:
    Bt, E = a.shape
    lib = L.lib()
    ws = L.workspace(lib.cc_similarity_workspace_bytes(Bt, b.shape[0], E), a.device)
    L.check(lib.cc_scaled_dot_nt_f32(L.ptr(a), L.ptr(b), Bt, b.shape[0], E, float(mult), L.ptr(out), out.stride(0),
                                     L.ptr(ws), ws.numel(), _st(a)), "cc_scaled_dot_nt_f32")


@scaled_dot_nt_out.register_fake
def _(a, b, mult, out):
    return None


@custom_op(NS + "::rank_counts", mutates_args=(), device_types="cuda")
def rank_counts(sim: torch.Tensor, transpose: bool, diag_offset: int) -> torch.Tensor:
    """utils/metrics.py:11-26 without the sort: per row (#greater, #equal) than the ground-truth entry."""
    rows, cols = (sim.shape[1], sim.shape[0]) if transpose else sim.shape
    rs, cs = (sim.stride(1), sim.stride(0)) if transpose else (sim.stride(0), sim.stride(1))
    counts = _e(rows, 2, like=sim, dtype=torch.int32)
    L.check(L.lib().cc_rank_counts_f32(L.ptr(sim), rows, cols, rs, cs, int(diag_offset), L.ptr(counts), _st(sim)),
            "cc_rank_counts_f32")
    return counts


@rank_counts.register_fake
def _(sim, transpose, diag_offset):
    return sim.new_empty((sim.shape[1] if transpose else sim.shape[0], 2), dtype=torch.int32)


def _check_sim_f32(name, sim):
    """The retrieval-tail kernels take bare pointers and walk fp32 [rows, cols] matrices: anything else is refused here, from
    the tensor's metadata alone."""
    if sim.dim() != 2 or sim.dtype != torch.float32:
        raise ValueError("%s: sim %s %s is not a 2-D fp32 matrix" % (name, tuple(sim.shape), sim.dtype))


def _check_per_row(name, what, t, dtype, rows, sim):
    if t.dtype != dtype or t.dim() != 1 or t.numel() != int(rows) or not t.is_contiguous() or t.device != sim.device:
        raise ValueError("%s: %s %s %s on %s is not one contiguous %s per row (%d) on %s"
                         % (name, what, tuple(t.shape), t.dtype, t.device, dtype, int(rows), sim.device))


@custom_op(NS + "::rank_counts_cols", mutates_args=(), device_types="cuda")
def rank_counts_cols(sim: torch.Tensor, gt_cols: torch.Tensor) -> torch.Tensor:
    """utils/metrics.py:38-65: sim [R, C] contiguous, gt_cols [R] int32 -> (#greater, #equal, #equal before) per row."""
    _check_sim_f32("rank_counts_cols", sim)
    if not sim.is_contiguous():
        raise ValueError("rank_counts_cols: sim %s with strides %s is not contiguous" % (tuple(sim.shape), tuple(sim.stride())))
    _check_per_row("rank_counts_cols", "gt_cols", gt_cols, torch.int32, sim.shape[0], sim)
    R, C = sim.shape
    counts = _e(R, 3, like=sim, dtype=torch.int32)
    L.check(L.lib().cc_rank_counts_cols_f32(L.ptr(sim), R, C, C, 1, L.ptr(gt_cols), L.ptr(counts), _st(sim)),
            "cc_rank_counts_cols_f32")
    return counts


@rank_counts_cols.register_fake
def _(sim, gt_cols):
    return sim.new_empty((sim.shape[0], 3), dtype=torch.int32)


@custom_op(NS + "::contrastive_loss_grad", mutates_args=(), device_types="cuda")
def contrastive_loss_grad(text: torch.Tensor, visual: torch.Tensor, video_mask: torch.Tensor,
                          logit_scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The training branch's loss with its gradient (clip4clip.py:245-262,357-366; losses.py:8-18): text [n,E], visual
    [n,Tn,E], video_mask [n,Tn] int64 -> (loss3 [3], d_text, d_visual, d_logit_scale [1]) for d loss3[2] = 1."""
    n, Tn, E = visual.shape
    loss3 = _e(3, like=text, dtype=torch.float32)
    d_text, d_visual = torch.empty_like(text), torch.empty_like(visual)
    d_ls = _e(1, like=text, dtype=torch.float32)
    ws = L.workspace(L.lib().cc_contrastive_grad_workspace_bytes(n, Tn, E), text.device)
    L.check(L.lib().cc_contrastive_loss_grad_f32(L.ptr(text), L.ptr(visual), L.ptr(video_mask), video_mask.stride(0),
                                                 video_mask.stride(1), n, Tn, E, float(logit_scale), 1.0, L.ptr(loss3),
                                                 L.ptr(d_text), L.ptr(d_visual), L.ptr(d_ls), L.ptr(ws), ws.numel(), _st(text)),
            "cc_contrastive_loss_grad_f32")
    return loss3, d_text, d_visual, d_ls


@contrastive_loss_grad.register_fake
def _(text, visual, video_mask, logit_scale):
    return text.new_empty((3,)), torch.empty_like(text), torch.empty_like(visual), text.new_empty((1,))


@custom_op(NS + "::contrastive_loss_grad_dev", mutates_args=(), device_types="cuda")
def contrastive_loss_grad_dev(text: torch.Tensor, visual: torch.Tensor, video_mask: torch.Tensor,
                              logit_scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """contrastive_loss_grad with logit_scale read from the device (a 0-d / 1-element fp32 tensor: the parameter itself)."""
    n, Tn, E = visual.shape
    loss3 = _e(3, like=text, dtype=torch.float32)
    d_text, d_visual = torch.empty_like(text), torch.empty_like(visual)
    d_ls = _e(1, like=text, dtype=torch.float32)
    ws = L.workspace(L.lib().cc_contrastive_grad_workspace_bytes(n, Tn, E), text.device)
    L.check(L.lib().cc_contrastive_loss_grad_dev_f32(L.ptr(text), L.ptr(visual), L.ptr(video_mask), video_mask.stride(0),
                                                     video_mask.stride(1), n, Tn, E, 0.0, L.ptr(logit_scale), 1.0, L.ptr(loss3),
                                                     L.ptr(d_text), L.ptr(d_visual), L.ptr(d_ls), L.ptr(ws), ws.numel(), _st(text)),
            "cc_contrastive_loss_grad_dev_f32")
    return loss3, d_text, d_visual, d_ls


@contrastive_loss_grad_dev.register_fake
def _(text, visual, video_mask, logit_scale):
    return text.new_empty((3,)), torch.empty_like(text), torch.empty_like(visual), text.new_empty((1,))


def _contrastive_grad_dsl(text, visual, video_mask, scale_value, scale_dev):
    n, Tn, E = visual.shape
    loss3 = _e(3, like=text, dtype=torch.float32)
    d_text, d_visual = torch.empty_like(text), torch.empty_like(visual)
    d_ls = _e(1, like=text, dtype=torch.float32)
    ws = L.workspace(L.lib().cc_contrastive_grad_dsl_workspace_bytes(n, Tn, E), text.device)
    head = (L.ptr(text), L.ptr(visual), L.ptr(video_mask), video_mask.stride(0), video_mask.stride(1), n, Tn, E)
    tail = (1.0, L.ptr(loss3), L.ptr(d_text), L.ptr(d_visual), L.ptr(d_ls), L.ptr(ws), ws.numel(), _st(text))
    if scale_dev is None:
        L.check(L.lib().cc_contrastive_loss_grad_dsl_f32(*head, float(scale_value), *tail), "cc_contrastive_loss_grad_dsl_f32")
    else:
        L.check(L.lib().cc_contrastive_loss_grad_dsl_dev_f32(*head, 0.0, L.ptr(scale_dev), *tail),
                "cc_contrastive_loss_grad_dsl_dev_f32")
    return loss3, d_text, d_visual, d_ls


@custom_op(NS + "::contrastive_loss_grad_dsl", mutates_args=(), device_types="cuda")
def contrastive_loss_grad_dsl(text: torch.Tensor, visual: torch.Tensor, video_mask: torch.Tensor,
                              logit_scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """contrastive_loss_grad with the CAMoE dual softmax between the logits and the two CrossEn terms (camoe_dsl):
    D = n * S * softmax(S, dim=0); same arguments and results."""
    return _contrastive_grad_dsl(text, visual, video_mask, logit_scale, None)


@contrastive_loss_grad_dsl.register_fake
def _(text, visual, video_mask, logit_scale):
    return text.new_empty((3,)), torch.empty_like(text), torch.empty_like(visual), text.new_empty((1,))


@custom_op(NS + "::contrastive_loss_grad_dsl_dev", mutates_args=(), device_types="cuda")
def contrastive_loss_grad_dsl_dev(text: torch.Tensor, visual: torch.Tensor, video_mask: torch.Tensor,
                                  logit_scale: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """contrastive_loss_grad_dsl with logit_scale read from the device (a 0-d / 1-element fp32 tensor: the parameter itself)."""
    return _contrastive_grad_dsl(text, visual, video_mask, 0.0, logit_scale)


@contrastive_loss_grad_dsl_dev.register_fake
def _(text, visual, video_mask, logit_scale):
    return text.new_empty((3,)), torch.empty_like(text), torch.empty_like(visual), text.new_empty((1,))


@custom_op(NS + "::dsl_col_stats", mutates_args=(), device_types="cuda")
def dsl_col_stats(sim: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """camoe_dsl: sim [rows, cols] fp32 (unit column stride) -> (m [cols] = column maxima, s [cols] = sum_i exp(sim_ij - m_j));
    rows == 0 gives (-inf, 0), a NaN in a column makes its pair NaN.  Fixed summation order."""
    rows, cols = sim.shape
    m = _e(cols, like=sim, dtype=torch.float32)
    s = _e(cols, like=sim, dtype=torch.float32)
    nb = L.lib().cc_dsl_col_stats_workspace_bytes(rows, cols)
    ws = L.workspace(nb, sim.device) if rows else None
    L.check(L.lib().cc_dsl_col_stats_f32(L.ptr(sim) if rows else None, rows, cols, sim.stride(0) if rows else cols, L.ptr(m),
                                         L.ptr(s), L.ptr(ws), ws.numel() if rows else 0, _st(sim)), "cc_dsl_col_stats_f32")
    return m, s


@dsl_col_stats.register_fake
def _(sim):
    return sim.new_empty((sim.shape[1],)), sim.new_empty((sim.shape[1],))


@custom_op(NS + "::dsl_rescale_stats_", mutates_args=("s",), device_types="cuda")
def dsl_rescale_stats_(s: torch.Tensor, m_local: torch.Tensor, m_global: torch.Tensor) -> None:
    """camoe_dsl, row-sharded: s[j] *= exp(m_local[j] - m_global[j]) in place (0 stays 0) - [cols] contiguous fp32 each."""
    L.check(L.lib().cc_dsl_rescale_stats_f32(L.ptr(m_local), L.ptr(m_global), L.ptr(s), s.numel(), _st(s)),
            "cc_dsl_rescale_stats_f32")


@dsl_rescale_stats_.register_fake
def _(s, m_local, m_global):
    return None


@custom_op(NS + "::dsl_apply_", mutates_args=("sim",), device_types="cuda")
def dsl_apply_(sim: torch.Tensor, m: torch.Tensor, s: torch.Tensor, n_total: int) -> None:
    """camoe_dsl: sim[i, j] <- n_total * sim[i, j] * exp(sim[i, j] - m[j]) / s[j] in place (sim [rows, cols] fp32, unit column
    stride; m, s [cols] contiguous fp32)."""
    rows, cols = sim.shape
    L.check(L.lib().cc_dsl_apply_f32(L.ptr(sim) if rows else None, rows, cols, sim.stride(0) if rows else cols, L.ptr(m),
                                     L.ptr(s), int(n_total), _st(sim)), "cc_dsl_apply_f32")


@dsl_apply_.register_fake
def _(sim, m, s, n_total):
    return None


@custom_op(NS + "::rank_counts_ref", mutates_args=(), device_types="cuda")
def rank_counts_ref(sim: torch.Tensor, ref_vals: torch.Tensor, transpose: bool) -> torch.Tensor:
    """(#greater, #equal) than ref_vals[i] per row of sim (per COLUMN with transpose=True, through the strides): the
    partial video->text counts of a row block of the similarity matrix (clip-sharded eval)."""
    _check_sim_f32("rank_counts_ref", sim)
    rows, cols = (sim.shape[1], sim.shape[0]) if transpose else sim.shape
    _check_per_row("rank_counts_ref", "ref_vals", ref_vals, torch.float32, rows, sim)
    rs, cs = (sim.stride(1), sim.stride(0)) if transpose else (sim.stride(0), sim.stride(1))
    counts = _e(rows, 2, like=sim, dtype=torch.int32)
    L.check(L.lib().cc_rank_counts_ref_f32(L.ptr(sim), rows, cols, rs, cs, L.ptr(ref_vals), L.ptr(counts), _st(sim)),
            "cc_rank_counts_ref_f32")
    return counts


@rank_counts_ref.register_fake
def _(sim, ref_vals, transpose):
    return sim.new_empty((sim.shape[1] if transpose else sim.shape[0], 2), dtype=torch.int32)


@custom_op(NS + "::group_max_rows", mutates_args=(), device_types="cuda")
def group_max_rows(sim: torch.Tensor, group: torch.Tensor, n_groups: int) -> torch.Tensor:
    """[n_groups, cols] maxima of sim's rows per group id (int32 [rows]), NaN ignored, -inf for groups without a row:
    tensor_video_to_text_sim (utils/metrics.py:68-76).  sim [rows, cols] fp32 with unit column stride (any row stride)."""
    _check_sim_f32("group_max_rows", sim)
    if sim.stride(1) != 1:
        raise ValueError("group_max_rows: sim %s with strides %s does not have a unit column stride"
                         % (tuple(sim.shape), tuple(sim.stride())))
    _check_per_row("group_max_rows", "group", group, torch.int32, sim.shape[0], sim)
    if int(n_groups) <= 0:
        raise ValueError("group_max_rows: n_groups >= 1, not %d" % int(n_groups))
    rows, cols = sim.shape
    out = _e(int(n_groups), cols, like=sim, dtype=torch.float32)
    L.check(L.lib().cc_group_max_rows_f32(L.ptr(sim) if rows else None, rows, cols, sim.stride(0) if rows else cols,
                                          L.ptr(group) if rows else None, int(n_groups), L.ptr(out), _st(sim)),
            "cc_group_max_rows_f32")
    return out


@group_max_rows.register_fake
def _(sim, group, n_groups):
    return sim.new_empty((n_groups, sim.shape[1]))


@custom_op(NS + "::contrastive_loss", mutates_args=(), device_types="cuda")
def contrastive_loss(sim: torch.Tensor) -> torch.Tensor:
    """CrossEn(sim), CrossEn(sim.T) and their mean (modules/losses.py:8-18, clip4clip.py:250-253) -> [3] fp32.
    sim [n, n] fp32, any strides."""
    _check_sim_f32("contrastive_loss", sim)
    if sim.shape[0] != sim.shape[1]:
        raise ValueError("contrastive_loss: sim %s is not square" % (tuple(sim.shape),))
    n = sim.shape[0]
    out = _e(3, like=sim, dtype=torch.float32)
    ws = L.workspace(2 * n * 4, sim.device)
    L.check(L.lib().cc_contrastive_loss_f32(L.ptr(sim), n, sim.stride(0), sim.stride(1), L.ptr(out), L.ptr(ws), ws.numel(),
                                            _st(sim)), "cc_contrastive_loss_f32")
    return out


@contrastive_loss.register_fake
def _(sim):
    return sim.new_empty((3,))


OPS = ("contrastive_loss", "contrastive_loss_grad", "contrastive_loss_grad_dev", "contrastive_loss_grad_dsl",
       "contrastive_loss_grad_dsl_dev", "dsl_col_stats", "dsl_rescale_stats_", "dsl_apply_", "spectral_laplacian", "spectral_graph_laplacian", "spectral_embedding", "svd_sign_flip", "linear_f16", "linear_f16_out", "layernorm", "attention_f16", "fold_layernorm_linear", "row_stats",
       "linear_ln_f16", "inproj_attention_f16", "linear_resid_stats_f16", "head_project", "token_cluster", "token_cluster_train", "token_cluster_backward", "token_apply_selection",
       "batch_kmedoids", "kmedoids_from_dist",
       "pairwise_distance", "pairwise_distance_cross", "token_norms", "vit_encode", "text_encode", "clip_encode_out", "clip_encode",
       "loose_similarity", "video_pool_normalize", "normalize_rows", "scaled_dot_nt", "scaled_dot_nt_out", "rank_counts",
       "rank_counts_cols", "rank_counts_ref", "group_max_rows", "normalize_rows_planes", "video_pool_normalize_planes",
       "scaled_dot_planes", "key_masked_attention", "key_masked_attention_backward", "seqtransf_forward", "linear_ln_act_f16",
       "similarity_topk", "dsl_col_stats_planes", "similarity_topk_dsl",
       "similarity_topk_grouped", "similarity_topk_grouped_dsl", "similarity_topk_masked", "dsl_col_stats_planes_masked",
       "pack_row_mask", "similarity_rank", "similarity_topk_deep", "similarity_topk_merge", "similarity_target_score",
       "similarity_count", "video_window_pool_planes") + tuple(FRAME_OPS)


def logit_multiplier(logit_scale):
    """exp(logit_scale) on the host (clip4clip.py:357-358 computes it with a device op; the value is a parameter)."""
    return math.exp(float(logit_scale))
