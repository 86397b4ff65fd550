"""N4, first slice of training: forward WITH saved activations and backward of one ResidualAttentionBlock
(modules/clip.py:196-253; the reference gets the backward from torch.autograd inside main.py:321
``scaler.scale(loss).backward()``).

    x [L, N, W] (LND, as the reference's blocks see it)
    y = x + out_proj(MHA(in_proj(ln_1(x))))          z = y + c_proj(QuickGELU(c_fc(ln_2(y))))

* forward: the op-level HIP entry points of the inference path (LayerNorm -> fp16, cc_linear_f16, cc_attention_f16,
  residual epilogue), keeping what the backward needs: x, ln_1(x), qkv, the attention output, y, ln_2(y), the c_fc output
  before and after QuickGELU.
* backward: the four Linear layers' dgrad (dX = dY W) and wgrad (dW = dY^T X) run on the SAME fp16 MFMA GEMM kernel with
  swapped operand roles - ``cc_linear_f16(a, w)`` computes a w^T, so dX = linear(dY, W^T) and dW = linear(dY^T, X^T) with the
  row count (padded to 64) as the contraction; gradients enter the matrix cores as fp16 with a per-tensor power-of-two scale
  chosen on the device (cc_cast_transpose_f16 / cc_linear_unscaled_f16: no host synchronisation); LayerNorm, QuickGELU, attention
  and bias gradients are the fp32 kernels of csrc/backward.hip.
* ``ResidualAttentionBlockFunction`` wires both into torch.autograd (d/dx and the 12 parameter gradients), so a block can sit
  in a graph that ends in losses.contrastive_loss; dist.GradientBuckets then averages the gradients over the ranks.

Round 4, later: the towers themselves (encode_image_train / encode_text_train below: patch embedding, ln_pre, the blocks with
a token-cluster module in front, the heads), BertAdam (utils/optimization.py) on cc_bertadam_step_f32 and train_epoch
(main.py:291-378) - CLIP4Clip.forward in training mode runs on them, so a training step reaches every parameter.  What is NOT
here: linear_patch='3d' and mean_residual in training, and fusion (train_epoch takes the reference's GradScaler, or a
DeviceGradScaler - the same recipe decided on the device, which GraphedTrainStep(scaler=...) captures; the master
weights are fp32 and the HIP backward scales per tensor on the device) - per-op launches from Python, checked against torch.autograd on the
reference model (tests/test_r4_gpu.py, fixture tests/golden/r4_golden.npz) to 1e-2 of each tensor's largest entry.
Transposed fp16 copies (W^T, dY^T, X^T) come from cc_cast_transpose_f16 (one read per matrix); the scale of a gradient operand
is divided out in the consuming GEMM's epilogue (cc_linear_unscaled_f16).
"""
import torch

from . import _lib as L
from . import ops
from .torch_ops import _st


def _check(rc, what):
    L.check(rc, what)


def _pad64(n):
    return -(-n // 64) * 64


def _cast_transpose(x, scaled, want_out=True, col_sums=False, amax=None, want_t=True, col_partials=False):
    """One read of a matrix -> its fp16 operand copies for a Linear's backward (cc_cast_transpose_f16):
    x fp32 [M, C] -> (x16 [M, C], x16^T [C, Mp] zero padded to a multiple of 64, scale or None); x fp16 -> (x, x^T, None).
    scaled: the device-chosen power-of-two scale of the gradients (returned as a 1-element device tensor); amax: a 2-float
    device tensor whose first entry already holds the largest |x| (written by the kernel that produced x) - the pass over x that
    finds it is skipped, the scale lands in the second entry."""
    x = x.contiguous()
    M, C = x.shape
    Mp = _pad64(M)
    out_t = torch.empty(C, Mp, device=x.device, dtype=torch.float16) if want_t else None    # (want_t False: the fp16 copy only)
    lib = L.lib()
    if x.dtype == torch.float16:
        _check(lib.cc_cast_transpose_f16(None, L.ptr(x), None, L.ptr(out_t), M, C, Mp, 0, None, None, None, None, 0, _st(x)),
               "cc_cast_transpose_f16")
        return x, out_t, None
    out = torch.empty(M, C, device=x.device, dtype=torch.float16) if want_out else None
    scratch = (amax if amax is not None else torch.empty(2, device=x.device, dtype=torch.float32)) if scaled else None
    cs = torch.empty(C, device=x.device, dtype=torch.float32) if (col_sums and not col_partials) else None
    # col_partials: the per-tile partial column sums [Mp / 64, C] stay in a tensor of their own and are returned instead of the
    # sums - cc_wgrad_tn_f16 adds them in the launch that adds its slices (the shared workspace is that call's scratch)
    ws = None
    if col_partials:
        ws = torch.empty(Mp // 64, C, device=x.device, dtype=torch.float32)
    elif col_sums:
        ws = L.workspace(lib.cc_cast_transpose_colsum_workspace_bytes(Mp, C), x.device)
    _check(lib.cc_cast_transpose_f16(L.ptr(x), None, L.ptr(out), L.ptr(out_t), M, C, Mp, (2 if amax is not None else 1) if scaled else 0,
                                     L.ptr(scratch[0:1]) if scaled else None, L.ptr(scratch[1:2]) if scaled else None, L.ptr(cs),
                                     L.ptr(ws), ws.numel() * ws.element_size() if ws is not None else 0, _st(x)), "cc_cast_transpose_f16")
    if col_partials:
        return out, out_t, (scratch[1:2] if scaled else None), ws
    if col_sums:
        return out, out_t, (scratch[1:2] if scaled else None), cs
    return out, out_t, (scratch[1:2] if scaled else None)


def _cast_scaled(x32):
    """fp32 tensor -> (fp16 copy scaled by a device-chosen power of two, the scale as a 1-element device tensor)."""
    x32 = x32.contiguous()
    out = torch.empty(x32.shape, device=x32.device, dtype=torch.float16)
    scratch = torch.empty(2, device=x32.device, dtype=torch.float32)
    _check(L.lib().cc_cast_scaled_f16(L.ptr(x32), L.ptr(out), x32.numel(), L.ptr(scratch[0:1]), L.ptr(scratch[1:2]), _st(x32)),
           "cc_cast_scaled_f16")
    return out, scratch[1:2]


def _unscale(x32, scale):
    _check(L.lib().cc_unscale_f32(L.ptr(x32), x32.numel(), L.ptr(scale), None, _st(x32)), "cc_unscale_f32")
    return x32


def _linear_unscaled(a16, w16, scale):
    """(a w^T) / scale in fp32: the GEMM with the operand's device-chosen scale undone in its epilogue."""
    M, K = a16.shape
    N = w16.shape[0]
    assert a16.dtype == torch.float16 and w16.dtype == torch.float16 and a16.is_contiguous() and w16.is_contiguous()
    assert w16.shape[1] == K and scale.dtype == torch.float32
    out = torch.empty(M, N, device=a16.device, dtype=torch.float32)
    _check(L.lib().cc_linear_unscaled_f16(L.ptr(a16), L.ptr(w16), L.ptr(out), M, N, K, L.ptr(scale), _st(a16)),
           "cc_linear_unscaled_f16")
    return out


def _wgrad_tn(dy16, x16, scale, col_partial=None):
    """dW [N1, N2] fp32 = (dy16^T x16) / scale from the row-major fp16 matrices dy16 [M, N1], x16 [M, N2] (cc_wgrad_tn_f16).
    col_partial [chunks, N1] (cc_cast_transpose_f16's partial column sums of dY): also returns the bias gradient [N1]."""
    M, N1 = dy16.shape
    N2 = x16.shape[1]
    assert dy16.dtype == torch.float16 and x16.dtype == torch.float16 and dy16.is_contiguous() and x16.is_contiguous()
    assert x16.shape[0] == M and scale.dtype == torch.float32
    lib = L.lib()
    dw = torch.empty(N1, N2, device=dy16.device, dtype=torch.float32)
    db = None
    if col_partial is not None:
        assert col_partial.dtype == torch.float32 and col_partial.is_contiguous() and col_partial.shape[1] == N1
        db = torch.empty(N1, device=dy16.device, dtype=torch.float32)
    ws = L.workspace(lib.cc_wgrad_tn_workspace_bytes(M, N1, N2), dy16.device)
    _check(lib.cc_wgrad_tn_f16(L.ptr(dy16), L.ptr(x16), L.ptr(dw), M, N1, N2, L.ptr(scale), L.ptr(col_partial),
                               col_partial.shape[0] if col_partial is not None else 0, L.ptr(db), L.ptr(ws), ws.numel(), _st(dy16)),
           "cc_wgrad_tn_f16")
    return dw if col_partial is None else (dw, db)


def _linear_resid(a16, w16, bias, resid):
    """resid + a w^T + bias in fp32 (cc_linear_resid_f16): the residual epilogue reading the rows it adds from ``resid`` - the
    forward keeps its input for the backward, so it cannot accumulate in place and used to copy it first."""
    M, K = a16.shape
    N = w16.shape[0]
    assert a16.dtype == torch.float16 and w16.dtype == torch.float16 and a16.is_contiguous() and w16.is_contiguous()
    assert w16.shape[1] == K and resid.dtype == torch.float32 and resid.is_contiguous() and tuple(resid.shape) == (M, N)
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == N)
    out = torch.empty(M, N, device=a16.device, dtype=torch.float32)
    _check(L.lib().cc_linear_resid_f16(L.ptr(a16), L.ptr(w16), L.ptr(bias), L.ptr(resid), L.ptr(out), M, N, K, 0, _st(a16)),
           "cc_linear_resid_f16")
    return out


def _column_sums(x32):
    rows, cols = x32.shape
    out = torch.empty(cols, device=x32.device, dtype=torch.float32)
    lib = L.lib()
    ws = L.workspace(lib.cc_column_sums_workspace_bytes(rows, cols), x32.device)
    _check(lib.cc_column_sums_f32(L.ptr(x32), rows, cols, L.ptr(out), L.ptr(ws), ws.numel(), _st(x32)), "cc_column_sums_f32")
    return out


def _ln_backward(x, gamma, dy, dres, eps=1e-5, amax=None, need_params=True):
    """need_params False (a frozen LayerNorm): dg = db = None and the launch that reduces the per-workgroup gamma / beta
    partial sums does not run (the dx kernel still leaves those partials in the workspace)."""
    rows, W = x.shape
    dx = torch.empty_like(x)
    dg, db = (torch.empty(W, device=x.device), torch.empty(W, device=x.device)) if need_params else (None, None)
    lib = L.lib()
    ws = L.workspace(lib.cc_layernorm_backward_workspace_bytes(rows, W), x.device)
    _check(lib.cc_layernorm_backward_f32(L.ptr(x), W, L.ptr(gamma), L.ptr(dy), L.ptr(dres), L.ptr(dx), L.ptr(dg), L.ptr(db),
                                         rows, W, float(eps), L.ptr(amax), L.ptr(ws), ws.numel(), _st(x)), "cc_layernorm_backward_f32")
    return dx, dg, db


def _wt16(w):
    """W [N, K] (fp32 master weight or fp16) -> W^T [K, Np] fp16, the dgrad's operand (columns behind N are zeros and are
    sliced away: cc_linear_f16 takes the row stride from the shape, so the view must be made contiguous only when N % 64)."""
    w = w.detach()
    N, K = w.shape
    _, wt, _ = _cast_transpose(w.float() if w.dtype not in (torch.float16, torch.float32) else w, scaled=False, want_out=False)
    return wt if wt.shape[1] == N else wt[:, :N].contiguous()


def _w16_pair(w):
    """fp32 master weight [N, K] -> (W fp16 for the forward GEMM, W^T [K, N] fp16 for the backward's dgrad) from ONE read."""
    w = w.detach()
    if w.dtype != torch.float32:
        return w.to(torch.float16).contiguous(), None
    w16, wt, _ = _cast_transpose(w, scaled=False)
    N = w.shape[0]
    return w16, (wt if wt.shape[1] == N else wt[:, :N].contiguous())


def _grad_linear(dy32, x16, w16_t, need_dx=True, amax=None, need_dw=True, need_db=True):
    """Gradients of y = x W^T + b for dy [M, N] fp32, x [M, K] fp16, W^T [K, N] fp16 -> (dx [M, K], dW [N, K], db [N]) fp32.
    The gradient is read ONCE for its two fp16 layouts (row-major for dX = dY W, transposed + padded for dW = dY^T X).
    need_dw False (a frozen layer, main.py's freeze_layer_num): no transposed copies, no wgrad GEMM, dW = None; need_db False:
    no column sums, db = None; nothing needed at all: (None, None, None) without a launch."""
    if not (need_dx or need_dw or need_db):
        return None, None, None
    # round 5: the weight gradient multiplies dY and X as they lie in memory (cc_wgrad_tn_f16: LDS transposing reads) wherever both
    # widths are multiples of its 128-wide tile - every layer of the CLIP towers; other widths keep the transposed copies
    M, N1 = dy32.shape
    tn = need_dw and N1 % 128 == 0 and x16.shape[1] % 128 == 0
    if need_db:
        dy16, dy16_t, scale, db = _cast_transpose(dy32, scaled=True, col_sums=True, amax=amax,   # (+ the bias gradient, same read)
                                                  want_t=need_dw and not tn, col_partials=tn)
    else:
        dy16, dy16_t, scale = _cast_transpose(dy32, scaled=True, amax=amax, want_t=need_dw and not tn)
        db = None
    dw = None
    if tn and need_db:
        dw, db = _wgrad_tn(dy16, x16, scale, col_partial=db)                                  # dY^T X (+ the bias sums' last step)
    elif tn:
        dw = _wgrad_tn(dy16, x16, scale)
    elif need_dw:
        _, x16_t, _ = _cast_transpose(x16, scaled=False)
        dw = _linear_unscaled(dy16_t, x16_t, scale)                                           # dY^T X
    # (dX last: the kernel that consumes it runs next and finds it in the memory-side cache)
    dx = _linear_unscaled(dy16, w16_t, scale) if need_dx else None                            # dY W
    return dx, dw, db


def _token_shift_rows(y, N, Lt, mid_shift, adjoint):
    """token_shift (or its transpose) of the frame-major rows y [N * Lt, W]: the CLS rows, segments of mid_shift[0] frames."""
    seg, div = mid_shift
    W = y.shape[1]
    return torch.ops.centerclip.token_shift(y.view(N, Lt, W), True, seg, div, 5, adjoint).view(N * Lt, W)


def block_forward_train(block, x_lnd, mid_shift=None, key_mask=None):
    """-> (z [L, N, W] fp32, saved dict).  ``block``: a centerclip_amd.clip.ResidualAttentionBlock without a cluster module.
    ``mid_shift`` (segment, fold_div): token_shift's second shift between the attention residual and ln_2 (clip.py:246-248),
    y' = S(y); None (default): the plain block.  ``key_mask`` [N, L] int64 (any strides): the seqTransf head's additive
    (1 - mask[key]) * -1e6 on every key of sequence n (module_cross.py:102-104, cc_key_masked_attention_f16)."""
    if block.tokencluster_inter is not None:
        raise NotImplementedError("block backward: blocks with a token-cluster module are not covered by this slice")
    L.require_device(x_lnd)
    Lt, N, W = x_lnd.shape
    M = N * Lt
    causal = block.attn_mask is not None
    f32 = lambda t: t.detach().float().contiguous()
    x = x_lnd.detach().float().permute(1, 0, 2).contiguous().view(M, W)              # frame-major rows (row = seq*L + token)
    wq, wo, wf, wp = (_w16_pair(w) for w in (block.attn.in_proj_weight, block.attn.out_proj.weight, block.mlp["c_fc"].weight,
                                             block.mlp["c_proj"].weight))
    n1 = ops.layernorm(x, f32(block.ln_1.weight), f32(block.ln_1.bias), eps=block.ln_1.eps, out_f16=True)
    qkv = ops.linear_f16(n1, wq[0], f32(block.attn.in_proj_bias), "f16")
    if key_mask is not None:
        if causal:
            raise ValueError("block_forward_train: a key mask and a causal mask together are not built")
        att = torch.ops.centerclip.key_masked_attention(qkv, key_mask, N, Lt, block.n_head)
    else:
        att = ops.attention_f16(qkv, N, Lt, block.n_head, causal=causal)
    y = _linear_resid(att, wo[0], f32(block.attn.out_proj.bias), x)           # x + out_proj(att): x itself is kept for the backward
    if mid_shift is not None:
        y = _token_shift_rows(y, N, Lt, mid_shift, False)                      # y' = S(y): what ln_2 and the residual read
    n2 = ops.layernorm(y, f32(block.ln_2.weight), f32(block.ln_2.bias), eps=block.ln_2.eps, out_f16=True)
    u_pre = ops.linear_f16(n2, wf[0], f32(block.mlp["c_fc"].bias), "f16")
    u = torch.empty_like(u_pre)
    _check(L.lib().cc_quick_gelu_f16(L.ptr(u_pre), L.ptr(u), u.numel(), _st(u)), "cc_quick_gelu_f16")
    z = _linear_resid(u, wp[0], f32(block.mlp["c_proj"].bias), y)
    wt = dict(in_proj=wq[1], out_proj=wo[1], c_fc=wf[1], c_proj=wp[1])                  # W^T of the same read, for the dgrads
    saved = dict(x=x, n1=n1, qkv=qkv, att=att, y=y, n2=n2, u_pre=u_pre, u=u, shape=(Lt, N, W), causal=causal, wt=wt,
                 mid_shift=mid_shift, key_mask=key_mask)
    # (a VIEW of the frame-major rows: the next block's permute + contiguous then costs nothing - a chain of plain blocks never
    # copies its activations between the two layouts)
    return z.view(N, Lt, W).permute(1, 0, 2), saved


def block_backward(block, saved, dz_lnd, need=None, need_dx=True):
    """dz [L, N, W] -> (dx [L, N, W], {parameter name: gradient}) for the forward that produced ``saved``.  ``need``
    (optional): {parameter name: bool} - parameter gradients that nobody asked for (frozen layers) are not computed (None):
    no wgrad GEMM, no bias column sums, no launch reducing the gamma / beta partial sums.  ``need_dx`` False (the first trainable block of a tower
    behind a frozen prefix: nothing below can receive a gradient): dx = None, the in_proj dgrad and - with a frozen ln_1 - the
    ln_1 backward do not run; with in_proj frozen as well the backward stops behind out_proj."""
    need = need or {}
    nw = lambda key: bool(need.get(key, True))
    ln1 = nw("ln_1.weight") or nw("ln_1.bias")
    ln2 = nw("ln_2.weight") or nw("ln_2.bias")
    Lt, N, W = saved["shape"]
    M = N * Lt
    wt = saved.get("wt", {})
    f16t = lambda w, key: wt[key] if wt.get(key) is not None else _wt16(w)              # W^T as the dgrad's operand
    f32 = lambda t: t.detach().float().contiguous()
    dz = dz_lnd.detach().float().permute(1, 0, 2).contiguous().view(M, W)
    g = {}
    # z = y + c_proj(u)
    du, g["mlp.c_proj.weight"], g["mlp.c_proj.bias"] = _grad_linear(dz, saved["u"], f16t(block.mlp["c_proj"].weight, "c_proj"), need_dw=nw("mlp.c_proj.weight"), need_db=nw("mlp.c_proj.bias"))
    # u = QuickGELU(u_pre)
    # (the three gradients this function produces AND multiplies publish their largest magnitude from the producing kernel:
    #  the fp16 cast of each then needs no pass of its own to choose the scale)
    am = torch.zeros(3, 2, device=dz.device, dtype=torch.float32)
    du_pre = torch.empty_like(du)
    _check(L.lib().cc_quick_gelu_backward_f16(L.ptr(saved["u_pre"]), L.ptr(du), L.ptr(du_pre), du.numel(), L.ptr(am[0]), _st(du)),
           "cc_quick_gelu_backward_f16")
    # u_pre = c_fc(ln_2(y))
    dn2, g["mlp.c_fc.weight"], g["mlp.c_fc.bias"] = _grad_linear(du_pre, saved["n2"], f16t(block.mlp["c_fc"].weight, "c_fc"), amax=am[0], need_dw=nw("mlp.c_fc.weight"), need_db=nw("mlp.c_fc.bias"))
    dy, g["ln_2.weight"], g["ln_2.bias"] = _ln_backward(saved["y"], f32(block.ln_2.weight), dn2, dz, eps=block.ln_2.eps, amax=am[1], need_params=ln2)   # + the residual branch
    if saved.get("mid_shift") is not None:
        # y' = S(y): dy = S^T dy' (the CLS rows' opposite shift; the largest magnitude am[1] the LayerNorm backward published
        # still bounds it - S^T only moves and zeroes values)
        dy = _token_shift_rows(dy, N, Lt, saved["mid_shift"], True)
    # y = x + out_proj(att)
    datt, g["attn.out_proj.weight"], g["attn.out_proj.bias"] = _grad_linear(dy, saved["att"], f16t(block.attn.out_proj.weight, "out_proj"), amax=am[1], need_dw=nw("attn.out_proj.weight"), need_db=nw("attn.out_proj.bias"))
    if not (need_dx or ln1 or nw("attn.in_proj_weight") or nw("attn.in_proj_bias")):
        for k in ("attn.in_proj_weight", "attn.in_proj_bias", "ln_1.weight", "ln_1.bias"):
            g[k] = None
        return None, g
    dqkv = torch.empty(M, 3 * W, device=dz.device, dtype=torch.float32)
    km = saved.get("key_mask")
    if km is not None:
        _check(L.lib().cc_key_masked_attention_backward_f16(L.ptr(saved["qkv"]), L.ptr(km), km.stride(0), km.stride(1), L.ptr(datt),
                                                            L.ptr(dqkv), N, Lt, block.n_head, W, L.ptr(am[2]), _st(dz)),
               "cc_key_masked_attention_backward_f16")
    else:
        ab_bytes = L.lib().cc_attention_backward_workspace_bytes(N, Lt, block.n_head)       # (0 for Lt <= 64)
        ab_ws = L.workspace(ab_bytes, dz.device) if ab_bytes else None
        _check(L.lib().cc_attention_backward_f16(L.ptr(saved["qkv"]), L.ptr(datt), L.ptr(dqkv), N, Lt, block.n_head, W,
                                                 int(saved["causal"]), L.ptr(am[2]), L.ptr(ab_ws), ab_bytes, _st(dz)),
               "cc_attention_backward_f16")
    dn1, g["attn.in_proj_weight"], g["attn.in_proj_bias"] = _grad_linear(
        dqkv, saved["n1"], f16t(block.attn.in_proj_weight, "in_proj") if (need_dx or ln1) else None, need_dx=need_dx or ln1,
        amax=am[2], need_dw=nw("attn.in_proj_weight"), need_db=nw("attn.in_proj_bias"))
    if not (need_dx or ln1):
        g["ln_1.weight"] = g["ln_1.bias"] = None
        return None, g
    dx, g["ln_1.weight"], g["ln_1.bias"] = _ln_backward(saved["x"], f32(block.ln_1.weight), dn1, dy, eps=block.ln_1.eps, need_params=ln1)
    return (dx.view(N, Lt, W).permute(1, 0, 2) if need_dx else None), g


_PARAM_ORDER = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight",
                "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight",
                "ln_2.bias")


class ResidualAttentionBlockFunction(torch.autograd.Function):
    """z = block(x) with the HIP forward / backward above inside torch.autograd: gradients reach x and the block's 12
    parameter tensors (passed as arguments so that autograd sees them)."""

    @staticmethod
    def forward(ctx, block, x, *params):
        z, saved = block_forward_train(block, x, mid_shift=getattr(block, "mid_shift", None), key_mask=getattr(block, "key_mask", None))
        # (nothing of this call can receive a gradient - a frozen block on an input without one: keep nothing for a backward)
        ctx.block, ctx.saved = block, (saved if any(ctx.needs_input_grad) else None)
        # (the activations and the forward-time W^T copies live in ctx.saved, outside autograd's version tracking: remember the
        #  parameters' versions, so that a weight changed in place between forward and backward is an error, as it is for
        #  tensors kept with save_for_backward, and not a silently stale W^T)
        ctx.versions = tuple(p._version for p in params)
        return z

    @staticmethod
    def backward(ctx, dz):
        named = dict(ctx.block.named_parameters())
        if tuple(named[k]._version for k in _PARAM_ORDER) != ctx.versions:
            raise RuntimeError("ResidualAttentionBlockFunction: a parameter of the block was modified in place between forward "
                               "and backward (the saved W^T copies are those of the forward)")
        need = {k: bool(ctx.needs_input_grad[2 + i]) for i, k in enumerate(_PARAM_ORDER)}
        dx, g = block_backward(ctx.block, ctx.saved, dz, need=need, need_dx=bool(ctx.needs_input_grad[1]))
        return (None, dx) + tuple((g[k].view_as(named[k]).to(named[k].dtype) if (need[k] and g[k] is not None) else None)
                                  for k in _PARAM_ORDER)


def block_apply(block, x_lnd):
    """Differentiable block forward: ``z = block_apply(block, x); loss(z).backward()`` fills x.grad and block.*.grad."""
    named = dict(block.named_parameters())
    return ResidualAttentionBlockFunction.apply(block, x_lnd, *[named[k] for k in _PARAM_ORDER])


# ================================================================================================ the towers, differentiable
# What main.py:291-378 (train_epoch) needs from the model: CLIP4Clip.forward in training mode with gradients reaching every
# parameter.  The towers below are the reference's forward (modules/clip.py:320-345 visual, :471-496 text) composed of the HIP
# forward / backward pieces: patch embedding and the projection heads as GEMMs (LinearFunction: dgrad / wgrad on the forward
# kernel), LayerNorms (LayerNormFunction), the blocks (ResidualAttentionBlockFunction), the token-cluster module (its own
# autograd, cluster/cluster.py).  What stays torch glue: reshapes / permutes / concatenation, the broadcast adds of the class
# and positional embeddings, the embedding-table gather with its scatter-add gradient, the EOT row gather.

class LinearFunction(torch.autograd.Function):
    """y [M, N] fp32 = x [M, K] @ w[N, K]^T (+ b): fp16 MFMA operands, fp32 accumulate; gradients as _grad_linear, each one
    only where autograd asks for it.  An fp16 x (the patch gather's output) is the GEMM operand and the saved activation as
    it is - no copy."""

    @staticmethod
    def forward(ctx, x, w, b):
        x16 = x.detach().to(torch.float16).contiguous()
        if any(ctx.needs_input_grad[1:]):                     # (x itself is only needed for the weight gradient)
            ctx.save_for_backward(x16, w)
        else:
            ctx.save_for_backward(None, w)
        ctx.has_bias = b is not None
        return ops.linear_f16(x16, w.detach().to(torch.float16).contiguous(), None if b is None else b.detach().float().contiguous(),
                              "f32")

    @staticmethod
    def backward(ctx, dy):
        x16, w = ctx.saved_tensors
        need_dx, need_dw = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        need_db = ctx.has_bias and bool(ctx.needs_input_grad[2])
        dx, dw, db = _grad_linear(dy.contiguous().float(), x16, _wt16(w) if need_dx else None, need_dx=need_dx, need_dw=need_dw,
                                  need_db=need_db)
        return dx, (dw.to(w.dtype) if need_dw else None), db


class LayerNormFunction(torch.autograd.Function):
    """LayerNorm over the last dim of x [rows, W] fp32 (modules/clip.py:183-189), backward = cc_layernorm_backward_f32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.detach().float().contiguous()
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        return ops.layernorm(x, gamma.detach().float().contiguous(), beta.detach().float().contiguous(), eps)

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        need_g, need_b = bool(ctx.needs_input_grad[1]), bool(ctx.needs_input_grad[2])
        dx, dg, db = _ln_backward(x, gamma.detach().float().contiguous(), dy.contiguous().float(), None, ctx.eps,
                                  need_params=need_g or need_b)
        return (dx if ctx.needs_input_grad[0] else None), (dg.to(gamma.dtype) if need_g else None), \
            (db.to(gamma.dtype) if need_b else None), None


def _layernorm(ln, x2d):
    return LayerNormFunction.apply(x2d, ln.weight, ln.bias, ln.eps)


def _blocks(transformer, x_lnd, start=0):
    """The resblocks from block ``start`` on, on LND activations; a block's token-cluster module runs in front of it
    (clip.py:236-242)."""
    for blk in list(transformer.resblocks)[start:]:
        tc = blk.tokencluster_inter
        if tc is not None:
            if getattr(tc, "mean_residual", False):
                raise NotImplementedError("training towers: mean_residual is not built")
            x_lnd, _ = tc(x_lnd)
            # token_shift shifts the CLS rows again behind the attention (clip.py:246-248)
            x_lnd = _plain(blk, x_lnd, (tc.original_frame, tc.shift_fold_div) if tc.algorithm == 'token_shift' else None)
        else:
            x_lnd = block_apply(blk, x_lnd)
    return x_lnd


class _NoCluster:
    """A view of a block without its cluster module (block_forward_train refuses blocks that carry one: here the module has
    already run); ``mid_shift``: token_shift's second shift, which the block itself applies."""

    def __init__(self, blk, mid_shift=None):
        self._blk = blk
        self.tokencluster_inter = None
        self.mid_shift = mid_shift

    def __getattr__(self, name):
        return getattr(self._blk, name)


class _KeyMasked(_NoCluster):
    """A block of the seqTransf head with its key mask (block_forward_train(key_mask=...))."""

    def __init__(self, blk, key_mask):
        super().__init__(blk)
        self.key_mask = key_mask


def seq_head_train(model, visual_output, video_mask):
    """CLIP4Clip's seqTransf head (clip4clip.py:335-349) with gradients: visual_output [B, T, D] + video_mask [B, T] ->
    [B, T, D].  The position rows are a slice of frame_position_embeddings.weight (rows >= T get exactly zero gradient), the
    blocks run block_forward_train / block_backward with the key mask, the outer residual is an autograd add."""
    L.require_device(visual_output)
    B, T, D = visual_output.shape
    mask = video_mask if video_mask.dtype == torch.long else video_mask.to(torch.long)
    x = visual_output.float() + model.frame_position_embeddings.weight[:T].float().unsqueeze(0)
    x = x.permute(1, 0, 2)                                                      # NLD -> LND (a view: the block reads it once)
    for blk in model.transformerClip.resblocks:
        named = dict(blk.named_parameters())
        x = ResidualAttentionBlockFunction.apply(_KeyMasked(blk, mask), x, *[named[k] for k in _PARAM_ORDER])
    return x.permute(1, 0, 2) + visual_output.float()


def _plain(blk, x_lnd, mid_shift=None):
    view = _NoCluster(blk, mid_shift)
    named = dict(blk.named_parameters())
    return ResidualAttentionBlockFunction.apply(view, x_lnd, *[named[k] for k in _PARAM_ORDER])


# The frozen prefix of a tower (clip4clip.py:449-471 freeze_cip_layers, called by main.py:102 in every shipped launcher): the
# leading run of stages in which no parameter requires a gradient - the front end (visual: patch / class / position embedding +
# ln_pre; text: token + position embedding), then blocks 0, 1, ...  Nothing in it needs activations for a backward, so it runs
# under no_grad in ONE enqueue of the inference path's kernels (cc_vit_encode_prefix_frames / cc_text_encode_prefix) and hands the
# first trainable block the fp32 residual stream.
_GLUE_FRONT = False      # private, for the tests: True = the towers' fronts as torch glue + per-op launches whatever is frozen


def _none_trainable(params):
    return not any(p.requires_grad for p in params)


def _prefix_blocks(transformer):
    n = 0
    for blk in transformer.resblocks:
        tc = blk.tokencluster_inter
        if not _none_trainable(blk.parameters()) or (tc is not None and getattr(tc, "mean_residual", False)):
            break
        n += 1
    return n


def visual_prefix_blocks(vis):
    """Number of leading blocks in the visual tower's frozen prefix (0: the front end alone), None: no frozen prefix."""
    if _GLUE_FRONT or vis.linear_patch != '2d' or not _none_trainable(vis.prefix_parameters(0)):
        return None
    return _prefix_blocks(vis.transformer)


def text_prefix_blocks(clip):
    """The text tower's counterpart of visual_prefix_blocks."""
    if _GLUE_FRONT or not _none_trainable(clip.text_prefix_parameters(0)):
        return None
    return _prefix_blocks(clip.transformer)


def encode_image_train(clip, video, video_frame):
    """CLIP.encode_image (modules/clip.py:460-469 with VisualTransformer.forward :320-345, linear_patch '2d') with gradients:
    video [F, 3, H, W] fp32, or the loader's uint8 frames [F, 3, H, W] / [F, H, W, 3] (the patch gather applies
    dataloaders/transforms.py's u8/255 -> (x - mean)/std) -> (features [F', embed_dim], cluster_loss)."""
    vis = clip.visual
    if vis.linear_patch != '2d':
        raise NotImplementedError("training towers: linear_patch='3d' is not built")
    L.require_device(video)
    F, p, W = video.shape[0], vis.patch_size, vis.width
    g = vis.input_resolution // p
    n = visual_prefix_blocks(vis)
    if n is not None:
        with torch.no_grad():
            x = vis.encode_prefix(video, video_frame, n, forced_medoids=getattr(vis, "forced_medoids", None))
        # (frame-major rows: the first trainable block's own permute back finds them contiguous, no copy)
        x = _blocks(vis.transformer, x.permute(1, 0, 2), start=n).permute(1, 0, 2)
    else:
        if _GLUE_FRONT or (p % 8 and video.dtype != torch.uint8):
            # (a patch size off the gather's 8-wide grid - no CLIP tower has one - keeps the reshape, as before)
            if video.dtype == torch.uint8:
                raise ValueError("the torch-glue front takes normalised float frames")
            # conv1 (kernel = stride = p, no bias) as a GEMM over the patch rows (c, kh, kw) - a reshape of the frames
            a = video.float().view(F, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F * g * g, 3 * p * p)
        else:
            # the encoders' patch gather: the fp16 patch matrix straight from the frames - LinearFunction's operand and saved
            # activation (no fp32 permute-copy of the patches, no separate cast)
            a = torch.ops.centerclip.patch_gather(video if video.dtype == torch.uint8 else video.float(), vis.input_resolution, p)
        x = LinearFunction.apply(a, vis.conv1.weight.view(W, -1), None).view(F, g * g, W)
        cls = vis.class_embedding.to(x.dtype) + torch.zeros(F, 1, W, dtype=x.dtype, device=x.device)
        x = torch.cat([cls, x], dim=1) + vis.positional_embedding.to(x.dtype)
        x = _layernorm(vis.ln_pre, x.reshape(F * (g * g + 1), W)).view(F, g * g + 1, W)
        x = _blocks(vis.transformer, x.permute(1, 0, 2).contiguous()).permute(1, 0, 2)          # NLD -> LND -> NLD
    cls_rows = x[:, 0, :].contiguous()                        # ln_post(x) @ proj, of which encode_image keeps the CLS row
    feats = LinearFunction.apply(_layernorm(vis.ln_post, cls_rows), vis.proj.t(), None)
    return feats, torch.zeros((), device=video.device)


def encode_text_train(clip, ids):
    """CLIP.encode_text (modules/clip.py:471-496) with gradients: ids [B, n_ctx] -> [B, embed_dim]."""
    L.require_device(ids)
    B, n_ctx = ids.shape
    W = clip.transformer.width
    n = text_prefix_blocks(clip)
    if n is not None:
        with torch.no_grad():
            x = clip.encode_text_prefix(ids, n)
        x = _blocks(clip.transformer, x.permute(1, 0, 2), start=n).permute(1, 0, 2).contiguous()
    else:
        # (autograd records nothing for a tensor that does not require a gradient: a frozen token_embedding gets no scatter-add)
        x = clip.token_embedding(ids).float() + clip.positional_embedding[:n_ctx].float()
        x = _blocks(clip.transformer, x.permute(1, 0, 2).contiguous()).permute(1, 0, 2).contiguous()
    eot = x[torch.arange(B, device=x.device), ids.argmax(dim=-1)]                             # the EOT token has the largest id
    return LinearFunction.apply(_layernorm(clip.ln_final, eot.contiguous()), clip.text_projection.t(), None)


# ================================================================================================ BertAdam
def warmup_cosine(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    import math
    return 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x, warmup=0.002):
    return x / warmup if x < warmup else 1.0


def warmup_linear(x, warmup=0.002):
    return x / warmup if x < warmup else max((x - 1.) / (warmup - 1.), 0)


SCHEDULES = {'warmup_cosine': warmup_cosine, 'warmup_constant': warmup_constant, 'warmup_linear': warmup_linear}


class BertAdam(torch.optim.Optimizer):
    """utils/optimization.py:55-170 (the optimizer main.py:161-167 builds): same constructor, same state names
    ('step', 'next_m', 'next_v'), same per-tensor clipping / decoupled weight decay / schedule; the tensor arithmetic of a
    step is one cc_bertadam_step_f32 call per parameter (no host synchronisation)."""

    def __init__(self, params, lr, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, capturable=False):
        # capturable (not in the reference): the scheduled learning rate of each group reaches the kernels through a device
        # float, so a step captured into a hipGraph can be replayed with the schedule's next value (GraphedTrainStep)
        self.capturable = bool(capturable)
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        super().__init__(params, dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e,
                                      weight_decay=weight_decay, max_grad_norm=max_grad_norm))

    @staticmethod
    def _lr(group, step):
        if group['t_total'] != -1:
            return group['lr'] * SCHEDULES[group['schedule']](step / group['t_total'], group['warmup'])
        return group['lr']

    def get_lr(self):
        lr = []
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    return [0]
                lr.append(self._lr(group, state['step']))
        return lr

    _MULTI_MAX_N = 8192                     # CC_BERTADAM_MULTI_MAX_N (include/centerclip_hip.h)

    def _multi_small(self, items, hyper, capturing, device):
        """All small tensors of groups with the same (b1, b2, e, max_grad_norm) in ONE launch (cc_bertadam_multi_f32): the
        records (cc_bertadam_item: four tensor pointers, the group's device learning rate, n, weight decay) are staged through
        pinned memory and re-sent only when a pointer changed.  A captured step owns its own staging buffers (the graph replays
        the host-to-device copy), allocated during the eager warm-up that precedes the capture."""
        import numpy as np
        rec = np.zeros(len(items), dtype=np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('lr_dev', '<u8'),
                                                   ('n', '<i4'), ('lr', '<f4'), ('wd', '<f4'), ('pad', '<i4')]))
        for i, (p, grad, m, v, lr_dev, wd) in enumerate(items):
            rec[i] = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), lr_dev.data_ptr(), p.numel(), 0.0, wd, 0)
        raw = rec.tobytes()
        slot = self._multi.setdefault(hyper, {})
        if capturing:
            host, dev = slot.pop("spare", (None, None))
            if host is None or host.numel() != len(raw):
                raise RuntimeError("BertAdam: run one eager step with the same parameters before capturing (staging buffers)")
            host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            dev.copy_(host, non_blocking=True)
            self._multi_keep.append((host, dev))                  # the graph reads both on every replay
        else:
            if slot.get("raw") != raw:
                host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
                if slot.get("dev") is None or slot["dev"].numel() != len(raw):
                    slot["dev"] = torch.empty(len(raw), dtype=torch.uint8, device=device)
                slot["dev"].copy_(host, non_blocking=True)
                slot["raw"] = raw
            if "spare" not in slot or slot["spare"][0].numel() != len(raw):
                slot["spare"] = (torch.empty(len(raw), dtype=torch.uint8).pin_memory(),
                                 torch.empty(len(raw), dtype=torch.uint8, device=device))
            dev = slot["dev"]
        b1, b2, e, max_norm = hyper
        sc = getattr(self, "_sc", None)
        if sc is not None:
            _check(L.lib().cc_bertadam_multi_scaled_f32(L.ptr(dev), len(items), b1, b2, e, max_norm, L.ptr(sc[0]), L.ptr(sc[1]),
                                                        _st(dev)), "cc_bertadam_multi_scaled_f32")
            return
        _check(L.lib().cc_bertadam_multi_f32(L.ptr(dev), len(items), b1, b2, e, max_norm, _st(dev)), "cc_bertadam_multi_f32")

    def _multi_large(self, items, hyper, capturing, device):
        """All large tensors of groups with the same (b1, b2, e, max_grad_norm) in TWO launches (cc_bertadam_multi_large_f32:
        every tensor's norm workgroups, then every tensor's step workgroups) instead of two per tensor - ~100 tensors of a
        ViT-B/32 CLIP: 204 launches -> 2.  Records (cc_bertadam_big_item) staged like the small tensors' (see _multi_small)."""
        import numpy as np
        lib = L.lib()
        rec = np.zeros(len(items), dtype=np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('lr_dev', '<u8'),
                                                   ('n', '<i8'), ('lr', '<f4'), ('wd', '<f4'), ('nb0', '<i4'), ('nb', '<i4'),
                                                   ('sb0', '<i4'), ('sb', '<i4')]))
        nb0 = sb0 = 0
        for i, (p, grad, m, v, lr_dev, wd) in enumerate(items):
            nb, sb = int(lib.cc_bertadam_norm_blocks(p.numel())), int(lib.cc_bertadam_step_blocks(p.numel()))
            rec[i] = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), lr_dev.data_ptr(), p.numel(), 0.0, wd, nb0, nb, sb0, sb)
            nb0 += nb
            sb0 += sb
        raw = rec.tobytes()
        slot = self._multi.setdefault((hyper, "large"), {})
        if slot.get("partial") is None or slot["partial"].numel() < nb0:
            if capturing:
                raise RuntimeError("BertAdam: run one eager step with the same parameters before capturing (partial sums)")
            slot["partial"] = torch.empty(nb0, dtype=torch.float64, device=device)
        if capturing:
            host, dev = slot.pop("spare", (None, None))
            if host is None or host.numel() != len(raw):
                raise RuntimeError("BertAdam: run one eager step with the same parameters before capturing (staging buffers)")
            host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            dev.copy_(host, non_blocking=True)
            self._multi_keep.append((host, dev))
        else:
            if slot.get("raw") != raw:
                host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
                if slot.get("dev") is None or slot["dev"].numel() != len(raw):
                    slot["dev"] = torch.empty(len(raw), dtype=torch.uint8, device=device)
                slot["dev"].copy_(host, non_blocking=True)
                slot["raw"] = raw
            if "spare" not in slot or slot["spare"][0].numel() != len(raw):
                slot["spare"] = (torch.empty(len(raw), dtype=torch.uint8).pin_memory(),
                                 torch.empty(len(raw), dtype=torch.uint8, device=device))
            dev = slot["dev"]
        b1, b2, e, max_norm = hyper
        part = slot["partial"]
        sc = getattr(self, "_sc", None)
        if sc is not None:
            _check(lib.cc_bertadam_multi_large_scaled_f32(L.ptr(dev), len(items), nb0, sb0, b1, b2, e, max_norm, L.ptr(part),
                                                          part.numel() * 8, L.ptr(sc[0]), L.ptr(sc[1]), _st(dev)),
                   "cc_bertadam_multi_large_scaled_f32")
            return
        _check(lib.cc_bertadam_multi_large_f32(L.ptr(dev), len(items), nb0, sb0, b1, b2, e, max_norm, L.ptr(part),
                                               part.numel() * 8, _st(dev)), "cc_bertadam_multi_large_f32")

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lib = L.lib()
        capturing = self.capturable and torch.cuda.is_current_stream_capturing()
        if not hasattr(self, "_lr_dev"):
            self._lr_dev = {}                                     # group index -> 1-element device tensor (not optimizer state)
            self._multi, self._multi_keep = {}, []
        small, large = {}, {}                                     # (b1, b2, e, max_grad_norm) -> records of the small / large tensors
        sc = getattr(self, "_sc", None)                           # (multiplier, found_inf) device floats: DeviceGradScaler.step
        if not capturing:
            self._last = []                                       # the parameters this step counts (for _uncount)
        for gi, group in enumerate(self.param_groups):
            lr_set = False
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("BertAdam (HIP): fp32 contiguous parameters (the master weights)")
                L.require_device(p)
                grad = p.grad if (p.grad.dtype == torch.float32 and p.grad.is_contiguous()) else None
                if grad is None:
                    p.grad = p.grad.float().contiguous()
                    grad = p.grad
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['next_m'] = torch.zeros_like(p)
                    state['next_v'] = torch.zeros_like(p)
                ws = L.workspace(lib.cc_bertadam_workspace_bytes(), p.device)
                lr_dev = None
                if self.capturable:
                    lr_dev = self._lr_dev.get(gi)
                    if lr_dev is None or lr_dev.device != p.device:
                        lr_dev = self._lr_dev[gi] = torch.zeros(1, device=p.device, dtype=torch.float32)
                    if not capturing and not lr_set:
                        lr_dev.fill_(float(self._lr(group, state['step'])))
                        lr_set = True
                if self.capturable and p.numel() <= self._MULTI_MAX_N:
                    hyper = (float(group['b1']), float(group['b2']), float(group['e']), float(group['max_grad_norm']))
                    small.setdefault(hyper, []).append((p, grad, state['next_m'], state['next_v'], lr_dev, float(group['weight_decay'])))
                elif self.capturable:
                    hyper = (float(group['b1']), float(group['b2']), float(group['e']), float(group['max_grad_norm']))
                    large.setdefault(hyper, []).append((p, grad, state['next_m'], state['next_v'], lr_dev, float(group['weight_decay'])))
                elif sc is not None:
                    _check(lib.cc_bertadam_step_scaled_f32(L.ptr(p), L.ptr(grad), L.ptr(state['next_m']), L.ptr(state['next_v']),
                                                           p.numel(), float(self._lr(group, state['step'])), float(group['b1']),
                                                           float(group['b2']), float(group['e']), float(group['weight_decay']),
                                                           float(group['max_grad_norm']), L.ptr(lr_dev), L.ptr(ws), ws.numel(),
                                                           L.ptr(sc[0]), L.ptr(sc[1]), _st(p)), "cc_bertadam_step_scaled_f32")
                else:
                    _check(lib.cc_bertadam_step_f32(L.ptr(p), L.ptr(grad), L.ptr(state['next_m']), L.ptr(state['next_v']), p.numel(),
                                                    float(self._lr(group, state['step'])), float(group['b1']), float(group['b2']),
                                                    float(group['e']), float(group['weight_decay']), float(group['max_grad_norm']),
                                                    L.ptr(lr_dev), L.ptr(ws), ws.numel(), _st(p)), "cc_bertadam_step_f32")
                if not capturing:
                    state['step'] += 1
                    self._last.append(p)
        for hyper, items in small.items():
            self._multi_small(items, hyper, capturing, items[0][0].device)
        for hyper, items in large.items():
            self._multi_large(items, hyper, capturing, items[0][0].device)
        return loss

    @torch.no_grad()
    def _scaled_step(self, scaler, max_norm):
        """DeviceGradScaler.step: the statistics over every gradient of the step (norm of the unscaled gradients, the
        multiplier inv_scale * global clip coefficient, found_inf), then step() on the *_scaled_f32 launches."""
        grads = []
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                L.require_device(p)
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                grads.append(p.grad)
        if not grads:
            return False
        raw, count, nblk = _adamw_table([(g, g, None, None, 0) for g in grads])
        if not hasattr(self, "_stat_staged"):
            self._stat_staged = {}
        table = self._stat_staged.setdefault(len(raw), _Staged("BertAdam")).upload(raw, grads[0].device, _capturing())
        self._sc = scaler._stats(table, count, nblk, max_norm, grads[0].device)
        try:
            self.step()
        finally:
            self._sc = None
        return True

    def _uncount(self):
        """The last eager step turned out to be skipped on the device (DeviceGradScaler): take its count back."""
        for p in getattr(self, "_last", ()):
            self.state[p]['step'] -= 1
        self._last = []

    def refresh_lr(self):
        """capturable: write every group's scheduled learning rate (from the host-side step counts) into its device float -
        call before replaying a captured step."""
        for gi, group in enumerate(self.param_groups):
            steps = [self.state[p]['step'] for p in group['params'] if p in self.state and len(self.state[p])]
            if steps and getattr(self, "_lr_dev", {}).get(gi) is not None:
                self._lr_dev[gi].fill_(float(self._lr(group, steps[0])))

    def advance(self):
        """capturable: count one replayed step for every parameter that has state."""
        for group in self.param_groups:
            for p in group['params']:
                if p in self.state and len(self.state[p]):
                    self.state[p]['step'] += 1


# ================================================================================================ AdamW + global clipping
# torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ (main.py:168-175, 316-333) on the multi-tensor kernels of
# csrc/adamw.hip: one record per tensor (cc_adamw_item), every tensor of a step in one launch.
_ADAMW_ITEM = None
_adamw_blocks_cache = {}


def _adamw_item_dtype():
    global _ADAMW_ITEM
    if _ADAMW_ITEM is None:
        import numpy as np
        _ADAMW_ITEM = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('n', '<i8'), ('blk0', '<i4'),
                                ('blocks', '<i4'), ('scal', '<i4'), ('pad', '<i4')])
    return _ADAMW_ITEM


def _adamw_table(entries):
    """entries: (param, grad, exp_avg or None, exp_avg_sq or None, scalar index) -> (cc_adamw_item records as bytes, count,
    total blocks).  Empty tensors get no record."""
    import numpy as np
    lib = L.lib()
    entries = [e for e in entries if e[0].numel() > 0]
    rec = np.zeros(len(entries), dtype=_adamw_item_dtype())
    blk0 = 0
    for i, (p, g, m, v, si) in enumerate(entries):
        n = p.numel()
        nb = _adamw_blocks_cache.get(n)
        if nb is None:
            nb = _adamw_blocks_cache[n] = int(lib.cc_adamw_blocks(n))
        rec[i] = (p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(), n, blk0, nb,
                  si, 0)
        blk0 += nb
    return rec.tobytes(), len(entries), blk0


class _Staged:
    """A small host-built table in device memory (the cc_adamw_item records, the per-class scalars): uploaded through pinned
    memory when its bytes change.  A captured step stages its own copy - the graph replays that host-to-device copy from a
    pinned buffer set aside during the eager warm-up, so later eager uploads never touch what the graph reads."""

    def __init__(self, who):
        self.who, self.raw, self.dev, self.spare, self.keep = who, None, None, None, []

    def upload(self, raw, device, capturing):
        if capturing:
            host, dev = self.spare if self.spare is not None else (None, None)
            self.spare = None
            if host is None or host.numel() != len(raw):
                raise RuntimeError("%s: run one eager step with the same parameters before capturing (staging buffers)" % self.who)
            host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            dev.copy_(host, non_blocking=True)
            self.keep.append((host, dev))                     # the graph reads both on every replay
            return dev
        if self.raw != raw:
            host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
            if self.dev is None or self.dev.numel() != len(raw) or self.dev.device != device:
                self.dev = torch.empty(len(raw), dtype=torch.uint8, device=device)
            self.dev.copy_(host, non_blocking=True)
            self.raw = raw
        if self.spare is None or self.spare[0].numel() != len(raw):
            self.spare = (torch.empty(len(raw), dtype=torch.uint8).pin_memory(),
                          torch.empty(len(raw), dtype=torch.uint8, device=device))
        return self.dev


def _clip_launches(table, count, nblk, max_norm, device, coef_only=False):
    """||g|| over the table's gradients and the clip coefficient -> a [2] device float tensor (norm, coef); unless coef_only,
    the gradients are multiplied by the coefficient in place (cc_grad_scale_f32)."""
    lib = L.lib()
    out = torch.empty(2, dtype=torch.float32, device=device)
    ws = L.workspace(lib.cc_grad_norm_workspace_bytes(nblk), device)
    st = _st(out)
    _check(lib.cc_grad_norm_partials_f32(L.ptr(table), count, nblk, L.ptr(ws), ws.numel(), st), "cc_grad_norm_partials_f32")
    _check(lib.cc_grad_clip_coef_f32(L.ptr(ws), nblk, float(max_norm), L.ptr(out), st), "cc_grad_clip_coef_f32")
    if not coef_only:
        _check(lib.cc_grad_scale_f32(L.ptr(table), count, nblk, L.ptr(out[1:]), st), "cc_grad_scale_f32")
    return out


_clip_staged = {}


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ (L2): the gradients are scaled in place by min(1, max_norm / (||g|| + 1e-6)), and the
    total norm comes back as a 0-d device tensor.  HIP kernels only (cc_grad_norm_partials_f32 -> cc_grad_clip_coef_f32 ->
    cc_grad_scale_f32): no host synchronisation, capturable.  The fp64 partial sums are added in the order of `parameters`,
    so the same parameters in the same order give the same bits."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_ (HIP): only the L2 norm (norm_type=2), as main.py uses it")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        L.require_device(g)
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
            raise RuntimeError("clip_grad_norm_ (HIP): fp32 contiguous gradients on one device")
    raw, count, nblk = _adamw_table([(g, g, None, None, 0) for g in grads])
    if count == 0:
        return torch.zeros((), dtype=torch.float32, device=dev)
    capturing = _capturing()
    slot = _clip_staged.setdefault((dev, len(raw)), _Staged("clip_grad_norm_"))
    table = slot.upload(raw, dev, capturing)
    return _clip_launches(table, count, nblk, max_norm, dev)[0]


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (the optimizer main.py:168-175 builds for --optim AdamW): same constructor and validation, same state
    names ('step', 'exp_avg', 'exp_avg_sq': a state_dict loads into torch.optim.AdamW and back), the reference's extra group
    keys ('lr_mult', 'decay_mult', written by lr_scheduler) pass through.  A step is ONE cc_adamw_multi_f32 launch over every
    tensor with a gradient; the per-(group, step count) scalars (1 - lr wd, lr / (1 - b1^t), sqrt(1 - b2^t), ...) are host
    arithmetic in double, as torch computes them, and reach the kernel through a small device array.

    capturable=True: the record table and the scalars are staged so that a step captured into a hipGraph can be replayed -
    refresh_lr() before a replay writes the scalars for the groups' current lr / weight_decay and the next step count,
    advance() after it counts the step (the protocol of BertAdam, used by GraphedTrainStep)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 capturable=False):
        if amsgrad:
            raise ValueError("AdamW (HIP): amsgrad=True is not supported (the reference trains without it)")
        if maximize:
            raise ValueError("AdamW (HIP): maximize=True is not supported (the reference trains without it)")
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.capturable = bool(capturable)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    def load_state_dict(self, state_dict):
        """Also takes torch.optim.AdamW's state (a tensor-valued 'step', its extra group keys)."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if torch.is_tensor(st.get('step')):
                st['step'] = int(st['step'].item())

    @staticmethod
    def _scalars(group, t):
        """cc_adamw_scalars of a group at step count t (after the step), in torch's double arithmetic."""
        b1, b2 = (float(b) for b in group['betas'])
        lr, wd = float(group['lr']), float(group['weight_decay'])
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        return (1 - lr * wd, b1, 1 - b1, b2, 1 - b2, lr / bc1, bc2 ** 0.5, float(group['eps']))

    def _upload_scalars(self, rows, device):
        import numpy as np
        arr = np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(-1)
        host = torch.from_numpy(arr).pin_memory()
        dev = getattr(self, "_scal_dev", None)
        if dev is None or dev.numel() < arr.size or dev.device != device:
            if getattr(self, "_cap", None) is not None:
                raise RuntimeError("AdamW: more (group, step count) classes than when the step was captured")
            dev = self._scal_dev = torch.zeros(max(arr.size, 8 * 16), dtype=torch.float32, device=device)
        dev[:arr.size].copy_(host, non_blocking=True)
        return dev

    def _prepare(self):
        """-> (device, table, count, total blocks, scalars) for the parameters that have a gradient; advances the step counts
        unless a capture is running."""
        capturing = _capturing()
        if capturing and not self.capturable:
            raise RuntimeError("AdamW: build it with capturable=True to capture its step")
        entries, classes, dev = [], {}, None
        for gi, group in enumerate(self.param_groups):
            if group.get('amsgrad') or group.get('maximize'):
                raise ValueError("AdamW (HIP): amsgrad / maximize are not supported")
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("AdamW (HIP): sparse gradients are not supported")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("AdamW (HIP): fp32 contiguous parameters (the master weights)")
                L.require_device(p)
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError("AdamW (HIP): all parameters on one device")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif torch.is_tensor(state['step']):
                    state['step'] = int(state['step'].item())
                t = state['step'] + 1
                ci = classes.setdefault((gi, t), (len(classes), p))[0]
                entries.append((p, p.grad, state['exp_avg'], state['exp_avg_sq'], ci))
                if not capturing:
                    state['step'] = t
        if not capturing:
            self._last = [e[0] for e in entries]                  # the parameters this step counts (for _uncount)
        if not entries:
            return None
        raw, count, nblk = _adamw_table(entries)
        if not hasattr(self, "_staged"):
            self._staged = {}
        table = self._staged.setdefault(len(raw), _Staged("AdamW")).upload(raw, dev, capturing)
        ordered = sorted(classes.items(), key=lambda kv: kv[1][0])
        if capturing:
            # what refresh_lr / advance need: per class its group and one of its parameters (whose step count is the class's)
            if getattr(self, "_scal_dev", None) is None or self._scal_dev.numel() < 8 * len(ordered):
                raise RuntimeError("AdamW: run one eager step with the same parameters before capturing (scalars)")
            self._cap = dict(classes=[(gi, p) for (gi, _), (_, p) in ordered], params=[e[0] for e in entries])
            scal = self._scal_dev
        else:
            scal = self._upload_scalars([self._scalars(self.param_groups[gi], t) for (gi, t), _ in ordered], dev)
        return dev, table, count, nblk, scal

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        prep = self._prepare()
        if prep is not None:
            dev, table, count, nblk, scal = prep
            _check(L.lib().cc_adamw_multi_f32(L.ptr(table), count, nblk, L.ptr(scal), None, _st(scal)), "cc_adamw_multi_f32")
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_norm):
        """clip_grad_norm_(the parameters with a gradient, max_norm) followed by step(), fused: the step launch multiplies each
        gradient by the device-side clip coefficient as it loads it and writes the clipped gradient back (one read-modify-write
        pass over the gradients less).  Bit for bit clip_grad_norm_ over the same parameters in group order + step().
        -> the total norm before clipping (0-d device tensor)."""
        prep = self._prepare()
        if prep is None:
            return torch.tensor(0.0)
        dev, table, count, nblk, scal = prep
        out = _clip_launches(table, count, nblk, max_norm, dev, coef_only=True)
        _check(L.lib().cc_adamw_multi_f32(L.ptr(table), count, nblk, L.ptr(scal), L.ptr(out[1:]), _st(scal)),
               "cc_adamw_multi_f32")
        return out[0]

    @torch.no_grad()
    def _scaled_step(self, scaler, max_norm):
        """DeviceGradScaler.step: norm partials -> cc_grad_scaler_stats_f32 (norm of the unscaled gradients, the multiplier
        inv_scale * clip coefficient, found_inf) -> cc_adamw_multi_scaled_f32, which applies the multiplier as it loads each
        gradient and writes nothing when found_inf is set.  No pass unscales the gradients."""
        prep = self._prepare()
        if prep is None:
            return False
        dev, table, count, nblk, scal = prep
        mult, found = scaler._stats(table, count, nblk, max_norm, dev)
        _check(L.lib().cc_adamw_multi_scaled_f32(L.ptr(table), count, nblk, L.ptr(scal), L.ptr(mult), L.ptr(found), _st(scal)),
               "cc_adamw_multi_scaled_f32")
        return True

    def _uncount(self):
        """The last eager step turned out to be skipped on the device (DeviceGradScaler): take its count back."""
        for p in getattr(self, "_last", ()):
            self.state[p]['step'] -= 1
        self._last = []

    def refresh_lr(self):
        """capturable: write the captured step's scalars (each group's current lr / weight_decay, the next step count) into
        their device array - call before replaying a captured step."""
        cap = getattr(self, "_cap", None)
        if cap is None:
            return
        rows = [self._scalars(self.param_groups[gi], self.state[p]['step'] + 1) for gi, p in cap['classes']]
        self._upload_scalars(rows, self._scal_dev.device)

    def advance(self):
        """capturable: count one replayed step for every parameter the captured step updates."""
        cap = getattr(self, "_cap", None)
        for p in (cap['params'] if cap is not None else ()):
            self.state[p]['step'] += 1


class lr_scheduler:
    """The reference's per-iteration learning-rate scheduler (utils/lr_scheduler.py, main.py:171-174 with mode 'cos'), written
    to its interface: a linear slow start from slow_start_lr over slow_start_iters iterations, then
      cos   lr = init_lr / 2 (1 + cos(pi T / total))            poly  lr = init_lr (1 - T / total)^0.9
      HTD   lr = init_lr / 2 (1 - tanh(lower + (upper - lower) T / total))
      step  lr = init_lr multiplier^(epoch // lr_step), or ^(number of milestones passed)
    with T counted from the end of the slow start and total = all_iters - slow_start_iters, clamped below at end_lr.  A call
    writes lr * lr_mult and weight_decay * decay_mult into every parameter group.  Host arithmetic only."""

    def __init__(self, mode='cos', init_lr=0.1, all_iters=300, lr_milestones=None, lr_step=100, lr_step_multiplier=0.1,
                 slow_start_iters=0, slow_start_lr=1e-8, end_lr=1e-8, lower_bound=-6.0, upper_bound=3.0, weight_decay=1e-4,
                 iters_per_epoch=None):
        if mode not in ('cos', 'poly', 'HTD', 'step'):
            raise ValueError("lr_scheduler: mode must be one of 'cos', 'poly', 'HTD', 'step', got %r" % (mode,))
        self.mode, self.init_lr, self.now_lr, self.end_lr = mode, init_lr, init_lr, end_lr
        self.slow_start_iters, self.slow_start_lr = slow_start_iters, slow_start_lr
        self.total_iters = all_iters - slow_start_iters
        self.lr_step, self.lr_milestones, self.lr_step_multiplier = lr_step, lr_milestones, lr_step_multiplier
        self.lower_bound, self.upper_bound = lower_bound, upper_bound
        self.weight_decay = weight_decay
        self.iters_per_epoch = iters_per_epoch             # (only for calls without global_step)

    def lr_at(self, T, epoch=None):
        """The learning rate at iteration T (epoch: for mode 'step')."""
        import math
        if self.slow_start_iters > 0 and T <= self.slow_start_iters:
            lr = (1.0 * T / self.slow_start_iters) * (self.init_lr - self.slow_start_lr)
            lr = min(lr + self.slow_start_lr, self.init_lr)
        elif self.mode == 'cos':
            lr = 0.5 * self.init_lr * (1.0 + math.cos(1.0 * (T - self.slow_start_iters) / self.total_iters * math.pi))
        elif self.mode == 'poly':
            lr = self.init_lr * pow(1.0 - 1.0 * (T - self.slow_start_iters) / self.total_iters, 0.9)
        elif self.mode == 'HTD':
            ratio = 1.0 * (T - self.slow_start_iters) / self.total_iters
            lr = 0.5 * self.init_lr * (1.0 - math.tanh(self.lower_bound + (self.upper_bound - self.lower_bound) * ratio))
        elif self.lr_milestones is None:
            lr = self.init_lr * (self.lr_step_multiplier ** (epoch // self.lr_step))
        else:
            lr = self.init_lr * (self.lr_step_multiplier ** sum(1 for mile in self.lr_milestones if epoch >= mile))
        return max(lr, self.end_lr)

    def __call__(self, optimizer, i=None, epoch=None, global_step=None):
        T = (epoch * self.iters_per_epoch + i) if global_step is None else global_step
        lr = self.now_lr = self.lr_at(T, epoch)
        for group in optimizer.param_groups:
            group['lr'] = lr * group['lr_mult']
            group['weight_decay'] = self.weight_decay * group['decay_mult']


def prep_optim_params_groups(args, model, coef_lr=1.):
    """utils/optimization.py:173-222: CLIP parameters at lr * coef_lr, newly added modules at lr, no weight decay for biases /
    LayerNorm.  BertAdam (the default): 'lr' / 'weight_decay' per group; args.optim == 'AdamW': every group at args.lr with
    the 'lr_mult' / 'decay_mult' keys that lr_scheduler applies."""
    model = getattr(model, 'module', model)
    named = list(model.named_parameters())
    no_decay = ['bias', 'LayerNorm.bias', 'LayerNorm.weight']
    no_clip = args.new_added_modules
    dec = [(n, p) for n, p in named if not any(nd in n for nd in no_decay)]
    nodec = [(n, p) for n, p in named if any(nd in n for nd in no_decay)]
    is_clip = lambda n: "clip." in n and not any(nd in n for nd in no_clip)
    if getattr(args, 'optim', 'BertAdam') == 'AdamW':
        return [{'params': [p for n, p in dec if is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr, 'lr_mult': coef_lr,
                 'decay_mult': 1},
                {'params': [p for n, p in nodec if is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr, 'lr_mult': coef_lr,
                 'decay_mult': 0.0},
                {'params': [p for n, p in dec if not is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr, 'lr_mult': 1.0,
                 'decay_mult': 1.0},
                {'params': [p for n, p in nodec if not is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr, 'lr_mult': 1.0,
                 'decay_mult': 0.0}]
    return [{'params': [p for n, p in dec if is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr * coef_lr},
            {'params': [p for n, p in nodec if is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr * coef_lr},
            {'params': [p for n, p in dec if not is_clip(n)], 'weight_decay': args.wd},
            {'params': [p for n, p in nodec if not is_clip(n)], 'weight_decay': 0.0}]


# ================================================================================================ loss scaling on the device
class DeviceGradScaler:
    """torch.amp.GradScaler's recipe (main.py:160, 320-328: scale(loss).backward(), unscale_, clip, step, update) with every
    decision on the device, so that the same object runs eagerly in train_epoch and inside a captured GraphedTrainStep:

        scale(loss)            loss * scale (the device float; the HIP backward passes a power of two through exactly)
        unscale_(optimizer)    launches NOTHING: the gradients stay scaled in memory until step() - no pass over them exists
        clip_grad_norm_(optimizer, max_norm)   (after unscale_) asks step() for global clipping of the unscaled gradients
        step(optimizer)        the norm partials of every gradient -> cc_grad_scaler_stats_f32 (norm of the unscaled
                               gradients, ONE multiplier inv_scale * clip coefficient, found_inf) -> the optimizer's
                               *_scaled_f32 launches, which apply the multiplier as they load a gradient (and store that
                               value back) and write nothing at all when found_inf is set.  Only centerclip_amd.train.AdamW /
                               BertAdam have such launches: any other optimizer raises.
        update(new_scale=None) cc_grad_scaler_update_f32, GradScaler.update's rule (backoff on found_inf, growth after
                               growth_interval clean steps in a row), plus two device counters: steps taken / skipped.

    The state_dict has torch's keys (scale, growth_factor, backoff_factor, growth_interval, _growth_tracker): a checkpoint
    written from either class loads into the other.

    Step counts.  A skipped step must not advance the optimizer's state['step'] (bias correction, BertAdam's schedule), and
    whether a step was skipped is known on the device only.  Design: the flag is copied into a pinned host word right behind
    the optimizer launch (inside the graph when captured), and the count of step k is settled at the START of step k + 1 -
    sync() waits for step k's event and then either takes back the count an eager step() advanced, or lets a captured step's
    optimizer advance().  Nothing waits between enqueueing a step's work and its end.  The alternative - counts and the
    per-class scalars (1 - b1^t, the schedules) on the device - would have to restate torch's double-precision host arithmetic
    there, bit for bit, for both optimizers; the deferred count keeps that arithmetic where it is.  Call sync() (or
    GraphedTrainStep.sync()) before reading optimizer.state_dict()."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)
        if self._enabled:
            if not float(init_scale) > 0.0:
                raise ValueError("DeviceGradScaler: init_scale must be > 0, got %r" % (init_scale,))
            if not float(growth_factor) > 1.0:
                raise ValueError("DeviceGradScaler: the growth factor must be > 1.0, got %r" % (growth_factor,))
            if not 0.0 < float(backoff_factor) < 1.0:
                raise ValueError("DeviceGradScaler: the backoff factor must be in (0, 1), got %r" % (backoff_factor,))
            if int(growth_interval) != growth_interval or int(growth_interval) < 1:
                raise ValueError("DeviceGradScaler: growth_interval must be a positive integer, got %r" % (growth_interval,))
        self._init_scale, self._growth_factor = float(init_scale), float(growth_factor)
        self._backoff_factor, self._growth_interval = float(backoff_factor), int(growth_interval)
        self._init_growth_tracker = 0
        self._f = None            # device float32 [8]: scale, 1 / scale, norm, multiplier, found_inf
        self._c = None            # device int32 [4]: growth tracker, steps taken, steps skipped
        self._pin = self._event = self._pending = None
        self._unscaled, self._max_norm, self._stepped = set(), {}, False

    # ------------------------------------------------------------------------------------------------ state
    def _ensure(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.CenterClipHipError("DeviceGradScaler runs on MI355X only: got a %s tensor (no CPU fallback)" % device)
        if self._f is None:
            self._f = torch.zeros(8, dtype=torch.float32, device=device)
            self._c = torch.zeros(4, dtype=torch.int32, device=device)
            self._pin = torch.zeros(1, dtype=torch.float32).pin_memory()
            self._event = torch.cuda.Event()
            self._set_scale(self._init_scale)
            self._c[0] = self._init_growth_tracker
        elif self._f.device != device:
            raise RuntimeError("DeviceGradScaler: one device per scaler (%s, then %s)" % (self._f.device, device))

    def _set_scale(self, value):
        if torch.is_tensor(value):
            if value.numel() != 1 or value.requires_grad:
                raise ValueError("DeviceGradScaler.update: new_scale must be a float or a 1-element tensor without a gradient")
            self._f[0:1].copy_(value.detach().reshape(1).to(torch.float32))
        else:
            self._f[0:1].fill_(float(value))
        self._f[1:2].copy_(self._f[0:1].double().reciprocal().float())        # as GradScaler._unscale_grads_ computes it

    def is_enabled(self):
        return self._enabled

    def get_scale(self):
        if not self._enabled:
            return 1.0
        return self._init_scale if self._f is None else float(self._f[0])

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def counters(self):
        """-> (steps taken, steps skipped) as update() has counted them on the device (reads the device: synchronises)."""
        if self._c is None:
            return 0, 0
        c = self._c.tolist()
        return int(c[1]), int(c[2])

    def state_dict(self):
        if not self._enabled:
            return {}
        tracker = self._init_growth_tracker if self._c is None else int(self._c[0])
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of "
                               "GradScaler.")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._f is not None:
            self._set_scale(self._init_scale)
            self._c[0:1].fill_(self._init_growth_tracker)

    def _snapshot(self):
        return self._f.clone(), self._c.clone()

    def _restore(self, snap):
        self._f.copy_(snap[0])
        self._c.copy_(snap[1])
        self._pending, self._stepped = None, False
        self._unscaled.clear()
        self._max_norm.clear()

    # ------------------------------------------------------------------------------------------------ the protocol
    def scale(self, outputs):
        if not self._enabled:
            return outputs
        if not torch.is_tensor(outputs):
            return type(outputs)(self.scale(o) for o in outputs)
        self._ensure(outputs.device)
        return outputs * self._f[0]

    @staticmethod
    def _ours(optimizer, what):
        if not isinstance(optimizer, (AdamW, BertAdam)):
            raise TypeError("DeviceGradScaler.%s: centerclip_amd.train.AdamW or BertAdam (the optimizers with launches that can "
                            "be skipped on the device), got %s" % (what, type(optimizer).__name__))

    def unscale_(self, optimizer):
        """Marks the optimizer's gradients as to be read unscaled; launches nothing - step() applies inv_scale together with
        the clip coefficient, so p.grad still holds the SCALED values until then (and the unscaled, clipped ones after)."""
        if not self._enabled:
            return
        self._ours(optimizer, "unscale_")
        if id(optimizer) in self._unscaled:
            raise RuntimeError("unscale_() has already been called on this optimizer since the last update().")
        self._unscaled.add(id(optimizer))

    def clip_grad_norm_(self, optimizer, max_norm):
        """torch.nn.utils.clip_grad_norm_ over the optimizer's parameters, on the UNSCALED gradients (call unscale_ first,
        main.py:324-326): deferred into step(), where it costs no launch of its own."""
        if not self._enabled:
            return
        self._ours(optimizer, "clip_grad_norm_")
        if id(optimizer) not in self._unscaled:
            raise RuntimeError("DeviceGradScaler.clip_grad_norm_: call unscale_(optimizer) first")
        if not float(max_norm) >= 0.0:
            raise ValueError("DeviceGradScaler.clip_grad_norm_: max_norm must be >= 0")
        self._max_norm[id(optimizer)] = float(max_norm)

    def _stats(self, table, count, nblk, max_norm, device):
        """-> (multiplier, found_inf): 1-element views of the device state, written by cc_grad_scaler_stats_f32."""
        self._ensure(device)
        lib = L.lib()
        ws = L.workspace(lib.cc_grad_norm_workspace_bytes(nblk), self._f.device)
        st = _st(self._f)
        _check(lib.cc_grad_norm_partials_f32(L.ptr(table), count, nblk, L.ptr(ws), ws.numel(), st), "cc_grad_norm_partials_f32")
        _check(lib.cc_grad_scaler_stats_f32(L.ptr(ws), nblk, L.ptr(self._f[1:2]), float(max_norm), L.ptr(self._f[2:5]), st),
               "cc_grad_scaler_stats_f32")
        return self._f[3:4], self._f[4:5]

    def grad_norm(self):
        """The norm of the unscaled gradients the last step() measured (0-d device tensor)."""
        return self._f[2]

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        self._ours(optimizer, "step")
        if "closure" in kwargs or args:
            raise RuntimeError("Closure use is not currently supported if GradScaler is enabled.")
        capturing = _capturing()
        if not capturing:
            self.sync()                                           # the previous step's count, before this one's host arithmetic
        max_norm = self._max_norm.pop(id(optimizer), -1.0)
        ran = optimizer._scaled_step(self, max_norm)
        if not ran:                                               # (no gradient anywhere: nothing to skip)
            for p in (p for g in optimizer.param_groups for p in g['params']):
                self._ensure(p.device)
                break
            if self._f is None:
                raise RuntimeError("DeviceGradScaler.step: the optimizer has no parameters")
            self._f[4:5].zero_()
        self._pin.copy_(self._f[4:5], non_blocking=True)          # (captured: a copy node of the graph)
        if not capturing and ran:
            self._mark(optimizer, "eager")
        self._stepped = True
        return None

    def _mark(self, optimizer, mode):
        self._event.record()
        self._pending = (optimizer, mode)

    def sync(self):
        """Settle the last step's count (see the class docstring): waits for that step, no-op when nothing is pending."""
        if self._pending is None:
            return
        optimizer, mode = self._pending
        self._pending = None
        self._event.synchronize()
        skipped = float(self._pin[0]) != 0.0
        if mode == "eager" and skipped:
            optimizer._uncount()
        elif mode == "graph" and not skipped:
            optimizer.advance()

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            if _capturing():
                raise RuntimeError("DeviceGradScaler.update(new_scale=...) inside a capture")
            if self._f is None:
                if torch.is_tensor(new_scale):
                    self._ensure(new_scale.device)
                    self._set_scale(new_scale)
                else:
                    self._init_scale = float(new_scale)
            else:
                self._set_scale(new_scale)
        else:
            if not self._stepped:
                raise RuntimeError("No inf checks were recorded prior to update.")
            _check(L.lib().cc_grad_scaler_update_f32(L.ptr(self._f[0:2]), L.ptr(self._f[4:5]), L.ptr(self._c), self._growth_factor,
                                                     self._backoff_factor, self._growth_interval, _st(self._f)),
                   "cc_grad_scaler_update_f32")
        self._stepped = False
        self._unscaled.clear()
        self._max_norm.clear()


def _device_scaler(scaler):
    """GraphedTrainStep's scaler argument -> (DeviceGradScaler or None, the torch GradScaler it was copied from or None)."""
    if scaler is None:
        return None, None
    if isinstance(scaler, DeviceGradScaler):
        return (scaler if scaler.is_enabled() else None), None
    if isinstance(scaler, torch.amp.GradScaler):
        if not scaler.is_enabled():
            return None, None
        dev = DeviceGradScaler()
        dev.load_state_dict(scaler.state_dict())
        return dev, scaler
    raise TypeError("GraphedTrainStep: scaler must be a DeviceGradScaler or a torch.amp.GradScaler, got %s" % type(scaler).__name__)


# ================================================================================================ train_epoch
def train_epoch(epoch, args, model, train_dataloader, device, optimizer, global_step, scheduler=None, buckets=None,
                log=None, scaler=None):
    """main.py:291-378 for this path: zero_grad -> forward (training branch of CLIP4Clip.forward) -> backward ->
    [gradient average over the ranks, dist.GradientBuckets] -> [clip_grad_norm_] -> optimizer.step -> clamp logit_scale.
    ``model``: a centerclip_amd.clip4clip.CLIP4Clip in training mode.  -> (mean loss, global_step).

    ``scaler`` (main.py:309-330, the reference's ``--fp16`` branch): a ``torch.cuda.amp.GradScaler`` (or anything with its
    scale / unscale_ / step / update).  The forward here always feeds the matrix cores fp16 operands with fp32 accumulation
    and keeps fp32 master weights - what ``autocast`` gives the reference - so the branch adds what the scaler itself does:
    the loss is multiplied by the scale before backward (the HIP backward picks a power-of-two scale per gradient tensor on
    the device, so the factor passes through exactly), gradients are unscaled (and averaged over the ranks) before clipping,
    a step whose gradients hold an inf / NaN is skipped and the scale backed off, as GradScaler.step / update do.
    A ``DeviceGradScaler`` runs the same branch without a host decision (no unscaling pass, no .item() on found_inf); its
    clipping is its own clip_grad_norm_ over the optimizer's parameters, folded into the step's one multiplier."""
    model.train()
    total_loss, nb = 0.0, 0
    for step, batch in enumerate(train_dataloader):
        optimizer.zero_grad()
        if scheduler is not None:
            scheduler(optimizer, global_step=global_step)
        input_ids, input_mask, segment_ids, video, video_mask = tuple(t.to(device=device, non_blocking=True) for t in batch)
        output = model(input_ids, segment_ids, input_mask, video, video_mask)
        loss = output['loss'].mean()
        if args.gradient_accumulation_steps > 1:
            loss = loss / args.gradient_accumulation_steps
        if scaler is not None:
            scaler.scale(loss).backward()
        else:
            loss.backward()
        if (step + 1) % args.gradient_accumulation_steps == 0:
            if buckets is not None:
                buckets.reduce()
            if scaler is not None:
                if getattr(args, "clip_grad_norm", None) is not None:
                    scaler.unscale_(optimizer)           # (clipping sees the true gradients, main.py:324-326)
                    if isinstance(scaler, DeviceGradScaler) and scaler.is_enabled():
                        scaler.clip_grad_norm_(optimizer, args.clip_grad_norm)     # (fused into step(): one multiplier)
                    else:
                        torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_grad_norm)
                scaler.step(optimizer)                   # skipped when a gradient holds an inf / NaN
                scaler.update()
            else:
                if getattr(args, "clip_grad_norm", None) is not None:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_grad_norm)
                optimizer.step()
            global_step += 1
        with torch.no_grad():                                    # (main.py:336-340; tracked, so the cached copies refresh)
            model.clip.logit_scale.clamp_(0.1, 4.6052)
        if log is not None:
            log(epoch, step, float(loss.detach()), float(output['sim_loss'].detach()), global_step)
        total_loss += float(loss.detach())
        nb += 1
    if isinstance(scaler, DeviceGradScaler):
        scaler.sync()                                            # the last step's count
    return total_loss / max(nb, 1), global_step


class GraphedTrainStep:
    """One training step (forward, backward, optimizer, logit_scale clamp - main.py:300-340 for one batch) captured into a
    hipGraph and replayed on static input buffers: no op of the step synchronises with the host, so the replay runs at the GPU
    time of its kernels instead of the host's launch rate (cfg-2 shape: 19 ms against 40-100 ms launched op by op).
    Single process (a captured step cannot contain the RCCL exchange of GradientBuckets); fixed batch shape; an optimizer
    built with capturable=True.  The first call warms up eagerly (2 steps on the given batch) and captures - on a snapshot:
    parameters, moments and step counts are put back before the one replay that counts, so that EVERY call, the first
    included, is exactly one optimizer step (main.py:300-340) and the schedule position equals the caller's step count."""

    def __init__(self, model, optimizer, gradient_accumulation_steps=1, scheduler=None, clip_grad_norm=None, global_step=0,
                 scaler=None):
        """scaler: a DeviceGradScaler - the launchers' precision=amp recipe (main.py:320-328) inside the captured step: scale
        the loss, backward, gradient statistics, clip-and-step or step (skipped on the device when a gradient holds an inf /
        NaN), scale update, logit_scale clamp.  A torch.amp.GradScaler is accepted too: its hyper-parameters and state are
        copied into a DeviceGradScaler (self.scaler), and write_back_scaler() copies the state back.  None or a disabled
        scaler: exactly the graph without one.  A skipped step does not advance the optimizer's state['step'] while
        global_step advances (main.py:344-345); the count of call k is settled at the start of call k + 1 (the flag arrives in
        a pinned word the graph writes; see DeviceGradScaler) - call sync() before optimizer.state_dict().
        scheduler (e.g. lr_scheduler): called as scheduler(optimizer, global_step=k) on the host before every step, k = the
        number of calls made so far + global_step (main.py:302); its lr reaches the captured step through refresh_lr().
        clip_grad_norm: global gradient clipping inside the captured step, before the optimizer (main.py:327-333) -
        AdamW.clip_and_step, or clip_grad_norm_ then step() for BertAdam."""
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs BertAdam(..., capturable=True) or AdamW(..., capturable=True)")
        if gradient_accumulation_steps != 1:
            raise NotImplementedError("GraphedTrainStep: gradient accumulation is not built")
        self.model, self.optimizer = model, optimizer
        self.scheduler, self.clip_grad_norm, self.global_step = scheduler, clip_grad_norm, int(global_step)
        self._moments = ('exp_avg', 'exp_avg_sq') if isinstance(optimizer, AdamW) else ('next_m', 'next_v')
        self.scaler, self._torch_scaler = _device_scaler(scaler)
        self.graph = self.static = self.loss = None

    def sync(self):
        """Settle the last call's step count (with a scaler it is known only once that call has run): waits for it."""
        if self.scaler is not None:
            self.scaler.sync()

    def write_back_scaler(self):
        """Copy the device scaler's state (scale, growth tracker, hyper-parameters) into the torch.amp.GradScaler this step
        was built from, e.g. before a checkpoint saves that object's state_dict (main.py:262-272); -> that GradScaler.
        Without one (a DeviceGradScaler was passed: it IS the state) -> None."""
        if self._torch_scaler is None:
            return None
        self._torch_scaler.load_state_dict(self.scaler.state_dict())
        return self._torch_scaler

    def _schedule(self):
        if self.scheduler is not None:
            self.scheduler(self.optimizer, global_step=self.global_step)

    def _step(self):
        self.optimizer.zero_grad(set_to_none=True)       # (captured: the gradients live in the graph's pool, no fill + accumulate)
        out = self.model(self.static[0], self.static[2], self.static[1], self.static[3], self.static[4])
        loss = out['loss'].mean()
        if self.scaler is not None:
            sc = self.scaler
            sc.scale(loss).backward()
            if self.clip_grad_norm is not None:
                sc.unscale_(self.optimizer)
                sc.clip_grad_norm_(self.optimizer, self.clip_grad_norm)
            sc.step(self.optimizer)
            sc.update()
            with torch.no_grad():
                self.model.clip.logit_scale.clamp_(0.1, 4.6052)
            return loss.detach()
        loss.backward()
        if self.clip_grad_norm is None:
            self.optimizer.step()
        elif isinstance(self.optimizer, AdamW):
            self.optimizer.clip_and_step(self.clip_grad_norm)
        else:
            clip_grad_norm_([p for g in self.optimizer.param_groups for p in g['params']], self.clip_grad_norm)
            self.optimizer.step()
        with torch.no_grad():
            self.model.clip.logit_scale.clamp_(0.1, 4.6052)
        return loss.detach()

    def _tensors(self):
        # (a frozen parameter cannot change in a step: it is neither copied nor written back - the packed copies of a frozen
        #  prefix, whose addresses the captured graph holds, stay valid)
        seen, out = set(), []
        for p in list(self.model.parameters()) + [p for g in self.optimizer.param_groups for p in g['params']]:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                out.append(p)
        return out

    def _snapshot(self):
        """Copies of everything a step changes: every parameter, and per parameter the optimizer's (step, first moment, second
        moment) - next_m / next_v for BertAdam, exp_avg / exp_avg_sq for AdamW."""
        snap = []
        km, kv = self._moments
        for p in self._tensors():
            st = self.optimizer.state.get(p, {})
            snap.append((p, p.detach().clone(), st.get('step'), st[km].clone() if km in st else None,
                         st[kv].clone() if kv in st else None))
        return snap

    @torch.no_grad()
    def _restore(self, snap):
        """In place (the captured graph holds the addresses of the parameters and of the moments the warm-up created);
        Tensor.copy_ bumps the version counter, so cached fp16 / folded copies of the weights refresh."""
        km, kv = self._moments
        for p, value, step, m, v in snap:
            p.copy_(value)
            st = self.optimizer.state.get(p)
            if not st:
                continue
            st['step'] = 0 if step is None else step
            st[km].zero_() if m is None else st[km].copy_(m)
            st[kv].zero_() if v is None else st[kv].copy_(v)

    def __call__(self, batch):
        """batch = (input_ids, input_mask, segment_ids, video, video_mask) as the dataloaders yield it -> the step's loss (a
        device tensor that the next call overwrites)."""
        dev = next(self.model.parameters()).device
        if self.graph is None:
            self.model.train()
            self.static = [t.to(dev).clone() for t in batch]
            snap = self._snapshot()
            if self.scaler is not None:
                self.scaler.sync()                                # (an eager step the caller made with it before)
                self.scaler._ensure(dev)
                sc_snap = self.scaler._snapshot()
            for _ in range(2):                                    # allocator / staging-buffer warm-up (the optimizer's records)
                self._schedule()
                self._step()
            if self.scaler is not None:
                self.scaler.sync()                                # (no host wait may fall into the capture)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):                    # (the capture pass does not execute)
                self.loss = self._step()
            self._restore(snap)                                   # the two warm-up steps never happened
            if self.scaler is not None:
                self.scaler._restore(sc_snap)                     # ... nor did their scale updates and counters
            return self._replay()
        self.sync()                                               # the previous call's count, BEFORE this call's work is enqueued
        for dst, src in zip(self.static, batch):
            dst.copy_(src, non_blocking=True)
        return self._replay()

    def _replay(self):
        self._schedule()
        self.optimizer.refresh_lr()
        self.graph.replay()
        if self.scaler is not None:
            self.scaler._mark(self.optimizer, "graph")            # counted (or not) by the next sync()
        else:
            self.optimizer.advance()
        self.global_step += 1
        return self.loss
