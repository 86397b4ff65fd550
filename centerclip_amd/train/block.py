"""One ResidualAttentionBlock (modules/clip.py:196-253) for training: the forward that keeps what the backward needs, the
backward, and both inside torch.autograd (the reference gets the backward from autograd, main.py:321).

    x [L, N, W] (LND, as the reference's blocks see it)
    y = x + out_proj(MHA(in_proj(ln_1(x))))          z = y + c_proj(act(c_fc(ln_2(y))))      act: QuickGELU | exact GELU

* forward: the op-level HIP entry points of the inference path (LayerNorm -> fp16, cc_linear_f16, cc_attention_f16,
  residual epilogue), keeping x, ln_1(x), qkv, the attention output, y, ln_2(y), the c_fc output before and after QuickGELU.
* backward: the four Linear layers' dgrad (dX = dY W) and wgrad (dW = dY^T X) run on the fp16 MFMA GEMM kernels; gradients
  enter the matrix cores as fp16 with a per-tensor power-of-two scale chosen on the device (cc_cast_transpose_f16, one read
  per matrix, no host synchronisation) and divided out in the consuming GEMM's epilogue (cc_linear_unscaled_f16,
  cc_wgrad_tn_f16); LayerNorm, QuickGELU, attention and bias gradients are the fp32 kernels of csrc/backward.hip.
* ``ResidualAttentionBlockFunction`` / ``block_apply`` wire both into torch.autograd (d/dx and the 12 parameter gradients);
  ``LinearFunction`` and ``LayerNormFunction`` do the same for the towers' patch embedding, projections and LayerNorms
  (modules/clip.py:183-189).  Checked against torch.autograd on the reference model (tests/test_r4_gpu.py) and against
  float64 at the shipped widths (tests/test_backward_gpu.py).
"""
import torch

from .. import _lib as L
from .. import ops
from ..torch_ops import _st


def _check(rc, what):
    L.check(rc, what)



MAX_TRAIN_TOKENS = 320      # cc_attention_backward_f16: five 64-key tiles on the query side


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


def block_forward_train(block, x_lnd, mid_shift=None, key_mask=None, cluster_done=False):
    """-> (z [L, N, W] fp32, saved dict).  ``block``: a centerclip_amd.clip.ResidualAttentionBlock; one that carries a cluster
    module is refused unless ``cluster_done`` says the caller has already run that module on ``x_lnd`` (clip.py:236-242).
    ``mid_shift`` (segment, fold_div): token_shift's second shift between the attention residual and ln_2 (clip.py:246-248),
    y' = S(y); None (default): the plain block.  ``key_mask`` [N, L] int64 (any strides): the seqTransf head's additive
    (1 - mask[key]) * -1e6 on every key of sequence n (module_cross.py:102-104, cc_key_masked_attention_f16)."""
    if block.tokencluster_inter is not None and not cluster_done:
        raise NotImplementedError("block backward: blocks with a token-cluster module are not covered by this slice")
    L.require_device(x_lnd)
    Lt, N, W = x_lnd.shape
    if Lt > MAX_TRAIN_TOKENS:
        raise NotImplementedError("block training: %d tokens per sequence - the attention backward is built up to %d "
                                  "(ViT-L/14 at 224 px has 257; 336 px, 577 tokens, is evaluation only)" % (Lt, MAX_TRAIN_TOKENS))
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
    act = "cc_quick_gelu_f16" if block.quick_gelu else "cc_gelu_f16"              # the block's activation (a construction argument)
    _check(getattr(L.lib(), act)(L.ptr(u_pre), L.ptr(u), u.numel(), _st(u)), act)
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
    # u = act(u_pre): QuickGELU, or the exact GELU of a block built with quick_gelu=False
    # (the three gradients this function produces AND multiplies publish their largest magnitude from the producing kernel:
    #  the fp16 cast of each then needs no pass of its own to choose the scale)
    am = torch.zeros(3, 2, device=dz.device, dtype=torch.float32)
    du_pre = torch.empty_like(du)
    act = "cc_quick_gelu_backward_f16" if block.quick_gelu else "cc_gelu_backward_f16"
    _check(getattr(L.lib(), act)(L.ptr(saved["u_pre"]), L.ptr(du), L.ptr(du_pre), du.numel(), L.ptr(am[0]), _st(du)), act)
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
    parameter tensors (passed as arguments so that autograd sees them).  ``options``: block_forward_train's keywords."""

    @staticmethod
    def forward(ctx, block, options, x, *params):
        z, saved = block_forward_train(block, x, **options)
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
        need = {k: bool(ctx.needs_input_grad[3 + i]) for i, k in enumerate(_PARAM_ORDER)}
        dx, g = block_backward(ctx.block, ctx.saved, dz, need=need, need_dx=bool(ctx.needs_input_grad[2]))
        return (None, None, dx) + tuple((g[k].view_as(named[k]).to(named[k].dtype) if (need[k] and g[k] is not None) else None)
                                  for k in _PARAM_ORDER)


def block_apply(block, x_lnd, mid_shift=None, key_mask=None, cluster_done=False):
    """Differentiable block forward: ``z = block_apply(block, x); loss(z).backward()`` fills x.grad and block.*.grad.
    The keywords are block_forward_train's."""
    named = dict(block.named_parameters())
    options = dict(mid_shift=mid_shift, key_mask=key_mask, cluster_done=cluster_done)
    return ResidualAttentionBlockFunction.apply(block, options, x_lnd, *[named[k] for k in _PARAM_ORDER])


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
