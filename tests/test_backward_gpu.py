"""The training backward (N4) at the widths the product trains, against float64.

* the block: train.block_forward_train / block_backward at W = 768 (12 heads) and W = 512 (8 heads, causal) on up to 9,600
  rows against oracle.clip_oracle.block_backward64 (pinned to the reference's autograd in tests/test_oracle_backward.py);
* power-of-two homogeneity: every scale of the HIP backward is a power of two, so dz * 2^k must give 2^k times the
  gradients bit for bit - and a gradient whose largest entry is 1e-36 must come out finite and accurate;
* the kernels one by one (LayerNorm backward, QuickGELU, column sums, the scaled fp16 casts, the bias gradient of the sliced
  weight gradient, BertAdam's large-tensor and multi-tensor paths) against float64, where a sum is bounded by
  n * 2^-24 * sum|terms| with n the kernel's longest serial chain: any correct order passes, a dropped or doubled term fails.
"""
import math

import numpy as np
import pytest
import torch

from oracle.recipes import WIDE_BLOCK_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                                                  # unit roundoff of fp32
CC_ERR_INVALID = -1


def _rel(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- the block

def _wide_block(tag):
    from centerclip_amd.clip import ResidualAttentionBlock
    from oracle.recipes import block_grad_inputs
    cfg = WIDE_BLOCK_CASES[tag]
    x, dz, sd = block_grad_inputs(cfg)
    blk = ResidualAttentionBlock(cfg["W"], cfg["heads"], attn_mask=(lambda n: None) if cfg["causal"] else None, block_id=1, args=None)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, blk.to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(dz).to(DEV)


def _errors(z, dx, grads, ref):
    zr, dxr, gr = ref
    errs = {"z": _rel(z, zr), "dx": _rel(dx, dxr)}
    for k, v in grads.items():
        errs[k] = _rel(v.reshape(gr[k].shape), gr[k])
    return errs


@pytest.mark.parametrize("tag", sorted(WIDE_BLOCK_CASES))
def test_block_backward_at_shipped_widths_against_float64(tag):
    """z, dx and the 12 parameter gradients within 2e-3 of each tensor's largest entry of the float64 block on the same
    (fp16-representable) weights; identical bits on a second run; the same gradients in .grad through block_apply."""
    from centerclip_amd import train
    from oracle.clip_oracle import block_backward64
    cfg, blk, x, dz = _wide_block(tag)
    z, saved = train.block_forward_train(blk, x)
    dx, grads = train.block_backward(blk, saved, dz)
    ref = block_backward64(x, dz, {k: v for k, v in blk.state_dict().items()}, cfg["heads"], cfg["causal"])
    errs = _errors(z, dx, grads, ref)
    print(f"[{tag}] relative errors:", {k: "%.1e" % e for k, e in errs.items()})
    assert len(grads) == 12 and max(errs.values()) < 2e-3, errs
    dx2, grads2 = train.block_backward(blk, saved, dz)
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    xa = x.clone().requires_grad_(True)
    (train.block_apply(blk, xa) * dz).sum().backward()
    assert torch.equal(xa.grad, dx)
    for k, p_ in blk.named_parameters():
        assert p_.grad is not None and torch.equal(p_.grad.reshape(-1), grads[k].reshape(-1)), k


@pytest.mark.parametrize("tag", ["wb_vit32", "wb_vit16", "wb_text"])
def test_block_backward_is_power_of_two_homogeneous(tag):
    """block_backward(saved, dz 2^k) == 2^k block_backward(saved, dz) bit for bit for k in {-40, -16, 16, 40} (k = 16: a
    GradScaler factor passes through exactly, as train_epoch relies on): no absolute epsilon or threshold in any backward
    kernel.  Then dz scaled to a largest entry of ~1e-36 (below 16384 / FLT_MAX, where an unclamped cast scale overflows):
    every output finite and within the 2e-3 bound of the scaled float64 reference."""
    from centerclip_amd import train
    from oracle.clip_oracle import block_backward64
    cfg, blk, x, dz = _wide_block(tag)
    _, saved = train.block_forward_train(blk, x)
    dx, grads = train.block_backward(blk, saved, dz)
    for k in (-40, -16, 16, 40):
        f = 2.0 ** k
        dxk, gk = train.block_backward(blk, saved, dz * f)
        assert torch.equal(dxk, dx * f), k
        for name in grads:
            assert torch.equal(gk[name], grads[name] * f), (k, name)
    f = 2.0 ** round(math.log2(1e-36 / float(dz.abs().max())))
    dzt = dz * f                                                   # (its smallest entries are fp32 denormals)
    assert 5e-37 < float(dzt.abs().max()) < 2e-36
    dxt, gt = train.block_backward(blk, saved, dzt)
    outs = {"dx": dxt, **gt}
    assert all(bool(torch.isfinite(v).all()) for v in outs.values()), [k for k, v in outs.items() if not torch.isfinite(v).all()]
    _, dx64, g64 = block_backward64(x, dzt.double() / f, {k: v for k, v in blk.state_dict().items()}, cfg["heads"], cfg["causal"])
    errs = {"dx": _rel(dxt.double() / f, dx64)}
    for name, v in gt.items():
        errs[name] = _rel(v.double().reshape(g64[name].shape) / f, g64[name])
    print(f"[{tag}] tiny dz, relative errors:", {k: "%.1e" % e for k, e in errs.items()})
    assert max(errs.values()) < 2e-3, errs


# ---------------------------------------------------------------------------------------------------- LayerNorm backward

def _ln_call(x, x_stride, gamma, dy, dres, rows, W, amax=None, eps=1e-5):
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    dx = torch.empty(rows, W, device=DEV)
    dg, db = torch.empty(W, device=DEV), torch.empty(W, device=DEV)
    lib = L.lib()
    nb = lib.cc_layernorm_backward_workspace_bytes(rows, W)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=DEV)
    rc = lib.cc_layernorm_backward_f32(L.ptr(x), x_stride, L.ptr(gamma), L.ptr(dy), L.ptr(dres), L.ptr(dx), L.ptr(dg), L.ptr(db),
                                       rows, W, eps, L.ptr(amax), L.ptr(ws), nb, _st(dy))
    return rc, dx, dg, db


@pytest.mark.parametrize("W", [4, 60, 128, 252, 256, 260, 512, 768, 1020, 1024])
def test_layernorm_backward_against_float64(W):
    """cc_layernorm_backward_f32 against float64 from the same fp32 x, dy, gamma: with and without dres, x with a row
    stride > W, rows with mean 300 and std 0.01; dx, dgamma, dbeta within the summation bound of every term (the row
    statistics are wave trees of depth <= 16; dgamma / dbeta add 8 rows per wave, 4 waves, ceil(blocks / 8) partials and 8
    segments); dx_amax == max|dx|."""
    eps = 1e-5
    g = _gen(W)
    for i, rows in enumerate((1, 31, 32, 33, 97, 9600)):
        big_mean = i % 2 == 1
        stride = W + 8 if i % 3 == 2 else W
        xb = torch.randn(rows, stride, device=DEV, generator=g)
        xb = xb * 0.01 + 300.0 if big_mean else xb * 1.5 + 0.2
        x = xb[:, :W]
        gamma = 1.0 + 0.2 * torch.randn(W, device=DEV, generator=g)
        dy = torch.randn(rows, W, device=DEV, generator=g) * 1e-2
        dres = torch.randn(rows, W, device=DEV, generator=g) * 1e-2 if i % 2 == 0 else None
        am = torch.zeros(1, device=DEV)
        rc, dx, dg, db = _ln_call(xb, stride, gamma, dy, dres, rows, W, amax=am, eps=eps)
        assert rc == 0
        # float64 reference and bounds
        xd, gd, dyd = x.double(), gamma.double(), dy.double()
        mu = xd.mean(1, keepdim=True)
        var = ((xd - mu) ** 2).mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        xh = (xd - mu) * rstd
        gg = dyd * gd
        c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
        want = rstd * (gg - c1 - xh * c2) + (dres.double() if dres is not None else 0.0)
        gam = 16 * U
        e_mu = gam * xd.abs().mean(1, keepdim=True)                       # the row mean
        e_xh = rstd * e_mu + xh.abs() * (2 * gam + (rstd * e_mu) ** 2 + 4 * U)   # xhat: mean + rstd (variance of the shifted rows)
        e_rstd = 2 * gam + (rstd * e_mu) ** 2 + 4 * U
        e_c1 = gam * gg.abs().mean(1, keepdim=True)
        e_c2 = gam * (gg * xh).abs().mean(1, keepdim=True) + (gg.abs() * e_xh).mean(1, keepdim=True)
        core = rstd * (gg - c1 - xh * c2)
        bound = 2 * (rstd * (4 * U * (gg.abs() + c1.abs() + (xh * c2).abs()) + e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh)
                     + core.abs() * e_rstd + 2 * U * want.abs())
        err = (dx.double() - want).abs()
        assert bool((err <= bound).all()), (rows, float((err / bound).max()))
        blocks = -(-rows // 32)
        n = 8 + 4 + -(-blocks // 8) + 8
        want_dg, want_db = (dyd * xh).sum(0), dyd.sum(0)
        assert bool(((dg.double() - want_dg).abs() <= n * U * (dyd * xh).abs().sum(0) * 2 + (dyd.abs() * e_xh).sum(0) * 2).all()), rows
        assert bool(((db.double() - want_db).abs() <= n * U * dyd.abs().sum(0)).all()), rows
        assert float(am[0]) == float(dx.abs().max())


def test_layernorm_backward_argument_checks():
    """W outside 4..1024 or not a multiple of 4, and x_stride < W or not a multiple of 4, are CC_ERR_INVALID."""
    rows = 8
    buf = torch.zeros(rows, 1040, device=DEV)
    gamma = torch.ones(1040, device=DEV)
    dy = torch.zeros(rows, 1040, device=DEV)
    for W in (6, 1028):
        assert _ln_call(buf, 1040, gamma, dy, None, rows, W)[0] == CC_ERR_INVALID, W
    for stride in (60, 66, 130):
        assert _ln_call(buf, stride, gamma, dy, None, rows, 64)[0] == CC_ERR_INVALID, stride
    assert _ln_call(buf, 68, gamma, dy, None, rows, 64)[0] == 0


# ---------------------------------------------------------------------------------------------------- QuickGELU

def _gelu_inputs(n, seed):
    g = _gen(seed)
    x = torch.randn(n, device=DEV, generator=g) * 3.0
    k = n // 8
    if k:
        x[:k] = -torch.rand(k, device=DEV, generator=g) * 70.0                         # the long negative tail (sigmoid -> 0)
        x[k:2 * k] = (torch.rand(k, device=DEV, generator=g) * 2 - 1) * 65504.0        # the whole fp16 range
    x16 = x.half()
    x16[:4] = torch.tensor([0.0, -0.0, 65504.0, -65504.0], device=DEV).half()
    if n >= 8:
        x16[-4:] = torch.tensor([6e-8, -6e-8, -17.0, 17.0], device=DEV).half()          # fp16 subnormals, both sides
    return x16


def _f16_ulp(y16):
    a = y16.float().abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10).double()


@pytest.mark.parametrize("n", [4, 1020, 1028, 8192 * 1024 + 4, 9600 * 3072])
def test_quick_gelu_forward_and_backward_against_float64(n):
    """cc_quick_gelu_f16 within one fp16 ulp of the float64 value rounded to fp16; cc_quick_gelu_backward_f16 within
    2e-6 |du| (1 + |x|) elementwise (a wrong constant - 1.70 for 1.702 - is off by ~1e-4 |du| near |x| = 1).  Sizes beyond
    8192 * 1024 elements run the grid-stride loops (c_fc at cfg 2: 29.5 M); ±0, ±65504 and a long negative tail included."""
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    x16 = _gelu_inputs(n, n % 9973)
    out = torch.empty_like(x16)
    L.check(L.lib().cc_quick_gelu_f16(L.ptr(x16), L.ptr(out), n, _st(out)), "cc_quick_gelu_f16")
    xd = x16.double()
    s = torch.sigmoid(1.702 * xd)
    want = (xd * s).half()
    err = (out.double() - want.double()).abs()
    assert bool((err <= _f16_ulp(want)).all()) and torch.equal(torch.signbit(out[:2]), torch.signbit(want[:2]))
    du = torch.randn(n, device=DEV, generator=_gen(n % 7919 + 1))
    dout = torch.empty_like(du)
    am = torch.zeros(1, device=DEV)
    L.check(L.lib().cc_quick_gelu_backward_f16(L.ptr(x16), L.ptr(du), L.ptr(dout), n, L.ptr(am), _st(du)), "cc_quick_gelu_backward_f16")
    want_d = du.double() * (s + 1.702 * xd * s * (1 - s))
    err = (dout.double() - want_d).abs()
    assert bool((err <= 2e-6 * du.double().abs() * (1 + xd.abs())).all()), float((err / (du.double().abs() * (1 + xd.abs()))).max())
    assert float(am[0]) == float(dout.abs().max())


def test_quick_gelu_refuses_ragged_sizes():
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    x16 = torch.zeros(8, device=DEV, dtype=torch.float16)
    du = torch.zeros(8, device=DEV)
    assert L.lib().cc_quick_gelu_f16(L.ptr(x16), L.ptr(x16.clone()), 6, _st(du)) == CC_ERR_INVALID
    assert L.lib().cc_quick_gelu_backward_f16(L.ptr(x16), L.ptr(du), L.ptr(du.clone()), 6, None, _st(du)) == CC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- column sums

@pytest.mark.parametrize("rows", [1, 127, 128, 129, 1025, 9600, 38400])
def test_column_sums_against_float64(rows):
    """cc_column_sums_f32 (128-row chunks, then 8 segments of chunks, uneven where chunks > 8) within
    (128 + ceil(chunks / 8) + 8) 2^-24 sum|x| of the float64 column sums; bit-stable from run to run."""
    from centerclip_amd import train
    g = _gen(rows)
    chunks = -(-rows // 128)
    n = 128 + -(-chunks // 8) + 8
    for cols in (1, 3, 31, 33, 257, 768, 3072):
        x = torch.randn(rows, cols, device=DEV, generator=g) * 1e-3 + 1e-4
        got = train._column_sums(x)
        xd = x.double()
        assert bool(((got.double() - xd.sum(0)).abs() <= n * U * xd.abs().sum(0)).all()), (rows, cols)
        assert torch.equal(train._column_sums(x), got)


# ---------------------------------------------------------------------------------------------------- scaled fp16 casts

def _check_cast(x, out16, scale, amax):
    s = float(scale)
    assert s > 0 and math.isfinite(s) and math.frexp(s)[0] == 0.5, s                  # a power of two
    assert 2.0 ** -126 <= 1.0 / s and s <= 2.0 ** 126
    if amax == 0.0:
        assert s == 1.0
    elif amax >= 2.0 ** -112:
        assert 8192.0 <= s * amax <= 16384.0 * (1 + 2.0 ** -16), (amax, s)
    else:
        assert s == 2.0 ** 126, (amax, s)                                              # the clamp
    assert torch.equal(out16, (x.double() * s).half()), amax
    assert bool(torch.isfinite(out16).all())


@pytest.mark.parametrize("amax", [0.0, 1e-20, 1e-34, 6e-35, 1e-36, 1e-40, 1e38, 3e-4])
def test_cast_scaled_and_transpose_edges(amax):
    """cc_cast_scaled_f16 / cc_cast_transpose_f16 / cc_unscale_f32: the fp16 copy == (x * scale) rounded to fp16 bit for bit,
    the scale a power of two with scale * amax in [8192, 16384] (16384 at powers of two) where that is <= 2^126 and 2^126
    below, a finite inverse; ragged sizes (the tail loop) and a source 4 bytes into a buffer; the column sums from the same
    read against float64, also with the amax given (scaled = 2); unscale divides exactly."""
    from centerclip_amd import _lib as L, train
    from centerclip_amd.torch_ops import _st
    g = _gen(17)
    for n in (1, 3, 5, 1021, 4096, 9600 * 3 + 1):
        u = torch.rand(n, device=DEV, generator=g) * 2 - 1
        u[n // 2] = -1.0
        base = torch.empty(n + 1, device=DEV)
        base[1:] = (u.double() * amax).float()
        x = base[1:]                                                                   # 4 bytes past a 16-byte boundary
        a = float(x.abs().max())
        for src in (x, x.clone()):
            out16, scale = train._cast_scaled(src)
            torch.cuda.synchronize()
            _check_cast(src, out16, scale, a)
    for M, C in ((50, 64), (9600, 768), (33, 4)):
        u = torch.rand(M, C, device=DEV, generator=g) * 2 - 1
        u[M // 3, C // 2] = 1.0
        x = (u.double() * amax).float()
        a = float(x.abs().max())
        out, out_t, scale, cs = train._cast_transpose(x, scaled=True, col_sums=True)
        _check_cast(x, out, scale, a)
        assert torch.equal(out_t[:, :M], out.t()) and not out_t[:, M:].any()
        n_cs = 4 + 16 + -(-M // 64) + 8                  # 4 rows per thread, 16 row groups per tile, the tiles, slack
        if amax < 1e30:                                  # (sums of 1e38 entries overflow fp32)
            assert bool(((cs.double() - x.double().sum(0)).abs() <= n_cs * U * x.double().abs().sum(0)).all())
        am = torch.tensor([a, 0.0], device=DEV)
        out2, out2_t, scale2, cs2 = train._cast_transpose(x, scaled=True, col_sums=True, amax=am)
        assert float(scale2) == float(scale) and torch.equal(out2, out) and torch.equal(out2_t, out_t)
        assert torch.equal(cs2, cs) or amax >= 1e30
        y = torch.randn(M, C, device=DEV, generator=g)
        want = (y.double() / float(scale)).float()
        got = train._unscale(y.clone(), scale)
        assert torch.equal(got, want)


def test_cast_scale_over_all_exponents():
    """The scale for amax = m 2^e over every float exponent (denormals included), m in {1, 1 + 2^-23, 1.5, 2 - 2^-23} and
    the neighbours of 2^-112: 2^(13 - e) (2^(14 - e) at m = 1; either at m = 1 + 2^-23, where log2f may round up) - the
    unclamped rule's value wherever that is <= 2^126 - and 2^126 for every amax below 2^-112 (the unclamped rule: 2^127 or
    inf there)."""
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    vals = []
    for e in range(-149, 128):
        for m in (1.0, 1.0 + 2.0 ** -23, 1.5, 2.0 - 2.0 ** -23):
            a = np.float32(m * 2.0 ** e) if e > -126 else np.float32(2.0 ** e)
            if np.isfinite(a) and a > 0:
                vals.append(float(a))
    t112 = np.float32(2.0 ** -112)
    vals += [float(np.nextafter(t112, np.float32(0))), float(t112), float(np.nextafter(t112, np.float32(1)))]
    vals = sorted(set(vals))
    xs = torch.zeros(len(vals), 4, device=DEV)
    xs[:, 1] = -torch.tensor(vals, device=DEV)                                        # amax sits in a negative entry
    out16 = torch.empty(len(vals), 4, device=DEV, dtype=torch.float16)
    scratch = torch.zeros(len(vals), 2, device=DEV)
    lib = L.lib()
    for i in range(len(vals)):
        L.check(lib.cc_cast_scaled_f16(L.ptr(xs[i]), L.ptr(out16[i]), 4, L.ptr(scratch[i, 0:1]), L.ptr(scratch[i, 1:2]), _st(xs)),
                "cc_cast_scaled_f16")
    torch.cuda.synchronize()
    scales = scratch[:, 1].double().cpu().numpy()
    amaxes = scratch[:, 0].double().cpu().numpy()
    for a, s, am in zip(vals, scales, amaxes):
        assert am == a
        if a < 2.0 ** -112:
            assert s == 2.0 ** 126, (a, s)
            continue
        m, ex = math.frexp(a)                                                          # a = m 2^ex, m in [0.5, 1)
        e = ex - 1
        assert 8192.0 <= s * a <= 16384.0 * (1 + 2.0 ** -16), (a, s)
        if m == 0.5:
            assert s == 2.0 ** (14 - e), (a, s)
        elif m * 2 == 1.0 + 2.0 ** -23:
            assert s in (2.0 ** (13 - e), 2.0 ** (14 - e)), (a, s)
        else:
            assert s == 2.0 ** (13 - e), (a, s)
    assert bool(torch.isfinite(out16).all())


# ---------------------------------------------------------------------------------------------------- bias gradient, S > 1

@pytest.mark.parametrize("N1,N2", [(768, 768), (3072, 768), (768, 3072), (2304, 768)])
def test_wgrad_bias_gradient_at_9600_rows(N1, N2):
    """cc_wgrad_tn_f16 at M = 9,600 (the row range in slices, S > 1) with the bias gradient from cc_cast_transpose_f16's
    per-tile partials: the bias gradient within (4 + 16 + ceil(tiles / 8) + 8) 2^-24 sum|dy| of float64 column sums, dW
    within M 2^-24 sum|terms| of float64 on the fp16 operands."""
    from centerclip_amd import _lib as L, train
    M = 9600
    if (N1, N2) == (768, 768):
        assert L.lib().cc_wgrad_tn_workspace_bytes(M, N1, N2) > 256                      # (S > 1: slice partials in ws)
    g = _gen(N1 + N2)
    dy = torch.randn(M, N1, device=DEV, generator=g) * 1e-3
    dy[::7] *= 30.0
    x16 = torch.randn(M, N2, device=DEV, generator=g).half()
    dy16, _, scale, part = train._cast_transpose(dy, scaled=True, col_sums=True, want_t=False, col_partials=True)
    dw, db = train._wgrad_tn(dy16, x16, scale, col_partial=part)
    dyd = dy.double()
    n = 4 + 16 + M // 64 + 8
    assert bool(((db.double() - dyd.sum(0)).abs() <= n * U * dyd.abs().sum(0)).all())
    a, b = dy16.double() / float(scale), x16.double()
    want = a.t() @ b
    assert bool(((dw.double() - want).abs() <= M * U * (a.abs().t() @ b.abs())).all())
    assert _rel(dw, dyd.t() @ b) < 2e-3
    dw2, db2 = train._wgrad_tn(dy16, x16, scale, col_partial=part)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


# ---------------------------------------------------------------------------------------------------- BertAdam

def _adam_groups(params, clip):
    from centerclip_amd.train import BertAdam
    return lambda capturable=False: BertAdam([{'params': params[0::2], 'weight_decay': 0.2}, {'params': params[1::2], 'weight_decay': 0.0}],
                                             lr=1e-2, b1=0.9, b2=0.98, e=1e-6, max_grad_norm=clip, capturable=capturable)


@pytest.mark.parametrize("n", [8192, 8193, 512 * 1024 + 3, 2 ** 22 + 1])
def test_bertadam_large_tensors_against_float64(n):
    """cc_bertadam_multi_f32 on tensors above and at the one-workgroup size, clipping engaged and not, weight decay 0.2 and 0,
    two steps, gradients as views into one flat buffer at offsets that are not multiples of 4 floats (the norm pass's
    scalar branch): parameters and moments against the float64 restatement at rtol 2e-6, atol 2e-7."""
    from oracle.clip_oracle import bertadam_step64
    g = _gen(n)
    for norm in (0.3, 40.0):                                                           # max_grad_norm 1: clipping off / on
        ps = [torch.nn.Parameter(torch.randn(n, device=DEV, generator=g)) for _ in range(2)]
        ref = [[p.detach().double().clone(), torch.zeros(n, device=DEV, dtype=torch.float64),
                torch.zeros(n, device=DEV, dtype=torch.float64)] for p in ps]
        opt = _adam_groups(ps, 1.0)()
        flat = torch.empty(2 * n + 16, device=DEV)
        offs = (1, (n + 4) // 4 * 4 + 2)                                                # 4 and 8 bytes past 16-byte boundaries
        for it in range(2):
            for j, p in enumerate(ps):
                gr = torch.randn(n, device=DEV, generator=g)
                gr = gr * (norm / float(gr.double().norm()))
                view = flat[offs[j]: offs[j] + n]
                view.copy_(gr)
                p.grad = view
                bertadam_step64(ref[j][0], gr.double(), ref[j][1], ref[j][2], 1e-2, 0.9, 0.98, 1e-6, 0.2 if j == 0 else 0.0, 1.0)
            opt.step()
            for j, p in enumerate(ps):
                assert p.grad.data_ptr() % 16 != 0
                np.testing.assert_allclose(p.detach().cpu().numpy(), ref[j][0].cpu().numpy(), rtol=2e-6, atol=2e-7)
                st = opt.state[p]
                np.testing.assert_allclose(st['next_m'].cpu().numpy(), ref[j][1].cpu().numpy(), rtol=2e-6, atol=1e-8)
                np.testing.assert_allclose(st['next_v'].cpu().numpy(), ref[j][2].cpu().numpy(), rtol=2e-6, atol=1e-10)


@pytest.mark.parametrize("sizes", ["large", "small", "mixed"])
def test_bertadam_multi_tensor_launches_equal_per_tensor_steps(sizes):
    """One table of N records (cc_bertadam_multi_f32: 37 tensors of mixed sizes > 8192, each found by bisection; 100 tensors of
    1..8192 elements, one workgroup each; both kinds in one table, with the one-workgroup records first, last and twice in a
    row between two large ones) == N tables of one record (one BertAdam per tensor), bit for bit - p, next_v and the
    written-back gradient - over three steps with clipping engaged on some tensors.  For capturable False and True (the
    learning rate in the record / read from the group's device float), which also equal each other."""
    from centerclip_amd.train import BertAdam
    rng = np.random.default_rng(37 if sizes == "large" else 100)
    if sizes == "large":
        ns = [int(v) for v in rng.integers(8193, 400_000, size=37)]
        ns[:3] = [8193, 2 ** 20 + 5, 9600 + 1]
    elif sizes == "small":
        ns = [int(v) for v in rng.integers(1, 8193, size=100)]
        ns[:3] = [1, 8192, 4]
    else:
        ns = [4, 8192, 8193, 1, 8192, 9601, 2 ** 20 + 5, 8193, 3]
    g = _gen(len(ns))
    init = [torch.randn(n, device=DEV, generator=g) for n in ns]
    grads = [[torch.randn(n, device=DEV, generator=g) * (0.5 if j % 3 else 5.0) / math.sqrt(n) for j, n in enumerate(ns)]
             for _ in range(3)]
    tables = {}
    for capturable in (False, True):
        pa = [torch.nn.Parameter(t.clone()) for t in init]
        pb = [torch.nn.Parameter(t.clone()) for t in init]
        oa = _adam_groups(pa, 1.0)(capturable)
        ob = [BertAdam([{'params': [p], 'weight_decay': 0.0 if j % 2 else 0.2}], lr=1e-2, b1=0.9, b2=0.98, e=1e-6,
                       max_grad_norm=1.0, capturable=capturable) for j, p in enumerate(pb)]
        for it in range(3):
            for j in range(len(ns)):
                pa[j].grad, pb[j].grad = grads[it][j].clone(), grads[it][j].clone()
            oa.step()
            for o in ob:
                o.step()
            for j in range(len(ns)):
                assert torch.equal(pa[j], pb[j]), (capturable, it, j, ns[j])
                assert torch.equal(oa.state[pa[j]]['next_v'], ob[j].state[pb[j]]['next_v']), (capturable, it, j, ns[j])
                assert torch.equal(pa[j].grad, pb[j].grad), (capturable, it, j, ns[j])
        tables[capturable] = (pa, [oa.state[p]['next_v'] for p in pa], [p.grad for p in pa])
    for x, y in zip(tables[False], tables[True]):
        for j in range(len(ns)):
            assert torch.equal(x[j], y[j]), (j, ns[j])


def test_bertadam_captured_step_keeps_its_tables_through_eager_uploads():
    """A captured capturable BertAdam step reads record tables of its own: an eager step in between - on fewer parameters,
    then on all of them with gradients at other addresses, so that both tables (small: 1 and 8192 elements, large: 8193 and
    20000) are uploaded afresh - changes nothing a replay reads.  After every step the parameters, next_m, next_v and the
    host-side state['step'] equal, bit for bit, those of a non-capturable BertAdam taking one step per call."""
    ns = [1, 8192, 8193, 20000]
    g = _gen(4)
    init = [torch.randn(n, device=DEV, generator=g) for n in ns]
    pa = [torch.nn.Parameter(t.clone()) for t in init]
    pb = [torch.nn.Parameter(t.clone()) for t in init]
    oa, ob = _adam_groups(pa, 1.0)(False), _adam_groups(pb, 1.0)(True)
    static = [torch.zeros(n, device=DEV) for n in ns]

    def grads(use, static_b):
        for j, n in enumerate(ns):
            gr = torch.randn(n, device=DEV, generator=g) * (0.5 if j % 3 else 5.0) / math.sqrt(n)     # (clipped: tensors 0, 3)
            if j not in use:
                pa[j].grad = pb[j].grad = None
                continue
            pa[j].grad = gr.clone()
            pb[j].grad = static[j] if static_b else gr.clone()
            if static_b:
                static[j].copy_(gr)

    def same(what):
        for j in range(len(ns)):
            sa, sb = oa.state[pa[j]], ob.state[pb[j]]
            assert torch.equal(pa[j], pb[j]), (what, j)
            assert torch.equal(sa['next_m'], sb['next_m']) and torch.equal(sa['next_v'], sb['next_v']), (what, j)
            assert sa['step'] == sb['step'], (what, j, sa['step'], sb['step'])

    def replay(what):
        grads(range(4), True)
        oa.step()
        ob.refresh_lr()
        graph.replay()
        ob.advance()
        same(what)

    grads(range(4), True)
    oa.step()
    ob.step()
    same("eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # (the capture pass does not execute)
        ob.step()
    replay("first replay")
    grads((0, 3), False)                                            # other record bytes, small and large: fresh uploads
    oa.step()
    ob.step()
    same("eager on a subset")
    replay("replay after the subset")
    grads(range(4), False)                                          # tables of the captured size, other gradient addresses
    oa.step()
    ob.step()
    same("eager on other gradients")
    replay("last replay")
    assert [oa.state[p]['step'] for p in pa] == [6, 5, 5, 6]
