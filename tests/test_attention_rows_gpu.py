"""The matrix-core attention kernels on the MI355X (``-m gpu``), element by element against float64 inside the a-priori
bounds of tests/attention_ref.py, on scores that are peaked, drift from key tile to key tile, reach the thousands or sit at
the fp16 floor of P; with loud neighbouring sequences whose rows a dropped guard would read; and, for the backward kernels,
with d_out magnitudes 2^12 apart between the heads of a sequence and between sequences.
tests/test_attention_rows_host.py shows without a GPU that the documented arithmetic stays inside these bounds on every case
below and that dropped, doubled, leaked or mis-scaled keys do not.

Every case prints the share of the bound it used; the last test prints the largest share per kernel (DESIGN.md records them).
"""
import numpy as np
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NSEQ, HEADS, W = ar.NSEQ, ar.HEADS, ar.HEADS * 64
SHARES = {}


def _note(kernel, share):
    SHARES[kernel] = max(SHARES.get(kernel, 0.0), share)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


FORWARD_CASES = [(k, L) for k in ("wave", "block", "long") for L in ar.FORWARD_LENGTHS[k]]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("recipe", ar.RECIPES)
@pytest.mark.parametrize("kernel,L", FORWARD_CASES)
def test_forward_rows_within_the_bound(kernel, L, recipe, causal):
    """ops.attention_f16 frame-major and its LND form on the same sequences: |y - float64| <= bound for
    every element; uniform_coded also bit for bit against the output worked out from the documented arithmetic."""
    from centerclip_amd import ops
    assert ar.kernel_of(L) == kernel
    lens, offs = ar.uniform_layout(NSEQ, L)
    form = ar.form_of(L)
    qkv_np = ar.make_qkv(recipe, lens, offs, HEADS, seed=L)
    ref = ar.attention_float64(qkv_np, lens, offs, HEADS, causal)
    bound = ar.forward_bound(qkv_np, lens, offs, HEADS, causal, form)
    qkv = _dev(qkv_np)
    y = ops.attention_f16(qkv, NSEQ, L, HEADS, causal)
    lnd = qkv.view(NSEQ, L, -1).permute(1, 0, 2).contiguous().view(NSEQ * L, -1)
    y_lnd = ops.attention_f16(lnd, NSEQ, L, HEADS, causal, seq_rows=1, tok_rows=NSEQ).view(L, NSEQ, -1).permute(1, 0, 2).reshape(NSEQ * L, -1)
    want_bits = ar.uniform_coded_expected(lens, offs, HEADS, causal, form).view(np.uint16) if recipe == "uniform_coded" else None
    for entry, got in (("frame-major", y), ("LND", y_lnd)):
        got = got.cpu().numpy()
        share = ar.share_of_bound(np.abs(got.astype(np.float64) - ref), bound)
        print("%s L %d %s causal %d %s: share of the bound %.3f" % (kernel, L, recipe, causal, entry, share))
        _note({"wave": "attention_wave_kernel", "block": "attention_kernel", "long": "attention_long_kernel"}[kernel], share)
        assert share <= 1.0, (entry, share)
        if want_bits is not None:
            assert np.array_equal(got.view(np.uint16), want_bits), entry


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("kind", ar.FUSED_KINDS)
@pytest.mark.parametrize("L", ar.FUSED_LENGTHS)
def test_fused_inproj_attention_rows_within_the_bound(L, kind, causal):
    """ops.inproj_attention_f16 (q, k, v never leave the chip), uniform and packed, against float64 on the qkv that linear_ln_f16
    returns for the same inputs: high-gain weights (peaked rows, |score| in the hundreds) and loud neighbouring sequences."""
    from centerclip_amd import ops
    for packed, lens in ((False, [L] * NSEQ), (True, [L, max(1, L // 3), max(1, L - 1)])):
        offs = [int(o) for o in np.concatenate([[0], np.cumsum(lens)[:-1]])]
        x, w, b, gamma, beta = ar.fused_inputs(kind, lens, HEADS, seed=L)
        pad = NSEQ * L - x.shape[0]
        if pad:
            x = np.concatenate([x, np.random.default_rng(L).standard_normal((pad, W)).astype(np.float32)])
        h16, st, _ = ops.row_stats(_dev(x))
        wf, c1, c2 = ops.fold_layernorm_linear(_dev(w), _dev(b), _dev(gamma), _dev(beta))
        qkv_np = ops.linear_ln_f16(h16, wf, c1, c2, st, 1).cpu().numpy()
        if packed:
            got = ops.inproj_attention_f16(h16, wf, c1, c2, st, 1, NSEQ, L, HEADS, causal=causal,
                                           seq_off=torch.tensor(offs, dtype=torch.int32, device=DEV),
                                           seq_len=torch.tensor(lens, dtype=torch.int32, device=DEV))
        else:
            got = ops.inproj_attention_f16(h16, wf, c1, c2, st, 1, NSEQ, L, HEADS, causal=causal)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        ref = ar.attention_float64(qkv_np, lens, offs, HEADS, causal)
        bound = ar.forward_bound(qkv_np, lens, offs, HEADS, causal, "resident")
        used = sum(lens)
        share = ar.share_of_bound(np.abs(got[:used].astype(np.float64) - ref[:used]), bound[:used])
        print("fused L %d %s causal %d packed %d: share of the bound %.3f" % (L, kind, causal, packed, share))
        _note("EPI_ATTN_LN, L <= 56" if L <= 56 else "EPI_ATTN_LN, L > 56", share)
        assert share <= 1.0, (packed, share)
        assert not got[used:].any()                              # rows behind the packed sequences: untouched


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("recipe", ar.BACKWARD_RECIPES)
@pytest.mark.parametrize("L", ar.BACKWARD_LENGTHS)
def test_backward_rows_within_the_bound(L, recipe, causal):
    """cc_attention_backward_f16 against float64 autograd inside backward_bound, assessed per (sequence, head): d_out of
    (sequence s, head h) has magnitude 2^(-12 (2 s + h)), so one scale per launch - or per sequence - loses whole heads."""
    from centerclip_amd import _lib as L_
    from centerclip_amd.torch_ops import _st
    lens, offs = ar.uniform_layout(NSEQ, L)
    qkv_np = ar.make_qkv(recipe, lens, offs, HEADS, seed=L)
    do_np = ar.make_d_out(lens, offs, HEADS, seed=L)
    want = ar.attention_backward_float64(qkv_np, do_np, lens, offs, HEADS, causal)
    bound = ar.backward_bound(qkv_np, do_np, lens, offs, HEADS, causal)
    qkv, d_out = _dev(qkv_np), _dev(do_np)
    got = torch.empty(NSEQ * L, 3 * W, device=DEV)
    am = torch.zeros(2, device=DEV)
    nb = L_.lib().cc_attention_backward_workspace_bytes(NSEQ, L, HEADS)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
    L_.check(L_.lib().cc_attention_backward_f16(L_.ptr(qkv), L_.ptr(d_out), L_.ptr(got), NSEQ, L, HEADS, W, int(causal),
                                                L_.ptr(am), L_.ptr(ws), nb, _st(got)), "cc_attention_backward_f16")
    torch.cuda.synchronize()
    assert float(am[0]) == float(got.abs().max())
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    shares = {key: ar.share_of_bound(e, b) for (key, e), (_, b) in
              zip(ar.head_blocks(err, lens, offs, HEADS, 3), ar.head_blocks(bound, lens, offs, HEADS, 3))}
    print("backward L %d %s causal %d: share of the bound per (sequence, head)" % (L, recipe, causal),
          {k: "%.3f" % v for k, v in shares.items()})
    _note("attention_backward_mfma_kernel" if L <= 64 else "attention_backward_q / kv kernels", max(shares.values()))
    assert max(shares.values()) <= 1.0, shares


def test_zz_largest_share_of_the_bound_per_kernel():
    """Prints what the cases above recorded (run with -s); nothing is asserted beyond share <= 1."""
    for kernel in sorted(SHARES):
        print("largest share of the bound: %-36s %.3f" % (kernel, SHARES[kernel]))
    assert all(s <= 1.0 for s in SHARES.values())
