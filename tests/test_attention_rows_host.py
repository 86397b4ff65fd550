"""The yardsticks of tests/test_attention_rows_gpu.py, checked without a GPU.

The GPU tests hold every attention kernel to attention_ref.forward_bound / backward_bound, element by element, on inputs
with peaked, drifting, extreme and floor-level scores.  Such a bound is only worth something if (a) the documented
arithmetic - emulated here in numpy with fp16 P, fp32 sums, the online rescale of the streamed form and per-head scales in
the backward pass - stays inside it on EVERY recipe and shape of the GPU sweep, and (b) a subtly wrong kernel does not.
(b) is shown with mutants of the emulation; CAUGHT_BY names the recipe on which each one must exceed the bound (or miss
the bit-exact uniform_coded output):

  drop_last_key      the last key of a ragged tile dropped            uniform_coded (bits), peaked (bound: somebody's peak)
  double_key         a key counted twice                              uniform_coded (bits)
  stale_max          alpha forced to 1 in the streamed form           ascending (bound)
  neighbour_leak     padding keys read from the next sequence, 1e-6   loud_neighbour (bound)
  swap_norm          P rounded unnormalised in the resident form,     uniform_coded (bits)
                     normalised in the streamed form
  causal_off_by_one  key q + 1 visible                                uniform_coded (bits), ascending (bound)
  launch_scale       one pair of fp16 scales per launch (backward)    gaussian and every other backward recipe (bound)

The last test records why the per-element measure is needed: the suite's older global measures (4e-3 / 2e-3 of the largest
entry of the whole tensor) accept the neighbour_leak and launch_scale mutants.
"""
import numpy as np
import pytest

import attention_ref as ar

NSEQ, HEADS = ar.NSEQ, ar.HEADS
ALL_L = [L for k in ("wave", "block", "long") for L in ar.FORWARD_LENGTHS[k]]
CAUGHT_BY = {
    "drop_last_key": ("uniform_coded", "peaked"),
    "double_key": ("uniform_coded",),
    "stale_max": ("ascending",),
    "neighbour_leak": ("loud_neighbour",),
    "swap_norm": ("uniform_coded",),
    "causal_off_by_one": ("uniform_coded", "ascending"),
}


def _forward_case(recipe, L, causal, mutant=None, form=None):
    lens, offs = ar.uniform_layout(NSEQ, L)
    form = form or ar.form_of(L)
    qkv = ar.make_qkv(recipe, lens, offs, HEADS, seed=L)
    y = ar.emulate_forward(qkv, lens, offs, HEADS, causal, form, mutant)
    ref = ar.attention_float64(qkv, lens, offs, HEADS, causal)
    bound = ar.forward_bound(qkv, lens, offs, HEADS, causal, form)
    err = np.abs(y.astype(np.float64) - ref)
    bits = None
    if recipe == "uniform_coded":
        bits = np.array_equal(y.view(np.uint16), ar.uniform_coded_expected(lens, offs, HEADS, causal, form).view(np.uint16))
    return err, bound, bits, ref


def _rejected(err, bound, bits):
    return bool((err > bound).any()) or bits is False


# ----------------------------------------------------------------------------------------------- the recipes are what they say
def test_recipes_have_the_properties_they_are_named_for():
    for L in (50, 197, 577):
        lens, offs = ar.uniform_layout(NSEQ, L)
        for recipe in ar.RECIPES:
            qkv = ar.make_qkv(recipe, lens, offs, HEADS, seed=L)
            assert np.isfinite(qkv.astype(np.float32)).all()
            q, k, v = ar._heads_of(qkv, 0, L, HEADS, np.float64)
            s = q[0] @ k[0].T / 8.0
            top2 = np.sort(s, axis=1)[:, -2:]
            if recipe == "peaked":
                assert (top2[:, 1] - top2[:, 0] >= 30.0).all()
            elif recipe == "ascending":
                assert (s[:, 64:] - s[:, :-64] >= 20.0).all()
            elif recipe == "descending":
                assert (s[:, :-64] - s[:, 64:] >= 20.0).all()
            elif recipe == "extreme":
                assert np.abs(s).max() > 1000.0 and np.abs(qkv[:, :2 * HEADS * 64].astype(np.float32)).max() <= 20.0
            elif recipe == "floor":
                assert set(np.round(np.unique(s), 1)) == {0.0, -10.0, -12.0, -16.6, -18.0}
                assert (np.sum(s == 0.0, axis=1) == 1).all()
            elif recipe == "uniform_coded":
                assert not s.any()
            elif recipe == "loud_neighbour":
                q1, k1, v1 = ar._heads_of(qkv, L, L, HEADS, np.float64)
                assert np.abs(v[0]).max() <= 1.0 and (np.abs(v1[0]) == 30000.0).all() and (np.abs(k1[0]) == 15.0).all()


def test_backward_reference_matches_the_closed_form():
    lens, offs = ar.uniform_layout(2, 37)
    qkv = ar.make_qkv("gaussian", lens, offs, HEADS, seed=1)
    do = ar.make_d_out(lens, offs, HEADS, seed=1)
    want = ar.attention_backward_float64(qkv, do, lens, offs, HEADS, True)
    q, k, v = ar._heads_of(qkv, 37, 37, HEADS, np.float64)
    _, _, p = ar._softmax64(q[1], k[1], True)
    g = do[37:, 64:].astype(np.float64)
    dp = g @ v[1].T
    ds = p * (dp - (p * dp).sum(axis=1, keepdims=True))
    W = HEADS * 64
    np.testing.assert_allclose(want[37:, 64:128], ds @ k[1] / 8.0, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(want[37:, W + 64:W + 128], ds.T @ q[1] / 8.0, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(want[37:, 2 * W + 64:], p.T @ g, rtol=1e-10, atol=1e-300)


# ------------------------------------------------------------------------- (a) the documented arithmetic is inside the bound
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ALL_L)
def test_emulation_is_within_the_forward_bound(L, causal):
    worst = {}
    for recipe in ar.RECIPES:
        err, bound, bits, _ = _forward_case(recipe, L, causal)
        worst[recipe] = ar.share_of_bound(err, bound)
        assert bits is not False, (recipe, "the emulation misses the bit-exact output")
    print("L %d causal %d: share of the bound" % (L, causal), {r: "%.2f" % s for r, s in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("lens", ar.PACKED_LENGTHS)
def test_emulation_is_within_the_forward_bound_packed(lens):
    """Packed sequences of lengths that straddle the kernels' switches, with NaN in the gap and guard rows: reference, bound
    and emulation read nothing outside a sequence (the layout a GPU test of the seq_off / seq_len form would use)."""
    offs, rows = ar.packed_layout(lens)
    form = ar.form_of(max(lens))
    for causal in (False, True):
        for recipe in ar.RECIPES:
            qkv = ar.make_qkv(recipe, lens, offs, HEADS, seed=sum(lens), rows=rows, fill=np.nan)
            y = ar.emulate_forward(qkv, lens, offs, HEADS, causal, form)
            ref = ar.attention_float64(qkv, lens, offs, HEADS, causal)
            bound = ar.forward_bound(qkv, lens, offs, HEADS, causal, form)
            assert ar.share_of_bound(np.abs(y.astype(np.float64) - ref), bound) <= 1.0, (recipe, causal)


@pytest.mark.parametrize("kind", ar.FUSED_KINDS)
@pytest.mark.parametrize("L", ar.FUSED_LENGTHS)
def test_emulation_is_within_the_forward_bound_fused_inputs(L, kind):
    for lens in ([L] * NSEQ, [L, max(1, L // 3), L - 1 if L > 1 else 1]):
        offs = [int(o) for o in np.concatenate([[0], np.cumsum(lens)[:-1]])]
        qkv = ar.fused_qkv_float64(*ar.fused_inputs(kind, lens, HEADS, seed=L))
        q, k, v = ar._heads_of(qkv, offs[1], lens[1], HEADS, np.float64)
        if kind == "high_gain":
            assert np.abs(q[0] @ k[0].T / 8.0).max() > 100.0
        else:
            q0, k0, v0 = ar._heads_of(qkv, 0, lens[0], HEADS, np.float64)
            assert np.abs(v[0]).max() > 1000.0 and np.abs(v0[0]).max() < 8.0
        for causal in (False, True):
            for mutant in (None, "swap_norm"):                # the fused form above 56 tokens rounds the unnormalised P
                y = ar.emulate_forward(qkv, lens, offs, HEADS, causal, "resident", mutant)
                err = np.abs(y.astype(np.float64) - ar.attention_float64(qkv, lens, offs, HEADS, causal))
                assert ar.share_of_bound(err, ar.forward_bound(qkv, lens, offs, HEADS, causal, "resident")) <= 1.0


def _backward_case(recipe, L, causal, mutant=None):
    lens, offs = ar.uniform_layout(NSEQ, L)
    qkv = ar.make_qkv(recipe, lens, offs, HEADS, seed=L)
    do = ar.make_d_out(lens, offs, HEADS, seed=L)
    got = ar.emulate_backward(qkv, do, lens, offs, HEADS, causal, mutant)
    want = ar.attention_backward_float64(qkv, do, lens, offs, HEADS, causal)
    bound = ar.backward_bound(qkv, do, lens, offs, HEADS, causal)
    return np.abs(got.astype(np.float64) - want), bound, want


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", ar.BACKWARD_LENGTHS)
def test_emulation_is_within_the_backward_bound(L, causal):
    worst = {}
    for recipe in ar.BACKWARD_RECIPES:
        err, bound, _ = _backward_case(recipe, L, causal)
        lens, offs = ar.uniform_layout(NSEQ, L)
        worst[recipe] = max(ar.share_of_bound(e, b) for (_, e), (_, b) in
                            zip(ar.head_blocks(err, lens, offs, HEADS, 3), ar.head_blocks(bound, lens, offs, HEADS, 3)))
    print("L %d causal %d: share of the bound" % (L, causal), {r: "%.2f" % s for r, s in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------- (b) the mutants are outside of it
@pytest.mark.parametrize("mutant", ar.FORWARD_MUTANTS)
def test_forward_mutants_are_rejected(mutant):
    """Every mutant is rejected on each recipe CAUGHT_BY names, at one shape per kernel family where the mutation can act (a
    ragged last tile; the streamed form for stale_max; the causal mask for causal_off_by_one)."""
    causal = mutant == "causal_off_by_one"
    # (swap_norm: up to 64 keys every code is 1 and both orders round the same number 1 / n, so the forms agree bit for bit)
    shapes = {"stale_max": (321, 577), "swap_norm": (197, 577)}.get(mutant, (50, 197, 577))
    matrix = {}
    for L in shapes:
        for recipe in ar.RECIPES:
            matrix[(L, recipe)] = _rejected(*_forward_case(recipe, L, causal, mutant)[:3])
    print(mutant, "rejected on:", sorted(k for k, hit in matrix.items() if hit))
    for L in shapes:
        for recipe in CAUGHT_BY[mutant]:
            assert matrix[(L, recipe)], (mutant, L, recipe)


@pytest.mark.parametrize("L", [50, 64, 197, 320])
def test_launch_wide_scale_is_rejected(L):
    for recipe in ar.BACKWARD_RECIPES:
        err, bound, _ = _backward_case(recipe, L, False, "launch_scale")
        assert (err > bound).any(), recipe
        lens, offs = ar.uniform_layout(NSEQ, L)
        hit = [key for (key, e), (_, b) in zip(ar.head_blocks(err, lens, offs, HEADS, 3), ar.head_blocks(bound, lens, offs, HEADS, 3))
               if (e > b).any()]
        assert (NSEQ - 1, HEADS - 1) in hit and (0, 0) not in hit, (recipe, hit)     # the quietest head loses, the loudest does not


# ------------------------------------------------------------------------------- why the global measures were not enough
def test_global_measures_accept_the_leak_and_the_launch_wide_scale():
    """test_attention's measure (max |delta| < 4e-3 of the largest output entry) accepts the neighbour leak, and the backward
    tests' measure (2e-3 of the largest entry of each q / k / v part over all sequences and heads) accepts the launch-wide
    scale; the per-element bound rejects both on the same inputs."""
    for L in (50, 197, 577):
        err, bound, _, ref = _forward_case("loud_neighbour", L, False, "neighbour_leak")
        assert err.max() < 4e-3 * np.abs(ref).max() and (err > bound).any()
    W = HEADS * 64
    for L in (50, 197):
        err, bound, want = _backward_case("gaussian", L, False, "launch_scale")
        for part in range(3):
            sl = slice(part * W, (part + 1) * W)
            assert err[:, sl].max() <= 2e-3 * np.abs(want[:, sl]).max()
        assert (err > bound).any()
