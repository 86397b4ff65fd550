"""What a GEMM workgroup does before its first MFMA, one op at a time (needs a real MI355X, ``-m gpu``): the reduction of the
producer's partial row statistics (folded LayerNorm, the residual epilogue's re-centring) at every slot count up to
CC_LN_MAX_SLOTS, the rider's device-side row count, and the few-rows kernel against outputs recorded before the prologue was
reworked (tests/golden/gemm_rows_prologue.npz, written by tools/gen_golden_gemm_prologue.py).

Every check here is on bits.  The statistics are fp32 sums in slot order, left to right:
  * integer-valued partials make every order exact, so all slot counts of one row sum must give the same output bits;
  * generic partials are built to cancel (+-2^24 / +-2^26 pairs around small terms), so that the sum depends on the order in
    its leading digits; the host adds them in fp32, left to right, and hands the result to the same launch as ONE slot, which
    then has nothing left to add.  Mean, variance, rsqrt and the epilogue are the kernel's own in both launches (the compiler
    may contract them, which a host restatement could not follow), the adds are the host's.  The LayerNorm-folded Linear is
    checked against float64 on top, with the bound test_clip_gpu.py states for the same op (3e-3 of the largest entry)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOT_COUNTS = (1, 7, 8, 9, 12, 16, 17, 24, 32)                  # 32 = CC_LN_MAX_SLOTS (asserted below)
EPI_F16, EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32_RESID_STATS = 0, 5, 6, 7
TILES = {1: (128, 128, 64), 2: (128, 64, 64), 3: (64, 128, 64), 4: (64, 64, 64), 5: (256, 256, 64), 6: (256, 128, 64),
         7: (256, 192, 64), 8: (64, 64, 128), 10: (128, 256, 64)}   # id -> BM, BN, BK
GUARD = 3
SENT32, SENT16 = -31337.25, -1234.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_rows_prologue.npz")


def _lib():
    from centerclip_amd import _lib as L
    return L, L.lib()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def ptr(t):
    return t.data_ptr() if t is not None else None


def tiles_for(N, K, resid=False):
    """auto + every tile id that divides the shape (7 exists for the fp16-output epilogues only)"""
    return [0] + [t for t, (_, bn, bk) in TILES.items() if N % bn == 0 and K % bk == 0 and not (resid and t == 7)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ partial statistics
def seq_sum(p):
    """fp32 sum over the last axis, left to right, starting from +0 - the kernel's order"""
    s = np.zeros(p.shape[:-1], dtype=np.float32)
    for u in range(p.shape[-1]):
        s = (s + p[..., u]).astype(np.float32)
    return s


def int_partials(rng, total, slots, spread):
    """[M, slots] integer-valued fp32 partials that sum to `total` [M] (int64); every partial sum stays far below 2^24"""
    p = rng.randint(-spread, spread + 1, size=(total.shape[0], slots)).astype(np.int64)
    p[:, -1] = total - p[:, :-1].sum(1)
    assert np.abs(p).sum(1).max() < 2 ** 23
    return p.astype(np.float32)


def cancelling_partials(rng, M, slots, big, draw):
    """[M, slots] fp32: small terms `draw(shape)`, with +big on slot i and -big on slot i + 2 for every fourth i: added left to
    right the small terms between them lose their low bits, in another order (or more accurately) they do not"""
    p = draw((M, slots)).astype(np.float32)
    for i in range(0, slots - 2, 4):
        p[:, i] += np.float32(big)
        p[:, i + 2] -= np.float32(big)
    return p.astype(np.float32)


def generic_stats(seed, M, slots, K):
    """-> (stats [M, slots, 2] fp32 with order-dependent sums, the same summed by the host into one slot [M, 1, 2])"""
    rng = np.random.RandomState(seed)
    s = cancelling_partials(rng, M, slots, 2.0 ** 24, lambda sh: rng.standard_normal(sh) * 4.0)
    q = cancelling_partials(rng, M, slots, 2.0 ** 26, lambda sh: rng.uniform(0.5, 1.5, sh) * (4.0 * K / slots))
    st = np.stack([s, q], axis=-1)
    one = np.stack([seq_sum(s), seq_sum(q)], axis=-1)[:, None, :]
    if slots >= 3:                                               # the inputs discriminate: fp32 in slot order is not the exact sum
        exact = np.stack([s.astype(np.float64).sum(1), q.astype(np.float64).sum(1)], axis=-1).astype(np.float32)
        differ = float((one[:, 0, :] != exact).mean())
        assert differ > 0.5 or M < 8, (slots, differ)
    assert (one[:, 0, 1] / K - (one[:, 0, 0] / K) ** 2 > 0.5).all()          # a sane variance for the LayerNorm
    return st.astype(np.float32), one.astype(np.float32)


_ln_inputs = {}


def ln_inputs(N, K, M=300):
    """integer-valued fp16 rows with their exact sums, a weight and the fold's column vectors (any values do: the kernel
    evaluates rs * (x w^T - mu c1) + c2 whatever they mean)"""
    if (N, K) not in _ln_inputs:
        rng = np.random.RandomState(1000 + N + K)
        x = rng.randint(-4, 5, size=(M, K))
        x[:, 0] = 4
        x[:, 1] = -4                                             # no constant row
        w = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float16)
        c1 = (rng.standard_normal(N) * 0.3).astype(np.float32)
        c2 = (rng.standard_normal(N) * 0.2).astype(np.float32)
        _ln_inputs[(N, K)] = dict(x=x, h16=dev(x.astype(np.float16)), w=dev(w), c1=dev(c1), c2=dev(c2), tot=x.sum(1),
                                  totsq=(x * x).sum(1))
    return _ln_inputs[(N, K)]


def int_stats(inp, slots, seed):
    rng = np.random.RandomState(seed)
    return dev(np.stack([int_partials(rng, inp["tot"], slots, 1000), int_partials(rng, inp["totsq"], slots, 5000)], axis=-1))


def test_slot_bound_is_the_librarys():
    from centerclip_amd import ops
    assert ops.LN_MAX_SLOTS == SLOT_COUNTS[-1]


# ------------------------------------------------------------------------------------------------ a. slot counts, exact partials
@pytest.mark.parametrize("N,K", [(192, 64), (192, 128), (256, 64), (256, 128)])
def test_linear_ln_every_slot_count_gives_the_same_bits(N, K):
    from centerclip_amd import ops
    inp = ln_inputs(N, K)
    stats = {s: int_stats(inp, s, 7 * s + K) for s in SLOT_COUNTS}
    ran = 0
    for M in (1, 65, 257):
        for tile in tiles_for(N, K):
            for gelu in (False, True):
                outs = {s: ops.linear_ln_f16(inp["h16"][:M], inp["w"], inp["c1"], inp["c2"], stats[s][:M].contiguous(), s, gelu=gelu,
                                             tile=tile) for s in SLOT_COUNTS}
                assert bool(torch.isfinite(outs[1].float()).all())
                for s in SLOT_COUNTS:
                    assert same_bits(outs[s], outs[1]), (M, tile, gelu, s)
                ran += 1
    print("linear_ln N = %d K = %d: %d (M, tile, activation) cases x %d slot counts, all bit-equal" % (N, K, ran, len(SLOT_COUNTS)))


# (nseq, L, packed lengths or None): M = 1, 65, 257 rows as the issue lists them, and 300 rows of packed sequences
ATTN_CASES = [(1, 1, None), (5, 13, None), (257, 1, None), (1, 65, None), (3, 100, (100, 57, 100))]


def attn_run(inp, st, slots, nseq, L, heads, lens):
    from centerclip_amd import ops
    M = nseq * L
    kw = {}
    if lens is not None:
        kw = dict(seq_off=dev(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)), seq_len=dev(np.asarray(lens, np.int32)))
    return ops.inproj_attention_f16(inp["h16"][:M], inp["w"], inp["c1"], inp["c2"], st[:M].contiguous(), slots, nseq, L, heads, **kw)


@pytest.mark.parametrize("heads", [1, 2])                       # K = W = 64 / 128, N = 3 W = 192 / 384 (the form has no N = 256)
def test_inproj_attention_every_slot_count_gives_the_same_bits(heads):
    from centerclip_amd import ops
    W = heads * 64
    inp = ln_inputs(3 * W, W)
    stats = {s: int_stats(inp, s, 11 * s + W) for s in SLOT_COUNTS}
    for nseq, L, lens in ATTN_CASES:
        outs = {s: attn_run(inp, stats[s], s, nseq, L, heads, lens) for s in SLOT_COUNTS}
        assert bool(torch.isfinite(outs[1].float()).all())
        for s in SLOT_COUNTS:
            assert same_bits(outs[s], outs[1]), (nseq, L, lens, s)
        if lens is None and L <= 56:                             # the one-launch form against its two launches, bit for bit
            M = nseq * L
            qkv = ops.linear_ln_f16(inp["h16"][:M], inp["w"], inp["c1"], inp["c2"], stats[12][:M].contiguous(), 12)
            assert same_bits(outs[12], ops.attention_f16(qkv, nseq, L, heads)), (nseq, L)


# ------------------------------------------------------------------------------------------------ b. generic partials
@pytest.mark.parametrize("N,K", [(192, 64), (192, 128), (256, 64), (256, 128)])
def test_linear_ln_generic_partials_are_added_in_slot_order(N, K):
    from centerclip_amd import ops
    inp = ln_inputs(N, K)
    worst = 0.0
    for s in SLOT_COUNTS:
        st, one = generic_stats(100 * s + K, 257, s, K)
        std, oned = dev(st), dev(one)
        # float64 on the host-added sums and the same fp16 operands
        mu = oned[:, 0, 0].double() / K
        rs = 1.0 / torch.sqrt((oned[:, 0, 1].double() / K - mu * mu).clamp_min(0.0) + 1e-5)
        pre = rs[:, None] * (inp["h16"][:257].double() @ inp["w"].double().t() - mu[:, None] * inp["c1"].double()) + inp["c2"].double()
        for M in (1, 65, 257):
            for tile in tiles_for(N, K):
                for gelu in (False, True):
                    got = ops.linear_ln_f16(inp["h16"][:M], inp["w"], inp["c1"], inp["c2"], std[:M].contiguous(), s, gelu=gelu, tile=tile)
                    want = ops.linear_ln_f16(inp["h16"][:M], inp["w"], inp["c1"], inp["c2"], oned[:M].contiguous(), 1, gelu=gelu, tile=tile)
                    assert same_bits(got, want), (s, M, tile, gelu)
                    ref = pre[:M] * torch.sigmoid(1.702 * pre[:M]) if gelu else pre[:M]
                    e = float((got.double() - ref).abs().max() / ref.abs().max())
                    worst = max(worst, e)
                    assert e < 3e-3, (s, M, tile, gelu, e)
    print("linear_ln N = %d K = %d, generic partials: bit-equal to the host-added one-slot launch at every slot count; worst "
          "error vs float64 %.3g (bound 3e-03)" % (N, K, worst))


@pytest.mark.parametrize("heads", [1, 2])
def test_inproj_attention_generic_partials_are_added_in_slot_order(heads):
    """(bit-equality to the host-added one-slot launch; the attention itself is held to float64 by test_r4_gpu.py)"""
    W = heads * 64
    inp = ln_inputs(3 * W, W)
    for s in SLOT_COUNTS:
        st, one = generic_stats(200 * s + W, 300, s, W)
        std, oned = dev(st), dev(one)
        for nseq, L, lens in ATTN_CASES:
            got = attn_run(inp, std, s, nseq, L, heads, lens)
            assert bool(torch.isfinite(got.float()).all())
            assert same_bits(got, attn_run(inp, oned, 1, nseq, L, heads, lens)), (s, nseq, L, lens)


# ------------------------------------------------------------------------------------------------ c. residual re-centring
@pytest.mark.parametrize("M", [65, 300])
def test_residual_recentring_adds_the_shift_slots_in_order(M):
    """cc_linear_resid_stats_f16 with the previous sublayer's partial sums in 1 / 8 / 12 / 24 slots against the same launch with
    those slots added by the host (fp32, slot order) into one: the fp32 rows, the centred fp16 copy, shift_out and the
    written statistics, bit for bit."""
    from centerclip_amd import ops
    N = K = 128
    rng = np.random.RandomState(77 + M)
    a = dev((rng.standard_normal((M, K))).astype(np.float16))
    w = dev((rng.standard_normal((N, K)) * K ** -0.5).astype(np.float16))
    bias = dev((rng.standard_normal(N) * 0.5).astype(np.float32))
    h0 = dev((rng.standard_normal((M, N)) * 2 + 0.3).astype(np.float32))
    shift_in = dev((rng.standard_normal(M) * 0.5).astype(np.float32))
    for s in (1, 8, 12, 24):
        sums = cancelling_partials(rng, M, s, 2.0 ** 24, lambda sh: rng.standard_normal(sh) * 16.0)
        st = np.stack([sums, rng.uniform(1.0, 2.0, sums.shape).astype(np.float32)], axis=-1).astype(np.float32)
        one = np.stack([seq_sum(sums), np.ones(M, np.float32)], axis=-1)[:, None, :].astype(np.float32)
        if s >= 3:
            assert float((one[:, 0, 0] != sums.astype(np.float64).sum(1).astype(np.float32)).mean()) > 0.5
        for tile in tiles_for(N, K, resid=True):
            res = []
            for stats_in in (dev(st), dev(one)):
                h = h0.clone()
                h16, stats, slots, shift_out = ops.linear_resid_stats_f16(a, w, bias, h, tile=tile, shift_in=shift_in, stats_in=stats_in)
                res.append((h, h16, stats.clone(), slots, shift_out))
            (h_a, c_a, st_a, sl_a, sh_a), (h_b, c_b, st_b, sl_b, sh_b) = res
            tag = (M, s, tile)
            assert sl_a == sl_b, tag
            assert same_bits(h_a, h_b) and same_bits(c_a, c_b) and same_bits(st_a, st_b) and same_bits(sh_a, sh_b), tag
            # c_row = shift_in + sum / N, the copy is centred by it
            want_shift = shift_in + dev(one[:, 0, 0]) / N
            assert float((sh_a - want_shift).abs().max()) <= 1e-6 * float(want_shift.abs().max()), tag
            assert torch.equal(c_a, (h_a - sh_a[:, None]).half()), tag


# ------------------------------------------------------------------------------------------------ d. rider with a device-side row count
def sentinel(rows, cols, dtype):
    return torch.full((rows, cols), SENT16 if dtype == torch.float16 else SENT32, dtype=dtype, device=DEV)


def holds_sentinel(t):
    return bool((bits(t) == bits(torch.full((1,), SENT16 if t.dtype == torch.float16 else SENT32, dtype=t.dtype, device=DEV))).all())


class PairProblem:
    """one fp16-output problem of cc_linear_pair_f16 (EPI_F16 or EPI_F16_LN) with a sentinel-filled output"""

    def __init__(self, M, N, K, seed, epi):
        rng = np.random.RandomState(seed)
        self.M, self.N, self.K, self.epi = M, N, K, epi
        self.a = dev(rng.standard_normal((M, K)).astype(np.float16))
        self.w = dev((rng.standard_normal((N, K)) * K ** -0.5).astype(np.float16))
        self.bias = dev((rng.standard_normal(N) * 0.5).astype(np.float32))
        self.c1 = dev((rng.standard_normal(N) * 0.3).astype(np.float32))
        self.stats = dev(generic_stats(seed + 1, M, 12, K)[0])

    def struct(self, out, M=None, m_dev=None):
        L, _ = _lib()
        p = L.LinearProblem(a=ptr(self.a), w=ptr(self.w), bias=ptr(self.bias), c=ptr(out), M=self.M if M is None else M, N=self.N,
                            K=self.K, ldc=self.N, m_dev=ptr(m_dev))
        if self.epi == EPI_F16_LN:
            p.ln_stats, p.ln_slots, p.ln_c1, p.ln_eps = ptr(self.stats), 12, ptr(self.c1), 1e-5
        return p

    def out(self):
        return sentinel(self.M + GUARD, self.N, torch.float16)


def pair_launch(p0, p1, epi, tile):
    L, lib = _lib()
    slots = (ctypes.c_int32 * 2)()
    rc = lib.cc_linear_pair_f16(ctypes.byref(p0), ctypes.byref(p1) if p1 is not None else None, epi, tile, slots, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("epi", [EPI_F16, EPI_F16_LN])
def test_rider_with_device_side_row_count(epi):
    carrier, rider = PairProblem(300, 256, 128, 31, epi), PairProblem(65, 128, 64, 32, epi)
    for tile in (1, 4, 6):                                       # 128x128, 64x64, 256x128: each divides both problems
        alone = carrier.out()
        assert pair_launch(carrier.struct(alone), None, epi, tile) == 0
        assert holds_sentinel(alone[carrier.M:]) and not holds_sentinel(alone[:carrier.M])
        for m in (0, 1, rider.M):
            m_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
            co, ro = carrier.out(), rider.out()
            assert pair_launch(carrier.struct(co), rider.struct(ro, m_dev=m_dev), epi, tile) == 0, (tile, m)
            assert same_bits(co, alone), (tile, m)                                  # the carrier is unchanged
            assert holds_sentinel(ro[m:]), (tile, m)                                # rows behind the count are untouched
            if m:
                want = rider.out()
                assert pair_launch(rider.struct(want, M=m), None, epi, tile) == 0
                assert same_bits(ro[:m], want[:m]) and bool(torch.isfinite(ro[:m].float()).all()), (tile, m)


# ------------------------------------------------------------------------------------------------ e. the few-rows kernel, recorded outputs
ROWS_M = (1, 16, 48, 64, 65)
ROWS_N, ROWS_K, ROWS_SLOTS = 64, 288, 12                          # two column blocks; 9 k-steps: a ragged last wave


def rows_case(M, addr, epi):
    """-> (struct fields kept alive, outputs by name) of one few-rows problem; inputs from a seeded numpy stream"""
    L, _ = _lib()
    rng = np.random.RandomState(9000 + 10 * M + (1 if addr == "map" else 0) + 100 * epi)
    N, K = ROWS_N, ROWS_K
    if addr == "map":
        R = 2 * M + 3
        prow = rng.permutation(R)[:M]
        row_map, row_step = dev(prow.astype(np.int32)), 0
    else:
        R, prow, row_map, row_step = (M - 1) * 2 + 2, np.arange(M) * 2, None, 2
    keep = dict(a=dev(rng.standard_normal((R, K)).astype(np.float16)), w=dev((rng.standard_normal((N, K)) * K ** -0.5).astype(np.float16)),
                bias=dev((rng.standard_normal(N) * 0.5).astype(np.float32)), row_map=row_map)
    out = {}
    p = L.LinearProblem(a=ptr(keep["a"]), w=ptr(keep["w"]), bias=ptr(keep["bias"]), M=M, N=N, K=K, ldc=N, row_step=row_step,
                        row_map=ptr(row_map))
    if epi == EPI_F16_GELU_LN:
        keep["stats"] = dev(generic_stats(int(rng.randint(1 << 30)), R, ROWS_SLOTS, K)[0])
        keep["c1"] = dev((rng.standard_normal(N) * 0.3).astype(np.float32))
        out["C"] = sentinel(R + GUARD, N, torch.float16)
        p.ln_stats, p.ln_slots, p.ln_c1, p.ln_eps = ptr(keep["stats"]), ROWS_SLOTS, ptr(keep["c1"]), 1e-5
    else:
        sums = cancelling_partials(rng, R, ROWS_SLOTS, 2.0 ** 24, lambda sh: rng.standard_normal(sh) * 16.0)
        keep["shift_stats"] = dev(np.stack([sums, np.ones_like(sums)], axis=-1).astype(np.float32))
        keep["shift_in"] = dev((rng.standard_normal(R) * 0.5).astype(np.float32))
        out["C"] = sentinel(R + GUARD, N, torch.float32)
        out["C"][dev(prow.astype(np.int64))] = dev((rng.standard_normal((M, N)) * 2 + 0.3).astype(np.float32))
        out["c16"] = sentinel(R + GUARD, N, torch.float16)
        out["stats"] = sentinel(R + GUARD, (N // 32) * 2, torch.float32)
        out["shift"] = sentinel(R + GUARD, 1, torch.float32)
        p.c16, p.stats_out, p.shift_out = ptr(out["c16"]), ptr(out["stats"]), ptr(out["shift"])
        p.shift_in, p.shift_stats, p.shift_slots = ptr(keep["shift_in"]), ptr(keep["shift_stats"]), ROWS_SLOTS
    p.c = ptr(out["C"])
    return p, keep, out


def rows_run(M, addr, epi):
    L, lib = _lib()
    p, keep, out = rows_case(M, addr, epi)
    slots = (ctypes.c_int32 * 2)()
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(p), None, epi, slots, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    del keep
    return {k: bits(v).cpu().numpy() for k, v in out.items()}


def write_golden(path=GOLDEN):
    """(tools/gen_golden_gemm_prologue.py, on the commit BEFORE the prologue change)"""
    rec = {}
    for epi in (EPI_F16_GELU_LN, EPI_F32_RESID_STATS):
        for addr in ("map", "step"):
            for M in ROWS_M:
                for k, v in rows_run(M, addr, epi).items():
                    rec["e%d/%s/m%d/%s" % (epi, addr, M, k)] = v
    np.savez_compressed(path, **rec)
    return path, len(rec)


@pytest.mark.parametrize("epi", [EPI_F16_GELU_LN, EPI_F32_RESID_STATS])
@pytest.mark.parametrize("addr", ["map", "step"])
def test_few_rows_kernel_gives_the_recorded_bits(addr, epi):
    gold = np.load(GOLDEN)
    for M in ROWS_M:
        got = rows_run(M, addr, epi)
        for k, v in got.items():
            want = gold["e%d/%s/m%d/%s" % (epi, addr, M, k)]
            assert v.shape == want.shape and v.dtype == want.dtype and np.array_equal(v, want), (epi, addr, M, k)
        sent = np.int32(np.float32(SENT32).view(np.int32)) if got["C"].dtype == np.int32 else np.int16(np.float16(SENT16).view(np.int16))
        assert int((got["C"] != sent).any(axis=1).sum()) == M, (epi, addr, M)       # exactly the selected rows were written
