"""The launch forms the fused encoders use, one op at a time, against float64 (needs a real MI355X, ``-m gpu``):
two problems in one launch (cc_linear_pair_f16), the few-rows kernel (cc_linear_rows_pair_f16), the device-side row
count, the patch-embedding epilogue and in_proj + attention with a rider (cc_inproj_attention_pair_f16).

Every output lives in a buffer with sentinel-filled guard rows behind it, rows a launch must not write hold the sentinel
too, and every test asserts the sentinel bit for bit.  Bounds (the ones the suite states for the same quantities, see
test_clip_gpu.py / test_r2_gpu.py / test_r4_gpu.py): fp32 outputs 2e-4 of the largest entry, fp16 outputs 2e-3,
LayerNorm-folded fp16 outputs 3e-3, summed statistics rtol 1e-5 / atol 1e-3, few-rows against all-rows kernel 2e-4 (fp32) /
3e-3 (fp16), one-launch attention 2e-3.  Each test prints its worst figure next to the bound."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32_PATCH, EPI_F32, EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32_RESID_STATS = range(8)
EPI_NAME = {0: "f16", 1: "f16_gelu", 2: "f32_resid", 4: "f32"}
GUARD = 3                                   # sentinel rows behind every output
SENT32, SENT16 = -31337.25, -1234.0         # exactly representable; never produced by the data below
TILE_OF = {(128, 128, 64): 1, (128, 64, 64): 2, (64, 128, 64): 3, (64, 64, 64): 4, (256, 256, 64): 5, (256, 128, 64): 6,
           (256, 192, 64): 7, (64, 64, 128): 8, (128, 256, 64): 10}
TILE_BN = {1: 128, 2: 64, 3: 128, 4: 64, 5: 256, 6: 128, 7: 192, 8: 64, 10: 256}


def _lib():
    from centerclip_amd import _lib as L
    return L, L.lib()


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel(rows, cols, dtype):
    return torch.full((rows, cols), SENT16 if dtype == torch.float16 else SENT32, dtype=dtype, device=DEV)


def holds_sentinel(t):
    return bool((bits(t) == bits(torch.full((1,), SENT16 if t.dtype == torch.float16 else SENT32, dtype=t.dtype, device=DEV))).all())


def untouched(buf, written_rows):
    """every row of buf [R + GUARD, ...] outside written_rows still holds the sentinel"""
    keep = torch.ones(buf.shape[0], dtype=torch.bool, device=DEV)
    if len(written_rows):
        keep[torch.as_tensor(written_rows, device=DEV, dtype=torch.long)] = False
    return holds_sentinel(buf[keep])


def randn(gen, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=gen, device=DEV) * scale + shift


def ptr(t):
    return t.data_ptr() if t is not None else None


class timing:
    """arms cc_debug_gemm_timing_* around ONE launch of the tile kernel -> .rec = (BM, BN, WM, WN, EPI, BK, M0 N0 K0 M1 N1 K1)"""

    def __enter__(self):
        _, lib = _lib()
        lib.cc_debug_gemm_timing_begin.argtypes = [ctypes.c_int]
        lib.cc_debug_gemm_timing_read.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
        torch.cuda.synchronize()
        assert lib.cc_debug_gemm_timing_begin(1) == 0
        self.rec = None
        return self

    def __exit__(self, *exc):
        _, lib = _lib()
        n = lib.cc_debug_gemm_timing_end()
        torch.cuda.synchronize()
        if n == 1:
            us, info = ctypes.c_float(), (ctypes.c_int * 12)()
            assert lib.cc_debug_gemm_timing_read(0, ctypes.byref(us), info) == 0
            self.rec = list(info)
        lib.cc_debug_gemm_timing_begin(0)
        return False

    @property
    def tile(self):
        return TILE_OF[(self.rec[0], self.rec[1], self.rec[5])]


class Spec:
    """One GEMM problem: inputs for any epilogue on R physical rows, of which the launch addresses `M` logical rows at the
    physical rows `prow` (the tile kernel: prow = 0..M-1) and computes the first `m` of them (m < M: a device-side count)."""

    def __init__(self, M, N, K, seed, rows=None, R=None, m=None, bias=True, ratio=0.0):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.M, self.N, self.K = M, N, K
        self.prow = list(range(M)) if rows is None else list(rows)
        self.R = R if R is not None else max(self.prow) + 1
        self.m = M if m is None else m
        self.m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device=DEV)
        R = self.R
        self.a = randn(gen, R, K).half()
        self.w = randn(gen, N, K, scale=K ** -0.5).half()
        self.bias = randn(gen, N, scale=0.5) if bias else None
        h0 = randn(gen, R, N, scale=2.0, shift=0.3)
        if ratio:                                            # row means large against the spread
            sign = (torch.rand(R, 1, generator=gen, device=DEV) > 0.5).float() * 2 - 1
            h0 = h0 - h0.mean(1, keepdim=True) + sign * ratio * h0.std(1, keepdim=True)
        self.h0 = h0
        # folded LayerNorm: the rows x [R, K] fp32 as the centred copy + one-slot statistics, the folded weight
        self.x = randn(gen, R, K, scale=1.5, shift=0.3)
        self.gamma, self.beta = torch.rand(K, generator=gen, device=DEV) + 0.5, randn(gen, K, scale=0.2)
        self.w2, self.b2 = randn(gen, N, K, scale=K ** -0.5), randn(gen, N, scale=0.1)
        self._ln = self._centre = None
        self.row_step, self.row_map = 0, None

    def ln(self):
        from centerclip_amd import ops
        if self._ln is None:
            h16, st, _ = ops.row_stats(self.x)
            wf, c1, c2 = ops.fold_layernorm_linear(self.w2, self.b2, self.gamma, self.beta)
            self._ln = (h16, st.contiguous(), wf, c1, c2)
        return self._ln

    def centre(self):
        from centerclip_amd import ops
        if self._centre is None:
            _, st0, sh0 = ops.row_stats(self.h0)             # what the previous sublayer left behind
            self._centre = (st0.contiguous(), sh0.contiguous())
        return self._centre

    def sel(self, n=None):
        return torch.as_tensor(self.prow[:self.m if n is None else n], device=DEV, dtype=torch.long)

    # ---- float64 on the same operands, rows = the first n logical rows
    def ref(self, epi, n=None):
        r = self.sel(n)
        if epi in (EPI_F16_LN, EPI_F16_GELU_LN):
            pre = F.layer_norm(self.x[r].double(), (self.K,), self.gamma.double(), self.beta.double(), 1e-5) @ self.w2.double().t() \
                + self.b2.double()
            return pre * torch.sigmoid(1.702 * pre) if epi == EPI_F16_GELU_LN else pre
        y = self.a[r].double() @ self.w.double().t()
        if self.bias is not None:
            y = y + self.bias.double()
        if epi == EPI_F16_GELU:
            y = y * torch.sigmoid(1.702 * y)
        if epi in (EPI_F32_RESID, EPI_F32_RESID_STATS):
            y = y + self.h0[r].double()
        return y

    # ---- output buffers of one launch (physical rows + guard) and the struct that points at them
    def outputs(self, epi, centred=True):
        R, N = self.R + GUARD, self.N
        o = {}
        if epi in (EPI_F32_RESID, EPI_F32_RESID_STATS):
            o["C"] = sentinel(R, N, torch.float32)
            o["C"][self.sel()] = self.h0[self.sel()]                  # in place: the computed rows hold the residual stream
        else:
            o["C"] = sentinel(R, N, torch.float32 if epi == EPI_F32 else torch.float16)
        if epi == EPI_F32_RESID_STATS:
            o["c16"] = sentinel(R, N, torch.float16)
            o["stats"] = sentinel(R, 32 * 2, torch.float32)           # [R][slots][2] once the slot count is known
            if centred:
                o["shift"] = sentinel(R, 1, torch.float32)
        return o

    def struct(self, epi, o, centred=True):
        L, _ = _lib()
        p = L.LinearProblem(M=self.M, N=self.N, K=self.K, ldc=self.N, c=ptr(o["C"]), m_dev=ptr(self.m_dev),
                            row_step=self.row_step, row_map=ptr(self.row_map))
        if epi in (EPI_F16_LN, EPI_F16_GELU_LN):
            h16, st, wf, c1, c2 = self.ln()
            p.a, p.w, p.bias, p.ln_stats, p.ln_slots, p.ln_c1, p.ln_eps = ptr(h16), ptr(wf), ptr(c2), ptr(st), 1, ptr(c1), 1e-5
        else:
            p.a, p.w, p.bias = ptr(self.a), ptr(self.w), ptr(self.bias)
        if epi == EPI_F32_RESID_STATS:
            p.c16, p.stats_out = ptr(o["c16"]), ptr(o["stats"])
            if centred:
                st0, sh0 = self.centre()
                p.shift_in, p.shift_stats, p.shift_slots, p.shift_out = ptr(sh0), ptr(st0), 1, ptr(o["shift"])
        return p

    # ---- the same problem (first n rows) alone through the existing single-problem entry at a forced tile
    def alone(self, epi, tile, n=None, centred=True):
        from centerclip_amd import ops
        n = self.m if n is None else n
        o = {}
        if epi in (EPI_F16_LN, EPI_F16_GELU_LN):
            h16, st, wf, c1, c2 = self.ln()
            o["C"] = ops.linear_ln_f16(h16[:n], wf, c1, c2, st[:n], 1, gelu=epi == EPI_F16_GELU_LN, tile=tile)
        elif epi == EPI_F32_RESID_STATS:
            h = self.h0[:n].clone()
            kw = {}
            if centred:
                st0, sh0 = self.centre()
                kw = dict(shift_in=sh0[:n], stats_in=st0[:n].view(n, 1, 2))
            o["c16"], o["stats"], o["slots"], o["shift"] = ops.linear_resid_stats_f16(self.a[:n], self.w, self.bias, h, tile=tile, **kw)
            o["C"] = h
        elif epi == EPI_F32_RESID:
            o["C"] = ops.linear_f16(self.a[:n], self.w, self.bias, "f32_resid", out=self.h0[:n].clone(), tile=tile)
        else:
            o["C"] = ops.linear_f16(self.a[:n], self.w, self.bias, EPI_NAME[epi], tile=tile)
        return o


def launch(specs, epi, tile=0, rows=False, centred=True):
    """-> (status, [outputs per problem], [slots per problem], tile the launch ran or None)"""
    L, lib = _lib()
    outs = [s.outputs(epi, centred) for s in specs]
    ps = [s.struct(epi, o, centred) for s, o in zip(specs, outs)]
    p1 = ctypes.byref(ps[1]) if len(ps) > 1 else None
    slots = (ctypes.c_int32 * 2)()
    st = L.stream_ptr()
    if rows:
        rc = lib.cc_linear_rows_pair_f16(ctypes.byref(ps[0]), p1, epi, slots, st)
        torch.cuda.synchronize()
        return rc, outs, list(slots), None
    with timing() as t:
        rc = lib.cc_linear_pair_f16(ctypes.byref(ps[0]), p1, epi, tile, slots, st)
    if rc == 0:
        assert t.rec[4] == epi and t.rec[6:9] == [specs[0].M, specs[0].N, specs[0].K]
        assert t.rec[9:12] == ([specs[1].M, specs[1].N, specs[1].K] if len(specs) > 1 else [0, 0, 0])
    return rc, outs, list(slots), (t.tile if rc == 0 else None)


def nothing_written(spec, epi, o):
    """after a refused launch: every output is as it was allocated"""
    fresh = spec.outputs(epi)
    return all(same_bits(o[k], fresh[k]) for k in o)


TOL = {EPI_F16: 2e-3, EPI_F16_GELU: 2e-3, EPI_F32: 2e-4, EPI_F32_RESID: 2e-4, EPI_F16_LN: 3e-3, EPI_F16_GELU_LN: 3e-3,
       EPI_F32_RESID_STATS: 2e-4}


def check_problem(spec, epi, o, slots, want, worst, centred=True, tag=None):
    """one problem of a tile-kernel launch: its rows [0, m) equal `want` (the stand-alone run) bit for bit and float64 within
    the bound, everything else holds the sentinel"""
    m, N = spec.m, spec.N
    rows = list(range(m))
    assert same_bits(o["C"][:m], want["C"][:m]), tag
    e = relerr(o["C"][:m].float(), spec.ref(epi))
    worst[epi] = max(worst.get(epi, 0.0), e)
    assert e < TOL[epi], (tag, e)
    assert untouched(o["C"], rows), tag
    if epi != EPI_F32_RESID_STATS:
        return
    assert slots == want["slots"], (tag, slots, want["slots"])
    stats = o["stats"].view(-1)[:m * slots * 2].view(m, slots, 2)                      # the [M][slots][2] layout
    assert same_bits(stats, want["stats"][:m]), tag
    assert holds_sentinel(o["stats"].view(-1)[m * slots * 2:]), tag
    assert same_bits(o["c16"][:m], want["c16"][:m]) and untouched(o["c16"], rows), tag
    c16 = o["c16"][:m]
    s = stats.sum(1).double().cpu().numpy()
    np.testing.assert_allclose(s[:, 0], c16.double().sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[:, 1], (c16.double() ** 2).sum(-1).cpu().numpy(), rtol=1e-5)
    if centred:
        assert same_bits(o["shift"][:m, 0], want["shift"][:m]) and untouched(o["shift"], rows), tag
        assert torch.equal(c16, (o["C"][:m] - o["shift"][:m]).half()), tag
        assert float((o["shift"][:m, 0] - spec.h0[:m].mean(1)).abs().max()) <= 1e-3 * float(spec.h0[:m].abs().max()), tag
    else:
        assert torch.equal(c16, o["C"][:m].half()), tag


def tile_divides(tile, epi, specs):
    if tile == 7 and epi not in (EPI_F16, EPI_F16_GELU, EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32):
        return False
    return all(s.N % TILE_BN[tile] == 0 and s.K % (128 if tile == 8 else 64) == 0 for s in specs)


# ------------------------------------------------------------------------------------------------ a. pair = two stand-alone launches
# (carrier M, carrier K, rider M, rider N, rider K): every value of the issue's lists, the rider's K never the carrier's
PAIR_SHAPES = [(257, 64, 1, 512, 128), (300, 256, 65, 768, 64), (257, 768, 130, 512, 256), (300, 768, 1, 768, 192),
               (300, 64, 130, 768, 768), (257, 256, 65, 512, 768)]
_pair_specs = {}


def pair_specs(i):
    if i not in _pair_specs:
        cm, ck, rm, rn, rk = PAIR_SHAPES[i]
        _pair_specs[i] = (Spec(cm, 768, ck, 1000 + i), Spec(rm, rn, rk, 2000 + i))
    return _pair_specs[i]


@pytest.mark.parametrize("epi", [EPI_F16, EPI_F16_GELU, EPI_F32, EPI_F32_RESID, EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32_RESID_STATS])
def test_pair_equals_its_two_standalone_launches(epi):
    worst, ran = {}, set()
    for i in range(len(PAIR_SHAPES)):
        specs = pair_specs(i)
        for tile in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):
            rc, outs, slots, t = launch(specs, epi, tile)
            tag = (PAIR_SHAPES[i], epi, tile)
            if tile and not tile_divides(tile, epi, specs):
                assert rc == -1, tag                                   # e.g. tile 7 with N = 512, tile 8 with K = 192
                assert all(nothing_written(s, epi, o) for s, o in zip(specs, outs)), tag
                continue
            assert rc == 0, tag
            assert t == tile or tile == 0, tag
            ran.add(t)
            for s, o, sl in zip(specs, outs, slots):
                check_problem(s, epi, o, sl, s.alone(epi, t), worst, tag=tag)
    assert {1, 2, 3, 4, 5, 6, 8, 10} <= ran
    print("group a, epilogue %d: worst error vs float64 %.3g (bound %.0e)" % (epi, worst[epi], TOL[epi]))


# ------------------------------------------------------------------------------------------------ b. the automatic fallback
@pytest.mark.parametrize("carrier,rider,first,fallback", [((9600, 2304, 768), (130, 512, 256), 7, 1),
                                                          ((300, 768, 768), (65, 768, 192), 8, 4)])
def test_auto_tile_falls_back_to_one_that_divides_the_rider(carrier, rider, first, fallback):
    _, lib = _lib()
    epi = EPI_F16
    assert lib.cc_linear_tile_for(*carrier, epi) == first                             # the carrier alone would take this tile ...
    assert rider[1] % TILE_BN[first] or rider[2] % (128 if first == 8 else 64)         # ... which does not divide the rider
    specs = (Spec(*carrier, 31), Spec(*rider, 32))
    rc, outs, slots, t = launch(specs, epi, 0)
    assert rc == 0 and t == fallback, (rc, t)
    worst = {}
    for s, o in zip(specs, outs):
        check_problem(s, epi, o, 0, s.alone(epi, fallback), worst)
    print("group b, carrier %s: ran tile %d, worst error vs float64 %.3g (bound %.0e)" % (carrier, t, worst[epi], TOL[epi]))


# ------------------------------------------------------------------------------------------------ c. device-side row count
@pytest.mark.parametrize("epi", [EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32_RESID, EPI_F32_RESID_STATS])
@pytest.mark.parametrize("on_rider", [True, False])
def test_device_side_row_count(epi, on_rider):
    worst = {}
    cshape, rshape = (300, 768, 256), (130, 512, 128)
    for m in (1, 64, 65, None):
        carrier = Spec(*cshape, 41, m=None if on_rider else (m or cshape[0]))
        rider = Spec(*rshape, 42, m=(m or rshape[0]) if on_rider else None)
        for tile in (0, 1, 4, 6):
            if tile and not tile_divides(tile, epi, (carrier, rider)):
                continue
            rc, outs, slots, t = launch((carrier, rider), epi, tile)
            tag = (epi, on_rider, m, tile)
            assert rc == 0, tag
            for s, o, sl in zip((carrier, rider), outs, slots):
                # rows < m: the run with M = m, bit for bit; rows >= m of every output: the sentinel (check_problem)
                check_problem(s, epi, o, sl, s.alone(epi, t, n=s.m), worst, tag=tag)
    print("group c, epilogue %d, m_dev on the %s: worst error vs float64 %.3g (bound %.0e)"
          % (epi, "rider" if on_rider else "carrier", worst[epi], TOL[epi]))


# ------------------------------------------------------------------------------------------------ d. the few-rows kernel
def rows_spec(M, N, K, addr, seed, ratio=0.0):
    if addr == "map":
        R = 3 * M + 5
        rows = torch.randperm(R, generator=torch.Generator().manual_seed(seed))[:M].tolist()       # distinct, in no order
        s = Spec(M, N, K, seed, rows=rows, R=R, ratio=ratio)
        s.row_map = torch.tensor(rows, dtype=torch.int32, device=DEV)
    else:
        s = Spec(M, N, K, seed, rows=[i * addr for i in range(M)], R=(M - 1) * addr + 2, ratio=ratio)
        s.row_step = 0 if addr == 1 and seed % 2 else addr                                           # 0 means 1
    return s


def check_rows_problem(s, epi, o, slots, worst, tag):
    """-> nothing; float64 on the selected rows, the sentinel everywhere else"""
    r = s.sel()
    tol = 3e-3 if epi == EPI_F16_GELU_LN else 2e-4
    e = relerr(o["C"][r].float(), s.ref(epi))
    worst["f64"] = max(worst.get("f64", 0.0), e)
    assert e < tol, (tag, e)
    assert untouched(o["C"], s.prow), tag
    if epi != EPI_F32_RESID_STATS:
        return
    assert slots == s.N // 32, tag
    assert untouched(o["c16"], s.prow) and untouched(o["shift"], s.prow), tag
    stats = o["stats"].view(-1)[:s.R * slots * 2].view(s.R, slots, 2)                   # [physical row][N / 32][2]
    assert untouched(stats, s.prow) and holds_sentinel(o["stats"].view(-1)[s.R * slots * 2:]), tag
    c16, shift = o["c16"][r], o["shift"][r]
    assert torch.equal(c16, (o["C"][r] - shift).half()), tag
    assert float((shift[:, 0] - s.h0[r].mean(1)).abs().max()) <= 1e-3 * float(s.h0[r].abs().max()), tag
    # slot cb holds the sums of columns [32 cb, 32 cb + 32) of the centred copy
    blk = c16.double().view(len(r), slots, 32)
    np.testing.assert_allclose(stats[r][:, :, 0].double().cpu().numpy(), blk.sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(stats[r][:, :, 1].double().cpu().numpy(), (blk ** 2).sum(-1).cpu().numpy(), rtol=1e-5)


def all_rows_tile_kernel(s, epi):
    """the tile kernel on ALL physical rows of the same inputs -> its outputs"""
    full = Spec.__new__(Spec)
    full.__dict__.update(s.__dict__)
    full.M = full.m = s.R
    full.prow, full.row_step, full.row_map, full.m_dev = list(range(s.R)), 0, None, None
    return full.alone(epi, 0)


ROWS_CASES = [(1, 32, 1), (48, 768, 50), (64, 64, "map"), (65, 1024, 197), (130, 768, "map"), (130, 32, 50), (1, 1024, "map"),
              (48, 64, 197), (64, 768, 1), (65, 64, 50), (130, 1024, 1), (48, 32, "map")]


@pytest.mark.parametrize("epi", [EPI_F16_GELU_LN, EPI_F32_RESID, EPI_F32_RESID_STATS])
@pytest.mark.parametrize("K", [32, 64, 288, 768, 800, 3072])
def test_few_rows_kernel(K, epi):
    """K = 32 / 64: waves without work; 288 = 9 k-steps: a ragged last wave; 768 / 800: a partial last batch of three
    k-steps; 3072 = 12 k-steps per wave: four batches."""
    worst = {}
    for c, (M, N, addr) in enumerate(ROWS_CASES):
        s = rows_spec(M, N, K, addr, 5000 + 13 * c + K, ratio=10.0 if c % 2 else 0.0)
        tag = (M, N, K, addr, epi)
        rc, (o,), slots, _ = launch((s,), epi, rows=True)
        assert rc == 0, tag
        check_rows_problem(s, epi, o, slots[0], worst, tag)
        if N % 64 == 0 and K % 64 == 0:                     # the all-rows kernel takes this shape: same inputs, all rows
            want, r = all_rows_tile_kernel(s, epi), s.sel()
            e = relerr(o["C"][r].float(), want["C"][r].float())
            worst["tile"] = max(worst.get("tile", 0.0), e)
            assert e < (3e-3 if epi == EPI_F16_GELU_LN else 2e-4), (tag, e)
            if epi == EPI_F32_RESID_STATS:
                e = relerr(o["c16"][r].float(), want["c16"][r].float())
                worst["tile16"] = max(worst.get("tile16", 0.0), e)
                assert e < 3e-3, (tag, e)
                assert float((o["shift"][r, 0] - want["shift"][r]).abs().max()) <= 1e-3 * float(s.h0[r].abs().max()), tag
    print("group d, epilogue %d, K = %d: worst error vs float64 %.3g (bound %.0e), vs the all-rows kernel %.3g fp32/LN "
          "(bound %.0e) %.3g fp16 copy (bound 3e-03)" % (epi, K, worst["f64"], 3e-3 if epi == EPI_F16_GELU_LN else 2e-4,
                                                         worst.get("tile", 0.0), 3e-3 if epi == EPI_F16_GELU_LN else 2e-4,
                                                         worst.get("tile16", 0.0)))


@pytest.mark.parametrize("epi", [EPI_F16_GELU_LN, EPI_F32_RESID, EPI_F32_RESID_STATS])
def test_few_rows_pair_equals_two_single_launches(epi):
    a, b = rows_spec(65, 768, 288, 50, 61, ratio=10.0), rows_spec(48, 64, 800, "map", 62)
    rc, outs, slots, _ = launch((a, b), epi, rows=True)
    assert rc == 0
    worst = {}
    for s, o, sl in zip((a, b), outs, slots):
        rc1, (o1,), sl1, _ = launch((s,), epi, rows=True)
        assert rc1 == 0 and sl == sl1[0]
        assert all(same_bits(o[k], o1[k]) for k in o), epi
        check_rows_problem(s, epi, o, sl, worst, (s.M, s.N, s.K, epi))


def test_few_rows_last_block_tail_as_a_chain():
    """out_proj (statistics + centring shift) -> c_fc (LN-folded QuickGELU reading those N / 32 slots) -> c_proj on the CLS
    rows of 48 frames of 50 tokens, rows with |mean| = 10 sigma, against float64 h += ...; LN; GELU; h += ... on those rows."""
    from centerclip_amd import ops
    L, lib = _lib()
    W, Mr, step = 768, 48, 50
    s = rows_spec(Mr, W, W, step, 71, ratio=10.0)                              # a = attention rows, w / bias = out_proj, h0
    gen = torch.Generator(device=DEV).manual_seed(72)
    gamma, beta = torch.rand(W, generator=gen, device=DEV) + 0.5, randn(gen, W, scale=0.2)
    w2, b2 = randn(gen, 4 * W, W, scale=W ** -0.5), randn(gen, 4 * W, scale=0.1)
    w3, b3 = randn(gen, W, 4 * W, scale=(4 * W) ** -0.5).half(), randn(gen, W, scale=0.1)
    r = s.sel()
    h1 = s.ref(EPI_F32_RESID_STATS)
    pre = F.layer_norm(h1, (W,), gamma.double(), beta.double(), 1e-5) @ w2.double().t() + b2.double()
    y = pre * torch.sigmoid(1.702 * pre)
    h2 = h1 + y @ w3.double().t() + b3.double()
    # out_proj
    rc, (o,), slots, _ = launch((s,), EPI_F32_RESID_STATS, rows=True)
    assert rc == 0 and slots[0] == W // 32
    e1 = relerr(o["C"][r], h1)
    # c_fc on the same physical rows, reading the N / 32 slots out_proj wrote
    wf, c1, c2 = ops.fold_layernorm_linear(w2, b2, gamma, beta)
    y16 = sentinel(s.R + GUARD, 4 * W, torch.float16)
    p = L.LinearProblem(a=ptr(o["c16"]), w=ptr(wf), bias=ptr(c2), c=ptr(y16), M=Mr, N=4 * W, K=W, ldc=4 * W, ln_stats=ptr(o["stats"]),
                        ln_slots=slots[0], ln_c1=ptr(c1), ln_eps=1e-5, row_step=step)
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(p), None, EPI_F16_GELU_LN, None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    e2 = relerr(y16[r].float(), y)
    assert untouched(y16, s.prow)
    # c_proj, in place on the fp32 rows
    p = L.LinearProblem(a=ptr(y16), w=ptr(w3), bias=ptr(b3), c=ptr(o["C"]), M=Mr, N=W, K=4 * W, ldc=W, row_step=step)
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(p), None, EPI_F32_RESID, None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    e3 = relerr(o["C"][r], h2)
    assert untouched(o["C"], s.prow)
    print("group d, chain: out_proj %.3g (bound 2e-04), c_fc %.3g (bound 3e-03), c_proj %.3g (bound 2e-04)" % (e1, e2, e3))
    assert e1 < 2e-4 and e2 < 3e-3 and e3 < 2e-4


def test_few_rows_refusals():
    L, lib = _lib()
    for N, K in ((48, 64), (64, 48)):                                          # N % 32, K % 32
        for epi in (EPI_F16_GELU_LN, EPI_F32_RESID, EPI_F32_RESID_STATS):
            s = rows_spec(4, N, K, 1, 81)
            z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=DEV)
            s._ln = (z(s.R, K, dt=torch.float16), z(s.R, 2), z(N, K, dt=torch.float16), z(N), z(N))
            s._centre = (z(s.R, 2), z(s.R))
            rc, (o,), _, _ = launch((s,), epi, rows=True)
            assert rc == -2 and nothing_written(s, epi, o), (N, K, epi)
    s = rows_spec(3, 1056, 64, 50, 82)
    rc, (o,), _, _ = launch((s,), EPI_F32_RESID_STATS, rows=True)              # 33 slots per row: not supported ...
    assert rc == -2 and nothing_written(s, EPI_F32_RESID_STATS, o)
    rc, (o,), _, _ = launch((s,), EPI_F32_RESID, rows=True)                    # ... the plain residual add is
    assert rc == 0 and relerr(o["C"][s.sel()], s.ref(EPI_F32_RESID)) < 2e-4 and untouched(o["C"], s.prow)
    s = rows_spec(4, 64, 64, 1, 83)
    for epi in (EPI_F16, EPI_F16_GELU, EPI_F32, EPI_F16_LN):                  # epilogues the kernel does not have
        rc, (o,), _, _ = launch((s,), epi, rows=True)
        assert rc == -2 and nothing_written(s, epi, o), epi
    o = s.outputs(EPI_F32_RESID)
    p = s.struct(EPI_F32_RESID, o)
    for M in (0, -3):                                                          # M <= 0
        p.M = M
        assert lib.cc_linear_rows_pair_f16(ctypes.byref(p), None, EPI_F32_RESID, None, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert nothing_written(s, EPI_F32_RESID, o)


# ------------------------------------------------------------------------------------------------ e. the patch embedding's epilogue
@pytest.mark.parametrize("N", [128, 768])
@pytest.mark.parametrize("K", [192, 640])
@pytest.mark.parametrize("Fr,n", [(3, 4), (6, 49), (2, 196)])
def test_patch_embedding_epilogue(Fr, n, N, K):
    """out row f (n + 1) + 1 + i = patch row (f n + i) of a w^T + bias + pos[1 + i]; the class-token rows f (n + 1) are not
    written.  (6, 49): 294 patch rows, ragged over 256, frame boundaries inside and across row tiles."""
    L, lib = _lib()
    M = Fr * n
    gen = torch.Generator(device=DEV).manual_seed(Fr * 1000 + n + N + K)
    a, w = randn(gen, M, K).half(), randn(gen, N, K, scale=K ** -0.5).half()
    bias = randn(gen, N, scale=0.5) if (Fr + N // 128) % 2 else None          # conv1 has no bias: both forms
    pos = randn(gen, n + 1, N, scale=0.7)
    ref = a.double() @ w.double().t() + (bias.double() if bias is not None else 0.0)
    ref = (ref.view(Fr, n, N) + pos[1:].double()).reshape(M, N)
    out_rows = [f * (n + 1) + 1 + i for f in range(Fr) for i in range(n)]
    first, worst = None, 0.0
    for tile in (0, 1, 4, 5, 6, 10):
        out = sentinel(Fr * (n + 1) + GUARD, N, torch.float32)
        p = L.LinearProblem(a=ptr(a), w=ptr(w), bias=ptr(bias), c=ptr(out), M=M, N=N, K=K, ldc=N, pos=ptr(pos), patch_n=n)
        with timing() as t:
            rc = lib.cc_linear_pair_f16(ctypes.byref(p), None, EPI_F32_PATCH, tile, None, L.stream_ptr())
        if tile and N % TILE_BN[tile]:
            assert rc == -1 and holds_sentinel(out), tile
            continue
        assert rc == 0 and (tile == 0 or t.tile == tile) and t.rec[4] == EPI_F32_PATCH, (tile, rc, t.rec)
        got = out[torch.as_tensor(out_rows, device=DEV)]
        e = relerr(got, ref)
        worst = max(worst, e)
        assert e < 2e-4, (tile, e)
        assert untouched(out, out_rows), tile                                  # class-token rows and the guard
        first = out if first is None else first
        assert same_bits(out, first), tile                                     # one k order: the same bits on every tile
    print("group e, F %d n %d N %d K %d: worst error vs float64 %.3g (bound 2e-04)" % (Fr, n, N, K, worst))


# ------------------------------------------------------------------------------------------------ f. in_proj + attention with a rider
def attn_inputs(M, W, seed):
    from centerclip_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = randn(g, M, W, scale=1.5, shift=0.3)
    w, b = randn(g, 3 * W, W, scale=0.04), randn(g, 3 * W, scale=0.1)
    gamma, beta = 1.0 + 0.1 * randn(g, W), 0.1 * randn(g, W)
    h16, st, _ = ops.row_stats(x)
    wf, c1, c2 = ops.fold_layernorm_linear(w, b, gamma, beta)
    return h16, st.contiguous(), wf, c1, c2


def attn_ref(qkv, off, lens, heads, causal):
    """float64 softmax(q k^T / 8 [+ causal mask]) v per sequence on the fp16 q, k, v -> {first row: [len, W]}"""
    W, out = heads * 64, {}
    for o, n in zip(off, lens):
        q, k, v = (t.view(n, heads, 64).permute(1, 0, 2) for t in qkv[o:o + n].double().split(W, dim=1))
        sc = q @ k.transpose(-1, -2) / 8.0
        if causal:
            sc = sc + torch.full((n, n), float("-inf"), device=DEV, dtype=torch.float64).triu(1)
        out[o] = (sc.softmax(-1) @ v).permute(1, 0, 2).reshape(n, W)
    return out


# (carrier nseq, L, heads, rider bound L, rider heads, row-tile height the cost rule gives): together all three heights
ATTN_CASES = [(24, 50, 2, 32, 1, 192), (24, 50, 2, 77, 3, 192), (3, 197, 2, 32, 3, 224), (3, 197, 2, 77, 1, 224),
              (5, 256, 1, 77, 2, 256), (5, 256, 1, 32, 2, 256)]
assert {c[5] for c in ATTN_CASES} == {192, 224, 256}


@pytest.mark.parametrize("nseq,L,heads,Lr,rheads,height", ATTN_CASES)
def test_inproj_attention_with_a_rider(nseq, L, heads, Lr, rheads, height):
    """A ViT carrier and 8 causal captions packed back to back (seq_off / seq_len / m_dev) in one launch; the row-tile
    height is chosen over both problems and read from the timing record (192 / 224 / 256 rows: ATTN_CASES has all three)."""
    from centerclip_amd import ops
    Lb, lib = _lib()
    W, Wr = heads * 64, rheads * 64
    lens = [Lr, 1, Lr // 2 + 1, 5, Lr - 1, 20, 9, Lr] if Lr == 32 else [77, 1, 40, 5, 76, 20, 65, 33]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    total, Mr, M = int(sum(lens)), 8 * Lr, nseq * L
    ch, rh = attn_inputs(M, W, 900 + L), attn_inputs(Mr, Wr, 950 + Lr)
    seq_off, seq_len = torch.from_numpy(off).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    m_dev = torch.tensor([total], dtype=torch.int32, device=DEV)
    oc, orr = sentinel(M + GUARD, W, torch.float16), sentinel(Mr + GUARD, Wr, torch.float16)

    def prob(h, out, rows, width, Ltok, ns, causal, **kw):
        h16, st, wf, c1, c2 = h
        return Lb.LinearProblem(a=ptr(h16), w=ptr(wf), bias=ptr(c2), c=ptr(out), M=rows, N=3 * width, K=width, ldc=width,
                                ln_stats=ptr(st), ln_slots=1, ln_c1=ptr(c1), ln_eps=1e-5, att_L=Ltok, att_nseq=ns,
                                att_causal=int(causal), **kw)
    p0 = prob(ch, oc, M, W, L, nseq, False)
    p1 = prob(rh, orr, Mr, Wr, Lr, 8, True, att_seq_off=ptr(seq_off), att_seq_len=ptr(seq_len), m_dev=ptr(m_dev))
    with timing() as t:
        rc = lib.cc_inproj_attention_pair_f16(ctypes.byref(p0), ctypes.byref(p1), Lb.stream_ptr())
    assert rc == 0
    assert t.rec[0] == height and t.rec[4] == 8 and t.rec[6:] == [M, 3 * W, W, Mr, 3 * Wr, Wr], t.rec
    # the sentinel: guard rows of the carrier; rows behind the packed captions (= behind m_dev) and the guard of the rider
    assert untouched(oc, range(M)) and untouched(orr, range(total))
    assert torch.isfinite(oc[:M].float()).all() and torch.isfinite(orr[:total].float()).all()
    if L <= 56 and Lr <= 56:                                                   # both sides: the stand-alone entry's bits
        h16, st, wf, c1, c2 = ch
        assert torch.equal(oc[:M], ops.inproj_attention_f16(h16, wf, c1, c2, st, 1, nseq, L, heads, causal=False))
        h16, st, wf, c1, c2 = rh
        alone = ops.inproj_attention_f16(h16, wf, c1, c2, st, 1, 8, Lr, rheads, causal=True, seq_off=seq_off, seq_len=seq_len)
        assert torch.equal(orr[:total], alone[:total])
    # float64 on the fp16 q, k, v of the same inputs, at the one-launch tests' bound
    worst = 0.0
    for (h16, st, wf, c1, c2), out, o_, l_, hd, causal in ((ch, oc, [i * L for i in range(nseq)], [L] * nseq, heads, False),
                                                           (rh, orr, off.tolist(), lens, rheads, True)):
        ref = attn_ref(ops.linear_ln_f16(h16, wf, c1, c2, st, 1), o_, l_, hd, causal)
        scale = max(float(r.abs().max()) for r in ref.values())
        for o, r in ref.items():
            e = float((out[o:o + len(r)].double() - r).abs().max()) / max(scale, 1e-3)
            worst = max(worst, e)
            assert e <= 2e-3, (o, len(r), e)
    print("group f, carrier (%d, %d, %d) rider L %d: %d-row tiles, worst error vs float64 %.3g (bound 2e-03)"
          % (nseq, L, heads, Lr, t.rec[0], worst))
