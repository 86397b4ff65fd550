"""CPU-only half of the weight-gradient tests (csrc/wgrad.hip); the launches are in tests/test_wgrad_gpu.py.

  * the slice count of every case of tests/wgrad_ref.py as the library reports it, and the property the case is listed for
    (depth, tail length, a short last slice, empty slices, a one-slice group in the reduce) derived from that count - a plan
    change that takes a property away fails here, on a machine without a device;
  * the emulation of the documented work split equals the exact product on every lattice case, and every mutant of it - a
    defect the kernel could have - is rejected by the case the table names for it;
  * the gap this closes: a tail boundary that is wrong for one fragment entry gives the very same result as the correct one
    at the row counts the older test runs (77 and 200: tails 13 and 8) and passes its max-norm measure there;
  * the status of every early return of cc_wgrad_tn_f16 that precedes the first HIP call.
"""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_ref as wr

CC_ERR_INVALID, CC_ERR_UNSUPPORTED, CC_ERR_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from centerclip_amd import build
    build.build(verbose=False)
    from centerclip_amd import _lib as L
    return L.lib()


def _slices(lib, c):
    return wr.slices_from_workspace_bytes(lib.cc_wgrad_tn_workspace_bytes(c.M, c.N1, c.N2), c.N1, c.N2)


# ---------------------------------------------------------------------------------------------------- (a) the plan

def test_every_case_has_the_property_it_is_listed_for(lib):
    seen_nk = set()
    for group, cases in wr.GROUPS.items():
        for c in cases:
            p = wr.properties(c.M, _slices(lib, c))
            for key, want in c.want.items():
                assert p[key] == want, (group, wr.case_id(c), key, p[key], want)
            seen_nk.update(n for n in p["nks"] if n > 0)
            if p["empty"]:
                rps, sl = wr.plan(c.M, p["S"])
                assert all(sl[i][0] > c.M and sl[i][2] <= 0 for i in p["empty"])          # m_begin > M, no stage
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9} <= seen_nk
    assert sorted(c.want["tail"] for c in wr.TAIL) == list(range(1, 32))
    assert sorted(c.want["nk"] for c in wr.DEPTH) == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 8]
    assert {c.want["tail"] for c in wr.DEPTH} == {1, 31, 32}
    assert [c.want["chunks"] for c in wr.BIAS_ONE] == [1, 1, 1, 2, 8, 9, 16]
    assert sum(1 for c in wr.SLICES if c.want.get("single_group")) == 3
    assert all(c.M <= 2 ** 20 for c in wr.LATTICE_CASES)                                   # 16 M < 2^24: fp32 sums are exact


# ---------------------------------------------------------------------------------------------------- (b) emulation, mutants

@pytest.fixture(scope="module")
def lattice_runs(lib):
    """(case, S, dY, X, exact / 8 as fp32) per lattice case; computed once, never modified."""
    runs = {}
    for c in wr.LATTICE_CASES:
        dy, x = wr.lattice(c)
        ref = wr.exact(dy, x, 8.0)
        ref32 = ref.astype(np.float32)
        assert np.array_equal(ref32.astype(np.float64), ref)
        runs[wr.case_id(c)] = (_slices(lib, c), dy, x, ref32)
    return runs


def test_references_agree_on_a_lattice():
    for c in (wr.DEPTH[3], wr.PLACEMENT[3], wr.SLICES[0]):
        dy, x = wr.lattice(c)
        assert float(np.abs(dy.astype(np.float64)).max()) == 4.0 and not (dy == 0).any() and not (x == 0).any()
        assert np.array_equal(wr.exact(dy, x), wr.exact_int(dy, x).astype(np.float64))
    dy, x = wr.lattice(wr.PLACEMENT[3])
    assert not np.array_equal(dy, x)


def test_emulation_is_exact_on_every_lattice_case(lattice_runs):
    for name, (S, dy, x, ref32) in lattice_runs.items():
        assert np.array_equal(wr.emulate(dy, x, S, 8.0), ref32), name


def test_bias_emulation_is_exact_on_every_chunk_count():
    for c in wr.BIAS_ONE + wr.BIAS_SLICED:
        dy32 = wr.lattice(c)[0].astype(np.float32)
        assert np.array_equal(wr.bias_emulate(dy32), dy32.astype(np.float64).sum(0).astype(np.float32)), wr.case_id(c)


@pytest.mark.parametrize("mutant", sorted(wr.MUTANTS))
def test_every_mutant_is_rejected_by_its_named_case(lattice_runs, mutant):
    for c in wr.MUTANTS[mutant]:
        if mutant == "bias_segment_off_by_one":
            dy32 = wr.lattice(c)[0].astype(np.float32)
            assert not np.array_equal(wr.bias_emulate(dy32, mutant), wr.bias_emulate(dy32)), wr.case_id(c)
            continue
        S, dy, x, ref32 = lattice_runs[wr.case_id(c)]
        assert not np.array_equal(wr.emulate(dy, x, S, 8.0, mutant), ref32), wr.case_id(c)


@pytest.mark.parametrize("M,N1,N2", [(77, 384, 128), (200, 128, 256)])
def test_one_entry_tail_mutant_passes_the_older_measure(M, N1, N2, monkeypatch):
    """The operands and the measure of test_weight_gradient_without_transposed_copies at its two small row counts.  The tail
    boundary wrong for the entry of row 17 only: the same bits as the correct split (tails 13 and 8 never ask about row 17), so
    it passes; the measure itself is not blind - the same defect at the entry a tail of 13 or 8 does ask about fails it."""
    g = torch.Generator().manual_seed(M + 3 * N1 + 7 * N2)
    dy = torch.randn(M, N1, generator=g).half().numpy()
    x = torch.randn(M, N2, generator=g).half().numpy()
    ref = wr.exact(dy, x, 8.0)
    good = wr.emulate(dy, x, 1, 8.0)
    bad = wr.emulate(dy, x, 1, 8.0, "tail_boundary_off_by_one")
    err, allowed = wr.existing_max_norm_measure(bad, ref, M)
    assert np.array_equal(bad, good) and err <= allowed
    tail = M - (M - 1) // 32 * 32
    assert tail != wr.OFF_BY_ONE_ROW
    monkeypatch.setattr(wr, "OFF_BY_ONE_ROW", tail)
    err, allowed = wr.existing_max_norm_measure(wr.emulate(dy, x, 1, 8.0, "tail_boundary_off_by_one"), ref, M)
    assert err > allowed


def test_one_entry_tail_mutant_for_every_row_needs_its_own_tail(lattice_runs, monkeypatch):
    """Entry r of the clear is asked about by the tail of r rows alone: the 31 tails of the table are all needed."""
    for r in (1, 8, 13, 16, 17, 31):
        monkeypatch.setattr(wr, "OFF_BY_ONE_ROW", r)
        rejecting = []
        for c in wr.TAIL:
            _, dy, x, ref32 = lattice_runs[wr.case_id(c)]
            if not np.array_equal(wr.emulate(dy, x, 1, 8.0, "tail_boundary_off_by_one"), ref32):
                rejecting.append(c.want["tail"])
        assert rejecting == [r]


# ---------------------------------------------------------------------------------------------------- (c) early returns

# Pointers that are only tested against NULL point into this host buffer; no case below reaches a launch.
_BUF = (ctypes.c_char * 4096)()
PTR = ctypes.c_void_p(ctypes.addressof(_BUF))


def _call(lib, dy=PTR, x=PTR, dw=PTR, M=257, N1=128, N2=128, scale=None, part=None, chunks=0, db=None, ws=PTR, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cc_wgrad_tn_workspace_bytes(M, N1, N2)
    return lib.cc_wgrad_tn_f16(dy, x, dw, M, N1, N2, scale, part, chunks, db, ws, ws_bytes, None)


def test_early_returns(lib):
    for kw in ({"dy": None}, {"x": None}, {"dw": None}, {"M": 0}, {"M": -5}, {"N1": 0}, {"N2": 0}, {"N1": -128}, {"N2": -128}):
        assert _call(lib, ws_bytes=1 << 30, **kw) == CC_ERR_INVALID, kw
    for kw in ({"N1": 64}, {"N2": 192}, {"N1": 129}, {"N2": 127}, {"N1": 100, "N2": 100}):
        assert _call(lib, ws_bytes=1 << 30, **kw) == CC_ERR_UNSUPPORTED, kw
        assert lib.cc_wgrad_tn_workspace_bytes(257, kw.get("N1", 128), kw.get("N2", 128)) == 0
    assert lib.cc_wgrad_tn_workspace_bytes(0, 128, 128) == 0 and lib.cc_wgrad_tn_workspace_bytes(257, -128, 128) == 0
    assert _call(lib, part=PTR, chunks=5) == CC_ERR_INVALID                                # col_partial without bias_grad
    assert _call(lib, db=PTR, chunks=5) == CC_ERR_INVALID                                  # ... and the reverse
    assert _call(lib, part=PTR, db=PTR, chunks=0) == CC_ERR_INVALID
    assert _call(lib, part=PTR, db=PTR, chunks=-1) == CC_ERR_INVALID
    for M in (200, 257, 9600):                                                             # S = 1 (256 bytes) and S > 1
        need = lib.cc_wgrad_tn_workspace_bytes(M, 128, 128)
        assert need == (256 if M == 200 else _slices(lib, wr.Case(128, 128, M, {})) * 128 * 128 * 4)
        assert _call(lib, M=M, ws_bytes=need - 1) == CC_ERR_WORKSPACE
        assert _call(lib, M=M, ws=None) == CC_ERR_WORKSPACE
        assert _call(lib, M=M, part=PTR, db=PTR, chunks=4, ws_bytes=need - 1) == CC_ERR_WORKSPACE
