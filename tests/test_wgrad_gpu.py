"""cc_wgrad_tn_f16 (csrc/wgrad.hip) on the MI355X (``-m gpu``) at every pipeline depth, tail and slice plan of the case table
in tests/wgrad_ref.py (tests/test_wgrad_host.py holds each case to the property it is listed for).

  * integer lattices: dY and X hold integers of magnitude <= 4, so every product and partial sum is an integer below 2^24 and
    the fp32 result is exact in any summation order - dW must EQUAL the float64 product, no tolerance; any dropped, doubled
    or misplaced row, column or slice fails;
  * the same one step upstream: an integer-valued fp32 dY through cc_cast_transpose_f16's device-chosen power-of-two scale
    and its partial column sums - dW and the bias gradient exact, with 1 .. 16 chunks and one slice (no slice blocks in the
    reduce launch) and with S > 1;
  * float operands (a heavy-tailed gradient against outlier channels; cancelling row pairs) element by element inside
    M 2^-24 (|dY|^T |X|) / scale of float64 on the same fp16 operands.
"""
import numpy as np
import pytest
import torch

import wgrad_ref as wr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _wgrad(dy16, x16, scale):
    """train._wgrad_tn, or the same call with a NULL scale_dev (scale None)."""
    from centerclip_amd import _lib as L, train
    if scale is not None:
        return train._wgrad_tn(dy16, x16, torch.tensor([scale], device=DEV, dtype=torch.float32))
    M, N1 = dy16.shape
    N2 = x16.shape[1]
    lib = L.lib()
    dw = torch.empty(N1, N2, device=DEV, dtype=torch.float32)
    ws = L.workspace(lib.cc_wgrad_tn_workspace_bytes(M, N1, N2), dy16.device)
    L.check(lib.cc_wgrad_tn_f16(L.ptr(dy16), L.ptr(x16), L.ptr(dw), M, N1, N2, None, None, 0, None, L.ptr(ws), ws.numel(),
                                L.stream_ptr(dy16.device)), "cc_wgrad_tn_f16")
    return dw


def _exact32(dy16, x16, scale):
    """The float64 product of the operands, divided by the (power-of-two) scale, as fp32 - checked to be exact there."""
    ref = dy16.double().t() @ x16.double()
    if scale is not None:
        ref = ref / scale
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref)
    return ref32


def _lattice_case(c, scale=8.0, twice=False):
    dy, x = (_dev(a) for a in wr.lattice(c))
    dw = _wgrad(dy, x, scale)
    ref = _exact32(dy, x, scale)
    wrong = int((dw != ref).sum())
    assert wrong == 0, "%s: %d of %d entries differ, first at %s" % (wr.case_id(c), wrong, ref.numel(),
                                                                      (dw != ref).nonzero()[0].tolist())
    assert torch.equal(dw, ref)
    if twice:
        assert torch.equal(_wgrad(dy, x, scale), dw)


# ---------------------------------------------------------------------------------------------------- lattices

@pytest.mark.parametrize("c", wr.DEPTH, ids=wr.case_id)
def test_pipeline_depth(c):
    """One slice of 1 .. 8 stages (the prologue's and the loop's branches, the ring's wrap), last stage full or of one row."""
    _lattice_case(c)


def test_every_tail_length():
    """96 + t rows, t = 1 .. 31: the fourth stage is the tail; each t asks about another entry of the register clear."""
    for c in wr.TAIL:
        _lattice_case(c)


@pytest.mark.parametrize("c", wr.PLACEMENT, ids=wr.case_id)
def test_tile_placement(c):
    """More tiles along N1 than N2, the reverse, and a square grid with dY != X."""
    _lattice_case(c)


@pytest.mark.parametrize("c", wr.SLICES, ids=wr.case_id)
def test_slice_plans(c):
    """S > 1: a short last slice, a last slice of one row in a reduce group of its own (S = 9, 17, 25), empty slices behind
    the last row (they must add a zero tile), and two shipped shapes - exact, and the same bits on a second call."""
    _lattice_case(c, twice=True)


@pytest.mark.parametrize("c", wr.SCALE, ids=wr.case_id)
def test_scales(c):
    """scale_dev 2^-20, 1, 8, 2^100 and NULL: the division by a power of two is exact in the tile store (S = 1) and in the
    reduce (S > 1)."""
    for scale in wr.SCALES:
        _lattice_case(c, scale=scale)


@pytest.mark.parametrize("c", wr.BIAS_ONE + wr.BIAS_SLICED, ids=wr.case_id)
def test_cast_scale_and_bias_fold_are_exact(c):
    """fp32 integers -> cc_cast_transpose_f16 (device-chosen scale, partial column sums per 64 rows) -> cc_wgrad_tn_f16:
    the scale is a power of two and the fp16 copy is dY times it; dW == dY^T X and the bias gradient == the column sums."""
    from centerclip_amd import train
    dy16_host, x_host = wr.lattice(c)
    dy32, x16 = _dev(dy16_host.astype(np.float32)), _dev(x_host)
    dy16, _, scale, part = train._cast_transpose(dy32, scaled=True, col_sums=True, want_t=False, col_partials=True)
    s = float(scale)
    assert wr.is_power_of_two(s) and part.shape == (c.want["chunks"], c.N1)
    assert torch.equal(dy16.double(), dy32.double() * s)
    dw, db = train._wgrad_tn(dy16, x16, scale, col_partial=part)
    assert torch.equal(dw, _exact32(dy32, x16, None))
    assert torch.equal(db.double(), dy32.double().sum(0))
    dw2, db2 = train._wgrad_tn(dy16, x16, scale, col_partial=part)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


# ---------------------------------------------------------------------------------------------------- floats, per element

def _share(dw, dy16, x16, scale):
    ref = (dy16.double().t() @ x16.double()) / scale
    bnd = dy16.shape[0] * wr.U * (dy16.double().abs().t() @ x16.double().abs()) / scale
    assert bool((bnd > 0).all())
    return float(((dw.double() - ref).abs() / bnd).max()), float(ref.abs().max() / (bnd / (dy16.shape[0] * wr.U)).max())


@pytest.mark.parametrize("c", wr.FLOAT, ids=wr.case_id)
def test_heavy_tailed_gradient_against_outlier_channels(c):
    """Recipe one (wgrad_ref.heavy_tailed): dY is the fp16 copy cc_cast_transpose_f16 makes.  Largest share of the bound
    measured on MI355X: 0.013 at M = 257, 8e-4 at M = 2,049."""
    from centerclip_amd import train
    dy32, x16 = (_dev(a) for a in wr.heavy_tailed(c))
    dy16, _, scale, _ = train._cast_transpose(dy32, scaled=True, col_sums=True, want_t=False, col_partials=True)
    assert float(dy16.abs().min()) >= 2.0 ** -14                                   # no fp16 subnormal (out of scope)
    dw = train._wgrad_tn(dy16, x16, scale)
    share, _ = _share(dw, dy16, x16, float(scale))
    print("[heavy %s] largest share of the per-element bound: %.2e" % (wr.case_id(c), share))
    assert share <= 1.0


@pytest.mark.parametrize("c", wr.FLOAT, ids=wr.case_id)
def test_cancelling_row_pairs(c):
    """Recipe two (wgrad_ref.cancelling): every entry is small against the sum of its terms' magnitudes."""
    dy16, x16 = (_dev(a) for a in wr.cancelling(c))
    assert float(dy16.abs().min()) >= 2.0 ** -14 and float(x16.abs().min()) >= 2.0 ** -14
    dw = _wgrad(dy16, x16, 8.0)
    share, cancel = _share(dw, dy16, x16, 8.0)
    print("[cancel %s] largest share of the per-element bound: %.2e; max|dW| / max sum|terms| = %.1e" % (wr.case_id(c), share, cancel))
    assert cancel < 0.1
    assert share <= 1.0
