"""CPU-only: argument validation of the paired / few-rows / in_proj + attention entry points (cc_linear_pair_f16,
cc_linear_rows_pair_f16, cc_inproj_attention_pair_f16) and the layout of their problem struct.  Every call here is refused
before anything is enqueued, so the pointers are never dereferenced and no GPU is needed."""
import ctypes

import pytest

CC_ERR_INVALID = -1
EPI_F16, EPI_F32_RESID, EPI_F32_PATCH, EPI_F16_LN, EPI_F16_GELU_LN, EPI_F32_RESID_STATS = 0, 2, 3, 5, 6, 7
FAKE = 0x10000          # a non-NULL address that is never read: each case below is invalid for ONE other reason


@pytest.fixture(scope="module")
def L():
    from centerclip_amd import build
    build.build(verbose=False)
    from centerclip_amd import _lib
    _lib.lib()
    return _lib


def problem(L, **kw):
    """A complete problem for every epilogue (all operands set, 64 x 128 x 64), then the case's defect."""
    f = dict(a=FAKE, w=FAKE, bias=FAKE, c=FAKE, M=64, N=128, K=64, ldc=128, ln_stats=FAKE, ln_slots=1, ln_c1=FAKE, ln_eps=1e-5,
             stats_out=FAKE, c16=FAKE, pos=FAKE, patch_n=4)
    f.update(kw)
    return L.LinearProblem(**f)


def attn_problem(L, **kw):
    f = dict(a=FAKE, w=FAKE, bias=FAKE, c=FAKE, M=64, N=192, K=64, ldc=64, ln_stats=FAKE, ln_slots=1, ln_c1=FAKE, ln_eps=1e-5,
             att_L=32, att_nseq=2, att_causal=0)
    f.update(kw)
    return L.LinearProblem(**f)


def test_struct_layout_matches_the_library(L):
    assert ctypes.sizeof(L.LinearProblem) == L.lib().cc_linear_problem_size()


@pytest.mark.parametrize("field", ["a", "w", "c"])
def test_null_operands_are_refused(L, field):
    lib = L.lib()
    slots = (ctypes.c_int32 * 2)()
    good = problem(L)
    bad = problem(L, **{field: None})
    for epi in (EPI_F16, EPI_F32_RESID, EPI_F32_RESID_STATS):
        assert lib.cc_linear_pair_f16(ctypes.byref(bad), None, epi, 0, slots, None) == CC_ERR_INVALID
        assert lib.cc_linear_pair_f16(ctypes.byref(good), ctypes.byref(bad), epi, 0, slots, None) == CC_ERR_INVALID    # the rider too
    assert lib.cc_linear_pair_f16(None, None, EPI_F16, 0, slots, None) == CC_ERR_INVALID
    for epi in (EPI_F32_RESID, EPI_F16_GELU_LN, EPI_F32_RESID_STATS):
        assert lib.cc_linear_rows_pair_f16(ctypes.byref(bad), None, epi, slots, None) == CC_ERR_INVALID
        assert lib.cc_linear_rows_pair_f16(ctypes.byref(good), ctypes.byref(bad), epi, slots, None) == CC_ERR_INVALID
    assert lib.cc_linear_rows_pair_f16(None, None, EPI_F32_RESID, slots, None) == CC_ERR_INVALID
    abad = attn_problem(L, **{field: None})
    assert lib.cc_inproj_attention_pair_f16(ctypes.byref(abad), None, None) == CC_ERR_INVALID
    assert lib.cc_inproj_attention_pair_f16(ctypes.byref(attn_problem(L)), ctypes.byref(abad), None) == CC_ERR_INVALID
    assert lib.cc_inproj_attention_pair_f16(None, None, None) == CC_ERR_INVALID


def test_epilogue_operands_are_required(L):
    lib = L.lib()
    slots = (ctypes.c_int32 * 2)()
    pair = lambda p, epi, so=slots: lib.cc_linear_pair_f16(ctypes.byref(p), None, epi, 0, so, None)
    rows = lambda p, epi, so=slots: lib.cc_linear_rows_pair_f16(ctypes.byref(p), None, epi, so, None)
    # the statistics epilogue without its outputs
    for miss in ("c16", "stats_out"):
        assert pair(problem(L, **{miss: None}), EPI_F32_RESID_STATS) == CC_ERR_INVALID
        assert rows(problem(L, **{miss: None}), EPI_F32_RESID_STATS) == CC_ERR_INVALID
    assert pair(problem(L), EPI_F32_RESID_STATS, None) == CC_ERR_INVALID
    assert rows(problem(L), EPI_F32_RESID_STATS, None) == CC_ERR_INVALID
    # centring statistics without a slot count / a place for the shift
    assert pair(problem(L, shift_stats=FAKE, shift_slots=0, shift_out=FAKE), EPI_F32_RESID_STATS) == CC_ERR_INVALID
    assert pair(problem(L, shift_stats=FAKE, shift_slots=1, shift_out=None), EPI_F32_RESID_STATS) == CC_ERR_INVALID
    assert rows(problem(L, shift_stats=FAKE, shift_slots=33, shift_out=FAKE), EPI_F32_RESID_STATS) == CC_ERR_INVALID
    # the folded LayerNorm without its statistics / column sums / c2, or with a slot count out of range
    for epi in (EPI_F16_LN, EPI_F16_GELU_LN):
        for kw in (dict(ln_stats=None), dict(ln_c1=None), dict(bias=None), dict(ln_slots=0), dict(ln_slots=33)):
            assert pair(problem(L, **kw), epi) == CC_ERR_INVALID
    assert rows(problem(L, ln_stats=None), EPI_F16_GELU_LN) == CC_ERR_INVALID
    # the patch epilogue without the positional embedding / the patch count
    assert pair(problem(L, pos=None), EPI_F32_PATCH) == CC_ERR_INVALID
    assert pair(problem(L, patch_n=0), EPI_F32_PATCH) == CC_ERR_INVALID
    # sizes, row stride, epilogue id
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(ldc=64), dict(ldc=132), dict(K=32), dict(N=96)):
        assert pair(problem(L, **kw), EPI_F16) == CC_ERR_INVALID, kw
    assert rows(problem(L, M=0), EPI_F32_RESID) == CC_ERR_INVALID
    assert pair(problem(L), 8) == CC_ERR_INVALID and pair(problem(L), -1) == CC_ERR_INVALID


def test_row_selection_belongs_to_the_rows_entry(L):
    lib = L.lib()
    slots = (ctypes.c_int32 * 2)()
    good = problem(L)
    for kw in (dict(row_map=FAKE), dict(row_step=50)):
        sel = problem(L, **kw)
        for epi in (EPI_F16_GELU_LN, EPI_F32_RESID, EPI_F32_RESID_STATS):
            assert lib.cc_linear_pair_f16(ctypes.byref(sel), None, epi, 0, slots, None) == CC_ERR_INVALID
            assert lib.cc_linear_pair_f16(ctypes.byref(good), ctypes.byref(sel), epi, 0, slots, None) == CC_ERR_INVALID
    # ... and the device-side row count to the tile kernel
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(problem(L, m_dev=FAKE)), None, EPI_F32_RESID, slots, None) == CC_ERR_INVALID
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(problem(L, row_step=-1)), None, EPI_F32_RESID, slots, None) == CC_ERR_INVALID


def test_forced_tile_must_divide_both_problems(L):
    lib = L.lib()
    carrier = problem(L, M=300, N=768, K=768, ldc=768)
    for tile, kw in ((7, dict(N=512, ldc=512)), (8, dict(K=192)), (5, dict(N=128)), (10, dict(N=128)), (9, {}), (11, {})):
        rider = problem(L, **kw)
        assert lib.cc_linear_pair_f16(ctypes.byref(carrier), ctypes.byref(rider), EPI_F16, tile, None, None) == CC_ERR_INVALID, tile


def test_packed_sequences_need_offsets_and_lengths(L):
    lib = L.lib()
    good = attn_problem(L)
    for kw in (dict(att_seq_off=FAKE), dict(att_seq_len=FAKE), dict(att_nseq=0), dict(att_L=0), dict(M=63), dict(ln_slots=0),
               dict(ln_stats=None), dict(bias=None), dict(M=65, att_seq_off=FAKE, att_seq_len=FAKE)):
        bad = attn_problem(L, **kw)
        assert lib.cc_inproj_attention_pair_f16(ctypes.byref(bad), None, None) == CC_ERR_INVALID, kw
        assert lib.cc_inproj_attention_pair_f16(ctypes.byref(good), ctypes.byref(bad), None) == CC_ERR_INVALID, kw
    # outside the one-launch form (an output row stride other than W, more than 256 tokens, selected rows): unsupported,
    # again before any launch
    for kw in (dict(N=384, K=128, ldc=64), dict(att_L=257, att_nseq=1, M=257), dict(row_step=2)):
        assert lib.cc_inproj_attention_pair_f16(ctypes.byref(attn_problem(L, **kw)), None, None) == -2, kw
