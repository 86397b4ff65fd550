"""The exact GELU x Phi(x) of the OpenCLIP-format checkpoints on the GPU (needs a real MI355X, ``-m gpu``):

* the elementwise pair cc_gelu_f16 / cc_gelu_backward_f16 against float64 with the bounds of the QuickGELU pair
  (test_backward_gpu.py): forward within one fp16 ulp of the float64 value rounded to fp16, backward within
  2e-6 |du| (1 + |x|);
* the two new GEMM epilogues (bias + GELU, LN-folded + GELU) on every tile, through the paired launch with a device-side
  row count and through the few-rows kernel, against float64 on the same fp16 operands with test_linear_pair_gpu.py's
  bounds (2e-3 / 3e-3 of the largest entry) - and, with pre-activations of at most 4, MORE than 2e-3 away from the
  float64 QuickGELU value (the two activations differ by 0.0203 at |x| = 2.27), so the ids are no alias of the old ones;
* a tiny CLIP built with quick_gelu=False against the oracle with its activation swapped (embeddings within 1e-3), both row
  policies, uint8 frames, graphed evaluation lanes, the seqTransf head untouched;
* training: one block and the whole tiny step against float64 autograd with nn.GELU's function, the captured step against
  eager steps, a frozen first block.
"""
import ctypes
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerclip_amd import torch_ops  # noqa: F401  (registers torch.ops.centerclip)
from oracle import clip_oracle as clo

pytestmark = pytest.mark.gpu
DEV = "cuda"
CC_ERR_INVALID = -1
EPI_F16_GELU_ERF, EPI_F16_GELU_ERF_LN = 9, 10
SENT16 = -1234.0                                  # exactly representable in fp16; never produced by the data below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_gelu(x):
    """x Phi(x) with Phi through erfc (accurate in the negative tail in any precision; differentiable)."""
    return x * (0.5 * torch.special.erfc(-x / math.sqrt(2.0)))


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------- elementwise
def _gelu_inputs(n, seed):
    """test_backward_gpu._gelu_inputs: the long negative tail, the whole fp16 range, +-0, +-65504, subnormals."""
    g = _gen(seed)
    x = torch.randn(n, device=DEV, generator=g) * 3.0
    k = n // 8
    if k:
        x[:k] = -torch.rand(k, device=DEV, generator=g) * 70.0
        x[k:2 * k] = (torch.rand(k, device=DEV, generator=g) * 2 - 1) * 65504.0
    x16 = x.half()
    x16[:4] = torch.tensor([0.0, -0.0, 65504.0, -65504.0], device=DEV).half()
    if n >= 8:
        x16[-4:] = torch.tensor([6e-8, -6e-8, -17.0, 17.0], device=DEV).half()
    return x16


def _f16_ulp(y16):
    a = y16.float().abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10).double()


@pytest.mark.parametrize("n", [4, 1020, 1028, 8192 * 1024 + 4])
def test_gelu_forward_and_backward_against_float64(n):
    """cc_gelu_f16 within one fp16 ulp of the float64 value rounded to fp16 (signs of +-0 kept, nothing non-finite);
    cc_gelu_backward_f16 within 2e-6 |du| (1 + |x|) of du (Phi(x) + x phi(x)); out_amax == the largest written magnitude.
    The last size runs the grid-stride loop."""
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    x16 = _gelu_inputs(n, n % 9973)
    out = torch.empty_like(x16)
    L.check(L.lib().cc_gelu_f16(L.ptr(x16), L.ptr(out), n, _st(out)), "cc_gelu_f16")
    xd = x16.double()
    want = exact_gelu(xd).half()
    err = (out.double() - want.double()).abs()
    ulps = err / _f16_ulp(want)
    print("n = %d: forward worst %.2f fp16 ulp (bound 1)" % (n, float(ulps.max())))
    assert bool(torch.isfinite(out).all())
    assert bool((err <= _f16_ulp(want)).all()), (float(ulps.max()), float(x16[ulps.argmax()]))
    assert torch.equal(torch.signbit(out[:2]), torch.signbit(want[:2])) and float(out[0]) == 0.0 and float(out[1]) == 0.0
    assert float(out[2]) == 65504.0 and float(out[3]) == 0.0
    du = torch.randn(n, device=DEV, generator=_gen(n % 7919 + 1))
    dout = torch.empty_like(du)
    am = torch.zeros(1, device=DEV)
    L.check(L.lib().cc_gelu_backward_f16(L.ptr(x16), L.ptr(du), L.ptr(dout), n, L.ptr(am), _st(du)), "cc_gelu_backward_f16")
    cdf = 0.5 * torch.special.erfc(-xd / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2.0 * math.pi)
    want_d = du.double() * (cdf + xd * pdf)
    err = (dout.double() - want_d).abs()
    den = du.double().abs() * (1 + xd.abs())
    print("n = %d: backward worst %.2e |du| (1 + |x|) (bound 2e-6)" % (n, float((err / den.clamp_min(1e-300)).max())))
    assert bool(torch.isfinite(dout).all()) and bool((err <= 2e-6 * den).all())
    assert float(am[0]) == float(dout.abs().max())
    # not the QuickGELU pair under another name: the two differ by 0.02 near |x| = 2.27
    q = torch.empty_like(x16)
    L.check(L.lib().cc_quick_gelu_f16(L.ptr(x16), L.ptr(q), n, _st(q)), "cc_quick_gelu_f16")
    if n > 8:
        assert float((q.float() - out.float()).abs().max()) > 0.015


def test_gelu_refuses_ragged_sizes():
    from centerclip_amd import _lib as L
    from centerclip_amd.torch_ops import _st
    x16 = torch.zeros(8, device=DEV, dtype=torch.float16)
    du = torch.zeros(8, device=DEV)
    assert L.lib().cc_gelu_f16(L.ptr(x16), L.ptr(x16.clone()), 6, _st(du)) == CC_ERR_INVALID
    assert L.lib().cc_gelu_backward_f16(L.ptr(x16), L.ptr(du), L.ptr(du.clone()), 6, None, _st(du)) == CC_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- epilogues
class Problem:
    """Operands of one GEMM for both new epilogues, the pre-activations' largest magnitude scaled to ``peak`` (<= 4 where
    the test also proves the distance from QuickGELU), and their float64 pre-activations."""

    def __init__(self, M, N, K, seed, peak=3.9):
        from centerclip_amd import ops
        g = _gen(seed)
        r = lambda *s: torch.randn(*s, generator=g, device=DEV)
        self.M, self.N, self.K = M, N, K
        # bias + activation: a [M, K] fp16, w [N, K] fp16, bias [N]
        a, w, bias = r(M, K).half(), (r(N, K) * K ** -0.5).half(), r(N) * 0.5
        s = peak / float((a.double() @ w.double().t() + bias.double()).abs().max())
        self.a, self.w, self.bias = a, (w.float() * s).half(), bias * s
        self.pre = self.a.double() @ self.w.double().t() + self.bias.double()
        # LN-folded: rows x [M, K] fp32 -> centred fp16 copy + one-slot statistics, the folded weight
        self.x = r(M, K) * 1.5 + 0.3
        gamma, beta = torch.rand(K, generator=g, device=DEV) + 0.5, r(K) * 0.2
        w2, b2 = r(N, K) * K ** -0.5, r(N) * 0.1
        ln = F.layer_norm(self.x.double(), (K,), gamma.double(), beta.double(), 1e-5)
        s2 = peak / float((ln @ w2.double().t() + b2.double()).abs().max())
        w2, b2 = w2 * s2, b2 * s2
        self.pre_ln = ln @ w2.double().t() + b2.double()
        self.h16, st, _ = ops.row_stats(self.x)
        self.st = st.contiguous()
        self.wf, self.c1, self.c2 = ops.fold_layernorm_linear(w2, b2, gamma, beta)
        assert float(self.pre.abs().max()) <= 4.0 and float(self.pre_ln.abs().max()) <= 4.0

    def pre_of(self, epi):
        return self.pre_ln if epi == EPI_F16_GELU_ERF_LN else self.pre

    def struct(self, epi, out, m_dev=None, row_step=0, row_map=None):
        from centerclip_amd import _lib as L
        p = L.LinearProblem(M=self.M, N=self.N, K=self.K, ldc=self.N, c=out.data_ptr(), m_dev=None if m_dev is None else m_dev.data_ptr(),
                            row_step=row_step, row_map=None if row_map is None else row_map.data_ptr())
        if epi == EPI_F16_GELU_ERF_LN:
            p.a, p.w, p.bias, p.ln_stats, p.ln_slots, p.ln_c1, p.ln_eps = (self.h16.data_ptr(), self.wf.data_ptr(), self.c2.data_ptr(),
                                                                           self.st.data_ptr(), 1, self.c1.data_ptr(), 1e-5)
        else:
            p.a, p.w, p.bias = self.a.data_ptr(), self.w.data_ptr(), self.bias.data_ptr()
        return p


TOL = {EPI_F16_GELU_ERF: 2e-3, EPI_F16_GELU_ERF_LN: 3e-3}        # test_linear_pair_gpu.TOL for ids 1 and 6
_problems = {}


def problem(M, N, K, seed):
    key = (M, N, K, seed)
    if key not in _problems:
        _problems[key] = Problem(M, N, K, seed)
    return _problems[key]


def _check_act(out, pre, epi, tag, worst):
    """out against float64 GELU(pre) within the id's bound - and more than 2e-3 away from float64 QuickGELU(pre)."""
    e = _relerr(out.float(), exact_gelu(pre))
    away = _relerr(out.float(), quick_gelu(pre))
    worst[epi] = max(worst.get(epi, 0.0), e)
    worst["away"] = min(worst.get("away", 1.0), away)
    assert e < TOL[epi], (tag, e)
    assert away > 2e-3, (tag, away)


def _run_tile(P, epi, tile):
    from centerclip_amd import ops
    if epi == EPI_F16_GELU_ERF_LN:
        return ops.linear_ln_f16(P.h16, P.wf, P.c1, P.c2, P.st, 1, gelu="erf", tile=tile)
    return ops.linear_f16(P.a, P.w, P.bias, "f16_gelu_erf", tile=tile)


@pytest.mark.parametrize("epi", [EPI_F16_GELU_ERF, EPI_F16_GELU_ERF_LN])
def test_epilogues_on_every_tile_against_float64(epi):
    """ops.linear_f16(..., 'f16_gelu_erf') / ops.linear_ln_f16(..., gelu='erf') at every tile id (forced) and the dispatcher's
    own choice: M = 257 (no multiple of any tile height; three row tiles of 128), N = 768 (every tile width divides it),
    K = 64 and 192 (and 128 for the 128-deep tile 8); the QuickGELU ids on the same operands give other values."""
    from centerclip_amd import _lib as L, ops
    lib = L.lib()
    worst, ran = {}, set()
    for K in (64, 192, 128):
        P = problem(257, 768, K, 7000 + K)
        pre = P.pre_of(epi)
        for tile in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):
            if tile == 8 and K % 128:
                with pytest.raises(L.CenterClipHipError):
                    _run_tile(P, epi, tile)
                continue
            if K == 128 and tile not in (0, 8):
                continue
            y = _run_tile(P, epi, tile)
            assert y.shape == (257, 768) and y.dtype == torch.float16
            _check_act(y, pre, epi, (K, tile), worst)
            ran.add(tile or lib.cc_linear_tile_for(257, 768, K, epi))
        # the QuickGELU id on the same operands: the old values, not the new ones
        if epi == EPI_F16_GELU_ERF_LN:
            q = ops.linear_ln_f16(P.h16, P.wf, P.c1, P.c2, P.st, 1, gelu=True)
        else:
            q = ops.linear_f16(P.a, P.w, P.bias, "f16_gelu")
        assert _relerr(q.float(), quick_gelu(pre)) < TOL[epi] and _relerr(q.float(), exact_gelu(pre)) > 2e-3
    assert ran >= {1, 2, 3, 4, 5, 6, 7, 8, 10}
    print("epilogue %d: worst error vs float64 GELU %.3g (bound %.0e); nearest to float64 QuickGELU %.3g (must exceed 2e-3)"
          % (epi, worst[epi], TOL[epi], worst["away"]))
    # out= with a row stride (the id through linear_f16_out)
    if epi == EPI_F16_GELU_ERF:
        P = problem(257, 768, 64, 7064)
        buf = torch.full((257, 800), SENT16, device=DEV, dtype=torch.float16)
        ops.linear_f16(P.a, P.w, P.bias, "f16_gelu_erf", out=buf[:, :768])
        assert torch.equal(buf[:, :768], _run_tile(P, epi, 0)) and bool((buf[:, 768:] == SENT16).all())


@pytest.mark.parametrize("epi", [EPI_F16_GELU_ERF, EPI_F16_GELU_ERF_LN])
def test_epilogues_in_the_paired_launch_with_a_device_side_row_count(epi):
    """cc_linear_pair_f16: carrier 300 x 768 x 192 + rider 130 x 512 x 64 whose row count (65) is read from the device: each
    problem's rows equal its stand-alone launch at the tile the pair ran bit for bit, rows behind the count and the guard rows
    keep the sentinel."""
    from centerclip_amd import _lib as L
    lib = L.lib()
    car, rid = problem(300, 768, 192, 7101), problem(130, 512, 64, 7102)
    m = 65
    m_dev = torch.tensor([m], dtype=torch.int32, device=DEV)
    worst = {}
    for tile in (0, 1, 4):
        oc = torch.full((300 + 3, 768), SENT16, device=DEV, dtype=torch.float16)
        orr = torch.full((130 + 3, 512), SENT16, device=DEV, dtype=torch.float16)
        pc, pr = car.struct(epi, oc), rid.struct(epi, orr, m_dev=m_dev)
        slots = (ctypes.c_int32 * 2)()
        rc = lib.cc_linear_pair_f16(ctypes.byref(pc), ctypes.byref(pr), epi, tile, slots, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (epi, tile, rc)
        ran = tile or 4                 # (auto: the carrier's 64x64 choice at 300 rows also divides the rider)
        _check_act(oc[:300], car.pre_of(epi), epi, ("carrier", tile), worst)
        e = _relerr(orr[:m].float(), exact_gelu(rid.pre_of(epi)[:m]))
        assert e < TOL[epi], ("rider", tile, e)
        assert bool((oc[300:] == SENT16).all()) and bool((orr[m:] == SENT16).all()), tile
        if tile:
            assert torch.equal(oc[:300], _run_tile(car, epi, ran)), tile
    print("paired launch, epilogue %d: worst error vs float64 %.3g (bound %.0e)" % (epi, worst[epi], TOL[epi]))


def test_few_rows_kernel_with_the_new_epilogue():
    """cc_linear_rows_pair_f16 with id 10: the CLS rows of 48 frames of 50 tokens (row_step = 50; 4 x 128 -> 512 columns, K =
    192) and a rider on mapped rows (5 rows, 64 columns, K = 64) against float64 on those rows; every other row keeps the
    sentinel; id 9 (no LN-folded operands) is not a few-rows epilogue."""
    from centerclip_amd import _lib as L
    lib = L.lib()
    epi = EPI_F16_GELU_ERF_LN
    step, Mr = 50, 48
    big = problem((Mr - 1) * step + 2, 512, 192, 7201)
    small = problem(23, 64, 64, 7202)
    rows_b = torch.arange(Mr, device=DEV) * step
    map_s = torch.tensor([17, 3, 22, 0, 9], dtype=torch.int32, device=DEV)
    ob = torch.full((big.M + 3, 512), SENT16, device=DEV, dtype=torch.float16)
    os_ = torch.full((small.M + 3, 64), SENT16, device=DEV, dtype=torch.float16)
    pb, ps = big.struct(epi, ob, row_step=step), small.struct(epi, os_, row_map=map_s)
    pb.M, ps.M = Mr, 5
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(pb), ctypes.byref(ps), epi, None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    worst = {}
    _check_act(ob[rows_b], big.pre_ln[rows_b], epi, "row_step", worst)
    _check_act(os_[map_s.long()], small.pre_ln[map_s.long()], epi, "row_map", worst)
    keep = torch.ones(ob.shape[0], dtype=torch.bool, device=DEV)
    keep[rows_b] = False
    assert bool((ob[keep] == SENT16).all())
    keep = torch.ones(os_.shape[0], dtype=torch.bool, device=DEV)
    keep[map_s.long()] = False
    assert bool((os_[keep] == SENT16).all())
    # the tile kernel on all rows of the same operands agrees on the selected rows to the fp16 rounding
    full = _run_tile(big, epi, 0)
    assert _relerr(ob[rows_b].float(), full[rows_b].float()) < 3e-3
    print("few rows, epilogue 10: worst error vs float64 %.3g (bound 3e-03)" % worst[epi])
    fresh = torch.full_like(ob, SENT16)
    pq = big.struct(EPI_F16_GELU_ERF, fresh, row_step=step)
    pq.M = Mr
    assert lib.cc_linear_rows_pair_f16(ctypes.byref(pq), None, EPI_F16_GELU_ERF, None, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((fresh == SENT16).all())


def test_wrapper_refuses_unknown_activation_names():
    from centerclip_amd import ops
    P = problem(257, 768, 64, 7064)
    with pytest.raises(ValueError, match="gelu"):
        ops.linear_ln_f16(P.h16, P.wf, P.c1, P.c2, P.st, 1, gelu="tanh")
    with pytest.raises(ValueError, match="epilogue"):
        ops.linear_f16(P.a, P.w, P.bias, "f16_gelu_tanh")


# ---------------------------------------------------------------------------------------------------- towers
TINY = dict(B=2, T=4, T_new=2, K=16, cluster_block=2, words=32, patch=16, res=112, width=128, layers=3, embed=128, vocab=512)


def _tiny_sd(seed=0):
    """Random weights of a small CLIP (patch 16, 112 px: 50 tokens per frame; width 128, 3 layers; text width 128, 2 layers),
    rounded through fp16 - under the OpenAI / OpenCLIP key names."""
    from centerclip_amd.clip import CLIP
    c = TINY
    torch.manual_seed(seed)
    m = CLIP(c["embed"], c["res"], c["layers"], c["width"], c["patch"], 77, c["vocab"], 128, 2, 2, args=None)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _task_config(quick_gelu=0, sim_header="meanP"):
    c = TINY
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=c["T"], target_frames_blocks=[c["T"], c["T_new"], c["T_new"]],
                     cluster_num_blocks=[49, c["K"], c["K"]], cluster_distance='euclidean', cluster_threshold=1e-6,
                     cluster_iter_limit=100, minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/16', aggregation=None, pre_norm=False,
                     loose_type=True, sim_header=sim_header, linear_patch='2d', cross_num_hidden_layers=2, quick_gelu=quick_gelu)


def _ids(B, seed=1):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, TINY["words"], dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(4, TINY["words"] + 1, (1,), generator=gen))
        ids[b, 0], ids[b, n - 1] = 510, 511
        ids[b, 1:n - 1] = torch.randint(1, 500, (n - 2,), generator=gen)
    return ids


def _batch(seed, B=None):
    c = TINY
    B = B or c["B"]
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, 1, c["T"], 3, c["res"], c["res"], generator=g).half().float()
    vmask = torch.ones(B, 1, c["T"], dtype=torch.long)
    vmask[-1, 0, c["T"] - 1:] = 0
    ids = _ids(B, seed + 1)
    return ids, (ids > 0).long(), video, vmask


def _nrm(x):
    return x / x.norm(dim=-1, keepdim=True)


def _emb_err(a, b):
    return float((_nrm(a.detach().cpu().float()) - _nrm(b.float())).abs().max())


@pytest.fixture(scope="module")
def tiny_eval():
    """The oracle's embeddings of one clip and three captions with the activation swapped for the exact GELU (and, for the
    visual tower, with QuickGELU too), its block-2 medoids - computed once."""
    sd = _tiny_sd()
    c = TINY
    video = torch.randn(c["T"], 3, c["res"], c["res"], generator=torch.Generator().manual_seed(4)).half().float()
    ids = _ids(3)
    plan = {1: (c["T_new"], c["K"])}
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(clo, "quick_gelu", exact_gelu)
        vis, med = clo.visual_forward(sd, video, c["T"], cluster_plan=plan, return_medoids=True)
        text = clo.text_forward(sd, ids)
    finally:
        mp.undo()
    vis_q = clo.visual_forward(sd, video, c["T"], cluster_plan=plan, forced_medoids={1: med[1]})
    return dict(sd=sd, video=video, ids=ids, vis=vis, med=med[1], text=text, vis_q=vis_q)


@pytest.mark.parametrize("all_rows", [False, True])
def test_tiny_towers_against_the_oracle_with_the_exact_activation(tiny_eval, all_rows):
    """build_clip_model(..., quick_gelu=False): encode (forced medoids), encode_text (compacted captions under the shipped
    policy) and encode_pair within 1e-3 of the oracle whose activation is the exact GELU, under the shipped row policy and
    under CC_ROWS_ALL_TEXT | CC_ROWS_ALL_LAST_BLOCK; the QuickGELU oracle on the same weights is further away than the exact one; uint8
    frames give the float frames' bits."""
    from centerclip_amd.clip import build_clip_model
    t, c = tiny_eval, TINY
    model, _ = build_clip_model(dict(t["sd"]), args=_task_config(), quick_gelu=False)
    model = model.to(DEV)
    video, ids = t["video"].to(DEV), t["ids"].to(DEV)
    with model.row_policy(all_text_rows=all_rows, all_last_block_rows=all_rows):
        feats, _ = model.visual.encode(video, c["T"], forced_medoids=t["med"])
        tfeat = model.encode_text(ids)
        model.visual.forced_medoids = t["med"]
        vpair, tpair = model.encode_pair(video, ids, video_frame=c["T"])
        torch.cuda.synchronize()
        assert model._text_pack.struct.activation == 1 and model._text_pack.struct.row_policy == (3 if all_rows else 0)
        assert model.visual._pack.struct.activation == 1 and model.visual._pack.struct.row_policy == (2 if all_rows else 0)
        u8 = torch.randint(0, 256, (c["T"], c["res"], c["res"], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
        f_u8, _ = model.visual.encode(u8.to(DEV), c["T"], forced_medoids=t["med"])
        f_fl, _ = model.visual.encode(clo.loader_normalize(u8, channels_last=True).to(DEV), c["T"], forced_medoids=t["med"])
    ev, et, evp, etp = _emb_err(feats, t["vis"]), _emb_err(tfeat, t["text"]), _emb_err(vpair, t["vis"]), _emb_err(tpair, t["text"])
    print("all_rows=%d: visual %.2e text %.2e, paired %.2e / %.2e (bound 1e-3); vs the QuickGELU oracle %.2e"
          % (all_rows, ev, et, evp, etp, _emb_err(feats, t["vis_q"])))
    assert feats.shape == t["vis"].shape == (c["T_new"], c["embed"]) and tfeat.shape == t["text"].shape
    assert max(ev, et, evp, etp) <= 1e-3
    assert _emb_err(feats, t["vis_q"]) > ev                    # the activation is really the other one
    assert torch.equal(f_u8, f_fl)
    # the default build of the same weights is the reference's model
    ref_model, _ = build_clip_model(dict(t["sd"]), args=_task_config())
    fq, _ = ref_model.to(DEV).visual.encode(video, c["T"], forced_medoids=t["med"])
    assert not torch.equal(fq, feats) and _emb_err(fq, t["vis_q"]) <= 1e-3 and _emb_err(fq, t["vis"]) > _emb_err(fq, t["vis_q"])


def _model(quick_gelu=0, sim_header="meanP", sd=None):
    from centerclip_amd.clip4clip import CLIP4Clip
    return CLIP4Clip.from_state_dict(dict(sd if sd is not None else _tiny_sd(3)), _task_config(quick_gelu, sim_header)).float().to(DEV)


class _Clips(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        self.ids, self.mask, self.video, self.vmask = _batch(seed, B=n)

    def __len__(self):
        return self.ids.shape[0]

    def __getitem__(self, i):
        return self.ids[i], self.mask[i], torch.zeros_like(self.ids[i]), self.video[i], self.vmask[i]


def test_eval_epoch_graphed_lanes_equal_the_eager_forward():
    """eval_epoch over two batches of two clips: the graphed lanes (two model instances, a hipGraph each) cache the operand
    rows of the eager one-batch-at-a-time loop, and those are the rows of the model's own forward."""
    from centerclip_amd import eval as ceval
    model = _model().eval()
    assert model.replica().clip.quick_gelu is False
    loader = torch.utils.data.DataLoader(_Clips(4, 21), batch_size=2, shuffle=False)

    def rows(**kw):
        seen, orig = {}, ceval._sharded_metrics

        def grab(core, cache, *a):
            seen["video"], seen["text"] = torch.cat(cache.video).clone(), torch.cat(cache.text).clone()
            return orig(core, cache, *a)
        ceval._sharded_metrics = grab
        try:
            ceval.eval_epoch(model, loader, DEV, **kw)
        finally:
            ceval._sharded_metrics = orig
        return seen
    base = rows(in_flight=1)
    for kw in (dict(in_flight=1, graphed=True), dict(in_flight=2, graphed=True)):
        got = rows(**kw)
        assert torch.equal(got["video"], base["video"]) and torch.equal(got["text"], base["text"]), kw
    ids, am, seg, video, vm = (x.to(DEV) for x in next(iter(loader)))
    with torch.no_grad():
        vis = model(ids, seg, am, video, vm)["visual_output"]
        vmask = model.get_video_mask_after_cluster(vm.view(-1, vm.shape[-1]))
        want = ceval.HipBackend.video_operand(vis.contiguous(), vmask.contiguous())
    assert torch.equal(base["video"][:2], want)


def test_seqtransf_head_keeps_quickgelu():
    """Two seqTransf models on the same weights, towers with the exact GELU and with QuickGELU: for the same per-segment
    features the head's output is the same, bit for bit (cc_seqtransf_forward_f32 does not read the towers' activation)."""
    sd = _tiny_sd(3)
    m0, m1 = _model(0, "seqTransf", sd).eval(), _model(1, "seqTransf", sd).eval()
    assert all(b.quick_gelu for b in m0.transformerClip.resblocks) and not m0.clip.quick_gelu and m1.clip.quick_gelu
    g = torch.Generator().manual_seed(8)
    vis = torch.randn(3, TINY["T_new"], TINY["embed"], generator=g).to(DEV)
    mask = torch.ones(3, TINY["T_new"], dtype=torch.long, device=DEV)
    mask[1, 1:] = 0
    with torch.no_grad():
        h0, h1 = m0.seq_head(vis, mask), m1.seq_head(vis, mask)
        torch.cuda.synchronize()
        assert torch.equal(h0, h1) and not torch.equal(h0, vis)
        # ... while the towers of the two models differ
        ids, am, video, vm = (x.to(DEV) for x in _batch(31))
        v0 = m0(ids, torch.zeros_like(ids), am, video, vm)["visual_output"]
        v1 = m1(ids, torch.zeros_like(ids), am, video, vm)["visual_output"]
    assert not torch.equal(v0, v1)


# ---------------------------------------------------------------------------------------------------- training
def _rel(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("causal", [False, True])
def test_block_training_against_float64_autograd(causal, monkeypatch):
    """block_forward_train / block_backward of a block built with quick_gelu=False (L = 50, N = 2, W = 128) against float64
    autograd through the same block with the exact GELU: z, dx and the 12 parameter gradients within 2e-3 of each tensor's
    largest entry (test_backward_gpu's measure and bound); the QuickGELU block on the same weights is further from that reference."""
    from centerclip_amd import train
    from centerclip_amd.clip import ResidualAttentionBlock
    from oracle.recipes import block_grad_inputs
    cfg = dict(seed=411 + causal, L=50, N=2, W=128, heads=2, causal=causal)
    x, dz, sd = block_grad_inputs(cfg)
    x, dz = torch.from_numpy(x).to(DEV), torch.from_numpy(dz).to(DEV)
    mask = (lambda n: None) if causal else None
    blk = ResidualAttentionBlock(128, 2, attn_mask=mask, block_id=1, args=None, quick_gelu=False)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    blk = blk.to(DEV)
    z, saved = train.block_forward_train(blk, x)
    dx, grads = train.block_backward(blk, saved, dz)
    monkeypatch.setattr(clo, "quick_gelu", F.gelu)                     # nn.GELU()'s function, float64
    zr, dxr, gr = clo.block_backward64(x, dz, dict(blk.state_dict()), 2, causal)
    errs = {"z": _rel(z, zr), "dx": _rel(dx, dxr)}
    for k, v in grads.items():
        errs[k] = _rel(v.reshape(gr[k].shape), gr[k])
    print("[causal=%d] relative errors:" % causal, {k: "%.1e" % e for k, e in errs.items()})
    assert len(grads) == 12 and max(errs.values()) < 2e-3, errs
    monkeypatch.undo()
    blk_q = ResidualAttentionBlock(128, 2, attn_mask=mask, block_id=1, args=None).to(DEV)
    blk_q.load_state_dict(blk.state_dict())
    zq, _ = train.block_forward_train(blk_q, x)
    assert _rel(zq, zr) > errs["z"] and not torch.equal(zq, z)
    # the block-level eval forward (clip.py's drop-in on LND activations) reads the same flag
    with torch.no_grad():
        ze = blk((x, -1, None))[0]
    assert _rel(ze, zr) < 2e-3 and not torch.equal(blk_q((x, -1, None))[0].detach(), ze)


@pytest.fixture(scope="module")
def tiny_step():
    """One HIP training step of the tiny CLIP4Clip with quick_gelu = 0 and float64 autograd through the oracle with the exact
    GELU on the same weights, batch and block-2 selection - computed once."""
    model = _model().train()
    ids, amask, video, vmask = (x.to(DEV) for x in _batch(103))
    out = model(ids, torch.zeros_like(ids), amask, video, vmask)
    out["loss"].backward()
    torch.cuda.synchronize()
    c = TINY
    med = model.clip.visual.transformer.resblocks[c["cluster_block"] - 1].tokencluster_inter.last_medoids.clone()
    named = dict(model.clip.named_parameters())
    hip = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
    p64 = {k: v.detach().to(torch.float64).requires_grad_(True) for k, v in named.items()}
    plan = {c["cluster_block"] - 1: (c["T_new"], c["K"])}
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(clo, "quick_gelu", F.gelu)
        loss64, seq64, vis64 = clo.clip4clip_train_loss_native(p64, ids, video.double(), vmask, c["T"], c["T_new"], plan,
                                                               forced_medoids={c["cluster_block"] - 1: med})
        loss64.backward()
    finally:
        mp.undo()
    ref = {k: p.grad for k, p in p64.items() if p.grad is not None}
    return dict(model=model, out=out, hip=hip, ref=ref, loss64=loss64.detach(), seq64=seq64.detach(), vis64=vis64.detach(),
                vmask=vmask, named=named)


def test_tiny_training_step_against_float64(tiny_step):
    """Every parameter gradient of the step against float64 autograd with test_train_full_gpu's measure and the per-group bounds
    test_vitl14_gpu's tiny step uses (BOUNDS_CFG5 / FEAT_BOUNDS_CFG5): the features within their bounds, the loss against
    float64 on the step's own features within the loss bound."""
    from test_train_full_gpu import _rel as rel_full, compare_grads, BOUNDS_CFG5, FEAT_BOUNDS_CFG5, GROUPS, _group
    s, c = tiny_step, TINY
    out = s["out"]
    e_seq, e_vis = rel_full(out["sequence_output"].detach(), s["seq64"]), rel_full(out["visual_output"].detach(), s["vis64"])
    _, _, own = clo.contrastive_loss_native(out["sequence_output"].detach().double(), out["visual_output"].detach().double(),
                                            clo.video_mask_after_cluster(s["vmask"].view(c["B"], c["T"]), c["T"], c["T_new"]),
                                            s["named"]["logit_scale"].detach().double())
    e_loss = abs(float(out["loss"].detach()) - float(own)) / abs(float(own))
    errs, bad = compare_grads(s["hip"], s["ref"], BOUNDS_CFG5)
    worst = {g: max([e for k, e in errs.items() if _group(k) == g] or [0.0]) for g in GROUPS}
    print("\n[tiny, exact GELU] sequence_output %.2e visual_output %.2e loss (own features) %.2e" % (e_seq, e_vis, e_loss))
    print("[tiny, exact GELU] worst per group:", {g: "%.2e" % e for g, e in worst.items()})
    assert e_seq <= FEAT_BOUNDS_CFG5["sequence_output"] and e_vis <= FEAT_BOUNDS_CFG5["visual_output"]
    assert e_loss <= FEAT_BOUNDS_CFG5["loss"]
    assert set(s["hip"]) == set(s["ref"]) and "logit_scale" in s["ref"]
    assert not bad, [(k, errs[k]) for k in bad]


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.clip.named_parameters()}


def test_tiny_training_with_a_frozen_first_block():
    """freeze_cip_layers(1): block 1 of both towers runs on the fused prefix entries, which read the model's activation too -
    the gradients of everything that still trains against float64 autograd (exact GELU) with this step's own selection."""
    from test_train_full_gpu import compare_grads, BOUNDS_CFG5
    model = _model().train()
    model.freeze_cip_layers(1)
    ids, amask, video, vmask = (x.to(DEV) for x in _batch(103))
    out = model(ids, torch.zeros_like(ids), amask, video, vmask)
    out["loss"].backward()
    torch.cuda.synchronize()
    c = TINY
    med = model.clip.visual.transformer.resblocks[c["cluster_block"] - 1].tokencluster_inter.last_medoids.clone()
    grads = {k: g for k, g in _grads(model).items() if g is not None}
    frozen = [k for k, p in model.clip.named_parameters() if not p.requires_grad]
    assert "visual.transformer.resblocks.0.mlp.c_fc.weight" in frozen and not set(frozen) & set(grads)
    assert "visual.transformer.resblocks.1.mlp.c_fc.weight" in grads
    p64 = {k: v.detach().to(torch.float64).requires_grad_(True) for k, v in model.clip.named_parameters()}
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(clo, "quick_gelu", F.gelu)
        loss64, _, _ = clo.clip4clip_train_loss_native(p64, ids, video.double(), vmask, c["T"], c["T_new"],
                                                       {c["cluster_block"] - 1: (c["T_new"], c["K"])},
                                                       forced_medoids={c["cluster_block"] - 1: med})
        loss64.backward()
    finally:
        mp.undo()
    assert abs(float(out["loss"].detach()) - float(loss64.detach())) <= 1e-3 * abs(float(loss64.detach()))
    ref = {k: p.grad for k, p in p64.items() if k in grads}
    assert set(ref) == set(grads) and all(v is not None for v in ref.values())
    errs, bad = compare_grads(grads, ref, BOUNDS_CFG5)
    print("[tiny, exact GELU, frozen block 1] worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, [(k, errs[k]) for k in bad]
    # the prefix of the QuickGELU model on the same weights is another function
    mq = _model(1).train()
    mq.freeze_cip_layers(1)
    frames = video.reshape(-1, 3, c["res"], c["res"])
    h0 = model.clip.visual.encode_prefix(frames, c["T"], 1)
    h1 = mq.clip.visual.encode_prefix(frames, c["T"], 1)
    assert h0.shape == h1.shape and not torch.equal(h0, h1)


def test_graphed_train_step_equals_eager_steps():
    """train.GraphedTrainStep with the exact GELU: two calls (capture + replay, replay) leave the parameters two eager steps
    leave, bit for bit (as test_amp_graph_gpu / test_vitl14_gpu compare them)."""
    from centerclip_amd.train import BertAdam, prep_optim_params_groups, train_epoch, GraphedTrainStep
    ids, amask, video, vmask = _batch(103)
    batch = (ids, amask, torch.zeros_like(ids), video, vmask)
    args = Namespace(lr=1e-3, wd=0.2, new_added_modules=["Cross"], gradient_accumulation_steps=1, clip_grad_norm=None)
    sd = _tiny_sd(3)

    def build(capturable):
        m = _model(0, sd=sd).train()
        o = BertAdam(prep_optim_params_groups(args, m), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                     e=1e-6, max_grad_norm=1.0, capturable=capturable)
        return m, o
    m0, o0 = build(False)
    train_epoch(0, args, m0, [batch] * 2, DEV, o0, 0)
    m1, o1 = build(True)
    stepper = GraphedTrainStep(m1, o1)
    for _ in range(2):
        loss = stepper(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and all(st["step"] == 2 for st in o1.state.values())
    for (k, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p0, p1), k
    # and the steps moved the weights away from where two QuickGELU steps move them
    mq = _model(1, sd=sd).train()
    oq = BertAdam(prep_optim_params_groups(args, mq), lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98,
                  e=1e-6, max_grad_norm=1.0, capturable=False)
    train_epoch(0, args, mq, [batch] * 2, DEV, oq, 0)
    w = "clip.visual.transformer.resblocks.0.mlp.c_fc.weight"
    assert not torch.equal(dict(mq.named_parameters())[w], dict(m0.named_parameters())[w])
