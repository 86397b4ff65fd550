"""cluster_algo 'temporal_shift' / 'token_shift' without a GPU: module construction on the fixture plans, the packed plan and the
shapes it implies, the ctypes mirror of cc_cluster_variant, the op registration and the C entry points' argument checks."""
import ctypes
import json
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ALGOS = ("token_shift", "temporal_shift")


def _plans():
    return json.loads(str(np.load(os.path.join(GOLD, "shift_golden.npz"))["plans"]))


def _args(algo, frames, tokens, T=4):
    return Namespace(cluster_inter=1, cluster_algo=algo, max_frames=T, target_frames_blocks=frames,
                     cluster_num_blocks=tokens, cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False,
                     loose_type=True, sim_header='meanP', linear_patch='2d')


def _small_clip(algo, plan):
    from centerclip_amd.clip import CLIP
    frames, tokens = _plans()[plan]
    return CLIP(64, 64, 3, 128, 16, 16, 200, 128, 2, 2, video_frames=4, args=_args(algo, frames, tokens))


@pytest.mark.parametrize("algo", ALGOS)
def test_get_cluster_inter_builds_shift_modules_on_the_fixture_plans(algo):
    from centerclip_amd.cluster import get_cluster_inter
    fires = {"all": [True, True, True], "last": [False, False, True]}
    for plan, (frames, tokens) in _plans().items():
        mods = [get_cluster_inter(128, i + 1, _args(algo, frames, tokens)) for i in range(3)]
        assert [m is not None for m in mods] == fires[plan]
        for m in mods:
            if m is not None:
                assert m.algorithm == algo and m.is_shift and not m.is_default_variant
                assert m.original_frame == 4 and m.shift_fold_div == 8
                assert not list(m.parameters())


@pytest.mark.parametrize("algo", ALGOS)
def test_shift_plans_keep_frames_and_tokens(algo):
    for plan in ("all", "last"):
        vis = _small_clip(algo, plan).visual
        assert vis.final_shape(4) == (4, 17)
        assert vis._final_meta(4) == (4, 17, None)
        assert vis.shift_segment() == 4
        assert vis.frames_per_call(8, 4) == 4
        assert vis.frames_per_call(24, 12) == 4          # segments of original_frame whatever the caller's video_frame
        with pytest.raises(AssertionError):
            vis.frames_per_call(6, 6)                     # 6 frames are not a multiple of original_frame 4
        with pytest.raises(AssertionError):
            vis.frames_per_call(8, -1)                    # video_frame is required


def _packed(vis):
    """The cc_vit_model the fused encoder gets (without the device copies of the weights)."""
    from centerclip_amd._lib_clip import VitModel, CC_MAX_LAYERS
    from centerclip_amd import _lib as L
    m = VitModel()
    variants = (L.ClusterVariant * CC_MAX_LAYERS)()
    tokens = (vis.input_resolution // vis.patch_size) ** 2
    m.layers = vis.transformer.layers
    for i, blk in enumerate(vis.transformer.resblocks):
        tc = blk.tokencluster_inter
        if tc is not None:
            m.cluster_frames[i], m.cluster_tokens[i] = tc.original_frame, tokens
            variants[i], _ = tc.variant(tokens, "cpu")
    m.cluster_variants = ctypes.cast(variants, ctypes.c_void_p)
    return m, variants


@pytest.mark.parametrize("algo", ALGOS)
def test_variant_and_forced_medoids_count_ignore_shift_blocks(algo):
    from centerclip_amd import _lib as L
    L.lib()
    from centerclip_amd._lib_clip import VitModel  # noqa: F401  (declares the encoder entry points)
    vis = _small_clip(algo, "all").visual
    m, variants = _packed(vis)
    for i in range(3):
        assert variants[i].algorithm == {"temporal_shift": 4, "token_shift": 5}[algo]
        assert variants[i].shift_fold_div == 8 and variants[i].shift_segment == 4
        assert m.cluster_frames[i] == 4 and m.cluster_tokens[i] == 16
    assert L.lib().cc_vit_forced_medoids_count(ctypes.byref(m), 2) == 0


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "centerclip_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"((?:const\s+)?(?:struct\s+)?\w+\s*\**)\s*(.*)", decl).groups()
        for n in names.split(","):
            fields.append((typ.replace(" ", ""), n.strip()))
    return fields


def test_cluster_variant_ctypes_layout_matches_the_header():
    """Field names and order of _lib.ClusterVariant = cc_cluster_variant, the two shift fields appended at the end, and
    offsets as a C compiler lays the header's struct out (natural alignment)."""
    from centerclip_amd import _lib as L
    fields = _header_struct_fields("cc_cluster_variant")
    assert [n for _, n in fields] == [n for n, _ in L.ClusterVariant._fields_]
    assert [n for _, n in fields][-2:] == ["shift_fold_div", "shift_segment"]
    off = 0
    for (typ, name), (_, ct) in zip(fields, L.ClusterVariant._fields_):
        size = 8 if typ.endswith("*") else 4
        assert ctypes.sizeof(ct) == size, name
        off = (off + size - 1) // size * size
        assert getattr(L.ClusterVariant, name).offset == off, name
        off += size
    assert ctypes.sizeof(L.ClusterVariant) == (off + 7) // 8 * 8


def test_shift_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import centerclip_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        x = torch.empty(17, 8, 128)
        y = torch.ops.centerclip.token_shift(x, False, 4, 8, 5, False)
        assert y.shape == x.shape and y.dtype == torch.float32
        h = torch.empty(136, 128)
        assert torch.ops.centerclip.token_shift_rows(h, 1, 17, 8, 17, 4, 8, 4, torch.empty(136, 128, dtype=torch.float16),
                                                     torch.empty(136 * 2), 1, torch.empty(136)) is None


@pytest.mark.parametrize("algo", ALGOS)
def test_fake_vit_encode_gives_every_frame_for_a_shift_plan(algo):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from centerclip_amd import torch_ops as T
    vis = _small_clip(algo, "all").visual
    handle = T.register_model(None, dict(embed_dim=64, width=128, final=vis._final_meta), None)
    try:
        with FakeTensorMode():
            frames = torch.empty(8, 3, 64, 64)
            feats, hidden, med = torch.ops.centerclip.vit_encode(frames, handle, 2, 4, True, True, None)
            assert tuple(feats.shape) == (8, 64)
            assert tuple(hidden.shape) == (8, 17, 128)
            assert med.numel() == 0
    finally:
        T.release_model(handle)


def test_shift_entry_points_validate_arguments_without_a_gpu():
    from centerclip_amd import _lib as L
    lib = L.lib()
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its argument check first
    q = ctypes.c_void_p(1 << 20)
    W, Lt, F = 128, 5, 8
    args = lambda **k: dict(dict(x=p, ts=W, fs=Lt * W, F=F, L=Lt, W=W, seg=4, div=8, mode=5, adj=0, out=q, ots=W, ofs=Lt * W), **k)

    def call(a):
        return lib.cc_token_shift_f32(a["x"], a["ts"], a["fs"], a["F"], a["L"], a["W"], a["seg"], a["div"], a["mode"], a["adj"],
                                      a["out"], a["ots"], a["ofs"], None)
    for bad in (dict(x=None), dict(out=None), dict(seg=3), dict(seg=0), dict(F=0), dict(W=0), dict(L=0), dict(div=0),
                dict(mode=3), dict(mode=6), dict(adj=2),
                dict(ts=W - 1),                                   # tokens alias
                dict(fs=W * (Lt - 1)),                            # frames alias
                dict(ofs=W),                                      # out layout aliases
                dict(out=p, ofs=2 * Lt * W)):                     # in place with other strides
        assert call(args(**bad)) == -1, bad
    # the fused-row form: W % 4, W > 1024, slots, segment, LDS budget
    def rows(**k):
        a = dict(h=p, tr=1, fr=Lt, F=F, L=Lt, W=W, seg=4, div=8, mode=4, h16=q, st=q, slots=1, sh=q)
        a.update(k)
        return lib.cc_token_shift_rows_f32(a["h"], a["tr"], a["fr"], a["F"], a["L"], a["W"], a["seg"], a["div"], a["mode"],
                                           a["h16"], a["st"], a["slots"], a["sh"], None)
    for bad in (dict(h=None), dict(h16=None), dict(st=None), dict(sh=None), dict(W=130), dict(W=1028), dict(slots=0),
                dict(slots=33), dict(seg=3), dict(mode=0), dict(fr=Lt - 1)):
        assert rows(**bad) == -1, bad
    assert rows(seg=32, F=32, W=1024, div=2) == -2                # 32 frames x 1024 channels x 4 bytes > 64 KiB of LDS
    assert lib.cc_token_shift_rows_lds_bytes(60, 768, 8) == 60 * 192 * 4


def test_mean_residual_with_a_shift_is_refused():
    from centerclip_amd.cluster import TokenShiftInter
    with pytest.raises(NotImplementedError):
        TokenShiftInter(algorithm="token_shift", mean_residual=True)
    with pytest.raises(ValueError):
        TokenShiftInter(algorithm="kmediods++")


@pytest.mark.parametrize("algo", ALGOS)
def test_shift_modules_are_their_own_class(algo):
    """get_cluster_inter builds TokenShiftInter for the shift algorithms, with the arguments it passes TokenClusterInter;
    TokenClusterInter itself builds the clustering algorithms only and names the class that builds a shift."""
    from centerclip_amd.cluster import TokenClusterInter, TokenShiftInter, get_cluster_inter
    m = get_cluster_inter(128, 1, _args(algo, [2, 2, 2], [16, 15, 14]))
    assert type(m) is TokenShiftInter and m.block_id == 1 and m.before_block_frames == 4 and m.after_block_frames == 2
    with pytest.raises(NotImplementedError, match="TokenShiftInter"):
        TokenClusterInter(algorithm=algo)
