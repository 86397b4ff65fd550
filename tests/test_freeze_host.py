"""Host side of frozen-layer training (no GPU): CLIP4Clip.freeze_cip_layers against the reference's own frozen sets
(tests/golden/freeze_golden.json, tools/gen_golden_freeze.py), the optimizers' host logic with gradient-less parameters in
their groups, dist.GradientBuckets over gloo with a frozen subset, and which stages the training towers treat as a frozen
prefix."""
import json
import os
import socket
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from centerclip_amd import train as cctrain

HERE = os.path.dirname(os.path.abspath(__file__))
LAYER_NUMS = (-1, 0, 1, 2, 3, 6, 11, 12)


def _golden_clip():
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files
          if k.startswith("sd/")}
    return g, sd


def _cfg(T, linear_patch='2d', sim_header='meanP'):
    return Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=T, target_frames_blocks=[4, 2, 2],
                     cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                     minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                     sim_header=sim_header, linear_patch=linear_patch, cross_num_hidden_layers=1)


def _model(linear_patch='2d', sim_header='meanP'):
    from centerclip_amd.clip4clip import CLIP4Clip
    g, sd = _golden_clip()
    if sim_header == "seqTransf":
        # the head runs on the visual features and needs embed_dim == transformer_width: the two projection matrices of the
        # fixture model (64 columns) are widened to 128 - shapes only, the parameter names the test compares do not change
        for k in ("text_projection", "visual.proj"):
            sd[k] = torch.cat([sd[k], sd[k]], dim=1)
    if linear_patch == "3d":
        sd["visual.conv2.weight"] = sd["visual.conv1.weight"].unsqueeze(2).repeat(1, 1, 3, 1, 1)
    return CLIP4Clip.from_state_dict(sd, _cfg(int(g["cfg"][11]), linear_patch, sim_header)).float()


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "freeze_golden.json")) as f:
        return json.load(f)


def test_fixture_covers_the_cases(gold):
    assert set(gold) == {"%d|%s|%s" % (k, p, h) for k in LAYER_NUMS for p in ("2d", "3d") for h in ("meanP", "seqTransf")}
    assert len(gold["0|2d|meanP"]) == 7 and gold["-1|2d|meanP"] == []


@pytest.mark.parametrize("sim_header", ["meanP", "seqTransf"])
@pytest.mark.parametrize("linear_patch", ["2d", "3d"])
@pytest.mark.parametrize("k", LAYER_NUMS)
def test_freeze_cip_layers_reproduces_the_reference(gold, k, linear_patch, sim_header):
    model = _model(linear_patch, sim_header)
    assert all(p.requires_grad for p in model.parameters())
    model.freeze_cip_layers(k)
    frozen = sorted(n for n, p in model.named_parameters() if not p.requires_grad)
    assert frozen == gold["%d|%s|%s" % (k, linear_patch, sim_header)]
    if sim_header == "seqTransf":
        assert all(p.requires_grad for n, p in model.named_parameters() if not n.startswith("clip."))


@pytest.mark.parametrize("bad", [13, -2])
def test_freeze_cip_layers_refuses_layer_numbers_out_of_range(bad):
    model = _model()
    with pytest.raises(AssertionError):
        model.freeze_cip_layers(bad)
    assert all(p.requires_grad for p in model.parameters())


def test_frozen_prefix_stages():
    """The towers' frozen prefix: None with a trainable front end, else the number of leading fully frozen blocks."""
    model = _model()
    clip = model.clip
    assert cctrain.visual_prefix_blocks(clip.visual) is None and cctrain.text_prefix_blocks(clip) is None
    model.freeze_cip_layers(0)
    assert cctrain.visual_prefix_blocks(clip.visual) == 0 and cctrain.text_prefix_blocks(clip) == 0
    model.freeze_cip_layers(1)
    assert cctrain.visual_prefix_blocks(clip.visual) == 1 and cctrain.text_prefix_blocks(clip) == 1
    model.freeze_cip_layers(12)                                     # 3 visual blocks, 2 text blocks: all of them
    assert cctrain.visual_prefix_blocks(clip.visual) == 3 and cctrain.text_prefix_blocks(clip) == 2
    # a trainable parameter inside a stage ends the prefix there; a frozen block behind a trainable one is not part of it
    clip.visual.transformer.resblocks[1].ln_2.bias.requires_grad = True
    assert cctrain.visual_prefix_blocks(clip.visual) == 1
    clip.visual.ln_pre.weight.requires_grad = True
    assert cctrain.visual_prefix_blocks(clip.visual) is None
    clip.positional_embedding.requires_grad = True
    assert cctrain.text_prefix_blocks(clip) is None
    # behind the cluster block (index 1: 4 frames -> 2 segments of 6 tokens) the prefix hands over the clustered shape
    assert clip.visual.prefix_shape(4, 1) == (4, 17, 0) and clip.visual.prefix_shape(4, 2) == (2, 7, 12)


def _params():
    torch.manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(6)), torch.nn.Parameter(torch.randn(2, 2))]
    ps[1].requires_grad = False                                     # frozen: in the group, never a gradient
    return ps


@pytest.mark.parametrize("name", ["BertAdam", "AdamW"])
def test_optimizers_keep_no_state_for_parameters_without_a_gradient(name):
    """The reference's groups hold the frozen parameters too (utils/optimization.py does not filter on requires_grad).  The
    host pass that collects a step's tensors runs up to the first device check: a parameter with a gradient on the CPU is
    refused there, one without a gradient is never looked at - no state entry."""
    ps = _params()
    groups = [{'params': ps[:2], 'weight_decay': 0.1}, {'params': ps[2:], 'weight_decay': 0.0}]
    opt = cctrain.BertAdam(groups, lr=1e-3) if name == "BertAdam" else cctrain.AdamW(groups, lr=1e-3)
    opt.step()                                                      # no gradient anywhere: nothing to do, no state
    assert len(opt.state) == 0
    if name == "AdamW":
        assert float(opt.clip_and_step(1.0)) == 0.0 and len(opt.state) == 0
    assert float(cctrain.clip_grad_norm_(ps, 1.0)) == 0.0
    ps[1].grad = None
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(RuntimeError):                               # the CPU gradient is refused ...
        opt.step()
    assert ps[1] not in opt.state and ps[2] not in opt.state        # ... and the gradient-less ones got no entry


def test_adamw_state_dict_with_frozen_parameters_round_trips_with_torch():
    """A state in which the frozen parameter has no entry loads from and into torch.optim.AdamW."""
    ps = _params()
    mk = lambda cls, p: cls([{'params': p[:2], 'weight_decay': 0.1}, {'params': p[2:], 'weight_decay': 0.0}], lr=1e-3)
    ref = mk(torch.optim.AdamW, ps)
    for p in (ps[0], ps[2]):
        p.grad = torch.full_like(p, 0.5)
    ref.step()
    sd = ref.state_dict()
    assert sorted(sd["state"]) == [0, 2]                            # torch keeps no state for the frozen one either
    ours = mk(cctrain.AdamW, _params())
    ours.load_state_dict(sd)
    mine = ours.state_dict()
    assert sorted(mine["state"]) == [0, 2] and all(mine["state"][i]["step"] == 1 for i in (0, 2))
    for i in (0, 2):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(mine["state"][i][k], sd["state"][i][k])
    back = mk(torch.optim.AdamW, _params())
    back.load_state_dict(mine)
    assert sorted(back.state_dict()["state"]) == [0, 2]


def test_graphed_step_snapshot_leaves_frozen_parameters_alone():
    ps = _params()
    opt = cctrain.AdamW([{'params': ps}], lr=1e-3, capturable=True)
    holder = torch.nn.Module()
    holder.ps = torch.nn.ParameterList(ps)
    step = cctrain.GraphedTrainStep(holder, opt)
    assert [id(p) for p in step._tensors()] == [id(ps[0]), id(ps[2])]
    v = ps[1]._version
    step._restore(step._snapshot())
    assert ps[1]._version == v and ps[0]._version > 0


# ------------------------------------------------------------------------------------------ gloo world-2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, case_frozen_buckets(rank, world)))
    finally:
        dist.destroy_process_group()


def _grads(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return [torch.randn(5, 3, generator=g), torch.randn(7, generator=g), torch.randn(2, 4, generator=g)]


def case_frozen_buckets(rank, world):
    from centerclip_amd.dist import GradientBuckets
    ps = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7)), torch.nn.Parameter(torch.zeros(2, 4))]
    ps[1].requires_grad = False                                     # the same frozen subset on both ranks
    buckets = GradientBuckets(ps, bucket_bytes=64)                  # several buckets
    ok = all(id(p) != id(ps[1]) for p in buckets.params)
    for _ in range(2):
        for i in (0, 2):
            ps[i].grad = _grads(rank)[i].clone()
        buckets.reduce()
        want = [sum(_grads(r)[i] for r in range(world)) / world for i in range(3)]
        ok = ok and ps[1].grad is None
        ok = ok and all(torch.allclose(ps[i].grad, want[i], atol=1e-6) for i in (0, 2))
    return bool(ok)


def test_gradient_buckets_skip_frozen_parameters_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == {0: True, 1: True}


def test_fixture_medoids_are_what_the_reference_picked():
    """tests/test_freeze_gpu.py imposes v_medoids of clip_golden.npz where the k-medoids block lies inside the frozen prefix.
    They are the reference's own selection: the oracle's tower (pinned to the reference's features by
    tests/test_oracle_clip.py) picks exactly these ids itself, and gives the same features with them forced."""
    from oracle import clip_oracle as clo
    g, sd = _golden_clip()
    video, T = torch.from_numpy(g["video"]), int(g["cfg"][11])
    own, picked = clo.visual_forward(sd, video, T, cluster_plan={1: (2, 6)}, return_medoids=True)
    assert sorted(picked) == [1] and np.array_equal(picked[1].numpy(), g["v_medoids"])
    forced = clo.visual_forward(sd, video, T, cluster_plan={1: (2, 6)}, forced_medoids={1: torch.from_numpy(g["v_medoids"])})
    np.testing.assert_allclose(own.numpy(), g["v_feat"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(forced.numpy(), own.numpy(), rtol=0, atol=1e-6)
