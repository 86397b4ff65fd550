"""CPU pins of the whole-model float64 oracle of the training step (oracle.clip_oracle: visual_forward / text_forward /
clip4clip_train_loss_native with native=True, contrastive_loss_and_grads with a dtype) that the full-size GPU step
(tests/test_train_full_gpu.py) is compared with: against the default fp32 oracle, and against the reference's own fp32
training step (tests/golden/r4_golden.npz tr_*, oracle/gen_golden_r4.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as co

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_PLAN = {1: (2, 6)}          # clip_golden's model: block 2 clusters 4 frames -> 2 segments of 6 tokens


@pytest.fixture(scope="module")
def r4():
    return np.load(os.path.join(GOLDEN, "r4_golden.npz"))


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _small_model():
    g = np.load(os.path.join(GOLDEN, "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k])
          for k in g.files if k.startswith("sd/")}
    B, T = int(g["cfg"][10]), int(g["cfg"][11])
    return g, sd, B, T


def test_native_whole_model_at_fp32_reproduces_the_fp32_oracle():
    """native=True run in fp32 with the selection the fp32 oracle made reproduces the default fp32 oracle (the forward
    fixtures' tolerance: conv1 is a GEMM here); return_medoids leaves the default results unchanged; the native path refuses
    a clustering block without a forced selection."""
    g, sd, B, T = _small_model()
    video, ids = torch.from_numpy(g["video"]), torch.from_numpy(g["t_ids"])
    feat, hidden, med = co.visual_forward(sd, video, T, cluster_plan=SMALL_PLAN, return_hidden=True, return_medoids=True)
    assert set(med) == {1} and tuple(med[1].shape) == (2 * B, 6)
    assert torch.equal(feat, co.visual_forward(sd, video, T, cluster_plan=SMALL_PLAN))
    nfeat, nhidden, nmed = co.visual_forward(sd, video, T, cluster_plan=SMALL_PLAN, forced_medoids=med, return_hidden=True,
                                             return_medoids=True, native=True)
    assert nfeat.dtype == torch.float32 and torch.equal(nmed[1], med[1])
    np.testing.assert_allclose(nfeat.numpy(), feat.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(nhidden.numpy(), hidden.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(co.text_forward(sd, ids, native=True).numpy(), co.text_forward(sd, ids).numpy(),
                               rtol=0, atol=2e-5)
    vid = video.view(B, 1, T, *video.shape[1:])
    vmask = torch.ones(B, 1, T, dtype=torch.long)
    want = co.clip4clip_train_loss(sd, ids[:B], vid, vmask, T, 2, SMALL_PLAN, float(sd["logit_scale"]))
    got, seq, vis = co.clip4clip_train_loss_native(sd, ids[:B], vid, vmask, T, 2, SMALL_PLAN, forced_medoids=med)
    assert got.dtype == torch.float32 and tuple(seq.shape) == (B, 1, 64) and tuple(vis.shape) == (B, 2, 64)
    assert abs(float(got) - float(want)) <= 2e-5 * max(1.0, abs(float(want)))
    with pytest.raises(ValueError):
        co.visual_forward(sd, video, T, cluster_plan=SMALL_PLAN, native=True)


def test_float64_whole_model_matches_reference_training_step(r4):
    """The float64 training step of the whole-model oracle, with the fp32 selection forced, against the reference's own fp32
    step (tr_*: the loss, the encode_image / encode_text features and torch.autograd's gradient of the 74 parameters that
    receive one): within 1e-4 of each tensor's largest entry (fp32 rounding of the fixture), exactly the same parameters
    reached, every gradient float64."""
    g, sd, B, T = _small_model()
    video, ids = torch.from_numpy(g["video"]), torch.from_numpy(g["t_ids"])[:B]
    _, med = co.visual_forward(sd, video, T, cluster_plan=SMALL_PLAN, return_medoids=True)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    loss, seq, vis = co.clip4clip_train_loss_native(p, ids, video.double().view(B, 1, T, *video.shape[1:]),
                                                    torch.ones(B, 1, T, dtype=torch.long), T, 2, SMALL_PLAN,
                                                    forced_medoids=med)
    loss.backward()
    assert loss.dtype == seq.dtype == vis.dtype == torch.float64
    errs = {"loss": abs(float(loss.detach()) - float(r4["tr_loss"])) / abs(float(r4["tr_loss"])),
            "vfeat": _rel(vis.detach().numpy().reshape(r4["tr_vfeat"].shape), r4["tr_vfeat"]),
            "tfeat": _rel(seq.detach().numpy().reshape(r4["tr_tfeat"].shape), r4["tr_tfeat"])}
    keys = [k[len("tr_grad/"):] for k in r4.files if k.startswith("tr_grad/")]
    assert len(keys) == 74 and "logit_scale" in keys
    assert {k for k, v in p.items() if v.grad is not None} == set(keys)
    for k in keys:
        assert p[k].grad.dtype == torch.float64
        errs[k] = _rel(p[k].grad.numpy().reshape(r4["tr_grad/" + k].shape), r4["tr_grad/" + k])
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("worst against the reference's fp32 step:", [(k, "%.1e" % e) for k, e in worst])
    assert worst[0][1] < 1e-4, worst


def test_contrastive_loss_dtype_argument():
    """contrastive_loss_and_grads in float64 agrees with its fp32 default (whose values tests/test_r3_gpu.py pins)."""
    from oracle.recipes import loss_grad_case
    seq, vis, vmask = loss_grad_case("lg_a", 6, 3, 64)
    s, v, m = torch.from_numpy(seq), torch.from_numpy(vis), torch.from_numpy(vmask)
    r32 = co.contrastive_loss_and_grads(s, v, m, 2.5)
    r64 = co.contrastive_loss_and_grads(s, v, m, 2.5, dtype=torch.float64)
    assert all(t.dtype == torch.float32 for t in r32) and all(t.dtype == torch.float64 for t in r64)
    for a, b in zip(r32, r64):
        assert _rel(a.numpy(), b.numpy()) < 1e-5
