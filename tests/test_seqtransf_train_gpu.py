"""sim_header 'seqTransf' end to end: the towers and the head together, in evaluation and in training, against float64.

* evaluation (cfg-2 shape, a padded clip): CLIP4Clip's own tower features -> get_similarity_logits (the strided segment mask
  after clustering, the head, the meanP tail) against the oracle towers (oracle.clip_oracle, float64 on the device, the HIP
  path's block-7 selection forced) composed with the head restatement tests/seqtransf_ref.py: <= 1e-3 on L2-normalised
  pooled features and on cosine similarities (logits / exp(logit_scale)), the project's parity contract (README).
* training: the cfg-2 step (ViT-B/32, 12 frames -> 3 segments at block 7, K = 49, B = 16, one padded clip) and a ViT-B/16
  step (cfg-5 shapes, B = 4) through CLIP4Clip.forward in .train() and loss.backward(), against float64 autograd of the oracle
  towers + the head restatement + oracle.clip_oracle.contrastive_loss_native, with the selection forced.  Every gradient is
  compared relative to its own largest entry, in_proj per q / k / v third, with the groups of tests/test_train_full_gpu.py
  and a new 'head' group (frame_position_embeddings, transformerClip).  The comparison helper must reject perturbed copies of
  the HIP gradients; GraphedTrainStep (captured) must give the same bits as eager steps.

Measured worst errors on an MI355X (relative to each tensor's largest entry, the loss to itself; the HIP path gives the same
bits run to run).  Each bound below (BOUNDS_* / FEAT_BOUNDS_*) is at most twice the measured worst and never above 2.5e-2.
                 patch    vis_embed vis_blocks vis_head txt_embed txt_blocks txt_head logit_scale head    | loss    seq     visual
  cfg 2, B = 16  1.38e-3  3.92e-3   7.22e-3    5.47e-3  3.87e-3   5.87e-3    3.04e-3  7.89e-5     9.20e-3 | 5.44e-8 7.26e-4 3.70e-4
  cfg 5, B = 4   1.47e-3  5.82e-3   1.11e-2    6.27e-3  3.46e-3   9.31e-3    4.51e-3  1.02e-3     1.23e-2 | 6.51e-7 7.72e-4 3.00e-4
The head's worst tensors are the k thirds of its in_proj weights (cfg 2: 9.2e-3, blocks 1-3; cfg 5: 1.23e-2): the head's
blocks multiply fp16 operands like the towers' (~2^-11 per operand), and a k-gradient is a difference of nearly equal terms
(dS sums to zero over the keys).  Evaluation through the towers: pooled 5.2e-5, cosine 6.7e-5 (bound 1e-3).
"""
import os
import sys

import pytest
import torch

import seqtransf_ref as ref
import test_train_full_gpu as full
from oracle import clip_oracle as clo

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 2.5e-2
LAYERS = 4
GROUPS = full.GROUPS + ("head",)


def _bench():
    return full._bench()


def _group(label):
    if label.startswith(("frame_position_embeddings.", "transformerClip.")):
        return "head"
    return full._group(label)


def compare_grads(hip, ref_g, bounds):
    """hip, ref {name: gradient}; bounds {group: bound} -> ({label: error}, [labels above their group's bound])."""
    errs = {}
    for name, r in ref_g.items():
        for (label, a), (_, b) in zip(full._pieces(name, hip[name].reshape(r.shape)), full._pieces(name, r)):
            # (an in_proj_bias k third has no gradient in exact arithmetic: measured against the whole tensor, as there)
            errs[label] = full._rel(a, b, r if label.endswith("in_proj_bias[k]") else None)
    bad = [k for k, e in errs.items() if not e <= bounds[_group(k)]]
    return errs, bad


def _model(cfg, seed_w, train):
    from centerclip_amd.clip4clip import CLIP4Clip
    b = _bench()
    args = b.task_config(cfg)
    args.sim_header, args.cross_num_hidden_layers = "seqTransf", LAYERS
    m = CLIP4Clip.from_state_dict(dict(b.random_state_dict(cfg, seed=seed_w)), args).to(DEV)
    with torch.no_grad():                        # a head that is not only the text blocks (the initialisation trick)
        g = torch.Generator().manual_seed(seed_w + 7)
        for p in list(m.transformerClip.parameters()) + [m.frame_position_embeddings.weight]:
            p.add_((torch.randn(p.shape, generator=g) * 0.02).to(DEV))
    return m.train() if train else m.eval()


def _ref_loss(model, cfg, ids, video, vmask, med, clip64, head64):
    """float64 oracle towers + head restatement + contrastive_loss_native -> (loss, seq, vis (before the head), segment mask)."""
    B, T, Tn = cfg["B"], cfg["T"], cfg["T_new"]
    plan = {cfg["cluster_block"] - 1: (Tn, cfg["K"])}
    vm = clo.video_mask_after_cluster(vmask.view(B, T), T, Tn).to(DEV)
    seq = clo.text_forward(clip64, ids.view(B, -1), native=True).view(B, 1, -1)
    vis = clo.visual_forward(clip64, video.double().reshape((-1,) + tuple(video.shape[3:])), T, cluster_plan=plan,
                             forced_medoids={cfg["cluster_block"] - 1: med}, native=True).view(B, Tn, -1)
    h = ref.head(vis, vm, head64["frame_position_embeddings.weight"], ref.blocks_from_state(head64, LAYERS),
                 model.transformerClip.heads)
    _, _, loss = clo.contrastive_loss_native(seq, h, vm, clip64["logit_scale"])
    return loss, seq, vis, vm, h


def _step(cfg, seed_w, seed_batch):
    model = _model(cfg, seed_w, train=True)
    ids, amask, video, vmask = _bench().synthetic_batch(cfg, DEV, seed=seed_batch)
    video = video.half().float()                              # the patch GEMM's input quantisation, for both sides
    assert int(vmask.sum()) < vmask.numel()

    def step():
        out = model(ids, torch.zeros_like(ids), amask, video, vmask)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out

    out = step()
    med = model.clip.visual.transformer.resblocks[cfg["cluster_block"] - 1].tokencluster_inter.last_medoids.clone()
    hip = {(k[5:] if k.startswith("clip.") else k): p.grad.detach().clone() for k, p in model.named_parameters()
           if p.grad is not None}
    clip64 = {k: v.detach().double().requires_grad_(True) for k, v in model.clip.named_parameters()}
    head64 = {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters() if not k.startswith("clip.")}
    loss64, seq64, vis64, _, _ = _ref_loss(model, cfg, ids, video, vmask, med, clip64, head64)
    loss64.backward()
    ref_g = {k: p.grad for k, p in list(clip64.items()) + list(head64.items()) if p.grad is not None}
    return dict(model=model, step=step, out=out, med=med, hip=hip, ref=ref_g, loss64=loss64.detach(), seq64=seq64.detach(),
                vis64=vis64.detach(), cfg=cfg, batch=(ids, amask, video, vmask))


def measure(s):
    """-> (worst error per group, loss, sequence_output and visual_output errors, {label: error})."""
    out = s["out"]
    errs, _ = compare_grads(s["hip"], s["ref"], {g: 0.0 for g in GROUPS})
    worst = {g: max(e for k, e in errs.items() if _group(k) == g) for g in GROUPS}
    e_loss = abs(float(out["loss"].detach()) - float(s["loss64"])) / abs(float(s["loss64"]))
    e_seq = full._rel(out["sequence_output"].detach(), s["seq64"])
    e_vis = full._rel(out["visual_output"].detach(), s["vis64"])
    return worst, dict(loss=e_loss, sequence_output=e_seq, visual_output=e_vis), errs


def _check_step(s, bounds, feat_bounds, tag):
    worst, feats, errs = measure(s)
    print(f"\n[{tag}] features", {k: "%.2e" % v for k, v in feats.items()})
    print(f"[{tag}] worst per group:", {g: "%.2e" % e for g, e in worst.items()})
    print(f"[{tag}] five worst tensors:", [(k, "%.2e" % e) for k, e in full._worst(errs)])
    assert all(feats[k] <= feat_bounds[k] for k in feats), feats
    bad = [k for k, e in errs.items() if not e <= bounds[_group(k)]]
    assert not bad, [(k, errs[k]) for k in bad]
    assert set(s["hip"]) == set(s["ref"]) and "logit_scale" in s["ref"]
    assert {k for k in s["hip"] if _group(k) == "head"} == {k for k, _ in s["model"].named_parameters() if not k.startswith("clip.")}


# per group: <= 2x the measured worst (module docstring), never above 2.5e-2
BOUNDS_CFG2 = dict(patch=2.7e-3, vis_embed=7.8e-3, vis_blocks=1.44e-2, vis_head=1.09e-2, txt_embed=7.7e-3, txt_blocks=1.17e-2,
                   txt_head=6e-3, logit_scale=1.5e-4, head=1.84e-2)
BOUNDS_CFG5 = dict(patch=2.9e-3, vis_embed=1.16e-2, vis_blocks=2.2e-2, vis_head=1.25e-2, txt_embed=6.9e-3, txt_blocks=1.86e-2,
                   txt_head=9e-3, logit_scale=2e-3, head=2.46e-2)
FEAT_BOUNDS_CFG2 = dict(loss=1e-7, sequence_output=1.45e-3, visual_output=7.3e-4)
FEAT_BOUNDS_CFG5 = dict(loss=1.3e-6, sequence_output=1.54e-3, visual_output=5.9e-4)
assert all(max(b.values()) <= CAP for b in (BOUNDS_CFG2, BOUNDS_CFG5, FEAT_BOUNDS_CFG2, FEAT_BOUNDS_CFG5))


@pytest.fixture(scope="module")
def cfg2_step():
    return _step(_bench().CFG2, seed_w=0, seed_batch=100)


def test_cfg2_seqtransf_training_step_against_float64(cfg2_step):
    _check_step(cfg2_step, BOUNDS_CFG2, FEAT_BOUNDS_CFG2, "cfg2 seqTransf")


def test_cfg2_seqtransf_comparison_rejects_perturbed_gradients(cfg2_step):
    """One head tensor scaled by 1 + 3 * bound, the gradients of head blocks 1 and 2 swapped, one head's rows of a head
    in_proj_weight's v part zeroed, and the position table's gradient shifted by one row: each is rejected."""
    hip, ref_g = cfg2_step["hip"], cfg2_step["ref"]
    assert not compare_grads(hip, ref_g, BOUNDS_CFG2)[1]
    name = "transformerClip.resblocks.2.mlp.c_fc.weight"
    scaled = dict(hip)
    scaled[name] = hip[name] * (1 + 3 * BOUNDS_CFG2["head"])
    assert compare_grads(scaled, ref_g, BOUNDS_CFG2)[1] == [name]
    swapped = dict(hip)
    for k in hip:
        if k.startswith("transformerClip.resblocks.1."):
            k2 = k.replace(".resblocks.1.", ".resblocks.2.")
            swapped[k], swapped[k2] = hip[k2], hip[k]
    bad = compare_grads(swapped, ref_g, BOUNDS_CFG2)[1]
    assert any(".resblocks.1." in k for k in bad) and any(".resblocks.2." in k for k in bad), bad
    name = "transformerClip.resblocks.0.attn.in_proj_weight"
    W = hip[name].shape[1]
    zeroed = dict(hip)
    zeroed[name] = hip[name].clone()
    zeroed[name][2 * W + 3 * 64:2 * W + 4 * 64] = 0
    assert compare_grads(zeroed, ref_g, BOUNDS_CFG2)[1] == [name + "[v]"]
    name = "frame_position_embeddings.weight"
    shifted = dict(hip)
    shifted[name] = torch.roll(hip[name], 1, 0)
    assert compare_grads(shifted, ref_g, BOUNDS_CFG2)[1] == [name]


def test_cfg2_seqtransf_training_step_is_deterministic_and_exact_where_it_must_be(cfg2_step):
    """A repeated step gives the same bits; position rows behind T_new get exactly zero gradient."""
    s = cfg2_step
    model = s["model"]
    g0 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=False)
    out = s["step"]()
    assert torch.equal(out["loss"].detach(), s["out"]["loss"].detach())
    for k, p in model.named_parameters():
        if k in g0:
            assert torch.equal(p.grad, g0[k]), k
    assert not model.frame_position_embeddings.weight.grad[s["cfg"]["T_new"]:].any()


def test_vit_b16_seqtransf_training_step_against_float64():
    cfg = dict(_bench().FORWARD_CFGS["cfg5"], B=4)
    s = _step(cfg, seed_w=1, seed_batch=101)
    _check_step(s, BOUNDS_CFG5, FEAT_BOUNDS_CFG5, "cfg5 B=4 seqTransf")


def test_graphed_train_step_equals_eager_steps_with_the_head():
    """Three captured steps (GraphedTrainStep) against three eager train_epoch steps, BertAdam and AdamW: every parameter,
    the head's included, bit for bit."""
    from argparse import Namespace
    from centerclip_amd.train import AdamW, BertAdam, GraphedTrainStep, prep_optim_params_groups, train_epoch
    cfg = dict(_bench().CFG2, B=8)
    ids, amask, video, vmask = _bench().synthetic_batch(cfg, "cpu", seed=5)
    batch = (ids, amask, torch.zeros_like(ids), video, vmask)
    args = Namespace(lr=1e-4, wd=0.2, new_added_modules=["Cross"], gradient_accumulation_steps=1, clip_grad_norm=None)
    for opt in ("bertadam", "adamw"):
        def make(capturable):
            m = _model(cfg, seed_w=2, train=True)
            groups = prep_optim_params_groups(args, m, coef_lr=1e-3)
            if opt == "bertadam":
                o = BertAdam(groups, lr=args.lr, warmup=0.2, t_total=20, schedule='warmup_linear', b1=0.9, b2=0.98, e=1e-6,
                             max_grad_norm=1.0, capturable=capturable)
            else:
                o = AdamW(groups, lr=args.lr, weight_decay=0.2, capturable=capturable)
            return m, o
        m0, o0 = make(False)
        train_epoch(0, args, m0, [batch] * 3, DEV, o0, 0)
        m1, o1 = make(True)
        stepper = GraphedTrainStep(m1, o1)
        for _ in range(3):
            loss = stepper(batch)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        moved = 0
        for (k, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
            assert torch.equal(p0, p1), (opt, k)
        h0 = _model(cfg, seed_w=2, train=True)
        for (k, p0), (_, ph) in zip(m0.named_parameters(), h0.named_parameters()):
            if not k.startswith("clip."):
                moved += int(not torch.equal(p0, ph))
        assert moved == 1 + 12 * LAYERS, moved                     # the head trained: every one of its tensors moved


def test_similarity_logits_through_the_towers_against_float64():
    """cfg 2 in .eval(): the model's own tower features (fused encoders, the padded clip's strided segment mask from
    get_video_mask_after_cluster) -> get_similarity_logits, against the oracle towers + the head restatement in float64."""
    cfg = _bench().CFG2
    model = _model(cfg, seed_w=3, train=False)
    ids, amask, video, vmask = _bench().synthetic_batch(cfg, DEV, seed=102)
    video = video.half().float()
    B, T = cfg["B"], cfg["T"]
    with torch.no_grad():
        out = model(ids, torch.zeros_like(ids), amask, video, vmask)
        vfeat, _ = model.clip.visual.encode(video.reshape((-1,) + tuple(video.shape[3:])), T, want_medoids=True)
        med = model.clip.visual.last_medoids.clone()
        assert torch.equal(vfeat.view(B, cfg["T_new"], -1), out["visual_output"])     # the same selection as the forward
        logits, _ = model.get_similarity_logits(out["sequence_output"], out["visual_output"], amask, vmask)
        vm = model.get_video_mask_after_cluster(vmask.view(B, T))
        head = model.seq_head(out["visual_output"], vm)
        clip64 = {k: v.detach().double() for k, v in model.clip.named_parameters()}
        head64 = {k: v.detach().double() for k, v in model.named_parameters() if not k.startswith("clip.")}
        _, seq64, _, vm64, h64 = _ref_loss(model, cfg, ids, video, vmask, med, clip64, head64)
    assert torch.equal(vm.cpu(), vm64.cpu()) and int(vm.sum()) < vm.numel()
    pooled, pooled64 = ref.pooled(head.double(), vm), ref.pooled(h64, vm64)
    t64 = seq64.squeeze(1) / seq64.squeeze(1).norm(dim=-1, keepdim=True)
    cos64 = t64 @ pooled64.t()
    dp = float((pooled - pooled64).abs().max())
    dc = float((logits.double() / torch.exp(model.clip.logit_scale.detach().double()) - cos64).abs().max())
    print("cfg2 towers + head: pooled %.2e  cosine %.2e" % (dp, dc))
    assert dp <= 1e-3 and dc <= 1e-3
