"""CPU oracle for the CLIP forward / similarity rows of the hot path.

TEST INFRASTRUCTURE ONLY (see oracle/cluster_oracle.py for the rules).  Plain PyTorch fp32,
functional, driven by a state dict with the reference's key names.  Pinned against
the imported reference by tests/golden/clip_golden.npz (oracle/gen_golden.py clip).

Citations are relative to /root/reference.
"""
import math

import torch
import torch.nn.functional as F

from . import cluster_oracle as co


# constants of the reference's loader, dataloaders/decode.py:43-48
PIXEL_MEAN = (0.48145466, 0.4578275, 0.40821073)
PIXEL_STD = (0.26862954, 0.26130258, 0.27577711)


def loader_normalize(frames_u8, channels_last=False, mean=PIXEL_MEAN, std=PIXEL_STD):
    """What the reference's evaluation loader makes of decoded uint8 frames:
    HWC -> CHW permute (dataloaders/transforms.py:157), ``img.float().div_(255)`` (:166,
    GroupToTensorBCHW(div=True)), then TensorNormalize (:19-34) = torchvision
    ``functional.normalize``: ``tensor.sub_(mean[:,None,None]).div_(std[:,None,None])`` with the
    constants as fp32 tensors.  torchvision is a third-party dependency that is absent from this
    image (so dataloaders/transforms.py cannot be imported: parity of this row is pinned by
    this restatement of its published two-line algorithm, checked against plain IEEE numpy
    arithmetic in tests/test_oracle_clip.py, not by reference-generated fixtures).
    frames_u8 [N,3,H,W] or [N,H,W,3] uint8 -> [N,3,H,W] fp32."""
    x = torch.as_tensor(frames_u8)
    if channels_last:
        x = x.permute(0, 3, 1, 2)
    x = x.contiguous().float().div_(255.0)
    m = torch.as_tensor(mean, dtype=torch.float32)[None, :, None, None]
    sd = torch.as_tensor(std, dtype=torch.float32)[None, :, None, None]
    return x.sub_(m).div_(sd)


def layer_norm(x, w, b, eps=1e-5, native=False):
    """modules/clip.py:183-189: nn.LayerNorm evaluated in fp32.  native: in x's own dtype and on its device (a float64
    reference for the backward: autograd through it gives float64 gradients)."""
    if native:
        return F.layer_norm(x, (x.shape[-1],), w.to(x), b.to(x), eps)
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps)


def quick_gelu(x):
    """modules/clip.py:192-194."""
    return x * torch.sigmoid(1.702 * x)


def mha(x, sd, pre, heads, causal, native=False):
    """nn.MultiheadAttention forward on [N, L, W] (batch first here; the reference feeds LND,
    clip.py:205,220-226): packed in_proj (rows q,k,v), heads = contiguous W/heads slices,
    softmax(q k^T / sqrt(d) + mask) v, out_proj.  native: see layer_norm."""
    N, L, W = x.shape
    d = W // heads
    c = (lambda t: t.to(x)) if native else (lambda t: t.float())
    qkv = x @ c(sd[pre + "attn.in_proj_weight"]).t() + c(sd[pre + "attn.in_proj_bias"])
    q, k, v = qkv.split(W, dim=-1)
    q = q.view(N, L, heads, d).transpose(1, 2)
    k = k.view(N, L, heads, d).transpose(1, 2)
    v = v.view(N, L, heads, d).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(d)
    if causal:                                             # clip.py:448-454
        s = s + (torch.full((L, L), float("-inf"), dtype=s.dtype, device=s.device) if native
                 else torch.full((L, L), float("-inf"))).triu_(1)
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(N, L, W)
    return o @ c(sd[pre + "attn.out_proj.weight"]).t() + c(sd[pre + "attn.out_proj.bias"])


def resblock(x, sd, pre, heads, causal, res_x=None, native=False):
    """ResidualAttentionBlock without the cluster hook (clip.py:240,251), x [N, L, W]; res_x: the residual the cluster
    module handed back (mean_residual, clip.py:239-242) - the attention branch is added to it instead of to x.
    native: see layer_norm."""
    c = (lambda t: t.to(x)) if native else (lambda t: t.float())
    x = (x if res_x is None else res_x) + mha(layer_norm(x, sd[pre + "ln_1.weight"], sd[pre + "ln_1.bias"], native=native), sd,
                                              pre, heads, causal, native=native)
    h = layer_norm(x, sd[pre + "ln_2.weight"], sd[pre + "ln_2.bias"], native=native)
    h = quick_gelu(h @ c(sd[pre + "mlp.c_fc.weight"]).t() + c(sd[pre + "mlp.c_fc.bias"]))
    return x + h @ c(sd[pre + "mlp.c_proj.weight"]).t() + c(sd[pre + "mlp.c_proj.bias"])


def block_backward64(x_lnd, dz_lnd, sd, heads, causal):
    """The float64 reference of one block's forward and backward on its own device: x, dz [L, N, W] LND, sd the 12 parameter
    tensors under the reference's names -> (z [L, N, W], dx [L, N, W], {name: gradient}), torch.autograd through resblock."""
    x = x_lnd.detach().to(torch.float64).permute(1, 0, 2).contiguous().requires_grad_(True)
    p = {k: v.detach().to(device=x.device, dtype=torch.float64).requires_grad_(True) for k, v in sd.items()}
    z = resblock(x, p, "", heads, causal, native=True)
    (z * dz_lnd.detach().to(x).permute(1, 0, 2)).sum().backward()
    return z.detach().permute(1, 0, 2), x.grad.permute(1, 0, 2), {k: v.grad for k, v in p.items()}


def bertadam_step64(p, g, m, v, lr_scheduled, b1, b2, e, weight_decay, max_grad_norm):
    """utils/optimization.py:100-170, one step on one tensor in float64 (in place on p, g, m, v, which are float64 tensors):
    clip_grad_norm_(p, max_grad_norm) rescales g by max / (||g|| + 1e-6) when that is < 1, then the moments, the update
    m / (sqrt(v) + e) (+ weight_decay * p) and p -= lr_scheduled * update.  No bias correction."""
    if max_grad_norm > 0:
        coef = max_grad_norm / (float(g.norm()) + 1e-6)
        if coef < 1:
            g.mul_(coef)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    upd = m / (v.sqrt() + e)
    if weight_decay > 0.0:
        upd += weight_decay * p
    p.add_(-lr_scheduled * upd)


def visual_forward(sd, video, T, cluster_plan=None, cluster_cfg=None, forced_medoids=None, return_hidden=False,
                   linear_patch='2d', mean_residual=(), native=False, return_medoids=False):
    """VisualTransformer.forward + the ln_post/proj tail of CLIP.encode_image
    (clip.py:304-349,460-469).  video [B*T,3,H,W]; cluster_plan {block_index(0-based): (T_new, K)};
    cluster_cfg dict(distance, threshold, iter_limit, norm_p, split_size, pre_norm[, algorithm, aggregation]).
    forced_medoids {block_index: int64 [T_new*B, K]} replaces the k-medoids result (to compare
    embeddings "given identical medoid sets").  mean_residual: block indices whose cluster module has
    mean_residual set (cluster.py:228-235: residual = the mean over each segment's frames of EVERY token, CLS included; the
    token count must not change).  Returns features [B*T_final, E] (and the hidden state [B*T_final, L, W]).
    return_medoids: also return {block_index: medoid ids [T_new*B, K]} (last item): the selections the default k-medoids
    blocks made here, and in native mode the forced ones.
    native: the whole tower in video's dtype and on its device, differentiable with respect to every tensor of sd (a
    float64 reference of the training backward); the conv1 patch embedding is the equal reshape + GEMM, and every
    k-medoids block must be given its selection in forced_medoids (the reference selects under no_grad, fast_kmeans.py:13,44:
    the selection is a constant of the backward).  Only linear_patch '2d' with plain medoid gathers."""
    W = sd["visual.conv1.weight"].shape[0]
    p = sd["visual.conv1.weight"].shape[-1]
    heads = W // 64
    layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    if native:
        return _visual_forward_native(sd, video, T, cluster_plan or {}, forced_medoids or {}, return_hidden, return_medoids,
                                      W, p, heads, layers, linear_patch, cluster_cfg, mean_residual)
    picked_ids = {}
    if linear_patch == '3d':                                                           # clip.py:306-319
        x3 = video.float().reshape(-1, T, video.shape[-3], video.shape[-2], video.shape[-1]).permute(0, 2, 1, 3, 4)
        x3 = F.conv3d(x3, sd["visual.conv2.weight"].float(), stride=(1, p, p), padding=(1, 0, 0)).permute(0, 2, 1, 3, 4)
        x = x3.reshape(-1, x3.shape[-3], x3.shape[-2], x3.shape[-1])
    else:
        x = F.conv2d(video.float(), sd["visual.conv1.weight"].float(), stride=p)      # clip.py:324
    x = x.reshape(x.shape[0], W, -1).permute(0, 2, 1)                                  # [BT, n, W]
    cls = sd["visual.class_embedding"].float().expand(x.shape[0], 1, W)
    x = torch.cat([cls, x], dim=1) + sd["visual.positional_embedding"].float()         # :334-336
    x = layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])            # :338
    frames = T
    cluster_plan = cluster_plan or {}
    for i in range(layers):
        res_x = None
        if i in cluster_plan:                                                           # :236-242
            T_new, K = cluster_plan[i]
            x_lnd = x.permute(1, 0, 2).contiguous()
            if i in mean_residual:                                                      # cluster.py:228-235
                Lt, BT, _ = x_lnd.shape
                assert Lt == K + 1
                r = x_lnd.reshape(Lt, BT // frames, frames, W)
                r = torch.stack([it.mean(dim=2) for it in torch.split(r, frames // T_new, dim=2)], dim=2)
                res_x = r.contiguous().reshape(Lt, (BT // frames) * T_new, W).permute(1, 0, 2).contiguous()
            if forced_medoids is not None and i in forced_medoids:
                x_lnd = gather_with_medoids(x_lnd, frames, T_new, forced_medoids[i])
            elif (cluster_cfg or {}).get("algorithm", "kmediods++") != "kmediods++" or \
                    (cluster_cfg or {}).get("aggregation") not in [None, "None"]:
                c = cluster_cfg                                                         # N2 variants
                x_lnd = co.literal_token_cluster_variant(x_lnd, frames, T_new, K, c.get("algorithm", "kmediods++"),
                                                         c.get("aggregation"), None, None,
                                                         c.get("distance", "euclidean"), c.get("threshold", 1e-6),
                                                         c.get("iter_limit", 100), c.get("norm_p", 2.0),
                                                         c.get("split_size", 16), c.get("pre_norm", False))
            else:
                c = cluster_cfg or {}
                x_lnd, picked_ids[i], _ = co.literal_token_cluster(x_lnd, frames, T_new, K, c.get("distance", "euclidean"),
                                                                   c.get("threshold", 1e-6), c.get("iter_limit", 100),
                                                                   c.get("norm_p", 2.0), c.get("split_size", 16),
                                                                   c.get("pre_norm", False), return_ids=True)
            x = x_lnd.permute(1, 0, 2).contiguous()
            frames = T_new
        x = resblock(x, sd, "visual.transformer.resblocks.%d." % i, heads, causal=False, res_x=res_x)
    feat = layer_norm(x[:, 0, :], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"].float()
    out = (feat, x) if return_hidden else (feat,)
    if return_medoids:
        out = out + (picked_ids,)
    return out if len(out) > 1 else out[0]


def _visual_forward_native(sd, video, T, cluster_plan, forced_medoids, return_hidden, return_medoids, W, p, heads, layers,
                           linear_patch, cluster_cfg, mean_residual):
    """visual_forward(native=True): the same op sequence in video's dtype, on its device."""
    if linear_patch != '2d' or mean_residual:
        raise NotImplementedError("native visual_forward: linear_patch '2d' without mean_residual only")
    c = cluster_cfg or {}
    if c.get("algorithm", "kmediods++") != "kmediods++" or c.get("aggregation") not in [None, "None"]:
        raise NotImplementedError("native visual_forward: k-medoids with medoid gathers only")
    cv = lambda t: t.to(video)
    F_, g = video.shape[0], video.shape[-1] // p
    # conv1 (kernel = stride = p, no bias, clip.py:324) as the GEMM over the (c, kh, kw) patch rows it is
    a = video.reshape(F_, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F_, g * g, 3 * p * p)
    x = a @ cv(sd["visual.conv1.weight"]).reshape(W, -1).t()                            # [BT, n, W]
    cls = cv(sd["visual.class_embedding"]).expand(x.shape[0], 1, W)
    x = torch.cat([cls, x], dim=1) + cv(sd["visual.positional_embedding"])             # :334-336
    x = layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"], native=True)
    frames, picked_ids = T, {}
    for i in range(layers):
        if i in cluster_plan:
            T_new, K = cluster_plan[i]
            if i not in forced_medoids:
                raise ValueError("native visual_forward: block %d clusters; give its selection in forced_medoids" % i)
            med = forced_medoids[i].to(device=video.device, dtype=torch.long)
            assert tuple(med.shape) == (T_new * (x.shape[0] // frames), K), (tuple(med.shape), T_new, K)
            x = gather_with_medoids(x.permute(1, 0, 2), frames, T_new, med, native=True).permute(1, 0, 2)
            picked_ids[i] = med
            frames = T_new
        x = resblock(x, sd, "visual.transformer.resblocks.%d." % i, heads, causal=False, native=True)
    feat = layer_norm(x[:, 0, :], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"], native=True) @ cv(sd["visual.proj"])
    out = (feat, x) if return_hidden else (feat,)
    if return_medoids:
        out = out + (picked_ids,)
    return out if len(out) > 1 else out[0]


def gather_with_medoids(x_lnd, T, T_new, medoids, native=False):
    """The gather / CLS-mean half of TokenClusterInter.forward with given medoid ids
    (modules/cluster/cluster.py:287-289,303-310).  native: the row index is made on x's device (differentiable either way)."""
    tokens, cls = co.regroup_segments(x_lnd, T, T_new)
    P, _, W = tokens.shape
    B, fd, K = P // T_new, T // T_new, medoids.shape[1]
    rows = torch.arange(P, device=tokens.device) if native else torch.arange(P)
    picked = tokens[rows.unsqueeze(-1), medoids.to(tokens.device) if native else medoids]
    picked = picked.reshape(T_new, B, K, W).permute(1, 0, 2, 3).reshape(B * T_new, K, W)
    seg_cls = torch.stack([c.mean(dim=1) for c in torch.split(cls, fd, dim=1)], dim=1).reshape(B * T_new, 1, W)
    return torch.cat([seg_cls, picked], dim=1).permute(1, 0, 2).contiguous()


def text_forward(sd, ids, native=False):
    """CLIP.encode_text (clip.py:471-496): embed + positional, 12 causal blocks, ln_final,
    text_projection, row at the first argmax of the ids.  native: in the dtype of sd's token embedding and on its device
    (ids are moved there), differentiable with respect to every tensor of sd."""
    W = sd["ln_final.weight"].shape[0]
    heads = W // 64
    layers = len(set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")))
    if native:
        emb = sd["token_embedding.weight"]
        ids = ids.to(emb.device)
        x = emb[ids] + sd["positional_embedding"].to(emb)[:ids.shape[1]]
    else:
        x = sd["token_embedding.weight"].float()[ids] + sd["positional_embedding"].float()[:ids.shape[1]]
    for i in range(layers):
        x = resblock(x, sd, "transformer.resblocks.%d." % i, heads, causal=True, native=native)
    proj = sd["text_projection"].to(x) if native else sd["text_projection"].float()
    x = layer_norm(x, sd["ln_final.weight"], sd["ln_final.bias"], native=native) @ proj
    return x[torch.arange(x.shape[0], device=x.device if native else None), ids.argmax(dim=-1)]


def video_mask_after_cluster(video_mask, max_frames, final_frames):
    """clip4clip.py:436-447: a segment inherits the mask of its last frame."""
    fd = max_frames // final_frames
    inds = torch.arange(fd - 1, video_mask.shape[-1], video_mask.shape[-1] // final_frames, device=video_mask.device)
    return video_mask[:, inds]


def mean_pool_visual(visual, video_mask):
    """clip4clip.py:305-316 preceded/followed by the L2 normalisations of :357-360."""
    v = visual / visual.norm(dim=-1, keepdim=True)
    m = video_mask.to(torch.float).unsqueeze(-1)
    s = torch.sum(m, dim=1, dtype=torch.float)
    s[s == 0.] = 1.
    v = torch.sum(v * m, dim=1) / s
    return v / v.norm(dim=-1, keepdim=True)


def loose_similarity(sequence_output, visual_output, video_mask, logit_scale):
    """clip4clip.py:357-366 (meanP, eval branch): exp(logit_scale) * t_hat @ v_bar^T."""
    v = mean_pool_visual(visual_output.float(), video_mask)
    t = sequence_output.float().squeeze(1)
    t = t / t.norm(dim=-1, keepdim=True)
    return math.exp(float(logit_scale)) * torch.matmul(t, v.t())


def similarity_matrix_blocked(seq_batches, vis_batches, mask_batches, logit_scale):
    """main.py:502-534 (_run_on_single_gpu): text-batch x video-batch blocks concatenated."""
    rows = []
    for t in seq_batches:
        rows.append(torch.cat([loose_similarity(t, v, m, logit_scale) for v, m in zip(vis_batches, mask_batches)], dim=-1))
    return torch.cat(rows, dim=0)


def cross_en(sim_matrix):
    """modules/losses.py:8-18: mean over rows of -log_softmax(sim, -1)[i, i]."""
    return -torch.diag(F.log_softmax(sim_matrix.float(), dim=-1)).mean()


def clip4clip_forward(sd, ids, video, video_mask, max_frames, final_frames, cluster_plan, logit_scale,
                      pre_visual_pooling=False, forced_medoids=None):
    """CLIP4Clip.forward (eval branch) followed by get_similarity_logits (modules/clip4clip.py:199-243,412-434) for the
    meanP head: ids [B, 1, L] (or [B, L]), video [B, 1, T, 3, H, W], video_mask [B, 1, T] ->
    (sequence_output [B, 1, E], visual_output [B, T_new, E] or pooled [B, E], logits [B, B])."""
    ids = ids.view(-1, ids.shape[-1])
    T = video.shape[2]
    v = video.reshape((-1,) + tuple(video.shape[3:])).float()
    vmask = video_mask.view(-1, video_mask.shape[-1])
    if cluster_plan:
        vmask = video_mask_after_cluster(vmask, max_frames, final_frames)
    seq = text_forward(sd, ids).view(ids.shape[0], 1, -1)
    vis = visual_forward(sd, v, T, cluster_plan=cluster_plan, forced_medoids=forced_medoids).view(vmask.shape[0], -1, seq.shape[-1])
    if pre_visual_pooling:
        pooled = mean_pool_visual(vis, vmask)
        t = seq.squeeze(1)
        t = t / t.norm(dim=-1, keepdim=True)
        return seq, pooled, math.exp(float(logit_scale)) * torch.matmul(t, pooled.t())
    return seq, vis, loose_similarity(seq, vis, vmask, logit_scale)


def clip4clip_train_loss(sd, ids, video, video_mask, max_frames, final_frames, cluster_plan, logit_scale):
    """The loss of the training branch at world size 1 (clip4clip.py:245-262): (CrossEn(sim) + CrossEn(sim^T)) / 2."""
    _, _, sim = clip4clip_forward(sd, ids, video, video_mask, max_frames, final_frames, cluster_plan, logit_scale)
    return (cross_en(sim) + cross_en(sim.t())) / 2


def clip4clip_train_loss_native(sd, ids, video, video_mask, max_frames, final_frames, cluster_plan, forced_medoids=None):
    """clip4clip_train_loss with native towers (visual_forward / text_forward native=True): in video's dtype and on its
    device, differentiable with respect to every tensor of sd, logit_scale (sd['logit_scale']) included; each k-medoids
    block's selection is given in forced_medoids.  ids [B, L], video [B, 1, T, 3, H, W], video_mask [B, 1, T] ->
    (loss, sequence_output [B, 1, E], visual_output [B, T', E])."""
    ids = ids.view(-1, ids.shape[-1])
    T = video.shape[2]
    v = video.reshape((-1,) + tuple(video.shape[3:]))
    vmask = video_mask.view(-1, video_mask.shape[-1]).to(video.device)
    if cluster_plan:
        vmask = video_mask_after_cluster(vmask, max_frames, final_frames)
    seq = text_forward(sd, ids, native=True).view(ids.shape[0], 1, -1)
    vis = visual_forward(sd, v, T, cluster_plan=cluster_plan, forced_medoids=forced_medoids, native=True)
    vis = vis.view(vmask.shape[0], -1, seq.shape[-1])
    _, _, loss = contrastive_loss_native(seq, vis, vmask, sd["logit_scale"].to(v))
    return loss, seq, vis


def _cross_en_native(sim):
    """cross_en in sim's own dtype."""
    return -torch.diag(F.log_softmax(sim, dim=-1)).mean()


def contrastive_loss_native(sequence_output, visual_output, video_mask, logit_scale):
    """The training branch's loss (clip4clip.py:245-262: the meanP similarity of :357-366, CrossEn both ways) in the
    features' dtype and on their device, differentiable in the features and in logit_scale (a tensor) ->
    (CrossEn(S), CrossEn(S^T), their mean)."""
    v = visual_output / visual_output.norm(dim=-1, keepdim=True)
    m = video_mask.to(device=v.device, dtype=v.dtype).unsqueeze(-1)
    den = torch.sum(m, dim=1)
    den = torch.where(den == 0., torch.ones_like(den), den)
    v = torch.sum(v * m, dim=1) / den
    v = v / v.norm(dim=-1, keepdim=True)
    t = sequence_output.reshape(sequence_output.shape[0], -1)
    t = t / t.norm(dim=-1, keepdim=True)
    sim = logit_scale.exp() * torch.matmul(t, v.t())
    l1, l2 = _cross_en_native(sim), _cross_en_native(sim.t())
    return l1, l2, (l1 + l2) / 2


def contrastive_loss_and_grads(sequence_output, visual_output, video_mask, logit_scale, dtype=torch.float32):
    """The training branch's loss (clip4clip.py:245-262) and torch.autograd's gradients of it with respect to
    sequence_output, visual_output and logit_scale, evaluated in dtype on the features' device (float64: the reference of
    the GPU tests at training batch sizes) -> (loss3 [CrossEn(S), CrossEn(S^T), mean], d_seq, d_vis, d_logit_scale)."""
    seq = sequence_output.detach().clone().to(dtype).requires_grad_(True)
    vis = visual_output.detach().clone().to(dtype).requires_grad_(True)
    ls = torch.tensor(float(logit_scale), dtype=dtype, device=seq.device, requires_grad=True)
    l1, l2, loss = contrastive_loss_native(seq, vis, video_mask, ls)
    loss.backward()
    return torch.stack([l1.detach(), l2.detach(), loss.detach()]), seq.grad, vis.grad, ls.grad
