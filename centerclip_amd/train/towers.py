"""The two towers and the seqTransf head with gradients: what main.py:291-378 (train_epoch) needs from the model is
CLIP4Clip.forward in training mode with gradients reaching every parameter.  The towers are the reference's forward
(modules/clip.py:320-345 visual, :471-496 text; the head: clip4clip.py:335-349) composed of the pieces of ``block``: patch
embedding and the projection heads as GEMMs (LinearFunction), LayerNorms (LayerNormFunction), the blocks (block_apply), the
token-cluster module (its own autograd, cluster/cluster.py).  What stays torch glue: reshapes / permutes / concatenation,
the broadcast adds of the class and positional embeddings, the embedding-table gather with its scatter-add gradient, the
EOT row gather.  A tower's frozen prefix (clip4clip.py:449-471 freeze_cip_layers) runs on the fused inference kernels.
"""
import torch

from .. import _lib as L
from ..torch_ops import patch_cols
from .block import LinearFunction, _layernorm, block_apply


def _blocks(transformer, x_lnd, start=0):
    """The resblocks from block ``start`` on, on LND activations; a block's token-cluster module runs in front of it
    (clip.py:236-242)."""
    for blk in list(transformer.resblocks)[start:]:
        tc = blk.tokencluster_inter
        if tc is not None:
            if getattr(tc, "mean_residual", False):
                raise NotImplementedError("training towers: mean_residual is not built")
            x_lnd, _ = tc(x_lnd)
            # token_shift shifts the CLS rows again behind the attention (clip.py:246-248)
            mid_shift = (tc.original_frame, tc.shift_fold_div) if tc.algorithm == 'token_shift' else None
            x_lnd = block_apply(blk, x_lnd, mid_shift=mid_shift, cluster_done=True)
        else:
            x_lnd = block_apply(blk, x_lnd)
    return x_lnd


def seq_head_train(model, visual_output, video_mask):
    """CLIP4Clip's seqTransf head (clip4clip.py:335-349) with gradients: visual_output [B, T, D] + video_mask [B, T] ->
    [B, T, D].  The position rows are a slice of frame_position_embeddings.weight (rows >= T get exactly zero gradient), the
    blocks run block_forward_train / block_backward with the key mask, the outer residual is an autograd add."""
    L.require_device(visual_output)
    B, T, D = visual_output.shape
    mask = video_mask if video_mask.dtype == torch.long else video_mask.to(torch.long)
    x = visual_output.float() + model.frame_position_embeddings.weight[:T].float().unsqueeze(0)
    x = x.permute(1, 0, 2)                                                      # NLD -> LND (a view: the block reads it once)
    for blk in model.transformerClip.resblocks:
        x = block_apply(blk, x, key_mask=mask)
    return x.permute(1, 0, 2) + visual_output.float()


# The frozen prefix of a tower (clip4clip.py:449-471 freeze_cip_layers, called by main.py:102 in every shipped launcher): the
# leading run of stages in which no parameter requires a gradient - the front end (visual: patch / class / position embedding +
# ln_pre; text: token + position embedding), then blocks 0, 1, ...  Nothing in it needs activations for a backward, so it runs
# under no_grad in ONE enqueue of the inference path's kernels (cc_vit_encode_prefix_frames / cc_text_encode_prefix) and hands the
# first trainable block the fp32 residual stream.
_GLUE_FRONT = False      # private, for the tests: True = the towers' fronts as torch glue + per-op launches whatever is frozen


def _none_trainable(params):
    return not any(p.requires_grad for p in params)


def _prefix_blocks(transformer):
    n = 0
    for blk in transformer.resblocks:
        tc = blk.tokencluster_inter
        if not _none_trainable(blk.parameters()) or (tc is not None and getattr(tc, "mean_residual", False)):
            break
        n += 1
    return n


def visual_prefix_blocks(vis):
    """Number of leading blocks in the visual tower's frozen prefix (0: the front end alone), None: no frozen prefix."""
    if _GLUE_FRONT or vis.linear_patch != '2d' or not _none_trainable(vis.prefix_parameters(0)):
        return None
    return _prefix_blocks(vis.transformer)


def text_prefix_blocks(clip):
    """The text tower's counterpart of visual_prefix_blocks."""
    if _GLUE_FRONT or not _none_trainable(clip.text_prefix_parameters(0)):
        return None
    return _prefix_blocks(clip.transformer)


def _front(vis, x, F, g):
    """The patch embedding's rows [F * g * g, W] -> class and position embedding, ln_pre, the blocks (clip.py:324-338)."""
    W = vis.width
    x = x.view(F, g * g, W)
    cls = vis.class_embedding.to(x.dtype) + torch.zeros(F, 1, W, dtype=x.dtype, device=x.device)
    x = torch.cat([cls, x], dim=1) + vis.positional_embedding.to(x.dtype)
    x = _layernorm(vis.ln_pre, x.reshape(F * (g * g + 1), W)).view(F, g * g + 1, W)
    return _blocks(vis.transformer, x.permute(1, 0, 2).contiguous()).permute(1, 0, 2)          # NLD -> LND -> NLD


def encode_image_train(clip, video, video_frame):
    """CLIP.encode_image (modules/clip.py:460-469 with VisualTransformer.forward :304-345) with gradients:
    video [F, 3, H, W] fp32, or the loader's uint8 frames [F, 3, H, W] / [F, H, W, 3] (the patch gather applies
    dataloaders/transforms.py's u8/255 -> (x - mean)/std) -> (features [F', embed_dim], cluster_loss).
    linear_patch '3d' (clip.py:306-317): conv2 over clips of video_frame frames as a GEMM over the 3-d patch gather's rows;
    conv1 takes no part and receives no gradient."""
    vis = clip.visual
    F, p, W = video.shape[0], vis.patch_size, vis.width
    g = vis.input_resolution // p
    p3d = vis.linear_patch == '3d'
    if p3d:
        if not video_frame or video_frame <= 0 or F % video_frame:
            raise ValueError("linear_patch='3d': video_frame %r must divide the %d frames (clip.py:307)" % (video_frame, F))
        if p % 8:
            raise ValueError("linear_patch='3d': patch size %d is off the patch gather's 8-wide grid" % p)
        seg = vis.shift_segment()
        if seg is not None and video_frame != seg:
            raise NotImplementedError("linear_patch='3d' with a shift module needs video_frame == original_frame")
    L.require_device(video)
    n = visual_prefix_blocks(vis)
    if n is not None:
        with torch.no_grad():
            x = vis.encode_prefix(video, video_frame, n, forced_medoids=getattr(vis, "forced_medoids", None))
        # (frame-major rows: the first trainable block's own permute back finds them contiguous, no copy)
        x = _blocks(vis.transformer, x.permute(1, 0, 2), start=n).permute(1, 0, 2)
    elif p3d:
        # conv2 (kernel (3, p, p), stride (1, p, p), zero padding 1 along t, no bias) as a GEMM over the 3-d patch rows
        # (c, kt, kh, kw): the fp16 matrix is written once and is LinearFunction's operand and saved activation
        a = torch.ops.centerclip.patch_gather3d(video if video.dtype == torch.uint8 else video.float(), int(video_frame),
                                                vis.input_resolution, p)
        x = _front(vis, LinearFunction.apply(a, vis.conv2.weight.view(W, -1), None), F, g)
    else:
        w = vis.conv1.weight.view(W, -1)
        if _GLUE_FRONT:
            if video.dtype == torch.uint8:
                raise ValueError("the torch-glue front takes normalised float frames")
            # conv1 (kernel = stride = p, no bias) as a GEMM over the patch rows (c, kh, kw) - a reshape of the frames
            a = video.float().view(F, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(F * g * g, 3 * p * p)
        else:
            # the encoders' patch gather: the fp16 patch matrix straight from the frames - LinearFunction's operand and saved
            # activation (no fp32 permute-copy of the patches, no separate cast)
            a = torch.ops.centerclip.patch_gather(video if video.dtype == torch.uint8 else video.float(), vis.input_resolution, p)
        Kp = patch_cols(p)
        if Kp != w.shape[1]:
            # a patch size off the 8-wide grid (ViT-L/14): the rows are padded to a multiple of 64 columns - zeros in the patch
            # matrix (the gather writes them), zeros appended to the weight; conv1's gradient is the first 3 p^2 columns of
            # the product's (the pad's backward is that slice)
            if a.shape[1] != Kp:
                a = torch.nn.functional.pad(a, (0, Kp - a.shape[1]))
            w = torch.nn.functional.pad(w, (0, Kp - w.shape[1]))
        x = _front(vis, LinearFunction.apply(a, w, None), F, g)
    cls_rows = x[:, 0, :].contiguous()                        # ln_post(x) @ proj, of which encode_image keeps the CLS row
    feats = LinearFunction.apply(_layernorm(vis.ln_post, cls_rows), vis.proj.t(), None)
    return feats, torch.zeros((), device=video.device)


def encode_text_train(clip, ids):
    """CLIP.encode_text (modules/clip.py:471-496) with gradients: ids [B, n_ctx] -> [B, embed_dim]."""
    L.require_device(ids)
    B, n_ctx = ids.shape
    W = clip.transformer.width
    n = text_prefix_blocks(clip)
    if n is not None:
        with torch.no_grad():
            x = clip.encode_text_prefix(ids, n)
        x = _blocks(clip.transformer, x.permute(1, 0, 2), start=n).permute(1, 0, 2).contiguous()
    else:
        # (autograd records nothing for a tensor that does not require a gradient: a frozen token_embedding gets no scatter-add)
        x = clip.token_embedding(ids).float() + clip.positional_embedding[:n_ctx].float()
        x = _blocks(clip.transformer, x.permute(1, 0, 2).contiguous()).permute(1, 0, 2).contiguous()
    eot = x[torch.arange(B, device=x.device), ids.argmax(dim=-1)]                             # the EOT token has the largest id
    return LinearFunction.apply(_layernorm(clip.ln_final, eot.contiguous()), clip.text_projection.t(), None)
