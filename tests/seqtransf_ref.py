"""Plain-torch restatement of the seqTransf similarity head (modules/clip4clip.py:335-366 with module_cross.py:88-112), in
whatever dtype its inputs have (the tests run it in float64).  Pinned to the reference's own float64 run by
tests/test_seqtransf_host.py; the GPU tests use it as their reference."""
import torch

BLOCK_PARAMS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight",
                "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight",
                "ln_2.bias")


def blocks_from_state(sd, layers, prefix="transformerClip.resblocks."):
    """{name: tensor} -> [{param: tensor}] for blocks 0..layers-1."""
    return [{p: sd["%s%d.%s" % (prefix, i, p)] for p in BLOCK_PARAMS} for i in range(layers)]


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def key_masked_attention(q, k, v, mask):
    """q, k, v [B, H, L, 64], mask [B, L] -> softmax(q k^T / 8 + (1 - mask[key]) * -1e6) v  [B, H, L, 64]."""
    s = q @ k.transpose(-1, -2) / 8.0 + ((1.0 - mask.to(q.dtype)) * -1e6)[:, None, None, :]
    return torch.softmax(s, dim=-1) @ v


def block(x, p, mask, heads):
    """One module_cross.ResidualAttentionBlock on x [B, L, W] (batch-major) with the key mask [B, L]."""
    B, L, W = x.shape
    h = _ln(x, p["ln_1.weight"], p["ln_1.bias"])
    qkv = h @ p["attn.in_proj_weight"].t() + p["attn.in_proj_bias"]
    q, k, v = (t.reshape(B, L, heads, W // heads).transpose(1, 2) for t in qkv.split(W, dim=-1))
    o = key_masked_attention(q, k, v, mask).transpose(1, 2).reshape(B, L, W)
    x = x + o @ p["attn.out_proj.weight"].t() + p["attn.out_proj.bias"]
    u = _ln(x, p["ln_2.weight"], p["ln_2.bias"]) @ p["mlp.c_fc.weight"].t() + p["mlp.c_fc.bias"]
    u = u * torch.sigmoid(1.702 * u)
    return x + u @ p["mlp.c_proj.weight"].t() + p["mlp.c_proj.bias"]


def head(vis, mask, pos, blocks, heads):
    """visual_output [B, T, D], video_mask [B, T], position table [>= T, D] -> x + visual_output (clip4clip.py:337-349)."""
    T = vis.shape[1]
    x = vis + pos[:T].unsqueeze(0)
    for p in blocks:
        x = block(x, p, mask, heads)
    return x + vis


def pooled(vis, mask):
    """normalise, masked mean over the segments, normalise (clip4clip.py:359-360, _mean_pooling_for_similarity_visual)."""
    v = vis / vis.norm(dim=-1, keepdim=True)
    m = mask.to(v.dtype).unsqueeze(-1)
    v = (v * m).sum(1) / m.sum(1)
    return v / v.norm(dim=-1, keepdim=True)


def logits(seq, vis, mask, pos, blocks, heads, logit_scale):
    """_loose_similarity with sim_header='seqTransf' (eval branch): seq [Bt, 1, D] -> [Bt, Bv]."""
    t = seq.squeeze(1)
    t = t / t.norm(dim=-1, keepdim=True)
    return torch.exp(logit_scale) * t @ pooled(head(vis, mask, pos, blocks, heads), mask).t()


def cross_en_symmetric(sim):
    """(CrossEn(sim) + CrossEn(sim^T)) / 2 (modules/losses.py:8-18)."""
    ce = lambda s: -torch.diagonal(torch.log_softmax(s, dim=-1)).mean()
    return (ce(sim) + ce(sim.t())) / 2
