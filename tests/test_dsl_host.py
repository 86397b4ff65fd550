"""camoe_dsl without a GPU: the flag's plumbing (CLIP4Clip reads it, eval_epoch resolves explicit argument > args > model) and
the clip-sharded evaluation with the dual softmax over gloo, world 2, on a torch-CPU stand-in for eval.HipBackend - sharded ==
single process == the float64 restatement (tests/dsl_ref.py) applied to the unsharded matrix, single- and multi-sentence
protocols, a partition in which one rank receives no rows, and a NaN column (a fully masked clip)."""
import os
import socket
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dsl_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ the flag
def _small_clip4clip(**extra):
    from centerclip_amd.clip4clip import CLIP4Clip
    g = np.load(os.path.join(HERE, "golden", "clip_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    cfg = Namespace(cluster_inter=1, cluster_algo='kmediods++', max_frames=int(g["cfg"][11]), target_frames_blocks=[4, 2, 2],
                    cluster_num_blocks=[16, 6, 6], cluster_distance='euclidean', cluster_threshold=1e-6, cluster_iter_limit=100,
                    minkowski_norm_p=2.0, pretrained_clip_name='ViT-B/32', aggregation=None, pre_norm=False, loose_type=True,
                    sim_header='meanP', linear_patch='2d', **extra)
    return CLIP4Clip.from_state_dict(sd, cfg)


def test_clip4clip_reads_camoe_dsl_from_the_task_config():
    assert _small_clip4clip().camoe_dsl is False
    assert _small_clip4clip(camoe_dsl=0).camoe_dsl is False
    assert _small_clip4clip(camoe_dsl=1).camoe_dsl is True


def test_contrastive_loss_takes_the_dsl_keyword_and_has_no_cpu_path():
    from centerclip_amd._lib import CenterClipHipError
    from centerclip_amd.losses import contrastive_loss
    from centerclip_amd import ops
    with pytest.raises(CenterClipHipError):
        contrastive_loss(torch.randn(3, 1, 8), torch.randn(3, 2, 8), torch.ones(3, 2, dtype=torch.long), torch.tensor(1.0), dsl=True)
    with pytest.raises(CenterClipHipError):
        ops.dual_softmax(torch.randn(3, 4))


# ------------------------------------------------------------------------------------------------ stand-ins
class _TorchBackend:
    """Torch-CPU stand-in for eval.HipBackend, the dual-softmax methods included (same semantics as the HIP ops: (-inf, 0) for
    no rows, NaN columns stay NaN, in-place rescale and apply).  Test infrastructure only."""
    calls = []

    @staticmethod
    def _normalize(x):
        return x / x.norm(dim=-1, keepdim=True)

    @classmethod
    def text_operand(cls, feats):
        return cls._normalize(feats.float())

    @classmethod
    def video_operand(cls, v, m):
        if v.dim() == 2:
            return cls._normalize(v.float())
        v = cls._normalize(v.float())
        m = m.to(torch.float).unsqueeze(-1)
        s = m.sum(dim=1)
        s[s == 0.] = 1.
        return cls._normalize((v * m).sum(dim=1) / s)           # (a fully masked clip: 0 / 0 = a NaN row)

    @staticmethod
    def video_operand_rows(n):
        return n + 2

    @staticmethod
    def dot_operands(text_op, video_op, n_video, mult):
        return mult * text_op @ video_op[:n_video].t()

    @staticmethod
    def counts_cols(sim, gt):
        d = sim.gather(1, gt.long().view(-1, 1))
        before = (sim == d) & (torch.arange(sim.shape[1])[None, :] < gt.long().view(-1, 1))
        return torch.stack([(sim > d).sum(1), (sim == d).sum(1), before.sum(1)], 1).to(torch.int32)

    @staticmethod
    def counts_ref_columns(sim, ref):
        return torch.stack([(sim > ref[None, :]).sum(0), (sim == ref[None, :]).sum(0)], 1).to(torch.int32)

    @staticmethod
    def group_max(sim, groups, n_groups):
        best = torch.full((n_groups, sim.shape[1]), float("-inf"))
        if sim.shape[0]:
            clean = torch.where(sim != sim, torch.full_like(sim, float("-inf")), sim)
            best.scatter_reduce_(0, groups.long().view(-1, 1).expand(-1, sim.shape[1]), clean, "amax", include_self=True)
        return best

    @classmethod
    def dsl_col_stats(cls, sim):
        cls.calls.append("stats")
        if sim.shape[0] == 0:
            return torch.full((sim.shape[1],), float("-inf")), torch.zeros(sim.shape[1])
        m = sim.max(dim=0).values
        m = torch.where(torch.isnan(sim).any(dim=0), torch.full_like(m, float("nan")), m)
        return m, torch.exp(sim - m[None, :]).sum(dim=0)

    @classmethod
    def dsl_rescale_stats(cls, s, m_local, m_global):
        cls.calls.append("rescale")
        s.copy_(torch.where(s == 0, torch.zeros_like(s), s * torch.exp(m_local - m_global)))
        return s

    @classmethod
    def dsl_apply(cls, sim, m, s, n_total):
        cls.calls.append("apply")
        sim.copy_((float(n_total) * sim) * (torch.exp(sim - m[None, :]) / s[None, :]))
        return sim


class _TableModel(torch.nn.Module):
    """Stands in for CLIP4Clip: features are looked up from the inputs (ids carry a row number, 'frames' are features)."""

    def __init__(self, E=8, camoe_dsl=None):
        super().__init__()
        self.table = torch.randn(64, E, generator=torch.Generator().manual_seed(5))
        if camoe_dsl is not None:
            self.camoe_dsl = camoe_dsl

    def forward(self, input_ids=None, token_type_ids=None, attention_mask=None, video=None, video_mask=None):
        out = {'sequence_output': None, 'visual_output': None}
        if input_ids is not None:
            out['sequence_output'] = self.table[input_ids.view(-1, input_ids.shape[-1])[:, 0]].unsqueeze(1)
        if video is not None:
            out['visual_output'] = video[:, 0].float()                  # [b, T, E]
        return out

    def get_video_mask_after_cluster(self, m):
        return m

    def _logit_scale_value(self):
        return 1.5


SENTENCES = [3, 1, 4, 2, 3]


def _dataset(multi, masked_clip=None, E=8, T=3):
    """11 single-caption clips, or 5 clips with 3/1/4/2/3 sentences (13 items).  item = (ids, mask, seg, video, vmask);
    ``masked_clip``: that clip's mask is all zero (its column of the matrix is NaN)."""
    g = torch.Generator().manual_seed(23)
    sentences = SENTENCES if multi else [1] * 11
    videos = torch.randn(len(sentences), 1, T, E, generator=g)
    vmask = torch.ones(len(sentences), 1, T, dtype=torch.long)
    vmask[1, 0, T - 1] = 0
    if masked_clip is not None:
        vmask[masked_clip] = 0
    items = []
    rows = torch.randperm(64, generator=g)                  # distinct text rows: no exact ties in the matrix
    for v, ns in enumerate(sentences):
        for _ in range(ns):
            ids = torch.zeros(1, 4, dtype=torch.long)
            ids[0, 0] = int(rows[len(items)])
            items.append((ids, (ids >= 0).long(), torch.zeros_like(ids), videos[v], vmask[v]))
    attrs = {}
    if multi:
        attrs = dict(multi_sentence_per_video=True, cut_off_points=list(torch.tensor(sentences).cumsum(0).tolist()),
                     sentence_num=len(items), video_num=len(sentences))
    return items, attrs


class _Items(torch.utils.data.Dataset):
    def __init__(self, items, attrs):
        self.items = items
        for k, v in attrs.items():
            setattr(self, k, v)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _restated(model, items, multi):
    """The unsharded fp32 matrix the stand-in forms -> float64 dual softmax -> restated metrics; + the smallest rank gap."""
    text = torch.stack([model.table[it[0][0, 0]] for it in items])
    vid_items = items if not multi else [items[c - 1] for c in np.cumsum(SENTENCES)]
    vis = _TorchBackend.video_operand(torch.stack([it[3][0] for it in vid_items]), torch.stack([it[4][0] for it in vid_items]))
    sim = (float(np.exp(1.5)) * _TorchBackend.text_operand(text) @ vis.t()).numpy()
    d = R.dual_softmax64(sim)
    return R.metrics64(d, SENTENCES if multi else None), R.rank_gap(d, SENTENCES if multi else None)


# ------------------------------------------------------------------------------------------------ resolution order
def test_eval_epoch_resolves_explicit_argument_then_args_then_model():
    from torch.utils.data import DataLoader
    from centerclip_amd.eval import eval_epoch
    items, attrs = _dataset(False)
    loader = DataLoader(_Items(items, attrs), batch_size=4)
    dev = torch.device("cpu")

    def used(model, **kw):
        _TorchBackend.calls.clear()
        out = eval_epoch(model, loader, dev, backend=_TorchBackend, **kw)
        return bool(_TorchBackend.calls), out
    on, off = Namespace(camoe_dsl=1), Namespace(camoe_dsl=0)
    assert used(_TableModel())[0] is False                                   # nothing says so: off, no backend method called
    assert used(_TableModel(camoe_dsl=True))[0] is True                      # the model's attribute
    assert used(_TableModel(camoe_dsl=True), args=Namespace())[0] is True    # args without the field: still the model's
    assert used(_TableModel(camoe_dsl=True), args=off)[0] is False           # args over the model
    assert used(_TableModel(camoe_dsl=False), args=on)[0] is True
    assert used(_TableModel(camoe_dsl=True), args=on, camoe_dsl=False)[0] is False     # the explicit argument over both
    flag, out = used(_TableModel(), args=off, camoe_dsl=True)
    assert flag is True and _TorchBackend.calls == ["stats", "apply"]        # one process: no rescale
    # and the flag changes what is ranked: the restated metrics of D, not those of S
    (r1, info), gap = _restated(_TableModel(), items, False)
    assert gap > 1e-4 and abs(out[0] - r1) < 1e-9 and list(out[2]) == info
    plain = used(_TableModel())[1]
    assert list(plain[2]) != info


# ------------------------------------------------------------------------------------------------ gloo, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, fn_name, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, globals()[fn_name](rank, world)))
    finally:
        dist.destroy_process_group()


def _run(fn_name, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn_name, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def case_sharded_dsl(rank, world):
    """Every rank: eval_epoch(shard=True, camoe_dsl=True); rank 0 alone: the single-process call.  Both == the restatement.
    batch 3: the batches are dealt to both ranks; batch 16: ONE batch, rank 1 receives no text row (and no video)."""
    from torch.utils.data import DataLoader
    from centerclip_amd.eval import eval_epoch
    model, dev = _TableModel(), torch.device("cpu")
    problems = []
    for multi in (False, True):
        # (the NaN column only under the single-sentence protocol: with several sentences per video the loop's video->text
        #  ranking of an all -inf row - flag on or off - counts its ties, which the restated compute_metrics does not)
        for masked in ((None,) if multi else (None, 2)):
            items, attrs = _dataset(multi, masked)
            (r1, info), gap = _restated(model, items, multi)
            if not gap > 1e-4:                             # fp32 stand-in against float64: ranks must not hang on roundoff
                problems.append(("gap", multi, masked, gap))
            for batch in (3, 16):
                loader = DataLoader(_Items(items, attrs), batch_size=batch, shuffle=False)
                box = [eval_epoch(model, loader, dev, backend=_TorchBackend, camoe_dsl=True) if rank == 0 else None]
                dist.broadcast_object_list(box, src=0)
                single = box[0]
                _TorchBackend.calls.clear()
                got = eval_epoch(model, loader, dev, shard=True, backend=_TorchBackend, camoe_dsl=True)
                if "rescale" not in _TorchBackend.calls:
                    problems.append(("no rescale", multi, masked, batch))
                for what, res in (("single", single), ("sharded", got)):
                    if not (abs(res[0] - r1) < 1e-9 and list(res[2]) == info):
                        problems.append((what, multi, masked, batch, res[0], r1, list(res[2]), info))
    return problems


def test_clip_sharded_eval_epoch_with_camoe_dsl_world2():
    res = _run("case_sharded_dsl")
    assert res == {0: [], 1: []}, res
