"""End-to-end retrieval evaluation on synthetic data, written the way the reference's main.py drives it (:98, :232-233, :381-499):

    model = CLIP4Clip.from_pretrained(...); eval_epoch(model, test_dataloader, device)

with random-init CLIP weights (no checkpoint / dataset access here) and a synthetic "dataset" of N clips + N captions.
Every compute step runs in the HIP library; swap the state dict for a real ViT-B/32 checkpoint and the loader for
dataloaders/* to evaluate a trained model.

    python examples/eval_synthetic.py [--clips 64] [--algo kmediods++|spectral|pooling] [--l14 1 [--oracle-check 1]]
    python examples/eval_synthetic.py --resume DIR/ckpt.pth.tar      (main.py's --resume ... --do_eval 1: evaluate a checkpoint)
    python examples/eval_synthetic.py --raw_frames 240x320           (decoded uint8 frames; resize + centre crop on the device)
    python examples/eval_synthetic.py --ragged 1                     (clips of mixed sizes and lengths, collated on the device)
    python examples/eval_synthetic.py --raw_frames 240x320 --yuv nv12  (YUV frames as a decoder leaves them, also p010, i444, ...; also with --ragged 1)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centerclip_amd.clip4clip import CLIP4Clip              # noqa: E402
from centerclip_amd.eval import eval_epoch                  # noqa: E402
import bench                                                # noqa: E402  (cfg-2 task config, random ViT-B/32 state dict)


def yuv_frames(layout, lead, H, W, generator):
    """Random frames of a named YUV layout as a decoder leaves them: [*lead, rows, W] with rows = 3H/2, 2H or 3H; uint8, or
    uint16 words (the sample above the layout's shift) for the 10-, 12- and 16-bit layouts."""
    from centerclip_amd.torch_ops import YUV_FORMATS
    _, sub_x, sub_y, depth, shift, _ = YUV_FORMATS[layout]
    den = 1 << (sub_x + sub_y)
    shape = tuple(lead) + (H * (den + 2) // den, W)
    if depth == 8:
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=generator)
    words = torch.randint(0, 1 << depth, shape, dtype=torch.int32, generator=generator) << shift
    return torch.from_numpy(words.numpy().astype("uint16"))


YUV_LAYOUTS = ["i420", "nv12", "i422", "i444", "i420p10", "i422p10", "i444p10", "p010", "i420p12", "p012", "p016", "i444p16"]


class SyntheticRetrieval(torch.utils.data.Dataset):
    """(input_ids, input_mask, segment_ids, video, video_mask) as dataloaders/* yield them (main.py:427)."""

    def __init__(self, n, frames=12, words=32, seed=0, raw_frames=None, yuv=None):
        """raw_frames (H, W): the video as a decoder leaves it - uint8 [n, 1, frames, H, W, 3] of that size, for
        eval_epoch(frame_transform=...) - instead of the transformed float tensor; with yuv (a layout name, "i420" .. "i444p16")
        before any colour conversion: [n, 1, frames, rows, W], the tight planes (uint8, or uint16 above 8 bits)."""
        g = torch.Generator().manual_seed(seed)
        if raw_frames is None:
            self.video = torch.randn(n, 1, frames, 3, 224, 224, generator=g)
        elif yuv:
            self.video = yuv_frames(yuv, (n, 1, frames), raw_frames[0], raw_frames[1], g)
        else:
            self.video = torch.randint(0, 256, (n, 1, frames, raw_frames[0], raw_frames[1], 3), dtype=torch.uint8, generator=g)
        self.ids = torch.randint(1, 49405, (n, words), generator=g)
        self.ids[:, 0] = 49406
        eot = torch.randint(3, words, (n,), generator=g)
        for i in range(n):
            self.ids[i, eot[i]] = 49407
            self.ids[i, eot[i] + 1:] = 0
        self.mask = (self.ids != 0).long()
        self.vmask = torch.ones(n, 1, frames, dtype=torch.long)

    def __len__(self):
        return self.video.shape[0]

    def __getitem__(self, i):
        return self.ids[i], self.mask[i], torch.zeros_like(self.ids[i]), self.video[i], self.vmask[i]


class RaggedRetrieval(torch.utils.data.Dataset):
    """The same items with the video as a decoder leaves it: uint8 [t, H, W, 3], H x W and t <= frames differing from clip to
    clip (the short side is not 224 for every clip, so some are resized and some only cropped).  ``collate`` packs a batch
    (preprocess.pack_clips) and builds its video mask from the clips' lengths."""
    SIZES = ((224, 298), (224, 398), (398, 224), (240, 320))

    def __init__(self, n, frames=12, seed=0, yuv=None):
        """yuv (a layout name): the clips before any colour conversion, [t, rows, W]"""
        self.text, self.frames, self.yuv = SyntheticRetrieval(n, frames=1, seed=seed, raw_frames=(4, 4)), frames, yuv
        g = torch.Generator().manual_seed(seed + 1)
        clip = lambda t, H, W: (yuv_frames(yuv, (t,), H, W, g) if yuv
                                else torch.randint(0, 256, (t, H, W, 3), dtype=torch.uint8, generator=g))
        self.video = [clip(frames - (i % 3) * 2, *self.SIZES[i % len(self.SIZES)]) for i in range(n)]

    def __len__(self):
        return len(self.video)

    def __getitem__(self, i):
        return self.text.ids[i], self.text.mask[i], torch.zeros_like(self.text.ids[i]), self.video[i]

    def collate(self, items):
        from centerclip_amd.preprocess import pack_clips, pack_yuv_clips
        packed = pack_yuv_clips([it[3] for it in items], self.yuv) if self.yuv else pack_clips([it[3] for it in items])
        return tuple(torch.stack([it[k] for it in items]) for k in range(3)) + (packed, packed.video_mask(self.frames).unsqueeze(1))


# ViT-L/14 at 224 px (OpenAI's ViT-L-14.pt geometry: width 1024, 24 layers, patch 14 -> 257 tokens per frame, embedding 768,
# text width 768): 12 frames -> 4 segments at block 13, K = 128.  Blocks 1-12 run the streaming attention (L = 257), blocks
# 13-24 the one-launch in_proj + attention form (L = 129).
L14 = dict(bench.CFG2, name="ViT-L/14 224^2: 12 frames -> 4 segments @block 13, 256 tokens/frame, K=128, batch 16, 32 words",
           patch=14, width=1024, layers=24, T_new=4, K=128, cluster_block=13)


def l14_state_dict(c, seed):
    """Random-init weights of the ViT-L/14 architecture (CLIP.initialize_parameters statistics, rounded through fp16)."""
    from centerclip_amd.clip import CLIP
    torch.manual_seed(seed)
    m = CLIP(768, c["res"], c["layers"], c["width"], c["patch"], 77, 49408, 768, 12, 12, video_frames=c["T"], args=None)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def l14_task_config(c):
    args = bench.task_config(c)
    cb, n = c["cluster_block"], c["layers"]
    args.target_frames_blocks = [c["T"]] * (cb - 1) + [c["T_new"]] * (n + 1 - cb)
    args.cluster_num_blocks = [c["K"]] * n
    args.pretrained_clip_name = 'ViT-L/14'
    return args


def oracle_check(sd, device, frames=2):
    """Normalised embeddings of one short clip (no clustering) and one caption against the CPU oracle on the same
    weights -> (max |delta| visual, text)."""
    from centerclip_amd.clip import build_clip_model
    from oracle import clip_oracle as clo
    model, _ = build_clip_model(dict(sd), args=None)
    model = model.to(device)
    data = SyntheticRetrieval(1, frames=frames, seed=5)
    video, ids = data.video[0, 0], data.ids[:1]
    vfeat, tfeat = model.encode_pair(video.to(device), ids.to(device), video_frame=frames)
    torch.cuda.synchronize()
    vref, tref = clo.visual_forward(sd, video, frames), clo.text_forward(sd, ids)
    nrm = lambda x: x / x.norm(dim=-1, keepdim=True)
    return float((nrm(vfeat.cpu()) - nrm(vref)).abs().max()), float((nrm(tfeat.cpu()) - nrm(tref)).abs().max())


def shift_plan(args):
    """The plan of scripts/activitynet.sh case 04: a shift module in every block (the frame count drops at block 1, the
    token count at every later block - the shift itself keeps both)."""
    args.target_frames_blocks = [args.max_frames - 1] * 12
    args.cluster_num_blocks = [55, 54, 53, 52, 51, 50, 48, 47, 46, 45, 44, 43]
    return args


def transform_ms(transform, video, device, reps=10):
    """Device time of the frame transform on one batch, from its own events (the first call builds and uploads the plan)."""
    x = video.to(device)
    transform(x)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        transform(x)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--algo", default="kmediods++", choices=["kmediods++", "spectral", "pooling", "sparse_sampling",
                                                             "token_shift", "temporal_shift"],
                    help="cluster_algo; the shift algorithms get a module in every block (scripts/activitynet.sh case 04)")
    ap.add_argument("--sim_header", default="meanP", choices=["meanP", "seqTransf"],
                    help="similarity head (clip4clip.py:324-367); seqTransf starts from the reference's initialisation trick")
    ap.add_argument("--cross_num_hidden_layers", type=int, default=4, help="blocks of the seqTransf head (params.py default 4)")
    ap.add_argument("--in-flight", type=int, default=None, help="batches in flight (model instances / streams); default: eval_epoch's own (2 on a GPU)")
    ap.add_argument("--camoe_dsl", type=int, default=0,
                    help="params.py's --camoe_dsl: rank the CAMoE dual softmax S * softmax(S, dim=0) * len(S) instead of S")
    ap.add_argument("--l14", type=int, default=0, help="ViT-L/14 at 224 px instead (257 tokens per frame, width 1024, 24 layers)")
    ap.add_argument("--quick_gelu", type=int, default=1,
                    help="0: both towers use the exact GELU of the OpenCLIP / LAION checkpoints (OpenCLIP's config key) instead of QuickGELU")
    ap.add_argument("--oracle-check", type=int, default=0, help="--l14: also compare one 2-frame clip's embeddings with the CPU oracle")
    ap.add_argument("--resume", default=None, help="main.py's --resume with --do_eval 1: a checkpoint (train_synthetic.py --output_dir) "
                                                   "whose weights are evaluated")
    ap.add_argument("--raw_frames", default=None, metavar="HxW",
                    help="the loader yields decoded uint8 frames of this size; Resize(res, BICUBIC) + CenterCrop(res) of CLIP's "
                         "transform run on the device (eval_epoch(frame_transform=...))")
    ap.add_argument("--ragged", type=int, default=0,
                    help="1: the loader yields PackedClips - decoded clips of mixed H x W and lengths - and preprocess.ClipCollate "
                         "resizes, crops and zero-pads them into the uniform batch on the device, at most two launches per batch")
    ap.add_argument("--yuv", default=None, choices=YUV_LAYOUTS,
                    help="with --raw_frames or --ragged: the frames are YUV as a decoder leaves them (PyAV's to_ndarray() of "
                         "yuv420p / nv12 / yuv422p / yuv444p / yuv420p10le / p010le ..., [..., rows, W], uint16 above 8 bits); the "
                         "conversion to RGB runs inside the device transform")
    a = ap.parse_args()
    if a.yuv and not (a.raw_frames or a.ragged):
        ap.error("--yuv describes decoded frames: give --raw_frames HxW or --ragged 1")
    device = torch.device("cuda:0")
    c = L14 if a.l14 else bench.CFG2
    args = l14_task_config(c) if a.l14 else bench.task_config(c)     # cfg 2: 12 frames -> 3 segments at block 7, K = 49
    args.cluster_algo = a.algo
    args.sim_header, args.cross_num_hidden_layers = a.sim_header, a.cross_num_hidden_layers
    args.camoe_dsl = a.camoe_dsl
    args.quick_gelu = a.quick_gelu
    if a.algo in ("token_shift", "temporal_shift"):
        shift_plan(args)
    vars(args).update(spectral_sigma=2.0, spectral_graph="HeatKernel", spectral_knn_k=1, spectral_spg=0, svd_correct_sign=1)
    sd = l14_state_dict(c, seed=0) if a.l14 else bench.random_state_dict(c, seed=0)
    if a.l14 and a.oracle_check:
        print("ViT-L/14, 2 frames + 1 caption, max|delta| of normalised embeddings vs oracle: visual %.2e text %.2e" % oracle_check(sd, device))
    model = CLIP4Clip.from_state_dict(sd, args).to(device).eval()
    if a.resume is not None:
        from centerclip_amd.train import resume
        resume(a.resume, model, load_from_pretrained=True)  # (the weights alone: nothing here trains)
        print("evaluating the weights of %s" % a.resume)
    raw = tuple(int(v) for v in a.raw_frames.lower().split("x")) if a.raw_frames else None
    loader = torch.utils.data.DataLoader(SyntheticRetrieval(a.clips, raw_frames=raw, yuv=a.yuv), batch_size=a.batch, shuffle=False)
    transform = None
    if raw is not None:
        from centerclip_amd.preprocess import FrameTransform, YuvFrameTransform
        transform = YuvFrameTransform(c["res"], layout=a.yuv) if a.yuv else FrameTransform(c["res"])
        print("frame transform %dx%d -> %d: %.3f ms per batch of %d clips" % (raw[0], raw[1], c["res"], transform_ms(
            transform, next(iter(loader))[3], device), a.batch))
    if a.ragged:
        from centerclip_amd.preprocess import ClipCollate, YuvClipCollate
        from centerclip_amd.search import FeatureGallery
        data = RaggedRetrieval(a.clips, frames=c["T"], yuv=a.yuv)
        loader = torch.utils.data.DataLoader(data, batch_size=a.batch, shuffle=False, collate_fn=data.collate)
        transform = (YuvClipCollate(c["res"], max_frames=c["T"], layout=a.yuv) if a.yuv
                     else ClipCollate(c["res"], max_frames=c["T"]))
        packed, vmask = next(iter(loader))[3:]
        print("ragged batch: %d clips, %d bytes, lengths %s" % (len(packed), packed.data.numel(), packed.table[:, 1].tolist()))
        # a FeatureGallery takes the collated tensor as it is
        pos = FeatureGallery(model).add(transform(packed.to(device)), vmask.to(device))
        print("FeatureGallery.add(collate(packed), mask): %d clips added" % len(pos))
    r1, seconds, info = eval_epoch(model, loader, device, args, log=print, in_flight=a.in_flight,
                                   **({"frame_transform": transform} if transform is not None else {}))
    print("\n".join(info))
    print("R@1 %.1f (random weights: chance level is %.1f); model time %.2f s for %d clips" % (r1, 100.0 / a.clips, seconds, a.clips))


if __name__ == "__main__":
    main()
