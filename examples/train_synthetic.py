"""A few training steps on synthetic data, written the way the reference's main.py drives them (:98-170, :291-378):

    model = CLIP4Clip.from_pretrained(...); optimizer = BertAdam(prep_optim_params_groups(...)); train_epoch(...)

or, with --optim AdamW, the recipe every shipped launcher uses (main.py:168-175, 316-333): AdamW(betas=(0.9, 0.98), eps=1e-6,
weight_decay=0.2) over the reference's lr_mult / decay_mult groups, the per-iteration 'cos' lr_scheduler with a 10 % slow start
and global gradient clipping at 1.0.  --optim-timing 1 times the optimizer step alone (HIP AdamW, clip_and_step and
torch.optim.AdamW(fused=True) + torch's clip over the same parameters).

with random-init ViT-B/32 weights at the cfg-2 shape (12 frames -> 3 segments at block 7, K = 49, batch 16) and fp32 master
weights.  Forward and backward of the towers, the loss and the optimizer step run in the HIP library (centerclip_amd.train);
the path is a correctness slice - per-op launches from Python, nothing fused or tuned - and the printed step time says so.

--freeze_layer_num K is handed to model.freeze_cip_layers as main.py:102 does (every shipped launcher passes 0; default -1:
nothing frozen): the frozen prefix of each tower then runs on the fused forward and gets no gradient work.  --uint8 1 draws
uint8 frames, as the loader yields them before its transform; the patch gather normalises them.  --linear_patch 3d trains
the Conv3d patch embedding (conv2) on the 3-d patch gather; the reference's freeze rule freezes nothing for such a model.  --camoe_dsl 1 trains on CAMoE's dual-softmax loss (the
launchers' --camoe_dsl): same step, the loss chain gains the column softmax and its gradient, still without a host read.

--precision amp is the launchers' setting (main.py:160 builds a GradScaler, train_epoch takes its scaler branch :320-328):
here a train.DeviceGradScaler - loss scaling, inf / NaN check, step skipping and the scale update all on the device - drives
the eager loop and, inside the graph, the captured step; the taken / skipped counters are printed at the end.

--epochs N runs train_epoch N times over the same loader; --output_dir DIR writes the reference's checkpoint after every epoch
(main.py:262-272: save_checkpoint(checkpoint_dict(...), is_best, DIR, filename='ckpt.pth.tar'); there is no eval here, so
is_best is "lowest mean loss so far"), and the captured step's own state_dict() as ckpt.graph.pth.tar.  --resume PATH restores
one (main.py:185-212) into the eager loop, which continues at the file's epoch and global_step, and then into the captured step
before its first call.

--augment multiscale|random_resized [--flip 1] trains the eager loop on the training loader's augmentations
(dataloaders/decode.py:32-41) done on the device: the loader hands over decoded uint8 frames - --raw_frames H,W as a decoder
leaves them (default 240,320), or with --uint8 1 the 224 x 224 uint8 frames - and train_epoch(frame_transform=
preprocess.TrainFrameTransform(...)) crops, resizes and flips each clip with one launch.  The captured step then runs on a batch
augmented the same way.

    python examples/train_synthetic.py [--steps 4] [--batch 16] [--optim BertAdam|AdamW] [--optim-timing 1] [--precision amp]
                                       [--epochs 1] [--output_dir DIR] [--resume DIR/ckpt.pth.tar]
                                       [--augment multiscale|random_resized] [--flip 1] [--raw_frames 240,320] [--yuv i420|nv12|p010|i444|...]
                                       [--freeze_layer_num 0] [--uint8 1] [--linear_patch 3d] [--camoe_dsl 1] [--quick_gelu 0] [--l14 1] [--lr 1e-3 --coef_lr 1 --same_batch 1]
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 examples/train_synthetic.py   (RCCL, bucketed)
"""
import argparse
import os
import sys
import time
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from centerclip_amd.clip4clip import CLIP4Clip              # noqa: E402
from centerclip_amd.train import (AdamW, BertAdam, DeviceGradScaler, checkpoint_dict, lr_scheduler,   # noqa: E402
                                  prep_optim_params_groups, resume, save_checkpoint, train_epoch)
from centerclip_amd import dist as ccdist                   # noqa: E402
from centerclip_amd.preprocess import TrainFrameTransform, YuvTrainFrameTransform   # noqa: E402
import bench                                                # noqa: E402
from eval_synthetic import SyntheticRetrieval, L14, l14_state_dict, l14_task_config   # noqa: E402


def shift_plan(args):
    """The plan of scripts/activitynet.sh case 04: a shift module in every block (the frame count drops at block 1, the
    token count at every later block - the shift itself keeps both)."""
    args.target_frames_blocks = [args.max_frames - 1] * 12
    args.cluster_num_blocks = [55, 54, 53, 52, 51, 50, 48, 47, 46, 45, 44, 43]
    return args


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--graph", type=int, default=1, help="also time the step captured into a hipGraph")
    ap.add_argument("--b16", type=int, default=0, help="ViT-B/16 instead (cfg-5 shape: 197 tokens per frame, 12 frames -> 4 segments, "
                                                       "K = 100; the attention backward's two-launch form)")
    ap.add_argument("--l14", type=int, default=0, help="ViT-L/14 at 224 px instead (257 tokens per frame, width 1024, 24 layers, "
                                                       "12 frames -> 4 segments at block 13, K = 128)")
    ap.add_argument("--sim_header", default="meanP", choices=["meanP", "seqTransf"],
                    help="similarity head (clip4clip.py:324-367); seqTransf starts from the reference's initialisation trick")
    ap.add_argument("--cross_num_hidden_layers", type=int, default=4, help="blocks of the seqTransf head (params.py default 4)")
    ap.add_argument("--optim", choices=["BertAdam", "AdamW"], default="BertAdam")
    ap.add_argument("--algo", default="kmediods++", choices=["kmediods++", "token_shift", "temporal_shift"],
                    help="cluster_algo; the shift algorithms get a module in every block (scripts/activitynet.sh case 04)")
    ap.add_argument("--optim-timing", type=int, default=0, help="also time the optimizer step alone (AdamW)")
    ap.add_argument("--freeze_layer_num", type=int, default=-1, help="main.py's --freeze_layer_num (the launchers pass 0)")
    ap.add_argument("--uint8", type=int, default=0, help="uint8 frames [T, 3, H, W], normalised inside the patch gather")
    ap.add_argument("--precision", choices=["fp32", "amp"], default="fp32",
                    help="amp: the launchers' GradScaler recipe on train.DeviceGradScaler, eager and captured")
    ap.add_argument("--lr", type=float, default=1e-7, help="learning rate of the new modules; the CLIP groups get lr * --coef_lr")
    ap.add_argument("--coef_lr", type=float, default=1e-3, help="main.py's --coef_lr")
    ap.add_argument("--same_batch", type=int, default=0, help="train every step on the first batch (shows the loss going down)")
    ap.add_argument("--linear_patch", choices=["2d", "3d"], default="2d",
                    help="params.py's --linear_patch; 3d: conv2 over (t, h, w) trains (random init), conv1 takes no part")
    ap.add_argument("--camoe_dsl", type=int, default=0,
                    help="params.py's --camoe_dsl: CAMoE's DSL loss - CrossEn on D = n * S * softmax(S, dim=0), both directions")
    ap.add_argument("--quick_gelu", type=int, default=1,
                    help="0: both towers train with the exact GELU of the OpenCLIP / LAION checkpoints instead of QuickGELU")
    ap.add_argument("--epochs", type=int, default=1, help="passes of train_epoch over the loader (main.py's --epochs)")
    ap.add_argument("--output_dir", default=None, help="main.py's --output_dir: write ckpt.pth.tar (and ckpt.best.pth.tar) after every epoch")
    ap.add_argument("--resume", default=None, help="main.py's --resume: a checkpoint to continue from (eager loop and captured step)")
    ap.add_argument("--augment", choices=["multiscale", "random_resized"], default=None,
                    help="train-time augmentation on the device (decode.py:32-41): one crop box per clip, resized to 224 px")
    ap.add_argument("--flip", type=int, default=0, help="with --augment: also one random horizontal flip per clip")
    ap.add_argument("--raw_frames", default="240,320", help="with --augment (and without --uint8 1): H,W of the decoded uint8 frames")
    ap.add_argument("--ragged", type=int, default=0,
                    help="1: the loader yields PackedClips - decoded clips of mixed H x W and lengths - collated on the device by "
                         "preprocess.ClipCollate: the evaluation transform, or with --augment one box and one flip per clip")
    ap.add_argument("--yuv", default=None, choices=["i420", "nv12", "i422", "i444", "i420p10", "i422p10", "i444p10", "p010",
                                                    "i420p12", "p012", "p016", "i444p16"],
                    help="with --augment or --ragged: the decoded frames are YUV ([..., rows, W], PyAV's to_ndarray() of yuv420p / "
                         "nv12 / yuv422p / yuv444p / yuv420p10le / p010le ..., uint16 above 8 bits); the conversion to RGB runs inside "
                         "the device transform")
    return ap


def main():
    a = build_parser().parse_args()
    if a.yuv and (a.uint8 or not (a.augment or a.ragged)):
        raise SystemExit("--yuv describes decoded frames: it goes with --augment or --ragged 1, without --uint8 1")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    if world > 1:
        torch.distributed.init_process_group("nccl")
    c = bench.CFG2
    if a.b16:
        c = dict(c, name="cfg5-shaped: ViT-B/16", patch=16, T_new=4, K=100)
    if a.l14:
        c = L14
    args = l14_task_config(c) if a.l14 else bench.task_config(c)
    args.sim_header, args.cross_num_hidden_layers = a.sim_header, a.cross_num_hidden_layers
    args.linear_patch = a.linear_patch
    args.camoe_dsl = a.camoe_dsl
    args.quick_gelu = a.quick_gelu
    if a.algo != "kmediods++":
        args.cluster_algo = a.algo
        shift_plan(args)
    sd = l14_state_dict(c, seed=0) if a.l14 else bench.random_state_dict(c, seed=0)
    model = CLIP4Clip.from_state_dict(sd, args).float().to(device)
    model.freeze_cip_layers(a.freeze_layer_num)             # (main.py:102, before the optimizer is built)
    targs = Namespace(lr=a.lr, wd=0.2, new_added_modules=["Cross", "cluster_embed"], gradient_accumulation_steps=1,
                      clip_grad_norm=None, optim=a.optim)
    total = 100 * a.steps

    def make_opt(capturable=False):
        """-> (optimizer, scheduler) of main.py:168-175 for --optim"""
        groups = prep_optim_params_groups(targs, model, coef_lr=a.coef_lr)
        if a.optim == "AdamW":
            return (AdamW(groups, lr=targs.lr, betas=(0.9, 0.98), eps=1e-6, weight_decay=targs.wd, capturable=capturable),
                    lr_scheduler('cos', init_lr=targs.lr, all_iters=total, slow_start_iters=0.1 * total, weight_decay=targs.wd))
        return BertAdam(groups, lr=targs.lr, warmup=0.1, t_total=total, schedule='warmup_cosine', b1=0.9, b2=0.98, e=1e-6,
                        max_grad_norm=1.0, capturable=capturable), None
    if a.optim == "AdamW":
        targs.clip_grad_norm = 1.0                          # main.py's default --clip_grad_norm
    opt, sched = make_opt()
    buckets = ccdist.GradientBuckets(model.parameters()) if world > 1 else None
    data = SyntheticRetrieval(a.batch * a.steps, seed=rank)
    if a.uint8:
        data.video = torch.randint(0, 256, data.video.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(rank))
    augment = None
    if a.augment is not None:
        if not a.uint8:                                     # frames as a decoder leaves them: uint8 [n, 1, T, H, W, 3]
            H, W = (int(v) for v in a.raw_frames.split(","))
            g = torch.Generator().manual_seed(rank)
            if a.yuv:
                from eval_synthetic import yuv_frames
                data.video = yuv_frames(a.yuv, data.video.shape[:3], H, W, g)
            else:
                data.video = torch.randint(0, 256, data.video.shape[:3] + (H, W, 3), dtype=torch.uint8, generator=g)
        augment = TrainFrameTransform(224, crop=a.augment, flip=bool(a.flip), seed=rank)
        if a.yuv:
            augment = YuvTrainFrameTransform(224, layout=a.yuv, crop=a.augment, flip=bool(a.flip), seed=rank)
    elif a.flip:
        raise SystemExit("--flip 1 goes with --augment")
    loader = torch.utils.data.DataLoader(data, batch_size=a.batch, shuffle=False)
    if a.ragged:
        from centerclip_amd.preprocess import ClipCollate, YuvClipCollate
        from eval_synthetic import RaggedRetrieval
        data = RaggedRetrieval(a.batch * a.steps, frames=c["T"], seed=rank, yuv=a.yuv)
        loader = torch.utils.data.DataLoader(data, batch_size=a.batch, shuffle=False, collate_fn=data.collate)
        augment = (YuvClipCollate(c["res"], max_frames=c["T"], train=augment, layout=a.yuv) if a.yuv
                   else ClipCollate(c["res"], max_frames=c["T"], train=augment))
    if a.same_batch:
        loader = [next(iter(loader))] * a.steps
    t, dts = [time.time()], []                              # the last time stamp; every step's duration

    def log(epoch, step, loss, sim_loss, gs):
        torch.cuda.synchronize()
        dts.append(time.time() - t[0])
        t[0] += dts[-1]
        if rank == 0:
            print("step %d  loss %.4f  %.0f ms" % (gs, loss, dts[-1] * 1e3), flush=True)
    scaler = DeviceGradScaler() if a.precision == "amp" else None          # (main.py:160: GradScaler(), init_scale 2^16)
    start_epoch, global_step, best = 0, 0, float("inf")
    if a.resume is not None:                                # main.py:185-212 (every rank reads the same file)
        t0 = time.time()
        start_epoch, global_step, _ = resume(a.resume, model, opt, scaler)
        torch.cuda.synchronize()
        if rank == 0:
            print("resumed %s in %.2f s: continuing from epoch %d, global_step %d" % (a.resume, time.time() - t0, start_epoch, global_step))
    if a.output_dir is not None and rank == 0:
        os.makedirs(a.output_dir, exist_ok=True)
    for epoch in range(start_epoch, a.epochs):
        t[0] = time.time()                                  # (a resume or a save is not part of the next step's time)
        tr_loss, global_step = train_epoch(epoch, targs, model, loader, device, opt, global_step, scheduler=sched, buckets=buckets,
                                           log=log, scaler=scaler, frame_transform=augment)
        if rank == 0:
            print("epoch %d/%d finished, train loss %.6f" % (epoch + 1, a.epochs, tr_loss))
        if a.output_dir is not None and rank == 0:          # main.py:262-272 (rank 0 saves)
            t0 = time.time()
            state = checkpoint_dict(model, opt, epoch + 1, global_step, best_acc1=0.0, scaler=scaler)
            save_checkpoint(state, tr_loss <= best, a.output_dir, filename='ckpt.pth.tar')
            best = min(best, tr_loss)
            print("saved %s in %.2f s" % (os.path.join(a.output_dir, 'ckpt.pth.tar'), time.time() - t0))
    if scaler is not None and rank == 0:
        print("eager, DeviceGradScaler: %d steps taken, %d skipped, scale %g" % (scaler.counters() + (scaler.get_scale(),)))
    if rank == 0:
        steady = sum(dts[2:]) / len(dts[2:]) if len(dts) > 2 else float("nan")
        print("steady step %.0f ms = %.1f clips/s per rank (unfused per-op training path, launched op by op)" % (steady * 1e3, a.batch / steady))
    if a.graph and world == 1:
        # the same step (forward, backward, optimizer, clamp) as ONE hipGraph on static input buffers (train.GraphedTrainStep):
        # no op of it synchronises with the host, so what remains is the GPU time of the unfused kernels
        from centerclip_amd.train import GraphedTrainStep
        gopt, gsched = make_opt(capturable=True)
        gscaler = DeviceGradScaler() if a.precision == "amp" else None
        stepper = GraphedTrainStep(model, gopt, scheduler=gsched, clip_grad_norm=targs.clip_grad_norm, scaler=gscaler)
        batch = next(iter(loader))
        if augment is not None:                             # (the captured step takes model-resolution frames)
            batch = tuple(batch[:3]) + (augment(batch[3].to(device)),) + tuple(batch[4:])
        if a.resume is not None:                            # in place of a first call's fresh start: restored, then captured
            t0 = time.time()
            g_epoch, g_step, _ = resume(a.resume, model, step=stepper)
            torch.cuda.synchronize()
            print("captured step resumed %s in %.2f s: continuing from epoch %d, global_step %d" % (a.resume, time.time() - t0, g_epoch, g_step))
        gloss = stepper(batch)
        for _ in range(3):
            stepper(batch)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(10):
            gloss = stepper(batch)
        torch.cuda.synchronize()
        ms = (time.time() - t0) / 10 * 1e3
        print("captured step (%s): %.1f ms = %.0f clips/s (loss %.4f)" % (a.optim, ms, a.batch / ms * 1e3, float(gloss)))
        if gscaler is not None:
            stepper.sync()                                  # the last call's step count (settled one call late)
            print("captured, DeviceGradScaler: %d steps taken, %d skipped, scale %g" % (gscaler.counters() + (gscaler.get_scale(),)))
        if a.output_dir is not None:
            t0 = time.time()
            save_checkpoint(stepper.state_dict(epoch=a.epochs), False, a.output_dir, filename='ckpt.graph.pth.tar')
            print("captured step: state_dict() + save_checkpoint %.2f s (global_step %d)" % (time.time() - t0, stepper.global_step))
    if a.optim_timing and rank == 0:
        optimizer_timing(model, device)
    if world > 1:
        torch.distributed.destroy_process_group()


def optimizer_timing(model, device, reps=20):
    """The optimizer step alone over the model's parameters (fp32 master weights, random gradients), each captured into a
    hipGraph and replayed (no host time inside the measurement), median of `reps` by device events: HIP AdamW.step, HIP
    AdamW.clip_and_step, torch.optim.AdamW(fused=True).step alone and after torch.nn.utils.clip_grad_norm_."""
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    hp = dict(lr=1e-7, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
    ours = AdamW(params, capturable=True, **hp)
    fused = torch.optim.AdamW(params, fused=True, capturable=True, **hp)

    def timed(fn):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                          # eager warm-up (staging buffers, torch's state)
            fn()
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]
    t_step = timed(ours.step)
    t_clip = timed(lambda: ours.clip_and_step(1.0))
    t_torch_step = timed(fused.step)
    t_torch = timed(lambda: (torch.nn.utils.clip_grad_norm_(params, 1.0), fused.step()))
    gb = 28.0 * n / 1e9                                     # p, m, v read + written, g read (fp32)
    print("optimizer over %d tensors, %.1f M parameters (%.2f GB per AdamW step), captured + replayed:" % (len(params), n / 1e6, gb))
    print("  HIP AdamW.step               %.3f ms  (%.2f TB/s)" % (t_step, gb / t_step))
    print("  HIP AdamW.clip_and_step      %.3f ms" % t_clip)
    print("  torch AdamW(fused=True).step %.3f ms  (%.2f TB/s)" % (t_torch_step, gb / t_torch_step))
    print("  torch clip_grad_norm_ + torch AdamW(fused=True).step %.3f ms" % t_torch)


if __name__ == "__main__":
    main()
