"""The training loop: ``train_epoch`` (main.py:291-378, launched op by op) and ``GraphedTrainStep``, the same step
(main.py:300-340 for one batch) captured into a hipGraph and replayed on static input buffers.
"""
import gc

import torch

from .checkpoint import checkpoint_dict, restore
from .optim import AdamW, clip_grad_norm_
from .scaler import DeviceGradScaler, _device_scaler


def train_epoch(epoch, args, model, train_dataloader, device, optimizer, global_step, scheduler=None, buckets=None,
                log=None, scaler=None, frame_transform=None):
    """main.py:291-378 for this path: zero_grad -> forward (training branch of CLIP4Clip.forward) -> backward ->
    [gradient average over the ranks, dist.GradientBuckets] -> [clip_grad_norm_] -> optimizer.step -> clamp logit_scale.
    ``model``: a centerclip_amd.clip4clip.CLIP4Clip in training mode.  -> (mean loss, global_step).

    ``scaler`` (main.py:309-330, the reference's ``--fp16`` branch): a ``torch.cuda.amp.GradScaler`` (or anything with its
    scale / unscale_ / step / update).  The forward here always feeds the matrix cores fp16 operands with fp32 accumulation
    and keeps fp32 master weights - what ``autocast`` gives the reference - so the branch adds what the scaler itself does:
    the loss is multiplied by the scale before backward (the HIP backward picks a power-of-two scale per gradient tensor on
    the device, so the factor passes through exactly), gradients are unscaled (and averaged over the ranks) before clipping,
    a step whose gradients hold an inf / NaN is skipped and the scale backed off, as GradScaler.step / update do.
    A ``DeviceGradScaler`` runs the same branch without a host decision (no unscaling pass, no .item() on found_inf); its
    clipping is its own clip_grad_norm_ over the optimizer's parameters, folded into the step's one multiplier.

    ``frame_transform`` (not in the reference, whose loader does this per frame on the CPU): a ``preprocess.FrameTransform`` -
    the loader hands over decoded uint8 frames of any size, resized and centre-cropped on the device right after the copy.
    None: the loop as it always was."""
    model.train()
    total_loss, nb = 0.0, 0
    for step, batch in enumerate(train_dataloader):
        optimizer.zero_grad()
        if scheduler is not None:
            scheduler(optimizer, global_step=global_step)
        input_ids, input_mask, segment_ids, video, video_mask = tuple(t.to(device=device, non_blocking=True) for t in batch)
        if frame_transform is not None:
            video = frame_transform(video)
        output = model(input_ids, segment_ids, input_mask, video, video_mask)
        loss = output['loss'].mean()
        if args.gradient_accumulation_steps > 1:
            loss = loss / args.gradient_accumulation_steps
        if scaler is not None:
            scaler.scale(loss).backward()
        else:
            loss.backward()
        if (step + 1) % args.gradient_accumulation_steps == 0:
            if buckets is not None:
                buckets.reduce()
            if scaler is not None:
                if getattr(args, "clip_grad_norm", None) is not None:
                    scaler.unscale_(optimizer)           # (clipping sees the true gradients, main.py:324-326)
                    if isinstance(scaler, DeviceGradScaler) and scaler.is_enabled():
                        scaler.clip_grad_norm_(optimizer, args.clip_grad_norm)     # (fused into step(): one multiplier)
                    else:
                        torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_grad_norm)
                scaler.step(optimizer)                   # skipped when a gradient holds an inf / NaN
                scaler.update()
            else:
                if getattr(args, "clip_grad_norm", None) is not None:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_grad_norm)
                optimizer.step()
            global_step += 1
        with torch.no_grad():                                    # (main.py:336-340; tracked, so the cached copies refresh)
            model.clip.logit_scale.clamp_(0.1, 4.6052)
        if log is not None:
            log(epoch, step, float(loss.detach()), float(output['sim_loss'].detach()), global_step)
        total_loss += float(loss.detach())
        nb += 1
    if isinstance(scaler, DeviceGradScaler):
        scaler.sync()                                            # the last step's count
    return total_loss / max(nb, 1), global_step


class GraphedTrainStep:
    """One training step (forward, backward, optimizer, logit_scale clamp - main.py:300-340 for one batch) captured into a
    hipGraph and replayed on static input buffers: no op of the step synchronises with the host, so the replay runs at the GPU
    time of its kernels instead of the host's launch rate (cfg-2 shape: 19 ms against 40-100 ms launched op by op).
    Single process (a captured step cannot contain the RCCL exchange of GradientBuckets); fixed batch shape; an optimizer
    built with capturable=True.  The first call warms up eagerly (2 steps on the given batch) and captures - on a snapshot:
    parameters, moments and step counts are put back before the one replay that counts, so that EVERY call, the first
    included, is exactly one optimizer step (main.py:300-340) and the schedule position equals the caller's step count."""

    def __init__(self, model, optimizer, gradient_accumulation_steps=1, scheduler=None, clip_grad_norm=None, global_step=0,
                 scaler=None):
        """scaler: a DeviceGradScaler - the launchers' precision=amp recipe (main.py:320-328) inside the captured step: scale
        the loss, backward, gradient statistics, clip-and-step or step (skipped on the device when a gradient holds an inf /
        NaN), scale update, logit_scale clamp.  A torch.amp.GradScaler is accepted too: its hyper-parameters and state are
        copied into a DeviceGradScaler (self.scaler), and write_back_scaler() copies the state back.  None or a disabled
        scaler: exactly the graph without one.  A skipped step does not advance the optimizer's state['step'] while
        global_step advances (main.py:344-345); the count of call k is settled at the start of call k + 1 (the flag arrives in
        a pinned word the graph writes; see DeviceGradScaler) - call sync() before optimizer.state_dict().
        scheduler (e.g. lr_scheduler): called as scheduler(optimizer, global_step=k) on the host before every step, k = the
        number of calls made so far + global_step (main.py:302); its lr reaches the captured step through refresh_lr().
        clip_grad_norm: global gradient clipping inside the captured step, before the optimizer (main.py:327-333) -
        AdamW.clip_and_step, or clip_grad_norm_ then step() for BertAdam."""
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs BertAdam(..., capturable=True) or AdamW(..., capturable=True)")
        if gradient_accumulation_steps != 1:
            raise NotImplementedError("GraphedTrainStep: gradient accumulation is not built")
        self.model, self.optimizer = model, optimizer
        self.scheduler, self.clip_grad_norm, self.global_step = scheduler, clip_grad_norm, int(global_step)
        self._moments = ('exp_avg', 'exp_avg_sq') if isinstance(optimizer, AdamW) else ('next_m', 'next_v')
        self.scaler, self._torch_scaler = _device_scaler(scaler)
        self.graph = self.static = self.loss = None

    def sync(self):
        """Settle the last call's step count (with a scaler it is known only once that call has run): waits for it."""
        if self.scaler is not None:
            self.scaler.sync()

    def write_back_scaler(self):
        """Copy the device scaler's state (scale, growth tracker, hyper-parameters) into the torch.amp.GradScaler this step
        was built from, e.g. before a checkpoint saves that object's state_dict (main.py:262-272); -> that GradScaler.
        Without one (a DeviceGradScaler was passed: it IS the state) -> None."""
        if self._torch_scaler is None:
            return None
        self._torch_scaler.load_state_dict(self.scaler.state_dict())
        return self._torch_scaler

    def state_dict(self, epoch=0, best_acc1=0.0):
        """The checkpoint dictionary (train.checkpoint_dict) of this step's model, optimizer, scaler and global_step, with the
        last call's step count settled first; epoch and best_acc1 are the caller's and pass through."""
        return checkpoint_dict(self.model, self.optimizer, epoch, self.global_step, best_acc1=best_acc1, step=self)

    def load_state_dict(self, d, load_from_pretrained=False):
        """Restore a checkpoint dictionary -> (start_epoch, global_step, best_acc1); the next call is step global_step + 1 of
        the resumed run.  Before the first call it is the plain restore (train.resume): warm-up, capture and the put-back
        of the snapshot then run on the restored values.  After the capture the same restore is entirely in place - the
        graph holds the addresses of the parameters, of the moments and of the scaler's words - and nothing is captured again:
        a checkpoint that would need a new tensor (another shape, no state for a parameter the graph updates, another value
        for a frozen parameter) raises before anything is written."""
        self.sync()                                               # (a pending count belongs to the state about to be replaced)
        out = restore(d, self.model, self.optimizer, self.scaler, load_from_pretrained, captured=self.graph is not None)
        if not load_from_pretrained:
            self.global_step = out[1]
            self.write_back_scaler()
        return out

    def _schedule(self):
        if self.scheduler is not None:
            self.scheduler(self.optimizer, global_step=self.global_step)

    def _step(self):
        self.optimizer.zero_grad(set_to_none=True)       # (captured: the gradients live in the graph's pool, no fill + accumulate)
        out = self.model(self.static[0], self.static[2], self.static[1], self.static[3], self.static[4])
        loss = out['loss'].mean()
        if self.scaler is not None:
            sc = self.scaler
            sc.scale(loss).backward()
            if self.clip_grad_norm is not None:
                sc.unscale_(self.optimizer)
                sc.clip_grad_norm_(self.optimizer, self.clip_grad_norm)
            sc.step(self.optimizer)
            sc.update()
        else:
            loss.backward()
            if self.clip_grad_norm is None:
                self.optimizer.step()
            elif isinstance(self.optimizer, AdamW):
                self.optimizer.clip_and_step(self.clip_grad_norm)
            else:
                clip_grad_norm_([p for g in self.optimizer.param_groups for p in g['params']], self.clip_grad_norm)
                self.optimizer.step()
        with torch.no_grad():
            self.model.clip.logit_scale.clamp_(0.1, 4.6052)
        return loss.detach()

    def _tensors(self):
        # (a frozen parameter cannot change in a step: it is neither copied nor written back - the packed copies of a frozen
        #  prefix, whose addresses the captured graph holds, stay valid)
        seen, out = set(), []
        for p in list(self.model.parameters()) + [p for g in self.optimizer.param_groups for p in g['params']]:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                out.append(p)
        return out

    def _snapshot(self):
        """Copies of everything a step changes: every parameter, and per parameter the optimizer's (step, first moment, second
        moment) - next_m / next_v for BertAdam, exp_avg / exp_avg_sq for AdamW."""
        snap = []
        km, kv = self._moments
        for p in self._tensors():
            st = self.optimizer.state.get(p, {})
            snap.append((p, p.detach().clone(), st.get('step'), st[km].clone() if km in st else None,
                         st[kv].clone() if kv in st else None))
        return snap

    @torch.no_grad()
    def _restore(self, snap):
        """In place (the captured graph holds the addresses of the parameters and of the moments the warm-up created);
        Tensor.copy_ bumps the version counter, so cached fp16 / folded copies of the weights refresh."""
        km, kv = self._moments
        for p, value, step, m, v in snap:
            p.copy_(value)
            st = self.optimizer.state.get(p)
            if not st:
                continue
            st['step'] = 0 if step is None else step
            st[km].zero_() if m is None else st[km].copy_(m)
            st[kv].zero_() if v is None else st[kv].copy_(v)

    def __call__(self, batch):
        """batch = (input_ids, input_mask, segment_ids, video, video_mask) as the dataloaders yield it -> the step's loss (a
        device tensor that the next call overwrites)."""
        dev = next(self.model.parameters()).device
        if self.graph is None:
            self.model.train()
            self.static = [t.to(dev).clone() for t in batch]
            snap = self._snapshot()
            if self.scaler is not None:
                self.scaler.sync()                                # (an eager step the caller made with it before)
                self.scaler._ensure(dev)
                sc_snap = self.scaler._snapshot()
            for _ in range(2):                                    # allocator / staging-buffer warm-up (the optimizer's records)
                self._schedule()
                self._step()
            if self.scaler is not None:
                self.scaler.sync()                                # (no host wait may fall into the capture)
            torch.cuda.synchronize()
            # dead reference cycles can own hipGraphs (a model that ran eval_epoch(graphed=True) holds its lanes and they hold
            # it); on ROCm a CUDAGraph's destructor synchronises the device, which ends the process when the cycle collector
            # happens to run it inside a capture - and torch.cuda.graph no longer collects before it begins
            gc.collect()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):                    # (the capture pass does not execute)
                self.loss = self._step()
            self._restore(snap)                                   # the two warm-up steps never happened
            if self.scaler is not None:
                self.scaler._restore(sc_snap)                     # ... nor did their scale updates and counters
            return self._replay()
        self.sync()                                               # the previous call's count, BEFORE this call's work is enqueued
        for dst, src in zip(self.static, batch):
            dst.copy_(src, non_blocking=True)
        return self._replay()

    def _replay(self):
        self._schedule()
        self.optimizer.refresh_lr()
        self.graph.replay()
        if self.scaler is not None:
            self.scaler._mark(self.optimizer, "graph")            # counted (or not) by the next sync()
        else:
            self.optimizer.advance()
        self.global_step += 1
        return self.loss
