"""The optimizers of main.py:161-175 on the HIP kernels, and what surrounds them:

* ``BertAdam`` (utils/optimization.py:55-170) with its warmup schedules, on the multi-tensor kernels of csrc/bertadam.hip:
  one record per tensor (cc_bertadam_item), every tensor of a step in one launch pair;
* ``AdamW`` and ``clip_grad_norm_`` (torch.optim.AdamW, torch.nn.utils.clip_grad_norm_; main.py:168-175, 316-333) on the
  multi-tensor kernels of csrc/adamw.hip: one record per tensor (cc_adamw_item), every tensor of a step in one launch;
* ``lr_scheduler`` (utils/lr_scheduler.py) and ``prep_optim_params_groups`` (utils/optimization.py:173-222): host arithmetic.

The multi-tensor launches read small host-built record tables; ``_Staged`` is the one way such a table reaches the device,
eagerly and inside a captured step.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from ..torch_ops import _st



# ================================================================================================ schedules
def warmup_cosine(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    return 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x, warmup=0.002):
    return x / warmup if x < warmup else 1.0


def warmup_linear(x, warmup=0.002):
    return x / warmup if x < warmup else max((x - 1.) / (warmup - 1.), 0)


SCHEDULES = {'warmup_cosine': warmup_cosine, 'warmup_constant': warmup_constant, 'warmup_linear': warmup_linear}


# ================================================================================================ record tables
def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _Staged:
    """A small host-built table in device memory (the optimizers' per-tensor records, the per-class scalars): uploaded through
    pinned memory when its bytes change.  A captured step stages its own copy - the graph replays that host-to-device copy from
    a pinned buffer set aside during the eager warm-up, so later eager uploads never touch what the graph reads."""

    def __init__(self, who):
        self.who, self.raw, self.dev, self.spare, self.keep = who, None, None, None, []

    def upload(self, raw, device, capturing):
        if capturing:
            host, dev = self.spare if self.spare is not None else (None, None)
            self.spare = None
            if host is None or host.numel() != len(raw):
                raise RuntimeError("%s: run one eager step with the same parameters before capturing (staging buffers)" % self.who)
            host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            dev.copy_(host, non_blocking=True)
            self.keep.append((host, dev))                     # the graph reads both on every replay
            return dev
        if self.raw != raw:
            host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
            if self.dev is None or self.dev.numel() != len(raw) or self.dev.device != device:
                self.dev = torch.empty(len(raw), dtype=torch.uint8, device=device)
            self.dev.copy_(host, non_blocking=True)
            self.raw = raw
        if self.spare is None or self.spare[0].numel() != len(raw):
            self.spare = (torch.empty(len(raw), dtype=torch.uint8).pin_memory(),
                          torch.empty(len(raw), dtype=torch.uint8, device=device))
        return self.dev


class _Optimizer(torch.optim.Optimizer):
    """What BertAdam and AdamW share: the staged record tables and the host-side step counts of the last eager step."""

    def __init__(self, params, defaults, capturable):
        super().__init__(params, defaults)
        self.capturable = bool(capturable)     # a step can be captured into a hipGraph and replayed (refresh_lr / advance)
        self._staged = {}                      # key -> _Staged: the record tables of this optimizer's launches
        self._last = []                        # the parameters whose state['step'] the last eager step advanced

    def _table(self, key, raw, device, capturing):
        return self._staged.setdefault(key, _Staged(type(self).__name__)).upload(raw, device, capturing)

    def _uncount(self):
        """The last eager step turned out to be skipped on the device (DeviceGradScaler): take its count back."""
        for p in self._last:
            self.state[p]['step'] -= 1
        self._last = []

    _moment_keys = ()                          # the two moment tensors of a parameter's state (set by the subclasses)

    def _pinned(self):
        """The parameters whose moments a captured step holds by address: their state can only be restored in place."""
        return ()

    def _check_state_dict(self, state_dict):
        """Everything load_state_dict needs of a state dict, checked without a write: the group structure, per parameter
        with state a 'step' and both moments in the parameter's shape, and for the parameters of a captured step (_pinned)
        state to copy from and one step count per captured class.  Raises ValueError."""
        who = type(self).__name__
        saved = state_dict['param_groups']
        if len(saved) != len(self.param_groups):
            raise ValueError("%s.load_state_dict: %d parameter groups in the state dict, %d here"
                             % (who, len(saved), len(self.param_groups)))
        ids = {}
        for gi, (group, sg) in enumerate(zip(self.param_groups, saved)):
            if len(group['params']) != len(sg['params']):
                raise ValueError("%s.load_state_dict: group %d holds %d parameters in the state dict, %d here"
                                 % (who, gi, len(sg['params']), len(group['params'])))
            for p, sid in zip(group['params'], sg['params']):
                ids[p] = (sid, gi)
        state = state_dict['state']
        for p, (sid, gi) in ids.items():
            st = state.get(sid)
            if not st:
                continue
            for k in ('step',) + self._moment_keys:
                if k not in st:
                    raise ValueError("%s.load_state_dict: the state of parameter %r has no %r" % (who, sid, k))
            for k in self._moment_keys:
                if not torch.is_tensor(st[k]) or st[k].shape != p.shape:
                    raise ValueError("%s.load_state_dict: %s of parameter %r is %s, the parameter is %s"
                                     % (who, k, sid, tuple(getattr(st[k], 'shape', ())), tuple(p.shape)))
        counts = {}
        for p in self._pinned():
            sid, gi = ids[p]
            if not state.get(sid):
                raise ValueError("%s.load_state_dict: the captured step updates parameter %r, and the state dict has no state "
                                 "for it (its moments can only be restored in place)" % (who, sid))
            counts.setdefault((gi, int(self.state[p]['step'])), set()).add(int(state[sid]['step']))
        if any(len(c) > 1 for c in counts.values()):
            raise ValueError("%s.load_state_dict: parameters the captured step counts together have different step counts in "
                             "the state dict" % who)

    def load_state_dict(self, state_dict):
        """torch's load_state_dict (group hyper-parameters from the state dict, state cast to each parameter's dtype and
        device), except that a parameter that already has moments of the same shape, dtype and device keeps those tensors: the
        loaded values are copied into them.  A captured step and the record tables (_Staged) hold their addresses - moments
        that torch had swapped for new tensors would be ignored by every replay, silently.  Checked before the first write
        (_check_state_dict): a state dict that does not fit raises ValueError and changes nothing."""
        self._check_state_dict(state_dict)
        kept = {p: st for p, st in self.state.items() if len(st)}
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for p, old in kept.items():
                new = self.state.get(p)
                if not new:
                    continue
                for k in self._moment_keys:
                    a, b = old.get(k), new.get(k)
                    if torch.is_tensor(a) and torch.is_tensor(b) and (a.shape, a.dtype, a.device) == (b.shape, b.dtype, b.device):
                        new[k] = a.copy_(b)
        for st in self.state.values():
            if torch.is_tensor(st.get('step')):
                st['step'] = int(st['step'].item())
        self._last = []                        # (no _uncount reaches back across a restore)


_ADAMW_ITEM = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('n', '<i8'), ('blk0', '<i4'),
                        ('blocks', '<i4'), ('scal', '<i4'), ('pad', '<i4')])
_adamw_blocks_cache = {}


def _adamw_table(entries):
    """entries: (param, grad, exp_avg or None, exp_avg_sq or None, scalar index) -> (cc_adamw_item records as bytes, count,
    total blocks).  Empty tensors get no record."""
    lib = L.lib()
    entries = [e for e in entries if e[0].numel() > 0]
    rec = np.zeros(len(entries), dtype=_ADAMW_ITEM)
    blk0 = 0
    for i, (p, g, m, v, si) in enumerate(entries):
        n = p.numel()
        nb = _adamw_blocks_cache.get(n)
        if nb is None:
            nb = _adamw_blocks_cache[n] = int(lib.cc_adamw_blocks(n))
        rec[i] = (p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(), n, blk0, nb,
                  si, 0)
        blk0 += nb
    return rec.tobytes(), len(entries), blk0


def _grads_table(grads):
    """_adamw_table over gradients alone: what the norm and scale kernels read of a record."""
    return _adamw_table([(g, g, None, None, 0) for g in grads])


_BERTADAM_ITEM = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('lr_dev', '<u8'), ('n', '<i8'),
                           ('lr', '<f4'), ('wd', '<f4'), ('norm_blk0', '<i4'), ('norm_blocks', '<i4'), ('step_blk0', '<i4'),
                           ('step_blocks', '<i4')])
_bertadam_blocks_cache = {}


def _bertadam_table(entries):
    """entries: (param, grad, next_m, next_v, lr, weight decay), lr a float or a 1-element device tensor (a record's lr or
    its lr_dev) -> (cc_bertadam_item records as bytes, count, total norm blocks, total step blocks).  Empty tensors get no
    record."""
    lib = L.lib()
    entries = [e for e in entries if e[0].numel() > 0]
    rec = np.zeros(len(entries), dtype=_BERTADAM_ITEM)
    nb0 = sb0 = 0
    for i, (p, g, m, v, lr, wd) in enumerate(entries):
        n = p.numel()
        blocks = _bertadam_blocks_cache.get(n)
        if blocks is None:
            blocks = _bertadam_blocks_cache[n] = (int(lib.cc_bertadam_norm_blocks(n)), int(lib.cc_bertadam_step_blocks(n)))
        lr_dev, lr = (lr.data_ptr(), 0.0) if torch.is_tensor(lr) else (0, lr)
        rec[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr_dev, n, lr, wd, nb0, blocks[0], sb0, blocks[1])
        nb0 += blocks[0]
        sb0 += blocks[1]
    return rec.tobytes(), len(entries), nb0, sb0


def _norm_partials(table, count, nblk, device, st):
    """cc_grad_norm_partials_f32 over the table's gradients -> the workspace that holds the nblk partial sums."""
    lib = L.lib()
    ws = L.workspace(lib.cc_grad_norm_workspace_bytes(nblk), device)
    L.check(lib.cc_grad_norm_partials_f32(L.ptr(table), count, nblk, L.ptr(ws), ws.numel(), st), "cc_grad_norm_partials_f32")
    return ws


def _clip_launches(table, count, nblk, max_norm, device, coef_only=False):
    """||g|| over the table's gradients and the clip coefficient -> a [2] device float tensor (norm, coef); unless coef_only,
    the gradients are multiplied by the coefficient in place (cc_grad_scale_f32)."""
    lib = L.lib()
    out = torch.empty(2, dtype=torch.float32, device=device)
    st = _st(out)
    ws = _norm_partials(table, count, nblk, device, st)
    L.check(lib.cc_grad_clip_coef_f32(L.ptr(ws), nblk, float(max_norm), L.ptr(out), st), "cc_grad_clip_coef_f32")
    if not coef_only:
        L.check(lib.cc_grad_scale_f32(L.ptr(table), count, nblk, L.ptr(out[1:]), st), "cc_grad_scale_f32")
    return out


_clip_staged = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ (L2): the gradients are scaled in place by min(1, max_norm / (||g|| + 1e-6)), and the
    total norm comes back as a 0-d device tensor.  HIP kernels only (cc_grad_norm_partials_f32 -> cc_grad_clip_coef_f32 ->
    cc_grad_scale_f32): no host synchronisation, capturable.  The fp64 partial sums are added in the order of `parameters`,
    so the same parameters in the same order give the same bits."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_ (HIP): only the L2 norm (norm_type=2), as main.py uses it")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        L.require_device(g)
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
            raise RuntimeError("clip_grad_norm_ (HIP): fp32 contiguous gradients on one device")
    raw, count, nblk = _grads_table(grads)
    if count == 0:
        return torch.zeros((), dtype=torch.float32, device=dev)
    table = _clip_staged.setdefault((dev, len(raw)), _Staged("clip_grad_norm_")).upload(raw, dev, _capturing())
    return _clip_launches(table, count, nblk, max_norm, dev)[0]


# ================================================================================================ BertAdam
class BertAdam(_Optimizer):
    """utils/optimization.py:55-170 (the optimizer main.py:161-167 builds): same constructor, same state names
    ('step', 'next_m', 'next_v'), same per-tensor clipping / decoupled weight decay / schedule; the tensor arithmetic of a
    step is one cc_bertadam_multi_f32 call (a norm and a step launch over one record per tensor, csrc/bertadam.hip) per
    (b1, b2, e, max_grad_norm) class, no host synchronisation."""

    def __init__(self, params, lr, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, capturable=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        # capturable (not in the reference): the scheduled learning rate of each group reaches the kernels through a device
        # float, so a step captured into a hipGraph can be replayed with the schedule's next value (GraphedTrainStep)
        super().__init__(params, dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e,
                                      weight_decay=weight_decay, max_grad_norm=max_grad_norm), capturable)
        self._lr_dev = {}                      # group index -> its learning rate as a 1-element device tensor (capturable)
        self._partial = {}                     # (b1, b2, e, max_grad_norm) -> the large tensors' fp64 norm partial sums

    _moment_keys = ('next_m', 'next_v')

    def _pinned(self):
        if not any(s.keep for s in self._staged.values()):        # (no table staged under a capture: nothing captured)
            return ()
        return [p for g in self.param_groups for p in g['params'] if p in self.state and len(self.state[p])]

    @staticmethod
    def _lr(group, step):
        if group['t_total'] != -1:
            return group['lr'] * SCHEDULES[group['schedule']](step / group['t_total'], group['warmup'])
        return group['lr']

    def get_lr(self):
        lr = []
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    return [0]
                lr.append(self._lr(group, state['step']))
        return lr

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._step(None)
        return loss

    def _step(self, sc):
        """One step over the parameters that have a gradient: per (b1, b2, e, max_grad_norm) class one record table and one
        cc_bertadam_multi_f32 call.  ``sc``: None, or the (multiplier, found_inf) device floats of DeviceGradScaler.step -
        cc_bertadam_multi_scaled_f32.  The learning rate: capturable, the group's device float; otherwise each record holds
        its parameter's own scheduled value."""
        lib = L.lib()
        capturing = _capturing()
        if capturing and not self.capturable:
            raise RuntimeError("BertAdam: build it with capturable=True to capture its step")
        classes = {}                                              # (b1, b2, e, max_grad_norm) -> _bertadam_table entries
        if not capturing:
            self._last = []
        for gi, group in enumerate(self.param_groups):
            lr_set = False
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("BertAdam (HIP): fp32 contiguous parameters (the master weights)")
                L.require_device(p)
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['next_m'] = torch.zeros_like(p)
                    state['next_v'] = torch.zeros_like(p)
                if self.capturable:
                    lr = self._lr_dev.get(gi)
                    if lr is None or lr.device != p.device:
                        lr = self._lr_dev[gi] = torch.zeros(1, device=p.device, dtype=torch.float32)
                    if not capturing and not lr_set:
                        lr.fill_(float(self._lr(group, state['step'])))
                        lr_set = True
                else:
                    lr = float(self._lr(group, state['step']))
                hyper = (float(group['b1']), float(group['b2']), float(group['e']), float(group['max_grad_norm']))
                classes.setdefault(hyper, []).append((p, p.grad, state['next_m'], state['next_v'], lr,
                                                      float(group['weight_decay'])))
                if not capturing:
                    state['step'] += 1
                    self._last.append(p)
        for hyper, entries in classes.items():
            raw, count, nb, sb = _bertadam_table(entries)
            if count == 0:
                continue
            device = entries[0][0].device
            part = self._partial.get(hyper)
            if nb and (part is None or part.numel() < nb):
                if capturing:
                    raise RuntimeError("BertAdam: run one eager step with the same parameters before capturing (partial sums)")
                part = self._partial[hyper] = torch.empty(nb, dtype=torch.float64, device=device)
            table = self._table(hyper, raw, device, capturing)
            args = (L.ptr(table), count, nb, sb) + hyper + (L.ptr(part), 0 if part is None else part.numel() * 8)
            if sc is not None:
                L.check(lib.cc_bertadam_multi_scaled_f32(*args, L.ptr(sc[0]), L.ptr(sc[1]), _st(table)),
                        "cc_bertadam_multi_scaled_f32")
            else:
                L.check(lib.cc_bertadam_multi_f32(*args, _st(table)), "cc_bertadam_multi_f32")

    @torch.no_grad()
    def _scaled_step(self, scaler, max_norm):
        """DeviceGradScaler.step: the statistics over every gradient of the step (norm of the unscaled gradients, the
        multiplier inv_scale * global clip coefficient, found_inf), then the step on the *_scaled_f32 launches."""
        grads = []
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                L.require_device(p)
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                grads.append(p.grad)
        if not grads:
            return False
        raw, count, nblk = _grads_table(grads)
        table = self._table(("grads", len(raw)), raw, grads[0].device, _capturing())
        self._step(scaler._stats(table, count, nblk, max_norm, grads[0].device))
        return True

    def refresh_lr(self):
        """capturable: write every group's scheduled learning rate (from the host-side step counts) into its device float -
        call before replaying a captured step."""
        for gi, group in enumerate(self.param_groups):
            steps = [self.state[p]['step'] for p in group['params'] if p in self.state and len(self.state[p])]
            if steps and self._lr_dev.get(gi) is not None:
                self._lr_dev[gi].fill_(float(self._lr(group, steps[0])))

    def advance(self):
        """capturable: count one replayed step for every parameter that has state."""
        for group in self.param_groups:
            for p in group['params']:
                if p in self.state and len(self.state[p]):
                    self.state[p]['step'] += 1


# ================================================================================================ AdamW
class AdamW(_Optimizer):
    """torch.optim.AdamW (the optimizer main.py:168-175 builds for --optim AdamW): same constructor and validation, same state
    names ('step', 'exp_avg', 'exp_avg_sq': a state_dict loads into torch.optim.AdamW and back), the reference's extra group
    keys ('lr_mult', 'decay_mult', written by lr_scheduler) pass through.  A step is ONE cc_adamw_multi_f32 launch over every
    tensor with a gradient; the per-(group, step count) scalars (1 - lr wd, lr / (1 - b1^t), sqrt(1 - b2^t), ...) are host
    arithmetic in double, as torch computes them, and reach the kernel through a small device array.

    capturable=True: the record table and the scalars are staged so that a step captured into a hipGraph can be replayed -
    refresh_lr() before a replay writes the scalars for the groups' current lr / weight_decay and the next step count,
    advance() after it counts the step (the protocol of BertAdam, used by GraphedTrainStep)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 capturable=False):
        if amsgrad:
            raise ValueError("AdamW (HIP): amsgrad=True is not supported (the reference trains without it)")
        if maximize:
            raise ValueError("AdamW (HIP): maximize=True is not supported (the reference trains without it)")
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False),
                         capturable)
        self._scal_dev = None                  # the per-(group, step count) scalars of the step: a device float array
        self._cap = None                       # of the captured step: its classes' (group, parameter) and its parameters

    _moment_keys = ('exp_avg', 'exp_avg_sq')

    def _pinned(self):
        return self._cap['params'] if self._cap is not None else ()

    @staticmethod
    def _scalars(group, t):
        """cc_adamw_scalars of a group at step count t (after the step), in torch's double arithmetic."""
        b1, b2 = (float(b) for b in group['betas'])
        lr, wd = float(group['lr']), float(group['weight_decay'])
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        return (1 - lr * wd, b1, 1 - b1, b2, 1 - b2, lr / bc1, bc2 ** 0.5, float(group['eps']))

    def _upload_scalars(self, rows, device):
        arr = np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(-1)
        host = torch.from_numpy(arr).pin_memory()
        dev = self._scal_dev
        if dev is None or dev.numel() < arr.size or dev.device != device:
            if self._cap is not None:
                raise RuntimeError("AdamW: more (group, step count) classes than when the step was captured")
            dev = self._scal_dev = torch.zeros(max(arr.size, 8 * 16), dtype=torch.float32, device=device)
        dev[:arr.size].copy_(host, non_blocking=True)
        return dev

    def _prepare(self):
        """-> (device, table, count, total blocks, scalars) for the parameters that have a gradient; advances the step counts
        unless a capture is running."""
        capturing = _capturing()
        if capturing and not self.capturable:
            raise RuntimeError("AdamW: build it with capturable=True to capture its step")
        entries, classes, dev = [], {}, None
        for gi, group in enumerate(self.param_groups):
            if group.get('amsgrad') or group.get('maximize'):
                raise ValueError("AdamW (HIP): amsgrad / maximize are not supported")
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("AdamW (HIP): sparse gradients are not supported")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("AdamW (HIP): fp32 contiguous parameters (the master weights)")
                L.require_device(p)
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError("AdamW (HIP): all parameters on one device")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif torch.is_tensor(state['step']):
                    state['step'] = int(state['step'].item())
                t = state['step'] + 1
                ci = classes.setdefault((gi, t), (len(classes), p))[0]
                entries.append((p, p.grad, state['exp_avg'], state['exp_avg_sq'], ci))
                if not capturing:
                    state['step'] = t
        if not capturing:
            self._last = [e[0] for e in entries]                  # the parameters this step counts (for _uncount)
        if not entries:
            return None
        raw, count, nblk = _adamw_table(entries)
        table = self._table(len(raw), raw, dev, capturing)
        ordered = sorted(classes.items(), key=lambda kv: kv[1][0])
        if capturing:
            # what refresh_lr / advance need: per class its group and one of its parameters (whose step count is the class's)
            if self._scal_dev is None or self._scal_dev.numel() < 8 * len(ordered):
                raise RuntimeError("AdamW: run one eager step with the same parameters before capturing (scalars)")
            self._cap = dict(classes=[(gi, p) for (gi, _), (_, p) in ordered], params=[e[0] for e in entries])
            scal = self._scal_dev
        else:
            scal = self._upload_scalars([self._scalars(self.param_groups[gi], t) for (gi, t), _ in ordered], dev)
        return dev, table, count, nblk, scal

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        prep = self._prepare()
        if prep is not None:
            dev, table, count, nblk, scal = prep
            L.check(L.lib().cc_adamw_multi_f32(L.ptr(table), count, nblk, L.ptr(scal), None, _st(scal)), "cc_adamw_multi_f32")
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_norm):
        """clip_grad_norm_(the parameters with a gradient, max_norm) followed by step(), fused: the step launch multiplies each
        gradient by the device-side clip coefficient as it loads it and writes the clipped gradient back (one read-modify-write
        pass over the gradients less).  Bit for bit clip_grad_norm_ over the same parameters in group order + step().
        -> the total norm before clipping (0-d device tensor)."""
        prep = self._prepare()
        if prep is None:
            return torch.tensor(0.0)
        dev, table, count, nblk, scal = prep
        out = _clip_launches(table, count, nblk, max_norm, dev, coef_only=True)
        L.check(L.lib().cc_adamw_multi_f32(L.ptr(table), count, nblk, L.ptr(scal), L.ptr(out[1:]), _st(scal)),
                "cc_adamw_multi_f32")
        return out[0]

    @torch.no_grad()
    def _scaled_step(self, scaler, max_norm):
        """DeviceGradScaler.step: norm partials -> cc_grad_scaler_stats_f32 (norm of the unscaled gradients, the multiplier
        inv_scale * clip coefficient, found_inf) -> cc_adamw_multi_scaled_f32, which applies the multiplier as it loads each
        gradient and writes nothing when found_inf is set.  No pass unscales the gradients."""
        prep = self._prepare()
        if prep is None:
            return False
        dev, table, count, nblk, scal = prep
        mult, found = scaler._stats(table, count, nblk, max_norm, dev)
        L.check(L.lib().cc_adamw_multi_scaled_f32(L.ptr(table), count, nblk, L.ptr(scal), L.ptr(mult), L.ptr(found), _st(scal)),
                "cc_adamw_multi_scaled_f32")
        return True

    def refresh_lr(self):
        """capturable: write the captured step's scalars (each group's current lr / weight_decay, the next step count) into
        their device array - call before replaying a captured step."""
        if self._cap is None:
            return
        rows = [self._scalars(self.param_groups[gi], self.state[p]['step'] + 1) for gi, p in self._cap['classes']]
        self._upload_scalars(rows, self._scal_dev.device)

    def advance(self):
        """capturable: count one replayed step for every parameter the captured step updates."""
        for p in (self._cap['params'] if self._cap is not None else ()):
            self.state[p]['step'] += 1


class lr_scheduler:
    """The reference's per-iteration learning-rate scheduler (utils/lr_scheduler.py, main.py:171-174 with mode 'cos'), written
    to its interface: a linear slow start from slow_start_lr over slow_start_iters iterations, then
      cos   lr = init_lr / 2 (1 + cos(pi T / total))            poly  lr = init_lr (1 - T / total)^0.9
      HTD   lr = init_lr / 2 (1 - tanh(lower + (upper - lower) T / total))
      step  lr = init_lr multiplier^(epoch // lr_step), or ^(number of milestones passed)
    with T counted from the end of the slow start and total = all_iters - slow_start_iters, clamped below at end_lr.  A call
    writes lr * lr_mult and weight_decay * decay_mult into every parameter group.  Host arithmetic only."""

    def __init__(self, mode='cos', init_lr=0.1, all_iters=300, lr_milestones=None, lr_step=100, lr_step_multiplier=0.1,
                 slow_start_iters=0, slow_start_lr=1e-8, end_lr=1e-8, lower_bound=-6.0, upper_bound=3.0, weight_decay=1e-4,
                 iters_per_epoch=None):
        if mode not in ('cos', 'poly', 'HTD', 'step'):
            raise ValueError("lr_scheduler: mode must be one of 'cos', 'poly', 'HTD', 'step', got %r" % (mode,))
        self.mode, self.init_lr, self.now_lr, self.end_lr = mode, init_lr, init_lr, end_lr
        self.slow_start_iters, self.slow_start_lr = slow_start_iters, slow_start_lr
        self.total_iters = all_iters - slow_start_iters
        self.lr_step, self.lr_milestones, self.lr_step_multiplier = lr_step, lr_milestones, lr_step_multiplier
        self.lower_bound, self.upper_bound = lower_bound, upper_bound
        self.weight_decay = weight_decay
        self.iters_per_epoch = iters_per_epoch             # (only for calls without global_step)

    def lr_at(self, T, epoch=None):
        """The learning rate at iteration T (epoch: for mode 'step')."""
        if self.slow_start_iters > 0 and T <= self.slow_start_iters:
            lr = (1.0 * T / self.slow_start_iters) * (self.init_lr - self.slow_start_lr)
            lr = min(lr + self.slow_start_lr, self.init_lr)
        elif self.mode == 'cos':
            lr = 0.5 * self.init_lr * (1.0 + math.cos(1.0 * (T - self.slow_start_iters) / self.total_iters * math.pi))
        elif self.mode == 'poly':
            lr = self.init_lr * pow(1.0 - 1.0 * (T - self.slow_start_iters) / self.total_iters, 0.9)
        elif self.mode == 'HTD':
            ratio = 1.0 * (T - self.slow_start_iters) / self.total_iters
            lr = 0.5 * self.init_lr * (1.0 - math.tanh(self.lower_bound + (self.upper_bound - self.lower_bound) * ratio))
        elif self.lr_milestones is None:
            lr = self.init_lr * (self.lr_step_multiplier ** (epoch // self.lr_step))
        else:
            lr = self.init_lr * (self.lr_step_multiplier ** sum(1 for mile in self.lr_milestones if epoch >= mile))
        return max(lr, self.end_lr)

    def __call__(self, optimizer, i=None, epoch=None, global_step=None):
        T = (epoch * self.iters_per_epoch + i) if global_step is None else global_step
        lr = self.now_lr = self.lr_at(T, epoch)
        for group in optimizer.param_groups:
            group['lr'] = lr * group['lr_mult']
            group['weight_decay'] = self.weight_decay * group['decay_mult']


def prep_optim_params_groups(args, model, coef_lr=1.):
    """utils/optimization.py:173-222: CLIP parameters at lr * coef_lr, newly added modules at lr, no weight decay for biases /
    LayerNorm.  BertAdam (the default): 'lr' / 'weight_decay' per group; args.optim == 'AdamW': every group at args.lr with
    the 'lr_mult' / 'decay_mult' keys that lr_scheduler applies."""
    model = getattr(model, 'module', model)
    named = list(model.named_parameters())
    no_decay = ['bias', 'LayerNorm.bias', 'LayerNorm.weight']
    no_clip = args.new_added_modules
    dec = [(n, p) for n, p in named if not any(nd in n for nd in no_decay)]
    nodec = [(n, p) for n, p in named if any(nd in n for nd in no_decay)]
    is_clip = lambda n: "clip." in n and not any(nd in n for nd in no_clip)
    if getattr(args, 'optim', 'BertAdam') == 'AdamW':
        return [{'params': [p for n, p in dec if is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr, 'lr_mult': coef_lr,
                 'decay_mult': 1},
                {'params': [p for n, p in nodec if is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr, 'lr_mult': coef_lr,
                 'decay_mult': 0.0},
                {'params': [p for n, p in dec if not is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr, 'lr_mult': 1.0,
                 'decay_mult': 1.0},
                {'params': [p for n, p in nodec if not is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr, 'lr_mult': 1.0,
                 'decay_mult': 0.0}]
    return [{'params': [p for n, p in dec if is_clip(n)], 'weight_decay': args.wd, 'lr': args.lr * coef_lr},
            {'params': [p for n, p in nodec if is_clip(n)], 'weight_decay': 0.0, 'lr': args.lr * coef_lr},
            {'params': [p for n, p in dec if not is_clip(n)], 'weight_decay': args.wd},
            {'params': [p for n, p in nodec if not is_clip(n)], 'weight_decay': 0.0}]
