"""``DeviceGradScaler``: torch.amp.GradScaler's recipe (main.py:160, 320-328) with every decision on the device, so that the
same object drives the eager train_epoch and a captured GraphedTrainStep; ``_device_scaler`` turns GraphedTrainStep's
scaler argument into one.  The kernels are csrc/adamw.hip's cc_grad_scaler_*_f32 and the optimizers' *_scaled_f32 launches.
"""
import torch

from .. import _lib as L
from ..torch_ops import _st
from .optim import AdamW, BertAdam, _capturing, _norm_partials


class DeviceGradScaler:
    """torch.amp.GradScaler's recipe (main.py:160, 320-328: scale(loss).backward(), unscale_, clip, step, update) with every
    decision on the device, so that the same object runs eagerly in train_epoch and inside a captured GraphedTrainStep:

        scale(loss)            loss * scale (the device float; the HIP backward passes a power of two through exactly)
        unscale_(optimizer)    launches NOTHING: the gradients stay scaled in memory until step() - no pass over them exists
        clip_grad_norm_(optimizer, max_norm)   (after unscale_) asks step() for global clipping of the unscaled gradients
        step(optimizer)        the norm partials of every gradient -> cc_grad_scaler_stats_f32 (norm of the unscaled
                               gradients, ONE multiplier inv_scale * clip coefficient, found_inf) -> the optimizer's
                               *_scaled_f32 launches, which apply the multiplier as they load a gradient (and store that
                               value back) and write nothing at all when found_inf is set.  Only centerclip_amd.train.AdamW /
                               BertAdam have such launches: any other optimizer raises.
        update(new_scale=None) cc_grad_scaler_update_f32, GradScaler.update's rule (backoff on found_inf, growth after
                               growth_interval clean steps in a row), plus two device counters: steps taken / skipped.

    The state_dict has torch's keys (scale, growth_factor, backoff_factor, growth_interval, _growth_tracker): a checkpoint
    written from either class loads into the other.

    Step counts.  A skipped step must not advance the optimizer's state['step'] (bias correction, BertAdam's schedule), and
    whether a step was skipped is known on the device only.  Design: the flag is copied into a pinned host word right behind
    the optimizer launch (inside the graph when captured), and the count of step k is settled at the START of step k + 1 -
    sync() waits for step k's event and then either takes back the count an eager step() advanced, or lets a captured step's
    optimizer advance().  Nothing waits between enqueueing a step's work and its end.  The alternative - counts and the
    per-class scalars (1 - b1^t, the schedules) on the device - would have to restate torch's double-precision host arithmetic
    there, bit for bit, for both optimizers; the deferred count keeps that arithmetic where it is.  Call sync() (or
    GraphedTrainStep.sync()) before reading optimizer.state_dict()."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)
        if self._enabled:
            if not float(init_scale) > 0.0:
                raise ValueError("DeviceGradScaler: init_scale must be > 0, got %r" % (init_scale,))
            if not float(growth_factor) > 1.0:
                raise ValueError("DeviceGradScaler: the growth factor must be > 1.0, got %r" % (growth_factor,))
            if not 0.0 < float(backoff_factor) < 1.0:
                raise ValueError("DeviceGradScaler: the backoff factor must be in (0, 1), got %r" % (backoff_factor,))
            if int(growth_interval) != growth_interval or int(growth_interval) < 1:
                raise ValueError("DeviceGradScaler: growth_interval must be a positive integer, got %r" % (growth_interval,))
        self._init_scale, self._growth_factor = float(init_scale), float(growth_factor)
        self._backoff_factor, self._growth_interval = float(backoff_factor), int(growth_interval)
        self._init_growth_tracker, self._init_counters = 0, (0, 0)
        self._f = None            # device float32 [8]: scale, 1 / scale, norm, multiplier, found_inf
        self._c = None            # device int32 [4]: growth tracker, steps taken, steps skipped
        self._pin = self._event = self._pending = None
        self._unscaled, self._max_norm, self._stepped = set(), {}, False

    # ------------------------------------------------------------------------------------------------ state
    def _ensure(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.CenterClipHipError("DeviceGradScaler runs on MI355X only: got a %s tensor (no CPU fallback)" % device)
        if self._f is None:
            self._f = torch.zeros(8, dtype=torch.float32, device=device)
            self._c = torch.zeros(4, dtype=torch.int32, device=device)
            self._pin = torch.zeros(1, dtype=torch.float32).pin_memory()
            self._event = torch.cuda.Event()
            self._set_scale(self._init_scale)
            self._c[0] = self._init_growth_tracker
            self._c[1], self._c[2] = self._init_counters
        elif self._f.device != device:
            raise RuntimeError("DeviceGradScaler: one device per scaler (%s, then %s)" % (self._f.device, device))

    def _set_scale(self, value):
        if torch.is_tensor(value):
            if value.numel() != 1 or value.requires_grad:
                raise ValueError("DeviceGradScaler.update: new_scale must be a float or a 1-element tensor without a gradient")
            self._f[0:1].copy_(value.detach().reshape(1).to(torch.float32))
        else:
            self._f[0:1].fill_(float(value))
        self._f[1:2].copy_(self._f[0:1].double().reciprocal().float())        # as GradScaler._unscale_grads_ computes it

    def is_enabled(self):
        return self._enabled

    def get_scale(self):
        if not self._enabled:
            return 1.0
        return self._init_scale if self._f is None else float(self._f[0])

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def counters(self):
        """-> (steps taken, steps skipped) as update() has counted them on the device (reads the device: synchronises)."""
        if self._c is None:
            return self._init_counters
        c = self._c.tolist()
        return int(c[1]), int(c[2])

    def state_dict(self):
        if not self._enabled:
            return {}
        tracker = self._init_growth_tracker if self._c is None else int(self._c[0])
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        """In place once the device words exist (a captured step holds their addresses).  'counters' - (steps taken, steps
        skipped), which train.checkpoint_dict adds to torch's keys - continues counters(); without it they stay as they are."""
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of "
                               "GradScaler.")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if "counters" in state_dict:
            self._init_counters = tuple(int(c) for c in state_dict["counters"])
        if self._f is not None:
            self._set_scale(self._init_scale)
            self._c[0:1].fill_(self._init_growth_tracker)
            if "counters" in state_dict:
                self._c[1:2].fill_(self._init_counters[0])
                self._c[2:3].fill_(self._init_counters[1])

    def _snapshot(self):
        return self._f.clone(), self._c.clone()

    def _restore(self, snap):
        self._f.copy_(snap[0])
        self._c.copy_(snap[1])
        self._pending, self._stepped = None, False
        self._unscaled.clear()
        self._max_norm.clear()

    # ------------------------------------------------------------------------------------------------ the protocol
    def scale(self, outputs):
        if not self._enabled:
            return outputs
        if not torch.is_tensor(outputs):
            return type(outputs)(self.scale(o) for o in outputs)
        self._ensure(outputs.device)
        return outputs * self._f[0]

    @staticmethod
    def _ours(optimizer, what):
        if not isinstance(optimizer, (AdamW, BertAdam)):
            raise TypeError("DeviceGradScaler.%s: centerclip_amd.train.AdamW or BertAdam (the optimizers with launches that can "
                            "be skipped on the device), got %s" % (what, type(optimizer).__name__))

    def unscale_(self, optimizer):
        """Marks the optimizer's gradients as to be read unscaled; launches nothing - step() applies inv_scale together with
        the clip coefficient, so p.grad still holds the SCALED values until then (and the unscaled, clipped ones after)."""
        if not self._enabled:
            return
        self._ours(optimizer, "unscale_")
        if id(optimizer) in self._unscaled:
            raise RuntimeError("unscale_() has already been called on this optimizer since the last update().")
        self._unscaled.add(id(optimizer))

    def clip_grad_norm_(self, optimizer, max_norm):
        """torch.nn.utils.clip_grad_norm_ over the optimizer's parameters, on the UNSCALED gradients (call unscale_ first,
        main.py:324-326): deferred into step(), where it costs no launch of its own."""
        if not self._enabled:
            return
        self._ours(optimizer, "clip_grad_norm_")
        if id(optimizer) not in self._unscaled:
            raise RuntimeError("DeviceGradScaler.clip_grad_norm_: call unscale_(optimizer) first")
        if not float(max_norm) >= 0.0:
            raise ValueError("DeviceGradScaler.clip_grad_norm_: max_norm must be >= 0")
        self._max_norm[id(optimizer)] = float(max_norm)

    def _stats(self, table, count, nblk, max_norm, device):
        """-> (multiplier, found_inf): 1-element views of the device state, written by cc_grad_scaler_stats_f32."""
        self._ensure(device)
        st = _st(self._f)
        ws = _norm_partials(table, count, nblk, self._f.device, st)
        L.check(L.lib().cc_grad_scaler_stats_f32(L.ptr(ws), nblk, L.ptr(self._f[1:2]), float(max_norm), L.ptr(self._f[2:5]), st),
                "cc_grad_scaler_stats_f32")
        return self._f[3:4], self._f[4:5]

    def grad_norm(self):
        """The norm of the unscaled gradients the last step() measured (0-d device tensor)."""
        return self._f[2]

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        self._ours(optimizer, "step")
        if "closure" in kwargs or args:
            raise RuntimeError("Closure use is not currently supported if GradScaler is enabled.")
        capturing = _capturing()
        if not capturing:
            self.sync()                                           # the previous step's count, before this one's host arithmetic
        max_norm = self._max_norm.pop(id(optimizer), -1.0)
        ran = optimizer._scaled_step(self, max_norm)
        if not ran:                                               # (no gradient anywhere: nothing to skip)
            for p in (p for g in optimizer.param_groups for p in g['params']):
                self._ensure(p.device)
                break
            if self._f is None:
                raise RuntimeError("DeviceGradScaler.step: the optimizer has no parameters")
            self._f[4:5].zero_()
        self._pin.copy_(self._f[4:5], non_blocking=True)          # (captured: a copy node of the graph)
        if not capturing and ran:
            self._mark(optimizer, "eager")
        self._stepped = True
        return None

    def _mark(self, optimizer, mode):
        self._event.record()
        self._pending = (optimizer, mode)

    def sync(self):
        """Settle the last step's count (see the class docstring): waits for that step, no-op when nothing is pending."""
        if self._pending is None:
            return
        optimizer, mode = self._pending
        self._pending = None
        self._event.synchronize()
        skipped = float(self._pin[0]) != 0.0
        if mode == "eager" and skipped:
            optimizer._uncount()
        elif mode == "graph" and not skipped:
            optimizer.advance()

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            if _capturing():
                raise RuntimeError("DeviceGradScaler.update(new_scale=...) inside a capture")
            if self._f is None:
                if torch.is_tensor(new_scale):
                    self._ensure(new_scale.device)
                    self._set_scale(new_scale)
                else:
                    self._init_scale = float(new_scale)
            else:
                self._set_scale(new_scale)
        else:
            if not self._stepped:
                raise RuntimeError("No inf checks were recorded prior to update.")
            L.check(L.lib().cc_grad_scaler_update_f32(L.ptr(self._f[0:2]), L.ptr(self._f[4:5]), L.ptr(self._c),
                                                      self._growth_factor, self._backoff_factor, self._growth_interval,
                                                      _st(self._f)), "cc_grad_scaler_update_f32")
        self._stepped = False
        self._unscaled.clear()
        self._max_norm.clear()


def _device_scaler(scaler):
    """GraphedTrainStep's scaler argument -> (DeviceGradScaler or None, the torch GradScaler it was copied from or None)."""
    if scaler is None:
        return None, None
    if isinstance(scaler, DeviceGradScaler):
        return (scaler if scaler.is_enabled() else None), None
    if isinstance(scaler, torch.amp.GradScaler):
        if not scaler.is_enabled():
            return None, None
        dev = DeviceGradScaler()
        dev.load_state_dict(scaler.state_dict())
        return dev, scaler
    raise TypeError("GraphedTrainStep: scaler must be a DeviceGradScaler or a torch.amp.GradScaler, got %s" % type(scaler).__name__)
