"""Checkpoints: what the reference writes after every epoch (main.py:262-272, utils/misc.py:14-27) and reads back with
``--resume`` (main.py:185-212), for the eager loop and for a captured ``GraphedTrainStep``.

The file is the reference's dictionary - 'epoch', 'global_step', 'arch', 'state_dict', 'best_acc1', 'optimizer', and 'scaler'
under precision=amp - of CPU tensors and plain Python values, so ``torch.load(path, weights_only=True)`` reads it and either
code base reads the other's files.

Restoring is in place wherever the destination exists: parameters by ``copy_`` (which bumps the version counters, so the cached
fp16 / folded copies refresh), moments through ``_Optimizer.load_state_dict``, the scaler's device words through
``DeviceGradScaler.load_state_dict``.  A captured step replays a graph that holds those addresses; a tensor swapped for a
new one would be ignored by every replay, silently.  Everything is checked before the first write.
"""
import os
import shutil

import torch

from .scaler import DeviceGradScaler

ARCH = 'CLIp4Clip'                             # (the reference's spelling, main.py:266)


def _plain(value):
    """Tensors -> detached CPU clones, containers -> dicts / lists of them, numbers and strings as they are."""
    if torch.is_tensor(value):
        return value.detach().to('cpu', copy=True)
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    raise TypeError("checkpoint_dict: a %s cannot be written for torch.load(weights_only=True)" % type(value).__name__)


def checkpoint_dict(model, optimizer, epoch, global_step, best_acc1=0.0, scaler=None, step=None):
    """The dictionary main.py:263-271 saves.  ``step``: a GraphedTrainStep - its last call's step count is settled first
    (sync()), and global_step and the scaler are the step's own; a plain DeviceGradScaler is settled the same way, because
    under it the count of step k is known only once step k has run.  Tensors are detached CPU clones: a later step cannot
    change a dictionary that has been built.  A DeviceGradScaler's entry also carries its 'counters' (steps taken, skipped),
    which torch.amp.GradScaler.load_state_dict ignores."""
    if step is not None:
        step.sync()
        global_step, scaler = step.global_step, step.scaler
    elif isinstance(scaler, DeviceGradScaler):
        scaler.sync()
    model = getattr(model, 'module', model)
    d = {'epoch': int(epoch), 'global_step': int(global_step), 'arch': ARCH, 'state_dict': _plain(model.state_dict()),
         'best_acc1': float(best_acc1), 'optimizer': _plain(optimizer.state_dict())}
    if scaler is not None and scaler.is_enabled():
        d['scaler'] = _plain(scaler.state_dict())
        if isinstance(scaler, DeviceGradScaler):
            d['scaler']['counters'] = list(scaler.counters())
    return d


def save_checkpoint(state, is_best, model_dir, filename='checkpoint.pth.tar'):
    """utils/misc.py:14-18: write ``state`` to model_dir/filename; is_best: also a copy named *.best.pth.tar."""
    path = os.path.join(model_dir, filename)
    torch.save(state, path)
    if is_best:
        shutil.copyfile(path, path.replace('pth.tar', 'best.pth.tar'))


def save_model(epoch, args, model, type_name=""):
    """utils/misc.py:21-27: the weights alone as args.output_dir/pytorch_model.bin.{type_name.}{epoch} -> that path."""
    model = getattr(model, 'module', model)
    path = os.path.join(args.output_dir, "pytorch_model.bin.%s%s" % (type_name + "." if type_name else "", epoch))
    torch.save(_plain(model.state_dict()), path)
    return path


def _check_model(model, sd, fixed):
    """Strict: the same names, the same shapes; ``fixed`` (names that may not be written): the same values.  ValueError."""
    own = model.state_dict(keep_vars=True)
    missing, unexpected = [k for k in own if k not in sd], [k for k in sd if k not in own]
    if missing or unexpected:
        raise ValueError("resume: the checkpoint's state_dict does not fit the model (missing %s, unexpected %s)"
                         % (missing[:4], unexpected[:4]))
    for k, dst in own.items():
        if not torch.is_tensor(sd[k]) or sd[k].shape != dst.shape:
            raise ValueError("resume: %s is %s in the checkpoint, %s in the model"
                             % (k, tuple(getattr(sd[k], 'shape', ())), tuple(dst.shape)))
    for k in fixed:
        if not torch.equal(own[k].detach(), sd[k].to(device=own[k].device, dtype=own[k].dtype)):
            raise ValueError("resume: %s is frozen inside the captured step (the graph holds its packed copy) and differs in "
                             "the checkpoint" % k)
    return own


def restore(d, model, optimizer=None, scaler=None, load_from_pretrained=False, captured=False):
    """A loaded checkpoint dictionary into model / optimizer / scaler -> (start_epoch, global_step, best_acc1); what resume()
    and GraphedTrainStep.load_state_dict share.  Checked first, then written: a dictionary that does not fit raises
    ValueError or RuntimeError and leaves all three as they were.  ``captured``: a graph holds the model's addresses - a frozen
    parameter (whose packed copy the graph reads) is not written and must already hold the checkpoint's value."""
    model = getattr(model, 'module', model)
    sd = d['state_dict']
    if any(k.startswith('module.') for k in sd):               # (saved from a DistributedDataParallel wrapper, main.py:198-199)
        sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    params = dict(model.named_parameters())
    fixed = [k for k, p in params.items() if captured and not p.requires_grad]
    own = _check_model(model, sd, fixed)
    full = not load_from_pretrained
    opt_sd = d.get('optimizer') if full and optimizer is not None else None
    sc_sd = d.get('scaler') if full and scaler is not None and scaler.is_enabled() else None
    if opt_sd is not None:
        if isinstance(scaler, DeviceGradScaler):
            scaler.sync()                                        # (a pending count belongs to the state about to be replaced)
        check = getattr(optimizer, '_check_state_dict', None)
        if check is not None:
            check(opt_sd)
    if sc_sd is not None:
        missing = [k for k in ("scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker") if k not in sc_sd]
        if missing:
            raise ValueError("resume: the checkpoint's scaler state has no %s" % missing)
    with torch.no_grad():
        for k, dst in own.items():
            if k not in fixed:
                dst.copy_(sd[k])
    if not full:
        return 0, 0, 0.0
    if opt_sd is not None:
        optimizer.load_state_dict(opt_sd)
    if sc_sd is not None:
        scaler.load_state_dict(sc_sd)
    return int(d['epoch']), int(d['global_step']), float(d.get('best_acc1', 0.0))


def resume(path, model, optimizer=None, scaler=None, step=None, load_from_pretrained=False, map_location='cpu'):
    """main.py:188-212: the checkpoint at ``path`` into model, optimizer and scaler -> (start_epoch, global_step, best_acc1).
    A missing file raises FileNotFoundError: the reference only logs it and trains from scratch, which loses a run without
    a word.  A 'module.' prefix on the weights' names is stripped; the weights load strictly; load_from_pretrained: the
    weights alone, -> (0, 0, 0.0), optimizer and scaler untouched.  Otherwise optimizer and scaler state are restored where
    both the key and the object exist.  ``step``: a GraphedTrainStep - its load_state_dict restores its own model, optimizer
    and scaler (in place once it has captured) and takes over global_step."""
    if not os.path.isfile(path):
        raise FileNotFoundError("resume: no checkpoint found at %r" % (path,))
    d = torch.load(path, map_location=map_location, weights_only=True)
    if step is not None:
        return step.load_state_dict(d, load_from_pretrained=load_from_pretrained)
    return restore(d, model, optimizer, scaler, load_from_pretrained)
