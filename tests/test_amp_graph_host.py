"""CPU-only: the host side of train.DeviceGradScaler and GraphedTrainStep(scaler=...) - constructor validation, torch's
state-dict keys and a round trip in both directions, the refusals that need no GPU (non-capturable optimizer, CPU tensors:
there is no CPU fallback), a disabled scaler counting as none, and the new entry points declared where ctypes finds them."""
import pytest
import torch


def test_constructor_validation():
    from centerclip_amd.train import DeviceGradScaler
    for kw in (dict(init_scale=0.0), dict(init_scale=-1.0), dict(growth_factor=1.0), dict(growth_factor=0.5),
               dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(growth_interval=0), dict(growth_interval=2.5)):
        with pytest.raises(ValueError):
            DeviceGradScaler(**kw)
    sc = DeviceGradScaler()
    assert sc.is_enabled() and sc.get_scale() == 2.0 ** 16
    assert (sc.get_growth_factor(), sc.get_backoff_factor(), sc.get_growth_interval()) == (2.0, 0.5, 2000)
    off = DeviceGradScaler(growth_factor=0.5, enabled=False)            # (a disabled scaler validates nothing, as torch's)
    assert not off.is_enabled() and off.get_scale() == 1.0 and off.state_dict() == {}


def test_state_dict_has_torchs_keys_and_round_trips_both_ways():
    from centerclip_amd.train import DeviceGradScaler
    ours = DeviceGradScaler(init_scale=2.0 ** 9, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)
    # (the same class for every device; torch disables a 'cuda' one on a machine without a GPU, and its state is then empty)
    theirs = torch.amp.GradScaler('cpu', init_scale=2.0 ** 5, growth_factor=1.5, backoff_factor=0.75, growth_interval=11)
    assert sorted(ours.state_dict()) == sorted(theirs.state_dict())
    sd_theirs = dict(theirs.state_dict())
    theirs.load_state_dict(ours.state_dict())                           # ours -> torch
    assert theirs.state_dict() == ours.state_dict()
    assert theirs.get_growth_factor() == 3.0 and theirs.get_backoff_factor() == 0.25 and theirs.get_growth_interval() == 7
    fresh = DeviceGradScaler()
    sd_theirs["_growth_tracker"] = 5
    fresh.load_state_dict(sd_theirs)                                    # torch -> ours
    assert fresh.state_dict() == sd_theirs and fresh.get_scale() == 2.0 ** 5
    with pytest.raises(RuntimeError):
        fresh.load_state_dict({})                                       # (saved from a disabled scaler)


def _tiny():
    model = torch.nn.Linear(4, 4)
    return model


def test_graphed_step_refuses_a_non_capturable_optimizer_and_foreign_scalers():
    from centerclip_amd.train import AdamW, BertAdam, DeviceGradScaler, GraphedTrainStep
    m = _tiny()
    for opt in (AdamW(m.parameters(), lr=1e-3), BertAdam(m.parameters(), lr=1e-3)):
        with pytest.raises(ValueError):
            GraphedTrainStep(m, opt, scaler=DeviceGradScaler())
    with pytest.raises(TypeError):
        GraphedTrainStep(m, AdamW(m.parameters(), lr=1e-3, capturable=True), scaler=object())
    with pytest.raises(NotImplementedError):                            # (accumulation stays out of the captured step)
        GraphedTrainStep(m, AdamW(m.parameters(), lr=1e-3, capturable=True), gradient_accumulation_steps=2, scaler=DeviceGradScaler())


def test_disabled_scaler_is_no_scaler():
    from centerclip_amd.train import AdamW, DeviceGradScaler, GraphedTrainStep
    m = _tiny()
    opt = AdamW(m.parameters(), lr=1e-3, capturable=True)
    assert GraphedTrainStep(m, opt, scaler=None).scaler is None
    assert GraphedTrainStep(m, opt, scaler=DeviceGradScaler(enabled=False)).scaler is None
    assert GraphedTrainStep(m, opt, scaler=torch.amp.GradScaler('cuda', enabled=False)).scaler is None
    step = GraphedTrainStep(m, opt, scaler=DeviceGradScaler(init_scale=4.0))
    assert step.scaler is not None and step.scaler.get_scale() == 4.0 and step.write_back_scaler() is None
    step.sync()                                                         # (nothing pending: no device needed)
    # a disabled scaler passes everything through
    off = DeviceGradScaler(enabled=False)
    x = torch.ones(3)
    assert off.scale(x) is x
    off.unscale_(opt)
    off.update()


def test_cpu_tensors_and_foreign_optimizers_raise():
    from centerclip_amd.train import AdamW, DeviceGradScaler
    sc = DeviceGradScaler()
    with pytest.raises(RuntimeError):
        sc.scale(torch.ones(()))                                        # no CPU fallback
    m = _tiny()
    sgd = torch.optim.SGD(m.parameters(), lr=0.1)
    for call in (sc.unscale_, sc.step):
        with pytest.raises(TypeError):
            call(sgd)
    opt = AdamW(m.parameters(), lr=1e-3)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError):
        sc.step(opt)                                                    # CPU parameters
    with pytest.raises(RuntimeError):
        sc.update()                                                     # no inf check was recorded
    sc.unscale_(opt)
    with pytest.raises(RuntimeError):
        sc.unscale_(opt)                                                # twice since the last update(), as torch refuses it
    with pytest.raises(RuntimeError):
        DeviceGradScaler().clip_grad_norm_(opt, 1.0)                    # before unscale_


def test_new_entry_points_are_exported_and_declared_for_ctypes():
    from centerclip_amd import _lib as L
    lib = L.lib()
    for name, nargs in (("cc_grad_scaler_stats_f32", 6), ("cc_adamw_multi_scaled_f32", 7), ("cc_grad_scaler_update_f32", 7),
                        ("cc_bertadam_multi_scaled_f32", 13)):
        assert len(getattr(lib, name).argtypes) == nargs, name
    # NULL pointers are rejected before anything touches the device
    assert lib.cc_grad_scaler_stats_f32(None, 1, None, 1.0, None, None) == -1
    assert lib.cc_adamw_multi_scaled_f32(None, 1, 1, None, None, None, None) == -1
    assert lib.cc_grad_scaler_update_f32(None, None, None, 2.0, 0.5, 1, None) == -1
    assert lib.cc_bertadam_multi_f32(None, 1, 0, 1, 0.9, 0.999, 1e-6, 1.0, None, 0, None) == -1
