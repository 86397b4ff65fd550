"""linear_patch='3d' in training, without a GPU: the reference fixture (tools/gen_golden_3d.py) against the model's parameter
names, which parameter gets no gradient, the argument errors of the training tower on CPU tensors, the library entry's NULL
checks and the example's --linear_patch."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import train3d_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T", [3, 1])
def test_fixture_names_are_the_models(T):
    g = fx.load(T)
    E, RES, P, VW, VL, CTX, VOCAB, TW, TH, TL, B, T_ = (int(v) for v in g["cfg"])
    assert (RES, P, VW, T_) == (32, 8, 64, T) and g["video"].shape == (B * T, 3, RES, RES)
    model = fx.model(T)
    named = dict(model.clip.named_parameters())
    grads = fx.gradients(g)
    assert set(grads) | fx.no_grad_names(g) == set(named) and not set(grads) & fx.no_grad_names(g)
    for n, v in grads.items():
        assert tuple(v.shape) == tuple(named[n].shape) and v.dtype == torch.float64 and bool(torch.isfinite(v).all()), n
    assert named["visual.conv2.weight"].shape == (VW, 3, 3, P, P)
    assert g["loss"].dtype == np.float64 and g["vfeat"].shape == (B * T, E) and g["tfeat"].shape == (B, E)
    sd = fx.state_dict()
    for n, p in named.items():
        assert torch.equal(p.detach(), sd[n].float()), n


@pytest.mark.parametrize("T", [3, 1])
def test_conv1_is_the_only_parameter_without_a_gradient(T):
    g = fx.load(T)
    assert fx.no_grad_names(g) == {"visual.conv1.weight"}
    grads = fx.gradients(g)
    assert float(grads["visual.conv2.weight"].abs().max()) > 0
    if T == 1:      # both temporal neighbours are padding: only the centre tap of conv2 sees data
        w = grads["visual.conv2.weight"]
        assert float(w[:, :, 0].abs().max()) == 0 and float(w[:, :, 2].abs().max()) == 0 and float(w[:, :, 1].abs().max()) > 0


def test_freeze_rule_keeps_every_parameter_trainable():
    model = fx.model(3)
    model.freeze_cip_layers(0)
    assert all(p.requires_grad for p in model.parameters())
    from centerclip_amd.train import towers
    assert towers.visual_prefix_blocks(model.clip.visual) is None


def test_argument_errors_need_no_device():
    from centerclip_amd.train import encode_image_train
    model = fx.model(3)
    video = torch.zeros(6, 3, 32, 32)
    for bad in (4, 5, 0, -1, None):
        with pytest.raises(ValueError, match="video_frame"):
            encode_image_train(model.clip, video, bad)
    with pytest.raises(ValueError, match="video_frame"):
        encode_image_train(model.clip, torch.zeros(6, 32, 32, 3, dtype=torch.uint8), 4)
    # a shift module: video_frame must be the module's original_frame, the rule of the inference path
    shift = fx.model(3, cluster_inter=1, cluster_algo='token_shift', target_frames_blocks=[2, 2], cluster_num_blocks=[15, 14])
    assert shift.clip.visual.shift_segment() == 3
    with pytest.raises(NotImplementedError, match="original_frame"):
        encode_image_train(shift.clip, video, 2)
    # good arguments on a CPU tensor stop at the device check: there is no CPU implementation
    with pytest.raises(RuntimeError):
        encode_image_train(model.clip, video, 3)


def test_library_entry_rejects_null_before_touching_the_device():
    from centerclip_amd import _lib as L
    from centerclip_amd._lib_clip import Frames
    lib = L.lib()
    assert lib.cc_patch_gather3d_f16(None, 6, 3, 32, 8, None, None) == -1
    fr = Frames()
    assert lib.cc_patch_gather3d_f16(ctypes.byref(fr), 6, 3, 32, 8, None, None) == -1      # no frames, no output


def test_op_is_registered_with_a_fake_kernel_and_no_cpu_implementation():
    import centerclip_amd.torch_ops  # noqa: F401
    op = torch.ops.centerclip.patch_gather3d
    assert [a.name for a in op.default._schema.arguments] == ["frames", "T", "resolution", "patch"]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = op(torch.empty(6, 3, 32, 32), 3, 32, 8)
    assert tuple(out.shape) == (6 * 16, 9 * 64) and out.dtype == torch.float16
    with pytest.raises(NotImplementedError):
        op(torch.zeros(6, 3, 32, 32), 3, 32, 8)


def test_example_parses_linear_patch():
    spec = importlib.util.spec_from_file_location("train_synthetic_example", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).linear_patch == "2d"
    assert ap.parse_args(["--linear_patch", "3d", "--uint8", "1", "--precision", "amp"]).linear_patch == "3d"
    with pytest.raises(SystemExit):
        ap.parse_args(["--linear_patch", "4d"])
