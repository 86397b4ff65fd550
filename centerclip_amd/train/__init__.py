"""Training on the HIP library: what the reference's main.py:98-170 and :291-378 drive, in six modules.

    block    one ResidualAttentionBlock's forward with saved activations and its backward, inside torch.autograd
    towers   the visual and text towers and the seqTransf head with gradients, and their frozen prefix
    optim    BertAdam, AdamW, global gradient clipping, the schedules, the parameter groups
    scaler   DeviceGradScaler: GradScaler's recipe decided on the device
    loop     train_epoch and GraphedTrainStep (the step captured into a hipGraph)
    checkpoint   checkpoint_dict, save_checkpoint, save_model, resume: the reference's checkpoint file, restored in place

CLIP4Clip.forward in training mode runs on the towers, so a training step reaches every parameter; master weights are fp32,
the matrix cores get fp16 operands with fp32 accumulation.  linear_patch='3d' trains conv2 on the 3-d patch gather (conv1 takes
no part and gets no gradient, as in the reference).  Not built: training with mean_residual, and gradient accumulation inside the
captured step.
"""
from .block import (LayerNormFunction, LinearFunction, ResidualAttentionBlockFunction, _PARAM_ORDER, _cast_scaled,  # noqa: F401
                    _cast_transpose, _column_sums, _grad_linear, _layernorm, _linear_resid, _linear_unscaled, _ln_backward,
                    _pad64, _token_shift_rows, _unscale, _w16_pair, _wgrad_tn, _wt16, block_apply, block_backward,
                    block_forward_train)
from .towers import (encode_image_train, encode_text_train, seq_head_train, text_prefix_blocks,                 # noqa: F401
                     visual_prefix_blocks)
from .optim import (SCHEDULES, AdamW, BertAdam, _adamw_table, _clip_launches, _Staged, clip_grad_norm_, lr_scheduler,  # noqa: F401
                    prep_optim_params_groups, warmup_constant, warmup_cosine, warmup_linear)
from .scaler import DeviceGradScaler, _device_scaler                                                          # noqa: F401
from .checkpoint import checkpoint_dict, resume, save_checkpoint, save_model                                 # noqa: F401
from .loop import GraphedTrainStep, train_epoch                                                               # noqa: F401
