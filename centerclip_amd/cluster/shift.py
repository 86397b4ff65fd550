"""Mirror of modules/cluster/shift.py (temporal_shift_wo_cls, token_shift) and of the shift branch of TokenClusterInter
(cluster.py:343-350) as a module of its own, ``TokenShiftInter``: get_cluster_inter returns it for cluster_algo
'temporal_shift' / 'token_shift'.  A fixed 0/1 map over the frames of each segment of original_frame consecutive frames
(torch.ops.centerclip.token_shift, cc_token_shift_f32), differentiable in x through its adjoint (the same kernel with
adjoint=1).  No parameters: checkpoints of models trained with a shift algorithm load as they do in the reference."""
import torch

from .. import _lib as L
from .. import torch_ops

SHIFT_ALGORITHMS = ('temporal_shift', 'token_shift')


class _Shift(torch.autograd.Function):
    """temporal_shift_wo_cls / token_shift of x: a fixed 0/1 map, so the backward is its transpose (the opposite shift with
    zero fill)."""

    @staticmethod
    def forward(ctx, x, frame_major, segment, fold_div, mode):
        ctx.cfg = (frame_major, segment, fold_div, mode)
        return torch.ops.centerclip.token_shift(x, frame_major, segment, fold_div, mode, False)

    @staticmethod
    def backward(ctx, g):
        frame_major, segment, fold_div, mode = ctx.cfg
        gx = torch.ops.centerclip.token_shift(g.contiguous().float(), frame_major, segment, fold_div, mode, True)
        return gx, None, None, None, None


def shift_tokens(x, algorithm, segment, fold_div=8, frame_major=False):
    """The shift of cluster_algo ``algorithm`` on x [L, F, W] (LND) or [F, L, W] (frame_major), differentiable in x."""
    L.require_device(x)
    if x.dtype != torch.float32:
        x = x.float()
    frames = x.shape[0 if frame_major else 1]
    if frames % segment:
        raise ValueError("%s: %d frames are not a multiple of original_frame %d" % (algorithm, frames, segment))
    return _Shift.apply(x.contiguous(), bool(frame_major), int(segment), int(fold_div), torch_ops.SHIFT_MODES[algorithm])


def temporal_shift_wo_cls(x, n_segment, fold_div=8):
    """shift.py:15-37: x [batch * n_segment, 1 + n, D] -> the patch tokens shifted, CLS rows copied."""
    return shift_tokens(x, 'temporal_shift', n_segment, fold_div, frame_major=True)


def token_shift(x, n_segment, fold_div=8):
    """shift.py:40-61: x [batch * n_segment, 1 + n, D] -> the CLS rows shifted, the patch tokens copied."""
    return shift_tokens(x, 'token_shift', n_segment, fold_div, frame_major=True)


class TokenShiftInter(torch.nn.Module):
    """TokenClusterInter of cluster_algo 'temporal_shift' / 'token_shift' (cluster.py:66-157,343-352): takes the constructor
    arguments get_cluster_inter passes to TokenClusterInter.  Frames and tokens are kept - cluster_num, after_block_frames and
    the clustering arguments are ignored, as in the reference; the frames are shifted within segments of original_frame
    consecutive frames of the batch, fold = W // shift_fold_div (8).  The block applies token_shift a second time between the
    attention residual and ln_2 (clip.py:246-248); forward returns (x', None) in LND."""

    is_shift = True
    is_default_variant = False

    def __init__(self, algorithm='token_shift', block_id=1, before_cluster_num=49, cluster_num=49, before_block_frames=12,
                 after_block_frames=12, original_frame=12, mean_residual=False, **_ignored):
        super().__init__()
        if algorithm not in SHIFT_ALGORITHMS:
            raise ValueError("TokenShiftInter: cluster_algo %r is not a shift (TokenClusterInter builds it)" % (algorithm,))
        if mean_residual:
            raise NotImplementedError("mean_residual with cluster_algo %r (not reachable from the reference's arguments)"
                                      % algorithm)
        self.algorithm = algorithm
        self.block_id = block_id
        self.original_frame = original_frame
        self.before_cluster_num, self.cluster_num = before_cluster_num, cluster_num
        self.before_block_frames, self.after_block_frames = before_block_frames, after_block_frames
        self.shift_fold_div = 8                                                   # cluster.py:157
        self.mean_residual = False
        self.last_medoids = None

    def forward(self, x):
        """x [1+n, B*T, W] (LND) -> (S(x) [1+n, B*T, W], None)   (cluster.py:343-352)"""
        return shift_tokens(x, self.algorithm, self.original_frame, self.shift_fold_div), None

    def cluster_frame_major(self, x_nld, keep_ids=False):
        """The same shift on frame-major activations [B*T, 1+n, W]."""
        return shift_tokens(x_nld, self.algorithm, self.original_frame, self.shift_fold_div, frame_major=True)

    def variant(self, N, device):
        """-> (cc_cluster_variant of this module for the fused encoders, tensors it points to (none))."""
        var = L.ClusterVariant()
        var.algorithm = torch_ops.SHIFT_MODES[self.algorithm]
        var.shift_fold_div, var.shift_segment = int(self.shift_fold_div), int(self.original_frame)
        return var, []
