"""The depth pre-training loss of VEON's first training stage
(``VeonDepthPretrain.forward_train``, mmdet3d/models/detectors/veon_depth_pretrain.py:
128-154): block-min ``downsample_depth`` of the predicted metric depth (by 8) and of the
LiDAR depth (by 16), the mean-absolute-error statistic and
``LSSViewTransformerRaw.get_depth_loss_own(zoe=True, ce=True)``
(mmdet3d/models/necks/view_transformer_raw.py:497-535): the scale-invariant log term and
the two-hot binary cross-entropy.

The reference selects rows with two boolean masks, reads ``.item()`` and divides by
``max(1.0, fg_mask.sum())``: four host synchronisations per step, so it cannot sit in a
captured graph.  On a ROCm device ``depth_pretrain_loss`` is native in both directions
(csrc/depth_loss.hip: three kernels, nothing read back, nothing of size rows x (D+1) in
memory); ``depth_pretrain_loss_torch`` is the reference's op sequence in torch at any
dtype: the CPU path and the tests' yardstick."""
import torch
import torch.nn.functional as F

from . import _lib
from .depth_ops import downsample_depth_torch

REC = 8                    # VEON_DEPTH_LOSS_REC of include/veon_hip.h
VALID_BELOW = 9225
SCALES = (1, 2, 4, 8, 16)


# ------------------------------------------------------------------ torch mirror
def bin_centers(D, lo, step, device=None):
    """The D+1 bin centres as the reference forms them (:417-418): fp32."""
    return torch.arange(D + 1, device=device) * step + (lo + step / 2)


def one_hot_depth_torch(depths, D, lo, step):
    """``get_one_hot_depth`` (:431-456) on a (B,N,H,W) map -> (B*N*H*W, D) rows."""
    d = depths.clamp_max(500).reshape(-1, 1)
    gap = -torch.abs(d - bin_centers(D, lo, step, depths.device)[None, :])
    index = gap.max(-1, keepdim=True)[1]
    return torch.zeros_like(gap).scatter_(-1, index, 1.0)[:, :-1]


def two_hot_depth_torch(depths, D, lo, step, gamma=4):
    """``get_two_hot_depth`` (:406-429) with its straight-through clamp, differentiable,
    on a (B,N,H,W) map -> (B*N*H*W, D) rows."""
    d = depths.reshape(-1, 1)
    gap = -torch.abs(d - bin_centers(D, lo, step, depths.device)[None, :]) * gamma
    min_gap = -16
    gap = torch.where(gap >= min_gap, gap, gap + (min_gap - gap.detach()))
    return torch.softmax(gap, dim=-1)[:, :-1]


def depth_loss_own_torch(depth_labels, depth_preds, D, lo, step, gamma=4, zoe=True, ce=True):
    """``get_depth_loss_own`` (:497-535) on already-downsampled (B,N,h,w) maps, op for
    op (boolean-mask selections and ``max(1.0, fg_mask.sum())`` included)."""
    loss = dict()
    if zoe:
        pred, gt = depth_preds.reshape(-1), depth_labels.reshape(-1)
        valid = gt < VALID_BELOW
        pred, gt = pred[valid], gt[valid]
        alpha = 1e-7
        g = torch.log(pred + alpha) - torch.log(gt + alpha)
        Dg = torch.var(g) + 0.15 * torch.pow(torch.mean(g), 2)
        loss['loss_depth_zoe'] = torch.clip(torch.sqrt(Dg), max=2.0)
    if ce:
        labels = one_hot_depth_torch(depth_labels, D, lo, step).to(depth_preds.dtype)
        preds = two_hot_depth_torch(depth_preds, D, lo, step, gamma)
        fg = torch.max(labels, dim=1).values > 0.0
        labels, preds = labels[fg], preds[fg]
        bce = F.binary_cross_entropy(preds, labels, reduction='none').sum() / max(1.0, fg.sum())
        loss['loss_depth_ce'] = bce * 0.05
    return loss


def depth_error_torch(depth_labels, depth_preds):
    """The statistic of forward_train (:141-145) as a tensor: mean |pred - gt| over the
    rows whose label is below 9225, no gradient."""
    with torch.no_grad():
        pred, gt = depth_preds.reshape(-1), depth_labels.reshape(-1)
        valid = gt < VALID_BELOW
        return torch.abs(pred[valid] - gt[valid]).mean()


def depth_pretrain_loss_torch(depth, gt_depth, D, lo, step, pred_scale=8, gt_scale=16,
                              gamma=4, zoe=True, ce=True):
    """The reference's sequence in torch, any dtype and device: downsample both maps,
    the statistic, ``get_depth_loss_own``.  -> the loss dict plus ``depth_error``."""
    _check_shapes(depth, gt_depth, pred_scale, gt_scale, ValueError)
    pred_ds = downsample_depth_torch(depth, pred_scale)
    gt_ds = downsample_depth_torch(gt_depth, gt_scale).to(depth.dtype)
    out = depth_loss_own_torch(gt_ds, pred_ds, D, lo, step, gamma, zoe, ce)
    out['depth_error'] = depth_error_torch(gt_ds, pred_ds)
    return out


# ------------------------------------------------------------------ native path
def _check_shapes(depth, gt_depth, sp, sg, error):
    if depth.dim() != 4 or gt_depth.dim() != 4 or depth.shape[:2] != gt_depth.shape[:2]:
        raise error('depth and gt_depth must be (B, N, H, W) maps of the same B, N; got '
                    '%s and %s' % (tuple(depth.shape), tuple(gt_depth.shape)))
    if sp not in SCALES or sg not in SCALES:
        raise error('scales must be in %s, got %s and %s' % (SCALES, sp, sg))
    (Hp, Wp), (Hg, Wg) = depth.shape[2:], gt_depth.shape[2:]
    if Hp % sp or Wp % sp or Hg % sg or Wg % sg:
        raise error('a map is not a multiple of its scale: %dx%d by %d, %dx%d by %d'
                    % (Hp, Wp, sp, Hg, Wg, sg))
    if (Hp // sp, Wp // sp) != (Hg // sg, Wg // sg) or 0 in depth.shape:
        raise error('the downsampled maps differ: %dx%d by %d against %dx%d by %d'
                    % (Hp, Wp, sp, Hg, Wg, sg))


def _check_native(*tensors):
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.VeonHipError('the native depth loss takes contiguous fp32 maps, got '
                                    '%s with strides %s' % (t.dtype, t.stride()))


def loss_rows(depth, gt_depth, D, lo, step, pred_scale=8, gt_scale=16, gamma=4):
    """veon_depth_loss_rows: -> the (rows, 8) fp32 record tensor of include/veon_hip.h."""
    dev = _lib.require_device(depth, gt_depth)
    _check_shapes(depth, gt_depth, pred_scale, gt_scale, _lib.VeonHipError)
    _check_native(depth, gt_depth)
    B, N, Hp, Wp = depth.shape
    Hg, Wg = gt_depth.shape[2:]
    rows = B * N * (Hp // pred_scale) * (Wp // pred_scale)
    rec = torch.empty((rows, REC), dtype=torch.float32, device=dev)
    _lib.launch('veon_depth_loss_rows', dev, B * N, Hp, Wp, pred_scale, Hg, Wg, gt_scale,
                int(D), float(lo), float(step), float(gamma), depth, gt_depth, rec)
    return rec


def unpack_rows(rec):
    """The record tensor's fields by name (views and integer decodes; for tests/tools)."""
    flags, packed = rec[:, 3].view(torch.int32), rec[:, 7].view(torch.int32)
    return dict(g=rec[:, 0], abs_err=rec[:, 1], bce=rec[:, 2], valid=(flags & 1).bool(),
                fg=(flags & 2).bool(), d=rec[:, 4], t=rec[:, 5], dbce=rec[:, 6],
                winner=packed & 0xff, winner_zero=(packed & 0x100).bool(),
                label_bin=packed >> 16)


def loss_reduce(rec):
    """veon_depth_loss_reduce: -> (out (3,) = loss_depth_zoe, loss_depth_ce, depth_error;
    coef (8,), the backward's coefficients)."""
    dev = _lib.require_device(rec)
    _check_native(rec)
    out = torch.empty((3,), dtype=torch.float32, device=dev)
    coef = torch.empty((8,), dtype=torch.float32, device=dev)
    _lib.launch('veon_depth_loss_reduce', dev, rec.shape[0], rec, out, coef)
    return out, coef


def loss_backward(rec, coef, shape, pred_scale, g_zoe=None, g_ce=None, out=None):
    """veon_depth_loss_bwd: the gradient map of ``shape`` = (B, N, Hp, Wp) for the
    upstream gradients ``g_zoe`` / ``g_ce`` (fp32 device scalars; None: that loss
    contributes nothing).  Every element of ``out`` is stored (no memset needed)."""
    dev = _lib.require_device(rec, coef, g_zoe, g_ce, out)
    B, N, Hp, Wp = (int(v) for v in shape)
    if pred_scale not in SCALES or Hp % pred_scale or Wp % pred_scale or \
            tuple(rec.shape) != (B * N * (Hp // pred_scale) * (Wp // pred_scale), REC) or \
            coef.numel() != 8:
        raise _lib.VeonHipError('records %s do not belong to a %s map at scale %d'
                                % (tuple(rec.shape), (B, N, Hp, Wp), pred_scale))
    if out is None:
        out = torch.empty((B, N, Hp, Wp), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, N, Hp, Wp):
        raise _lib.VeonHipError('out is %s, not %s' % (tuple(out.shape), (B, N, Hp, Wp)))
    scalars = [g for g in (g_zoe, g_ce) if g is not None]
    if any(g.numel() != 1 for g in scalars):
        raise _lib.VeonHipError('the upstream gradients must be scalars')
    _check_native(rec, coef, out, *scalars)
    _lib.launch('veon_depth_loss_bwd', dev, B * N, Hp, Wp, pred_scale, rec, coef, g_zoe, g_ce,
                out)
    return out


class _DepthLoss(torch.autograd.Function):
    """veon_depth_loss_rows + _reduce / veon_depth_loss_bwd; saves the row records and
    the coefficients only."""

    @staticmethod
    def forward(ctx, depth, gt_depth, D, lo, step, sp, sg, gamma):
        rec = loss_rows(depth.detach(), gt_depth, D, lo, step, sp, sg, gamma)
        out, coef = loss_reduce(rec)
        ctx.save_for_backward(rec, coef)
        ctx.shape, ctx.sp = tuple(depth.shape), sp
        ctx.set_materialize_grads(False)
        zoe, ce, err = out[0], out[1], out[2]
        ctx.mark_non_differentiable(err)
        return zoe, ce, err

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_zoe, g_ce, _g_err):
        if not ctx.needs_input_grad[0] or (g_zoe is None and g_ce is None):
            return (None,) * 8
        rec, coef = ctx.saved_tensors
        g_zoe, g_ce = (None if g is None else g.to(torch.float32).contiguous()
                       for g in (g_zoe, g_ce))
        return (loss_backward(rec, coef, ctx.shape, ctx.sp, g_zoe, g_ce),) + (None,) * 7


def depth_pretrain_loss(depth, gt_depth, D, lo, step, pred_scale=8, gt_scale=16, gamma=4,
                        zoe=True, ce=True):
    """``forward_train``'s loss from the full-resolution maps.

    depth (B, N, Hp, Wp): the predicted metric depth, may require grad; gt_depth
    (B, N, Hg, Wg): the LiDAR depth, zero where there is no return; Hp/pred_scale =
    Hg/gt_scale.  D, lo, step: the lift's depth bins (``grid_config['depth']`` = [lo, hi,
    step], D = (hi - lo)/step).  -> {'loss_depth_zoe' (if zoe), 'loss_depth_ce' (if ce),
    'depth_error'} as 0-dim tensors; ``depth_error`` carries no gradient.

    With d / t the block-min of a row's prediction / label block, zeros read as 1e5 (the
    gradient of d goes to the first minimal pixel in row-major order, and nowhere if that
    pixel was a zero): rows with t < 9225 are valid, g = log(d + 1e-7) - log(t + 1e-7),
    loss_depth_zoe = min(sqrt(var g + 0.15 mean(g)^2), 2), depth_error = mean |d - t|;
    rows whose label bin (nearest of the D+1 centres to min(t, 500)) is below D are
    foreground, loss_depth_ce = 0.05 * sum over them of BCE(two-hot(d), one-hot) /
    max(1, n_fg).  Fewer than two valid rows give NaN, as the torch formulation does.

    ROCm tensors: native (contiguous fp32 only, anything else raises VeonHipError), no
    host synchronisation, graph-capturable.  CPU tensors: ``depth_pretrain_loss_torch``."""
    pred_scale, gt_scale = int(pred_scale), int(gt_scale)
    if not depth.is_cuda:
        return depth_pretrain_loss_torch(depth, gt_depth, D, lo, step, pred_scale, gt_scale,
                                         gamma, zoe, ce)
    l_zoe, l_ce, err = _DepthLoss.apply(depth, gt_depth, int(D), float(lo), float(step),
                                        pred_scale, gt_scale, float(gamma))
    out = dict()
    if zoe:
        out['loss_depth_zoe'] = l_zoe
    if ce:
        out['loss_depth_ce'] = l_ce
    out['depth_error'] = err
    return out
