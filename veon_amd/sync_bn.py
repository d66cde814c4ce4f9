"""nn.SyncBatchNorm on the native training paths (csrc/conv3d_train.hip).

A synchronised train-mode BatchNorm is the plain one with one collective in the middle of
each direction: local per-channel sums and the local count go into ONE fp64 buffer
``stats[2C + 1]``, the ranks add their buffers (``all_reduce``), and the coefficients of
the apply pass come from the totals.  Forward: (sum y, sum y^2, n) -> mean, rstd, scale,
shift and the running buffers (identical on every rank).  Backward: (sum dz, sum dz xhat,
n) -> ca, cb, cc; the parameter gradients stay the LOCAL sums (DDP averages them).

``batch_norm_train`` is the same sequence in plain torch on (B, C, ...) tensors of any
device: the statement of the semantics (torch's own SyncBatchNorm refuses CPU tensors),
and the yardstick of the GPU tests.
"""
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from . import conv3d_ops

# number of collectives issued by ``all_reduce`` (the tests assert on it)
ALL_REDUCE_CALLS = 0
_DEFAULT = object()


def is_sync(bn):
    return isinstance(bn, nn.SyncBatchNorm)


def group_of(bn):
    """The process group ``bn`` synchronises over: its own, else the default group when
    torch.distributed is initialised, else None (no collective)."""
    group = getattr(bn, 'process_group', None)
    if group is not None:
        return group
    if dist.is_available() and dist.is_initialized():
        return dist.group.WORLD
    return None


def all_reduce(stats, group):
    """Sum the fp64 message over ``group`` in place; None: nothing to do.  With a group
    the collective is always issued, a world of one rank included, so that every rank
    issues the same sequence."""
    global ALL_REDUCE_CALLS
    if group is None:
        return stats
    assert stats.dtype == torch.float64 and stats.is_contiguous()
    ALL_REDUCE_CALLS += 1
    dist.all_reduce(stats, group=group)
    return stats


# ------------------------------------------------------------------ the C-sized algebra
def train_coeffs_ref(stats, gamma, beta, eps, momentum=0.1, running_mean=None,
                     running_var=None, num_batches_tracked=None, mean_offset=None):
    """What ``veon_bn_train_coeffs`` computes, in fp64 torch on any device: reduced
    ``stats`` (2C + 1) -> (mean, rstd, scale, shift) in fp64; the running buffers, when
    given, are updated in place (``momentum`` None: the cumulative average)."""
    C = gamma.numel()
    s = stats.double()
    n = s[2 * C]
    mean = s[:C] / n
    var = (s[C:2 * C] / n - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    scale = gamma.detach().double() * rstd
    shift = beta.detach().double() - mean * scale
    if running_mean is not None:
        with torch.no_grad():
            num_batches_tracked += 1
            f = momentum if momentum is not None else 1.0 / num_batches_tracked.double()
            mo = mean if mean_offset is None else mean + mean_offset.detach().double()
            unbiased = var * (n / (n - 1).clamp_min(1))
            running_mean.copy_(((1 - f) * running_mean.double() + f * mo)
                               .to(running_mean.dtype))
            running_var.copy_(((1 - f) * running_var.double() + f * unbiased)
                              .to(running_var.dtype))
    return mean, rstd, scale, shift


def bwd_coeffs_ref(stats, gamma, mean, rstd):
    """What ``veon_bn_bwd_coeffs`` computes, in fp64: reduced backward ``stats`` ->
    (ca, cb, cc) with dy = ca dz + cb y + cc (``conv3d_ops.bn_bwd_coefficients`` with the
    total count from the buffer)."""
    C = gamma.numel()
    s = stats.double()
    n = s[2 * C]
    g, mu, r = gamma.detach().double(), mean.double(), rstd.double()
    ca = g * r
    cb = -g * r * r * s[C:2 * C] / n
    cc = -g * r * s[:C] / n - cb * mu
    return ca, cb, cc


# ------------------------------------------------------------------- native wrappers
def _stats_buffer(C, dev, out=None):
    if out is None:
        return torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64 and out.numel() == 2 * C + 1 and out.is_contiguous()
    return out


def bn_sums_stats(y, out=None):
    """(sum y, sum y^2, n) of a PaddedVolume -> fp64 (2C + 1): the forward message
    (``out``: an existing buffer to overwrite)."""
    dev = _lib.require_device(y.storage, out)
    B, C, Z, Y, X = y.shape
    stats = _stats_buffer(C, dev, out)
    _lib.launch('veon_bn3d_sums_stats_bf16', dev, y.rows, stats,
                conv3d_ops._bn_workspace(C, dev), B, C, Z, Y, X)
    return stats


def bn_bwd_sums_stats(da, a, y, mean, rstd, out=None):
    """(sum dz, sum dz xhat, n) as ``conv3d_ops.bn_bwd_sums`` defines them -> (fp64
    (2C + 1) message, fp32 (2, C) local sums: dbeta, dgamma); ``out``: an existing pair of
    buffers to overwrite."""
    dev = _lib.require_device(da.storage, a.storage, y.storage, mean, rstd)
    B, C, Z, Y, X = y.shape
    assert da.shape == a.shape == y.shape
    assert mean.dtype == rstd.dtype == torch.float32 and mean.numel() == rstd.numel() == C
    stats = _stats_buffer(C, dev, None if out is None else out[0])
    sums = torch.empty((2, C), dtype=torch.float32, device=dev) if out is None else out[1]
    assert sums.dtype == torch.float32 and sums.numel() == 2 * C and sums.is_contiguous()
    _lib.launch('veon_bn3d_bwd_sums_stats_bf16', dev, da.rows, a.rows, y.rows,
                mean.contiguous(), rstd.contiguous(), stats, sums,
                conv3d_ops._bn_workspace(C, dev), B, C, Z, Y, X)
    return stats, sums


def _f32_vec(t, C, what):
    if t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous():
        raise _lib.VeonHipError('synchronised BN: %s must be a contiguous fp32 vector of %d '
                                'channels, got %s %s' % (what, C, t.dtype, tuple(t.shape)))
    return t


def bn_train_coeffs(stats, gamma, beta, eps, momentum=0.1, running_mean=None,
                    running_var=None, num_batches_tracked=None, mean_offset=None):
    """Reduced forward ``stats`` -> fp32 (mean, rstd, scale, shift) in one launch; the
    running buffers (fp32, fp32, int64; all or none) are updated in place on the device.
    ``momentum`` None: the cumulative average, from the device's counter."""
    dev = _lib.require_device(stats, gamma, beta, running_mean, running_var,
                              num_batches_tracked, mean_offset)
    C = gamma.numel()
    assert stats.dtype == torch.float64 and stats.numel() == 2 * C + 1 and stats.is_contiguous()
    gamma, beta = _f32_vec(gamma.detach(), C, 'gamma'), _f32_vec(beta.detach(), C, 'beta')
    if running_mean is not None:
        _f32_vec(running_mean, C, 'running_mean')
        _f32_vec(running_var, C, 'running_var')
        assert num_batches_tracked.dtype == torch.int64 and num_batches_tracked.numel() == 1
    if mean_offset is not None:
        mean_offset = _f32_vec(mean_offset.detach(), C, 'mean_offset')
    out = torch.empty((4, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_bn_train_coeffs', dev, stats, gamma, beta, mean_offset, float(eps),
                -1.0 if momentum is None else float(momentum), running_mean, running_var,
                num_batches_tracked, out[0], out[1], out[2], out[3], C)
    return out[0], out[1], out[2], out[3]


def bn_bwd_coeffs(stats, gamma, mean, rstd):
    """Reduced backward ``stats`` -> fp32 (ca, cb, cc) of ``bn_bwd_apply``, one launch."""
    dev = _lib.require_device(stats, gamma, mean, rstd)
    C = gamma.numel()
    assert stats.dtype == torch.float64 and stats.numel() == 2 * C + 1 and stats.is_contiguous()
    out = torch.empty((3, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_bn_bwd_coeffs', dev, stats, _f32_vec(gamma.detach(), C, 'gamma'),
                _f32_vec(mean, C, 'mean'), _f32_vec(rstd, C, 'rstd'), out[0], out[1], out[2],
                C)
    return out[0], out[1], out[2]


# ----------------------------------------- what the native autograd functions call
def forward_coeffs(y, bn, group, mean_offset=None):
    """The forward statistics interval of a synchronised ``bn`` on the stored conv output
    ``y`` (PaddedVolume): local sums, the collective, one coefficient launch (which also
    updates ``bn``'s buffers) -> fp32 (mean, rstd, scale, shift).  No host read-back."""
    stats = all_reduce(bn_sums_stats(y), group)
    track = bn.track_running_stats and bn.running_mean is not None
    return bn_train_coeffs(stats, bn.weight, bn.bias, bn.eps, bn.momentum,
                           bn.running_mean if track else None,
                           bn.running_var if track else None,
                           bn.num_batches_tracked if track else None, mean_offset)


def backward_coeffs(da, a, y, mean, rstd, gamma, group):
    """The backward interval -> ((ca, cb, cc), local fp32 sums (2, C): dbeta, dgamma)."""
    stats, sums = bn_bwd_sums_stats(da, a, y, mean, rstd)
    return bn_bwd_coeffs(all_reduce(stats, group), gamma, mean, rstd), sums


# ------------------------------------------------------------------------ torch mirror
def _dims(x):
    return [0] + list(range(2, x.dim()))


def _message(s0, s1, n):
    return torch.cat([s0.double(), s1.double(),
                      torch.tensor([float(n)], dtype=torch.float64, device=s0.device)])


class _BatchNormTrainFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, gamma, beta, ident, bn, relu, group):
        C = x.shape[1]
        x64 = x.detach().double()
        n = x.numel() // C
        stats = all_reduce(_message(x64.sum(_dims(x)), (x64 * x64).sum(_dims(x)), n), group)
        track = bn.track_running_stats and bn.running_mean is not None
        mean, rstd, scale, shift = train_coeffs_ref(
            stats, gamma, beta, bn.eps, bn.momentum, bn.running_mean if track else None,
            bn.running_var if track else None, bn.num_batches_tracked if track else None)
        z = x64 * conv3d_ops._bshape(scale, x) + conv3d_ops._bshape(shift, x)
        if ident is not None:
            z = z + ident.detach().double()
        a = (z.relu() if relu else z).to(x.dtype)
        ctx.relu, ctx.group, ctx.has_ident = relu, group, ident is not None
        ctx.save_for_backward(x, a, gamma, mean, rstd)
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, da):
        x, a, gamma, mean, rstd = ctx.saved_tensors
        C = x.shape[1]
        x64, d64 = x.double(), da.double()
        dz = d64 * (a > 0).double() if ctx.relu else d64
        xhat = (x64 - conv3d_ops._bshape(mean, x)) * conv3d_ops._bshape(rstd, x)
        dbeta, dgamma = dz.sum(_dims(x)), (dz * xhat).sum(_dims(x))
        # the collective is issued whatever needs a gradient: every rank runs the same list
        stats = all_reduce(_message(dbeta, dgamma, x.numel() // C), ctx.group)
        ca, cb, cc = bwd_coeffs_ref(stats, gamma, mean, rstd)
        b = conv3d_ops._bshape
        dx = (b(ca, x) * dz + b(cb, x) * x64 + b(cc, x)).to(x.dtype)
        return (dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype),
                dz.to(x.dtype) if ctx.has_ident else None, None, None, None)


def batch_norm_train(x, bn, ident=None, relu=True, group=_DEFAULT):
    """Train-mode (synchronised) BatchNorm (+ ``ident``) (+ ReLU) of ``x`` (B, C, ...) in
    plain torch under autograd, phase by phase what the native path runs: fp64 local sums
    and count, all-reduce over ``group`` (default: ``group_of(bn)``; None: no collective),
    coefficients, apply; backwards local sums, all-reduce, closed form.  Updates ``bn``'s
    running buffers; ``bn.weight.grad`` / ``bn.bias.grad`` receive the LOCAL sums."""
    if group is _DEFAULT:
        group = group_of(bn)
    return _BatchNormTrainFn.apply(x, bn.weight, bn.bias, ident, bn, relu, group)
