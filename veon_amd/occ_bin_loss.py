"""The occupancy term of VEON's training loss from the LOW-resolution logits:
``BCE_BinOcc_Loss`` (loss/occ_loss_utils/occ3d_nuscenes.py:200-212) on the trilinearly
upsampled ``bin_occ`` (san_in_veon_temporal.py:202-210).

The reference upsamples the two logit channels to the labelled grid, permutes them to the
labels' (X, Y, Z) order and calls ``F.cross_entropy`` with class weights and an ignore
index: a dozen launches in each direction.  On a ROCm device ``bin_occ_loss`` is native in
both directions (csrc/occ_bin_loss.hip): the upsampled logits are never stored, nothing is
read back, and the pair can sit in a captured graph.  ``bin_occ_loss_torch`` is the torch
sequence at any dtype (the CPU path and the tests' yardstick); ``bin_occ_loss_bwd_ref``
restates the native backward's gather formulation in torch, so the algorithm is checked
without a device."""
import torch
import torch.nn.functional as F

from . import _lib


def _check_args(bin_low, labels, occ_size, error):
    if not isinstance(bin_low, torch.Tensor) or bin_low.dim() != 5 or bin_low.shape[1] != 2 \
            or not bin_low.is_floating_point() or 0 in bin_low.shape:
        raise error('bin_low must be a floating-point (B, 2, z, y, x) tensor')
    if len(occ_size) != 3 or min(occ_size) < 1:
        raise error('occ_size must be (Z, Y, X)')
    Zo, Yo, Xo = occ_size
    if labels.is_floating_point() or tuple(labels.shape) != (bin_low.shape[0], Xo, Yo, Zo):
        raise error('labels must be an integer (B, X, Y, Z) = %s tensor, got %s %s'
                    % ((bin_low.shape[0], Xo, Yo, Zo), labels.dtype, tuple(labels.shape)))


# ------------------------------------------------------------------ torch sequence
def bin_occ_loss_torch(bin_low, labels, class_weights, occ_size, ignore_index=255,
                       free_index=17):
    """The torch sequence of ``OccLossFB.loss_voxel``: upsample, permute to the labels'
    order, ``BCE_BinOcc_Loss``.  Any device; fp64 logits stay fp64, every other dtype is
    computed in fp32 as the loss module does."""
    from .models.semantic_net.occ_loss import BCE_BinOcc_Loss
    occ_size = tuple(int(v) for v in occ_size)
    _check_args(bin_low, labels, occ_size, ValueError)
    x = bin_low if bin_low.dtype == torch.float64 else bin_low.float()
    bin_up = F.interpolate(x, size=occ_size, mode='trilinear',
                           align_corners=False).permute(0, 1, 4, 3, 2)
    return BCE_BinOcc_Loss(bin_up, labels, class_weights.to(bin_up),
                           ignore_index=ignore_index, free_index=free_index)


# ------------------------------------------------------------------ gather formulation
def _axis_taps(n_in, dtype, device):
    """Per low-resolution index i of an axis upsampled 2x: the 4 candidate outputs
    2i-1 .. 2i+2 (clipped copies where outside the grid) and the weight with which each
    reads i -- ATen's source-index rule (csrc/occ_interp.h ``source``) transposed."""
    n_out = 2 * n_in
    i = torch.arange(n_in, device=device).view(-1, 1)
    o = 2 * i - 1 + torch.arange(4, device=device).view(1, -1)
    inside = (o >= 0) & (o < n_out)
    src = (0.5 * (o.to(dtype) + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = (src - i0.to(dtype)).clamp(0, 1)
    l0 = 1 - l1
    w = l0 * (i0 == i).to(dtype) + l1 * (i1 == i).to(dtype)
    return o.clamp(0, n_out - 1), w * inside.to(dtype)


def bin_occ_loss_bwd_ref(bin_low, labels, class_weights, occ_size, ignore_index=255,
                         free_index=17, grad_out=1.0):
    """The native pair's algorithm in plain torch, in the dtype of ``bin_low``, for
    ``occ_size`` = 2x the low grid: per output voxel the coefficient
    c = w_t (p_0 - [t == 0]) (0 where ignored), then per LOW-resolution voxel the sum of c
    over the outputs 2i-1 .. 2i+2 of every axis times the weights with which they read it.
    -> (loss, gradient (B, 2, z, y, x)); channel 1 is the negative of channel 0."""
    occ_size = tuple(int(v) for v in occ_size)
    _check_args(bin_low, labels, occ_size, ValueError)
    B, _, zi, yi, xi = bin_low.shape
    if occ_size != (2 * zi, 2 * yi, 2 * xi):
        raise ValueError('the gather formulation covers the 2x upsampling only')
    dt, dev = bin_low.dtype, bin_low.device
    with torch.no_grad():
        up = F.interpolate(bin_low, size=occ_size, mode='trilinear', align_corners=False)
        lab = labels.long().permute(0, 3, 2, 1)                     # (B, Zo, Yo, Xo)
        counted = lab != ignore_index
        t = (lab >= free_index).long()
        w = class_weights.to(device=dev, dtype=dt)[t] * counted.to(dt)
        m = up.max(dim=1).values
        e = torch.exp(up - m[:, None])
        s = e.sum(1)
        nll = m + torch.log(s) - up.gather(1, t[:, None])[:, 0]
        den = w.sum()
        loss = (w * nll).sum() / den
        c = w * (e[:, 0] / s - (t == 0).to(dt))                     # d (w nll) / d up_0
        for axis, n_in in ((1, zi), (2, yi), (3, xi)):
            o, wt = _axis_taps(n_in, dt, dev)
            taps = c.index_select(axis, o.reshape(-1))
            shape = list(c.shape)
            shape[axis:axis + 1] = [n_in, 4]
            wshape = [1] * len(shape)
            wshape[axis:axis + 2] = [n_in, 4]
            c = (taps.reshape(shape) * wt.view(wshape)).sum(axis + 1)
        inv = torch.where(den > 0, 1 / den, torch.zeros_like(den))
        g0 = c * (inv * grad_out)
    return loss, torch.stack([g0, -g0], dim=1)


# ------------------------------------------------------------------ native path
# (B, Z, Y, X, device) -> fp64 partial sums, consumed inside one call.  As with the other
# native caches, one buffer per shape and device serves every stream: two streams that run
# the loss at the same shape concurrently must be ordered by the caller.
_WORKSPACES = {}


def loss_forward(bin_low, labels, class_weights, occ_size, ignore_index=255, free_index=17):
    """veon_occ_bin_loss_fwd: -> (coef (B, Xo, Yo, Zo) fp32, out (2,) = loss, 1 / sum w)
    of include/veon_hip.h.  ``bin_low`` fp32 with any strides, ``labels`` uint8 contiguous,
    ``class_weights`` (2,) fp32 on the device."""
    dev = _lib.require_device(bin_low, labels, class_weights)
    occ_size = tuple(int(v) for v in occ_size)
    _check_args(bin_low, labels, occ_size, _lib.VeonHipError)
    if bin_low.dtype != torch.float32 or labels.dtype != torch.uint8 or \
            not labels.is_contiguous() or class_weights.dtype != torch.float32 or \
            class_weights.numel() != 2 or not class_weights.is_contiguous():
        raise _lib.VeonHipError('the native occupancy loss takes fp32 logits, contiguous '
                                'uint8 labels and two fp32 class weights')
    B, _, zi, yi, xi = bin_low.shape
    Zo, Yo, Xo = occ_size
    nbytes = int(_lib.lib().veon_occ_bin_loss_workspace_bytes(B, Zo, Yo, Xo))
    if nbytes < 0:
        raise _lib.VeonHipError('bin_occ_loss: unsupported grid %s x %s' % (B, occ_size))
    key = (B, Zo, Yo, Xo, str(dev))
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    coef = torch.empty((B, Xo, Yo, Zo), dtype=torch.float32, device=dev)
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    _lib.launch('veon_occ_bin_loss_fwd', dev, bin_low, _lib.strides(bin_low), B, zi, yi, xi, Zo,
                Yo, Xo, labels, class_weights, int(ignore_index), int(free_index), coef, ws,
                nbytes, out)
    return coef, out


def loss_backward(coef, out, grad_out, low_shape, grad=None):
    """veon_occ_bin_loss_bwd (2x grids): -> the (B, 2, z, y, x) fp32 gradient, every
    element stored (``grad``: a contiguous tensor of that shape to write into).
    ``grad_out``: the upstream gradient, an fp32 device scalar."""
    dev = _lib.require_device(coef, out, grad_out, grad)
    B, zi, yi, xi = (int(v) for v in low_shape)
    if tuple(coef.shape) != (B, 2 * xi, 2 * yi, 2 * zi) or out.numel() != 2 or \
            grad_out.numel() != 1:
        raise _lib.VeonHipError('coefficients %s do not belong to a %s grid upsampled 2x'
                                % (tuple(coef.shape), (B, zi, yi, xi)))
    if grad is None:
        grad = torch.empty((B, 2, zi, yi, xi), dtype=torch.float32, device=dev)
    for t in (coef, out, grad_out, grad):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.VeonHipError('the native occupancy loss takes contiguous fp32 tensors')
    if tuple(grad.shape) != (B, 2, zi, yi, xi):
        raise _lib.VeonHipError('grad is %s, not %s' % (tuple(grad.shape), (B, 2, zi, yi, xi)))
    _lib.launch('veon_occ_bin_loss_bwd', dev, coef, out, grad_out, B, zi, yi, xi, grad)
    return grad


class _BinOccLoss(torch.autograd.Function):
    """veon_occ_bin_loss_fwd / veon_occ_bin_loss_bwd; saves the per-voxel coefficients and
    the two scalars (and, for a grid that is not 2x, what the torch backward needs)."""

    @staticmethod
    def forward(ctx, bin_low, labels, class_weights, occ_size, ignore_index, free_index):
        coef, out = loss_forward(bin_low.detach(), labels, class_weights, occ_size,
                                 ignore_index, free_index)
        ctx.low_shape = (bin_low.shape[0],) + tuple(bin_low.shape[2:])
        ctx.args = (occ_size, ignore_index, free_index)
        ctx.native = occ_size == tuple(2 * v for v in bin_low.shape[2:])
        if ctx.native:
            ctx.save_for_backward(coef, out)
        else:
            ctx.save_for_backward(bin_low.detach(), labels, class_weights)
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        if ctx.native:
            coef, out = ctx.saved_tensors
            g = g.to(torch.float32).contiguous()
            return (loss_backward(coef, out, g, ctx.low_shape),) + (None,) * 5
        # the native backward's stencil is the 2x one: any other scale takes the torch
        # sequence (and forms the upsampled logits)
        low, labels, cw = ctx.saved_tensors
        with torch.enable_grad():
            leaf = low.clone().requires_grad_(True)
            loss = bin_occ_loss_torch(leaf, labels, cw, *ctx.args)
            grad, = torch.autograd.grad(loss, leaf, g.to(loss.dtype))
        return (grad,) + (None,) * 5


def bin_occ_loss(bin_low, labels, class_weights, occ_size, ignore_index=255, free_index=17):
    """The weighted two-class cross entropy of the upsampled occupancy logits.

    bin_low (B, 2, z, y, x): the low-resolution logits, any strides, may require grad.
    labels (B, X, Y, Z): integer semantic labels with VALUES IN [0, 255] (any integer
    dtype; other dtypes than uint8 are cast on the device, without a read-back, so a value
    outside that range wraps instead of raising).  class_weights: (w_0, w_1) for occupied /
    free.  occ_size = (Z, Y, X): output voxel (zo, yo, xo) has label labels[b, xo, yo, zo].

        up   = trilinear(bin_low, occ_size, align_corners=False)
        t    = 0 where label < free_index, 1 where label >= free_index
        loss = sum w_t (logsumexp(up) - up_t) / sum w_t   over label != ignore_index

    -> a 0-dim tensor.  Every voxel ignored: NaN, with an all-zero gradient, as torch.

    ROCm fp32 tensors: native (csrc/occ_bin_loss.hip), no host synchronisation, no atomics,
    graph-capturable on one stream, bit-reproducible (the forward's partial sums live in one
    workspace per shape and device: calls of the same shape on different streams must be
    ordered by the caller); the backward is native for ``occ_size`` = 2x the low
    grid (VEON's) and the torch sequence for any other scale.  Other ROCm dtypes raise
    VeonHipError.  CPU tensors: ``bin_occ_loss_torch``."""
    occ_size = tuple(int(v) for v in occ_size)
    if not bin_low.is_cuda:
        return bin_occ_loss_torch(bin_low, labels, class_weights, occ_size, ignore_index,
                                  free_index)
    _check_args(bin_low, labels, occ_size, _lib.VeonHipError)
    if bin_low.dtype != torch.float32:
        raise _lib.VeonHipError('bin_occ_loss differentiates fp32 logits only, got %s'
                                % bin_low.dtype)
    labels = labels.to(torch.uint8).contiguous()
    cw = torch.as_tensor(class_weights).to(device=bin_low.device,
                                           dtype=torch.float32).contiguous()
    return _BinOccLoss.apply(bin_low, labels, cw, occ_size, int(ignore_index),
                             int(free_index))
