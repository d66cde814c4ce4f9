"""Autograd functions of the native training paths of token models (the HSA heads, the
DINOv2 blocks): each forward and backward is a sequence of HIP kernels of ``vit_ops``
(csrc/vit_block.hip, linear_train.hip, attention_train.hip) on half rows.

Conventions shared by all of them: activations between two kernels are half rows
[M, width]; parameters stay fp32 ``nn.Parameter`` s and their half copies are re-packed
every step; parameter gradients come back fp32 in the parameters' own layout, and only
those ``needs_input_grad`` asks for are computed.  In the fp16 flavour every gradient
between two kernels is rounded to fp16: loss scaling is the caller's business.
"""
import torch
import torch.nn.functional as F

from .. import conv3d_ops, fusion_ops, sync_bn, vit_ops

LORA_PAD = 64   # the rank is zero-padded to the GEMM's and the weight gradient's tile width


def _half_weight(w, transpose=False):
    """The half copy of an fp32 Linear weight, re-packed every step; ``transpose``:
    [K][N], the weight of the data gradient as a GEMM of ``vit_ops.linear``."""
    w = w.detach().float()
    return vit_ops.to_bf16(w.t().contiguous() if transpose else w)


def _bias(b):
    return None if b is None else b.detach().float().contiguous()


def lora_pad_a(lora_a):
    """lora_A fp32 [r, in] -> fp32 [64, in]: rows r.. zero."""
    r, k = lora_a.shape
    assert 0 < r <= LORA_PAD
    out = lora_a.new_zeros((LORA_PAD, k), dtype=torch.float32)
    out[:r] = lora_a.detach().float()
    return out


def lora_pad_b(lora_b, scaling):
    """lora_B fp32 [out, r] -> fp32 [out, 64] = scaling * B in columns 0..r-1, zero beyond
    (the scaling rides on B, so the branch is two plain GEMMs)."""
    n, r = lora_b.shape
    assert 0 < r <= LORA_PAD
    out = lora_b.new_zeros((n, LORA_PAD), dtype=torch.float32)
    out[:, :r] = lora_b.detach().float() * scaling
    return out


class _LNHalfFn(torch.autograd.Function):
    """nn.LayerNorm of fp32 tokens [..., d] -> half rows [M, d]; backward on
    ``veon_layernorm_f32_bwd`` from the half gradient (statistics recomputed from the
    saved input)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x2 = x.detach().contiguous().view(-1, x.shape[-1])
        ctx.eps, ctx.shape = eps, x.shape
        ctx.save_for_backward(x2, gamma)
        return vit_ops.layernorm(x2, gamma.detach(), beta.detach(), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dxn):
        x2, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dg, de = vit_ops.layernorm_f32_bwd(dxn.contiguous(), x2,
                                               gamma.detach().contiguous(), ctx.eps)
        return (dx.view(ctx.shape) if need[0] else None, dg if need[1] else None,
                de if need[2] else None, None)


class _GeluFn(torch.autograd.Function):
    """Exact GELU on half rows from the saved pre-activation."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return vit_ops.gelu(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh):
        y, = ctx.saved_tensors
        return vit_ops.gelu_bwd(dh.contiguous(), y)


class _QuickGeluFn(torch.autograd.Function):
    """CLIP's QuickGELU on half rows from the saved pre-activation."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return vit_ops.quickgelu(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh):
        y, = ctx.saved_tensors
        return vit_ops.quickgelu_bwd(dh.contiguous(), y)


class _FFHiddenFn(torch.autograd.Function):
    """The first half of ``FeedForward`` for training (csrc/linear_train.hip): fp32 tokens
    x -> h = GELU(LN(x) W1^T + b1), half.  Saved for backward: x, the half rows LN(x) and the
    pre-activation y1 (GELU is not invertible).  Parameter gradients are fp32 in the
    parameters' own layout.  In the fp16 flavour every gradient between two kernels is
    rounded to fp16: loss scaling is the caller's business."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, eps):
        x2 = x.detach().contiguous().view(-1, x.shape[-1])
        xn = vit_ops.layernorm(x2, gamma.detach(), beta.detach(), eps)
        y1 = vit_ops.linear(xn, _half_weight(w1), b1.detach().float().contiguous())
        ctx.eps = eps
        ctx.save_for_backward(x2, xn, y1, gamma, w1)
        return vit_ops.gelu(y1).view(*x.shape[:-1], -1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh):
        x2, xn, y1, gamma, w1 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy1 = vit_ops.gelu_bwd(dh.contiguous().view(y1.shape), y1)
        db1 = vit_ops.colsum(dy1).to(w1.dtype) if need[4] else None
        dw1 = vit_ops.linear_wgrad(dy1, xn).to(w1.dtype) if need[3] else None
        dx = dg = de = None
        if need[0] or need[1] or need[2]:
            dxn = vit_ops.linear(dy1, _half_weight(w1, transpose=True))
            dx, dg, de = vit_ops.layernorm_f32_bwd(dxn, x2, gamma.detach().contiguous(),
                                                   ctx.eps)
            dx = dx.view(*dh.shape[:-1], -1) if need[0] else None
        return dx, dg, de, dw1, db1, None


class _LinearTrainFn(torch.autograd.Function):
    """nn.Linear on half rows for training: a [.., K] half -> a W^T + b, half (``b`` may be
    None); backward: bias gradient (column sum), weight gradient (``vit_ops.linear_wgrad``)
    and the data gradient as a GEMM on the transposed weight.  Gradients as in
    ``_FFHiddenFn``."""

    @staticmethod
    def forward(ctx, a, w, b):
        ctx.save_for_backward(a, w)
        return vit_ops.linear(a, _half_weight(w), _bias(b))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        a, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        db = vit_ops.colsum(dy).to(w.dtype) if need[2] else None
        dw = vit_ops.linear_wgrad(dy, a).to(w.dtype) if need[1] else None
        da = vit_ops.linear(dy, _half_weight(w, transpose=True)) if need[0] else None
        return da, dw, db


class _LoRALinearTrainFn(torch.autograd.Function):
    """An unmerged ``LoRALinear`` on half rows: y = a W^T + b + (a A^T)(s B)^T.  B A is NOT
    merged into the half weight (B starts at zero and moves by the learning rate: a delta
    below half an ulp of W would vanish from the forward); the low-rank branch runs as two
    GEMMs of its own on the rank zero-padded to 64, u = a A_pad^T [M, 64] and u (s B)_pad^T,
    added to the frozen product as half tensors.  Saved: a and u.  Backward: du = dy (s B)_pad
    (a GEMM), d(sB)_pad = dy^T u and dA_pad = du^T a by ``vit_ops.linear_wgrad``; dA and dB
    are their first r rows / columns.  The full-size weight gradient is computed only when
    ``w`` asks for one (LoRA freezes it)."""

    @staticmethod
    def forward(ctx, a, w, b, lora_a, lora_b, scaling):
        a_pad = vit_ops.to_bf16(lora_pad_a(lora_a))
        b_pad = vit_ops.to_bf16(lora_pad_b(lora_b, scaling))
        u = vit_ops.linear(a, a_pad)
        y = vit_ops.linear(a, _half_weight(w), _bias(b)) + vit_ops.linear(u, b_pad)
        ctx.scaling = scaling
        ctx.save_for_backward(a, u, w, lora_a, lora_b)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        a, u, w, lora_a, lora_b = ctx.saved_tensors
        need = ctx.needs_input_grad
        r, s = lora_a.shape[0], ctx.scaling
        dy = dy.contiguous()
        db = vit_ops.colsum(dy).to(w.dtype) if need[2] else None
        dw = vit_ops.linear_wgrad(dy, a).to(w.dtype) if need[1] else None
        da = dla = dlb = None
        if need[0] or need[3]:
            # du = dy (s B)_pad: the GEMM's weight is (s B)_pad^T [64, out]
            du = vit_ops.linear(dy, vit_ops.to_bf16(lora_pad_b(lora_b, s).t().contiguous()))
            if need[3]:
                dla = vit_ops.linear_wgrad(du, a)[:r].to(lora_a.dtype)
            if need[0]:
                da = vit_ops.linear(dy, _half_weight(w, transpose=True)) + vit_ops.linear(
                    du, vit_ops.to_bf16(lora_pad_a(lora_a).t().contiguous()))
        if need[4]:
            dlb = (vit_ops.linear_wgrad(dy, u)[:, :r] * s).to(lora_b.dtype)
        return da, dw, db, dla, dlb, None


def _pad_rows64(t):
    """fp32 [p, ...] -> fp32 [pad64(p), ...], rows p.. zero (the GEMM's and the weight
    gradient's tile width, as the LoRA rank)."""
    t = t.detach().float()
    pad = -t.shape[0] % LORA_PAD
    return F.pad(t, (0, 0) * (t.dim() - 1) + (0, pad)) if pad else t.contiguous()


class _CatFusionTrainFn(torch.autograd.Function):
    """``CatFusionLift`` for training (csrc/fusion_train.hip): fp32 NCHW maps x1, x2 ->
    relu(cat(conv1(LN1(cat(r(x1), r(x2)))), conv2(LN2(r(x2))))), r the bilinear resize to
    ``size``, as the NCHW view of fp32 channels-last rows.  The two 1x1 convs are GEMMs on
    half rows whose epilogue adds the bias and applies the ReLU; their output widths are
    zero-padded to multiples of 64 (weight rows, bias) and the padding rows of dW and db are
    dropped.

    Saved for backward: the resized fp32 rows ``rc`` and the two half GEMM outputs.  The
    normalised half rows are NOT saved: they are as large as ``rc`` again (65 MB against
    78 MB at the VEON shape) and one more ``dual_layernorm`` of ``rc`` in backward, run only
    when a conv weight asks for its gradient, rebuilds them bit for bit.  Parameter
    gradients are fp32 in the parameters' own layout, only those ``needs_input_grad`` asks
    for; an input that needs no gradient gets no adjoint launch."""

    @staticmethod
    def forward(ctx, x1, x2, g1, b1, w1, c1, g2, b2, w2, c2, size, eps1, eps2):
        x1c, x2c = x1.detach().contiguous(), x2.detach().contiguous()
        N, C1 = x1c.shape[:2]
        p1, p2 = w1.shape[0], w2.shape[0]
        rc = fusion_ops.resize_cat(x1c, x2c, size)
        xn1, xn2 = fusion_ops.dual_layernorm(
            rc, C1, g1.detach().contiguous(), b1.detach().contiguous(), eps1,
            g2.detach().contiguous(), b2.detach().contiguous(), eps2)
        y1 = vit_ops.linear(xn1, vit_ops.to_bf16(_pad_rows64(w1.view(p1, -1))),
                            _pad_rows64(c1), vit_ops.EPI_AFFINE_RELU)
        y2 = vit_ops.linear(xn2, vit_ops.to_bf16(_pad_rows64(w2.view(p2, -1))),
                            _pad_rows64(c2), vit_ops.EPI_AFFINE_RELU)
        ctx.size, ctx.eps = tuple(size), (eps1, eps2)
        ctx.shapes = (x1.shape, x2.shape)
        ctx.save_for_backward(rc, y1, y2, g1, b1, w1, g2, b2, w2)
        out = fusion_ops.join(y1, y2, p1, p2)
        return out.view(N, size[0], size[1], p1 + p2).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        rc, y1, y2, g1, b1, w1, g2, b2, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        p1, p2 = w1.shape[0], w2.shape[0]
        C = rc.shape[1]
        C1 = C - w2[0].numel()
        (eps1, eps2), size = ctx.eps, ctx.size
        g1, g2 = g1.detach().contiguous(), g2.detach().contiguous()
        # channels-last rows of the upstream gradient (no copy when it arrives that way)
        rows = dout.float().permute(0, 2, 3, 1).contiguous().view(-1, p1 + p2)
        dy1, dy2 = fusion_ops.relu_split(rows, y1, y2, p1, p2)
        dc1 = vit_ops.colsum(dy1)[:p1].to(w1.dtype) if need[5] else None
        dc2 = vit_ops.colsum(dy2)[:p2].to(w2.dtype) if need[9] else None
        dw1 = dw2 = None
        if need[4] or need[8]:
            xn1, xn2 = fusion_ops.dual_layernorm(
                rc, C1, g1, b1.detach().contiguous(), eps1, g2, b2.detach().contiguous(),
                eps2)
            if need[4]:
                dw1 = vit_ops.linear_wgrad(dy1, xn1)[:p1].view(w1.shape).to(w1.dtype)
            if need[8]:
                dw2 = vit_ops.linear_wgrad(dy2, xn2)[:p2].view(w2.shape).to(w2.dtype)
            del xn1, xn2
        dx1 = dx2 = dg1 = db1 = dg2 = db2 = None
        if need[0] or need[1] or need[2] or need[3] or need[6] or need[7]:
            # data gradients as GEMMs on the transposed padded weights [Cin][pad64(p)]
            dxn1 = vit_ops.linear(
                dy1, vit_ops.to_bf16(_pad_rows64(w1.view(p1, -1)).t().contiguous()))
            dxn2 = vit_ops.linear(
                dy2, vit_ops.to_bf16(_pad_rows64(w2.view(p2, -1)).t().contiguous()))
            drc, dg1, db1, dg2, db2 = fusion_ops.dual_layernorm_bwd(
                dxn1, dxn2, rc, C1, g1, eps1, g2, eps2)
            if need[0]:
                dx1 = fusion_ops.resize_adjoint(drc, ctx.shapes[0], size, 0)
            if need[1]:
                dx2 = fusion_ops.resize_adjoint(drc, ctx.shapes[1], size, C1)
        return (dx1, dx2, dg1 if need[2] else None, db1 if need[3] else None, dw1, dc1,
                dg2 if need[6] else None, db2 if need[7] else None, dw2, dc2, None, None,
                None)


# ------------------------------------------------- padded volumes (storage tensors)
# The differentiable values of the native training paths on volumes are the STORAGE tensors
# of PaddedVolumes (half, guard rows included), as in ``_ResBlockTrainFn``; ``shape`` is the
# (B, C, Z, Y, X) of the volume a storage tensor holds.
def _rows_linear(xs, shape, w, b):
    """1x1x1 conv as ``_LinearTrainFn`` on the rows of the padded grid -> storage.  The
    halo rows of the result hold the bias (zeros without one); the guard rows are zero."""
    guard = (xs.shape[0] - conv3d_ops.PaddedVolume.rows_of(shape)) // 2
    y = _LinearTrainFn.apply(xs[guard:xs.shape[0] - guard], w.view(w.shape[0], -1), b)
    return F.pad(y, (0, 0, guard, guard))


class _BNReLUTrainFn(torch.autograd.Function):
    """Train-mode BatchNorm3d + ReLU of a stored volume ``ys`` with a ZERO halo.  ``bias``
    is the bias of the 1x1x1 conv that produced ``ys`` WITHOUT adding it (so the halo
    stayed zero): a per-channel constant ahead of train-mode BN cancels in the output and
    has zero gradient, so it only enters the running mean (None: the conv has no bias)."""

    @staticmethod
    def forward(ctx, ys, g, b, bias, shape, bn):
        y = conv3d_ops.PaddedVolume.from_storage(ys, shape)
        B, C, Z, Y, X = shape
        n = B * Z * Y * X
        ctx.shape = tuple(shape)
        # an nn.SyncBatchNorm: the group's statistics (sync_bn.py); the choice and the
        # group are taken once, here
        ctx.sync = (sync_bn.group_of(bn),) if sync_bn.is_sync(bn) else None
        if ctx.sync is not None:
            mu, r, scale, shift = sync_bn.forward_coeffs(y, bn, ctx.sync[0], mean_offset=bias)
            a = conv3d_ops.bn_apply(y, scale, shift, relu=True)
            ctx.save_for_backward(ys, a.storage, mu, r, g, bias)
            return a.storage
        mean, var, rstd = conv3d_ops.bn_batch_stats(conv3d_ops.bn_sums(y), n, bn.eps)
        conv3d_ops.bn_update_running(
            bn, mean if bias is None else mean + bias.detach().double(), var, n)
        scale = g.detach().double() * rstd
        shift = b.detach().double() - mean * scale
        a = conv3d_ops.bn_apply(y, scale.float(), shift.float(), relu=True)
        ctx.save_for_backward(ys, a.storage, mean.float(), rstd.float(), g, bias)
        return a.storage

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        ys, as_, mu, r, g, bias = ctx.saved_tensors
        B, C, Z, Y, X = ctx.shape
        vol = conv3d_ops.PaddedVolume.from_storage
        y, a, da = vol(ys, ctx.shape), vol(as_, ctx.shape), vol(dout.contiguous(), ctx.shape)
        n = B * Z * Y * X
        if ctx.sync is not None:
            coeffs, s = sync_bn.backward_coeffs(da, a, y, mu, r, g, ctx.sync[0])
        else:
            s = conv3d_ops.bn_bwd_sums(da, a, y, mu, r)
            coeffs = conv3d_ops.bn_bwd_coefficients(s, n, g, mu, r)
        dy = conv3d_ops.bn_bwd_apply(da, a, y, *coeffs)
        return (dy.storage, s[1].to(g.dtype), s[0].to(g.dtype),
                torch.zeros_like(bias) if bias is not None and ctx.needs_input_grad[3] else None, None, None)
