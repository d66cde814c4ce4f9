"""Conv3d body of VEON's 3D alignment network -- mirror of ``ResBlock3D`` and the
``layers_3d_body`` stack of ``AlignNetOcc3D``
(mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:224-228, 363-399).

The reference builds each conv as an mmcv ``ConvModule`` (conv -> norm -> act,
bias=False, BN3d); parameter names follow that layout (``conv1.conv.weight``,
``conv1.bn.weight`` ...) so a VEON checkpoint's ``layers_3d_body.*`` keys load
unchanged.  mmcv is absent here, so this is a restatement of ConvModule's
documented order; numerics are pinned against torch's own Conv3d /
BatchNorm3d (tests/test_conv3d_gpu.py), not against reference-generated vectors.

In eval mode on a ROCm device the whole stack runs on the implicit-GEMM MFMA
kernel (csrc/conv3d.hip): the lifted (B,C,Z,Y,X) fp32 volume is packed once into
the zero-padded channels-last bf16 grid, every conv writes the next conv's
padded input, BatchNorm (eval) + ReLU + the identity add are the conv's
epilogue, and the result is unpacked once at the end.  Training and CPU tensors
take the plain PyTorch formulation (the definition of the module), unless
``ResBlock3D.hip_train`` is set: then a training-mode block on a ROCm volume trains
on the same padded grid (csrc/conv3d_train.hip: train-mode BatchNorm passes, data
gradient through the forward kernel, MFMA weight gradient).  ``_PredHead3D.hip_train``
is the same switch for the two prediction heads: their 1x1x1 convs train as GEMMs on the
rows of that grid, straight from the body's storage when both are native.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib, conv3d_ops, sync_bn, vit_ops
from .._native_cache import NativeCacheMixin
from .._train_fns import LORA_PAD, _BNReLUTrainFn, _half_weight, _rows_linear
from ... import half as _half


class ConvModule3d(NativeCacheMixin, nn.Module):
    """Conv3d -> BN3d -> ReLU with mmcv ConvModule's attribute names."""

    _native_cache = ('_hip', '_hip3', '_hip_out')

    def __init__(self, cin, cout, kernel_size=3, stride=1, padding=1, bias=False,
                 norm=True, act=True):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, kernel_size, stride, padding, bias=bias)
        self.bn = nn.BatchNorm3d(cout) if norm else None
        self.activate = nn.ReLU(inplace=True) if act else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        if self.activate is not None:
            x = self.activate(x)
        return x

    def folded(self, pack=True):
        """(packed bf16 weight, fp32 scale, fp32 shift) of conv + eval-mode BN."""
        w = conv3d_ops.pack_weight(self.conv.weight) if pack else None
        cout = self.conv.out_channels
        dev = self.conv.weight.device
        scale = torch.ones(cout, device=dev)
        shift = torch.zeros(cout, device=dev)
        if self.bn is not None:
            scale = (self.bn.weight.detach().float() /
                     torch.sqrt(self.bn.running_var.float() + self.bn.eps))
            shift = self.bn.bias.detach().float() - \
                self.bn.running_mean.float() * scale
        if self.conv.bias is not None:
            shift = shift + self.conv.bias.detach().float() * scale
        return w, scale.contiguous(), shift.contiguous()


def _pointwise(vol, cm, out_channels=None, epilogue=None):
    """1x1x1 ConvModule3d on a PaddedVolume as one GEMM over its rows (the halo
    rows get the bias/shift -- they are never unpacked)."""
    if '_hip' not in cm.__dict__ or cm.__dict__['_hip'] is None:
        conv = cm.conv
        cout = conv.out_channels
        npad = (cout + 7) // 8 * 8       # the GEMM wants N % 4 == 0, rows 16-B
        w = torch.zeros(npad, conv.in_channels, device=conv.weight.device)
        w[:cout] = conv.weight.detach().float().view(cout, -1)
        _, scale, shift = cm.folded(pack=False)
        sc = torch.ones(npad, device=w.device)
        sh = torch.zeros(npad, device=w.device)
        sc[:cout], sh[:cout] = scale, shift
        cm.__dict__['_hip'] = (w.to(_half.dtype()).contiguous(), sc, sh, npad)
    w, sc, sh, npad = cm.__dict__['_hip']
    B, C, Z, Y, X = vol.shape
    key = (B, npad, Z, Y, X, str(vol.device))
    bufs = cm.__dict__.setdefault('_hip_out', {})
    if key not in bufs:  # reused across calls: the result is consumed at once
        bufs[key] = conv3d_ops.PaddedVolume(B, npad, Z, Y, X, vol.device)
    out = bufs[key]
    epi = vit_ops.EPI_AFFINE_RELU if cm.activate is not None else vit_ops.EPI_AFFINE
    if epilogue is not None:
        assert cm.activate is None
        epi = epilogue
    vit_ops.linear(vol.rows, w, sh, epi, out=out.rows, gamma=sc)
    return out


def _stage_train(cm, xs, shape):
    """A 1x1x1 ConvModule3d (conv -> train-mode BN -> ReLU) on the storage ``xs`` of a
    PaddedVolume of ``shape`` -> (storage, shape).  The GEMM runs without the conv's bias,
    so the halo stays zero; the bias only enters the running mean (``_BNReLUTrainFn``)."""
    ys = _rows_linear(xs, shape, cm.conv.weight, None)
    oshape = (shape[0], cm.conv.out_channels) + tuple(shape[2:])
    return _BNReLUTrainFn.apply(ys, cm.bn.weight, cm.bn.bias, cm.conv.bias, oshape,
                                cm.bn), oshape


class _SigmTailFn(torch.autograd.Function):
    """The last conv of ``PredHead3DSem`` with its ``sigmoid - 0.5`` for training: one
    GEMM with the ``EPI_AFFINE_SIGM`` epilogue on the storage ``xs`` (the halo stays zero:
    sigmoid(0) - 0.5 = 0), handed over as an fp32 (B, C, z, y, x) tensor whose channel
    stride is 1 (what ``voxel_cosine`` reads without a copy).  Saved: the input and the
    stored half output f, which is all the activation's backward needs:
    d pre = d f (0.25 - f^2), fused with the pack of the channels-last gradient that
    ``voxel_cosine``'s backward returns (any other layout is made channels-last first)."""

    @staticmethod
    def forward(ctx, xs, w, shape):
        x = conv3d_ops.PaddedVolume.from_storage(xs, shape)
        B, _, Z, Y, X = shape
        f = conv3d_ops.PaddedVolume(B, w.shape[0], Z, Y, X, xs.device)
        vit_ops.linear(x.rows, _half_weight(w.view(w.shape[0], -1)), None,
                       vit_ops.EPI_AFFINE_SIGM, out=f.rows)
        ctx.shape = tuple(shape)
        ctx.save_for_backward(xs, f.storage, w)
        return conv3d_ops.unpack_cl(f).permute(0, 4, 1, 2, 3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs, fs, w = ctx.saved_tensors
        B, _, Z, Y, X = ctx.shape
        vol = conv3d_ops.PaddedVolume.from_storage
        x, f = vol(xs, ctx.shape), vol(fs, (B, w.shape[0], Z, Y, X))
        if g.dtype != torch.float32 or g.stride(1) != 1:
            g = g.float().permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        dpre = conv3d_ops.sigm_bwd_pack_cl(g, f)
        need_x, need_w = ctx.needs_input_grad[:2]
        dw = vit_ops.linear_wgrad(dpre.rows, x.rows).view_as(w).to(w.dtype) if need_w else None
        dxs = None
        if need_x:
            dx = x.like()
            vit_ops.linear(dpre.rows, _half_weight(w.view(w.shape[0], -1), transpose=True),
                           out=dx.rows)
            dxs = dx.storage
        return dxs, dw, None


class _PredHead3D(nn.Module):
    """Shared machinery of the two prediction heads: a chain of 1x1x1
    ConvModules.  On a PaddedVolume (or a ROCm fp32 volume at inference) the
    chain runs as GEMMs on the channels-last rows.

    ``hip_train`` (class attribute, default False): opt-in native TRAINING path, as on
    ``ResBlock3D``.  When set, a training-mode head with grad enabled whose widths the
    kernels support runs its chain under autograd on the storage tensor of a PaddedVolume
    (``_rows_linear`` + ``_BNReLUTrainFn`` per conv -> BN -> ReLU stage); its input is a
    ROCm fp32 volume, which it packs, or the ``(storage, shape)`` pair that
    ``run_blocks(..., return_storage=True)`` hands over.  Parameter gradients are fp32 in
    the parameters' own layout.  Anything else takes the torch definition.  Hooks on the
    ConvModules do not fire on the native path."""

    _names = ()
    hip_train = False
    # whether ``_train_native`` zero-pads a last conv narrower than 64 outputs to 64 rows
    # (PredHead3DOcc); a head that does not needs every output width a multiple of 64
    _pads_narrow_tail = False

    def _chain(self):
        return [getattr(self, n) for n in self._names]

    def _train_structure_ok(self):
        """The part of ``_hip_train_ok`` that depends on the module alone: 1x1x1 stride-1
        fp32 convs, every GEMM width a multiple of 64 (in a head that pads it,
        ``_pads_narrow_tail``, a last conv without BN may have at most 8 outputs instead:
        it is zero-padded to 64 rows), BN in training mode with affine
        parameters and running statistics at a width the sums kernel supports."""
        chain = self._chain()
        for cm in chain:
            c = cm.conv
            if c.kernel_size != (1, 1, 1) or c.stride != (1, 1, 1) or c.padding != (0, 0, 0) \
                    or c.weight.dtype != torch.float32 or c.in_channels % 64:
                return False
            if cm.bn is None:
                if cm is not chain[-1] or cm.activate is not None or c.bias is not None:
                    return False
                if c.out_channels % 64 and not (self._pads_narrow_tail
                                                and c.out_channels <= 8):
                    return False
                continue
            bn = cm.bn
            if c.out_channels % 64 or cm.activate is None or not (
                    bn.training and bn.affine and bn.track_running_stats
                    and bn.running_mean is not None):
                return False
            if _lib.lib().veon_bn3d_sums_workspace_bytes(c.out_channels) < 0:
                return False
        return True

    def _hip_train_ok(self, x):
        """The native training path's own test: the switch, training mode, grad enabled,
        a ROCm fp32 volume or a (storage, shape) pair, and ``_train_structure_ok``."""
        if not (self.hip_train and self.training and torch.is_grad_enabled()):
            return False
        if isinstance(x, tuple):
            xs = x[0]
            ok = torch.is_tensor(xs) and xs.is_cuda and xs.dim() == 2 and xs.dtype == _half.dtype()
        else:
            ok = torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5
        return bool(ok) and self._train_structure_ok()

    @staticmethod
    def _train_input(x):
        """-> (storage, shape) of the head's input: handed over, or packed here."""
        if isinstance(x, tuple):
            return x[0], tuple(int(v) for v in x[1])
        return _PackFn.apply(x), tuple(x.shape)

    @staticmethod
    def _torch_input(x):
        return _UnpackFn.apply(*x) if isinstance(x, tuple) else x

    def _hip_ok(self, x):
        if not all(cm.conv.in_channels % 64 == 0 for cm in self._chain()):
            return False
        if isinstance(x, conv3d_ops.PaddedVolume):
            return True
        return x.is_cuda and not self.training and not torch.is_grad_enabled()

    def _run(self, x, return_volume=False, last_epilogue=None):
        """``last_epilogue``: GEMM epilogue of the LAST conv on the native path (the
        caller's output activation fused in); ignored by the PyTorch path."""
        if not self._hip_ok(x):
            if isinstance(x, conv3d_ops.PaddedVolume):
                x = conv3d_ops.unpack(x)
            for cm in self._chain():
                x = cm(x)
            return x
        vol = x if isinstance(x, conv3d_ops.PaddedVolume) else conv3d_ops.pack(x)
        chain = self._chain()
        for cm in chain:
            vol = _pointwise(vol, cm, epilogue=last_epilogue if cm is chain[-1] else None)
        if return_volume:
            return vol
        out = conv3d_ops.unpack(vol)
        return out[:, :self._chain()[-1].conv.out_channels]


class PredHead3DOcc(_PredHead3D):
    """Binary occupancy head (align_net_occ3d.py:431-470): 1x1x1 conv C -> C/4,
    BN, ReLU; 1x1x1 conv C/4 -> channels_out."""

    _names = ('occ_conv1', 'occ_conv2')
    _pads_narrow_tail = True

    def __init__(self, channels_in, channels_out, stride=1, use_checkpoint=False):
        super().__init__()
        mid = channels_in // 4
        self.occ_conv1 = ConvModule3d(channels_in, mid, 1, stride, 0, bias=False,
                                      norm=True, act=True)
        self.occ_conv2 = ConvModule3d(mid, channels_out, 1, stride, 0, bias=False,
                                      norm=False, act=False)
        self.use_checkpoint = use_checkpoint

    def forward(self, x):
        if self._hip_train_ok(x):
            return self._train_native(*self._train_input(x))
        return self._run(self._torch_input(x))

    def _train_native(self, xs, shape):
        """The last conv's weight is zero-padded to 64 output rows (as the LoRA branches pad
        their rank; autograd returns the parameter's rows of the padded gradient); its
        first 8 channels leave through the ordinary unpack of an 8-channel volume."""
        a, s1 = _stage_train(self.occ_conv1, xs, shape)
        w = self.occ_conv2.conv.weight
        cout = w.shape[0]
        if cout % 64:
            w = F.pad(w.view(cout, -1), (0, 0, 0, LORA_PAD - cout))
        ys = _rows_linear(a, s1, w, None)
        if cout % 64 == 0:
            return _UnpackFn.apply(ys, (s1[0], cout) + tuple(s1[2:]))
        out = _UnpackFn.apply(ys[:, :8].contiguous(), (s1[0], 8) + tuple(s1[2:]))
        return out[:, :cout]


class PredHead3DSem(_PredHead3D):
    """Feature head (align_net_occ3d.py:473-534): three 1x1x1 convs (BN+ReLU
    after the first two, the first with a conv bias), then sigmoid - 0.5."""

    _names = ('occ_conv1', 'occ_conv2', 'occ_conv3')

    def __init__(self, channels_in, channels_out, stride=1, use_checkpoint=False):
        super().__init__()
        self.occ_conv1 = ConvModule3d(channels_in, channels_in, 1, stride, 0,
                                      bias=True, norm=True, act=True)
        self.occ_conv2 = ConvModule3d(channels_in, channels_in, 1, stride, 0,
                                      bias=False, norm=True, act=True)
        self.occ_conv3 = ConvModule3d(channels_in, channels_out, 1, stride, 0,
                                      bias=False, norm=False, act=False)
        self.use_checkpoint = use_checkpoint

    def forward(self, x, return_volume=False):
        """``return_volume`` (MFMA path only): keep the result -- sigmoid - 0.5
        applied in place on the bf16 rows -- as the PaddedVolume that
        ``semantic_inference_3d_fused`` consumes."""
        if not return_volume and self._hip_train_ok(x):
            xs, shape = self._train_input(x)
            xs, shape = _stage_train(self.occ_conv1, xs, shape)
            xs, shape = _stage_train(self.occ_conv2, xs, shape)
            return _SigmTailFn.apply(xs, self.occ_conv3.conv.weight, shape)
        x = self._torch_input(x)
        if return_volume and self._hip_ok(x):
            # sigmoid(x) - 0.5 = tanh(x/2)/2 in the last GEMM's epilogue (fp32, before
            # the bf16 rounding; halo rows are never read)
            return self._run(x, True, last_epilogue=vit_ops.EPI_AFFINE_SIGM)
        out = self._run(x, return_volume)
        if isinstance(out, conv3d_ops.PaddedVolume):
            out.rows.mul_(0.5).tanh_().mul_(0.5)
            return out
        return out.sigmoid() - 0.5


def semantic_inference_3d(ov_classifier_weight, feat_occ, occ_size):
    """The reference's order (san_in_veon_temporal.py:196-201, 257-259):
    trilinear-upsample the C-channel feature volume to ``occ_size``, then
    ``einsum('qc,bczhw->bqzhw')`` with the open-vocabulary classifier."""
    feat = nn.functional.interpolate(feat_occ, size=tuple(occ_size), mode='trilinear',
                                     align_corners=False)
    return torch.einsum('qc,bczhw->bqzhw', ov_classifier_weight, feat)


def classifier_logits_low(ov_classifier_weight, feat_occ):
    """Class logits at the head's resolution: (B,Q,z,y,x) fp32 -- for a PaddedVolume
    (``PredHead3DSem(..., return_volume=True)``) a strided view of the GEMM's
    channels-last rows (MFMA, fp32 logits), otherwise the einsum."""
    W = ov_classifier_weight
    Q, C = W.shape
    if isinstance(feat_occ, conv3d_ops.PaddedVolume):
        vol = feat_occ
        B, Cv, Z, Y, X = vol.shape
        assert Cv >= C
        qp = (Q + 7) // 8 * 8
        wp = torch.zeros(qp, Cv, device=W.device)
        wp[:Q, :C] = W.detach().float()
        if Cv % 64 == 0:
            logits = torch.zeros(vol.M, qp, dtype=torch.float32, device=W.device)
            vit_ops.linear_residual_(logits, vol.rows, wp.to(_half.dtype()).contiguous())
        else:   # a K the MFMA tile does not divide (toy widths): rocBLAS, same operands
            logits = vol.rows.float() @ wp.to(_half.dtype()).float().t()
        return logits.view(B, Z + 2, Y + 2, X + 2, qp)[:, 1:-1, 1:-1, 1:-1, :Q] \
            .permute(0, 4, 1, 2, 3)
    return torch.einsum('qc,bczhw->bqzhw', W, feat_occ)


def semantic_inference_3d_fused(ov_classifier_weight, feat_occ, occ_size):
    """Same logits with the two linear maps swapped: classify at the head's
    resolution (one GEMM over the voxels: C -> Q classes), then upsample Q
    channels instead of C (768 -> ~20: the 2 GB upsampled feature volume of the
    reference is never formed).  Interpolation weights are per-channel and sum
    to one, the classifier is per-voxel linear, so the results agree up to
    rounding.  ``feat_occ``: (B,C,Z,Y,X) tensor or the PaddedVolume of
    ``PredHead3DSem(..., return_volume=True)`` (GEMM on MFMA, fp32 logits)."""
    low = classifier_logits_low(ov_classifier_weight, feat_occ)
    return nn.functional.interpolate(low, size=tuple(occ_size), mode='trilinear',
                                     align_corners=False)


def _bn_sync(bn):
    """None for a plain BatchNorm; for an nn.SyncBatchNorm the 1-tuple of its process group
    (``(None,)``: no group, no collective).  Taken once in forward and kept on ``ctx``."""
    return (sync_bn.group_of(bn),) if sync_bn.is_sync(bn) else None


def _bn_train_native(y, bn, sync=None):
    """Batch statistics of the stored conv output ``y`` (PaddedVolume), the update of
    ``bn``'s buffers, and the fp32 (scale, shift) of the apply pass.  ``sync``
    (``_bn_sync``): the statistics of the whole group (veon_amd/sync_bn.py)."""
    if sync is not None:
        return sync_bn.forward_coeffs(y, bn, sync[0])
    B, C, Z, Y, X = y.shape
    n = B * Z * Y * X
    mean, var, rstd = conv3d_ops.bn_batch_stats(conv3d_ops.bn_sums(y), n, bn.eps)
    conv3d_ops.bn_update_running(bn, mean, var, n)
    scale = bn.weight.detach().double() * rstd
    shift = bn.bias.detach().double() - mean * scale
    return mean.float(), rstd.float(), scale.float(), shift.float()


def _bn_bwd_native(da, a, y, mu, r, g, n, sync=None):
    """The backward sums of one BN and the vectors of ``bn_bwd_apply``: -> (fp32 (2, C)
    LOCAL sums (dbeta, dgamma), (ca, cb, cc)); with ``sync`` the coefficients come from the
    group's sums and total count."""
    if sync is not None:
        coeffs, s = sync_bn.backward_coeffs(da, a, y, mu, r, g, sync[0])
        return s, coeffs
    s = conv3d_ops.bn_bwd_sums(da, a, y, mu, r)
    return s, conv3d_ops.bn_bwd_coefficients(s, n, g, mu, r)


class _ResBlockTrainFn(torch.autograd.Function):
    """One training step of ``ResBlock3D`` on padded rows (csrc/conv3d_train.hip).  The
    differentiable input and output are the STORAGE tensors of PaddedVolumes (half,
    guard rows included), so consecutive blocks chain without leaving the layout; the
    gradient between blocks is a padded half volume too.  Saved per conv: its input, its
    stored output y, mean and rstd; the ReLU masks are read from the stored activations
    (5 padded volumes per block: x, y1, a1, y2, out)."""

    @staticmethod
    def forward(ctx, xs, w1, g1, b1, w2, g2, b2, shape, blk):
        half = _half.dtype()
        x = conv3d_ops.PaddedVolume.from_storage(xs, shape)
        # the half copies of the weights are re-packed from the fp32 parameters every step
        y1 = conv3d_ops.conv3d_k3(x, conv3d_ops.pack_weight(w1))
        ctx.sync1, ctx.sync2 = _bn_sync(blk.conv1.bn), _bn_sync(blk.conv2.bn)
        mu1, r1, sc1, sh1 = _bn_train_native(y1, blk.conv1.bn, ctx.sync1)
        a1 = conv3d_ops.bn_apply(y1, sc1, sh1, relu=True)
        y2 = conv3d_ops.conv3d_k3(a1, conv3d_ops.pack_weight(w2))
        mu2, r2, sc2, sh2 = _bn_train_native(y2, blk.conv2.bn, ctx.sync2)
        out = conv3d_ops.bn_apply(y2, sc2, sh2, ident=x, relu=True)
        ctx.shape = tuple(shape)
        ctx.half = half
        ctx.save_for_backward(xs, y1.storage, a1.storage, y2.storage, out.storage,
                              mu1, r1, mu2, r2, w1, g1, w2, g2)
        return out.storage

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xs, y1s, a1s, y2s, outs, mu1, r1, mu2, r2, w1, g1, w2, g2 = ctx.saved_tensors
        vol = lambda t: conv3d_ops.PaddedVolume.from_storage(t, ctx.shape)  # noqa: E731
        x, y1, a1, y2, out = vol(xs), vol(y1s), vol(a1s), vol(y2s), vol(outs)
        da = vol(dout.contiguous())
        B, C, Z, Y, X = ctx.shape
        n = B * Z * Y * X
        need_x, need_w1, need_w2 = (ctx.needs_input_grad[i] for i in (0, 1, 4))
        # conv2: BN + identity + ReLU backwards, then its two gradients; dz2 (the identity
        # branch's gradient) is stored only when the block's input needs a gradient
        s2, coeffs2 = _bn_bwd_native(da, out, y2, mu2, r2, g2, n, ctx.sync2)
        dy2 = conv3d_ops.bn_bwd_apply(da, out, y2, *coeffs2, want_dz=need_x)
        dz2 = None
        if need_x:
            dy2, dz2 = dy2
        dw2 = conv3d_ops.conv3d_k3_wgrad(dy2, a1) if need_w2 else None
        da1 = conv3d_ops.conv3d_k3(dy2, conv3d_ops.pack_weight_dgrad(w2).to(ctx.half))
        # conv1: BN + ReLU backwards
        s1, coeffs1 = _bn_bwd_native(da1, a1, y1, mu1, r1, g1, n, ctx.sync1)
        dy1 = conv3d_ops.bn_bwd_apply(da1, a1, y1, *coeffs1)
        dw1 = conv3d_ops.conv3d_k3_wgrad(dy1, x) if need_w1 else None
        dxs = None
        if need_x:
            # dx = conv(dy1, flip(w1)) + dz2 (identity branch) as the conv's residual
            dxs = conv3d_ops.conv3d_k3(dy1, conv3d_ops.pack_weight_dgrad(w1).to(ctx.half),
                                       resid=dz2).storage
        wgrad = conv3d_ops.wgrad_to_param
        return (dxs, wgrad(dw1, w1), s1[1].to(g1.dtype), s1[0].to(g1.dtype),
                wgrad(dw2, w2), s2[1].to(g2.dtype), s2[0].to(g2.dtype), None, None)


class _ConvModuleTrainFn(torch.autograd.Function):
    """One training step of a ``ConvModule3d`` (3x3x3 conv -> train-mode BN -> ReLU) on
    padded rows: the single-conv sibling of ``_ResBlockTrainFn`` (no identity), built from
    the same ``conv3d_ops`` calls, storage tensors in and out.  Cin and Cout may differ.
    Saved: the input, the stored conv output y, the activation, mean and rstd.  No data
    gradient is computed for an input that needs none (a past frame)."""

    @staticmethod
    def forward(ctx, xs, w, g, b, shape, cm):
        x = conv3d_ops.PaddedVolume.from_storage(xs, shape)
        y = conv3d_ops.conv3d_k3(x, conv3d_ops.pack_weight(w))
        ctx.sync = _bn_sync(cm.bn)
        mu, r, sc, sh = _bn_train_native(y, cm.bn, ctx.sync)
        a = conv3d_ops.bn_apply(y, sc, sh, relu=True)
        ctx.shape, ctx.half = tuple(shape), _half.dtype()
        ctx.save_for_backward(xs, y.storage, a.storage, mu, r, w, g)
        return a.storage

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xs, ys, as_, mu, r, w, g = ctx.saved_tensors
        B, _, Z, Y, X = ctx.shape
        oshape = (B, w.shape[0], Z, Y, X)
        vol = conv3d_ops.PaddedVolume.from_storage
        x, y, a = vol(xs, ctx.shape), vol(ys, oshape), vol(as_, oshape)
        da = vol(dout.contiguous(), oshape)
        n = B * Z * Y * X
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        s, coeffs = _bn_bwd_native(da, a, y, mu, r, g, n, ctx.sync)
        dy = conv3d_ops.bn_bwd_apply(da, a, y, *coeffs)
        dw = conv3d_ops.conv3d_k3_wgrad(dy, x) if need_w else None
        dxs = None
        if need_x:
            dxs = conv3d_ops.conv3d_k3(dy, conv3d_ops.pack_weight_dgrad(w).to(ctx.half)).storage
        return (dxs, conv3d_ops.wgrad_to_param(dw, w), s[1].to(g.dtype), s[0].to(g.dtype),
                None, None)


def conv_module_train_ok(cm):
    """Whether ``_ConvModuleTrainFn`` can run the ConvModule3d ``cm`` (3x3x3, stride 1, no
    conv bias, train-mode BN with buffers, ReLU, widths the weight gradient supports)."""
    c = cm.conv
    return (c.kernel_size == (3, 3, 3) and c.stride == (1, 1, 1) and c.padding == (1, 1, 1)
            and c.bias is None and c.weight.dtype == torch.float32
            and conv3d_ops.wgrad_supported(c.in_channels, c.out_channels)
            and cm.bn is not None and cm.bn.training and cm.bn.affine
            and cm.bn.track_running_stats and cm.activate is not None)


def conv_module_train(cm, xs, shape):
    """``cm`` on the storage ``xs`` of a PaddedVolume of ``shape`` -> (storage, shape)."""
    out = _ConvModuleTrainFn.apply(xs, cm.conv.weight, cm.bn.weight, cm.bn.bias,
                                   tuple(shape), cm)
    return out, (shape[0], cm.conv.out_channels) + tuple(shape[2:])


class _PackFn(torch.autograd.Function):
    """(B,C,Z,Y,X) fp32 -> storage of its PaddedVolume; backwards the unpack."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        return conv3d_ops.pack(x).storage

    @staticmethod
    def backward(ctx, g):
        return conv3d_ops.unpack(conv3d_ops.PaddedVolume.from_storage(g.contiguous(),
                                                                      ctx.shape))


class _UnpackFn(torch.autograd.Function):
    """storage of a PaddedVolume -> (B,C,Z,Y,X) fp32; backwards the pack."""

    @staticmethod
    def forward(ctx, xs, shape):
        ctx.shape = tuple(shape)
        return conv3d_ops.unpack(conv3d_ops.PaddedVolume.from_storage(xs, shape))

    @staticmethod
    def backward(ctx, g):
        return conv3d_ops.pack(g).storage, None


def run_blocks(blocks, x, return_storage=False):
    """``blocks`` (ResBlock3D) applied in order to the fp32 volume ``x``.  A run of
    consecutive blocks that take the native training path (``ResBlock3D.hip_train``) is
    packed once and unpacked once; every other block is called as it is.
    ``return_storage``: when the LAST block belongs to a native run, that run is not
    unpacked and the result is the pair ``(storage, shape)`` of its PaddedVolume (what the
    prediction heads' native training path takes); otherwise the fp32 volume as usual."""
    blocks = list(blocks)
    i = 0
    while i < len(blocks):
        if not blocks[i]._hip_train_ok(x):
            x = blocks[i](x)
            i += 1
            continue
        shape = tuple(x.shape)
        xs = _PackFn.apply(x)
        while i < len(blocks) and blocks[i]._hip_train_ok(x):
            xs = blocks[i]._train_native(xs, shape)
            i += 1
        if return_storage and i == len(blocks):
            return xs, shape
        x = _UnpackFn.apply(xs, shape)
    return x


def run_blocks_into_heads(blocks, x, heads):
    """The LAST run of a decoder's blocks ahead of its prediction ``heads``: when every
    head takes its native training path on ``x``, a trailing run of native blocks hands its
    storage over (``run_blocks(..., return_storage=True)``: no unpack -> pack pair, one
    saved input for all heads); otherwise ``run_blocks`` as it is."""
    to_heads = torch.is_tensor(x) and all(h._hip_train_ok(x) for h in heads)
    return run_blocks(blocks, x, return_storage=to_heads)


class ResBlock3D(nn.Module):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + x) (align_net_occ3d.py:363-399;
    ``stride`` / ``downsample`` as the reference, unused by VEON).

    ``hip_train`` (class attribute, default False): opt-in native TRAINING path.  When
    set, a training-mode block on a ROCm fp32 tensor whose widths the kernels support
    runs ``_ResBlockTrainFn`` (train-mode BatchNorm with batch statistics, MFMA convs,
    data and weight gradients in HIP); anything else takes the torch definition.
    As on the inference fast path, the native path does not go through the
    ``__call__`` of ``conv1`` / ``conv2`` (nor, inside a run of ``run_blocks``, of the
    block): forward and backward hooks registered on them do not fire."""

    hip_train = False

    def __init__(self, channels_in, channels_out, stride=1, downsample=None,
                 use_checkpoint=False):
        super().__init__()
        self.conv1 = ConvModule3d(channels_in, channels_out, 3, stride, 1,
                                  bias=False, norm=True, act=True)
        self.conv2 = ConvModule3d(channels_out, channels_out, 3, 1, 1,
                                  bias=False, norm=True, act=False)
        self.downsample = downsample
        self.relu = nn.ReLU(inplace=True)
        self.use_checkpoint = use_checkpoint

    def forward(self, x):
        if self._hip_train_ok(x):
            return run_blocks([self], x)
        identity = x if self.downsample is None else self.downsample(x)
        x = self.conv2(self.conv1(x))
        return self.relu(x + identity)

    def _hip_train_ok(self, x):
        """The native training path's own test: the switch, training mode, a ROCm fp32
        volume, the inference path's structure test and the weight gradient's widths
        (both multiples of 64: stricter than ``hip_supported``), BN with buffers."""
        if not (self.hip_train and self.training and torch.is_tensor(x) and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 5):
            return False
        return self._train_structure_ok()

    def _train_structure_ok(self):
        """The part of ``_hip_train_ok`` that depends on the module alone (an
        nn.SyncBatchNorm in place of the BatchNorm3d passes it: sync_bn.py)."""
        if not self.hip_supported():
            return False
        c1, c2 = self.conv1, self.conv2
        return (conv3d_ops.wgrad_supported(c1.conv.in_channels, c1.conv.out_channels)
                and conv3d_ops.wgrad_supported(c2.conv.in_channels, c2.conv.out_channels)
                and all(cm.bn is not None and cm.bn.training and cm.bn.affine
                        and cm.bn.track_running_stats and cm.conv.bias is None
                        and cm.conv.weight.dtype == torch.float32 for cm in (c1, c2)))

    def _train_native(self, xs, shape):
        c1, c2 = self.conv1, self.conv2
        return _ResBlockTrainFn.apply(xs, c1.conv.weight, c1.bn.weight, c1.bn.bias,
                                      c2.conv.weight, c2.bn.weight, c2.bn.bias, shape, self)

    def hip_supported(self):
        c1, c2 = self.conv1.conv, self.conv2.conv
        return (self.downsample is None and c1.stride == (1, 1, 1)
                and c1.in_channels == c1.out_channels
                and c1.in_channels % 64 == 0 and c2.out_channels % 8 == 0)


class AlignBody3D(NativeCacheMixin, nn.Module):
    """``layers_3d_body``: ``layer_depth`` ResBlock3D on the lifted volume
    (align_net_occ3d.py:224-228; applied one block per fusion step in
    ``forward`` :252-264 -- ``forward`` here runs blocks ``[start, stop)``)."""

    # ``_bufs`` holds scratch volumes keyed by shape and device, not weights: it stays
    _native_cache = {'_hip': None}

    def __init__(self, embed_dim=256, layer_depth=4):
        super().__init__()
        self.layers_3d_body = nn.ModuleList(
            [ResBlock3D(embed_dim, embed_dim) for _ in range(layer_depth)])
        self.use_hip = True
        self._hip = None     # folded weights per block
        self._bufs = {}      # (shape, device) -> three PaddedVolumes

    def _use_hip(self, x):
        return (self.use_hip and x.is_cuda and not self.training
                and not torch.is_grad_enabled()
                and all(b.hip_supported() for b in self.layers_3d_body))

    def _volumes(self, shape, device):
        key = (tuple(shape), str(device))
        if key not in self._bufs:
            B, C, Z, Y, X = shape
            self._bufs[key] = [conv3d_ops.PaddedVolume(B, C, Z, Y, X, device)
                               for _ in range(3)]
        return self._bufs[key]

    def forward(self, x, start=0, stop=None, return_volume=False):
        """``return_volume``: hand the result over as the PaddedVolume the
        prediction heads consume directly (no unpack / re-pack)."""
        blocks = list(self.layers_3d_body)[start:stop]
        from_volume = isinstance(x, conv3d_ops.PaddedVolume)
        if from_volume and not (self.use_hip and not self.training
                                and all(b.hip_supported() for b in blocks)):
            x, from_volume = conv3d_ops.unpack(x), False
        if not from_volume and not self._use_hip(x):
            # torch definition, or (ResBlock3D.hip_train) the native training path with
            # one pack and one unpack around each run of native blocks
            return run_blocks(blocks, x)
        if self._hip is None:
            self._hip = [(b.conv1.folded(), b.conv2.folded())
                         for b in self.layers_3d_body]
        folded = self._hip[start:stop]
        internal = list(self._volumes(x.shape, x.device))
        external = None
        if from_volume:   # e.g. written by the lift's fused max-pool kernel
            src = x
            if not any(x is b for b in internal):
                external = x               # read only, never overwritten
        else:
            src = internal[0]
            conv3d_ops.pack(x, out=src)
        pool = [b for b in internal if b is not src]
        for (w1, s1, b1), (w2, s2, b2) in folded:
            tmp, dst = pool[0], pool[1]
            conv3d_ops.conv3d_k3(src, w1, s1, b1, relu=True, out=tmp)
            conv3d_ops.conv3d_k3(tmp, w2, s2, b2, resid=src, relu=True, out=dst)
            pool = [tmp] + pool[2:] + ([src] if src is not external else [])
            src = dst
        a = src
        return a if return_volume else conv3d_ops.unpack(a)
