"""The differentiable primitive of VEON's 2D->3D feature-alignment loss
(``Proj2Dto3DLoss``, models/semantic_net/loss/occ_loss_utils/occ3d_nuscenes.py:454-461,
497-504): the cosine between the trilinearly upsampled feature at a voxel and a row of
the class-embedding table, for a flat list of entries ``(voxel_i, label_i)``.

The reference upsamples ``feat_occ`` to (B, C, 16, 200, 200) fp32 (1.31 GB at C = 512,
san_in_veon_temporal.py:196-200), copies it once more when it reshapes the permuted view
(occ3d_nuscenes.py:372-373) and autograd keeps a gradient of that size for each, for a
loss that reads the feature at a few percent of the voxels.  On a ROCm device
``voxel_cosine`` is native in both directions (csrc/occ_align_loss.hip) and reads and
writes the LOW-resolution volume only; on CPU it runs the reference sequence in torch
(upsample, gather, cosine), which is the CPU tests' oracle."""
import torch
import torch.nn.functional as F

from . import _lib


def _check_args(feat_low, voxels, labels, table, occ_size, eps, batch):
    if not isinstance(feat_low, torch.Tensor) or feat_low.dim() != 5:
        raise ValueError('feat_low must be a (B, C, z, y, x) tensor')
    if not feat_low.is_floating_point():
        raise ValueError('feat_low must be a floating-point tensor')
    if table.dim() != 2 or table.shape[1] != feat_low.shape[1]:
        raise ValueError('table must be (K, C) with C = %d channels' % feat_low.shape[1])
    if table.shape[0] < 1:
        raise ValueError('table has no rows')
    if table.requires_grad:
        raise ValueError('voxel_cosine gives the table no gradient: pass table.detach()')
    if voxels.dim() != 2 or voxels.shape[1] != 3:
        raise ValueError('voxels must be (N, 3) (x, y, z)')
    if labels.dim() != 1 or labels.shape[0] != voxels.shape[0]:
        raise ValueError('labels must be (N,)')
    if voxels.is_floating_point() or labels.is_floating_point():
        raise ValueError('voxels and labels must be integer tensors')
    if len(occ_size) != 3 or min(int(v) for v in occ_size) < 1:
        raise ValueError('occ_size must be (Z, Y, X)')
    if not 0 <= batch < feat_low.shape[0]:
        raise ValueError('batch %d outside [0, %d)' % (batch, feat_low.shape[0]))
    if not eps > 0:
        raise ValueError('eps must be positive')
    for t in (voxels, labels, table):
        if t.device != feat_low.device:
            raise ValueError('tensors on different devices: %s vs %s' % (t.device,
                                                                         feat_low.device))
    if voxels.shape[0]:
        # a loss must not train on garbage: one reduction and one read-back (the only
        # host synchronisation of the forward)
        Zo, Yo, Xo = (int(v) for v in occ_size)
        hi = torch.tensor([Xo, Yo, Zo], device=voxels.device)
        bad = ((voxels < 0) | (voxels >= hi)).any() | (labels < 0).any() | \
            (labels >= table.shape[0]).any()
        if bool(bad):
            raise ValueError('a voxel lies outside the grid %s or a label outside [0, %d)'
                             % ((Zo, Yo, Xo), table.shape[0]))


def _reference(feat_low, voxels, labels, table, occ_size, eps, batch):
    """The reference sequence in torch: upsample, gather, cosine (differentiable with
    respect to ``feat_low`` through autograd)."""
    size = tuple(int(v) for v in occ_size)
    v = voxels.long()
    f_up = F.interpolate(feat_low[batch:batch + 1], size, mode='trilinear',
                         align_corners=False)[0]
    f = f_up[:, v[:, 2], v[:, 1], v[:, 0]].T                      # (N, C)
    t = table.to(f.dtype)[labels.long()]                           # (N, C)
    return F.cosine_similarity(f, t, dim=1, eps=eps)


class _VoxelCosine(torch.autograd.Function):
    """The native pair veon_occ_align_fwd / veon_occ_align_bwd."""

    @staticmethod
    def forward(ctx, feat_low, voxels, labels, table, occ_size, eps, batch):
        dev = _lib.require_device(feat_low, voxels, labels, table)
        B, C, zi, yi, xi = feat_low.shape
        Zo, Yo, Xo = occ_size
        K, N = table.shape[0], voxels.shape[0]
        vox = voxels.to(torch.int32).contiguous()
        lab = labels.to(torch.int32).contiguous()
        tab = table.detach().to(torch.float32).contiguous()
        feat = feat_low.detach()
        if feat.stride(1) != 1 and C % 4 == 0 and C >= 64:
            # the torch heads' NCDHW tensor: one channels-last copy of this sample
            # (C z y x 4 bytes) for the kernels' vector path costs a fraction of what the
            # any-stride path's scattered 4-byte loads do at these widths
            feat = feat[batch:batch + 1].permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        kb = batch if feat.shape[0] == B else 0           # the sample's index in ``feat``
        cos = torch.empty((N,), dtype=torch.float32, device=dev)
        stats = torch.empty((N, 2), dtype=torch.float32, device=dev)
        tnorm = torch.empty((K,), dtype=torch.float32, device=dev)
        _lib.launch('veon_occ_align_fwd', dev, feat, _lib.strides(feat), C, feat.shape[0], zi, yi,
                    xi, Zo, Yo, Xo, vox, lab, N, kb, tab, K, eps, tnorm, cos, stats)
        ctx.save_for_backward(feat, vox, lab, tab, tnorm, stats)
        ctx.occ_size, ctx.eps, ctx.batch, ctx.kb, ctx.B = occ_size, eps, batch, kb, B
        return cos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        feat, vox, lab, tab, tnorm, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        B, (C, zi, yi, xi) = ctx.B, feat.shape[1:]
        Zo, Yo, Xo = ctx.occ_size
        if (Zo, Yo, Xo) != (2 * zi, 2 * yi, 2 * xi):
            # the native backward's inverted index is the 2x stencil: any other scale
            # goes through the torch sequence (and forms the upsampled volume)
            with torch.enable_grad():
                leaf = feat.clone().requires_grad_(True)
                cos = _reference(leaf, vox, lab, tab, ctx.occ_size, ctx.eps, ctx.kb)
                grad, = torch.autograd.grad(cos, leaf, g.to(cos.dtype))
            if grad.shape[0] != B:
                full = grad.new_zeros((B, C, zi, yi, xi))
                full[ctx.batch] = grad[ctx.kb]
                grad = full
            return (grad,) + (None,) * 6
        dev = feat.device
        N, K = vox.shape[0], tab.shape[0]
        # channels-last rows are what the kernel stores; autograd takes any strides
        buf = torch.empty((B, zi, yi, xi, C), dtype=torch.float32, device=dev)
        if B > 1:
            buf[:ctx.batch].zero_()
            buf[ctx.batch + 1:].zero_()
        g = g.to(torch.float32).contiguous()
        occ_rows = torch.full((Zo * Yo * Xo,), -1, dtype=torch.int32, device=dev)
        order = seg = rows = None
        M = 0
        if N:
            # entries grouped by output voxel, in entry order within a voxel (a stable
            # sort); the number of distinct voxels sizes the workspace: one read-back
            v = vox.long()
            keys = (v[:, 2] * Yo + v[:, 1]) * Xo + v[:, 0]
            keys, order = torch.sort(keys, stable=True)
            uniq, counts = torch.unique_consecutive(keys, return_counts=True)
            M = uniq.shape[0]
            seg = torch.zeros((M + 1,), dtype=torch.int32, device=dev)
            seg[1:] = torch.cumsum(counts, 0)
            occ_rows[uniq] = torch.arange(M, dtype=torch.int32, device=dev)
            order = order.to(torch.int32)
            rows = torch.empty((M, C), dtype=torch.float32, device=dev)
        _lib.launch('veon_occ_align_bwd', dev, feat, _lib.strides(feat), C, feat.shape[0], zi, yi, xi,
                    vox, lab, N, ctx.kb, tab, K, ctx.eps, tnorm, stats, g, order, seg, M, occ_rows,
                    rows, buf[ctx.batch])
        return (buf.permute(0, 4, 1, 2, 3),) + (None,) * 6


def voxel_cosine(feat_low, voxels, labels, table, occ_size, eps=1e-6, batch=0):
    """cos_i between the upsampled feature at ``voxels[i]`` and ``table[labels[i]]``.

    feat_low: (B, C, z, y, x), any strides, may require grad (a tensor whose channel
    stride is not 1, with C % 4 == 0 and C >= 64, is copied to channels-last once per
    call, sample ``batch`` only, for the kernels' vector path).  voxels: (N, 3) integer
    (x, y, z) in ``occ_size`` = (Z, Y, X), the convention of ``retrieve_points``, all of
    sample ``batch``, in any order, repeats allowed.  labels: (N,) integer rows of
    ``table`` (K, C), which gets no gradient (one that requires grad is refused).

        cos_i = <f_i, t_i> / (max(|f_i|, eps) * max(|t_i|, eps)),
        f_i = trilinear(feat_low[batch], align_corners=False)[voxel_i], t_i = table[labels_i]

    i.e. ``nn.CosineSimilarity(dim=1, eps=eps)``: each norm is clamped on its own.  The
    gradient is autograd's for that function: ATen applies the clamp under a no-grad
    guard, so below the clamp the gradient still flows through the norm,
    ``u/n - (<f,u>/n^2) f/|f|`` with n = max(|f|, eps), u = t/max(|t|, eps).

    -> (N,) in feat_low's dtype on CPU, fp32 on a device.  A voxel outside the grid or a
    label outside [0, K) raises ValueError (this check reads one flag back from the
    device: the forward synchronises once).  On a ROCm device both directions are native
    and read/write only the low-resolution volume; fp32 only (half features that
    require grad are refused).  The backward groups the entries by voxel with a torch
    sort and reads the number of distinct voxels back (a second synchronisation); it
    returns a channels-last-strided gradient for the whole (B, C, z, y, x) tensor, zero
    outside sample ``batch``: a caller that loops over the B samples writes B^2 sample
    volumes and lets autograd add them (nothing at B = 1, VEON's training batch per
    device).  Its native form covers the 2x upsampling
    VEON uses; any other ``occ_size`` takes the torch sequence in the backward (the
    forward is native for every size).  On CPU: the torch sequence."""
    occ_size = tuple(int(v) for v in occ_size)
    eps, batch = float(eps), int(batch)
    _check_args(feat_low, voxels, labels, table, occ_size, eps, batch)
    if not feat_low.is_cuda:
        return _reference(feat_low, voxels, labels, table, occ_size, eps, batch)
    if feat_low.dtype != torch.float32:
        if feat_low.requires_grad and torch.is_grad_enabled():
            raise ValueError('voxel_cosine differentiates fp32 features only, got %s'
                             % feat_low.dtype)
        feat_low = feat_low.float()
    if feat_low.shape[1] > 1024:
        raise ValueError('voxel_cosine holds at most 1024 channels')
    return _VoxelCosine.apply(feat_low, voxels, labels, table, occ_size, eps, batch)
