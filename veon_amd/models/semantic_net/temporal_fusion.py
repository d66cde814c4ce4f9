"""Temporal path of VEON's 3D alignment network -- mirrors of

* ``TemporalFusionMultiFrame`` and its parts ``BeforeFusionLayer``,
  ``TemporalFusionMultiFrameMiddle3x3Seq``, ``TemporalDeformable``,
  ``TemporalFusionDeformMiddle``
  (mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:13-204), with the
  reference's attribute names so a VEON checkpoint's ``temporal_fusion.*`` keys
  load unchanged;
* ``SANInVeonTemporal.align_after_lss``
  (mmdet3d/models/semantic_net/san_in_veon_temporal.py:325-365): the rigid warp
  of a past frame's lifted volume into the current ego frame.

The PyTorch formulation below is the definition (CPU, training); it is pinned by
vectors generated from the reference's own classes
(oracle/tools/gen_golden_temporal.py).  Two quirks of the reference are kept on
purpose because trained weights depend on them: ``TemporalDeformable`` stacks its
base grid as (z, y, x) while ``grid_sample`` reads the last axis as (x, y, z), so
the W-axis sampling position is driven by the voxel's z index and vice versa; and
the offsets are divided by (D, H, W) in normalised units.

On a ROCm device at inference the whole fusion runs on ``PaddedVolume`` rows
(csrc/conv3d.hip, csrc/temporal.hip): 3x3x3 convs on the implicit-GEMM MFMA
kernel with BN/ReLU/GELU epilogues, 1x1x1 projections as GEMMs, the deformable
sampling + 8-sample attention in one gather kernel, and the warp as a trilinear
gather on the channels-last grid (the zero halo is the zero padding).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import conv3d_ops, vit_ops
from .._native_cache import NativeCacheMixin
from .._train_fns import _BNReLUTrainFn, _rows_linear
from .align_net_body import (ConvModule3d, _PackFn, _UnpackFn, conv_module_train,
                             conv_module_train_ok)
from ... import half as _half


def _conv_bn(cin, cout):
    return ConvModule3d(cin, cout, 3, 1, 1, bias=False, norm=True, act=True)


def _fast(x):
    return isinstance(x, conv3d_ops.PaddedVolume)


def _conv_hip(cm, vol, out=None):
    """ConvModule3d (3x3x3 + BN + ReLU) on a PaddedVolume."""
    if cm.__dict__.get('_hip3') is None:
        cm.__dict__['_hip3'] = cm.folded(pack=True)
    w, sc, sh = cm.__dict__['_hip3']
    return conv3d_ops.conv3d_k3(vol, w, sc, sh, relu=cm.activate is not None, out=out)


def _cat(vols):
    """Channel concatenation of PaddedVolumes (halo rows stay zero)."""
    B, _, Z, Y, X = vols[0].shape
    C = sum(v.shape[1] for v in vols)
    out = conv3d_ops.PaddedVolume.__new__(conv3d_ops.PaddedVolume)
    out.shape = (B, C, Z, Y, X)
    out.guard, out.M = vols[0].guard, vols[0].M
    out.storage = torch.cat([v.storage for v in vols], dim=1)
    out.rows = out.storage[out.guard:out.guard + out.M]
    return out


# ------------------------------------------------- native training (storage tensors)
# The differentiable values of the native training path are the STORAGE tensors of
# PaddedVolumes (half, guard rows included), as in ``_ResBlockTrainFn``; ``shape`` is the
# (B, C, Z, Y, X) of the volume a storage tensor holds.  ``_rows_linear`` and
# ``_BNReLUTrainFn`` live in ``models/_train_fns.py`` (the prediction heads share them).
class _ConvBiasTrainFn(torch.autograd.Function):
    """3x3x3 conv (+ bias) on padded rows, no norm, no activation: the stored output is
    the pre-activation.  Backward: bias gradient (``colsum``), MFMA weight gradient, data
    gradient through the forward kernel.  The incoming gradient has a zero halo."""

    @staticmethod
    def forward(ctx, xs, w, b, shape):
        x = conv3d_ops.PaddedVolume.from_storage(xs, shape)
        shift = None if b is None else b.detach().float().contiguous()
        ctx.shape, ctx.half = tuple(shape), _half.dtype()
        ctx.save_for_backward(xs, w)
        return conv3d_ops.conv3d_k3(x, conv3d_ops.pack_weight(w), None, shift).storage

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dys):
        xs, w = ctx.saved_tensors
        B, _, Z, Y, X = ctx.shape
        vol = conv3d_ops.PaddedVolume.from_storage
        x, dy = vol(xs, ctx.shape), vol(dys.contiguous(), (B, w.shape[0], Z, Y, X))
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        db = vit_ops.colsum(dy.rows).to(w.dtype) if need_b else None
        dw = conv3d_ops.wgrad_to_param(conv3d_ops.conv3d_k3_wgrad(dy, x), w) if need_w else None
        dxs = None
        if need_x:
            dxs = conv3d_ops.conv3d_k3(dy, conv3d_ops.pack_weight_dgrad(w).to(ctx.half)).storage
        return dxs, dw, db, None


class _GeluVolFn(torch.autograd.Function):
    """Exact GELU on a storage tensor from the saved pre-activation (zero stays zero: the
    halo survives in both directions)."""

    @staticmethod
    def forward(ctx, ys):
        ctx.save_for_backward(ys)
        return vit_ops.gelu(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh):
        ys, = ctx.saved_tensors
        return vit_ops.gelu_bwd(dh.contiguous(), ys)


class BeforeFusionLayer(nn.Module):
    """One shared conv applied to every frame (align_net_occ3d.py:77-86)."""

    def __init__(self, channels):
        super().__init__()
        self.offset_conv = _conv_bn(channels, channels)

    def forward(self, feat_list):
        if _fast(feat_list[0]):
            return [_conv_hip(self.offset_conv, f) for f in feat_list]
        return [self.offset_conv(f) for f in feat_list]


class TemporalFusionMultiFrameMiddle3x3Seq(nn.Module):
    """Folds the past frames oldest-first, two at a time, then the current one
    (align_net_occ3d.py:25-46).  Returns (reference feature, folded past)."""

    def __init__(self, channels, seqs=2):
        super().__init__()
        self.t_fuse = nn.ModuleList([_conv_bn(channels * 2, channels)
                                     for _ in range(seqs)])

    def forward(self, cur_occ_feat, prev_occ_feats):
        fast = _fast(cur_occ_feat)
        cat = _cat if fast else (lambda ts: torch.cat(ts, dim=1))
        conv = (lambda cm, v: _conv_hip(cm, v)) if fast else (lambda cm, v: cm(v))
        past = prev_occ_feats[-1]
        idx = 0
        for frame in prev_occ_feats[-2::-1]:
            past = conv(self.t_fuse[idx], cat([frame, past]))
            idx += 1
        ref = conv(self.t_fuse[idx], cat([cur_occ_feat, past]))
        return ref, past


class TemporalDeformable(NativeCacheMixin, nn.Module):
    """Deformable cross-frame attention (align_net_occ3d.py:89-204): queries and
    sampling offsets from one volume, keys/values sampled trilinearly from the
    other at ``num_samples`` points per head, softmax over the samples.

    ``hip_train`` (class attribute, default False): opt-in native TRAINING path.  When
    set, a training-mode module on ROCm fp32 tensors (or, inside
    ``TemporalFusionMultiFrame``, on the storage tensors of PaddedVolumes) whose widths
    the kernels support trains on padded half rows: projections as GEMMs with MFMA weight
    gradients, the offset convs on the implicit-GEMM kernel, the deformable attention and
    its backward in csrc/temporal.hip / temporal_train.hip, train-mode BatchNorm passes.
    ``out_proj`` runs without its bias there (it cancels in train-mode BN; it enters the
    running mean, and its gradient is exactly zero).  As on the other native training
    paths, the inner modules are not called: hooks registered on them do not fire."""

    hip_train = False

    def __init__(self, channels, num_heads=4, num_samples=8):
        super().__init__()
        assert channels % num_heads == 0
        self.channels, self.num_heads, self.num_samples = channels, num_heads, num_samples
        self.head_dim = channels // num_heads
        self.offset_conv = nn.Sequential(
            nn.Conv3d(channels, channels, 3, padding=1),
            nn.GELU(),
            nn.Conv3d(channels, num_heads * num_samples * 3, 3, padding=1, bias=False),
            nn.Tanh())
        self.key_value_proj = nn.Conv3d(channels, channels * 2, 1)
        self.query_proj = nn.Conv3d(channels, channels, 1)
        self.out_proj = nn.Conv3d(channels, channels, 1)
        self.final_norm = nn.BatchNorm3d(channels)
        self.out_activate = nn.ReLU()

    # ------------------------------------------------------------ definition
    def sampling_grid(self, offsets):
        """offsets (N, S, 3, D, H, W) in tanh units -> grid_sample grid
        (N, S*D, H, W, 3).  Component a of the last axis is built from the a-th
        of (z, y, x) and divided by the a-th of (D, H, W) -- the reference's
        order, which grid_sample then reads as (x, y, z)."""
        N, S, _, D, H, W = offsets.shape
        dev, dt = offsets.device, offsets.dtype
        axes = [torch.linspace(-1, 1, n, device=dev, dtype=dt) for n in (D, H, W)]
        base = torch.stack(torch.meshgrid(*axes, indexing='ij'), dim=0)  # (3,D,H,W)
        size = torch.tensor([D, H, W], device=dev, dtype=dt).view(1, 1, 3, 1, 1, 1)
        g = (base.view(1, 1, 3, D, H, W) + offsets / size).clamp(-1, 1)
        return g.permute(0, 1, 3, 4, 5, 2).reshape(N, S * D, H, W, 3)

    def attend(self, kv, query, offsets):
        """kv (B, 2C, D,H,W) laid out per head as [key | value]; query (B,C,...);
        offsets (B, heads*S*3, ...) after tanh -> fused (B, C, D, H, W)."""
        B, C, D, H, W = query.shape
        nh, S, hd = self.num_heads, self.num_samples, self.head_dim
        grid = self.sampling_grid(offsets.reshape(B * nh, S, 3, D, H, W))
        got = F.grid_sample(kv.reshape(B * nh, 2 * hd, D, H, W), grid, mode='bilinear',
                            padding_mode='border', align_corners=True)
        got = got.view(B, nh, 2 * hd, S, D, H, W)
        key, value = got[:, :, :hd], got[:, :, hd:]
        q = query.view(B, nh, hd, 1, D, H, W) * hd ** -0.5
        attn = (q * key).sum(dim=2, keepdim=True).softmax(dim=3)
        return (attn * value).sum(dim=3).reshape(B, C, D, H, W)

    def forward(self, feat_prev, feat_curr):
        if _fast(feat_curr):
            return self.hip_forward(feat_prev, feat_curr)
        if self.hip_train_ok(feat_prev, feat_curr):
            shape = tuple(feat_curr.shape)
            out = self.train_native(_PackFn.apply(feat_prev), _PackFn.apply(feat_curr), shape)
            return _UnpackFn.apply(out, shape)
        fused = self.attend(self.key_value_proj(feat_prev), self.query_proj(feat_curr),
                            self.offset_conv(feat_curr))
        return self.out_activate(self.final_norm(self.out_proj(fused)))

    # ------------------------------------------------------- native training
    def train_supported(self):
        """Widths and parameters the native training chain takes: C % 64 == 0, head dim
        32 or 64, 8 samples, fp32 parameters, train-mode BN with buffers."""
        bn = self.final_norm
        return (self.channels % 64 == 0 and self.head_dim in (32, 64)
                and self.num_samples == conv3d_ops.DEFORM_SAMPLES
                and self.num_heads * 2 * (self.head_dim // 8) <= 64
                and 64 % (self.num_heads * 2 * (self.head_dim // 8)) == 0
                and all(p.dtype == torch.float32 for p in self.parameters())
                and bn.training and bn.affine and bn.track_running_stats)

    def hip_train_ok(self, *xs):
        return (self.hip_train and self.training and self.train_supported()
                and all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32
                        and x.dim() == 5 for x in xs))

    def project_kv_train(self, prev_s, shape):
        """key/value projection of the sampled volume (storage in, storage out); both
        calls of ``TemporalFusionDeformMiddle`` share it and autograd adds their dKV."""
        return _rows_linear(prev_s, shape, self.key_value_proj.weight, self.key_value_proj.bias)

    def train_native(self, prev_s, curr_s, shape, kv_s=None):
        """The training chain on storage tensors of PaddedVolumes of ``shape``."""
        B, C, Z, Y, X = shape
        if kv_s is None:
            kv_s = self.project_kv_train(prev_s, shape)
        q_s = _rows_linear(curr_s, shape, self.query_proj.weight, self.query_proj.bias)
        c1, c2 = self.offset_conv[0], self.offset_conv[2]
        hid = _GeluVolFn.apply(_ConvBiasTrainFn.apply(curr_s, c1.weight, c1.bias, shape))
        # output channels zero-padded to the weight gradient's tile (96 -> 128 for four
        # heads): the op ignores the surplus, F.pad's backward drops the padded rows of dW
        noff = c2.out_channels
        w2 = F.pad(c2.weight, (0,) * 8 + (0, -noff % 64))
        off_s = _ConvBiasTrainFn.apply(hid, w2, None, shape)     # tanh is taken in the op
        fused = conv3d_ops.deform_attention_train(kv_s, q_s, off_s, self.num_heads, shape)
        bn = self.final_norm
        y_s = _rows_linear(fused, shape, self.out_proj.weight, None)
        return _BNReLUTrainFn.apply(y_s, bn.weight, bn.bias, self.out_proj.bias, shape, bn)

    # ------------------------------------------------------------- MFMA path
    _native_cache = ('_hip',)

    def _packed(self):
        p = self.__dict__.get('_hip')
        if p is None:
            C = self.channels
            bf = lambda w: w.detach().reshape(w.shape[0], -1).to(_half.dtype()).contiguous()
            c1, c2 = self.offset_conv[0], self.offset_conv[2]
            bn = self.final_norm
            g = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
            p = dict(
                w1=conv3d_ops.pack_weight(c1.weight), b1=c1.bias.detach().float().contiguous(),
                w2=conv3d_ops.pack_weight(c2.weight),
                wkv=bf(self.key_value_proj.weight),
                bkv=self.key_value_proj.bias.detach().float().contiguous(),
                wq=bf(self.query_proj.weight),
                bq=self.query_proj.bias.detach().float().contiguous(),
                wo=bf(self.out_proj.weight), go=g.contiguous(),
                so=((self.out_proj.bias.detach().float() - bn.running_mean.float()) * g
                    + bn.bias.detach().float()).contiguous())
            self.__dict__['_hip'] = p
        return p

    def project_kv(self, feat_prev):
        """key/value projection of the sampled volume; both calls of
        ``TemporalFusionDeformMiddle`` share it."""
        p = self._packed()
        kv = feat_prev.like(2 * self.channels)
        vit_ops.linear(feat_prev.rows, p['wkv'], p['bkv'], vit_ops.EPI_BF16, out=kv.rows)
        return kv

    def hip_forward(self, feat_prev, feat_curr, kv=None):
        p = self._packed()
        if kv is None:
            kv = self.project_kv(feat_prev)
        q = feat_curr.like()
        vit_ops.linear(feat_curr.rows, p['wq'], p['bq'], vit_ops.EPI_BF16, out=q.rows)
        hid = conv3d_ops.conv3d_k3(feat_curr, p['w1'], None, p['b1'], act='gelu')
        off = conv3d_ops.conv3d_k3(hid, p['w2'])          # tanh is taken in the gather
        fused = conv3d_ops.deform_attention(kv, q, off, self.num_heads, self.num_samples)
        out = feat_curr.like()
        vit_ops.linear(fused.rows, p['wo'], p['so'], vit_ops.EPI_AFFINE_RELU, out=out.rows,
                       gamma=p['go'])
        conv3d_ops.zero_halo(out)   # the GEMM wrote relu(shift) into the halo rows
        return out


class TemporalFusionDeformMiddle(nn.Module):
    """(align_net_occ3d.py:13-22) concatenates the reference feature with its two
    deformable views: of the current frame and of the folded past."""

    def __init__(self, channels):
        super().__init__()
        self.t_deform = TemporalDeformable(channels=channels)

    def forward(self, mid_feat, occ_feat, prev_feat):
        if _fast(mid_feat):
            kv = self.t_deform.project_kv(mid_feat)
            a = self.t_deform.hip_forward(mid_feat, occ_feat, kv)
            b = self.t_deform.hip_forward(mid_feat, prev_feat, kv)
            return _cat([mid_feat, a, b])
        a = self.t_deform(mid_feat, occ_feat)
        b = self.t_deform(mid_feat, prev_feat)
        return torch.cat([mid_feat, a, b], dim=1)


class TemporalFusionMultiFrame(nn.Module):
    """(align_net_occ3d.py:49-74) current volume + aligned past volumes -> one
    volume of the same shape.  Accepts (B,C,Z,Y,X) tensors, or PaddedVolumes on
    the MFMA path (``hip_ok``).

    ``hip_train`` (class attribute, default False): opt-in native TRAINING path.  When
    set, a training-mode call on ROCm fp32 tensors whose widths the kernels support packs
    once, runs every ``ConvModule3d`` as conv -> train-mode BN -> ReLU on padded half rows
    (``before_fusion_layer`` frame by frame in the definition's order, each call with its
    own batch statistics and buffer update), the deformable middle as
    ``TemporalDeformable.train_native`` with one shared key/value projection, and unpacks
    once.  Past frames that need no gradient get no data gradient.  Anything else (other
    widths, CPU tensors, eval mode, the switch off) takes the paths above unchanged.  As
    on the other native training paths, the inner modules are not called: hooks
    registered on them do not fire."""

    hip_train = False

    def __init__(self, channels, seqs=2):
        super().__init__()
        self.t_final = _conv_bn(channels * 3, channels)
        self.before_fusion_layer = BeforeFusionLayer(channels)
        self.t_fuse_mid = TemporalFusionMultiFrameMiddle3x3Seq(channels, seqs=seqs)
        self.deform_fusion_layer = TemporalFusionDeformMiddle(channels)

    def hip_ok(self, x):
        c = self.t_final.conv.out_channels
        return (not self.training and not torch.is_grad_enabled() and c % 64 == 0
                and (c // self.deform_fusion_layer.t_deform.num_heads) in (32, 64)
                and self.deform_fusion_layer.t_deform.num_samples == 8
                and (_fast(x) or x.is_cuda))

    def hip_train_ok(self, cur, prevs):
        convs = [self.t_final, self.before_fusion_layer.offset_conv] + list(self.t_fuse_mid.t_fuse)
        return (self.hip_train and self.training and len(prevs) == len(self.t_fuse_mid.t_fuse)
                and all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32
                        and x.dim() == 5 and x.shape == cur.shape for x in [cur] + list(prevs))
                and self.deform_fusion_layer.t_deform.training
                and self.deform_fusion_layer.t_deform.train_supported()
                and all(conv_module_train_ok(cm) for cm in convs))

    def train_native(self, cur_occ_feat, prev_occ_feats):
        shape = tuple(cur_occ_feat.shape)
        wide = lambda k: (shape[0], k * shape[1]) + shape[2:]      # noqa: E731
        before = self.before_fusion_layer.offset_conv
        feats = [conv_module_train(before, _PackFn.apply(t), shape)[0]
                 for t in [cur_occ_feat] + list(prev_occ_feats)]
        cur, prevs = feats[0], feats[1:]
        past, idx = prevs[-1], 0
        for frame in prevs[-2::-1]:
            past = conv_module_train(self.t_fuse_mid.t_fuse[idx],
                                     torch.cat([frame, past], dim=1), wide(2))[0]
            idx += 1
        ref = conv_module_train(self.t_fuse_mid.t_fuse[idx],
                                torch.cat([cur, past], dim=1), wide(2))[0]
        td = self.deform_fusion_layer.t_deform
        kv = td.project_kv_train(ref, shape)
        a = td.train_native(ref, cur, shape, kv)
        b = td.train_native(ref, past, shape, kv)
        out = conv_module_train(self.t_final, torch.cat([ref, a, b], dim=1), wide(3))[0]
        return _UnpackFn.apply(out, shape)

    def forward(self, cur_occ_feat, prev_occ_feats):
        if not _fast(cur_occ_feat) and self.hip_train_ok(cur_occ_feat, prev_occ_feats):
            return self.train_native(cur_occ_feat, prev_occ_feats)
        feats = self.before_fusion_layer([cur_occ_feat] + list(prev_occ_feats))
        cur, prevs = feats[0], feats[1:]
        ref, past = self.t_fuse_mid(cur, prevs)
        fused = self.deform_fusion_layer(ref, cur, past)
        if _fast(fused):
            return _conv_hip(self.t_final, fused)
        return self.t_final(fused)

    def forward_fast(self, cur_occ_feat, prev_occ_feats):
        """fp32 (B,C,Z,Y,X) ROCm tensors in and out, MFMA path inside."""
        vols = [conv3d_ops.pack(t) for t in [cur_occ_feat] + list(prev_occ_feats)]
        return conv3d_ops.unpack(self.forward(vols[0], vols[1:]))


# --------------------------------------------------------------------- the warp
def voxel_centres(grid_config, ds_feat, shape):
    """First voxel centre and step (x, y, z) of the max-pooled grid
    (san_in_veon_temporal.py:326-340); ``ds_feat`` is given in (z, y, x) order."""
    step = [grid_config[s][2] * ds_feat[i] for i, s in enumerate(['z', 'y', 'x'])][::-1]
    first = [grid_config[s][0] + st / 2 for s, st in zip(['x', 'y', 'z'], step)]
    return first, step


def prev_from_cur(adj_metas):
    """(B,4,4) current-ego -> past-ego transforms (san_in_veon_temporal.py:343-345)."""
    cur2glob, prev2glob = adj_metas
    return torch.linalg.inv(prev2glob[:, 0]) @ cur2glob[:, 0]


def align_after_lss(occ_feat, adj_metas, grid_config, ds_feat):
    """Resample a past frame's volume (B,C,Z,Y,X) at the positions the current
    frame's voxel centres have in the past ego frame; trilinear, zeros outside
    (san_in_veon_temporal.py:325-365).  PaddedVolume in -> PaddedVolume out."""
    if _fast(occ_feat):
        B, C, Z, Y, X = occ_feat.shape
        first, step = voxel_centres(grid_config, ds_feat, (Z, Y, X))
        dev = occ_feat.device
        A = conv3d_ops.warp_affine(adj_metas[0].to(dev), adj_metas[1].to(dev), first, step)
        return conv3d_ops.warp_volume(occ_feat, A)
    B, C, Z, Y, X = occ_feat.shape
    dev, dt = occ_feat.device, occ_feat.dtype
    first, step = voxel_centres(grid_config, ds_feat, (Z, Y, X))
    axes = [torch.arange(n, device=dev) * st + f0
            for n, st, f0 in zip((X, Y, Z), step, first)]
    # reference order: the flattened list runs x-major (meshgrid 'ij' over x,y,z)
    pts = torch.stack(torch.meshgrid(*axes, indexing='ij'), dim=-1).to(dt)  # (X,Y,Z,3)
    T = prev_from_cur(adj_metas).to(dt)
    moved = torch.einsum('xyzj,bij->bxyzi', pts, T[:, :3, :3]) + T[:, None, None, None, :3, 3]
    moved = moved.permute(0, 3, 2, 1, 4)                                   # (B,Z,Y,X,3)
    lo = pts[0, 0, 0]
    span = pts[-1, -1, -1] - lo
    grid = (moved - lo) / span * 2 - 1
    return F.grid_sample(occ_feat, grid, mode='bilinear', padding_mode='zeros',
                         align_corners=True)
