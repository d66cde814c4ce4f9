"""BEVPoolv2 op -- host-side mirror of mmdet3d/ops/bev_pool_v2/bev_pool.py.

Same public names, argument order and return layout as the reference:

    bev_pool_v2(depth[B,N,D,H,W], feat[B,N,H,W,C], ranks_depth[P], ranks_feat[P],
                ranks_bev[P], bev_feat_shape=(B,Z,Y,X,C), interval_starts[I],
                interval_lengths[I]) -> Tensor[B,C,Z,Y,X]   (bev_pool.py:86-92)
    QuickCumsumCuda  (autograd.Function, bev_pool.py:11-83)
    TRTBEVPoolv2     (ONNX symbolic + eager forward, bev_pool.py:95-142)

What differs is underneath: the reference makes three full passes over the
voxel volume (new_zeros :27, kernel store, permute().contiguous() :91); here a
single fused HIP kernel writes the final (B,C,Z,Y,X) tensor once.  The fused
kernel needs the intervals ascending in voxel rank -- what
voxel_pooling_prepare_v2 always produces; for hand-made inputs that are not
sorted the op falls back to the reference's three-pass structure (still HIP).
There is no CPU path.
"""
import os

import torch

from ... import _lib
from . import bev_pool_v2_ext

__all__ = ['bev_pool_v2', 'TRTBEVPoolv2', 'QuickCumsumCuda']


def mark_sorted(interval_starts, first_rank, last_rank):
    """Tag produced-by-prepare interval arrays (ascending voxel ranks, intervals
    tiling the point arrays) so the op never has to sync.  The tag carries the
    tensor's version counter: an in-place update of the tensor voids it."""
    interval_starts._veon_sorted = (True, int(first_rank), int(last_rank),
                                    interval_starts._version, None, None)
    return interval_starts


def _sorted_info(ranks_bev, interval_starts, interval_lengths=None):
    """(fusable?, first_rank, last_rank) of the interval keys.  Fusable = keys
    strictly ascending AND the intervals tile the point arrays (starts[0] == 0,
    starts[i+1] == starts[i] + lengths[i], last end == P): the fused kernels
    derive every length from the next start, the reference kernel reads
    interval_lengths (bev_pool_cuda.cu:35), and the two agree exactly then.
    Cached on the tensor object together with the version counters of the
    tensors it was computed from; computing it costs one host sync."""
    tag = getattr(interval_starts, '_veon_sorted', None)
    if tag is not None:
        vs, vb, vl = tag[3], tag[4], tag[5]
        if (vs != interval_starts._version
                or (vb is not None and vb != ranks_bev._version)
                or (vl is not None and interval_lengths is not None
                    and vl != interval_lengths._version)):
            tag = None
    if tag is None:
        if interval_starts.numel() == 0:
            tag = (True, 0, -1)
        else:
            starts = interval_starts.long()
            keys = ranks_bev[starts]
            ok = torch.ones((), dtype=torch.bool, device=starts.device)
            if keys.numel() > 1:
                ok = ok & (keys[1:] > keys[:-1]).all()
            ok = ok & (starts[0] == 0)
            if interval_lengths is not None:
                lens = interval_lengths.long()
                if lens.numel() != starts.numel():
                    ok = ok & False
                else:
                    ok = ok & (starts[1:] == starts[:-1] + lens[:-1]).all()
                    ok = ok & (starts[-1] + lens[-1] == ranks_bev.numel())
            res = torch.stack([ok.long(), keys[0].long(), keys[-1].long()]).tolist()
            tag = (bool(res[0]), int(res[1]), int(res[2]))
        tag = tag + (interval_starts._version, ranks_bev._version,
                     None if interval_lengths is None else interval_lengths._version)
        interval_starts._veon_sorted = tag
    return tag[:3]


def _can_fuse(ranks_bev, interval_starts, n_voxels, interval_lengths=None):
    ok, first, last = _sorted_info(ranks_bev, interval_starts, interval_lengths)
    return ok and first >= 0 and last < n_voxels


def _cache_get(interval_starts, ranks_bev, name, key):
    """Index structure `name` cached on interval_starts for `key`, or None when
    absent or computed from other contents (version counters moved)."""
    ent = getattr(interval_starts, name, None)
    if ent is None or ent[1] != key:
        return None
    if ent[2] != (interval_starts._version, ranks_bev._version):
        return None
    return ent[0]


def _cache_put(interval_starts, ranks_bev, name, key, value):
    setattr(interval_starts, name,
            (value, key, (interval_starts._version, ranks_bev._version)))


_HALF = (torch.float16, torch.bfloat16)


def _feat_code(feat):
    """``feat_dtype`` of the *_ex entry points (include/veon_hip.h)."""
    if feat.dtype == torch.float16:
        return _lib.FEAT_F16
    if feat.dtype == torch.bfloat16:
        return _lib.FEAT_BF16
    return _lib.FEAT_F32


def _rows(feat):
    """``feat.contiguous()`` for the (B,N,H,W,C) feature rows.  The usual input is
    the permuted view of a contiguous (B,N,C,H,W) tensor
    (view_transformer.py:273-275): that transpose runs as one LDS-tiled kernel
    instead of PyTorch's strided copy (2 us instead of 5.5 us at S2)."""
    if feat.is_contiguous():
        return feat
    if (feat.is_cuda and feat.dim() == 5 and not (torch.is_grad_enabled()
                                                  and feat.requires_grad)
            and feat.dtype in (torch.float32, torch.float16, torch.bfloat16)):
        B, N, H, W, C = feat.shape
        if feat.stride() == (N * C * H * W, C * H * W, W, 1, H * W) and B * N <= 65535:
            out = torch.empty((B, N, H, W, C), dtype=feat.dtype, device=feat.device)
            _lib.launch('veon_feat_nchw_to_nhwc', feat.device, feat, out,
                        feat.element_size(), B * N, C, H * W)
            return out
    return feat.contiguous()


def _inference_feat(feat, *others):
    """The reference widens feat to fp32 before the kernel (bev_pool.py:21).
    When nothing needs a gradient, fp16 / bf16 rows are instead widened inside
    the kernel: same values, half the gather bytes, no fp32 copy."""
    if feat.dtype in _HALF and not (torch.is_grad_enabled() and any(
            t.requires_grad for t in (feat,) + others)):
        return _rows(feat)
    return _rows(feat).float()


def _prep_inputs(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                 interval_starts, interval_lengths):
    # casts of bev_pool.py:19-25 (no-ops for what the prepare produces)
    def as_(t, dtype):
        return t if (t.dtype == dtype and t.is_contiguous()) else t.contiguous().to(dtype)
    depth = as_(depth, torch.float32)
    feat = _inference_feat(feat, depth)
    ranks_bev = as_(ranks_bev, torch.int32)
    ranks_depth = as_(ranks_depth, torch.int32)
    ranks_feat = as_(ranks_feat, torch.int32)
    interval_lengths = as_(interval_lengths, torch.int32)
    starts = as_(interval_starts, torch.int32)
    if starts is not interval_starts:
        tag = getattr(interval_starts, '_veon_sorted', None)
        if tag is not None and tag[3] == interval_starts._version and tag[4] is None:
            mark_sorted(starts, tag[1], tag[2])   # a cast copy of trusted arrays
    return (depth, feat, ranks_depth, ranks_feat, ranks_bev, starts,
            interval_lengths)


def build_plan(ranks_bev, interval_starts, batch, voxels_per_batch,
               attach=True, counts=None):
    """Per-tile plan of the fused kernels (include/veon_hip.h
    ``veon_bev_pool_plan``).  With ``attach`` it is cached on
    ``interval_starts`` -- do that when the ranks themselves are cached
    (accelerate=True); otherwise it is rebuilt per call (two tiny kernels)."""
    dev = _lib.require_device(ranks_bev, interval_starts)
    n_ints = _lib.lib().veon_bev_pool_plan_ints(batch, voxels_per_batch)
    plan = torch.empty(n_ints, dtype=torch.int32, device=dev)
    _lib.launch('veon_bev_pool_plan', dev, interval_starts.numel(), ranks_bev.numel(),
                batch, voxels_per_batch, ranks_bev, interval_starts, counts, plan)
    if attach:
        _cache_put(interval_starts, ranks_bev, '_veon_plan', (batch, voxels_per_batch), plan)
    return plan


def build_voxel_table(ranks_bev, interval_starts, batch, voxels_per_batch,
                      attach=True, counts=None):
    """Dense voxel table of the row kernels (include/veon_hip.h
    ``veon_bev_pool_voxel_table``): vstart[v] = first point of voxel v in the
    rank-sorted arrays, B*vpb + 1 entries."""
    dev = _lib.require_device(ranks_bev, interval_starts)
    n_ints = _lib.lib().veon_bev_pool_voxel_table_ints(batch, voxels_per_batch)
    vstart = torch.empty(n_ints, dtype=torch.int32, device=dev)
    _lib.launch('veon_bev_pool_voxel_table', dev, interval_starts.numel(),
                ranks_bev.numel(), batch, voxels_per_batch, ranks_bev, interval_starts,
                counts, vstart)
    if attach:
        _cache_put(interval_starts, ranks_bev, '_veon_vstart', (batch, voxels_per_batch),
                   vstart)
    return vstart


def _voxel_table(ranks_bev, interval_starts, batch, vpb):
    vstart = _cache_get(interval_starts, ranks_bev, '_veon_vstart', (batch, vpb))
    if vstart is None:
        vstart = build_voxel_table(ranks_bev, interval_starts, batch, vpb)
    return vstart


# Row kernels (csrc/bev_pool_rows.hip) take over from the slab kernels at these
# channel counts (measured on MI355X, tools/poolbench.py: at C = 80 the fused
# max-pool is 34 -> 30 us with them, the full-resolution volume 34-40 -> 53 us;
# at C = 256 they win 2.3x / 3x).
ROWS_MIN_C = 128
ROWS_MIN_C_MAXPOOL = 64


def _check_out(out, shape, dev):
    if (tuple(out.shape) != shape or out.dtype != torch.float32
            or not out.is_contiguous() or out.device != dev):
        raise _lib.VeonHipError('out must be a contiguous fp32 %r tensor on %s'
                                % (shape, dev))


def _check_out_volume(out_volume, shape):
    if out_volume.shape != shape:
        raise _lib.VeonHipError('out_volume shape %r does not match the pooled '
                                'volume' % (out_volume.shape,))


def rows_forward(depth, feat, ranks_depth, ranks_feat, vstart, bev_feat_shape,
                 out=None, variant=0):
    """(B,C,Z,Y,X) fp32 volume by the row kernel, from the dense voxel table."""
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    dev = _lib.require_device(depth, feat, ranks_depth, ranks_feat, vstart)
    if vstart.numel() != B * Z * Y * X + 1:
        raise _lib.VeonHipError('voxel table does not match bev_feat_shape')
    if out is None:
        out = torch.empty((B, C, Z, Y, X), dtype=torch.float32, device=dev)
    else:
        _check_out(out, (B, C, Z, Y, X), dev)
    _lib.launch('veon_bev_pool_v2_fwd_rows', dev, C, B, Z * Y * X, depth, feat,
                _feat_code(feat), ranks_depth, ranks_feat, vstart, out, 0, feat.numel(),
                variant)
    return out


_COLD_ORDERS = {}
# 'azimuth' = cold_chunk_order(); default: the kernel's built-in order (measured on
# MI355X at the VEON shape: the azimuth order changes neither the L2 hit rate -- 60 % --
# nor FETCH_SIZE -- 82 vs 88 MB -- because a chunk of 32 consecutive x spans 25 m of the
# grid and so most azimuths; its imbalance between the XCDs then costs 10-20 %)
COLD_ORDER = os.environ.get('VEON_COLD_ORDER', 'none')


def cold_chunk_order(B, Zo, Yo, Xo, device, sectors=4, origin=None):
    """Order of the short-list chunks of the row max-pool kernel (include/veon_hip.h
    ``veon_bev_pool_v2_fwd_rows_maxpool_ordered``): chunks of the pooled volume sorted
    by AZIMUTH of their centre around ``origin`` (pooled-voxel coordinates (x, y);
    default: the centre of the grid, where the rig sits for every config of the
    reference) and dealt so that the workgroups one XCD receives (round-robin by
    linear id: i % 8) walk through ``sectors`` contiguous azimuth wedges.  A camera
    ray stays inside its wedge, so an XCD's 4 MiB L2 sees the feature rows of the one
    or two cameras that look that way (1/8 of the table) instead of all of them.  A
    static function of the grid: computed once on the host, cached on the device."""
    key = (int(B), int(Zo), int(Yo), int(Xo), str(device), int(sectors),
           None if origin is None else (float(origin[0]), float(origin[1])))
    tab = _COLD_ORDERS.get(key)
    if tab is None:
        import numpy as np
        chunk = _lib.lib().veon_bev_pool_rows_maxpool_chunk()
        plane = Zo * Yo * Xo
        nch = (plane + chunk - 1) // chunk
        ctr = np.minimum(np.arange(nch) * chunk + chunk // 2, plane - 1)
        xo, yo, zo = ctr % Xo, (ctr // Xo) % Yo, ctr // (Xo * Yo)
        ox, oy = (Xo / 2.0, Yo / 2.0) if origin is None else origin
        az = np.arctan2(yo + 0.5 - oy, xo + 0.5 - ox)
        rad = np.hypot(yo + 0.5 - oy, xo + 0.5 - ox)
        srt = np.lexsort((rad, zo, az))                  # azimuth, then z, then radius
        # 8 * sectors equal pieces of the sorted list; XCD k takes pieces k, k + 8, ...
        pieces = np.array_split(srt, 8 * sectors)
        per_xcd = [np.concatenate([pieces[k + 8 * j] for j in range(sectors)])
                   for k in range(8)]
        # cold workgroup i runs on XCD i % 8 and is that XCD's (i // 8)-th: deal the
        # XCDs' lists round-robin; lists differ in length by at most `sectors` chunks,
        # the leftovers go to whatever slots remain (still a permutation)
        order = np.full(nch, -1, dtype=np.int64)
        left = []
        for k, lst in enumerate(per_xcd):
            slots = np.arange(k, nch, 8)
            n = min(len(slots), len(lst))
            order[slots[:n]] = lst[:n]
            left.extend(lst[n:].tolist())
        order[order < 0] = np.array(left, dtype=np.int64)
        assert np.array_equal(np.sort(order), np.arange(nch))
        full = np.concatenate([order + b * nch for b in range(B)]).astype(np.int32)
        tab = torch.from_numpy(full).to(device)
        _COLD_ORDERS[key] = tab
    return tab


def rows_maxpool(depth, feat, ranks_depth, ranks_feat, vstart, bev_feat_shape, ds,
                 out_volume=None, chunk_order='default'):
    """Pool + (2,2,2) block max by the row kernel: (B,C,Z/2,Y/2,X/2) fp32, or the
    Conv3d body's padded bf16 input when ``out_volume`` is given.  ``chunk_order``:
    an int32 permutation of the cold chunks, None for the kernel's built-in order,
    'default' = the module's ``COLD_ORDER`` policy."""
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    dz, dy, dx = [int(v) for v in ds]
    dev = _lib.require_device(depth, feat, ranks_depth, ranks_feat, vstart)
    if vstart.numel() != B * Z * Y * X + 1:
        raise _lib.VeonHipError('voxel table does not match bev_feat_shape')
    if out_volume is not None:
        _check_out_volume(out_volume, (B, C, Z // dz, Y // dy, X // dx))
        target, padded, ret = out_volume.rows, 1, out_volume
    else:
        ret = torch.empty((B, C, Z // dz, Y // dy, X // dx), dtype=torch.float32,
                          device=dev)
        target, padded = ret, 0
    chunk_order = _cold_order(chunk_order, B, Z // dz, Y // dy, X // dx, dev)
    _lib.launch('veon_bev_pool_v2_fwd_rows_maxpool_ordered', dev, C, B, Z, Y, X, dz, dy, dx,
                depth, feat, _feat_code(feat), ranks_depth, ranks_feat, vstart, target,
                padded, feat.numel(), chunk_order)
    return ret


def _cold_order(chunk_order, B, Zo, Yo, Xo, dev):
    """The ``chunk_order`` argument of the row max-pool entry points: 'default' = the
    module's ``COLD_ORDER`` policy, None = the kernel's built-in order, or a checked
    int32 permutation of the cold chunks."""
    if isinstance(chunk_order, str):
        chunk_order = (cold_chunk_order(B, Zo, Yo, Xo, dev)
                       if COLD_ORDER == 'azimuth' else None)
    if chunk_order is not None:
        chunk = _lib.lib().veon_bev_pool_rows_maxpool_chunk()
        want = B * ((Zo * Yo * Xo + chunk - 1) // chunk)
        if (chunk_order.dtype != torch.int32 or chunk_order.numel() != want
                or chunk_order.device != dev or not chunk_order.is_contiguous()):
            raise _lib.VeonHipError('chunk_order must be a contiguous int32 permutation '
                                    'of %d chunks on %s' % (want, dev))
    return chunk_order


def rows_maxpool_winner(depth, feat, ranks_depth, ranks_feat, vstart, bev_feat_shape,
                        chunk_order='default'):
    """``rows_maxpool`` for fp32 rows plus the winner volume of the block max
    (include/veon_hip.h ``veon_bev_pool_v2_fwd_rows_maxpool_winner``):
    -> ((B,C,Z/2,Y/2,X/2) fp32, (B,Z/2,Y/2,X/2,C) uint8)."""
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    dev = _lib.require_device(depth, feat, ranks_depth, ranks_feat, vstart)
    if vstart.numel() != B * Z * Y * X + 1:
        raise _lib.VeonHipError('voxel table does not match bev_feat_shape')
    if feat.dtype != torch.float32:
        raise _lib.VeonHipError('the max-pool with winners takes fp32 feature rows')
    out = torch.empty((B, C, Z // 2, Y // 2, X // 2), dtype=torch.float32, device=dev)
    winner = torch.empty((B, Z // 2, Y // 2, X // 2, C), dtype=torch.uint8, device=dev)
    chunk_order = _cold_order(chunk_order, B, Z // 2, Y // 2, X // 2, dev)
    _lib.launch('veon_bev_pool_v2_fwd_rows_maxpool_winner', dev, C, B, Z, Y, X, 2, 2, 2,
                depth, feat, _lib.FEAT_F32, ranks_depth, ranks_feat, vstart, out,
                feat.numel(), chunk_order, winner)
    return out, winner


def build_point_table(ranks_depth, ranks_bev, table_len, n_voxels, counts=None):
    """Point -> voxel table of the fused backward (include/veon_hip.h
    ``veon_bev_pool_point_table``): pvox[ranks_depth[p]] = ranks_bev[p], -1 where the
    lift dropped the point.  ``counts``: device-side sizes of a sync-free prepare."""
    dev = _lib.require_device(ranks_depth, ranks_bev, counts)
    pvox = torch.empty(int(table_len), dtype=torch.int32, device=dev)
    _lib.launch('veon_bev_pool_point_table', dev, ranks_bev.numel(), int(table_len),
                int(n_voxels), ranks_depth, ranks_bev, counts, pvox)
    return pvox


def _point_table(ranks_depth, ranks_bev, interval_starts, table_len, n_voxels):
    """The table cached beside the voxel table (on ``interval_starts``: it lives as
    long as the cached ranks of accelerate=True do, one call otherwise)."""
    key = (int(table_len), int(n_voxels), ranks_depth.data_ptr(), ranks_depth._version)
    pvox = _cache_get(interval_starts, ranks_bev, '_veon_pvox', key)
    if pvox is None:
        pvox = build_point_table(ranks_depth, ranks_bev, table_len, n_voxels)
        _cache_put(interval_starts, ranks_bev, '_veon_pvox', key, pvox)
    return pvox


class _LiftMaxpoolFused(torch.autograd.Function):
    """Pool + (2,2,2) block max of a lift, differentiable w.r.t. depth and feat
    without the un-pooled volume in either direction: forward = the row max-pool
    kernel, which also records the winning child of every pooled (voxel, channel);
    backward = one wave per feature pixel walking its depth bins through the
    point -> voxel table.  The gradient is the reference's (bev_pool.py:43-83 behind
    ``torch.max(dim=-1).values`` of view_transformer_raw.py:549-553): all of it to the
    first maximal element of a block."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, vstart, pvox, bev_feat_shape,
                lift_layout):
        out, winner = rows_maxpool_winner(depth, feat, ranks_depth, ranks_feat, vstart,
                                          bev_feat_shape)
        ctx.save_for_backward(depth, feat, winner, pvox)
        ctx.geometry = (bev_feat_shape, lift_layout)
        return out

    @staticmethod
    def backward(ctx, out_grad):
        depth, feat, winner, pvox = ctx.saved_tensors
        (B, Z, Y, X, C), (n_images, D, H, W) = ctx.geometry
        dev = _lib.require_device(out_grad, depth, feat)
        og = out_grad.float().permute(0, 2, 3, 4, 1).contiguous()
        depth_grad = torch.zeros_like(depth) if ctx.needs_input_grad[0] else None
        feat_grad = torch.empty_like(feat)
        _lib.launch('veon_bev_pool_v2_bwd_rows_maxpool', dev, C, n_images, D, H * W, B, Z, Y,
                    X, og, winner, pvox, depth, feat, depth_grad, feat_grad)
        return (depth_grad, feat_grad if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


def _lift_maxpool_grad(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape,
                       interval_starts, ds, counts, vstart, lift_layout):
    """The training form of ``bev_pool_v2_maxpool`` (its ``lift_layout`` argument)."""
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    n_images, D, H, W = [int(v) for v in lift_layout]
    if (feat.dtype != torch.float32 or tuple(int(v) for v in ds) != (2, 2, 2) or C % 4
            or Z % 2 or Y % 2 or X % 2 or feat.numel() >= 2 ** 31):
        raise _lib.VeonHipError(
            'the differentiable fused max-pool takes fp32 feature rows, ds = (2,2,2) '
            'dividing the grid and C % 4 == 0 (got %s, ds %r, C %d)'
            % (feat.dtype, tuple(ds), C))
    if depth.numel() != n_images * D * H * W or feat.numel() != n_images * H * W * C:
        raise _lib.VeonHipError('lift_layout %r does not match depth %r / feat %r'
                                % (tuple(lift_layout), tuple(depth.shape),
                                   tuple(feat.shape)))
    _lib.require_device(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts)
    n_vox = B * Z * Y * X
    if counts is None:
        if vstart is None:
            vstart = _voxel_table(ranks_bev, interval_starts, B, Z * Y * X)
        pvox = _point_table(ranks_depth, ranks_bev, interval_starts, depth.numel(), n_vox)
    else:
        if vstart is None:
            vstart = build_voxel_table(ranks_bev, interval_starts, B, Z * Y * X,
                                       attach=False, counts=counts)
        pvox = build_point_table(ranks_depth, ranks_bev, depth.numel(), n_vox,
                                 counts=counts)
    return _LiftMaxpoolFused.apply(depth, feat, ranks_depth, ranks_feat, vstart, pvox,
                                   (B, Z, Y, X, C), (n_images, D, H, W))


def _rows_ok(C, ds=None, feat=None):
    if C < (ROWS_MIN_C if ds is None else ROWS_MIN_C_MAXPOOL) or C % 4:
        return False
    if feat is not None and feat.numel() >= 2 ** 31:   # 32-bit row offsets inside
        return False
    return ds is None or tuple(int(v) for v in ds) == (2, 2, 2)


def _fused_forward(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                   interval_starts, interval_lengths, bev_feat_shape, layout,
                   out=None):
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    dev = _lib.require_device(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                              interval_starts, interval_lengths)
    if out is not None:
        _check_out(out, (B, C, Z, Y, X) if layout == _lib.LAYOUT_BCZYX else (B, Z, Y, X, C),
                   dev)
    elif layout == _lib.LAYOUT_BCZYX:
        out = torch.empty((B, C, Z, Y, X), dtype=torch.float32, device=dev)
    else:
        out = torch.empty((B, Z, Y, X, C), dtype=torch.float32, device=dev)
    if layout == _lib.LAYOUT_BCZYX and _rows_ok(C, feat=feat):
        vstart = _voxel_table(ranks_bev, interval_starts, B, Z * Y * X)
        return rows_forward(depth, feat, ranks_depth, ranks_feat, vstart,
                            bev_feat_shape, out=out)
    plan = _cache_get(interval_starts, ranks_bev, '_veon_plan', (B, Z * Y * X))
    if plan is None:
        plan = build_plan(ranks_bev, interval_starts, B, Z * Y * X,
                          attach=False)
    _lib.launch('veon_bev_pool_v2_fwd_fused_ex', dev, C, interval_starts.numel(), B,
                Z * Y * X, depth, feat, _feat_code(feat), ranks_depth, ranks_feat, ranks_bev,
                interval_starts, interval_lengths, plan, out, layout)
    return out


def _backward_impl(out_grad_bzyxc, ranks_bev, depth, feat, ranks_feat,
                   ranks_depth):
    """QuickCumsumCuda.backward, bev_pool.py:43-83: re-sort the points by
    ranks_feat, rebuild intervals, launch the grad kernel."""
    depth_grad = torch.zeros_like(depth)
    feat_grad = torch.zeros_like(feat)
    if ranks_feat.numel() == 0:
        return depth_grad, feat_grad
    # group the points by feature pixel (stable, so the order inside a group
    # is the forward's storage order) and run-length encode the groups
    rf_sorted, order = torch.sort(ranks_feat, stable=True)
    _, counts = torch.unique_consecutive(rf_sorted, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    bev_pool_v2_ext.bev_pool_v2_backward(
        out_grad_bzyxc.contiguous(), depth_grad, feat_grad, depth, feat,
        ranks_depth[order].contiguous(), rf_sorted.contiguous(),
        ranks_bev[order].contiguous(), counts.int().contiguous(),
        starts.int().contiguous())
    return depth_grad, feat_grad


class QuickCumsumCuda(torch.autograd.Function):
    r"""BEVPoolv2 (`paper <https://arxiv.org/abs/2211.17111>`_); same contract
    as the reference class (bev_pool.py:11-83): returns the channels-last
    volume (B,Z,Y,X,C) and saves (ranks_bev, depth, feat, ranks_feat,
    ranks_depth) for backward."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                bev_feat_shape, interval_starts, interval_lengths):
        (depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
         interval_lengths) = _prep_inputs(depth, feat, ranks_depth, ranks_feat,
                                          ranks_bev, interval_starts,
                                          interval_lengths)
        B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
        feat = feat.float()
        if _can_fuse(ranks_bev, interval_starts, B * Z * Y * X, interval_lengths):
            out = _fused_forward(depth, feat, ranks_depth, ranks_feat,
                                 ranks_bev, interval_starts, interval_lengths,
                                 bev_feat_shape, _lib.LAYOUT_BZYXC)
        else:
            out = feat.new_zeros(tuple(int(s) for s in bev_feat_shape))
            bev_pool_v2_ext.bev_pool_v2_forward(
                depth, feat, out, ranks_depth, ranks_feat, ranks_bev,
                interval_lengths, interval_starts)
        ctx.save_for_backward(ranks_bev, depth, feat, ranks_feat, ranks_depth)
        return out

    @staticmethod
    def backward(ctx, out_grad):
        ranks_bev, depth, feat, ranks_feat, ranks_depth = ctx.saved_tensors
        depth_grad, feat_grad = _backward_impl(out_grad, ranks_bev, depth,
                                               feat, ranks_feat, ranks_depth)
        return depth_grad, feat_grad, None, None, None, None, None, None


class _BevPoolV2Fused(torch.autograd.Function):
    """bev_pool_v2 with the permute of bev_pool.py:91 folded into the kernel:
    returns (B,C,Z,Y,X) directly."""

    @staticmethod
    def forward(ctx, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                bev_feat_shape, interval_starts, interval_lengths):
        out = _fused_forward(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                             interval_starts, interval_lengths, bev_feat_shape,
                             _lib.LAYOUT_BCZYX)
        ctx.save_for_backward(ranks_bev, depth, feat, ranks_feat, ranks_depth)
        return out

    @staticmethod
    def backward(ctx, out_grad):
        ranks_bev, depth, feat, ranks_feat, ranks_depth = ctx.saved_tensors
        og = out_grad.permute(0, 2, 3, 4, 1).contiguous()
        depth_grad, feat_grad = _backward_impl(og, ranks_bev, depth, feat,
                                               ranks_feat, ranks_depth)
        return depth_grad, feat_grad, None, None, None, None, None, None


def bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                bev_feat_shape, interval_starts, interval_lengths, out=None):
    """Drop-in for mmdet3d.ops.bev_pool_v2.bev_pool.bev_pool_v2
    (bev_pool.py:86-92): returns the (B,C,Z,Y,X) contiguous fp32 volume,
    differentiable w.r.t. depth and feat.  veon_amd extension: ``out`` -- a
    caller-owned (B,C,Z,Y,X) fp32 tensor the fused inference kernel writes
    (every element) and returns, e.g. one chosen by ``placement.best_placed``;
    ignored when a gradient is needed or the intervals are not sorted."""
    (depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
     interval_lengths) = _prep_inputs(depth, feat, ranks_depth, ranks_feat,
                                      ranks_bev, interval_starts,
                                      interval_lengths)
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    if _can_fuse(ranks_bev, interval_starts, B * Z * Y * X, interval_lengths):
        no_grad = not (torch.is_grad_enabled()
                       and (depth.requires_grad or feat.requires_grad))
        if feat.dtype in _HALF or (out is not None and no_grad):
            # inference only (see _inference_feat): straight to the kernel
            return _fused_forward(depth, feat, ranks_depth, ranks_feat,
                                  ranks_bev, interval_starts, interval_lengths,
                                  bev_feat_shape, _lib.LAYOUT_BCZYX, out=out)
        return _BevPoolV2Fused.apply(depth, feat, ranks_depth, ranks_feat,
                                     ranks_bev, bev_feat_shape,
                                     interval_starts, interval_lengths)
    feat = feat.float()  # unsorted hand-made input: reference structure, fp32
    x = QuickCumsumCuda.apply(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                              bev_feat_shape, interval_starts,
                              interval_lengths)
    return x.permute(0, 4, 1, 2, 3).contiguous()


def bev_pool_v2_prepared(depth, feat, pre, bev_feat_shape, out=None):
    """Inference-only pooling straight from the device-resident output of the
    HIP prepare (``lss_prepare_hip.Prepared``): capacity-sized rank buffers and
    the plan the prepare emitted, no host synchronisation anywhere -- the whole
    per-call lift is hipGraph-capturable.  The plan alone drives the fused
    kernel, so the (unknown on the host) point / interval counts are not needed.
    An empty grid yields an all-zero (B,C,Z,Y,X) volume."""
    depth = depth.contiguous().float()
    feat = _inference_feat(feat, depth)
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    if pre.batch != B or pre.vpb != Z * Y * X:
        raise _lib.VeonHipError('prepared ranks do not match bev_feat_shape')
    dev = _lib.require_device(depth, feat, pre.ranks_bev)
    if out is not None:
        _check_out(out, (B, C, Z, Y, X), dev)
    if getattr(pre, 'vstart', None) is not None and _rows_ok(C, feat=feat):
        return rows_forward(depth, feat, pre.ranks_depth, pre.ranks_feat, pre.vstart,
                            bev_feat_shape, out=out)
    plan = pre.plan
    if plan is None:  # voxel count not a multiple of the tile: built per call
        plan = build_plan(pre.ranks_bev, pre.interval_starts, B, Z * Y * X,
                          attach=False, counts=pre.counts)
    if out is None:
        out = torch.empty((B, C, Z, Y, X), dtype=torch.float32, device=dev)
    # The interval count is unknown on the host here (the buffers are capacity-sized);
    # the launcher only uses it to pick the LDS tile width (32 or 64 intervals per
    # pass; either is correct).  Passing the capacity always selected the wide, slower
    # variant (42 vs 35 us at S2): estimate it instead -- about 0.3 intervals per
    # frustum point on nuScenes-like rigs (S2: 72.7 k of 249 k, SV: 342 k of 1.49 M).
    n_est = max(1, int(0.3 * pre.interval_starts.numel()))
    _lib.launch('veon_bev_pool_v2_fwd_fused_ex', dev, C, n_est, B, Z * Y * X, depth, feat,
                _feat_code(feat), pre.ranks_depth, pre.ranks_feat, pre.ranks_bev,
                pre.interval_starts, pre.interval_lengths, plan, out, _lib.LAYOUT_BCZYX)
    return out


def build_row_table(ranks_bev, interval_starts, batch, voxels_per_batch,
                    row_voxels, counts=None, attach=True):
    """First interval of every (b,z,y) row of X voxels, for the fused
    pool+max-pool kernel (include/veon_hip.h ``veon_bev_pool_row_table``)."""
    dev = _lib.require_device(ranks_bev, interval_starts)
    n_rows = batch * (voxels_per_batch // row_voxels)
    table = torch.empty(2 * (n_rows + 1), dtype=torch.int32, device=dev)
    _lib.launch('veon_bev_pool_row_table', dev, interval_starts.numel(), ranks_bev.numel(),
                batch, voxels_per_batch, row_voxels, ranks_bev, interval_starts, counts,
                table, table[n_rows + 1:])
    if attach:
        _cache_put(interval_starts, ranks_bev, '_veon_rows',
                   (batch, voxels_per_batch, row_voxels), table)
    return table


def bev_pool_v2_maxpool(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                        bev_feat_shape, interval_starts, interval_lengths, ds,
                        counts=None, out_volume=None, vstart=None, lift_layout=None):
    """Fusion of ``bev_pool_v2`` with the (dz,dy,dx) block max of
    LSSViewTransformerRaw.forward (view_transformer_raw.py:545-553): returns
    (B, C, Z/dz, Y/dy, X/dx) without writing the full-resolution volume.
    Bit-equal to max-pooling ``bev_pool_v2``'s output.  Intervals must be
    ascending in voxel rank (what the prepare produces).  ``out_volume`` (a
    ``conv3d_ops.PaddedVolume`` of shape (B,C,Z/dz,Y/dy,X/dx)) receives the
    result rounded to bf16 in the Conv3d body's input layout instead, and is
    returned.  ``counts`` / ``vstart``: device-side sizes and dense voxel table of
    a sync-free prepare (capacity-sized rank buffers).

    Inference-only unless ``lift_layout = (n_images, D, H, W)`` is given: the caller's
    promise that the ranks are those of a lift (ranks_depth = (img*D + d)*H*W + hw, one
    point at most per value, ranks_feat = img*H*W + hw; view_transformer_raw.py:268-274
    -- hand-made ranks do not have it, which is why it is not inferred).  Then, when
    ``depth`` or ``feat`` needs a gradient, the call is differentiable
    (``_LiftMaxpoolFused``: fp32 rows, ds = (2,2,2), C % 4 == 0, no ``out_volume``) with
    the same forward values."""
    if (lift_layout is not None and torch.is_grad_enabled()
            and (depth.requires_grad or feat.requires_grad)):
        if out_volume is not None:
            raise ValueError('out_volume is the inference form of the fused max-pool: '
                             'it cannot carry a gradient')
        if feat.dtype != torch.float32:
            raise _lib.VeonHipError('the differentiable fused max-pool takes fp32 '
                                    'feature rows, got %s' % feat.dtype)
        return _lift_maxpool_grad(depth.contiguous().float(), _rows(feat), ranks_depth,
                                  ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
                                  ds, counts, vstart, lift_layout)
    depth = depth.contiguous().float()
    feat = _inference_feat(feat, depth)
    B, Z, Y, X, C = [int(s) for s in bev_feat_shape]
    dz, dy, dx = [int(v) for v in ds]
    dev = _lib.require_device(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                              interval_starts, interval_lengths)
    if _rows_ok(C, ds, feat) and (counts is None or vstart is not None):
        if vstart is None:
            vstart = _voxel_table(ranks_bev, interval_starts, B, Z * Y * X)
        return rows_maxpool(depth, feat, ranks_depth, ranks_feat, vstart,
                            bev_feat_shape, ds, out_volume=out_volume)
    table = None
    if counts is None:
        table = _cache_get(interval_starts, ranks_bev, '_veon_rows', (B, Z * Y * X, X))
    if table is None:
        table = build_row_table(ranks_bev, interval_starts, B, Z * Y * X, X,
                                counts=counts, attach=False)
    if out_volume is not None:
        _check_out_volume(out_volume, (B, C, Z // dz, Y // dy, X // dx))
        _lib.launch('veon_bev_pool_v2_fwd_maxpool_padded', dev, C, interval_starts.numel(),
                    B, Z, Y, X, dz, dy, dx, depth, feat, _feat_code(feat), ranks_depth,
                    ranks_feat, ranks_bev, interval_starts, interval_lengths, table,
                    out_volume.rows)
        return out_volume
    out = torch.empty((B, C, Z // dz, Y // dy, X // dx), dtype=torch.float32,
                      device=dev)
    _lib.launch('veon_bev_pool_v2_fwd_maxpool_ex', dev, C, interval_starts.numel(), B,
                Z, Y, X, dz, dy, dx, depth, feat, _feat_code(feat), ranks_depth, ranks_feat,
                ranks_bev, interval_starts, interval_lengths, table, out)
    return out


class TRTBEVPoolv2(torch.autograd.Function):
    """ONNX export shim, same symbolic as the reference (bev_pool.py:95-142)."""

    @staticmethod
    def symbolic(g, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                 interval_starts, interval_lengths, out_height=128,
                 out_width=128):
        return g.op('mmdeploy::bev_pool_v2', depth, feat, ranks_depth,
                    ranks_feat, ranks_bev, interval_starts, interval_lengths,
                    out_height_i=out_height, out_width_i=out_width)

    @staticmethod
    def forward(g, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                interval_starts, interval_lengths, out_height=128,
                out_width=128):
        # depth (N,D,H,W), feat (N,H,W,C) -> (1, out_h, out_w, C)
        feat = feat.unsqueeze(0)
        depth = depth.unsqueeze(0)
        bev_feat_shape = (depth.shape[0], 1, out_height, out_width,
                          feat.shape[-1])
        bev_feat = bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev,
                               bev_feat_shape, interval_starts,
                               interval_lengths)
        return bev_feat.squeeze(2).permute(0, 2, 3, 1)
