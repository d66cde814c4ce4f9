"""On-device Occ3D evaluation: the two metrics of the reference's occ_metrics.py, the
mIoU of ``Metric_mIoU`` (mmdet3d/datasets/occ_metrics.py:52-147), which is the one its
``NuScenesDatasetOccpancy.evaluate`` computes, and the F-score of ``Metric_FScore``
(occ_metrics.py:150-237), the geometry metric of the Occ3D benchmark.

    occ_labels   the label-only tail of the occupancy path (csrc/occ_tail.hip): uint8
                 labels as ``VEONTemporal.simple_test`` returns them, nothing else
                 written; optionally the confusion matrix in the same kernel
    occ_labels_grouped  the same against a detailed vocabulary: K logit rows, runs of
                 rows merged by their maximum (csrc/occ_tail.hip; a torch
                 mirror on the CPU)
    confusion    the same confusion matrix for labels that already exist
    OccMiouMetric  ``Metric_mIoU`` with its state (an int64 histogram) on the device:
                 ``add_batch`` never synchronises, ``count_miou`` reads back once
    fscore_reach   a distance threshold on the voxel lattice as a table of integer
                 reaches, refused where the reference's answer would hang on rounding
    fscore_counts  the four integer counts per sample behind accuracy and completeness
                 (csrc/occ_fscore.hip; a torch mirror on the CPU)
    OccFScoreMetric  ``Metric_FScore`` with the per-sample counts on the device:
                 ``add_batch`` never synchronises, ``count_fscore`` reads back once

The reference finds nearest neighbours with two KD-trees per sample on the host.  Both of
its point sets are voxel centres of one lattice, so the nearest-neighbour test is an
integer stencil, and its totals are reproduced exactly, not approximately.
"""
import ctypes
import functools
import itertools

import numpy as np
import torch

from . import _lib
from .vocabulary import group_table, lowest_argmax, merge_runs

# occ_metrics.py:59-62
CLASS_NAMES = ['others', 'barrier', 'bicycle', 'bus', 'car', 'construction_vehicle',
               'motorcycle', 'pedestrian', 'traffic_cone', 'trailer', 'truck',
               'driveable_surface', 'other_flat', 'sidewalk', 'terrain', 'manmade',
               'vegetation', 'free']
IGNORE = 255


def _as_u8(t, what):
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError('%s must be a contiguous uint8 tensor, got %s' % (what, t.dtype))
    return t


def _check_counting(gt, mask, hist, shape, n_cl):
    """The optional arguments of the label tails: ``gt`` / ``mask`` uint8 of ``shape`` =
    (B, X, Y, Z), ``hist`` int64 with n_cl * n_cl elements."""
    for name, t in (('gt', gt), ('mask', mask)):
        if t is not None:
            _as_u8(t, name)
            assert tuple(t.shape) == shape, (name, tuple(t.shape))
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.is_contiguous()
        assert hist.numel() == n_cl * n_cl, (tuple(hist.shape), n_cl)


def _launch_labels(entry, dev, sem_low, bin_low, occ_size, table, gt, mask, hist):
    """uint8 (B,X,Y,Z) from ``entry``; ``table``: the arguments between the row count and
    ``bin_low`` (none, or the group table's three)."""
    assert sem_low.dtype == bin_low.dtype == torch.float32
    B, K, zi, yi, xi = sem_low.shape
    Zo, Yo, Xo = (int(v) for v in occ_size)
    labels = torch.empty((B, Xo, Yo, Zo), dtype=torch.uint8, device=dev)
    _lib.launch(entry, dev, sem_low, _lib.strides(sem_low), K, *table, bin_low,
                _lib.strides(bin_low), B, zi, yi, xi, Zo, Yo, Xo, labels, gt, mask, hist)
    return labels


def occ_labels(sem_low, bin_low, occ_size, gt=None, mask=None, hist=None):
    """Label volume (B,X,Y,Z) uint8 of the class logits ``sem_low`` (B,Q,z,y,x) and the
    occupancy logits ``bin_low`` (B,2,z,y,x) -- fp32, ANY strides -- at ``occ_size`` =
    (Z,Y,X): bit-equal to ``conv3d_ops.occ_classify(...)[2]``, without the upsampled
    volumes.  With ``gt`` (B,X,Y,Z) uint8 and ``hist`` ((Q+1, Q+1) int64, contiguous)
    the same kernel adds the sample's confusion matrix to ``hist`` (rows: ground truth;
    voxels with ``mask`` (uint8, optional) == 0 or gt > Q are skipped)."""
    dev = _lib.require_device(sem_low, bin_low, gt, mask, hist)
    assert sem_low.dtype == bin_low.dtype == torch.float32
    B, Q, zi, yi, xi = sem_low.shape
    assert tuple(bin_low.shape) == (B, 2, zi, yi, xi)
    Zo, Yo, Xo = (int(v) for v in occ_size)
    _check_counting(gt, mask, hist, (B, Xo, Yo, Zo), Q + 1)
    return _launch_labels('veon_occ_labels', dev, sem_low, bin_low, occ_size, (), gt, mask,
                          hist)


def confusion(pred, gt, mask=None, n_cl=18, hist=None, flag=None):
    """hist[g, p] += number of voxels with ground truth g and prediction p among those
    with ``mask`` != 0 (no mask: all) and gt < n_cl -- ``Metric_mIoU.hist_info`` after
    ``add_batch``'s masking.  ``pred``: uint8 or int64 labels, ``gt`` / ``mask`` uint8,
    all of one shape, contiguous.  ``hist`` (n_cl, n_cl) int64 is accumulated into (a
    new zero one by default) and returned.  A counted voxel whose prediction is outside
    [0, n_cl) lands in no bin and sets ``flag`` (an int32 tensor of one element, if
    given) to 1.  1 <= n_cl <= 64 (the kernel's counters live in LDS), otherwise
    ``VeonHipError`` on either device.  Native on a ROCm device; ``torch.bincount`` on
    the CPU."""
    if pred.dtype not in (torch.uint8, torch.int64) or not pred.is_contiguous():
        raise ValueError('pred must be contiguous uint8 or int64 labels, got %s' % pred.dtype)
    _as_u8(gt, 'gt')
    assert gt.shape == pred.shape, (tuple(gt.shape), tuple(pred.shape))
    if mask is not None:
        _as_u8(mask, 'mask')
        assert mask.shape == pred.shape
    if hist is None:
        hist = torch.zeros((n_cl, n_cl), dtype=torch.int64, device=pred.device)
    assert hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == n_cl * n_cl
    if flag is not None:
        assert flag.dtype == torch.int32 and flag.numel() == 1
    if pred.numel() == 0:
        return hist
    if pred.is_cuda:
        dev = _lib.require_device(pred, gt, mask, hist, flag)
        _lib.launch('veon_occ_confusion', dev, pred, pred.element_size(), gt, mask,
                    pred.numel(), n_cl, hist, flag)
        return hist
    if not 1 <= n_cl <= 64:
        raise _lib.VeonHipError('confusion: n_cl must be in [1, 64], got %d' % n_cl)
    p, g = pred.reshape(-1).long(), gt.reshape(-1).long()
    keep = g < n_cl
    if mask is not None:
        keep &= mask.reshape(-1) != 0
    bad = keep & ((p < 0) | (p >= n_cl))
    if flag is not None and bool(bad.any()):
        flag.fill_(1)
    keep &= ~bad
    hist.view(-1).add_(torch.bincount(n_cl * g[keep] + p[keep], minlength=n_cl * n_cl))
    return hist


# ------------------------------------------------------------- detailed vocabulary
def _group_arg(group):
    return _lib.host_array(group, ctypes.c_uint8)


def occ_grouped_reference(sem_low, bin_low, occ_size, group, n_merged, free_label):
    """The torch form of the grouped tail (``_merge_classes_prob``,
    san_in_veon_entry_temporal.py:273-297, then veon_temporal.py:220-229) and its CPU
    path: ``F.interpolate`` trilinear -> maximum over each run of rows (``torch.max``:
    NaN propagates) -> lowest merged channel that attains the maximum; a voxel with a NaN
    row, a non-finite maximum or softmax(occupancy)[0] <= 0.5 gets ``free_label``.
    -> (merged (B, n_merged, Z, Y, X), bin_up (B, 2, Z, Y, X), labels (B, X, Y, Z) int64)."""
    import torch.nn.functional as F
    group = group_table(group, n_merged, free_label, sem_low.shape[1])
    size = tuple(int(v) for v in occ_size)
    up = F.interpolate(sem_low.float(), size=size, mode='trilinear', align_corners=False)
    bin_up = F.interpolate(bin_low.float(), size=size, mode='trilinear', align_corners=False)
    merged = merge_runs(up, group, n_merged)
    cls, top = lowest_argmax(merged)
    scored = ~torch.isnan(up).any(dim=1) & torch.isfinite(top[:, 0])
    keep = scored & (torch.softmax(bin_up, dim=1)[:, 0] > 0.5)
    labels = torch.where(keep, cls, torch.full_like(cls, free_label))
    return merged, bin_up, labels.permute(0, 3, 2, 1).contiguous()


def occ_labels_grouped(sem_low, bin_low, occ_size, group, n_merged, free_label, gt=None,
                       mask=None, hist=None):
    """``occ_labels`` against a detailed vocabulary: ``sem_low`` (B,K,z,y,x) holds one
    logit row per detailed description, ``group`` (K ints, see ``group_table``) the merged
    channel of each row.  Each run of rows is merged by the maximum of its UPSAMPLED
    values, the label is the lowest merged channel that attains the maximum, and a voxel
    that is not kept (a NaN row, a non-finite maximum, softmax(occupancy)[0] <= 0.5) gets
    ``free_label`` -- the reference's ``_merge_classes_prob`` + ``simple_test`` without
    the K upsampled volumes.  -> labels (B,X,Y,Z) uint8.  With ``gt`` and ``hist`` ((n_cl,
    n_cl) int64, n_cl = max(n_merged, free_label + 1) <= 64) the confusion matrix is added
    to ``hist`` in the same kernel, as in ``occ_labels``.  Native on a ROCm device; the
    torch mirror (``occ_grouped_reference`` + ``confusion``) on the CPU."""
    B, K, zi, yi, xi = sem_low.shape
    group = group_table(group, n_merged, free_label, K, hist is not None)
    n_cl = max(int(n_merged), int(free_label) + 1)
    assert tuple(bin_low.shape) == (B, 2, zi, yi, xi)
    Zo, Yo, Xo = (int(v) for v in occ_size)
    if (gt is None) != (hist is None) or (mask is not None and gt is None):
        raise ValueError('gt and hist are given together; a mask needs both')
    _check_counting(gt, mask, hist, (B, Xo, Yo, Zo), n_cl)
    if not sem_low.is_cuda:
        labels = occ_grouped_reference(sem_low, bin_low, occ_size, group, n_merged,
                                       free_label)[2].to(torch.uint8)
        if hist is not None:
            confusion(labels, gt, mask, n_cl, hist)
        return labels
    dev = _lib.require_device(sem_low, bin_low, gt, mask, hist)
    return _launch_labels('veon_occ_labels_grouped', dev, sem_low, bin_low, occ_size,
                          (_group_arg(group), int(n_merged), int(free_label)), gt, mask, hist)


def _default_device(device):
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    return device


class _MetricInputs:
    """What ``add_batch`` of both metrics accepts (numpy arrays or tensors, on the host or
    the device, any integer or bool dtype), as tensors on ``self.device`` of the dtypes
    the kernels take; the mask choice of ``use_image_mask`` / ``use_lidar_mask``."""

    def _tensor(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        return t.to(self.device)

    def labels_u8(self, a):
        """Ground truth (or a mask) as contiguous uint8 on the metric's device; a label
        outside [0, 255) -- negative, 300 -- becomes 255 = ignore."""
        t = self._tensor(a)
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        elif t.dtype != torch.uint8:
            t = t.long()      # (int8 cannot hold 255, uint16 has no comparisons)
            t = torch.where((t >= 0) & (t < IGNORE), t, torch.full_like(t, IGNORE)).to(torch.uint8)
        return t.contiguous()

    def mask_u8(self, a):
        t = self._tensor(a)
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        elif t.dtype != torch.uint8:
            t = (t.long() != 0).to(torch.uint8)
        return t.contiguous()

    def select_mask(self, mask_lidar, mask_camera):
        """The mask ``add_batch`` applies (occ_metrics.py:123-131), or None."""
        if self.use_image_mask:
            return mask_camera
        if self.use_lidar_mask:
            return mask_lidar
        return None

    def pred_labels(self, a):
        """Predicted labels as contiguous uint8 or int64 on the metric's device."""
        pred = self._tensor(a)
        if pred.dtype == torch.bool:
            pred = pred.to(torch.uint8)
        elif pred.dtype not in (torch.uint8, torch.int64):
            pred = pred.long()
        return pred.contiguous()

    def batch_inputs(self, semantics_pred, semantics_gt, mask_lidar, mask_camera):
        """-> (pred, gt, mask or None) of one ``add_batch`` call, converted."""
        pred = self.pred_labels(semantics_pred)
        mask = self.select_mask(mask_lidar, mask_camera)
        if mask is None and (self.use_image_mask or self.use_lidar_mask):
            raise ValueError('the metric applies a mask but none was given')
        return pred, self.labels_u8(semantics_gt), None if mask is None else self.mask_u8(mask)


class OccMiouMetric(_MetricInputs):
    """``Metric_mIoU`` (occ_metrics.py:52-147) with the confusion matrix on ``device``.

    ``add_batch`` takes what the reference's takes (numpy arrays or tensors, on the host
    or the device, any integer or bool dtype) and only enqueues work; the kernels of the
    occupancy path can also add into ``hist`` directly (``VeonOccupancyPath.evaluate``).
    ``count_miou`` is the one read-back."""

    def __init__(self, num_classes=18, use_image_mask=True, use_lidar_mask=False,
                 device=None):
        if not 1 <= num_classes <= 64:
            raise ValueError('num_classes must be in [1, 64], got %d' % num_classes)
        self.num_classes = num_classes
        self.use_image_mask, self.use_lidar_mask = use_image_mask, use_lidar_mask
        self.class_names = list(CLASS_NAMES)
        device = _default_device(device)
        self.hist = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)
        self.device = self.hist.device      # with its index: 'cuda' is cuda:0, say
        # set by a counted prediction outside [0, num_classes); read at count_miou
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.cnt = 0

    def reset(self):
        self.hist.zero_()
        self.flag.zero_()
        self.cnt = 0

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar=None, mask_camera=None):
        self.cnt += 1
        pred, gt, mask = self.batch_inputs(semantics_pred, semantics_gt, mask_lidar,
                                           mask_camera)
        confusion(pred, gt, mask, self.num_classes, self.hist, self.flag)

    @staticmethod
    def per_class_iu_of(hist):
        """diag / (row + col - diag) in float64, NaN for a class absent from both."""
        h = np.asarray(hist, dtype=np.float64)
        d = np.diag(h)
        with np.errstate(divide='ignore', invalid='ignore'):
            return d / (h.sum(1) + h.sum(0) - d)

    def _read(self):
        """(hist as numpy, flag) in ONE copy to the host."""
        both = torch.cat([self.hist.view(-1), self.flag.long()]).cpu().numpy()
        return both[:-1].reshape(self.num_classes, self.num_classes), int(both[-1])

    def per_class_iu(self):
        return self.per_class_iu_of(self._read()[0])

    def count_miou(self):
        """-> (class_names, per-class IoU (numpy float64), cnt), as the reference."""
        hist, flag = self._read()
        if flag:
            raise ValueError('a prediction outside [0, %d) was added to the metric'
                             % self.num_classes)
        return self.class_names, self.per_class_iu_of(hist), self.cnt

    def miou(self):
        """The figure the reference prints: nanmean over the first num_classes - 1
        classes (without 'free'), in percent."""
        _, iu, _ = self.count_miou()
        return float(np.nanmean(iu[:self.num_classes - 1]) * 100)

    def all_reduce(self, group=None):
        """Sum ``hist``, the flag and ``cnt`` over the ranks of ``group`` (the
        data-parallel replicas each evaluate a share of the samples)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        cnt = torch.tensor([self.cnt], dtype=torch.int64, device=self.device)
        for t in (self.hist, self.flag, cnt):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.cnt = int(cnt.item())


# ------------------------------------------------------------------------------ F-score
MAX_REACH_XY = 3     # halo columns of the kernel's tile
MAX_Z = 64           # one z column is one 64-bit word
GUARD_BAND = 1e-9    # relative distance to the threshold below which nothing is decided


def fscore_reach(threshold, voxel_size=(0.4, 0.4, 0.4)):
    """The ball ``distance < threshold`` on the voxel lattice as integer reaches.

    Both point sets of ``Metric_FScore`` are voxel centres ``i * voxel + voxel / 2 +
    range_min`` of one lattice (occ_metrics.py:178-188), so the distance between two of
    them depends on their integer offset (dx, dy, dz) alone, and "the nearest point of the
    other set is closer than ``threshold``" (occ_metrics.py:213-227) is "the other set
    holds a voxel at an offset inside the ball".

    -> (R, table): ``table[dx + R, dy + R]`` (numpy int32, (2R+1, 2R+1)) is the largest
    dz >= 0 with (dx vx)^2 + (dy vy)^2 + (dz vz)^2 < threshold^2 in float64, or -1 where
    not even dz = 0 qualifies; R is the largest |dx| or |dy| with an entry >= 0.

    ValueError, on every device, if R > 3 or a reach > 63 (the kernel's halo and word), and
    if any lattice distance of the searched box lies within 1e-9 * threshold of the
    threshold: there the reference's own answer depends on the rounding of its float64
    coordinates (it forms 0.7999999999999972 for the distance 0.8), so there is nothing
    exact to reproduce.  1e-9 is a condition, not a measurement: four orders of magnitude
    above that rounding, far below any margin chosen on purpose."""
    t = float(threshold)
    v = [float(s) for s in voxel_size]
    if len(v) != 3 or not all(s > 0.0 for s in v) or not 0.0 < t < float('inf'):
        raise ValueError('fscore_reach: threshold %r and voxel_size %r must be positive'
                         % (threshold, voxel_size))
    S = MAX_REACH_XY + 1      # one ring further: an entry there means R > 3
    full = np.full((2 * S + 1, 2 * S + 1), -1, np.int64)
    for dx, dy in itertools.product(range(-S, S + 1), repeat=2):
        for dz in range(MAX_Z + 1):
            d2 = (dx * v[0]) ** 2 + (dy * v[1]) ** 2 + (dz * v[2]) ** 2
            if abs(d2 ** 0.5 - t) <= GUARD_BAND * t:
                raise ValueError(
                    'fscore_reach: the lattice distance %.17g at offset (%d, %d, %d) is within '
                    '%g of the threshold %.17g: which side it falls on depends on the '
                    'rounding of the voxel centres' % (d2 ** 0.5, dx, dy, dz, GUARD_BAND, t))
            if d2 < t * t:
                full[dx + S, dy + S] = dz
    near = np.argwhere(full >= 0) - S
    R = int(np.abs(near).max())       # (0, 0) always qualifies
    if R > MAX_REACH_XY:
        raise ValueError('fscore_reach: threshold %g reaches more than %d voxels in x or y'
                         % (t, MAX_REACH_XY))
    if int(full.max()) >= MAX_Z:
        raise ValueError('fscore_reach: threshold %g reaches %d or more voxels in z; at most '
                         '%d' % (t, MAX_Z, MAX_Z - 1))
    return R, np.ascontiguousarray(full[S - R:S + R + 1, S - R:S + R + 1].astype(np.int32))


DEFAULT_REACH = fscore_reach(0.6)     # the reference's defaults: offsets with d.d <= 2


def _reach_arg(reach, what):
    R, table = reach
    table = np.ascontiguousarray(table, dtype=np.int32)
    if not 0 <= R <= MAX_REACH_XY or table.shape != (2 * R + 1, 2 * R + 1):
        raise ValueError('%s: R must be in [0, %d] with a (2R+1, 2R+1) table, got R = %r and '
                         'shape %r' % (what, MAX_REACH_XY, R, table.shape))
    if int(table.min()) < -1 or int(table.max()) >= MAX_Z:
        raise ValueError('%s: reaches must be in [-1, %d]' % (what, MAX_Z - 1))
    return int(R), table


def _void_words(void):
    """The void labels as four 64-bit words (bit v % 64 of word v // 64), as Python ints."""
    words = [0, 0, 0, 0]
    for v in void:
        v = int(v)
        if not 0 <= v <= 255:
            raise ValueError('void labels must be in [0, 255], got %d' % v)
        words[v >> 6] |= 1 << (v & 63)
    return words


@functools.lru_cache(maxsize=64)
def _launch_tables(void, r_acc, acc_bytes, r_cmpl, cmpl_bytes):
    """The host arrays of one ``veon_occ_fscore_counts`` launch -- the void words and the
    two reach tables, checked -- built once per configuration: the call is about as long
    as its kernel.  -> (void words, r_acc, table, r_cmpl, table) as ctypes arrays / ints."""
    words = _void_words(void)
    vw = (ctypes.c_int64 * 4)(*[w - (1 << 64) if w >> 63 else w for w in words])
    out = [vw]
    for what, R, raw in (('reach_acc', r_acc, acc_bytes), ('reach_cmpl', r_cmpl, cmpl_bytes)):
        table = np.frombuffer(raw, dtype=np.int32)
        side = 2 * R + 1
        R, table = _reach_arg((R, table.reshape(side, side) if table.size == side * side
                               else table), what)
        out += [R, (ctypes.c_int * table.size)(*table.reshape(-1).tolist())]
    return tuple(out)


def _near(occ, reach):
    """occ (B,X,Y,Z) bool -> bool of the same shape: a voxel of ``occ`` lies within the
    reach table of this voxel.  Pad with empty voxels, shift, OR."""
    R, table = reach
    B, X, Y, Z = occ.shape
    rz = max(int(table.max()), 0)
    padded = torch.nn.functional.pad(occ, (rz, rz, R, R, R, R))
    out = torch.zeros_like(occ)
    for dx in range(-R, R + 1):
        for dy in range(-R, R + 1):
            for dz in range(-int(table[dx + R, dy + R]), int(table[dx + R, dy + R]) + 1):
                out |= padded[:, R + dx:R + dx + X, R + dy:R + dy + Y, rz + dz:rz + dz + Z]
    return out


def fscore_counts_torch(pred, gt, mask, void, reach_acc, reach_cmpl):
    """The torch mirror of the kernel (any device): -> (B, 4) int64."""
    lut = torch.zeros(256, dtype=torch.bool)
    lut[[int(v) for v in void]] = True
    lut = lut.to(pred.device)
    p = pred.long()
    occ_p = ((p < 0) | (p > 255)) | ~lut[p.clamp(0, 255)]
    occ_g = ~lut[gt.long()]
    if mask is not None:
        occ_p &= mask != 0
        occ_g &= mask != 0
    cols = [occ_p, occ_g, occ_p & _near(occ_g, reach_acc), occ_g & _near(occ_p, reach_cmpl)]
    return torch.stack([c.sum(dim=(1, 2, 3)) for c in cols], dim=1)


def fscore_counts(pred, gt, mask=None, void=(17, 255), reach_acc=DEFAULT_REACH,
                  reach_cmpl=DEFAULT_REACH, out=None):
    """-> int64 (B, 4): n_pred, n_gt, hit_pred, hit_gt per sample -- all that
    ``Metric_FScore.add_batch`` (occ_metrics.py:190-233) needs of a sample.  With ``out``
    ((B, 4) int64, contiguous) the counts are ADDED to it and it is returned.

    ``pred``: contiguous uint8 or int64 labels, ``gt`` / ``mask``: contiguous uint8, all
    (B, X, Y, Z) or (X, Y, Z); Z <= 64, otherwise ``VeonHipError`` on either device.  A
    voxel is occupied when its label is not in ``void`` (labels in [0, 255]; an int64
    prediction outside that range equals none of them and is occupied, as under the
    reference's ``==``) and its mask is not 0: the mask voids both volumes, as the
    reference's ``add_batch`` does by writing 255 into them.  The reference thereby
    CHANGES its arguments; nothing is written to the inputs here.  n_pred / n_gt: occupied
    voxels; hit_pred: occupied predicted voxels with an occupied ground-truth voxel inside
    ``reach_acc`` (an ``(R, table)`` of ``fscore_reach``); hit_gt: the same the other way
    round with ``reach_cmpl``.  Voxels outside the sample's grid are empty.  Native on a
    ROCm device (csrc/occ_fscore.hip: one launch, nothing allocated but a missing ``out``,
    nothing read back); the torch mirror on the CPU."""
    if pred.dtype not in (torch.uint8, torch.int64) or not pred.is_contiguous():
        raise ValueError('pred must be contiguous uint8 or int64 labels, got %s' % pred.dtype)
    _as_u8(gt, 'gt')
    if pred.dim() not in (3, 4):
        raise ValueError('pred must be (B, X, Y, Z) or (X, Y, Z), got %r' % (tuple(pred.shape),))
    assert gt.shape == pred.shape, (tuple(gt.shape), tuple(pred.shape))
    if mask is not None:
        _as_u8(mask, 'mask')
        assert mask.shape == pred.shape
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None]
        mask = None if mask is None else mask[None]
    B, X, Y, Z = pred.shape
    if Z > MAX_Z:
        raise _lib.VeonHipError('fscore_counts: Z must be at most %d (one z column is one '
                                '64-bit word), got %d' % (MAX_Z, Z))
    if out is None:
        out = torch.zeros((B, 4), dtype=torch.int64, device=pred.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (B, 4)
    if pred.numel() == 0:
        return out
    if pred.is_cuda:
        dev = _lib.require_device(pred, gt, mask, out)
        vw, r_acc, acc, r_cmpl, cmpl = _launch_tables(
            tuple(void), reach_acc[0], np.asarray(reach_acc[1], np.int32).tobytes(),
            reach_cmpl[0], np.asarray(reach_cmpl[1], np.int32).tobytes())
        _lib.launch('veon_occ_fscore_counts', dev, pred, pred.element_size(), gt, mask,
                    B, X, Y, Z, ctypes.addressof(vw), r_acc, ctypes.addressof(acc), r_cmpl,
                    ctypes.addressof(cmpl), out)
        return out
    _void_words(void)
    out += fscore_counts_torch(pred, gt, mask, void, _reach_arg(reach_acc, 'reach_acc'),
                               _reach_arg(reach_cmpl, 'reach_cmpl'))
    return out


class OccFScoreMetric(_MetricInputs):
    """``Metric_FScore`` (occ_metrics.py:150-237) with the per-sample counts on ``device``.

    The constructor takes the reference's arguments; ``leaf_size`` (of its KD-trees) and
    ``range`` (a translation, which cancels in every distance) are accepted and unused.
    The thresholds become reach tables at construction (``fscore_reach``: ValueError where
    the lattice makes a threshold undecidable or too wide for the kernel).

    ``add_batch`` takes one sample as the reference's does, or a batch, of the input kinds
    ``OccMiouMetric.add_batch`` takes -- ground truth outside [0, 255) reads 255 -- and
    only enqueues work: the four counts of each sample are appended to a buffer on the
    device.  ``count_fscore`` is the one read-back and does the reference's float64
    arithmetic on the host, sample by sample in the order they were added."""

    def __init__(self, leaf_size=10, threshold_acc=0.6, threshold_complete=0.6,
                 voxel_size=(0.4, 0.4, 0.4), range=(-40, -40, -1, 40, 40, 5.4),
                 void=(17, 255), use_lidar_mask=False, use_image_mask=False, device=None):
        self.leaf_size, self.range = leaf_size, list(range)
        self.threshold_acc, self.threshold_complete = threshold_acc, threshold_complete
        self.voxel_size = list(voxel_size)
        self.void = [int(v) for v in void]
        _void_words(self.void)
        self.use_lidar_mask, self.use_image_mask = use_lidar_mask, use_image_mask
        self.reach_acc = fscore_reach(threshold_acc, self.voxel_size)
        self.reach_cmpl = fscore_reach(threshold_complete, self.voxel_size)
        self.eps = 1e-8
        self.counts = torch.zeros((16, 4), dtype=torch.int64, device=_default_device(device))
        self.device = self.counts.device
        self.cnt = 0

    def reset(self):
        self.counts.zero_()
        self.cnt = 0

    def _rows(self, n):
        """The next ``n`` rows of the buffer, zero; it doubles as needed (device work
        only)."""
        need = self.cnt + n
        if need > self.counts.shape[0]:
            grown = torch.zeros((max(need, 2 * self.counts.shape[0]), 4), dtype=torch.int64,
                                device=self.device)
            grown[:self.cnt] = self.counts[:self.cnt]
            self.counts = grown
        return self.counts[self.cnt:need]

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar=None, mask_camera=None):
        pred, gt, mask = self.batch_inputs(semantics_pred, semantics_gt, mask_lidar,
                                           mask_camera)
        n = pred.shape[0] if pred.dim() == 4 else 1
        fscore_counts(pred, gt, mask, self.void, self.reach_acc, self.reach_cmpl,
                      out=self._rows(n))
        self.cnt += n

    def sample_counts(self):
        """(cnt, 4) int64 numpy: n_pred, n_gt, hit_pred, hit_gt of every sample added."""
        return self.counts[:self.cnt].cpu().numpy()

    def _per_sample(self, counts):
        bad = int(((counts[:, 0] > 0) & (counts[:, 1] == 0)).sum())
        if bad:
            raise ValueError('%d sample(s) with an occupied prediction and an empty ground '
                             'truth were added: the F-score is undefined there (the '
                             "reference's KD-tree raises)" % bad)
        rows = []
        for n_pred, n_gt, hit_pred, hit_gt in counts.tolist():
            if n_pred == 0:                  # occ_metrics.py:207-210
                rows.append((0.0, 0.0, 0.0))
                continue
            acc, cmpl = hit_pred / n_pred, hit_gt / n_gt      # the means of 0/1 masks
            rows.append((acc, cmpl, 2.0 / (1 / (acc + self.eps) + 1 / (cmpl + self.eps))))
        return rows

    def per_sample(self):
        """(cnt, 3) float64 numpy: accuracy, completeness, F-score of every sample."""
        return np.array(self._per_sample(self.sample_counts()), np.float64).reshape(-1, 3)

    def sums(self):
        """-> (tot_acc, tot_cmpl, tot_f1_mean) of the reference: plain running sums in
        the order of the samples (no compensated summation: bit for bit the reference's)."""
        tot_acc = tot_cmpl = tot_f1_mean = 0.0
        for acc, cmpl, f in self._per_sample(self.sample_counts()):
            tot_acc += acc
            tot_cmpl += cmpl
            tot_f1_mean += f
        return tot_acc, tot_cmpl, tot_f1_mean

    def count_fscore(self):
        """-> (accuracy, completeness, fscore, cnt): the means over the samples; the
        reference prints the third (occ_metrics.py:235-237)."""
        if self.cnt == 0:
            raise ValueError('no sample was added to the metric')
        tot_acc, tot_cmpl, tot_f1_mean = self.sums()
        return tot_acc / self.cnt, tot_cmpl / self.cnt, tot_f1_mean / self.cnt, self.cnt

    def all_reduce(self, group=None):
        """All-gather the per-sample counts over the ranks of ``group``, in rank order
        (padded to the longest rank for the collective): afterwards every rank holds
        every sample, and so the same means."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(group)
        n = torch.tensor([self.cnt], dtype=torch.int64, device=self.device)
        ns = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(ns, n, group=group)
        ns = [int(v) for v in torch.cat(ns).tolist()]
        longest = max(ns)
        own = torch.zeros((longest, 4), dtype=torch.int64, device=self.device)
        own[:self.cnt] = self.counts[:self.cnt]
        parts = [torch.zeros_like(own) for _ in range(world)]
        dist.all_gather(parts, own, group=group)
        self.counts = torch.cat([p[:k] for p, k in zip(parts, ns)] +
                                [torch.zeros((16, 4), dtype=torch.int64, device=self.device)])
        self.cnt = sum(ns)
