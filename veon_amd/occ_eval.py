"""On-device Occ3D evaluation: the mIoU of the reference's ``Metric_mIoU``
(mmdet3d/datasets/occ_metrics.py:52-147), which is the one metric its
``NuScenesDatasetOccpancy.evaluate`` computes.

    occ_labels   the label-only tail of the occupancy path (csrc/occ_eval.hip): uint8
                 labels as ``VEONTemporal.simple_test`` returns them, nothing else
                 written; optionally the confusion matrix in the same kernel
    confusion    the same confusion matrix for labels that already exist
    OccMiouMetric  ``Metric_mIoU`` with its state (an int64 histogram) on the device:
                 ``add_batch`` never synchronises, ``count_miou`` reads back once

The F-score (``Metric_FScore``: a KD-tree nearest-neighbour search per sample) is not
provided; ``evaluate`` of the reference does not call it.
"""
import ctypes

import numpy as np
import torch

from . import _lib

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
    for name, t in (('gt', gt), ('mask', mask)):
        if t is not None:
            _as_u8(t, name)
            assert tuple(t.shape) == (B, Xo, Yo, Zo), (name, tuple(t.shape))
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.is_contiguous()
        assert hist.numel() == (Q + 1) * (Q + 1), (tuple(hist.shape), Q)
    labels = torch.empty((B, Xo, Yo, Zo), dtype=torch.uint8, device=dev)
    s5 = ctypes.c_int64 * 5
    ss, bs = s5(*sem_low.stride()), s5(*bin_low.stride())
    _lib.launch('veon_occ_labels', dev, sem_low, ctypes.cast(ss, ctypes.c_void_p), Q,
                bin_low, ctypes.cast(bs, ctypes.c_void_p), B, zi, yi, xi, Zo, Yo, Xo,
                labels, gt, mask, hist)
    return labels


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


class OccMiouMetric:
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
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.hist = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)
        self.device = self.hist.device      # with its index: 'cuda' is cuda:0, say
        # set by a counted prediction outside [0, num_classes); read at count_miou
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.cnt = 0

    def reset(self):
        self.hist.zero_()
        self.flag.zero_()
        self.cnt = 0

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

    def add_batch(self, semantics_pred, semantics_gt, mask_lidar=None, mask_camera=None):
        self.cnt += 1
        pred = self._tensor(semantics_pred)
        if pred.dtype == torch.bool:
            pred = pred.to(torch.uint8)
        elif pred.dtype not in (torch.uint8, torch.int64):
            pred = pred.long()
        mask = self.select_mask(mask_lidar, mask_camera)
        if mask is None and (self.use_image_mask or self.use_lidar_mask):
            raise ValueError('the metric applies a mask but none was given')
        confusion(pred.contiguous(), self.labels_u8(semantics_gt),
                  None if mask is None else self.mask_u8(mask), self.num_classes,
                  self.hist, self.flag)

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
