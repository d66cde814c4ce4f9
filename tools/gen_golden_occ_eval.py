#!/usr/bin/env python
"""Fixture of the on-device mIoU: tests/golden/occ_eval_tiny.npz.

    python tools/gen_golden_occ_eval.py        (CPU; needs the reference tree)

Loads the reference's own ``Metric_mIoU`` (mmdet3d/datasets/occ_metrics.py) unmodified
through ``oracle.tools.ref_import.load`` (``termcolor`` is not installed: a name-only stub
stands in for it) and feeds it three seeded samples of (6, 5, 4) voxels in each of its
three mask modes.  Predictions are uint8 in 0..17; the ground truth holds 0..17 and some
255 (ignore); classes 2 and 9 occur in neither, so their IoU is NaN.  Data only:

    pred, gt                  (3, 6, 5, 4) uint8
    mask_lidar, mask_camera   (3, 6, 5, 4) bool
    <mode>_hist               (18, 18) float64, after add_batch of the three samples
    <mode>_iou                (18,) float64: count_miou()[1]
    <mode>_cnt                mode in {image, lidar, none}
    class_names               the metric's 18 names"""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.tools import ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'occ_eval_tiny.npz')
SHAPE, N, SEED, ABSENT = (6, 5, 4), 3, 11, (2, 9)
MODES = {'image': dict(use_image_mask=True, use_lidar_mask=False),
         'lidar': dict(use_image_mask=False, use_lidar_mask=True),
         'none': dict(use_image_mask=False, use_lidar_mask=False)}


def make_inputs():
    rng = np.random.RandomState(SEED)
    present = np.array([c for c in range(18) if c not in ABSENT], np.uint8)
    pred = present[rng.randint(0, len(present), (N,) + SHAPE)]
    gt = present[rng.randint(0, len(present), (N,) + SHAPE)]
    gt = np.where(rng.rand(N, *SHAPE) < 0.5, pred, gt)        # some voxels are right
    gt = np.where(rng.rand(N, *SHAPE) < 0.1, 255, gt).astype(np.uint8)
    mask_lidar = rng.rand(N, *SHAPE) < 0.6
    mask_camera = rng.rand(N, *SHAPE) < 0.7
    return pred, gt, mask_lidar, mask_camera


def main():
    stub = types.ModuleType('termcolor')
    stub.colored = None
    sys.modules.setdefault('termcolor', stub)
    ref = ref_import.load('mmdet3d/datasets/occ_metrics.py', 'ref_occ_metrics')
    pred, gt, mask_lidar, mask_camera = make_inputs()
    assert (gt == 255).any() and not np.isin(pred, ABSENT).any() and not np.isin(gt, ABSENT).any()
    out = dict(pred=pred, gt=gt, mask_lidar=mask_lidar, mask_camera=mask_camera)
    for mode, kw in MODES.items():
        m = ref.Metric_mIoU(num_classes=18, **kw)
        for i in range(N):
            m.add_batch(pred[i], gt[i], mask_lidar[i], mask_camera[i])
        with contextlib.redirect_stdout(io.StringIO()):
            names, iou, cnt = m.count_miou()
        assert np.isnan(iou[list(ABSENT)]).all() and np.isfinite(np.delete(iou, ABSENT)).all()
        out[mode + '_hist'], out[mode + '_iou'], out[mode + '_cnt'] = m.hist, iou, np.int64(cnt)
        out['class_names'] = np.array(names)
        print('%-5s: %d voxels counted, mIoU %.4f' % (mode, int(m.hist.sum()),
                                                      np.nanmean(iou[:17]) * 100))
    np.savez(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
