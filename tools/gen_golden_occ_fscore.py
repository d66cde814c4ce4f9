#!/usr/bin/env python
"""Fixture of the on-device F-score: tests/golden/occ_fscore_tiny.npz.

    python tools/gen_golden_occ_fscore.py      (CPU; needs the reference tree and sklearn)

Loads the reference's own ``Metric_FScore`` (mmdet3d/datasets/occ_metrics.py:150-237)
unmodified through ``oracle.tools.ref_import.load`` (``termcolor`` is not installed: a
name-only stub stands in for it) and feeds it four seeded samples of (9, 7, 5) voxels in
each of its three mask modes and in three configurations.  It is given COPIES: its
``add_batch`` writes 255 into the masked voxels of its arguments.  Sample 2 predicts
nothing but void; the ground truth holds some 255.  Data only:

    pred, gt                  (4, 9, 7, 5) uint8
    mask_lidar, mask_camera   (4, 9, 7, 5) bool
    configs                   the configurations' names
    <cfg>_threshold_acc, <cfg>_threshold_complete, <cfg>_voxel_size
    <cfg>_nearest             the lattice distances nearest to the two thresholds
    <cfg>_<mode>_tot          (4, 3) float64: tot_acc, tot_cmpl, tot_f1_mean after each
                              add_batch; mode in {image, lidar, none}
    <cfg>_<mode>_counts       (4, 4) int64: n_pred, n_gt, hit_pred, hit_gt per sample --
                              the sizes of the reference's point sets and the integers
                              whose ratios its per-sample means are (asserted: exactly)

Configurations: ``default`` (voxel 0.4, both thresholds 0.6: offsets up to one voxel);
``r2`` (thresholds 0.45 / 0.9: two voxels; the lattice distance 0.8944 lies 0.6 % below
0.9); ``aniso`` (voxel [0.5, 0.4, 0.2], thresholds 0.62 / 0.7 -- 0.6 IS a lattice distance
of that voxel, three steps in z, so the accuracy threshold stands 3 % above it).  No
lattice distance may lie within 1e-6 (relative) of a threshold: asserted below."""
import itertools
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.tools import ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'occ_fscore_tiny.npz')
SHAPE, N, SEED, ALL_VOID = (9, 7, 5), 4, 23, 2
MODES = {'image': dict(use_image_mask=True, use_lidar_mask=False),
         'lidar': dict(use_image_mask=False, use_lidar_mask=True),
         'none': dict(use_image_mask=False, use_lidar_mask=False)}
CONFIGS = {'default': dict(threshold_acc=0.6, threshold_complete=0.6,
                           voxel_size=[0.4, 0.4, 0.4]),
           'r2': dict(threshold_acc=0.45, threshold_complete=0.9, voxel_size=[0.4, 0.4, 0.4]),
           'aniso': dict(threshold_acc=0.62, threshold_complete=0.7,
                         voxel_size=[0.5, 0.4, 0.2])}
MARGIN = 1e-6


def make_inputs():
    rng = np.random.RandomState(SEED)
    pred = np.where(rng.rand(N, *SHAPE) < 0.25, rng.randint(0, 17, (N,) + SHAPE), 17)
    gt = np.where(rng.rand(N, *SHAPE) < 0.25, rng.randint(0, 17, (N,) + SHAPE), 17)
    gt = np.where(rng.rand(N, *SHAPE) < 0.08, 255, gt)
    pred[ALL_VOID] = 17
    mask_lidar = rng.rand(N, *SHAPE) < 0.6
    mask_camera = rng.rand(N, *SHAPE) < 0.7
    return pred.astype(np.uint8), gt.astype(np.uint8), mask_lidar, mask_camera


def nearest_lattice_distance(threshold, voxel):
    """The distance between two voxel centres that is nearest to ``threshold``."""
    best = None
    for d in itertools.product(range(0, 9), range(0, 9), range(0, 17)):
        dist = float(np.sqrt(sum((k * v) ** 2 for k, v in zip(d, voxel))))
        if best is None or abs(dist - threshold) < abs(best - threshold):
            best = dist
    return best


def main():
    stub = types.ModuleType('termcolor')
    stub.colored = None
    sys.modules.setdefault('termcolor', stub)
    ref = ref_import.load('mmdet3d/datasets/occ_metrics.py', 'ref_occ_metrics')
    pred, gt, mask_lidar, mask_camera = make_inputs()
    assert (gt == 255).any() and (pred[ALL_VOID] == 17).all()
    out = dict(pred=pred, gt=gt, mask_lidar=mask_lidar, mask_camera=mask_camera,
               configs=np.array(sorted(CONFIGS)))
    for cfg, kw in CONFIGS.items():
        near = [nearest_lattice_distance(kw[k], kw['voxel_size'])
                for k in ('threshold_acc', 'threshold_complete')]
        for k, d in zip(('threshold_acc', 'threshold_complete'), near):
            assert abs(d - kw[k]) > MARGIN * kw[k], (cfg, k, d)
            out['%s_%s' % (cfg, k)] = np.float64(kw[k])
        out[cfg + '_voxel_size'] = np.array(kw['voxel_size'], np.float64)
        out[cfg + '_nearest'] = np.array(near, np.float64)
        for mode, mkw in MODES.items():
            m = ref.Metric_FScore(**kw, **mkw)
            tot, counts = [], []
            for i in range(N):
                before = (m.tot_acc, m.tot_cmpl, m.tot_f1_mean)
                p, g = pred[i].copy(), gt[i].copy()
                m.add_batch(p, g, mask_lidar[i].copy(), mask_camera[i].copy())
                tot.append((m.tot_acc, m.tot_cmpl, m.tot_f1_mean))
                # p and g now hold the masked volumes: the sizes of the two point sets
                n_pred, n_gt = len(m.voxel2points(p)), len(m.voxel2points(g))
                if i == ALL_VOID:
                    assert n_pred == 0 and tot[-1] == before
                    counts.append((0, n_gt, 0, 0))
                    continue
                assert n_pred > 0 and n_gt > 0
                # the sample's own means stand alone only in a total that was zero: feed
                # the sample to a fresh metric
                one = ref.Metric_FScore(**kw, **mkw)
                one.add_batch(pred[i].copy(), gt[i].copy(), mask_lidar[i].copy(),
                              mask_camera[i].copy())
                hit_pred, hit_gt = round(one.tot_acc * n_pred), round(one.tot_cmpl * n_gt)
                assert hit_pred / n_pred == one.tot_acc and hit_gt / n_gt == one.tot_cmpl
                counts.append((n_pred, n_gt, hit_pred, hit_gt))
            assert m.cnt == N
            out['%s_%s_tot' % (cfg, mode)] = np.array(tot, np.float64)
            out['%s_%s_counts' % (cfg, mode)] = np.array(counts, np.int64)
            print('%-7s %-5s: F %.6f, counts %s' % (cfg, mode, m.tot_f1_mean / m.cnt,
                                                     np.array(counts).tolist()))
        print('%-7s nearest lattice distances %s' % (cfg, near))
    np.savez(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
