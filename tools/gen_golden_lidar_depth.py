#!/usr/bin/env python
"""Fixture of the LiDAR depth render: tests/golden/lidar_depth_tiny.npz.

    python tools/gen_golden_lidar_depth.py        (CPU; needs the reference tree)

Loads the reference's own mmdet3d/datasets/pipelines/loading.py unmodified by path
(``oracle.tools.ref_import.load``), with empty stand-ins for the packages it imports that
are not installed (cv2, mmcv, mmdet, pyquaternion, torchvision and its own sibling
modules): names only, no reference code.  Records the output of
``PointToMultiViewDepth(grid_config, downsample=1).points2depthmap`` for the two seeded
inputs of tests/lidar_depth_refs.py (``FIXTURES``), depth range [1.0, 45.0):

    (a) 32 x 88 map, 4 000 points      (b) 512 x 1408 map, 20 000 points

both uniform over the map plus a 10-pixel margin all round, depth uniform in [0, 60).

Only ``points2depthmap`` is recorded: ``__call__`` needs pyquaternion and the reference's
point-cloud classes, which are absent here.  Its projection lines (:811-820) are pinned by
the fp64 oracle of tests/lidar_depth_refs.py instead.  Data only:

    <case>_points (P, 3) fp32            the input, as it is
    <case>_size   (2,) int64             height, width
    <case>_index  (K,) int64, <case>_value (K,) fp32   the non-zero pixels of the map
    grid (3,) fp64

Also prints, per case, the occupied pixels, the pixels with two or more kept points and the
pixels where the reference's sort key ties between different depths (``tie_pixels``), and
on how many pixels the recorded map differs from the exact minimum."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.tools import ref_import  # noqa: E402
from tests import lidar_depth_refs as refs  # noqa: E402
from veon_amd import lidar_depth  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'lidar_depth_tiny.npz')


class _Registry:
    def register_module(self, *a, **k):
        return lambda cls: cls


def _stub(name, **attrs):
    if name in sys.modules:
        for k, v in attrs.items():
            if not hasattr(sys.modules[name], k):
                setattr(sys.modules[name], k, v)
        return
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


def load_reference_step():
    """-> the reference's PointToMultiViewDepth class."""
    if not os.path.isdir(ref_import.REF):
        raise RuntimeError('reference tree not present at %s' % ref_import.REF)
    blank = type('Blank', (object,), {})
    for name in ('cv2', 'mmcv', 'mmdet', 'mmdet.datasets', 'mmdet3d', 'mmdet3d.core',
                 'mmdet3d.datasets', 'mmdet3d.datasets.pipelines', 'torchvision'):
        _stub(name)
    _stub('pyquaternion', Quaternion=blank)
    _stub('mmdet3d.core.points', BasePoints=blank, get_points_type=None)
    _stub('mmdet3d.core.bbox', LiDARInstance3DBoxes=blank)
    _stub('mmdet.datasets.pipelines', LoadAnnotations=blank, LoadImageFromFile=blank)
    _stub('torchvision.transforms', Compose=blank)
    _stub('mmdet3d.datasets.pipelines.transform_depthanything', Resize=blank,
          NormalizeImage=blank, PrepareForNet=blank)
    _stub('mmdet3d.datasets.builder', PIPELINES=_Registry())
    mod = ref_import.load('mmdet3d/datasets/pipelines/loading.py',
                          'mmdet3d.datasets.pipelines.loading')
    return mod.PointToMultiViewDepth


def main():
    step = load_reference_step()(grid_config={'depth': list(refs.GRID)}, downsample=1)
    lo, hi = refs.GRID[:2]
    out = dict(grid=np.array(refs.GRID, np.float64))
    for case, cfg in refs.FIXTURES.items():
        h, w = cfg['height'], cfg['width']
        pts = refs.fixture_points(cfg['seed'], h, w, cfg['n'])
        ref = step.points2depthmap(pts.clone(), h, w)
        assert ref.shape == (h, w) and ref.dtype == torch.float32
        flat = ref.reshape(-1)
        idx = torch.nonzero(flat)[:, 0]
        out[case + '_points'] = pts.numpy()
        out[case + '_size'] = np.array([h, w], np.int64)
        out[case + '_index'] = idx.numpy()
        out[case + '_value'] = flat[idx].numpy()
        tie, _, occupied, multi = refs.tie_pixels(pts, h, w, lo, hi)
        exact = lidar_depth.points2depthmap_torch(pts, h, w, (lo, hi))
        differ = exact != ref
        assert bool((tie | ~differ).all()), 'a difference outside the tie pixels'
        print('%s: %dx%d, %d points: %d occupied pixels, %d with two or more kept points, '
              '%d tie pixels (%.2f %%), reference != exact minimum on %d'
              % (case, h, w, cfg['n'], int(occupied.sum()), int(multi.sum()), int(tie.sum()),
                 100.0 * int(tie.sum()) / int(occupied.sum()), int(differ.sum())))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
