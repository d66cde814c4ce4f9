#!/usr/bin/env python
"""Fixture of the camera-input preparation: tests/golden/image_inputs_tiny.npz.

    python tools/gen_golden_image_inputs.py        (CPU; needs the reference tree and Pillow)

Loads the reference's own mmdet3d/datasets/pipelines/loading.py unmodified by path
(``oracle.tools.ref_import.load``), with empty stand-ins for the packages it imports that
are not installed (cv2, mmcv, mmdet, pyquaternion, torchvision and its own sibling
modules): names only, no reference code.  Records, from the reference's
``PrepareImageInputs.sample_augmentation`` / ``img_transform`` / ``img_transform_core``
running on the installed Pillow, for the seeded frames of tests/image_inputs_refs.py:

    r<row>_b<b>_c<n>_img     the transformed uint8 image of table row / sample / camera
    r<row>_b<b>_c<n>_depth   its 2:1 ``resize`` (the depth branch's uint8 image)
    r<row>_c<n>_post_rot, _post_tran   (2, 2), (2,) fp32 from ``img_transform``
    strip_img, strip_depth   the 900 x 1600 -> 512 x 1408 window and its 256 x 704 depth
                             resize at the rows / columns of ``refs.STRIP`` only
    aug_<config>_test, aug_<config>_train   rows (resize, newW, newH, x0, y0, x1, y1, flip,
                             rotate) fp64 of ``sample_augmentation`` at 900 x 1600; train:
                             ``AUG_DRAWS`` draws after ``np.random.seed(AUG_SEED)``

The normalised outputs are not recorded: mmcv and cv2 are absent.  Data only.  Also prints,
per row, the share of output bytes at 0 or 255 (both clamps of the resampling occur)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import image_inputs_refs as refs  # noqa: E402
from tools.gen_golden_lidar_depth import _Registry, _stub  # noqa: E402
from oracle.tools import ref_import  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'image_inputs_tiny.npz')


def load_reference_step():
    """-> the reference's PrepareImageInputs class."""
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
    return mod.PrepareImageInputs


def aug_row(aug):
    resize, resize_dims, crop, flip, rotate = aug
    return [resize, *resize_dims, *crop, float(flip), rotate]


def main():
    from PIL import Image
    cls = load_reference_step()
    step = cls(refs.VEON_DATA_CONFIG, is_train=False)
    out = {}
    for row, cfg in sorted(refs.TABLE.items()):
        h, w = cfg['size']
        saturated, total = 0, 0
        for b in range(2 if row == refs.BATCH2_ROW else 1):
            frames = refs.table_frames(row, b + 1)[b]
            for n, (crop, flip) in enumerate(cfg['cams']):
                img, post_rot, post_tran = step.img_transform(
                    Image.fromarray(frames[n]), torch.eye(2), torch.zeros(2),
                    resize=cfg['resize_dims'][0] / w, resize_dims=cfg['resize_dims'],
                    crop=crop, flip=flip, rotate=0)
                key = 'r%d_b%d_c%d' % (row, b, n)
                out[key + '_img'] = np.array(img)
                out[key + '_depth'] = np.array(img.resize(refs.depth_dims(crop)))
                if b == 0:
                    out['r%d_c%d_post_rot' % (row, n)] = post_rot.numpy()
                    out['r%d_c%d_post_tran' % (row, n)] = post_tran.numpy()
                a = out[key + '_img']
                saturated, total = saturated + int(((a == 0) | (a == 255)).sum()), total + a.size
        print('row %d: %.1f %% of the output bytes at 0 or 255' % (row, 100.0 * saturated / total))

    s = refs.STRIP
    img = step.img_transform_core(Image.fromarray(refs.make_frame(s['seed'], *s['size'])),
                                  s['resize_dims'], s['crop'], s['flip'], 0)
    out['strip_img'] = np.array(img)[s['rows']][:, s['cols']]
    depth = np.array(img.resize(refs.depth_dims(s['crop'])))
    out['strip_depth'] = depth[[r // 2 for r in s['rows'][::2]]][:, [c // 2 for c in s['cols'][::2]]]

    for name, config in (('veon', refs.VEON_DATA_CONFIG), ('aug', refs.AUG_DATA_CONFIG)):
        out['aug_%s_test' % name] = np.array(
            [aug_row(cls(config, is_train=False).sample_augmentation(900, 1600))], np.float64)
        np.random.seed(refs.AUG_SEED)
        train = cls(config, is_train=True)
        out['aug_%s_train' % name] = np.array(
            [aug_row(train.sample_augmentation(900, 1600)) for _ in range(refs.AUG_DRAWS)],
            np.float64)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
