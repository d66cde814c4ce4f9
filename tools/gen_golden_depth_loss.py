#!/usr/bin/env python
"""Fixture of the depth pre-training loss: tests/golden/depth_loss_tiny.npz.

    python tools/gen_golden_depth_loss.py        (CPU; needs the reference tree)

Loads the reference's own ``LSSViewTransformerRaw`` (mmdet3d/models/necks/
view_transformer_raw.py) unmodified through ``oracle.tools.ref_import``, builds the seeded
inputs of tests/depth_loss_refs.py (B 1, N 2, 32 x 64 labels, 16 x 32 predictions, depth
grid [1, 45, 0.5], every planted hostile case) once unclipped and once clipped, and for
each runs what ``VeonDepthPretrain.forward_train`` runs: ``downsample_depth`` of the
prediction by 8 and of the label by 16, the mean-absolute-error statistic and
``get_depth_loss_own(gt_ds, pred_ds, zoe, ce)`` for the four (zoe, ce) combinations, with
autograd's gradient of the sum of the returned losses with respect to the prediction.
Data only:

    <case>_depth, <case>_gt_depth                     inputs, case in {unclipped, clipped}
    <case>_depth_error
    <case>_z<zoe>c<ce>_loss_depth_zoe / _loss_depth_ce  (those the combination returns)
    <case>_z<zoe>c<ce>_grad                           (zeros for z0c0: nothing to derive)
    grid, pred_scale, gt_scale"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.tools import ref_import  # noqa: E402
from tests import depth_loss_refs as refs  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'depth_loss_tiny.npz')
GRID = refs.GRIDS[89]
B, N, HG, WG, SP, SG, SEED = 1, 2, 32, 64, 8, 16, 5


def main():
    raw, _ = ref_import.load_view_transformers(lambda *a, **k: None)
    grid_config = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
                   'depth': list(GRID)}
    vt = raw.LSSViewTransformerRaw(grid_config=grid_config, input_size=(HG, WG), downsample=16,
                                   out_channels=8, collapse_z=False, ds_feat=[2, 2, 2])
    out = dict(grid=np.array(GRID, np.float64), pred_scale=np.int64(SP), gt_scale=np.int64(SG))
    for case in ('unclipped', 'clipped'):
        depth, gt = refs.make_inputs(SEED, B, N, HG, WG, GRID, SP, SG, clipped=case == 'clipped')
        out[case + '_depth'], out[case + '_gt_depth'] = depth.numpy(), gt.numpy()
        for zoe in (False, True):
            for ce in (False, True):
                leaf = depth.clone().requires_grad_(True)
                pred_ds = vt.downsample_depth(leaf, downsample=SP)
                gt_ds = vt.downsample_depth(gt, downsample=SG)
                valid = gt_ds.view(-1) < 9225
                err = torch.abs(pred_ds.view(-1)[valid] - gt_ds.view(-1)[valid]).mean()
                losses = vt.get_depth_loss_own(gt_ds, pred_ds, zoe=zoe, ce=ce)
                assert set(losses) == {k for k, on in (('loss_depth_zoe', zoe),
                                                       ('loss_depth_ce', ce)) if on}
                tag = '%s_z%dc%d_' % (case, zoe, ce)
                grad = torch.zeros_like(depth)
                if losses:
                    grad, = torch.autograd.grad(sum(losses.values()), leaf)
                for k, v in losses.items():
                    out[tag + k] = v.detach().numpy()
                out[tag + 'grad'] = grad.numpy()
                out[case + '_depth_error'] = err.detach().numpy()
        z = float(out[case + '_z1c1_loss_depth_zoe'])
        assert (z == 2.0) == (case == 'clipped'), (case, z)
        print('%s: zoe %.6f  ce %.6f  depth_error %.4f  max|grad| %.3e'
              % (case, z, float(out[case + '_z1c1_loss_depth_ce']),
                 float(out[case + '_depth_error']), float(np.abs(out[case + '_z1c1_grad']).max())))
    np.savez(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
