"""``veon_amd.occ_eval.OccMiouMetric`` on the CPU against the reference's own
``Metric_mIoU`` (mmdet3d/datasets/occ_metrics.py:52-147), recorded by
tools/gen_golden_occ_eval.py in tests/golden/occ_eval_tiny.npz: three samples, each
mask mode, two classes absent (NaN IoU), some ground truth 255."""
import os

import numpy as np
import pytest
import torch

from veon_amd.occ_eval import CLASS_NAMES, OccMiouMetric, confusion

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'occ_eval_tiny.npz')
MODES = {'image': dict(use_image_mask=True, use_lidar_mask=False),
         'lidar': dict(use_image_mask=False, use_lidar_mask=True),
         'none': dict(use_image_mask=False, use_lidar_mask=False)}


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _fill(metric, gold, conv=lambda a: a):
    for i in range(gold['pred'].shape[0]):
        metric.add_batch(conv(gold['pred'][i]), conv(gold['gt'][i]),
                         conv(gold['mask_lidar'][i]), conv(gold['mask_camera'][i]))
    return metric


@pytest.mark.parametrize('mode', sorted(MODES))
def test_metric_equals_the_reference(gold, mode):
    m = _fill(OccMiouMetric(device='cpu', **MODES[mode]), gold)
    want_hist, want_iou = gold[mode + '_hist'], gold[mode + '_iou']
    assert m.hist.dtype == torch.int64 and m.hist.shape == (18, 18)
    assert np.array_equal(m.hist.numpy(), want_hist)          # exactly: counts
    names, iou, cnt = m.count_miou()
    assert names == list(gold['class_names']) == CLASS_NAMES
    assert iou.dtype == np.float64
    assert np.isnan(want_iou).sum() == 2 and np.array_equal(np.isnan(iou), np.isnan(want_iou))
    np.testing.assert_allclose(iou, want_iou, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(m.per_class_iu(), want_iou, rtol=0, atol=1e-12, equal_nan=True)
    assert m.miou() == pytest.approx(float(np.nanmean(want_iou[:17]) * 100), abs=1e-10)
    assert cnt == m.cnt == 3 == int(gold[mode + '_cnt'])


def test_input_kinds_give_one_histogram(gold):
    """numpy and tensors, bool and uint8 masks, labels from int8 to int64, and int64
    ground truth whose ignored voxels read -1 or 300 instead of 255."""
    want = gold['image_hist']
    gt64 = gold['gt'].astype(np.int64)
    ign = np.flatnonzero(gt64.reshape(-1) == 255)
    assert len(ign) >= 2
    gt64.reshape(-1)[ign[0::2]] = -1
    gt64.reshape(-1)[ign[1::2]] = 300
    variants = {
        'numpy': dict(gold),
        'tensors': {k: torch.from_numpy(v) for k, v in gold.items() if v.dtype.kind in 'bu'},
        'uint8 masks': dict(gold, mask_camera=gold['mask_camera'].astype(np.uint8) * 7,
                            mask_lidar=gold['mask_lidar'].astype(np.uint8)),
        'int64 pred': dict(gold, pred=gold['pred'].astype(np.int64)),
        'int32 pred, int16 gt': dict(gold, pred=gold['pred'].astype(np.int32),
                                     gt=gold['gt'].astype(np.int16)),
        'int64 gt with -1 and 300': dict(gold, gt=gt64),
        # int8 cannot hold 255: its ignored voxels read -1; uint16 has no comparisons
        'int8 everything': dict(gold, pred=gold['pred'].astype(np.int8),
                                gt=np.where(gold['gt'] == 255, -1, gold['gt']).astype(np.int8),
                                mask_camera=gold['mask_camera'].astype(np.int8)),
        'uint16 everything': dict(gold, pred=gold['pred'].astype(np.uint16),
                                  gt=np.where(gold['gt'] == 255, 300, gold['gt']).astype(np.uint16),
                                  mask_camera=gold['mask_camera'].astype(np.uint16) * 300),
        'int8 tensors': dict(gold, pred=torch.from_numpy(gold['pred'].astype(np.int8)),
                             gt=torch.from_numpy(np.where(gold['gt'] == 255, -1, gold['gt'])
                                                 .astype(np.int8))),
        'tensor int64 gt': dict(gold, gt=torch.from_numpy(gt64),
                                pred=torch.from_numpy(gold['pred'])),
        'not contiguous': dict(gold, pred=np.asfortranarray(gold['pred']),
                               gt=torch.from_numpy(gold['gt']).transpose(1, 2)
                               .contiguous().transpose(1, 2)),
    }
    for name, data in variants.items():
        m = _fill(OccMiouMetric(device='cpu'), data)
        assert np.array_equal(m.hist.numpy(), want), name
        assert m.cnt == 3
        m.count_miou()      # nothing out of range


def test_out_of_range_prediction_raises_at_count_miou(gold):
    m = OccMiouMetric(device='cpu', use_image_mask=False)
    pred, gt = gold['pred'][0].copy(), gold['gt'][0].copy()
    pred[0, 0, 0], gt[0, 0, 0] = 18, 3         # a counted voxel
    m.add_batch(pred, gt, None, None)          # not here ...
    clean = OccMiouMetric(device='cpu', use_image_mask=False)
    pred[0, 0, 0], gt[0, 0, 0] = 17, 255       # the same sample without that voxel
    clean.add_batch(pred, gt, None, None)
    assert torch.equal(m.hist, clean.hist)     # it is in no bin
    with pytest.raises(ValueError, match='outside'):
        m.count_miou()                         # ... but here
    with pytest.raises(ValueError):
        m.miou()
    # where the ground truth is ignored, the prediction is never looked at
    pred[0, 0, 0] = 200
    clean.add_batch(pred, gt, None, None)
    clean.count_miou()
    neg = OccMiouMetric(device='cpu', use_image_mask=False)
    neg.add_batch(np.full((2, 2, 2), -1, np.int64), np.zeros((2, 2, 2), np.uint8), None, None)
    with pytest.raises(ValueError):
        neg.count_miou()


def test_reset(gold):
    m = _fill(OccMiouMetric(device='cpu'), gold)
    m.add_batch(np.full((1,), 18, np.uint8), np.zeros((1,), np.uint8), None, np.ones((1,), bool))
    assert m.cnt == 4 and int(m.hist.sum()) > 0 and int(m.flag) == 1
    m.reset()
    assert m.cnt == 0 and int(m.hist.sum()) == 0 and int(m.flag) == 0
    _fill(m, gold)
    assert np.array_equal(m.hist.numpy(), gold['image_hist'])


def test_hand_computed_three_classes():
    #          voxel   0  1  2  3  4  5    6  7
    pred = np.array([0, 0, 1, 1, 2, 0,   1, 2], np.uint8)
    gt = np.array([0, 1, 1, 1, 2, 255, 0, 2], np.uint8)
    mask = np.array([1, 1, 1, 1, 1, 1,   0, 1], bool)    # voxel 5 ignored, 6 masked
    m = OccMiouMetric(num_classes=3, device='cpu')
    m.add_batch(pred, gt, None, mask)
    assert m.hist.tolist() == [[1, 0, 0], [1, 2, 0], [0, 0, 2]]      # rows: ground truth
    _, iou, cnt = m.count_miou()
    assert iou.tolist() == [1 / 2, 2 / 3, 1.0] and cnt == 1
    assert m.miou() == pytest.approx((1 / 2 + 2 / 3) / 2 * 100, abs=1e-12)   # without the last
    # confusion() alone: no mask, accumulate into a given histogram
    h = confusion(torch.from_numpy(pred), torch.from_numpy(gt), n_cl=3)
    assert h.tolist() == [[1, 1, 0], [1, 2, 0], [0, 0, 2]]
    assert confusion(torch.from_numpy(pred), torch.from_numpy(gt), n_cl=3, hist=h) is h
    assert h.tolist() == [[2, 2, 0], [2, 4, 0], [0, 0, 4]]
    absent = OccMiouMetric(num_classes=3, device='cpu', use_image_mask=False)
    absent.add_batch(np.zeros(4, np.uint8), np.zeros(4, np.uint8), None, None)
    assert np.isnan(absent.per_class_iu()[1:]).all() and absent.miou() == 100.0


def test_labels_only_on_the_cpu_path():
    """labels_only on a tiny CPU path: the default call's labels as uint8 and no logits;
    from_pooled threads the keyword through."""
    from veon_amd.models.veon_occ import VeonOccupancyPath
    torch.manual_seed(0)
    grid = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
            'depth': [1.0, 13.0, 1.0]}
    net = VeonOccupancyPath(input_size=(64, 176), num_cam=2, clip_width=64, clip_layers=4,
                            clip_heads=1, clip_first_tail=2, clip_proj_dim=64, embed_dim=16,
                            n_classes=5, occ_size=(4, 20, 20), hsa_dim=64,
                            hsa_fusion_map=('0->1->1', '1->2->2'), grid_config=grid,
                            bf16_heads=False, two_streams=False, clip_image=64).eval()
    bin_low = torch.randn(2, 2, 2, 10, 10)
    feat = torch.randn(2, 64, 2, 10, 10)
    with torch.no_grad():
        full = net._classify(bin_low, feat)
        only = net._classify(bin_low, feat, labels_only=True)
        feats = net._classify(bin_low, feat, return_features=True, labels_only=True)
    assert set(full) == {'bin_occ', 'sem_occ', 'occ_pred_cls'}
    assert full['occ_pred_cls'].dtype == torch.int64
    assert set(only) == {'occ_pred_cls'}
    assert set(feats) == {'occ_pred_cls', 'feat_low', 'bin_low'}
    assert only['occ_pred_cls'].dtype == torch.uint8
    assert only['occ_pred_cls'].shape == (2, 20, 20, 4)
    assert torch.equal(only['occ_pred_cls'].long(), full['occ_pred_cls'])
    assert torch.equal(feats['occ_pred_cls'], only['occ_pred_cls'])
    assert len(full['occ_pred_cls'].unique()) > 2
    # with grad enabled: the same keys and labels
    again = net._classify(bin_low, feat, labels_only=True)
    assert set(again) == {'occ_pred_cls'} and torch.equal(again['occ_pred_cls'],
                                                          only['occ_pred_cls'])
    # the count of evaluate(), on the torch path: confusion() of the labels
    m = OccMiouMetric(num_classes=6, device='cpu', use_image_mask=False)
    gt = torch.randint(0, 6, (2, 20, 20, 4), dtype=torch.uint8)
    with torch.no_grad():
        net._classify(bin_low, feat, labels_only=True, count=(gt, None, m.hist))
    want = confusion(only['occ_pred_cls'], gt, n_cl=6)
    assert torch.equal(m.hist, want) and int(want.sum()) == gt.numel()


def test_evaluate_and_forward_labels_only_on_the_cpu_path():
    """The whole tiny path (tests/golden/path_tiny) on the CPU: forward(labels_only=True)
    and evaluate() give the default forward's labels, evaluate() adds their confusion
    matrix to the metric and counts the samples."""
    from oracle import lss_torch
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, 'cpu', native=False)
    vt = net.view_transformer

    def cpu_view_transform(input, depth, tran_feat):   # the lift: CPU oracle
        B, N, C, H, W = input[0].shape
        grid = (vt.grid_lower_bound, vt.grid_interval, vt.grid_size)
        cams = (input[1], input[3], input[4], input[5], input[6])
        return lss_torch.lift(vt.frustum, grid, cams, depth.view(B, N, -1, H, W),
                              tran_feat.view(B, N, C, H, W))
    vt.view_transform = cpu_view_transform
    images, geom, depth = _inputs(g, 'cpu')
    n_cl = net.ov_classifier_weight.shape[0] + 1
    with torch.no_grad():
        full = net(images, geom, depth=depth)
        only = net(images, geom, depth=depth, labels_only=True)
    assert set(only) == {'occ_pred_cls'} and only['occ_pred_cls'].dtype == torch.uint8
    assert torch.equal(only['occ_pred_cls'].long(), full['occ_pred_cls'])
    gen = torch.Generator().manual_seed(4)
    shape = full['occ_pred_cls'].shape
    gt = torch.randint(0, n_cl, shape, generator=gen)            # int64, as Occ3D loads it
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    mask = torch.rand(shape, generator=gen) >= 0.3               # bool
    m = OccMiouMetric(num_classes=n_cl, device='cpu')
    labels = net.evaluate(images, geom, gt.numpy(), mask.numpy(), m, depth=depth)
    assert torch.equal(labels, only['occ_pred_cls'])
    assert m.cnt == images.shape[0]
    want = confusion(labels, gt.to(torch.uint8), mask.to(torch.uint8), n_cl)
    assert torch.equal(m.hist, want) and 0 < int(want.sum()) < labels.numel()
    with pytest.raises(ValueError, match='classes'):
        net.evaluate(images, geom, gt, mask, OccMiouMetric(num_classes=n_cl + 1, device='cpu'))
    with pytest.raises(ValueError, match='mask'):
        net.evaluate(images, geom, gt, None, m)


def test_confusion_refuses_more_than_64_classes_on_the_cpu_too():
    from veon_amd._lib import VeonHipError
    pred = torch.zeros(16, dtype=torch.uint8)
    assert int(confusion(pred, pred, None, n_cl=64)[0, 0]) == 16
    for n_cl in (65, 0):
        with pytest.raises(VeonHipError, match='n_cl'):
            confusion(pred, pred, None, n_cl=n_cl)


def test_the_metric_knows_its_device_with_the_index():
    m = OccMiouMetric(device='cpu')
    assert m.device == m.hist.device == m.flag.device == torch.device('cpu')
