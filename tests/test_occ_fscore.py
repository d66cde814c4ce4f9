"""``veon_amd.occ_eval.OccFScoreMetric`` and ``fscore_counts`` on the CPU against the
reference's own ``Metric_FScore`` (mmdet3d/datasets/occ_metrics.py:150-237), recorded by
tools/gen_golden_occ_fscore.py in tests/golden/occ_fscore_tiny.npz (four samples, one of
them predicting only void, three mask modes, three configurations), and against an
independent float64 brute force over all pairs of voxel centres."""
import os

import numpy as np
import pytest
import torch

from veon_amd import _lib
from veon_amd.occ_eval import (DEFAULT_REACH, OccFScoreMetric, fscore_counts,
                               fscore_reach)

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'occ_fscore_tiny.npz')
MODES = {'image': dict(use_image_mask=True, use_lidar_mask=False),
         'lidar': dict(use_image_mask=False, use_lidar_mask=True),
         'none': dict(use_image_mask=False, use_lidar_mask=False)}
CONFIGS = ['aniso', 'default', 'r2']


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def config_kw(gold, cfg):
    return dict(threshold_acc=float(gold[cfg + '_threshold_acc']),
                threshold_complete=float(gold[cfg + '_threshold_complete']),
                voxel_size=gold[cfg + '_voxel_size'].tolist())


def fill(metric, gold, conv=lambda a: a, samples=None):
    for i in (range(gold['pred'].shape[0]) if samples is None else samples):
        metric.add_batch(conv(gold['pred'][i]), conv(gold['gt'][i]),
                         conv(gold['mask_lidar'][i]), conv(gold['mask_camera'][i]))
    return metric


def check_against_fixture(metric_of, gold, cfg, mode):
    """``metric_of(n)``: the metric after the first n samples.  Counts as integers, the
    per-sample values and the running totals with == in float64: they are the same IEEE
    operations on the same integers."""
    want_counts, want_tot = gold['%s_%s_counts' % (cfg, mode)], gold['%s_%s_tot' % (cfg, mode)]
    n = want_counts.shape[0]
    m = metric_of(n)
    counts = m.sample_counts()
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts)
    per = m.per_sample()
    assert per.dtype == np.float64 and per.shape == (n, 3)
    steps = np.diff(np.concatenate([np.zeros((1, 3)), want_tot]), axis=0)
    assert np.array_equal(per[0], steps[0])          # (later differences are rounded)
    void = int(np.flatnonzero(want_counts[:, 0] == 0)[0])
    assert np.array_equal(per[void], [0.0, 0.0, 0.0]) and want_counts[void, 1] > 0
    for k in range(1, n + 1):
        assert metric_of(k).sums() == tuple(want_tot[k - 1]), (cfg, mode, k)
    acc, cmpl, f, cnt = m.count_fscore()
    assert cnt == m.cnt == n
    assert (acc, cmpl, f) == tuple(want_tot[-1] / n)


@pytest.mark.parametrize('cfg', CONFIGS)
@pytest.mark.parametrize('mode', sorted(MODES))
def test_metric_equals_the_reference(gold, mode, cfg):
    assert sorted(gold['configs']) == CONFIGS

    def metric_of(n):
        m = OccFScoreMetric(device='cpu', **config_kw(gold, cfg), **MODES[mode])
        return fill(m, gold, samples=range(n))
    check_against_fixture(metric_of, gold, cfg, mode)


def test_batches_and_single_samples_give_the_same_counts(gold):
    m = OccFScoreMetric(device='cpu', use_image_mask=True)
    m.add_batch(gold['pred'][:3], gold['gt'][:3], None, gold['mask_camera'][:3])
    m.add_batch(gold['pred'][3], gold['gt'][3], None, gold['mask_camera'][3])
    assert m.cnt == 4 and np.array_equal(m.sample_counts(), gold['default_image_counts'])
    # more samples than the buffer first holds
    many = OccFScoreMetric(device='cpu', use_image_mask=True)
    for _ in range(9):
        fill(many, gold)
    assert many.cnt == 36
    assert np.array_equal(many.sample_counts(), np.tile(gold['default_image_counts'], (9, 1)))


def test_the_default_reaches():
    R, table = fscore_reach(0.6, [0.4, 0.4, 0.4])
    assert R == 1 and table.tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert DEFAULT_REACH[0] == 1 and np.array_equal(DEFAULT_REACH[1], table)
    R, table = fscore_reach(0.9, [0.4, 0.4, 0.4])      # dx^2 + dy^2 + dz^2 <= 5
    assert R == 2 and table[2].tolist() == [1, 2, 2, 2, 1] and table[0].tolist() == [-1, 0, 1, 0, -1]
    assert np.array_equal(table, table.T)
    R, table = fscore_reach(0.3, [0.4, 0.4, 0.4])      # the voxel itself only
    assert R == 0 and table.tolist() == [[0]]
    R, table = fscore_reach(0.7, [0.5, 0.4, 0.2])
    assert R == 1 and table.tolist() == [[1, 2, 1], [2, 3, 2], [1, 2, 1]]


# ------------------------------------------------------------------------- brute force
def brute_counts(pred, gt, mask, void, thr_acc, thr_cmpl, voxel, rng_min=(-40, -40, -1)):
    """All pairwise distances of the voxel centres, formed as the reference forms them
    (occ_metrics.py:184-186), then the minimum, then ``<``."""
    pred, gt = pred.astype(np.int64), gt.astype(np.int64)
    if mask is not None:
        pred[mask == 0] = 255
        gt[mask == 0] = 255

    def points(vol):
        idx = np.where(~np.isin(vol, list(void)))
        return np.stack([idx[k] * voxel[k] + voxel[k] / 2 + rng_min[k] for k in range(3)], axis=1)
    p, g = points(pred), points(gt)
    if len(p) == 0 or len(g) == 0:
        return len(p), len(g), 0, 0
    dist = np.sqrt(((p[:, None, :] - g[None, :, :]) ** 2).sum(-1))
    return len(p), len(g), int((dist.min(1) < thr_acc).sum()), int((dist.min(0) < thr_cmpl).sum())


def volumes(shape, seed, density=0.15):
    rng = np.random.RandomState(seed)
    pred = np.where(rng.rand(*shape) < density, rng.randint(0, 17, shape), 17).astype(np.uint8)
    gt = np.where(rng.rand(*shape) < density, rng.randint(0, 17, shape), 17)
    gt = np.where(rng.rand(*shape) < 0.05, 255, gt).astype(np.uint8)
    mask = (rng.rand(*shape) < 0.7).astype(np.uint8)
    return pred, gt, mask


# thresholds (acc, cmpl) with R = 1, 2, 3 and mixed; voxel sizes
BRUTE = [((0.6, 0.6), [0.4, 0.4, 0.4]), ((0.9, 0.6), [0.4, 0.4, 0.4]),
         ((1.3, 0.9), [0.4, 0.4, 0.4]), ((0.45, 1.3), [0.4, 0.4, 0.4]),
         ((0.62, 0.7), [0.5, 0.4, 0.2]), ((1.1, 1.25), [0.5, 0.4, 0.2])]


@pytest.mark.parametrize('thr,voxel', BRUTE)
def test_mirror_equals_the_brute_force(thr, voxel):
    reach = fscore_reach(thr[0], voxel), fscore_reach(thr[1], voxel)
    assert {fscore_reach(t, [0.4] * 3)[0] for t in (0.6, 0.9, 1.3)} == {1, 2, 3}
    # the wider the reach, the sparser the volume: not every voxel may find a neighbour
    density = {1: 0.12, 2: 0.04, 3: 0.015}[max(reach[0][0], reach[1][0])]
    for seed, shape in enumerate([(12, 11, 9), (5, 9, 3), (1, 1, 6), (7, 1, 1)]):
        for use_mask in (False, True):
            pred, gt, mask = volumes(shape, 40 + seed, density if seed == 0 else 0.3)
            mk = mask if use_mask else None
            want = brute_counts(pred, gt, mk, (17, 255), thr[0], thr[1], voxel)
            got = fscore_counts(torch.from_numpy(pred), torch.from_numpy(gt),
                                None if mk is None else torch.from_numpy(mk),
                                reach_acc=reach[0], reach_cmpl=reach[1])
            assert got.dtype == torch.int64 and got.shape == (1, 4)
            assert tuple(got[0].tolist()) == want, (shape, use_mask)
            assert seed or (0 < want[2] < want[0] and 0 < want[3] < want[1]), want


# -------------------------------------------------------------------------- error cases
def test_undecidable_and_too_wide_thresholds_raise():
    for t in (0.4, 0.8):          # a lattice distance itself
        with pytest.raises(ValueError, match='lattice distance'):
            fscore_reach(t, [0.4, 0.4, 0.4])
        with pytest.raises(ValueError, match='lattice distance'):
            OccFScoreMetric(threshold_acc=t, device='cpu')
        with pytest.raises(ValueError, match='lattice distance'):
            OccFScoreMetric(threshold_complete=t, device='cpu')
    fscore_reach(0.8 * (1 + 1e-8), [0.4, 0.4, 0.4])      # outside the guard band
    with pytest.raises(ValueError, match='lattice distance'):
        fscore_reach(0.8 * (1 + 1e-10), [0.4, 0.4, 0.4])
    assert fscore_reach(1.3, [0.4] * 3)[0] == 3
    with pytest.raises(ValueError, match='x or y'):      # R = 4
        fscore_reach(1.7, [0.4, 0.4, 0.4])
    with pytest.raises(ValueError, match='x or y'):
        fscore_reach(50.0, [0.4, 0.4, 0.4])
    with pytest.raises(ValueError, match='in z'):        # 64 voxels and more in z
        fscore_reach(0.7, [0.4, 0.4, 0.01])
    assert fscore_reach(0.635, [0.4, 0.4, 0.01])[1][1, 1] == 63
    with pytest.raises(ValueError):
        fscore_reach(0.0, [0.4, 0.4, 0.4])


def test_more_than_64_cells_in_z_are_refused():
    pred = torch.zeros((2, 3, 65), dtype=torch.uint8)
    with pytest.raises(_lib.VeonHipError, match='Z'):
        fscore_counts(pred, pred)
    with pytest.raises(_lib.VeonHipError, match='Z'):
        OccFScoreMetric(device='cpu').add_batch(pred.numpy(), pred.numpy(), None, None)
    fits = pred[..., :64].contiguous()
    assert fscore_counts(fits, fits).tolist() == [[384, 384, 384, 384]]


def test_empty_ground_truth_raises_at_count_fscore(gold):
    m = fill(OccFScoreMetric(device='cpu'), gold, samples=[0])
    pred = np.zeros((3, 3, 3), np.uint8)
    empty = np.full((3, 3, 3), 17, np.uint8)
    m.add_batch(pred, empty, None, None)           # not here ...
    m.add_batch(pred, np.full((3, 3, 3), 255, np.uint8), None, None)
    m.add_batch(empty, empty, None, None)          # nothing predicted: zeros, no error
    assert m.cnt == 4
    assert m.sample_counts()[1:].tolist() == [[27, 0, 0, 0], [27, 0, 0, 0], [0, 0, 0, 0]]
    for read in (m.count_fscore, m.sums, m.per_sample):
        with pytest.raises(ValueError, match='2 sample'):
            read()                                 # ... but here
    with pytest.raises(ValueError, match='no sample'):
        OccFScoreMetric(device='cpu').count_fscore()
    both_empty = OccFScoreMetric(device='cpu')
    both_empty.add_batch(empty, empty, None, None)
    assert both_empty.count_fscore() == (0.0, 0.0, 0.0, 1)


# ------------------------------------------------------------------------------ inputs
def test_inputs_are_unchanged(gold):
    arrays = [gold[k][0].copy() for k in ('pred', 'gt', 'mask_lidar', 'mask_camera')]
    tensors = [torch.from_numpy(a.copy()) for a in arrays]
    for mode in MODES.values():
        m = OccFScoreMetric(device='cpu', **mode)
        m.add_batch(*arrays)
        m.add_batch(*tensors)
        m.add_batch(arrays[0].astype(np.int64), *arrays[1:])
    for a, t, k in zip(arrays, tensors, ('pred', 'gt', 'mask_lidar', 'mask_camera')):
        assert np.array_equal(a, gold[k][0]) and np.array_equal(t.numpy(), gold[k][0]), k


def test_input_kinds_give_one_result(gold):
    """The kinds of tests/test_occ_eval.py::test_input_kinds_give_one_histogram."""
    want = gold['default_image_counts']
    gt64 = gold['gt'].astype(np.int64)
    wide = gt64.copy()          # (before any replacement: uint8 cannot hold -1 or 300)
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
        'int8 everything': dict(gold, pred=gold['pred'].astype(np.int8),
                                gt=np.where(wide == 255, -1, wide).astype(np.int8),
                                mask_camera=gold['mask_camera'].astype(np.int8)),
        'uint16 everything': dict(gold, pred=gold['pred'].astype(np.uint16),
                                  gt=np.where(wide == 255, 300, wide).astype(np.uint16),
                                  mask_camera=gold['mask_camera'].astype(np.uint16) * 300),
        'int8 tensors': dict(gold, pred=torch.from_numpy(gold['pred'].astype(np.int8)),
                             gt=torch.from_numpy(np.where(wide == 255, -1, wide)
                                                 .astype(np.int8))),
        'tensor int64 gt': dict(gold, gt=torch.from_numpy(gt64),
                                pred=torch.from_numpy(gold['pred'])),
        'not contiguous': dict(gold, pred=np.asfortranarray(gold['pred']),
                               gt=torch.from_numpy(gold['gt']).transpose(1, 2)
                               .contiguous().transpose(1, 2)),
    }
    for name, data in variants.items():
        m = fill(OccFScoreMetric(device='cpu', use_image_mask=True), data)
        assert np.array_equal(m.sample_counts(), want), name
        assert m.cnt == 4
    with pytest.raises(ValueError, match='mask'):
        OccFScoreMetric(device='cpu', use_image_mask=True).add_batch(
            gold['pred'][0], gold['gt'][0], gold['mask_lidar'][0], None)


def test_int64_predictions_outside_a_byte_are_occupied():
    pred = torch.full((1, 3, 3, 3), 17, dtype=torch.int64)
    gt = torch.full((1, 3, 3, 3), 17, dtype=torch.uint8)
    gt[0, 1, 1, 1] = 4
    assert fscore_counts(pred, gt).tolist() == [[0, 1, 0, 0]]
    pred[0, 0, 1, 1], pred[0, 2, 2, 2] = -1, 300          # one beside the gt voxel, one not
    assert fscore_counts(pred, gt).tolist() == [[2, 1, 1, 1]]
    pred[0, 0, 0, 0] = 255                                # void
    pred[0, 2, 0, 0] = 256 + 17                           # not label 17, and not near
    assert fscore_counts(pred, gt).tolist() == [[3, 1, 1, 1]]
    m = OccFScoreMetric(device='cpu')
    m.add_batch(pred.numpy()[0], gt.numpy()[0], None, None)
    assert m.sample_counts().tolist() == [[3, 1, 1, 1]]
    with pytest.raises(ValueError, match='void'):
        fscore_counts(pred, gt, void=(17, 300))


def test_out_accumulates_and_void_is_a_parameter(gold):
    pred, gt = torch.from_numpy(gold['pred']), torch.from_numpy(gold['gt'])
    mask = torch.from_numpy(gold['mask_camera'].astype(np.uint8))
    once = fscore_counts(pred, gt, mask)
    assert np.array_equal(once.numpy(), gold['default_image_counts'])
    out = once.clone()
    assert fscore_counts(pred, gt, mask, out=out) is out and torch.equal(out, 2 * once)
    assert torch.equal(fscore_counts(pred[1], gt[1], mask[1]), once[1:2])      # (X, Y, Z)
    # 255 not void: the ignored ground truth counts as occupied, the masked voxels do not
    wide = fscore_counts(pred, gt, mask, void=(17,))
    seen = mask != 0
    assert wide[:, 1].tolist() == ((gt != 17) & seen).sum(dim=(1, 2, 3)).tolist()
    assert bool((wide[:, 1] > once[:, 1]).all()) and torch.equal(wide[:, 0], once[:, 0])


def test_reset(gold):
    m = fill(OccFScoreMetric(device='cpu'), gold)
    assert m.cnt == 4
    m.reset()
    assert m.cnt == 0 and m.sample_counts().shape == (0, 4)
    fill(m, gold)
    assert np.array_equal(m.sample_counts(), gold['default_none_counts'])


def test_all_reduce_without_a_group_is_a_no_op(gold):
    m = fill(OccFScoreMetric(device='cpu'), gold)
    m.all_reduce()
    assert m.cnt == 4 and np.array_equal(m.sample_counts(), gold['default_none_counts'])


def test_the_metric_knows_its_device_with_the_index():
    m = OccFScoreMetric(device='cpu')
    assert m.device == m.counts.device == torch.device('cpu')
    assert (m.leaf_size, m.range) == (10, [-40, -40, -1, 40, 40, 5.4])


def test_evaluate_with_both_metrics_on_the_cpu_path():
    """The whole tiny path on the CPU: evaluate() with a list of both metrics returns the
    labels of the single-metric call, leaves the mIoU metric as that call leaves it and
    adds the labels' counts to the F-score metric."""
    from oracle import lss_torch
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    from veon_amd.occ_eval import OccMiouMetric
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
    gen = torch.Generator().manual_seed(4)
    shape = (images.shape[0], net.occ_size[2], net.occ_size[1], net.occ_size[0])
    gt = torch.randint(0, n_cl, shape, generator=gen)
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    mask = torch.rand(shape, generator=gen) >= 0.3
    void = (n_cl - 1, 255)
    alone = OccMiouMetric(num_classes=n_cl, device='cpu')
    want = net.evaluate(images, geom, gt, mask, alone, depth=depth)
    miou = OccMiouMetric(num_classes=n_cl, device='cpu')
    f_mask = OccFScoreMetric(void=void, use_image_mask=True, device='cpu')
    f_all = OccFScoreMetric(void=void, device='cpu')
    labels = net.evaluate(images, geom, gt, mask, [miou, f_mask, f_all], depth=depth)
    assert torch.equal(labels, want)
    assert torch.equal(miou.hist, alone.hist) and miou.cnt == alone.cnt == shape[0]
    gt8 = miou.labels_u8(gt)
    assert torch.equal(f_mask.counts[:shape[0]],
                       fscore_counts(labels, gt8, mask.to(torch.uint8), void))
    assert torch.equal(f_all.counts[:shape[0]], fscore_counts(labels, gt8, None, void))
    assert f_mask.cnt == f_all.cnt == shape[0] and int(f_all.counts[:, 2].sum()) > 0
    only = OccFScoreMetric(void=void, device='cpu')
    assert torch.equal(net.evaluate(images, geom, gt, None, only, depth=depth), want)
    assert torch.equal(only.counts, f_all.counts)
    with pytest.raises(ValueError, match='mask'):
        net.evaluate(images, geom, gt, None, (miou, f_mask), depth=depth)
    with pytest.raises(ValueError, match='at most one'):
        net.evaluate(images, geom, gt, mask, [miou, alone], depth=depth)
    assert torch.equal(miou.hist, alone.hist) and f_mask.cnt == shape[0]


def test_the_header_declares_the_entry_point():
    assert 'veon_occ_fscore_counts' in _lib.declared_symbols()
