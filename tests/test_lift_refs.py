"""CPU pins of tests/lift_refs.py: the references the GPU module
tests/test_lift_prepare_edges_gpu.py compares the index half of the lift with, and the
promises of the case builders on the very inputs that module uses."""
import numpy as np
import pytest
import torch

from tests import lift_refs as lr
from tests.conftest import load_golden

KEYS = ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths')


@pytest.mark.parametrize('name', ['lss_small', 'lss_small_b2', 'lss_mid'])
def test_prepare_ref_reproduces_the_golden_fixtures(name):
    g = load_golden(name)
    out = lr.prepare_ref(g['coor'], g['grid_lower_bound'], g['grid_interval'],
                         g['grid_size'])
    for got, key in zip(out, KEYS):
        assert got.dtype == np.int32 and np.array_equal(got, g[key]), key
    # keep = all True changes nothing; dropping a point removes exactly that point
    keep = np.ones(g['coor'].shape[:-1], bool)
    same = lr.prepare_ref(g['coor'], g['grid_lower_bound'], g['grid_interval'],
                          g['grid_size'], keep)
    assert all(np.array_equal(a, b) for a, b in zip(same, out))
    victim = int(g['ranks_depth'][7])
    keep.reshape(-1)[victim] = False
    less = lr.prepare_ref(g['coor'], g['grid_lower_bound'], g['grid_interval'],
                          g['grid_size'], keep)
    m = g['ranks_depth'] != victim
    assert np.array_equal(less[0], g['ranks_bev'][m])
    assert np.array_equal(less[1], g['ranks_depth'][m])
    assert np.array_equal(less[2], g['ranks_feat'][m])


def test_prepare_ref_drops_non_finite_points_and_returns_empties():
    lower, step, size = lr.axis_grid(4)
    coor = np.zeros((1, 1, 1, 1, 5, 3), np.float32)
    coor[..., 2] = 1.0
    coor[0, 0, 0, 0, :, 0] = [2.5, np.nan, 0.5, np.inf, 2.25]
    coor[0, 0, 0, 0, 2, 1] = np.nan                    # NaN on another axis of a kept x
    rb, rd, rf, st, ln = lr.prepare_ref(coor, lower, step, size)
    assert rb.tolist() == [2, 2] and rd.tolist() == [0, 4] and rf.tolist() == [0, 4]
    assert st.tolist() == [0] and ln.tolist() == [2]
    none = lr.prepare_ref(coor, lower, step, size, keep=np.zeros(5, bool))
    assert len(none) == 5 and all(a.size == 0 and a.dtype == np.int32 for a in none)


def test_vstart_and_plan_refs_on_a_worked_example():
    # 2 batch elements x 128 voxels: tiles [0,64) [64,128) | [128,192) [192,256)
    rb = np.array([0, 0, 63, 64, 64, 64, 130, 255], np.int32)
    st = np.array([0, 2, 3, 6, 7], np.int32)
    vs = lr.vstart_ref(rb, 256)
    assert vs.dtype == np.int32 and vs.size == 257
    assert vs[0] == 0 and vs[1] == 2 and vs[63] == 2 and vs[64] == 3 and vs[65] == 6
    assert vs[130] == 6 and vs[131] == 7 and vs[255] == 7 and vs[256] == 8
    assert (np.diff(vs) >= 0).all() and np.diff(vs).sum() == rb.size
    plan = lr.plan_ref(rb, st, 2, 128)
    assert plan.dtype == np.int32
    assert plan.tolist() == [[0, 2, 0, 3],      # voxels 0 (2 points) and 63
                             [2, 1, 3, 3],      # voxel 64, 3 points
                             [3, 1, 6, 1],      # voxel 130
                             [4, 1, 7, 1]]      # voxel 255
    # empty tiles carry the running counts; nothing kept: all zero
    plan = lr.plan_ref(rb[:6], st[:3], 2, 128)
    assert plan.tolist() == [[0, 2, 0, 3], [2, 1, 3, 3], [3, 0, 6, 0], [3, 0, 6, 0]]
    assert not lr.plan_ref(np.zeros(0, np.int32), np.zeros(0, np.int32), 2, 128).any()
    assert not lr.vstart_ref(np.zeros(0, np.int32), 15).any()


def test_twohot_keep_and_slot_on_a_worked_example():
    D, H, W, K = 6, 1, 2, 4
    # pixel 0: window [1,4), kept [2,4), tail dropped; pixel 1: window [4,6), kept
    # nothing of it, tail kept
    win = np.array([[1 | 3 << 16, 2 | 2 << 16],
                    [4 | 2 << 16, (0 | 0 << 16 | 1 << 31) - (1 << 32)]], np.int32)
    keep, slot = lr.twohot_keep_and_slot(win, D, H, W, K)
    keep, slot = keep.reshape(D, 2), slot.reshape(D, 2)
    assert keep[:, 0].tolist() == [False, False, True, True, False, False]
    assert keep[:, 1].tolist() == [True, True, True, True, False, False]
    assert slot[:, 0].tolist() == [0, 1, 2, 3, 0, 0]
    assert slot[:, 1].tolist() == [4, 4, 4, 4, 5, 6]
    # the same rule as the product's own mirror, on windows it built
    from veon_amd import depth_ops
    g = torch.Generator().manual_seed(5)
    metric = 0.5 + 50.0 * torch.rand(2, 3, 4, 11, generator=g)
    for eps in (0.0, 1e-3):
        tw = depth_ops.two_hot_windows(metric, 44, 1.0, 1.0, 4, eps)
        keep, slot = lr.twohot_keep_and_slot(tw.win.numpy(), 44, 4, 11, tw.K)
        assert np.array_equal(keep, tw.kept().numpy().reshape(-1))
        assert keep.all() == (eps == 0.0) and keep.any()
        assert slot.min() >= 0 and slot.max() < tw.wts.numel()
        dense = tw.dense().numpy().reshape(-1)
        assert np.array_equal(tw.wts.numpy().reshape(-1)[slot], dense)


def test_axis_rig_coordinates_are_exact():
    xs = np.array([0.5, 7.5, -3.5, 1023.5, 3135.5], np.float32)
    shifts = np.array([[0.0, 2.0], [64.0, -1.0]], np.float32)
    rig = lr.axis_rig(xs, 2, shifts, 2)
    assert tuple(rig['frustum'].shape) == (1, 1, 5, 3)
    coor = lr.rig_coor(rig)
    assert tuple(coor.shape) == (2, 2, 1, 1, 5, 3)
    want = xs[None, None] + shifts[:, :, None]
    assert np.array_equal(coor[..., 0].numpy().reshape(2, 2, 5), want)
    assert bool((coor[..., 1] == 0).all()) and bool((coor[..., 2] == 1).all())


def test_face_table_verdicts():
    ft = lr.face_table()
    coor, (lower, step, size) = ft['coor'], ft['grid']
    P = coor.shape[4]
    rb, rd, rf, st, ln = lr.prepare_ref(coor, lower, step, size)
    kept = np.zeros(2 * P, bool)
    kept[rd] = True
    want = lr.float_verdict(coor.numpy().reshape(-1, 3), lower, step, size)
    for i in np.flatnonzero(kept != want):
        raise AssertionError('%s: reference keeps %s' % (ft['labels'][i], kept[i]))
    for i, e in enumerate(ft['expect']):
        assert e is None or kept[i] == e, ft['labels'][i]
    lab = ft['labels']
    for a in 'xyz':
        for name in ('lower', 'lower-step/2', 'lower-0.49step', '-0.0'):
            assert kept[lab.index(a + ':' + name)], (a, name)
        for name in ('lower-step', 'upper', 'nan', '+inf', '-inf', '+1e30', '-1e30',
                     '+3e9step', '-3e9step'):
            assert not kept[lab.index(a + ':' + name)], (a, name)
    assert not kept[lab.index('all:nan')]
    # both batch elements hold the same table, 64 voxels apart
    n = rb.size // 2
    assert np.array_equal(rb[:n] + 64, rb[n:]) and np.array_equal(rd[:n] + P, rd[n:])
    # voxel 0 of every axis is reached from below the lower face (truncation toward 0)
    vox = {lab[i]: int(b) for i, b in zip(rd[:n], rb[:n])}
    mid = 3 + 8 * 1 + 32 * 1
    assert vox['x:lower-step/2'] == mid - 3 and vox['y:lower-step/2'] == mid - 8
    assert vox['z:lower-step/2'] == mid - 32 and vox['x:lower'] == mid - 3


@pytest.mark.parametrize('B,X', lr.SCAN_GRIDS)
def test_scan_cases_hold_their_promises(B, X):
    cases = lr.scan_cases(B, X)
    names = [c['name'].split('-')[1] for c in cases]
    assert names == (['bin0', 'last'] + (['seam'] if B * X > 1024 else [])
                     + ['once', 'second', 'none'])
    for c in cases:
        rb, rd, rf, st, ln = lr.prepare_ref(lr.rig_coor(c['rig']), *c['grid'])
        bins = c['bins']
        order = np.argsort(bins, kind='stable')
        order = order[bins[order] >= 0]
        assert np.array_equal(rb, bins[order]), c['name']
        assert np.array_equal(rd, order) and np.array_equal(rf, order), c['name']
        vs = lr.vstart_ref(rb, c['n_bins'])
        assert np.array_equal(np.diff(vs), np.bincount(rb, minlength=c['n_bins']))


def test_scan_grids_cover_the_stated_seams():
    grids = lr.SCAN_GRIDS
    assert [x for b, x in grids if b == 1 and x % 64 == 0] == \
        [64, 960, 1024, 1088, 2048, 2112, 3136]
    assert (2, 1088) in grids and {x for b, x in grids if x % 64} == {15, 189}


def test_run_cases_hold_their_promises():
    c = lr.run_cases()
    assert c['dims'] == (2, 2, 1, 1, 700)
    ref = lr.prepare_ref(c['coor'], *c['grid'])
    bins = c['bins']
    order = np.argsort(bins, kind='stable')
    order = order[bins[order] >= 0]
    assert np.array_equal(ref[0], bins[order]) and np.array_equal(ref[1], order)
    # the NaN variant drops the same points
    nan = lr.prepare_ref(c['coor_nan'], *c['grid'])
    assert torch.isnan(c['coor_nan']).any(-1).sum() > 20
    assert all(np.array_equal(a, b) for a, b in zip(ref, nan))
    assert ref[4].max() >= 200


@pytest.mark.parametrize('L', lr.LONG_BINS)
def test_long_bin_cases_hold_their_promises(L):
    c = lr.long_bin_cases(L)
    rb, rd, rf, st, ln = lr.prepare_ref(c['coor'], *c['grid'])
    assert ln.max() == L and ln.size == 302
    seg = rd[st[1]:st[1] + L]
    assert (np.diff(seg) > 0).all()                       # ascending point index
    assert c['coor'].shape[1] * c['coor'].shape[4] <= 4500
