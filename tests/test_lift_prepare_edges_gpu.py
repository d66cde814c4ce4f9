"""The index arrays of the lift (csrc/lss_prepare.hip) at the sort's seams, EXACTLY.

Every comparison is ``np.array_equal`` against tests/lift_refs.py (pinned on the CPU by
tests/test_lift_refs.py); only the first counts[0] / counts[1] entries of the capacity-
sized buffers are compared.  Covered: the coordinate entry on hand-made coordinates
(voxel faces, NaN / inf / huge values, wave-aggregated runs, voxels longer than the
rank pass's staged span), the camera entry the product runs (``prepare_cameras``: the
five arrays, ``counts``, the ``vstart`` table of the row pool kernels and the tile plan)
at the 1024-bin seams of the scan and on realistic rigs, the steady-state contract
(every call leaves the histogram zeroed) across CHANGING geometry, and the sparse and
two-hot entries against the same reference with an explicit keep mask.

NaN and inf are data here; no case passes a size, pointer or workspace outside an entry
point's documented contract."""
import functools

import numpy as np
import pytest
import torch

from oracle import lss_torch
from tests import lift_refs as lr
from tests.conftest import load_golden
from veon_amd import _lib, depth_ops, lss_prepare, lss_prepare_hip, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('ranks_bev', 'ranks_depth', 'ranks_feat', 'interval_starts', 'interval_lengths')


class _Owner:
    """Holds the lift workspaces of one test (lss_prepare_hip.lift_workspace)."""


def _np(t):
    return t.detach().cpu().numpy()


def _assert_arrays(got, ref, what):
    for g, r, name in zip(got, ref, NAMES):
        assert g.dtype == np.int32, (what, name)
        if not np.array_equal(g, r):
            n = min(g.size, r.size)
            bad = np.flatnonzero(g[:n] != r[:n])
            raise AssertionError(
                '%s: %s differs (%d vs %d entries, first mismatch at %s: got %s, want %s)'
                % (what, name, g.size, r.size, bad[:1], g[bad[:1]], r[bad[:1]]))


# ------------------------------------------------------------- (a) coordinate entry
def _coor_entry(coor, grid, B, vpb):
    """``lss_prepare.voxel_pooling_prepare_v2`` on a device ``coor`` -> (five numpy
    arrays, plan (tiles, 4) or None)."""
    out = lss_prepare.voxel_pooling_prepare_v2(coor.to(DEV), *grid)
    if out[0] is None:
        return lr._EMPTY, None
    plan = None
    if vpb % 64 == 0:
        p, key, _ = out[3]._veon_plan
        assert key == (B, vpb)
        plan = _np(p)[:4 * B * (vpb // 64)].reshape(-1, 4)
    return tuple(_np(t) for t in out), plan


def _check_coor_entry(coor, grid, B, vpb, what):
    ref = lr.prepare_ref(coor, *grid)
    got, plan = _coor_entry(coor, grid, B, vpb)
    assert got[0].size == ref[0].size, \
        '%s: %d points kept, the reference keeps %d' % (what, got[0].size, ref[0].size)
    _assert_arrays(got, ref, what)
    if vpb % 64 == 0 and ref[0].size:
        assert np.array_equal(plan, lr.plan_ref(ref[0], ref[3], B, vpb)), what + ': plan'
    print('%s: %d of %d points in %d intervals, longest %d: exact'
          % (what, ref[0].size, coor[..., 0].numel(), ref[3].size,
             ref[4].max() if ref[4].size else 0))
    return got, ref


def test_coordinate_entry_on_the_voxel_faces_and_non_finite_values():
    """Points on and one ulp beside every face, +-0, NaN, +-inf, +-1e30, +-3e9 steps: the
    device keeps exactly the points the reference keeps.  A NaN coordinate drops the
    point (it must not land in voxel 0 of its axis)."""
    ft = lr.face_table()
    got, ref = _check_coor_entry(ft['coor'], ft['grid'], ft['B'], ft['vpb'], 'face table')
    P = ft['coor'].shape[4]
    kept = np.zeros(2 * P, bool)
    kept[got[1]] = True
    for i, e in enumerate(ft['expect']):
        assert e is None or kept[i] == e, ft['labels'][i]


def test_coordinate_entry_drops_a_whole_nan_camera():
    """What a singular intrinsic matrix produces: every coordinate of one camera NaN.
    None of its points may be kept."""
    c = lr.run_cases()
    coor = c['coor'].clone()
    coor[1, 0] = float('nan')
    _check_coor_entry(coor, c['grid'], c['B'], c['vpb'], 'NaN camera')


@pytest.mark.parametrize('variant', ['coor', 'coor_nan'])
def test_coordinate_entry_on_wave_aggregated_runs(variant):
    c = lr.run_cases()
    _check_coor_entry(c[variant], c['grid'], c['B'], c['vpb'], 'runs/' + variant)


@pytest.mark.parametrize('L', lr.LONG_BINS)
def test_coordinate_entry_on_a_long_voxel(L):
    """One voxel of L points around the rank pass's block size (256) and staged span
    (3072), arrival order scrambled: ascending point index inside every interval."""
    c = lr.long_bin_cases(L)
    got, _ = _check_coor_entry(c['coor'], c['grid'], c['B'], c['vpb'], c['name'])
    assert got[4].max() == L


# ----------------------------------------------------------------- (b) camera entry
def _camera_entry(rig, grid, owner, n_bins, **kw):
    """``lss_prepare_hip.prepare_cameras`` -> dict(arrays, counts, vstart, plan) on the
    host; ``rig['frustum']`` stays on the CPU (its axes are copied by the wrapper)."""
    d = {k: v.to(DEV) for k, v in rig.items() if k != 'frustum'}
    before = dict(_lib.CALLS)
    ws = lss_prepare_hip.prepare_cameras(
        rig['frustum'], d['sensor2ego'], d['cam2imgs'], d['post_rots'], d['post_trans'],
        d['bda'], *grid, owner=owner, **kw)
    torch.cuda.synchronize()
    ran = [k for k in _lib.CALLS if k.startswith('veon_lss_prepare_cameras')
           and _lib.CALLS[k] != before.get(k, 0)]
    assert len(ran) == 1, ran
    assert ws.dirty is False
    kept, n_int = (int(v) for v in ws.counts.tolist())
    arrays = tuple(_np(t)[:n].copy() for t, n in (
        (ws.ranks_bev, kept), (ws.ranks_depth, kept), (ws.ranks_feat, kept),
        (ws.interval_starts, n_int), (ws.interval_lengths, n_int)))
    plan = None
    if ws.plan is not None:
        plan = _np(ws.plan)[:4 * (n_bins // 64)].reshape(-1, 4).copy()
    return dict(arrays=arrays, counts=(kept, n_int), vstart=_np(ws.vstart)[:n_bins + 1].copy(),
                plan=plan, entry=ran[0])


def _assert_camera_entry(got, ref, B, vpb, what):
    assert got['counts'] == (ref[0].size, ref[3].size), (what, got['counts'])
    _assert_arrays(got['arrays'], ref, what)
    n_bins = B * vpb
    vs = lr.vstart_ref(ref[0], n_bins)
    if not np.array_equal(got['vstart'], vs):
        bad = np.flatnonzero(got['vstart'] != vs)
        raise AssertionError('%s: vstart differs at %s of %d: got %s, want %s'
                             % (what, bad[:4], n_bins + 1, got['vstart'][bad[:4]], vs[bad[:4]]))
    if vpb % 64 == 0:
        assert got['plan'] is not None
        assert np.array_equal(got['plan'], lr.plan_ref(ref[0], ref[3], B, vpb)), what + ': plan'
    else:
        assert got['plan'] is None
    print('%s: %d points in %d intervals over %d bins (%s): arrays, vstart%s exact'
          % (what, ref[0].size, ref[3].size, n_bins, got['entry'][5:],
             ', plan' if vpb % 64 == 0 else ''))


@pytest.mark.parametrize('B,X', lr.SCAN_GRIDS)
def test_camera_entry_at_the_scan_seams(B, X):
    """Occupancy patterns around the 1024-bin blocks of the two-kernel scan, the last
    bin, a batch boundary inside a scan block, and grids without a plan: arrays, counts,
    the vstart table (all zero when nothing is kept) and the plan."""
    for c in lr.scan_cases(B, X):
        ref = lr.prepare_ref(lr.rig_coor(c['rig']), *c['grid'])
        got = _camera_entry(c['rig'], c['grid'], _Owner(), c['n_bins'])
        assert got['entry'] == 'veon_lss_prepare_cameras'
        _assert_camera_entry(got, ref, B, X, c['name'])
        if c['name'].endswith('none'):
            assert got['counts'] == (0, 0) and not got['vstart'].any()


def test_camera_entry_on_wave_aggregated_runs():
    c = lr.run_cases()
    ref = lr.prepare_ref(c['coor'], *c['grid'])
    got = _camera_entry(c['rig'], c['grid'], _Owner(), c['n_bins'])
    _assert_camera_entry(got, ref, c['B'], c['vpb'], 'runs')


def test_camera_entry_drops_a_camera_with_singular_intrinsics():
    """An all-zero intrinsic matrix (a padded, absent camera): det = 0 in the adjugate
    inverse, so every entry of that camera's matrices and every coordinate of its points
    is NaN.  None of them may be kept; the other cameras are untouched."""
    c = lr.run_cases()
    rig = {k: v.clone() for k, v in c['rig'].items()}
    rig['cam2imgs'][1, 0] = 0.0
    _, comb, _ = lss_prepare_hip.camera_matrices(
        rig['sensor2ego'].to(DEV), rig['cam2imgs'].to(DEV), rig['post_rots'].to(DEV))
    assert bool(torch.isnan(comb[1, 0]).all()) and bool(torch.isfinite(comb[1, 1]).all())
    coor = c['coor'].clone()
    coor[1, 0] = float('nan')
    ref = lr.prepare_ref(coor, *c['grid'])
    # the camera's 668 in-grid points (700 less the 32 dropped ones) are gone
    assert ref[0].size == lr.prepare_ref(c['coor'], *c['grid'])[0].size - 668
    got = _camera_entry(rig, c['grid'], _Owner(), c['n_bins'])
    _assert_camera_entry(got, ref, c['B'], c['vpb'], 'singular intrinsics')


# ---------------------------------------------------------------- (c) realistic rigs
GRID_C = {'x': [-40, 40, 2.5], 'y': [-40, 40, 2.5], 'z': [-1, 5.4, 0.8],
          'depth': [1.0, 45.0, 1.0]}
RIGS = ('synthetic', 'lss_small_b2')


@functools.lru_cache(maxsize=None)
def _rig_c(name):
    """A realistic rig, its grid, and the reference arrays: camera matrices by the
    device kernel whose arithmetic the camera entry repeats in LDS
    (``lss_prepare_hip.camera_matrices``), copied to the host; from there the CPU path
    (``lidar_coor_from_matrices_torch``, then ``prepare_ref``).  Computed once and
    shared; treat as read-only."""
    if name == 'synthetic':
        r = synthetic.make_rig(2, 3, (64, 176))
        rig = dict(frustum=lss_torch.make_frustum(GRID_C['depth'], (64, 176), 16),
                   sensor2ego=r['sensor2ego'], cam2imgs=r['intrins'],
                   post_rots=r['post_rots'], post_trans=r['post_trans'], bda=r['bda'])
        grid = lss_torch.grid_infos(GRID_C)
    else:
        g = load_golden(name)
        rig = {k: torch.from_numpy(g[s]) for k, s in (
            ('frustum', 'frustum'), ('sensor2ego', 'sensor2ego'), ('cam2imgs', 'intrins'),
            ('post_rots', 'post_rots'), ('post_trans', 'post_trans'), ('bda', 'bda'))}
        grid = tuple(torch.from_numpy(g[k]) for k in ('grid_lower_bound', 'grid_interval',
                                                      'grid_size'))
    B, N = rig['sensor2ego'].shape[:2]
    D, H, W, _ = rig['frustum'].shape
    vpb = int(grid[2][0]) * int(grid[2][1]) * int(grid[2][2])
    assert vpb % 64 == 0 and B == 2
    mats = lss_prepare_hip.camera_matrices(rig['sensor2ego'].to(DEV), rig['cam2imgs'].to(DEV),
                                           rig['post_rots'].to(DEV))
    pri, comb, trans = (m.cpu() for m in mats)
    coor = lss_prepare.lidar_coor_from_matrices_torch(rig['frustum'], pri, rig['post_trans'],
                                                      comb, trans, rig['bda'])
    ref = lr.prepare_ref(coor, *grid)
    assert ref[0].size > 1000 and ref[0][-1] >= vpb          # both batch elements occupied
    return dict(rig=rig, grid=grid, dims=(B, N, D, H, W), B=B, vpb=vpb, n_bins=B * vpb,
                mats=(pri, comb, trans), coor=coor, ref=ref)


@pytest.mark.parametrize('name', RIGS)
def test_camera_entry_on_realistic_rigs(name):
    c = _rig_c(name)
    got = _camera_entry(c['rig'], c['grid'], _Owner(), c['n_bins'])
    _assert_camera_entry(got, c['ref'], c['B'], c['vpb'], name)
    # the same matrices through the matrix entry (geometry fused, FROM = 0)
    pri, comb, trans = (m.to(DEV) for m in c['mats'])
    out = lss_prepare_hip.prepare_from_matrices(
        c['rig']['frustum'], pri, c['rig']['post_trans'].to(DEV), comb, trans,
        c['rig']['bda'].to(DEV), *c['grid'])
    _assert_arrays(tuple(_np(t) for t in out), c['ref'], name + ' from matrices')


# ------------------------------------------------------------------ (d) steady state
def _steady_geometries():
    """Same dims (2,2,1,1,1088) and vpb = 1088, changing geometry: dense, nothing kept,
    everything in one voxel, dense again."""
    X = 1088
    xs = np.random.RandomState(7).permutation(X) + 0.5
    dense = lr._axis_case('dense', xs, 2, [[0.0, 2.0], [64.0, -1.0]], 2, X)
    none = lr._axis_case('none', xs, 2, -5000.0, 2, X)
    one = lr._axis_case('one-voxel', np.full(X, 500.5), 2, 0.0, 2, X)
    again = lr._axis_case('dense-again', xs[::-1].copy(), 2, [[1.0, 0.0], [0.0, 3.0]], 2, X)
    assert (none['bins'] < 0).all() and set(one['bins']) == {500, X + 500}
    assert (dense['bins'] >= 0).sum() > 4000 and (again['bins'] >= 0).sum() > 4000
    assert len({c['dims'] for c in (dense, none, one, again)}) == 1
    return [dense, none, one, again]


@pytest.mark.parametrize('dirty_before', [(), (1, 3)])
def test_steady_state_across_changing_geometry(dirty_before):
    """One owner, one workspace: every call leaves the histogram zeroed for the next
    one (no memset node), whatever the geometry was.  Every call must equal the same
    call on a fresh owner and the reference; ``ws.dirty = True`` before a call takes
    the memset path instead."""
    owner = _Owner()
    seq = _steady_geometries()
    for i, c in enumerate(seq):
        if i in dirty_before:
            ws = lss_prepare_hip.lift_workspace(c['dims'], c['vpb'], torch.device(DEV), owner)
            ws.dirty = True
        got = _camera_entry(c['rig'], c['grid'], owner, 2 * c['vpb'])
        fresh = _camera_entry(c['rig'], c['grid'], _Owner(), 2 * c['vpb'])
        ref = lr.prepare_ref(lr.rig_coor(c['rig']), *c['grid'])
        _assert_camera_entry(fresh, ref, 2, c['vpb'], c['name'] + ' (fresh owner)')
        _assert_camera_entry(got, ref, 2, c['vpb'], c['name'] + ' (call %d of one owner)' % i)
    assert len(owner.__dict__['_veon_lift_workspaces']) == 1


# ------------------------------------------------------------------- (e) sparse entry
def test_sparse_entry_keeps_exactly_the_weights_at_or_above_eps():
    c = _rig_c('synthetic')
    eps = 1e-3
    e32 = np.float32(eps)
    rs = np.random.RandomState(3)
    w = (rs.rand(*c['dims']) * 2e-3).astype(np.float32)
    flat = w.reshape(-1)
    in_grid = c['ref'][1]                       # points the dense prepare keeps
    flat[in_grid[0::7]] = e32                   # exactly eps: kept
    flat[in_grid[3::7]] = np.nextafter(e32, np.float32(0))   # one ulp below: dropped
    keep = w >= e32
    assert keep.reshape(-1)[in_grid[0::7]].all() and not keep.reshape(-1)[in_grid[3::7]].any()
    ref = lr.prepare_ref(c['coor'], *c['grid'], keep=keep)
    assert 0 < ref[0].size < c['ref'][0].size
    got = _camera_entry(c['rig'], c['grid'], _Owner(), c['n_bins'],
                        depth_weights=torch.from_numpy(w).to(DEV), depth_eps=eps)
    assert got['entry'] == 'veon_lss_prepare_cameras_sparse'
    _assert_camera_entry(got, ref, c['B'], c['vpb'], 'sparse')


# ------------------------------------------------------------------ (f) two-hot entry
@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_twohot_entry_keeps_the_window_points_and_emits_compact_slots(eps):
    c = _rig_c('synthetic')
    B, N, D, H, W = c['dims']
    lo, _, step = GRID_C['depth']
    g = torch.Generator().manual_seed(11)
    metric = 0.5 + 50.0 * torch.rand(B, N, H, W, generator=g)     # some beyond the range
    metric[0, 0, 0, :3] = 0.0
    tw = depth_ops.two_hot_windows(metric.to(DEV), D, lo, step, 4, eps)
    assert tuple(tw.shape) == c['dims']
    keep, slot = lr.twohot_keep_and_slot(_np(tw.win), D, H, W, tw.K)
    assert keep.all() == (eps == 0.0)
    ref = lr.prepare_ref(c['coor'], *c['grid'], keep=keep)
    assert (ref[0].size == c['ref'][0].size) == (eps == 0.0) and ref[0].size > 0
    got = _camera_entry(c['rig'], c['grid'], _Owner(), c['n_bins'], twohot=tw)
    assert got['entry'] == 'veon_lss_prepare_cameras_twohot'
    want = (ref[0], slot[ref[1]], ref[2], ref[3], ref[4])
    _assert_camera_entry(got, want, c['B'], c['vpb'], 'two-hot eps %g' % eps)
