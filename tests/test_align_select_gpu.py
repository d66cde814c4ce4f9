"""GPU checks of the native entry selection of the feature-alignment loss
(csrc/occ_align_select.hip via veon_amd.align_select.select_entries and the ``hip_select``
switch of ``Proj2Dto3DLoss`` / ``OccLossFB``).

The oracle is always the mirror's ``select`` in fp64 on the CPU (``selection`` of
tests/test_align_loss.py), never the code under test.  The selection is discrete: on data
whose every decision has a margin fp32 cannot cross (the fixture by construction, the
synthetic cases through ``protect`` of tests/align_select_refs.py, whose 1 % cap is
asserted on the host while the case is built) the native lists EQUAL the oracle's: voxels,
labels, n_det and the per-camera counts.  Weights: within 32 * 2^-24 relative of the
oracle's fp64 weights (a sum of at most 17 positive priorities plus about six fp32
operations on exact integer counts)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import align_select_refs as refs
from tests.conftest import load_golden
from tests.test_align_loss import CASES, build_loss, fixture_inputs, selection
from veon_amd import _lib, align_select
from veon_amd.models.semantic_net.occ_loss import OccLossFB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
W_RTOL = 32 * U


def make_loss(case, ov=8, **kw):
    loss = OccLossFB(grid_config=case['grid_config'], high_conf_thr=case['high_conf_thr'],
                     stage2_start=case['stage2_start'], priority=case['priority'],
                     ov_class_number=ov, **kw)
    loss.epoch = case['epoch']
    return loss


@functools.lru_cache(maxsize=None)
def case_of(name):
    return refs.make_case(name)


@functools.lru_cache(maxsize=None)
def oracle_of(name, ov=8):
    """The fp64 CPU mirror's entry lists of a synthetic case (computed once, shared)."""
    case = refs.to_device(case_of(name), 'cpu', torch.float64)
    return selection(make_loss(case, ov), case)


def native_selection(loss, inp):
    """``select`` with the switch on; asserts that the native entry points ran."""
    loss.hip_select = True
    n0 = dict(_lib.CALLS)
    sel = selection(loss, inp)
    B = inp['sem_seg_ds'].shape[0]
    assert _lib.CALLS.get('veon_align_select_mark', 0) == n0.get('veon_align_select_mark', 0) + B
    return sel


def assert_same(got, want, what=''):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g['n_det'] == w['n_det'], (what, b, g['n_det'], w['n_det'])
        for k in ('det', 'soft', 'ignored'):
            assert g[k].dtype == torch.int64
            assert torch.equal(g[k].cpu(), w[k]), (what, b, k, g[k].tolist(), w[k].tolist())
        for k in ('voxels', 'labels'):
            assert g[k].dtype == torch.int32 and g[k].shape == w[k].shape, (what, b, k)
            assert torch.equal(g[k].cpu(), w[k]), (what, b, k)
        assert g['weights'].dtype == torch.float32
        gw, ww = g['weights'].double().cpu(), w['weights'].double()
        assert gw.shape == ww.shape
        if ww.numel():
            rel = float(((gw - ww).abs() / ww.abs().clamp_min(1e-300)).max())
            print('%s sample %d: n %d n_det %d max rel weight error %.2e'
                  % (what, b, ww.numel(), w['n_det'], rel))
            assert bool(((gw - ww).abs() <= W_RTOL * ww.abs()).all()), (what, b, rel)


def run_synthetic(name, ov=8, labels=None):
    case = case_of(name)
    if labels is not None:
        case = dict(case, voxel_semantics=labels)
    got = native_selection(make_loss(case, ov), refs.to_device(case, DEV))
    assert_same(got, oracle_of(name, ov), '%s ov %d' % (name, ov))
    return got


# ------------------------------------------------------------------ 1. the fixture

@pytest.mark.parametrize('case', CASES)
def test_fixture_lists_and_loss(case):
    g = load_golden('align_loss_tiny')
    inp64 = fixture_inputs(g, torch.float64)
    want = selection(build_loss(g, inp64, case), inp64)
    inp = fixture_inputs(g, torch.float32, DEV)
    loss = build_loss(g, inp, case)
    got = native_selection(loss, inp)
    assert_same(got, want, 'fixture ' + case)
    counts = torch.stack([torch.stack([s[k].cpu() for s in got]) for k in ('det', 'soft', 'ignored')])
    assert np.array_equal(counts.numpy(), g[case + '_counts'])
    # Proj2Dto3DLoss.forward on the native lists: the recorded losses and gradient, at the
    # bounds of test_mirror_matches_reference_fixture
    feat = inp['feat_low'].clone().requires_grad_(True)
    det, soft = loss.proj2dto3dloss(
        feat, inp['sem_seg_ds'], img_inputs=inp['img_inputs'],
        voxel_semantics=loss.masked_labels(inp['voxel_semantics'], inp['mask_camera']),
        class_reflection=inp['class_reflection'], ov_classifier_weight=inp['table'],
        occ_size=inp['occ_size'])
    np.testing.assert_allclose(float(det.detach()), float(g[case + '_loss_det']), atol=1e-5)
    np.testing.assert_allclose(float(soft.detach()), float(g[case + '_loss_soft']), atol=1e-5)
    grad, = torch.autograd.grad(det + soft, feat)
    ref = g[case + '_grad'].astype(np.float64)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(grad.double().cpu().numpy() / scale, ref / scale, atol=1e-5)


# ------------------------------------------------------------------ 2. the seams

def test_seam_partial_last_workgroup():
    """(a) 4 * 10*38*46 = 69 920 pairs = 273 * 256 + 32"""
    got = run_synthetic('seam_partial')
    assert got[0]['n_det'] > 1 and int(got[0]['soft'].sum()) > 0


def test_seam_scan_takes_two_passes():
    """(b) 2 * 16*100*100 = 320 000 pairs = 1 250 workgroup totals > the 1 024 one pass of
    the scan workgroup takes"""
    spec = refs.SPECS['seam_scan']
    assert spec['n_cam'] * int(np.prod(spec['occ'])) // 256 > 1024
    got = run_synthetic('seam_scan')
    assert got[0]['voxels'].shape[0] > 256 * 4          # and the second scan sees > 1 total


def test_camera_that_sees_nothing():
    """(c) equal bounds, zero per_cam, no division by a zero norm"""
    got = run_synthetic('blind_middle')
    assert int(got[0]['det'][1]) == 0 and int(got[0]['soft'][1]) == 0
    assert bool(torch.isfinite(got[0]['weights']).all())


def test_last_camera_empty_makes_no_forced_entry():
    """(d) no forced entry is made; the contrast is case (a), whose last camera has
    entries"""
    got = run_synthetic('blind_last')
    e = got[0]
    assert int(e['det'][3]) == 0 and int(e['soft'][3]) == 0
    want = oracle_of('blind_last')[0]
    assert want['voxels'].shape[0] == int(want['det'].sum() + want['soft'].sum())
    forced = oracle_of('seam_partial')[0]
    assert int(forced['det'][3]) > 0            # the contrast: a last camera with entries


def test_no_labelled_voxel():
    """(e) all labels free or ignored"""
    case = case_of('seam_partial')
    labels = torch.where(case['voxel_semantics'] == 255, case['voxel_semantics'],
                         torch.full_like(case['voxel_semantics'], 17))
    inp = refs.to_device(dict(case, voxel_semantics=labels), DEV)
    loss = make_loss(inp)
    e = native_selection(loss, inp)[0]
    assert e['voxels'].shape == (0, 3) and e['voxels'].dtype == torch.int32
    assert e['labels'].shape == (0,) and e['labels'].dtype == torch.int32
    assert e['weights'].shape == (0,) and e['weights'].dtype == torch.float32
    assert e['n_det'] == 0
    for k in ('det', 'soft', 'ignored'):
        assert e[k].dtype == torch.int64 and e[k].shape == (4,) and not e[k].any()
    feat = inp['feat_low'].clone().requires_grad_(True)
    det, soft = loss.proj2dto3dloss(
        feat, inp['sem_seg_ds'], img_inputs=inp['img_inputs'], voxel_semantics=inp['voxel_semantics'],
        class_reflection=inp['class_reflection'], ov_classifier_weight=inp['table'],
        occ_size=inp['occ_size'])
    assert float(det) == 0.0 and float(soft) == 0.0
    (det + soft + 0 * feat.sum()).backward()
    assert not feat.grad.any()


@pytest.mark.parametrize('ov', [17, 0])
def test_open_vocabulary_split(ov):
    """(f) ov 17: det_scale 0 and the det list is the forced entry only; ov 0: nothing is
    soft by its class alone"""
    got = run_synthetic('seam_partial', ov)
    if ov == 17:
        assert got[0]['n_det'] == 1 and float(got[0]['weights'][0]) == 0.0


def test_label_dtypes():
    """(g) int64 labels holding a negative value, int32 labels (converted by the wrapper)
    and uint8 labels give the same lists"""
    case = case_of('seam_partial')
    u8 = case['voxel_semantics'].masked_fill(case['mask_camera'] == 0, 255)
    assert u8.dtype == torch.uint8 and bool((u8 == 255).any())
    i64 = u8.long()
    i64[i64 == 255] = -3
    mask = torch.ones_like(case['mask_camera'])      # the mask is applied above already
    for labels in (i64, i64.to(torch.int32), u8):
        c = dict(case, voxel_semantics=labels, mask_camera=mask)
        inp = refs.to_device(c, DEV)
        got = native_selection(make_loss(c), inp)
        c64 = refs.to_device(c, 'cpu', torch.float64)
        assert_same(got, selection(make_loss(c64), c64), 'labels %s' % labels.dtype)


def test_batch_of_two():
    """(h) the forced entry appears only in the last sample; the weights carry 1 / B: the
    soft weights of a sample sum to 1 / B (each camera's class-balanced mean sums to its
    share of the entries)"""
    got = run_synthetic('batch2')
    want = oracle_of('batch2')
    assert len(got) == 2
    for e in got:
        assert abs(float(e['weights'][e['n_det']:].double().sum()) - 0.5) <= 1e-5
    # sample 0 lists every kept pair once; sample 1 lists its forced pair twice
    c = case_of('batch2')
    assert want[0]['voxels'].shape[0] == int(want[0]['det'].sum() + want[0]['soft'].sum())
    one = dict(c, **{k: c[k][1:] for k in ('feat_low', 'bin_low', 'sem_seg_ds', 'voxel_semantics',
                                           'mask_camera')})
    one['img_inputs'] = [t[1:] for t in c['img_inputs']]
    alone = native_selection(make_loss(one), refs.to_device(one, DEV))[0]
    assert torch.equal(alone['voxels'], got[1]['voxels']) and torch.equal(alone['labels'], got[1]['labels'])
    torch.testing.assert_close(alone['weights'] / 2, got[1]['weights'], rtol=0, atol=0)


def test_stage_two():
    """(i) dropped entries, soft entries that stay and a camera with ignored > 0"""
    got = run_synthetic('stage2')
    e = got[0]
    assert int(e['ignored'].sum()) > 0 and int(e['soft'].sum()) > 0 and int(e['ignored'].max()) > 0
    off = dict(case_of('stage2'), epoch=0)
    c64 = refs.to_device(off, 'cpu', torch.float64)
    before = selection(make_loss(c64), c64)[0]
    assert int(before['soft'].sum()) == int(e['soft'].sum() + e['ignored'].sum())


def test_map_smaller_than_the_image():
    """(j) a 7 x 11 map under a 20 x 36 image: ix = u * 11 / 35 - 0.5 is negative for
    u < 1.6 px, so zero-padded corners are sampled"""
    n = refs.padded_corner_samples(case_of('small_map'))
    print('small_map: %d kept pairs sample a zero-padded corner' % n)
    assert n > 100
    run_synthetic('small_map')


# ------------------------------------------------------------------ 3. determinism

def _flat(sel):
    return [(e['voxels'].clone(), e['labels'].clone(), e['weights'].clone(), e['n_det'],
             e['det'].clone(), e['soft'].clone(), e['ignored'].clone()) for e in sel]


def _equal(a, b):
    return all(x == y if isinstance(x, int) else torch.equal(x, y)
               for ea, eb in zip(a, b) for x, y in zip(ea, eb))


def test_bit_identical_and_workspace_independent():
    case = case_of('stage2')
    inp = refs.to_device(case, DEV)
    loss = make_loss(case)
    first = _flat(native_selection(loss, inp))
    assert _equal(first, _flat(native_selection(loss, inp)))
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            a = torch.tanh(a @ a * 1e-3)
    assert _equal(first, _flat(native_selection(loss, inp)))
    torch.cuda.synchronize()
    # every cached workspace poisoned: 0xFF bytes are -1 in the integers and NaN in the floats
    assert align_select._WORKSPACES
    for ws in align_select._WORKSPACES.values():
        for t in ws.values():
            if isinstance(t, torch.Tensor):
                t.view(torch.uint8).fill_(255)
    assert _equal(first, _flat(native_selection(loss, inp)))


# ------------------------------------------------------------------ 4. read-backs

def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    return sum('synchroniz' in str(w.message).lower() for w in rec)


def test_at_most_two_read_backs():
    case = case_of('stage2')
    inp = refs.to_device(case, DEV)
    on, off = make_loss(case), make_loss(case)
    native_selection(on, inp)                          # workspaces and constants in place
    selection(off, inp)
    n_mirror = _sync_warnings(lambda: selection(off, inp))
    n_native = _sync_warnings(lambda: selection(on, inp))
    print('synchronisation warnings per sample: native %d, mirror %d' % (n_native, n_mirror))
    if n_mirror == 0:
        pytest.skip('torch.cuda.set_sync_debug_mode is inert on this build')
    assert n_native <= 2 < n_mirror


# ------------------------------------------------------------------ 5. in place

def test_loss_voxel_with_the_switch():
    case = case_of('in_place')
    inp = refs.to_device(case, DEV)
    labels = inp['voxel_semantics'].masked_fill(inp['mask_camera'] == 0, 255)
    meta = dict(sem_seg_ds=inp['sem_seg_ds'], img_inputs=inp['img_inputs'],
                class_reflection=inp['class_reflection'], ov_classifier_weight=inp['table'])
    out, grads, sels = [], [], []
    for on in (False, True):
        loss = make_loss(case, hip_select=on)
        feat = inp['feat_low'].clone().requires_grad_(True)
        res = dict(feat_occ=feat, bin_occ=inp['bin_low'], occ_size=inp['occ_size'])
        n0 = _lib.CALLS.get('veon_align_select_emit', 0)
        terms = loss.loss_voxel(res, labels, meta, 'c_0')
        assert (_lib.CALLS.get('veon_align_select_emit', 0) > n0) == on
        grads.append(torch.autograd.grad(sum(terms.values()), feat)[0])
        out.append(terms)
        sels.append(selection(loss, inp))
    assert set(out[0]) == set(out[1]) == {'loss_binocc_c_0', 'loss_featalign_det_c_0',
                                          'loss_featalign_soft_c_0'}
    for k in out[0]:
        a, b = float(out[0][k].detach()), float(out[1][k].detach())
        print('%s: off %.8f on %.8f' % (k, a, b))
        assert abs(a - b) <= 1e-6 * abs(a), k
    scale = float(grads[0].abs().max())
    assert scale > 0 and float((grads[0] - grads[1]).abs().max()) <= 1e-6 * scale
    for e0, e1 in zip(*sels):
        assert e0['n_det'] == e1['n_det'] > 1
        for k in ('voxels', 'labels', 'det', 'soft', 'ignored'):
            assert torch.equal(e0[k], e1[k]), k
        assert bool(((e0['weights'] - e1['weights']).abs() <= W_RTOL * e0['weights'].abs()).all())
        assert int(e0['ignored'].sum()) > 0
