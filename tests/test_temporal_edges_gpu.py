"""The gather kernels of the temporal path (csrc/temporal.hip) at their edges, against
float64 references (tests/edge_refs.py, pinned on the CPU by tests/test_edge_refs.py).

Tolerance of the two volume kernels: the one tests/test_temporal_gpu.py states for
them, now against float64 instead of device fp32 --
    |got - ref| <= half_tol(2^-7, 4e-3):  rtol |ref| + atol rms(ref)
(bf16; both terms 8x tighter in the fp16 twins).  The voxel-index affine is a float32
rounding of a double result: |A - ref| <= 2^-23 max(1, |ref|) per entry.  Every numeric
test prints its largest err/bound ratio (run with -s) and has an fp16 twin.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import edge_refs as er
from tests.helpers import flavour, fp16_twin, half_tol, to_half  # noqa: F401
from veon_amd import _lib, conv3d_ops
from veon_amd.models.semantic_net import temporal_fusion as tfm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(tag, got, want, k=4e-3):
    want = want.double().cpu()
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), tag
    rms = want.pow(2).mean().sqrt().item() + 1e-12
    tol = half_tol(2.0 ** -7, k)
    bound = want.abs() * tol['rtol'] + tol['atol'] * rms
    ratio = ((got - want).abs() / bound).max().item()
    print('%s: max err/bound %.3f (rms %.3g)' % (tag, ratio, rms))
    assert ratio <= 1.0, (tag, ratio, rms)


def _halo_is_zero(vol):
    B, C, Z, Y, X = vol.shape
    halo = vol.rows.view(B, Z + 2, Y + 2, X + 2, C).clone()
    halo[:, 1:-1, 1:-1, 1:-1] = 0
    assert float(halo.float().abs().sum()) == 0.0


# --------------------------------------------------------------------------- grids, poses
# (first centre, step) in (x, y, z), and the grid_config / ds_feat (z, y, x) that give them
GRIDS = {
    'g454': ({'x': [-40.0, 40.0, 0.4], 'y': [-40.0, 40.0, 0.5], 'z': [-1.0, 5.4, 0.8]},
             (1, 1, 1)),                     # steps (0.4, 0.5, 0.8), first x -39.8
    'g848': ({'x': [-40.2, 40.2, 0.4], 'y': [-40.0, 40.0, 0.4], 'z': [-1.0, 5.4, 0.8]},
             (2, 1, 2)),                     # steps (0.8, 0.4, 1.6), first x -39.8
}
YAW90 = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
CYCLIC = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
NEG_PERM = [[0, 1, 0], [0, 0, -1], [-1, 0, 0]]
FAR = [1500.0, -900.0, 30.0]
FAMILIES = ['yaw', 'rot3d', 'yaw90', 'cyclic', 'far']


def _first_step(gname):
    grid, ds = GRIDS[gname]
    first, step = tfm.voxel_centres(grid, ds, None)
    assert abs(first[0] + 39.8) < 1e-9
    return first, step


def _about(centre, rot, trans):
    """Rigid motion: ``rot`` about ``centre``, then ``trans``."""
    c = np.asarray(centre, np.float64)
    return er.pose(rot, c - np.asarray(rot) @ c + np.asarray(trans, np.float64))


def _poses(family, B, centre, step):
    """(cur2glob, prev2glob) (B,4,4) float64.  The relative motion inv(prev) cur is a
    small rotation about the grid's centre plus a sub-metre shift, so that the volumes
    overlap; 'yaw90' / 'cyclic' hold exact signed permutation blocks (entries literally
    0 and +-1: the pivot search must swap rows) and differ by a fractional-voxel shift;
    'far' puts both frames 1.7 km from the origin."""
    cur, prev = [], []
    for b in range(B):
        s = 1.0 + 0.37 * (b % 7) - 0.2 * (b % 3)
        frac = np.array([0.3, -0.45, 0.2]) * np.asarray(step) * s
        if family == 'yaw':
            c = er.pose(er.rot_xyz(yaw=0.2 - 0.07 * b), [3.0, -2.0, 0.1 * b])
            d = _about(centre, er.rot_xyz(yaw=0.06 * s), frac)
        elif family == 'rot3d':
            c = er.pose(er.rot_xyz(0.3, -0.3, 0.7 + 0.1 * b), [12.0, 5.0 - b, -1.0])
            d = _about(centre, er.rot_xyz(0.05 * s, -0.04 * s, 0.07 * s), frac)
        elif family == 'far':
            c = er.pose(er.rot_xyz(0.3, -0.28, 2.1 - 0.05 * b), FAR)
            d = _about(centre, er.rot_xyz(0.02 * s, 0.03, -0.05 * s), frac)
        else:
            blocks = {'yaw90': [YAW90, NEG_PERM], 'cyclic': [CYCLIC, YAW90, NEG_PERM]}[family]
            c = er.pose(blocks[b % len(blocks)], [20.0 + b, -7.5, 1.25])
            d = er.pose(np.eye(3), frac)
        cur.append(c)
        prev.append(c @ d if family not in ('yaw90', 'cyclic') else c @ np.linalg.inv(d))
    cur, prev = np.stack(cur), np.stack(prev)
    if family in ('yaw90', 'cyclic'):
        for m in (cur, prev):
            assert set(np.unique(m[:, :3, :3])) <= {-1.0, 0.0, 1.0}
            assert (m[:, 0, 0] == 0).all()                # a leading zero: row swap needed
    return cur, prev


def _t32(m):
    return torch.from_numpy(np.asarray(m, np.float32)).to(DEV)


# ------------------------------------------------------------------------- warp affine
def _check_affine(tag, A, cur, prev, first, step):
    ref = er.affine_ref(cur, prev, first, step)
    got = A.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), tag
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    ratio = (np.abs(got - ref) / bound).max()
    print('%s: max err/bound %.3f (largest |ref| %.1f)' % (tag, ratio, np.abs(ref).max()))
    assert ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize('B', [1, 3, 65])
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_warp_affine_matches_float64_algebra(gname, family, B):
    first, step = _first_step(gname)
    centre = [f + 40 * s for f, s in zip(first, step)]
    cur, prev = _poses(family, B, centre, step)
    A = conv3d_ops.warp_affine(_t32(cur), _t32(prev)[:, None], first, step)
    assert tuple(A.shape) == (B, 3, 4)
    _check_affine('%s %s B%d' % (gname, family, B), A, cur, prev, first, step)


test_warp_affine_matches_float64_algebra_fp16 = fp16_twin(test_warp_affine_matches_float64_algebra)


def test_warp_affine_far_poses_with_large_rotation_between_frames():
    """1500 m / -900 m / 30 m in both frames, under a metre apart, 90 degrees and a full
    3-D rotation between them: the offsets reach hundreds of voxels."""
    first, step = _first_step('g848')
    cur = np.stack([er.pose(er.rot_xyz(0.3, -0.3, 0.4), FAR), er.pose(YAW90, FAR)])
    prev = np.stack([er.pose(er.rot_xyz(-0.2, 0.3, 1.9), [1500.4, -899.5, 30.3]),
                     er.pose(CYCLIC, [1499.7, -900.6, 29.9])])
    A = conv3d_ops.warp_affine(_t32(cur), _t32(prev), first, step)
    _check_affine('far, rotated', A, cur, prev, first, step)


test_warp_affine_far_poses_with_large_rotation_between_frames_fp16 = fp16_twin(
    test_warp_affine_far_poses_with_large_rotation_between_frames)


def test_warp_affine_raw_abi_with_wider_rows():
    """mat_stride = 20: the matrices embedded in wider rows (the surplus is NaN) give the
    stride-16 result bit for bit."""
    first, step = _first_step('g454')
    B = 65
    cur, prev = _poses('rot3d', B, [0.0, 0.0, 0.0], step)
    want = conv3d_ops.warp_affine(_t32(cur), _t32(prev), first, step)
    wide = []
    for m in (cur, prev):
        w = torch.full((B, 20), float('nan'), device=DEV)
        w[:, :16] = _t32(m).reshape(B, 16)
        wide.append(w)
    got = torch.full((B + 1, 3, 4), -7.0, device=DEV)
    f3 = ctypes.c_double * 3
    cf, cs = f3(*first), f3(*step)
    dev = torch.device(DEV)
    st = _lib.lib().veon_warp_affine(_lib.ptr(wide[0]), _lib.ptr(wide[1]), 20,
                                     ctypes.cast(cf, ctypes.c_void_p),
                                     ctypes.cast(cs, ctypes.c_void_p), _lib.ptr(got), B,
                                     _lib.stream_ptr(dev))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(got[:B], want)
    assert bool((got[B] == -7.0).all())                  # nothing past sample B - 1


test_warp_affine_raw_abi_with_wider_rows_fp16 = fp16_twin(test_warp_affine_raw_abi_with_wider_rows)


# ------------------------------------------------------------------------- warp volume
def _volume(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return to_half(torch.randn(*shape, generator=g))


def _centre_of(shape, first, step):
    Z, Y, X = shape[2:]
    return [f + 0.5 * (n - 1) * s for f, s, n in zip(first, step, (X, Y, Z))]


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('gname', sorted(GRIDS))
@pytest.mark.parametrize('shape', [(2, 64, 4, 6, 8), (1, 8, 3, 5, 7)])
def test_warp_volume_matches_float64_mirror(shape, gname, family):
    grid, ds = GRIDS[gname]
    first, step = _first_step(gname)
    cur, prev = _poses(family, shape[0], _centre_of(shape, first, step), step)
    occ = _volume(shape, shape[1] + len(family))
    want = er.warp_ref(occ, _t32(cur), _t32(prev), grid, ds)
    assert float((want != 0).double().mean()) > 0.3       # the volumes do overlap
    got = tfm.align_after_lss(conv3d_ops.pack(occ.to(DEV)), [_t32(cur)[:, None],
                                                             _t32(prev)[:, None]], grid, ds)
    _close('warp %s %s %s' % (shape, gname, family), conv3d_ops.unpack(got), want)
    _halo_is_zero(got)


test_warp_volume_matches_float64_mirror_fp16 = fp16_twin(test_warp_volume_matches_float64_mirror)


@pytest.mark.parametrize('family', ['rot3d', 'far'])
def test_warp_volume_veon_shape(family):
    shape = (1, 256, 8, 100, 100)
    grid, ds = GRIDS['g454']
    first, step = _first_step('g454')
    cur, prev = _poses(family, 1, _centre_of(shape, first, step), step)
    occ = _volume(shape, 5)
    want = er.warp_ref(occ, _t32(cur), _t32(prev), grid, ds)
    assert float((want != 0).double().mean()) > 0.3
    got = tfm.align_after_lss(conv3d_ops.pack(occ.to(DEV)), [_t32(cur), _t32(prev)], grid, ds)
    _close('warp %s %s' % (shape, family), conv3d_ops.unpack(got), want)
    _halo_is_zero(got)


test_warp_volume_veon_shape_fp16 = fp16_twin(test_warp_volume_veon_shape)


@pytest.mark.parametrize('family', ['rot3d', 'yaw90', 'cyclic', 'far'])
@pytest.mark.parametrize('shape', [(2, 64, 4, 6, 8), (1, 8, 3, 5, 7), (1, 256, 8, 100, 100)])
def test_same_pose_in_both_frames_returns_the_input(shape, family):
    grid, ds = GRIDS['g454']
    first, step = _first_step('g454')
    cur, _ = _poses(family, shape[0], _centre_of(shape, first, step), step)
    vol = conv3d_ops.pack(_volume(shape, 11).to(DEV))
    got = tfm.align_after_lss(vol, [_t32(cur), _t32(cur)], grid, ds)
    assert torch.equal(got.rows, vol.rows)               # halo included


test_same_pose_in_both_frames_returns_the_input_fp16 = fp16_twin(
    test_same_pose_in_both_frames_returns_the_input)


@pytest.mark.parametrize('k', [1, 2, -1])
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_whole_voxel_translation_is_a_shift(gname, axis, k):
    """Identity rotation, translation k * step along one axis of an anisotropic grid:
    the input shifted by k voxels, zeros shifted in, bit for bit."""
    grid, ds = GRIDS[gname]
    first, step = _first_step(gname)
    shape = (2, 64, 4, 6, 8)
    occ = _volume(shape, 13)
    cur = np.stack([np.eye(4)] * 2)
    cur[:, axis, 3] = k * step[axis]
    got = tfm.align_after_lss(conv3d_ops.pack(occ.to(DEV)), [_t32(cur), _t32(np.stack([np.eye(4)] * 2))],
                              grid, ds)
    dim = 4 - axis                                        # x is the last tensor axis
    want = torch.zeros_like(occ)
    n = shape[dim]
    dst = [slice(None)] * 5
    src = [slice(None)] * 5
    dst[dim] = slice(max(0, -k), n - max(0, k))
    src[dim] = slice(max(0, k), n - max(0, -k))
    want[tuple(dst)] = occ[tuple(src)]
    assert torch.equal(conv3d_ops.unpack(got).cpu(), want)
    _halo_is_zero(got)


test_whole_voxel_translation_is_a_shift_fp16 = fp16_twin(test_whole_voxel_translation_is_a_shift)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_shift_past_the_grid_is_all_zero(axis):
    grid, ds = GRIDS['g454']
    first, step = _first_step('g454')
    shape = (1, 8, 3, 5, 7)
    cur = np.eye(4)[None].copy()
    cur[:, axis, 3] = (shape[4 - axis] + 1) * step[axis]
    got = tfm.align_after_lss(conv3d_ops.pack(_volume(shape, 3).to(DEV)),
                              [_t32(cur), _t32(np.eye(4)[None])], grid, ds)
    assert float(got.rows.float().abs().sum()) == 0.0


test_shift_past_the_grid_is_all_zero_fp16 = fp16_twin(test_shift_past_the_grid_is_all_zero)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_samples_on_the_cut(axis):
    """Raw affine: along one axis of length n the samples sit at exactly -1, -0.5, 0, ...
    (batch element 0) and ..., n-1, n-0.5, n (batch element 1).  By hand: weight 0 at -1
    and n, half the edge voxel at -0.5 and n-0.5, the edge voxel itself at 0 and n-1."""
    shape = (2, 64, 6, 7, 8)
    n = shape[4 - axis]
    occ = _volume(shape, 17)
    A = torch.zeros(2, 3, 4)
    for i in range(3):
        A[:, i, i] = 1.0
    A[:, axis, axis] = 0.5
    A[0, axis, 3] = -1.0                                  # 0, 1, 2 -> -1, -0.5, 0
    A[1, axis, 3] = n - 0.5 * (n - 1)                     # n-3, n-2, n-1 -> n-1, n-0.5, n
    got = conv3d_ops.unpack(conv3d_ops.warp_volume(conv3d_ops.pack(occ.to(DEV)), A.to(DEV)))
    got = got.cpu().movedim(4 - axis, -1)
    v = occ.double().movedim(4 - axis, -1)
    want = torch.zeros_like(v)
    for b in range(2):
        for i in range(n):
            pos = 0.5 * i + float(A[b, axis, 3])
            i0 = math.floor(pos)
            t = pos - i0
            for idx, w in ((i0, 1 - t), (i0 + 1, t)):
                if 0 <= idx < n and w > 0:
                    want[b, ..., i] += w * v[b, ..., idx]
    _close('cut axis %d' % axis, got, want)
    assert float(got[0, ..., 0].abs().sum()) == 0.0 and float(got[1, ..., n - 1].abs().sum()) == 0.0
    assert torch.equal(got[0, ..., 1], to_half(0.5 * occ.movedim(4 - axis, -1)[0, ..., 0]))
    assert torch.equal(got[1, ..., n - 2], to_half(0.5 * occ.movedim(4 - axis, -1)[1, ..., n - 1]))
    assert torch.equal(got[0, ..., 2], occ.movedim(4 - axis, -1)[0, ..., 0])
    assert torch.equal(got[1, ..., n - 3], occ.movedim(4 - axis, -1)[1, ..., n - 1])


test_samples_on_the_cut_fp16 = fp16_twin(test_samples_on_the_cut)


# ---------------------------------------------------------------- deformable attention
LAYOUTS = [(32, 1), (32, 2), (32, 4), (32, 8), (64, 1), (64, 2), (64, 4)]   # (head dim, heads)


def _attention_inputs(B, C, heads, zyx, seed, offsets='randn', qscale=1.0, surplus=0):
    g = torch.Generator().manual_seed(seed)
    Z, Y, X = zyx
    kv = to_half(torch.randn(B, 2 * C, Z, Y, X, generator=g))
    q = to_half(torch.randn(B, C, Z, Y, X, generator=g) * qscale)
    noff = heads * 8 * 3
    if offsets == 'zero':
        off = torch.zeros(B, noff, Z, Y, X)
    elif offsets == 'nodes3':
        # Z == X and zero offsets: zn(z) is a node of X, yn(y) of Y, xn(x) of Z -- every
        # sample sits exactly on a voxel in all three axes (weights exactly 0 and 1)
        assert Z == X
        off = torch.zeros(B, noff, Z, Y, X)
    elif offsets == 'saturated':
        off = 8.0 * (torch.randint(0, 2, (B, noff, Z, Y, X), generator=g) * 2 - 1).float()
    elif offsets == 'nodes':
        # position along X = zn + tanh(o0) / Z (the reference's axis quirk): with Z = 2
        # and X = 9, tanh(o0) = +-0.5 is a shift of exactly one voxel from the nodes 0 and
        # 8 that zn selects; atanh(0.5) is not a half value, the nearest one is used, so
        # the samples sit within a rounding of the node, on either side of it.  Only X
        # can move by whole voxels: a shift along Y is tanh(o1) (Y-1)/(2Y) < 1/2 voxel,
        # and Z on nodes needs X - 1 to divide Z - 1, X on whole voxels X - 1 >= 2Z.
        # Here Y sits on its node (o1 = 0) and Z is fractional (x / 8); 'nodes3' is the
        # case with all three axes exactly on nodes.
        assert (Z, X) == (2, 9)
        pick = torch.randint(-1, 2, (B, heads * 8, 1, Z, Y, X), generator=g).float()
        off = torch.zeros(B, heads * 8, 3, Z, Y, X)
        off[:, :, 0:1] = pick * math.atanh(0.5)
        off = off.reshape(B, noff, Z, Y, X)
    else:
        off = torch.randn(B, noff, Z, Y, X, generator=g) * 1.5
    off = to_half(off)
    if surplus:
        off = torch.cat([off, torch.full((B, surplus, Z, Y, X), float('nan'))], dim=1)
    return kv, q, off


def _run_attention(tag, kv, q, off, heads):
    C = q.shape[1]
    mod = tfm.TemporalDeformable(C, num_heads=heads)
    want = er.attend_ref(mod, kv, q, off)
    got = conv3d_ops.deform_attention(conv3d_ops.pack(kv.to(DEV)), conv3d_ops.pack(q.to(DEV)),
                                      conv3d_ops.pack(off.to(DEV)), heads)
    _close(tag, conv3d_ops.unpack(got), want)
    _halo_is_zero(got)
    return got


@pytest.mark.parametrize('B,zyx', [(1, (3, 5, 7)), (2, (2, 4, 4))])
@pytest.mark.parametrize('hd,heads', LAYOUTS)
def test_deform_attention_every_lane_layout(hd, heads, B, zyx):
    kv, q, off = _attention_inputs(B, hd * heads, heads, zyx, hd + heads)
    _run_attention('layout hd %d heads %d %s' % (hd, heads, zyx), kv, q, off, heads)


test_deform_attention_every_lane_layout_fp16 = fp16_twin(test_deform_attention_every_lane_layout)


def test_deform_attention_veon_shape():
    kv, q, off = _attention_inputs(1, 256, 4, (8, 100, 100), 1)
    _run_attention('veon shape', kv, q, off, 4)


test_deform_attention_veon_shape_fp16 = fp16_twin(test_deform_attention_veon_shape)


@pytest.mark.parametrize('hd,heads', [(32, 4), (64, 2)])
@pytest.mark.parametrize('regime', ['zero', 'saturated', 'nodes', 'nodes3', 'randn'])
def test_deform_attention_offset_regimes(regime, hd, heads):
    zyx = {'nodes': (2, 4, 9), 'nodes3': (5, 4, 5)}.get(regime, (3, 5, 7))
    kv, q, off = _attention_inputs(1, hd * heads, heads, zyx, 7 + hd, offsets=regime)
    _run_attention('offsets %s hd %d' % (regime, hd), kv, q, off, heads)


test_deform_attention_offset_regimes_fp16 = fp16_twin(test_deform_attention_offset_regimes)


@pytest.mark.parametrize('hd,heads', [(32, 4), (64, 1)])
@pytest.mark.parametrize('qscale', [1.0, 16.0, 64.0])
def test_deform_attention_logit_scales(qscale, hd, heads):
    """q scaled by 1, 16, 64: the softmax over the 8 samples goes from flat to one-hot."""
    kv, q, off = _attention_inputs(2, hd * heads, heads, (3, 5, 7), 21 + hd, qscale=qscale)
    _run_attention('q x %g hd %d' % (qscale, hd), kv, q, off, heads)


test_deform_attention_logit_scales_fp16 = fp16_twin(test_deform_attention_logit_scales)


@pytest.mark.parametrize('hd,heads', [(32, 2), (64, 2)])
@pytest.mark.parametrize('where', ['last', 'first'])
def test_deform_attention_dominant_sample(where, hd, heads):
    """One sample's logit exceeds the other seven by ~45 (64 for head dim 64), arriving
    last (the running maximum jumps at the end and everything accumulated is rescaled
    away) or first (every later term underflows).  The keys ramp along X; the dominant
    sample alone is pushed one step further along it by a saturated offset."""
    Z, Y, X = 3, 5, 7
    C = hd * heads
    g = torch.Generator().manual_seed(hd)
    ramp = 0.5 * torch.arange(X).float().view(1, 1, 1, 1, X)
    kv = torch.randn(1, 2 * C, Z, Y, X, generator=g)
    kv = kv.view(1, heads, 2, hd, Z * Y, X)
    kv[:, :, 0] = 0.1 * kv[:, :, 0] + ramp
    kv = to_half(kv.reshape(1, 2 * C, Z, Y, X))
    q = to_half(16.0 * (1 + 0.1 * torch.randn(1, C, Z, Y, X, generator=g)))
    off = torch.zeros(1, heads, 8, 3, Z, Y, X)
    off[:, :, 7 if where == 'last' else 0, 0] = 8.0
    off = to_half(off.reshape(1, heads * 24, Z, Y, X))
    got = _run_attention('dominant sample %s hd %d' % (where, hd), kv, q, off, heads)
    assert bool(torch.isfinite(got.rows.float()).all())


test_deform_attention_dominant_sample_fp16 = fp16_twin(test_deform_attention_dominant_sample)


@pytest.mark.parametrize('zyx', [(1, 5, 7), (3, 1, 7), (3, 5, 1)])
@pytest.mark.parametrize('hd,heads', [(32, 4), (64, 1)])
def test_deform_attention_axis_of_length_one(hd, heads, zyx):
    kv, q, off = _attention_inputs(2, hd * heads, heads, zyx, 31 + hd)
    _run_attention('axis of length 1 %s hd %d' % (zyx, hd), kv, q, off, heads)


test_deform_attention_axis_of_length_one_fp16 = fp16_twin(test_deform_attention_axis_of_length_one)


@pytest.mark.parametrize('hd,heads', [(32, 4), (64, 1), (32, 1)])
def test_deform_attention_ignores_surplus_offset_channels(hd, heads):
    """off_channels > heads * 24, the surplus filled with NaN: the same bits."""
    kv, q, off = _attention_inputs(2, hd * heads, heads, (3, 5, 7), 41, surplus=8)
    noff = heads * 24
    assert off.shape[1] == noff + 8 and bool(torch.isnan(off[:, noff:]).all())
    wide = _run_attention('surplus channels hd %d heads %d' % (hd, heads), kv, q, off, heads)
    tight = conv3d_ops.deform_attention(conv3d_ops.pack(kv.to(DEV)), conv3d_ops.pack(q.to(DEV)),
                                        conv3d_ops.pack(off[:, :noff].contiguous().to(DEV)), heads)
    assert torch.equal(wide.rows, tight.rows)


test_deform_attention_ignores_surplus_offset_channels_fp16 = fp16_twin(
    test_deform_attention_ignores_surplus_offset_channels)
