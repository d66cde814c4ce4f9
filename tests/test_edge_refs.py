"""Pins the fp64 references of tests/edge_refs.py on the CPU, before the GPU edge
tests rely on them, and proves every cap those tests state (undecided shares, tie
shares, the value bound) on the exact inputs they use -- with ATen's fp32 op sequence on
the CPU standing in for the kernel, so that the reference alone is known to stay inside
each cap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import edge_refs as er
from tests.conftest import load_golden
from veon_amd import half
from veon_amd.models.semantic_net import temporal_fusion as tfm


# ------------------------------------------------------------------------ occ_tail_ref
@pytest.mark.parametrize('name', ['small', 'ragged', 'down', 'equal', 'z1', 'y1', 'x1', 'q40'])
def test_occ_tail_ref_matches_aten_float64(name):
    """F.interpolate on float64 input forms scale and source index in float64, the
    reference in float32 as the fp32 op does: the lambdas differ by a few float32 ulps
    of the source index (exactly zero for ratios that are powers of two)."""
    sem_low, bin_low, size = er.occ_inputs(name)
    r = er.occ_tail_ref(sem_low, bin_low, size)
    for got, low in ((r.sem, sem_low), (r.bin, bin_low)):
        want = F.interpolate(low.double(), size=size, mode='trilinear', align_corners=False)
        exact = all(m % n == 0 and (m // n) & (m // n - 1) == 0
                    for n, m in zip(low.shape[2:], size))
        # per axis |d lambda| <= 4 ulp32(src), |p1 - p0| <= 2 max|x|
        tol = 0.0 if exact else 3 * 4 * 2.0 ** -23 * max(low.shape[2:]) * 2 * low.abs().max().item()
        assert (got - want).abs().max().item() <= tol, (name, tol)


def test_occ_tail_ref_labels_follow_the_stated_rule():
    sem_low, bin_low, size = er.occ_inputs('small')
    r = er.occ_tail_ref(sem_low, bin_low, size)
    cls = r.sem.argmax(dim=1)
    want = torch.where(r.bin[:, 0] > r.bin[:, 1], cls, torch.full_like(cls, sem_low.shape[1]))
    assert torch.equal(r.labels, want.permute(0, 3, 2, 1))
    top = r.sem.sort(dim=1, descending=True).values
    assert torch.equal(r.sem_margin, top[:, 0] - top[:, 1])
    assert torch.equal(r.bin_margin, (r.bin[:, 0] - r.bin[:, 1]).abs())


def _cap_failures(name, fused, tail=None):
    sem_low, bin_low, size = er.occ_inputs(name)
    r = er.occ_tail_ref(sem_low, bin_low, size, fused_index=fused)
    sem, binv, occ = (tail or er.aten_tail)(sem_low, bin_low, size)
    out = []
    for key, got, ref, mag in (('sem', sem, r.sem, r.sem_abs), ('bin', binv, r.bin, r.bin_abs)):
        ratio = ((got.double() - ref).abs() / (er.VALUE_BOUND * mag)).max().item()
        if not ratio <= 1.0:
            out.append((key, 'err/bound', ratio))
    und = r.undecided()
    share = und.double().mean().item()
    if not share < er.UNDECIDED_CAP:
        out.append(('undecided share', share))
    differ = (occ != r.labels).permute(0, 3, 2, 1)
    if bool((differ & ~und).any()):
        out.append(('labels differ outside the undecided set', int((differ & ~und).sum())))
    # far below the cap: even at an absolute margin of 2e-5
    wide = ((r.sem_margin <= 2e-5) | (r.bin_margin <= 2e-5)).double().mean().item()
    if not (wide < 5e-5 or und.numel() < 2e4):
        out.append(('share at margin 2e-5', wide))
    return out, share


@pytest.mark.parametrize('name', sorted(er.OCC_CASES))
def test_aten_fp32_stays_inside_every_cap(name):
    """The value bound, the label rule outside the undecided set and the cap on that
    set's share, with ATen fp32 on the CPU in the kernel's place.  ATen must stay
    inside every cap against the reference that shares its source-index rounding: the
    contracted one where its build fuses scale*(dst+0.5)-0.5, else the plain one (which
    the library, built with contraction off, shares).  The share of undecided voxels is
    held under the cap for BOTH roundings, the plain one being what the GPU test uses.

    What pins what: the source-index FORMULA (``_axis``) is pinned by the comparison with
    ATen -- here in fp32 and in test_occ_tail_ref_matches_aten_float64.  The plain-fp32
    stand-in of the next test shares ``_axis`` with the reference, so it pins the
    ROUNDING of the blend only, not the formula."""
    plain, share_p = _cap_failures(name, False)
    fused, share_f = _cap_failures(name, True)
    assert not plain or not fused, (name, plain, fused)
    assert share_p < er.UNDECIDED_CAP and share_f < er.UNDECIDED_CAP


@pytest.mark.parametrize('name', sorted(er.OCC_CASES))
def test_plain_fp32_arithmetic_stays_inside_every_cap(name):
    """Where ATen's build fuses the source index ('down', 'ragged', 'q40' here: ratios
    that are not binary fractions) the test above pins only the fused variant of the
    reference.  This one pins the PLAIN variant -- the one the GPU tests use -- on every
    case, with the kernel's arithmetic in numpy float32 (no contraction) in its place."""
    failures, share = _cap_failures(name, False, er.plain_fp32_tail)
    assert not failures, (name, failures)
    assert share < er.UNDECIDED_CAP / 2, (name, share)     # not one voxel from the cap


def test_plain_fp32_stand_in_equals_aten_where_the_index_is_exact():
    for name in ('veon', 'small', 'q17'):                  # 2x ratios
        sem_low, bin_low, size = er.occ_inputs(name)
        a, b = er.plain_fp32_tail(sem_low, bin_low, size), er.aten_tail(sem_low, bin_low, size)
        r = er.occ_tail_ref(sem_low, bin_low, size)
        for u, v, mag in zip(a[:2], b[:2], (r.sem_abs, r.bin_abs)):
            assert bool(((u.double() - v.double()).abs() <= 2 * er.VALUE_BOUND * mag).all())
        differ = (a[2] != b[2]).permute(0, 3, 2, 1)
        assert not bool((differ & ~r.undecided()).any())


def test_the_two_source_index_roundings_differ_by_an_ulp_at_most():
    for n_in, n_out in ((9, 5), (10, 7), (6, 3), (5, 11), (9, 20), (2, 5), (100, 200), (4, 9)):
        a, b = er._axis(n_in, n_out), er._axis(n_in, n_out, fused=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert (a[3] - b[3]).abs().max().item() <= 2.0 ** -23 * n_in
        if n_out == 2 * n_in:
            assert torch.equal(a[3], b[3])


def test_equal_sizes_are_the_identity():
    sem_low, bin_low, size = er.occ_inputs('equal')
    r = er.occ_tail_ref(sem_low, bin_low, size)
    assert torch.equal(r.sem, sem_low.double()) and torch.equal(r.bin, bin_low.double())
    sem, binv, _ = er.aten_tail(sem_low, bin_low, size)
    assert torch.equal(sem, sem_low) and torch.equal(binv, bin_low)


def test_integer_logits_interpolate_exactly():
    """ATen fp32 == ATen fp64 == the reference on integer logits at a 2x ratio; about
    3 % of the voxels tie at the top and the first maximum wins; o0 == o1 is free."""
    sem_low, bin_low, size = er.occ_integer_inputs()
    Q = sem_low.shape[1]
    r = er.occ_tail_ref(sem_low, bin_low, size)
    sem, binv, occ = er.aten_tail(sem_low, bin_low, size)
    sem64 = F.interpolate(sem_low.double(), size=size, mode='trilinear', align_corners=False)
    assert torch.equal(sem.double(), sem64) and torch.equal(r.sem, sem64)
    assert torch.equal(binv.double(), r.bin)
    assert torch.equal(occ, r.labels)
    tied = (r.sem_margin == 0).double().mean().item()
    free = (r.bin_margin == 0)
    assert 0.01 < tied < 0.06, tied
    assert free.any() and bool((r.labels.permute(0, 3, 2, 1)[free] == Q).all())
    # nothing else is near a decision: the smallest non-zero margin is 1/64
    for m in (r.sem_margin, r.bin_margin):
        assert m[m > 0].min().item() >= 1.0 / 64


def test_special_values_keep_labels_in_range_and_touch_something():
    sem_low, bin_low, size, mask = er.occ_special_inputs()
    Q = sem_low.shape[1]
    touch = er.corner_touch(mask, size)
    assert 0.02 < touch.double().mean().item() < 0.5
    sem, binv, occ = er.aten_tail(sem_low, bin_low, size)
    assert int(occ.min()) >= 0 and int(occ.max()) <= Q
    # every non-finite output lies in the touched set, and the rule of the reference
    # agrees with ATen wherever the interpolated logits are finite
    bad = ~torch.isfinite(sem).all(dim=1) | ~torch.isfinite(binv).all(dim=1)
    assert bool(bad.any()) and not bool((bad & ~touch).any())
    r = er.occ_tail_ref(sem_low, bin_low, size)
    same = (occ == r.labels).permute(0, 3, 2, 1)
    assert bool(same[~bad & ~r.undecided()].all())
    # a NaN class logit, a +inf maximum and an all -inf voxel are all unscored -> free
    nan_cls = torch.isnan(sem).any(dim=1)
    pinf = (sem == float('inf')).any(dim=1)
    ninf_all = (sem == float('-inf')).all(dim=1)
    assert nan_cls.any() and pinf.any() and ninf_all.any()
    for m in (nan_cls, pinf, ninf_all):
        assert bool((occ.permute(0, 3, 2, 1)[m] == Q).all())
    # -inf in a non-maximal class alone does not unscore a voxel
    ninf_some = (sem == float('-inf')).any(dim=1) & ~ninf_all & ~nan_cls & ~pinf
    assert bool((occ.permute(0, 3, 2, 1)[ninf_some] < Q).any())


# ---------------------------------------------------------------------------- warp_ref
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_warp_ref_matches_the_stored_vectors(dt):
    """The vectors tests/test_temporal.py pins the mirror to; the volume is rounded to
    half first, so the tolerance is that rounding (unit roundoff times the largest
    entry) on top of the 1e-4 of the fp32 vectors."""
    g = load_golden('temporal_tiny')
    grid = {k: [float(v) for v in g['align_grid'][i]] for i, k in enumerate('xyz')}
    ds = tuple(int(v) for v in g['align_ds'])
    occ = torch.from_numpy(g['align_in'])
    want = torch.from_numpy(g['align_out']).double()
    with half.use(dt):
        out = er.warp_ref(occ, torch.from_numpy(g['align_cur2glob']),
                          torch.from_numpy(g['align_prev2glob']), grid, ds)
        rounded = er.half_round(occ)
    assert out.dtype == torch.float64
    u = 2.0 ** -9 if dt == torch.bfloat16 else 2.0 ** -12
    assert (out - want).abs().max().item() <= 1e-4 + 1e-4 * want.abs().max().item() \
        + u * occ.abs().max().item()
    # and on a volume that half holds exactly: the fp32 vectors' own tolerance
    with half.use(dt):
        exact = er.warp_ref(rounded.float(), torch.from_numpy(g['align_cur2glob']),
                            torch.from_numpy(g['align_prev2glob']), grid, ds)
    mirror = tfm.align_after_lss(rounded.float(), [torch.from_numpy(g['align_cur2glob']),
                                                   torch.from_numpy(g['align_prev2glob'])],
                                 grid, ds)
    assert torch.allclose(exact, mirror.double(), atol=1e-4, rtol=1e-4)


def test_warp_ref_identity_and_same_pose_return_the_input():
    grid = {'x': [-40.0, 40.0, 0.4], 'y': [-40.0, 40.0, 0.25], 'z': [-1.0, 5.4, 0.8]}
    ds = (1, 2, 2)
    occ = torch.randn(2, 3, 4, 6, 8)
    eye = torch.eye(4)[None].repeat(2, 1, 1)
    out = er.warp_ref(occ, eye, eye, grid, ds)
    assert (out - er.half_round(occ)).abs().max().item() <= 1e-12
    far = torch.from_numpy(np.stack([er.pose(er.rot_xyz(0.3, -0.2, 1.1), [1500.0, -900.0, 30.0]),
                                     er.pose(er.rot_xyz(0.0, 0.0, np.pi / 2), [3.0, 2.0, 1.0])]))
    out = er.warp_ref(occ, far, far, grid, ds)
    # inv(prev) cur = 1 to float64 rounding at a 1500 m translation
    assert (out - er.half_round(occ)).abs().max().item() <= 1e-8


def test_warp_ref_whole_voxel_shift():
    grid = {'x': [-4.0, 4.0, 0.4], 'y': [-3.0, 3.0, 0.5], 'z': [-1.0, 3.0, 0.8]}
    occ = torch.randn(1, 2, 5, 12, 20)
    cur = torch.eye(4)[None].clone()
    cur[0, 0, 3] = 2 * 0.4                  # current frame is 2 voxels ahead along x
    out = er.warp_ref(occ, cur, torch.eye(4)[None], grid, (1, 1, 1))
    want = torch.zeros_like(out)
    want[..., :-2] = er.half_round(occ)[..., 2:]
    assert (out - want).abs().max().item() <= 1e-5     # 0.8 is not a binary fraction


def test_affine_ref_is_the_mirrors_coordinate_chain():
    """affine_ref maps voxel indices the way align_after_lss moves voxel centres."""
    first, step = [-39.8, -39.75, -0.6], [0.4, 0.5, 0.8]
    cur = er.pose(er.rot_xyz(0.3, -0.3, 0.7), [1500.0, -900.0, 30.0])
    prev = er.pose(er.rot_xyz(0.28, -0.31, 0.75), [1500.6, -899.7, 30.1])
    A = er.affine_ref(cur[None], prev[None], first, step)[0]
    c32, p32 = (m.astype(np.float32).astype(np.float64) for m in (cur, prev))
    T = np.linalg.inv(p32) @ c32
    for idx in ([0, 0, 0], [3, 7, 2], [199, 0, 15]):
        p = np.array(step) * idx + first
        moved = T[:3, :3] @ p + T[:3, 3]
        want = (moved - first) / step
        assert np.abs(A @ np.append(idx, 1.0) - want).max() <= 1e-9


# -------------------------------------------------------------------------- attend_ref
def test_attend_ref_is_attend_in_float64():
    torch.manual_seed(0)
    mod = tfm.TemporalDeformable(64, num_heads=2)
    kv, q = torch.randn(2, 128, 3, 4, 5), torch.randn(2, 64, 3, 4, 5)
    off = torch.randn(2, 56, 3, 4, 5) * 1.5               # 48 used + 8 surplus
    off[:, 48:] = float('nan')
    got = er.attend_ref(mod, kv, q, off)
    want = mod.attend(er.half_round(kv), er.half_round(q),
                      torch.tanh(er.half_round(off[:, :48])))
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= 1e-12
    # and close to the fp32 mirror on the same operands
    want32 = mod.attend(er.half_round(kv).float(), er.half_round(q).float(),
                        torch.tanh(er.half_round(off[:, :48]).float()))
    assert (got - want32.double()).abs().max().item() <= 1e-4


# -------------------------------------------------------------------- depth inputs
def test_every_special_depth_is_hit():
    """The construction reaches what it claims: on a map large enough to hold each
    target once, every centre, every midpoint, both clamp edges and their neighbours
    appear as block minima; K = D + 1 for the wide-window parameters."""
    for params in er.DEPTH_PARAMS:
        D, lo, step, gamma = params
        vals, kinds = er.depth_targets(*params)
        h, w = 16, 44
        assert er.DEPTH_BN * h * w >= len(vals)
        _, want_min, kind = er.depth_map(h, w, 2, params)
        c = er.depth_centres(D, lo, step)
        reach = np.float32(16.0) / np.float32(gamma)
        seen = set(want_min.ravel().tolist())
        for v in list(c) + list((c[:-1] + c[1:]) / np.float32(2)):
            assert float(v) in seen or v == 0
        for edge in (c[0] - reach, c[-1] + reach):
            for v in (np.nextafter(edge, np.float32(-1e9)), edge, np.nextafter(edge, np.float32(1e9))):
                assert float(v) in seen or v == 0
        assert (kind == 0).any() and (kind == 1).any()
    from veon_amd import depth_ops
    assert depth_ops.two_hot_window_slots(8, 1.0, 0.5) == 9
    assert depth_ops.two_hot_window_slots(59, 1.0, 64.0) == 3
    assert depth_ops.two_hot_window_slots(59, 1.0, 4.0) == 11
