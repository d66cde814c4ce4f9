"""GPU checks of the training path of the fused lift + (2,2,2) max-pool
(bev_pool._LiftMaxpoolFused, LSSViewTransformerRaw.fuse_ds_grad).

Expected values never come from the code under test:
  * un-pooled sums: ``c_oracle.bev_pool_v2_fwd`` (the native forward is bit-exact
    against it, tests/test_pool_rows_gpu.py);
  * winners: CPU ``torch.max(dim=-1)`` over the '(dz dh dw)'-flattened blocks of that
    volume (first index among equal maxima, pinned in tests/test_lift_train.py), code
    255 where the winning child holds no point;
  * gradients: fp64 sums over the point lists.
Gradient tolerance: any fp32 evaluation order of a sum of n terms is within
n * 2^-24 * sum|terms| (1 + O(n 2^-24)) of the exact value; the bound used is twice
that, ``2 n 2^-24 sum|terms|``, n = C for an entry of depth_grad and the pixel's point
count for an entry of feat_grad -- hence exactly 0 where an entry has no terms.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import helpers
from tests.conftest import load_golden
from veon_amd import _lib, synthetic
from veon_amd import lss_prepare as _prep
from veon_amd.models import build_neck
from veon_amd.ops.bev_pool_v2 import bev_pool as bp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24
NEW_FWD = 'veon_bev_pool_v2_fwd_rows_maxpool_winner'
NEW_BWD = 'veon_bev_pool_v2_bwd_rows_maxpool'
NEW_TAB = 'veon_bev_pool_point_table'


def dev(a):
    return helpers.t(a, DEV)


def _calls(*names):
    return [_lib.CALLS.get(n, 0) for n in names]


# ------------------------------------------------------------------ CPU side
def _expected(depth, rows, rb, rd, rf, shape, gout, chunk=65536):
    """depth (table,), rows (R, C) fp32; rank-sorted point arrays; gout
    (B,C,Zo,Yo,Xo) fp32 -> dict(out, winner, dg, dg_bound, fg, fg_bound)."""
    B, Z, Y, X, C = shape
    Zo, Yo, Xo = Z // 2, Y // 2, X // 2
    nvox = B * Z * Y * X
    depth = np.ascontiguousarray(depth, np.float32).reshape(-1)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, C)
    st, ln = helpers.bp_intervals(rb) if len(rb) else (np.zeros(0, np.int32),) * 2
    full = c_oracle.bev_pool_v2_fwd(depth, rows, rd, rf, rb, st, ln, nvox)
    blocks = full.reshape(B, Zo, 2, Yo, 2, Xo, 2, C).transpose(0, 1, 3, 5, 7, 2, 4, 6) \
        .reshape(B, Zo, Yo, Xo, C, 8)
    vals, idx = torch.max(torch.from_numpy(np.ascontiguousarray(blocks)), dim=-1)   # CPU
    del blocks, full
    occ = np.zeros(nvox, bool)
    occ[rb] = True
    occ = occ.reshape(B, Zo, 2, Yo, 2, Xo, 2).transpose(0, 1, 3, 5, 2, 4, 6) \
        .reshape(B, Zo, Yo, Xo, 1, 8)
    idx = idx.numpy()
    won = np.take_along_axis(np.broadcast_to(occ, idx.shape + (8,)), idx[..., None], -1)[..., 0]
    winner = np.where(won, idx, 255).astype(np.uint8)
    out = vals.numpy().transpose(0, 4, 1, 2, 3)

    g_cl = np.ascontiguousarray(np.asarray(gout, np.float32).transpose(0, 2, 3, 4, 1)) \
        .reshape(-1, C)
    win_cl = winner.reshape(-1, C)
    rb64 = np.asarray(rb, np.int64)
    x, y, zb = rb64 % X, (rb64 // X) % Y, rb64 // (X * Y)          # zb = b*Z + z, Z even
    q = ((zb // 2) * Yo + y // 2) * Xo + x // 2
    k = ((zb % 2) * 2 + y % 2) * 2 + x % 2
    dg = np.zeros(depth.size)
    dg_abs = np.zeros(depth.size)
    fg = torch.zeros(rows.shape, dtype=torch.float64)
    fg_abs = torch.zeros(rows.shape, dtype=torch.float64)
    for s in range(0, len(rb), chunk):
        e = min(len(rb), s + chunk)
        m = np.where(win_cl[q[s:e]] == k[s:e, None], g_cl[q[s:e]], 0.0).astype(np.float64)
        t = m * rows[rf[s:e]].astype(np.float64)
        dg[rd[s:e]] = t.sum(1)                       # every kept point has its own rd
        dg_abs[rd[s:e]] = np.abs(t).sum(1)
        t = torch.from_numpy(m * depth[rd[s:e]].astype(np.float64)[:, None])
        ri = torch.from_numpy(np.asarray(rf[s:e], np.int64))
        fg.index_add_(0, ri, t)
        fg_abs.index_add_(0, ri, t.abs())
    n_pix = np.bincount(rf, minlength=rows.shape[0]).astype(np.float64)
    return dict(out=out, winner=winner, dg=dg, dg_bound=2 * C * EPS * dg_abs,
                fg=fg.numpy(), fg_bound=2 * n_pix[:, None] * EPS * fg_abs.numpy())


def _check_grads(exp, depth_grad, feat_grad, what=''):
    for name, got, key in (('depth_grad', depth_grad, 'dg'), ('feat_grad', feat_grad, 'fg')):
        if got is None:
            continue
        got = got.detach().cpu().numpy().astype(np.float64).reshape(exp[key].shape)
        err, bound = np.abs(got - exp[key]), exp[key + '_bound']
        worst = float((err - bound).max()) if err.size else 0.0
        print('%s %s: max |err| %.3e, max bound %.3e, entries with terms %d of %d'
              % (what, name, err.max() if err.size else 0.0,
                 bound.max() if bound.size else 0.0, int((bound > 0).sum()), bound.size))
        assert worst <= 0.0, (what, name, worst)
        assert not got[bound == 0].any(), (what, name)    # exact zeros without terms


def _features(rng, n_rows, C):
    """ReLU-ed normals (ties at zero inside blocks) with zeroed and negated channels."""
    f = np.maximum(rng.standard_normal((n_rows, C)), 0.0).astype(np.float32)
    kind = rng.integers(0, 4, C)
    kind[:min(2, C)] = (1, 2)[:min(2, C)]
    f[:, kind == 1] = 0.0
    f[:, kind == 2] *= -1.0
    return f


def _lift_case(rng, C, occ_p, heavy, dims=None):
    """Random points in the lift's layout: a subset of the B*N*D*H*W table entries,
    each with a random voxel, stably sorted by voxel."""
    n_img, D, H, W = dims or (int(rng.integers(1, 5)), int(rng.choice([3, 40, 64, 88])),
                              int(rng.integers(2, 6)), int(rng.integers(3, 12)))
    B = int(rng.integers(1, 3))
    Z, Y, X = 2 * int(rng.integers(1, 3)), 2 * int(rng.integers(1, 5)), \
        2 * int(rng.integers(1, 40))
    nvox, table = B * Z * Y * X, n_img * D * H * W
    keep = np.nonzero(rng.random(table) < rng.choice([0.3, 0.7, 1.0]))[0]
    allowed = np.nonzero(rng.random(nvox) < occ_p)[0]
    if len(allowed) == 0:
        allowed = rng.integers(0, nvox, 1)
    vox = allowed[rng.integers(0, len(allowed), len(keep))]
    if heavy:   # a few voxels with 60-700 points: warm and hot lists of the forward
        perm, pos = rng.permutation(len(keep)), 0
        for cnt in (int(rng.integers(60, 200)), int(rng.integers(300, 700)),
                    int(rng.integers(60, 700))):
            cnt = min(cnt, len(keep) - pos)
            vox[perm[pos:pos + cnt]] = rng.integers(0, nvox)
            pos += cnt
    order = np.argsort(vox, kind='stable')
    rd = keep[order].astype(np.int32)
    rb = vox[order].astype(np.int32)
    rf = ((rd // (D * H * W)) * (H * W) + rd % (H * W)).astype(np.int32)
    st, ln = helpers.bp_intervals(rb) if len(rb) else (np.zeros(0, np.int32),) * 2
    depth = rng.random((1, n_img, D, H, W), dtype=np.float32)
    feat = _features(rng, n_img * H * W, C).reshape(1, n_img, H, W, C)
    return depth, feat, (rb, rd, rf, st, ln), (B, Z, Y, X, C), (n_img, D, H, W)


def _pooled_counts(rb, shape):
    B, Z, Y, X, _ = shape
    rb = np.asarray(rb, np.int64)
    q = (((rb // (X * Y)) // 2) * (Y // 2) + ((rb // X) % Y) // 2) * (X // 2) + (rb % X) // 2
    return np.bincount(q, minlength=1)


def _run_op(depth, feat, ranks, shape, layout, gout, depth_grad=True):
    d = dev(depth).requires_grad_(depth_grad)
    f = dev(feat).requires_grad_()
    rb, rd, rf, st, ln = (dev(a) for a in ranks)
    out = bp.bev_pool_v2_maxpool(d, f, rd, rf, rb, shape, st, ln, (2, 2, 2),
                                 lift_layout=layout)
    out.backward(dev(gout))
    return out.detach(), d.grad, f.grad


# ------------------------------------------------------------------- op level
@pytest.mark.parametrize('C', [4, 64, 80, 256, 264, 512])
def test_op_random_lift_cases(C):
    rng = np.random.default_rng(300 + C)
    seen = np.zeros(3, bool)          # cold / warm / hot lists of the forward
    cases = [(0.02, False, None), (0.3, True, (4, 88, 4, 9)), (0.9, True, (3, 64, 5, 11)),
             (0.3, False, None)]
    for rep, (occ_p, heavy, dims) in enumerate(cases):
        depth, feat, ranks, shape, layout = _lift_case(rng, C, occ_p, heavy, dims)
        rb, rd, rf, st, ln = ranks
        cnt = _pooled_counts(rb, shape)
        seen |= [((cnt > 0) & (cnt <= 64)).any(), ((cnt > 64) & (cnt <= 256)).any(),
                 (cnt > 256).any()]
        B, Z, Y, X, _ = shape
        gout = rng.standard_normal((B, C, Z // 2, Y // 2, X // 2)).astype(np.float32)
        exp = _expected(depth, feat, rb, rd, rf, shape, gout)
        with torch.no_grad():
            plain = bp.bev_pool_v2_maxpool(dev(depth), dev(feat), dev(rd), dev(rf), dev(rb),
                                           shape, dev(st), dev(ln), (2, 2, 2))
        assert np.array_equal(plain.cpu().numpy(), exp['out']), rep
        before = _calls(NEW_FWD, NEW_BWD, NEW_TAB, 'veon_bev_pool_v2_bwd',
                        'veon_bev_pool_v2_fwd_rows')
        out, dg, fg = _run_op(depth, feat, ranks, shape, layout, gout)
        after = _calls(NEW_FWD, NEW_BWD, NEW_TAB, 'veon_bev_pool_v2_bwd',
                       'veon_bev_pool_v2_fwd_rows')
        assert [a - b for a, b in zip(after, before)] == [1, 1, 1, 0, 0], rep
        assert torch.equal(out, plain), rep
        # the winner volume, everywhere
        vs = bp.build_voxel_table(dev(rb), dev(st), B, Z * Y * X, attach=False)
        out2, winner = bp.rows_maxpool_winner(dev(depth), dev(feat), dev(rd), dev(rf), vs,
                                              shape)
        assert torch.equal(out2, plain), rep
        assert np.array_equal(winner.cpu().numpy(), exp['winner']), rep
        # the point table
        pvox = bp.build_point_table(dev(rd), dev(rb), depth.size, B * Z * Y * X)
        want_tab = np.full(depth.size, -1, np.int32)
        want_tab[rd] = rb
        assert np.array_equal(pvox.cpu().numpy(), want_tab), rep
        _check_grads(exp, dg, fg, 'C=%d case %d' % (C, rep))
        assert dg.shape == depth.shape and fg.shape == feat.shape
        # run to run, and without the depth gradient: the same bits
        out_b, dg_b, fg_b = _run_op(depth, feat, ranks, shape, layout, gout)
        assert torch.equal(out_b, out) and torch.equal(dg_b, dg) and torch.equal(fg_b, fg)
        out_c, dg_c, fg_c = _run_op(depth, feat, ranks, shape, layout, gout, depth_grad=False)
        assert dg_c is None and torch.equal(fg_c, fg) and torch.equal(out_c, out)
    assert seen.all(), seen


def test_point_table_from_device_counts():
    """Capacity-sized rank buffers with the sizes on the device (sync-free prepare)."""
    rng = np.random.default_rng(7)
    depth, feat, ranks, shape, layout = _lift_case(rng, 8, 0.3, False, (2, 5, 3, 4))
    rb, rd, rf, st, ln = ranks
    B, Z, Y, X, _ = shape
    n, pad = len(rb), 37
    junk = np.full(pad, 5, np.int32)        # beyond the count: must not be read as points
    counts = dev(np.array([n, len(st)], np.int32))
    pvox = bp.build_point_table(dev(np.concatenate([rd, junk])),
                                dev(np.concatenate([rb, junk])), depth.size,
                                B * Z * Y * X, counts=counts)
    want = np.full(depth.size, -1, np.int32)
    want[rd] = rb
    assert np.array_equal(pvox.cpu().numpy(), want)


def test_negative_sums_against_empty_neighbours_in_lift_layout():
    """The hand-made block of tests/test_pool_rows_gpu.py in the lift's layout: an
    all-negative full block sends the gradient to its first-largest child; a lone
    negative child loses against the zeros of its empty neighbours (code 255) and
    no gradient flows."""
    C = 4
    B, Z, Y, X = 1, 2, 2, 4
    vox = [z * Y * X + y * X + x for z in range(2) for y in range(2) for x in range(2)]
    vox += [2]
    rb = np.array(sorted(vox), np.int32)
    n = len(rb)
    n_img, D, H, W = 1, n, 1, 1               # one pixel, one depth bin per point
    rd = np.arange(n, dtype=np.int32)
    rf = np.zeros(n, np.int32)
    st, ln = helpers.bp_intervals(rb)
    # the child sums are -depth: two equal largest ones, the first of them wins
    dvals = np.linspace(2, 1, n, dtype=np.float32)
    dvals[rb == 5] = dvals[rb == 13] = 0.5     # children 3 (z0 y1 x1) and 7 (z1 y1 x1)
    depth = dvals.reshape(1, n_img, D, H, W)
    feat = -np.ones((1, n_img, H, W, C), np.float32)
    shape = (B, Z, Y, X, C)
    gout = np.arange(1, 1 + 2 * C, dtype=np.float32).reshape(1, C, 1, 1, 2)
    exp = _expected(depth, feat, rb, rd, rf, shape, gout)
    assert (exp['winner'][0, 0, 0, 0] == 3).all() and (exp['winner'][0, 0, 0, 1] == 255).all()
    assert (exp['out'][0, :, 0, 0, 0] == -0.5).all() and (exp['out'][0, :, 0, 0, 1] == 0).all()
    vs = bp.build_voxel_table(dev(rb), dev(st), B, Z * Y * X, attach=False)
    out, winner = bp.rows_maxpool_winner(dev(depth), dev(feat), dev(rd), dev(rf), vs, shape)
    assert np.array_equal(out.cpu().numpy(), exp['out'])
    assert np.array_equal(winner.cpu().numpy(), exp['winner'])
    out, dg, fg = _run_op(depth, feat, (rb, rd, rf, st, ln), shape, (n_img, D, H, W), gout)
    _check_grads(exp, dg, fg, 'hand-made block')
    dg = dg.cpu().numpy().reshape(-1)
    first = int(np.nonzero(rb == 5)[0][0])
    assert dg[first] == -gout[0, :, 0, 0, 0].sum() and np.count_nonzero(dg) == 1
    assert np.array_equal(fg.cpu().numpy().reshape(C), 0.5 * gout[0, :, 0, 0, 0])


def test_op_without_lift_layout_or_grad_is_unchanged():
    rng = np.random.default_rng(9)
    depth, feat, ranks, shape, layout = _lift_case(rng, 64, 0.3, False, (2, 5, 3, 4))
    rb, rd, rf, st, ln = (dev(a) for a in ranks)
    before = _calls(NEW_FWD, NEW_BWD)
    with torch.no_grad():
        a = bp.bev_pool_v2_maxpool(dev(depth), dev(feat), rd, rf, rb, shape, st, ln, (2, 2, 2))
        b = bp.bev_pool_v2_maxpool(dev(depth), dev(feat).requires_grad_(), rd, rf, rb, shape,
                                   st, ln, (2, 2, 2), lift_layout=layout)
    c = bp.bev_pool_v2_maxpool(dev(depth), dev(feat), rd, rf, rb, shape, st, ln, (2, 2, 2),
                               lift_layout=layout)          # nothing requires grad
    assert _calls(NEW_FWD, NEW_BWD) == before
    assert torch.equal(a, b) and torch.equal(a, c) and not c.requires_grad
    f = dev(feat).requires_grad_()
    with pytest.raises(_lib.VeonHipError):
        bp.bev_pool_v2_maxpool(dev(depth), f, rd, rf, rb, shape, st, ln, (2, 2, 2),
                               lift_layout=(layout[0] + 1,) + layout[1:])


# ----------------------------------------------------------------- neck level
def _grid(g):
    return {'x': list(g['grid_x']), 'y': list(g['grid_y']),
            'z': list(g['grid_z']), 'depth': list(g['grid_depth'])}


def _neck(g, mode):
    vt = build_neck(dict(
        type='LSSViewTransformerRaw', grid_config=_grid(g),
        input_size=tuple(int(v) for v in g['input_size']), downsample=16,
        out_channels=int(g['feat'].shape[2]), collapse_z=False,
        accelerate=(mode == 'accelerate'), ds_feat=[int(v) for v in g['ds_feat']])).to(DEV)
    vt.sync_free = (mode == 'sync_free')
    return vt


def _inputs(g):
    return [dev(g[k]) for k in ('sensor2ego', 'ego2global', 'intrins',
                                'post_rots', 'post_trans', 'bda')]


def _neck_ranks(vt, inp, mode):
    """The (integer) ranks the neck's configured prepare produces, on the host."""
    sensor2ego, _, cam2imgs, post_rots, post_trans, bda = inp
    if mode == 'accelerate':
        r = (vt.ranks_bev, vt.ranks_depth, vt.ranks_feat)
    elif mode == 'sync_free':
        pre = _prep._HIP_PREPARE.prepare_cameras(
            vt.frustum, sensor2ego, cam2imgs, post_rots, post_trans, bda,
            vt.grid_lower_bound, vt.grid_interval, vt.grid_size, owner=vt)
        n = int(pre.counts[0])
        r = (pre.ranks_bev[:n], pre.ranks_depth[:n], pre.ranks_feat[:n])
    else:
        pri, comb, trans = _prep.camera_matrices(sensor2ego, cam2imgs, post_rots)
        r = _prep.prepare_from_matrices(
            vt.frustum, pri, post_trans, comb, trans, bda,
            vt.grid_lower_bound, vt.grid_interval, vt.grid_size)[:3]
    return [t.cpu().numpy().astype(np.int32) for t in r]


def _neck_expected(g, vt, inp, mode, gout):
    rb, rd, rf = _neck_ranks(vt, inp, mode)
    assert np.all(rb[1:] >= rb[:-1]) and len(np.unique(rd)) == len(rd)
    B, N, C, H, W = g['feat'].shape
    X, Y, Z = (int(v) for v in g['grid_size'])
    rows = np.ascontiguousarray(g['feat'].transpose(0, 1, 3, 4, 2))
    return _expected(g['two_hot'], rows, rb, rd, rf, (B, Z, Y, X, C), gout)


@pytest.mark.parametrize('name', ['lss_small', 'lss_small_b2', 'lss_mid'])
@pytest.mark.parametrize('mode', ['percall', 'accelerate', 'sync_free'])
def test_neck_fused_training_path(name, mode):
    g = load_golden(name)
    assert [int(v) for v in g['ds_feat']] == [2, 2, 2] and g['feat'].shape[2] % 4 == 0
    inp = _inputs(g)
    vt = _neck(g, mode)
    with torch.no_grad():
        plain = vt([dev(g['feat'])] + inp, dev(g['two_hot']))     # the fused inference path
    rng = np.random.default_rng(17)
    gout = rng.standard_normal(tuple(plain.shape)).astype(np.float32)
    vt.fuse_ds_grad = True
    assert vt._can_fuse_ds(dev(g['feat']))
    before = _calls(NEW_FWD, NEW_BWD, 'veon_bev_pool_v2_bwd', 'veon_bev_pool_v2_fwd_rows')
    f = dev(g['feat']).requires_grad_()
    d = dev(g['two_hot']).requires_grad_()
    out = vt([f] + inp, d)
    out.backward(dev(gout))
    after = _calls(NEW_FWD, NEW_BWD, 'veon_bev_pool_v2_bwd', 'veon_bev_pool_v2_fwd_rows')
    assert [a - b for a, b in zip(after, before)] == [1, 1, 0, 0]
    assert torch.equal(out.detach(), plain)
    exp = _neck_expected(g, vt, inp, mode, gout)
    assert np.array_equal(plain.cpu().numpy(), exp['out'])
    B, N, C, H, W = g['feat'].shape
    fg_rows = f.grad.permute(0, 1, 3, 4, 2).contiguous()          # (B,N,H,W,C) rows
    _check_grads(exp, d.grad, fg_rows, '%s %s' % (name, mode))
    # a second step (cached tables in accelerate mode): the same bits
    f2 = dev(g['feat']).requires_grad_()
    out2 = vt([f2] + inp, dev(g['two_hot']))
    out2.backward(dev(gout))
    assert torch.equal(out2.detach(), plain) and torch.equal(f2.grad, f.grad)
    # out_volume cannot carry a gradient
    with pytest.raises(ValueError):
        vt([f2] + inp, dev(g['two_hot']), out_volume=object())


@pytest.mark.parametrize('mode', ['percall', 'sync_free'])
def test_neck_fused_training_path_takes_two_hot_windows_densified(mode):
    """A ``TwoHotWindows`` depth has no compact form under autograd: the fused training
    path lifts its dense tensor, exactly as if that tensor had been passed."""
    g = load_golden('lss_small_b2')
    inp = _inputs(g)
    vt = _neck(g, mode)
    vt.fuse_ds_grad = True
    tw = vt.get_two_hot_windows(dev(g['metric_depth']), downsample=8)
    dense = tw.dense()
    assert tuple(dense.shape) == tuple(g['two_hot'].shape)
    grads, outs = [], []
    before = _calls(NEW_FWD, NEW_BWD)
    for depth in (tw, dense):
        f = dev(g['feat']).requires_grad_()
        out = vt([f] + inp, depth)
        out.sum().backward()
        outs.append(out.detach())
        grads.append(f.grad)
    assert [a - b for a, b in zip(_calls(NEW_FWD, NEW_BWD), before)] == [2, 2]
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])
    assert grads[0].abs().sum() > 0


@pytest.mark.parametrize('name', ['lss_small_b2', 'lss_mid'])
def test_neck_unfused_structure_with_the_flag_has_the_reference_gradient(name):
    """Where the fused kernels do not apply (here: fuse_ds switched off) the flag still
    means the reference's gradient: first maximal element, not amax's even split."""
    g = load_golden(name)
    inp = _inputs(g)
    vt = _neck(g, 'percall')
    vt.fuse_ds = False
    vt.fuse_ds_grad = True
    rng = np.random.default_rng(18)
    f = dev(g['feat']).requires_grad_()
    d = dev(g['two_hot']).requires_grad_()
    before = _calls(NEW_FWD, NEW_BWD, 'veon_bev_pool_v2_bwd')
    out = vt([f] + inp, d)
    gout = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(dev(gout))
    after = _calls(NEW_FWD, NEW_BWD, 'veon_bev_pool_v2_bwd')
    assert [a - b for a, b in zip(after, before)] == [0, 0, 1]
    exp = _neck_expected(g, vt, inp, 'percall', gout)
    assert np.array_equal(out.detach().cpu().numpy(), exp['out'])
    _check_grads(exp, d.grad, f.grad.permute(0, 1, 3, 4, 2).contiguous(), name + ' unfused')


@pytest.mark.parametrize('name', ['lss_small_b2', 'lss_mid'])
def test_neck_default_is_untouched(name):
    """Flag off: output and gradients are what the un-fused structure with amax gives,
    restated here from the op (bev_pool_v2 under autograd, then amax)."""
    g = load_golden(name)
    inp = _inputs(g)
    vt = _neck(g, 'percall')
    assert vt.fuse_ds_grad is False
    rng = np.random.default_rng(19)
    f = dev(g['feat']).requires_grad_()
    d = dev(g['two_hot']).requires_grad_()
    before = _calls(NEW_FWD, NEW_BWD, NEW_TAB, 'veon_bev_pool_v2_bwd')
    out = vt([f] + inp, d)
    gout = dev(rng.standard_normal(tuple(out.shape)).astype(np.float32))
    out.backward(gout)
    after = _calls(NEW_FWD, NEW_BWD, NEW_TAB, 'veon_bev_pool_v2_bwd')
    assert [a - b for a, b in zip(after, before)] == [0, 0, 0, 1]
    rb, rd, rf = (dev(a) for a in _neck_ranks(vt, inp, 'percall'))
    st, ln = (dev(a) for a in helpers.bp_intervals(rb.cpu().numpy()))
    B, N, C, H, W = g['feat'].shape
    X, Y, Z = (int(v) for v in g['grid_size'])
    f2 = dev(g['feat']).requires_grad_()
    d2 = dev(g['two_hot']).requires_grad_()
    vol = bp.bev_pool_v2(d2, f2.permute(0, 1, 3, 4, 2), rd, rf, rb, (B, Z, Y, X, C), st, ln)
    ref = vol.view(B, C, Z // 2, 2, Y // 2, 2, X // 2, 2).amax(dim=(3, 5, 7))
    ref.backward(gout)
    assert torch.equal(out.detach(), ref.detach())
    assert torch.equal(f.grad, f2.grad) and torch.equal(d.grad, d2.grad)
    # and amax is NOT the first-max gradient on this input (ties are the normal case)
    vt.fuse_ds_grad = True
    f3 = dev(g['feat']).requires_grad_()
    vt([f3] + inp, dev(g['two_hot'])).backward(gout)
    assert not torch.equal(f3.grad, f.grad)


# ----------------------------------------------------------------- VEON shape
def test_veon_shape_training_step_never_holds_the_unpooled_volume():
    """SV: 6 cams 512x1408, D=88, C=256 into 200x200x16.  Forward bit-equal, gradients
    against the CPU construction, and the peak allocation of forward + backward below
    the byte size of the un-pooled volume (655.36 MB), which any path that
    materialises it cannot meet."""
    ranks, coor, rig, fr, gsize = helpers.oracle_ranks(synthetic.GRID_VEON, (512, 1408), 6)
    D, C, H, W = fr.shape[0], 256, 32, 88
    depth, feat = synthetic.make_depth_feat(1, 6, D, C, H, W, 0)
    rows = feat.permute(0, 1, 3, 4, 2).contiguous().numpy()
    depth = depth.numpy()
    shape = (1, int(gsize[2]), int(gsize[1]), int(gsize[0]), C)
    B, Z, Y, X, _ = shape
    rb, rd, rf, st, ln = ranks
    rng = np.random.default_rng(23)
    gout = rng.standard_normal((B, C, Z // 2, Y // 2, X // 2)).astype(np.float32)
    drb, drd, drf, dst, dln = (dev(a) for a in ranks)
    d = dev(depth).requires_grad_()
    f = dev(rows).requires_grad_()
    g_dev = dev(gout)
    with torch.no_grad():
        plain = bp.bev_pool_v2_maxpool(dev(depth), dev(rows), drd, drf, drb, shape, dst, dln,
                                       (2, 2, 2)).cpu()
    for attr in ('_veon_vstart', '_veon_pvox'):     # tables are part of the step's memory
        if hasattr(dst, attr):
            delattr(dst, attr)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = bp.bev_pool_v2_maxpool(d, f, drd, drf, drb, shape, dst, dln, (2, 2, 2),
                                 lift_layout=(6, D, H, W))
    out.backward(g_dev)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    volume_bytes = B * C * Z * Y * X * 4
    print('SV training step: peak allocation above the resident inputs %.1f MB '
          '(un-pooled volume %.2f MB)' % (peak / 1e6, volume_bytes / 1e6))
    assert peak < volume_bytes
    assert torch.equal(out.detach().cpu(), plain)
    exp = _expected(depth, rows, rb, rd, rf, shape, gout)
    assert np.array_equal(plain.numpy(), exp['out'])
    _check_grads(exp, d.grad, f.grad, 'SV')
