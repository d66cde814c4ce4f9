"""The two-stage column sums of the BatchNorm and LayerNorm passes on the MI355X at their
seams (``bn_sums``, ``bn_bwd_sums``, ``colsum``, ``layernorm_f32_bwd``,
``image_layernorm_bwd``; csrc/conv3d_train.hip, linear_train.hip, conv2d_train.hip,
ln_common.h; DESIGN sections 4k - 4m), shape by shape of tests/reduce_seams.py (the CPU
file asserts what makes each row a seam), and the same passes on degenerate statistics.

Operands are written into ``PaddedVolume(...).interior()`` / ``PaddedImage(...).interior()``
of a fresh zeroed grid, so no test depends on the widths the pack kernels accept.  The
BatchNorm sums, which walk halo rows like any other, are also run with operands on every
padded row (see ``FILLS``): with a zero halo most of their last blocks add only zeros.

Yardsticks (none of them taken from the code under test):
 * integer operands, on which every fp32 summation order is exact: equality with the
   fp64 sum;
 * one live row: the sum is a single term, compared with the fp64 closed forms
   (``ln_gelu_backward_ref``, ``bn_train_backward_ref``) under a bound counted in fp32
   roundings of that term; a dropped row gives 0, a doubled one twice the term;
 * NaN in every cached workspace before a repeated call: bit-equal, finite results;
 * constant rows and channels: the closed forms at variance 0, in fp64.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import reduce_seams as rs
from tests.helpers import flavour, fp16_twin, half_tol, halo_is_zero  # noqa: F401
from veon_amd import conv3d_ops, half, vit_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
U = 2.0 ** -24                  # unit roundoff of fp32
GRID = {'bn': conv3d_ops.PaddedVolume, 'ln_image': conv3d_ops.PaddedImage}


def RTOL():
    """The largest relative error of one rounding to the flavour's half: 2^-8 (bf16, 8
    significant bits) or 2^-11 (fp16), the rtol of ``_within_half_rounding``."""
    return half_tol(2.0 ** -8, 0.0)['rtol']


def _gen(shape, salt=0):
    return torch.Generator().manual_seed(sum(shape) + 7 * len(shape) + salt)


def _ints(size, g):
    """Integers in [-4, 4], none zero."""
    return (torch.randint(1, 5, size, generator=g) *
            (2 * torch.randint(0, 2, size, generator=g) - 1)).float()


def _grid(kind, shape, values=None, fill='interior'):
    """A fresh zeroed grid of the shape with ``values`` on its interior (B, spatial.., C),
    or with fill='padded' on EVERY padded row (M, C), the halo included."""
    grid = GRID[kind](*shape, DEV)
    if values is not None:
        (grid.interior() if fill == 'interior' else grid.rows).copy_(values.to(DEV))
    return grid


def _size(kind, shape, fill):
    """The size of the values ``_grid`` takes with this fill."""
    return _cl(shape) if fill == 'interior' else (rs.plan_of(kind, shape)['M'], shape[1])


# The BatchNorm sums walk all M padded rows alike and rely on the halo holding zeros.  With
# a zero halo the last block of most 'bn' rows of the table (and block 1 of all but one)
# lies in a halo plane and adds zeros, whatever the r1 clamp or stage two do with it; so
# the exact tests also run with integers on every padded row, where every block counts.
FILLS = ['interior', 'padded']


def _cl(shape):
    """(B, spatial.., C) of a (B, C, spatial..) shape."""
    B, C, *spatial = shape
    return (B, *spatial, C)


def _spatial(t):
    return list(range(t.dim() - 1))


def _within_half_rounding(got, want):
    rms = want.pow(2).mean().sqrt().item()
    tol = half_tol(2.0 ** -8, 2e-3)
    return bool(((got - want).abs() <= want.abs() * tol['rtol'] + tol['atol'] * rms).all())


def _balanced(C, g):
    """C values from {+-1, +-3} in a random order, each a quarter of them: the mean is
    exactly 0 and the variance exactly 5."""
    assert C % 8 == 0
    return torch.tensor([1., -1., 3., -3.]).repeat(C // 4)[torch.randperm(C, generator=g)]


# =========================================================== (a) integer operands, exact
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('shape', rs.shapes_of('bn'), ids=rs.ids_of('bn'))
def test_bn_sums_on_integers_are_exact(shape, fill, flavour):
    """y: integers in [-4, 4], none zero, on every interior voxel with a zero halo, or on
    every padded row: sum y and sum y^2 are integers below 2^24 at every step of any order,
    so both EQUAL the fp64 sums."""
    y = _grid('bn', shape, _ints(_size('bn', shape, fill), _gen(shape)), fill)
    assert halo_is_zero(y) == (fill == 'interior')
    got = conv3d_ops.bn_sums(y)
    y64 = y.rows.double()
    want = torch.stack([y64.sum(_spatial(y64)), (y64 * y64).sum(_spatial(y64))])
    assert float(want[1].max()) < 2.0 ** 24 and float(want[1].min()) > 0
    assert got.dtype == torch.float32 and torch.equal(got.double(), want)


test_bn_sums_on_integers_are_exact_fp16 = fp16_twin(test_bn_sums_on_integers_are_exact)


@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('mask', ['positive', 'masked'])
@pytest.mark.parametrize('shape', rs.shapes_of('bn'), ids=rs.ids_of('bn'))
def test_bn_bwd_sums_on_integers_are_exact(shape, mask, fill, flavour):
    """da, y: integers in [-4, 4]; mean: integers in [-2, 2]; rstd: powers of two in
    {1/2, 1, 2}: xhat = (y - mean) rstd is exact, |dz xhat| <= 48 in steps of 1/2, and both
    sums EQUAL the fp64 ones (48 M < 2^24).  a: strictly positive, or zero on a random
    half of the voxels (the ReLU mask).  Operands on the interior with a zero halo, or on
    every padded row."""
    C = shape[1]
    g = _gen(shape, 1)
    size = _size('bn', shape, fill)
    da = _grid('bn', shape, _ints(size, g), fill)
    y = _grid('bn', shape, _ints(size, g), fill)
    a_val = torch.randint(1, 5, size, generator=g).float()
    if mask == 'masked':
        a_val = a_val * torch.randint(0, 2, size, generator=g)
    a = _grid('bn', shape, a_val, fill)
    mean = torch.randint(-2, 3, (C,), generator=g).float().to(DEV)
    rstd = (2.0 ** torch.randint(-1, 2, (C,), generator=g).float()).to(DEV)
    got = conv3d_ops.bn_bwd_sums(da, a, y, mean, rstd)
    d64, a64, y64 = da.rows.double(), a.rows.double(), y.rows.double()
    dz = d64 * (a64 > 0)
    xhat = (y64 - mean.double()) * rstd.double()
    red = _spatial(y64)
    want = torch.stack([dz.sum(red), (dz * xhat).sum(red)])
    assert float((dz * xhat).abs().sum(red).max()) < 2.0 ** 23
    assert float(dz.abs().sum()) > 0
    assert torch.equal(got.double(), want)


test_bn_bwd_sums_on_integers_are_exact_fp16 = fp16_twin(test_bn_bwd_sums_on_integers_are_exact)


@pytest.mark.parametrize('shape', rs.shapes_of('colsum'), ids=rs.ids_of('colsum'))
def test_colsum_on_integers_is_exact(shape, flavour):
    dy = _ints(shape, _gen(shape)).to(half.dtype()).to(DEV)
    got = vit_ops.colsum(dy)
    assert got.shape == (shape[1],) and got.dtype == torch.float32
    assert torch.equal(got.double(), dy.double().sum(0))


test_colsum_on_integers_is_exact_fp16 = fp16_twin(test_colsum_on_integers_is_exact)


@pytest.mark.parametrize('shape', rs.shapes_of('ln_tokens'), ids=rs.ids_of('ln_tokens'))
def test_ln_tokens_dbeta_on_integers_is_exact(shape, flavour):
    """dbeta = sum dout of ``layernorm_f32_bwd`` on integer dout (fp32 and half), Gaussian
    x: EQUAL to the fp64 sum; dx and dgamma finite."""
    T, d = shape
    g = _gen(shape)
    x = (torch.randn(T, d, generator=g) * 1.5 + 0.3).to(DEV)
    gamma = (torch.rand(d, generator=g) + 0.5).to(DEV)
    dout = _ints(shape, g).to(DEV)
    for dt in (dout, dout.to(half.dtype())):
        dx, dg, db = vit_ops.layernorm_f32_bwd(dt, x, gamma, EPS)
        assert torch.equal(db.double(), dout.double().sum(0))
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dg).all())


test_ln_tokens_dbeta_on_integers_is_exact_fp16 = fp16_twin(
    test_ln_tokens_dbeta_on_integers_is_exact)


@pytest.mark.parametrize('shape', rs.shapes_of('ln_image'), ids=rs.ids_of('ln_image'))
def test_ln_image_dbeta_on_integers_is_exact(shape, flavour):
    """sums[1] = sum dout of ``image_layernorm_bwd`` in its four variants (GELU in front or
    not, dout a padded half image or fp32 tokens) on integer dout: EQUAL to the fp64 sum."""
    B, C, Y, X = shape
    g = _gen(shape)
    x = _grid('ln_image', shape, torch.randn(_cl(shape), generator=g) * 1.5 + 0.3)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    d_val = _ints(_cl(shape), g)
    dimg = _grid('ln_image', shape, d_val)
    dtok = d_val.reshape(B, Y * X, C).contiguous().to(DEV)
    want = d_val.double().sum((0, 1, 2)).to(DEV)
    for gelu in (False, True):
        for dout in (dimg, dtok):
            dx, sums = conv3d_ops.image_layernorm_bwd(dout, x, gamma, EPS, gelu_in=gelu)
            assert torch.equal(sums[1].double(), want), (gelu, torch.is_tensor(dout))
            assert bool(torch.isfinite(sums).all()) and halo_is_zero(dx)


test_ln_image_dbeta_on_integers_is_exact_fp16 = fp16_twin(
    test_ln_image_dbeta_on_integers_is_exact)


# ===================================================================== (b) one live row
def _ln_row_reference(dout, x, gamma, gelu):
    """fp64, of the one live row: dx, dgamma, dbeta and the bound of dgamma per channel,
    9 2^-24 |dout| (|u - mean| + |u| + |mean|) rstd with u = x or GELU(x)."""
    d64, x64, g64 = dout.double()[None], x.double()[None], gamma.double()
    dx64, dg64, db64 = conv3d_ops.ln_gelu_backward_ref(d64, x64, g64, EPS, gelu)
    u = F.gelu(x64[0]) if gelu else x64[0]
    mean = u.mean()
    rstd = ((u - mean).square().mean() + EPS).rsqrt()
    bound = 9 * U * d64[0].abs() * ((u - mean).abs() + u.abs() + mean.abs()) * rstd
    return dx64[0], dg64, db64, bound


@pytest.mark.parametrize('shape', rs.shapes_of('ln_tokens'), ids=rs.ids_of('ln_tokens'))
def test_ln_tokens_one_live_row(shape, flavour):
    """dout is zero but for one row r, at each row of ``reduce_seams.live_rows``: dgamma
    is the single term dout[r] xhat[r] within 9 2^-24 |dout| (|x - mean| + |x| + |mean|)
    rstd per channel (the T + 8 of test_row_passes_against_fp64 at T = 1), dbeta EQUALS
    dout[r], dx[r] is within 1e-5 of the row's RMS of the fp64 one, and dx is exactly zero
    on every other row.  The live row of x holds {+-1, +-3} with mean exactly 0 and
    variance exactly 5; the other rows are Gaussian.  Measured on an MI355X: the largest
    dgamma error is 0.084 of the bound, the largest dx error 5.3e-7 of the row's RMS
    (0.082 and 4.4e-7 in bf16); the 9 did not have to move."""
    T, d = shape
    g = _gen(shape, 2)
    x = (torch.randn(T, d, generator=g) * 1.5 + 0.3).to(DEV)
    gamma = (torch.rand(d, generator=g) + 0.5).to(DEV)
    live_x = _balanced(d, g).to(DEV)
    live_d = torch.randn(d, generator=g).to(half.dtype()).float().to(DEV)
    dx64, dg64, db64, bound = _ln_row_reference(live_d, live_x, gamma, False)
    rms = dx64.pow(2).mean().sqrt()
    assert float(dg64.abs().min()) > 0
    worst_g = worst_x = 0.0
    for as_half in (False, True):
        dout = torch.zeros(T, d, dtype=half.dtype() if as_half else torch.float32, device=DEV)
        for r in rs.live_rows('ln_tokens', shape):
            keep = x[r].clone()
            x[r] = live_x
            dout[r] = live_d
            dx, dg, db = vit_ops.layernorm_f32_bwd(dout, x, gamma, EPS)
            x[r] = keep
            dout[r] = 0
            err = (dg.double() - dg64).abs()
            worst_g = max(worst_g, float((err / bound).max()))
            worst_x = max(worst_x, float(((dx[r].double() - dx64).abs() / rms).max()))
            assert bool((err <= bound).all()), (as_half, r, float((err / bound).max()))
            assert torch.equal(db.double(), db64), (as_half, r)
            assert bool(((dx[r].double() - dx64).abs() <= 1e-5 * rms).all()), (as_half, r)
            dx[r] = 0
            assert float(dx.abs().max()) == 0.0, (as_half, r)
    print('ln tokens live row %s %s: dgamma error %.3f of the bound, dx error %.2e of the '
          'row RMS' % (half.name(), shape, worst_g, worst_x))


test_ln_tokens_one_live_row_fp16 = fp16_twin(test_ln_tokens_one_live_row)


@pytest.mark.parametrize('shape', rs.shapes_of('ln_image'), ids=rs.ids_of('ln_image'))
def test_ln_image_one_live_row(shape, flavour):
    """``image_layernorm_bwd`` in its four variants with dout zero but for one interior
    padded row r, at each row of ``reduce_seams.live_rows``: sums[0] (dgamma) is the single
    term within 9 2^-24 |dout| (|u - mean| + |u| + |mean|) rstd per channel, u = x or
    GELU(x) (the magnitude terms cover the rounding of the mean when GELU comes first);
    sums[1] EQUALS dout[r]; sums[2] (sum dx, fp32 before dx is rounded) is within 1e-5 of
    the row's RMS of the fp64 dx[r]; the half dx[r] is within half rounding of it, and dx
    is exactly zero on every other row, on the halo and in the guard rows.  Measured on an
    MI355X, bf16 / fp16: the largest dgamma error is 0.082 / 0.084 of the bound without
    GELU and 0.30 / 0.31 with it, the largest sum-dx error 1.5e-6 / 1.1e-6 of the row's
    RMS; the 9 did not have to move."""
    B, C, Y, X = shape
    g = _gen(shape, 2)
    x = _grid('ln_image', shape, torch.randn(_cl(shape), generator=g) * 1.5 + 0.3)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    live_x = _balanced(C, g).to(DEV)
    live_d = torch.randn(C, generator=g).to(half.dtype()).float().to(DEV)
    dimg = _grid('ln_image', shape)
    dtok = torch.zeros(B, Y * X, C, device=DEV)
    inner = rs.interior_rows('ln_image', shape)
    worst_g = {False: 0.0, True: 0.0}
    worst_x = 0.0
    for gelu in (False, True):
        dx64, dg64, db64, bound = _ln_row_reference(live_d, live_x, gamma, gelu)
        rms = dx64.pow(2).mean().sqrt()
        assert float(dg64.abs().max()) > 0
        for tokens in (False, True):
            for r in rs.live_rows('ln_image', shape):
                keep = x.rows[r].clone()
                x.rows[r] = live_x
                t = inner.index(r)          # the token of padded row r: (b Y + y - 1) X + x - 1
                if tokens:
                    dtok.view(-1, C)[t] = live_d
                else:
                    dimg.rows[r] = live_d
                dx, sums = conv3d_ops.image_layernorm_bwd(dtok if tokens else dimg, x, gamma,
                                                          EPS, gelu_in=gelu)
                x.rows[r] = keep
                dtok.view(-1, C)[t] = 0
                dimg.rows[r] = 0
                where = (gelu, tokens, r)
                err = (sums[0].double() - dg64).abs()
                worst_g[gelu] = max(worst_g[gelu], float((err / bound.clamp_min(1e-300)).max()))
                assert bool((err <= bound).all()), where
                assert torch.equal(sums[1].double(), db64), where
                err_x = (sums[2].double() - dx64).abs() / rms
                worst_x = max(worst_x, float(err_x.max()))
                assert bool((err_x <= 1e-5).all()), where
                assert _within_half_rounding(dx.rows[r].double(), dx64), where
                assert halo_is_zero(dx), where
                dx.rows[r] = 0
                assert float(dx.rows.float().abs().max()) == 0.0, where
    print('ln image live row %s %s: dgamma error %.3f (plain) %.3f (GELU) of the bound, '
          'sum dx error %.2e of the row RMS' % (half.name(), shape, worst_g[False],
                                                 worst_g[True], worst_x))


test_ln_image_one_live_row_fp16 = fp16_twin(test_ln_image_one_live_row)


@pytest.mark.parametrize('shape', rs.shapes_of('bn'), ids=rs.ids_of('bn'))
def test_bn_bwd_one_live_row(shape, flavour):
    """``bn_bwd_sums`` with da zero but for one padded row r, at each row of
    ``reduce_seams.live_rows`` (the block edges themselves: the kernel treats halo rows
    like any other, so y and a are filled on EVERY padded row here); y Gaussian, a
    positive, mean and rstd ordinary fp32 vectors.  sum dz EQUALS da[r]; sum dz xhat is the single term fl(dz fl(fl(y - mean)
    rstd)): three fp32 roundings, so within 4 2^-24 |dz xhat| of the fp64 product of the
    same fp32 operands.  Measured on an MI355X: at most 0.66 of that bound (0.65 in
    bf16)."""
    C = shape[1]
    g = _gen(shape, 3)
    size = _size('bn', shape, 'padded')
    y = _grid('bn', shape, torch.randn(size, generator=g) * 1.5 + 0.3, 'padded')
    a = _grid('bn', shape, torch.randint(1, 5, size, generator=g).float(), 'padded')
    da = _grid('bn', shape)
    mean = (torch.randn(C, generator=g) * 0.3).to(DEV)
    rstd = (torch.rand(C, generator=g) + 0.5).to(DEV)
    live_d = torch.randn(C, generator=g).to(half.dtype()).float().to(DEV)
    worst = 0.0
    for r in rs.live_rows('bn', shape):
        da.rows[r] = live_d
        got = conv3d_ops.bn_bwd_sums(da, a, y, mean, rstd)
        da.rows[r] = 0
        want = live_d.double() * ((y.rows[r].double() - mean.double()) * rstd.double())
        assert float(want.abs().max()) > 0
        err = (got[1].double() - want).abs()
        worst = max(worst, float((err / (4 * U * want.abs()).clamp_min(1e-300)).max()))
        assert torch.equal(got[0], live_d), r
        assert bool((err <= 4 * U * want.abs()).all()), r
    print('bn bwd live row %s %s: dgamma error %.3f of the bound' % (half.name(), shape, worst))


test_bn_bwd_one_live_row_fp16 = fp16_twin(test_bn_bwd_one_live_row)


# ==================================================================== (c) nothing stale
def _stale_runner(kind, shape):
    """() -> tuple of result tensors of every sum of the kind, on Gaussian operands."""
    g = _gen(shape, 4)
    C = shape[1]
    if kind == 'bn':
        y = _grid('bn', shape, torch.randn(_cl(shape), generator=g) * 1.5 + 0.3)
        da = _grid('bn', shape, torch.randn(_cl(shape), generator=g))
        a = _grid('bn', shape, torch.randn(_cl(shape), generator=g).relu())
        mean = (torch.randn(C, generator=g) * 0.3).to(DEV)
        rstd = (torch.rand(C, generator=g) + 0.5).to(DEV)
        return lambda: (conv3d_ops.bn_sums(y), conv3d_ops.bn_bwd_sums(da, a, y, mean, rstd))
    if kind == 'colsum':
        dy = torch.randn(shape, generator=g).to(half.dtype()).to(DEV)
        return lambda: (vit_ops.colsum(dy),)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    if kind == 'ln_tokens':
        x = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(DEV)
        dout = torch.randn(shape, generator=g).to(DEV)
        dh = dout.to(half.dtype())
        return lambda: (vit_ops.layernorm_f32_bwd(dout, x, gamma, EPS) +
                        vit_ops.layernorm_f32_bwd(dh, x, gamma, EPS))
    B, _, Y, X = shape
    x = _grid('ln_image', shape, torch.randn(_cl(shape), generator=g) * 1.5 + 0.3)
    dimg = _grid('ln_image', shape, torch.randn(_cl(shape), generator=g))
    dtok = torch.randn(B, Y * X, C, generator=g).to(DEV)

    def run():
        out = ()
        for gelu in (False, True):
            for dout in (dimg, dtok):
                dx, sums = conv3d_ops.image_layernorm_bwd(dout, x, gamma, EPS, gelu_in=gelu)
                out += (dx.rows, sums)
        return out
    return run


@pytest.mark.parametrize('kind,shape', rs.STALE, ids=[rs.ident(k, s) for k, s in rs.STALE])
def test_sums_leave_nothing_stale(kind, shape, flavour):
    """Every cached workspace (``conv3d_ops._WORKSPACES``, which ``vit_ops`` shares) holds
    NaN before a second call on the same inputs: the results are finite and bit-equal to
    the first call's, so stage two reads no partial that stage one did not write.  One
    shape on the minimum rows and one capped shape per kind."""
    assert vit_ops._workspace is conv3d_ops._workspace
    run = _stale_runner(kind, shape)
    first = run()                            # makes the wrappers cache their workspaces
    assert conv3d_ops._WORKSPACES
    known = len(conv3d_ops._WORKSPACES)
    for ws in conv3d_ops._WORKSPACES.values():
        ws.fill_(float('nan'))
    second = run()
    assert len(conv3d_ops._WORKSPACES) == known          # the filled tensors were the ones used
    assert len(first) == len(second)
    for a, b in zip(first, second):
        assert bool(torch.isfinite(b.float()).all())
        assert torch.equal(a, b)


test_sums_leave_nothing_stale_fp16 = fp16_twin(test_sums_leave_nothing_stale)


# ============================================================ (d) degenerate statistics
def _ncdhw(vol):
    return vol.interior().permute(0, 4, 1, 2, 3).double()


def test_bn_passes_with_constant_channels(flavour):
    """Channels 3 (all voxels 0, e.g. a region that ReLU emptied) and 5 (all voxels 3) of
    a (2, 16, 3, 5, 6) volume are constant, the others Gaussian.  ``bn_batch_stats``: var
    == 0 exactly, rstd == eps^-1/2 to fp64 rounding.  ``bn_apply``: channel 3 is
    fl(fl(shift) (+ ident)) rounded to half, i.e. beta (relu(beta + ident)) rounded to
    half, EXACTLY; channel 5 computes 3 scale + shift with scale = gamma eps^-1/2 ~ 316
    gamma, where rounding scale and shift to fp32 costs up to 2^-24 (3 scale + |shift|): it
    is beta within half rounding plus 2^-22 * 3 scale.  The backward sums, coefficients
    and ``bn_bwd_apply`` are finite and agree with ``bn_train_backward_ref`` in fp64 as in
    test_bn_passes_against_fp64 (dgamma of a constant channel is exactly 0)."""
    shape = (2, 16, 3, 5, 6)
    B, C, Z, Y, X = shape
    n = B * Z * Y * X
    g = _gen(shape)
    y_val = torch.randn(_cl(shape), generator=g) * 1.5 + 0.3
    y_val[..., 3] = 0.0
    y_val[..., 5] = 3.0
    y = _grid('bn', shape, y_val)
    ident = _grid('bn', shape, torch.randn(_cl(shape), generator=g))
    da = _grid('bn', shape, torch.randn(_cl(shape), generator=g))
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    y64 = _ncdhw(y)
    K = y.M
    red = [0, 2, 3, 4]

    mean, var, rstd = conv3d_ops.bn_batch_stats(conv3d_ops.bn_sums(y), n, EPS)
    assert mean.dtype == torch.float64
    for c, value in ((3, 0.0), (5, 3.0)):
        assert float(mean[c]) == value and float(var[c]) == 0.0
        assert abs(float(rstd[c]) - EPS ** -0.5) <= 4 * 2.0 ** -53 * EPS ** -0.5
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - mean * gamma.double() * rstd).float()
    for ident_v, relu in ((None, True), (ident, True), (None, False)):
        a64, m64, v64, r64 = conv3d_ops.bn_train_forward_ref(
            y64, gamma.double(), beta.double(), EPS,
            None if ident_v is None else _ncdhw(ident_v), relu)
        a = conv3d_ops.bn_apply(y, scale, shift, ident=ident_v, relu=relu)
        assert halo_is_zero(a) and bool(torch.isfinite(a.rows.float()).all())
        got = _ncdhw(a)
        assert _within_half_rounding(got, a64)
        # channel 3: the fp32 value is beta (+ ident) exactly; one rounding to half
        t = beta[3].float().expand(_cl(shape)[:-1])
        if ident_v is not None:
            t = t + ident_v.interior()[..., 3].float()
        t = t.relu() if relu else t
        assert torch.equal(a.interior()[..., 3], t.to(half.dtype()))
        # channel 5: within half rounding of the exact value plus the fp32 rounding of
        # scale and shift at |y scale| = 3 gamma eps^-1/2
        room = RTOL() * a64[:, 5].abs() + 2.0 ** -22 * 3 * float(scale[5])
        assert bool(((got[:, 5] - a64[:, 5]).abs() <= room).all())

    a = conv3d_ops.bn_apply(y, scale, shift, ident=ident, relu=True)
    a64, d64 = _ncdhw(a), _ncdhw(da)
    dy64, dg64, db64, dz64 = conv3d_ops.bn_train_backward_ref(d64, a64, y64, m64, r64,
                                                              gamma.double())
    bs = conv3d_ops.bn_bwd_sums(da, a, y, mean.float(), rstd.float())
    assert bool(torch.isfinite(bs).all())
    xhat = (y64 - m64.view(1, -1, 1, 1, 1)) * r64.view(1, -1, 1, 1, 1)
    want = torch.stack([db64, dg64])
    S = torch.stack([dz64.abs().sum(red), (dz64 * xhat).abs().sum(red)])
    assert bool(((bs.double() - want).abs() <= (K + 4) * U * S).all())
    assert float(bs[1, 3]) == 0.0 and float(bs[1, 5]) == 0.0
    ca, cb, cc = conv3d_ops.bn_bwd_coefficients(bs, n, gamma, mean.float(), rstd.float())
    for v in (ca, cb, cc):
        assert bool(torch.isfinite(v).all())
    dyv, dzv = conv3d_ops.bn_bwd_apply(da, a, y, ca, cb, cc, want_dz=True)
    assert halo_is_zero(dyv) and halo_is_zero(dzv)
    assert bool(torch.isfinite(dyv.rows.float()).all())
    assert _within_half_rounding(_ncdhw(dyv), dy64)
    assert torch.equal(_ncdhw(dzv), dz64)


test_bn_passes_with_constant_channels_fp16 = fp16_twin(test_bn_passes_with_constant_channels)


def test_bn_variance_of_channels_with_a_large_mean(flavour):
    """Integers in [-4, 4] plus an integer offset per channel (0, 16, 64, -64, ...; every
    value exact in half): the fp32 sums are exact (68^2 n < 2^24), so the variance of
    ``bn_batch_stats`` must equal the fp64 two-pass variance up to the fp64 rounding of its
    two terms, 4 2^-53 (E[y^2] + mean^2): the loss its docstring documents, 2^-24 (1 +
    mean^2 / var), is that of the fp32 sums and of nothing else in the algebra."""
    shape = (1, 8, 3, 13, 14)                # 1200 padded rows: two blocks
    B, C, Z, Y, X = shape
    n = B * Z * Y * X
    g = _gen(shape)
    offset = torch.tensor([0., 16., 64., -64., 32., -16., 60., -60.])
    y = _grid('bn', shape, _ints(_cl(shape), g) + offset)
    y64 = _ncdhw(y)
    assert torch.equal(y64, (y64.float().to(half.dtype())).double())
    sums = conv3d_ops.bn_sums(y)
    red = [0, 2, 3, 4]
    assert float((y64 * y64).sum(red).max()) < 2.0 ** 24
    assert torch.equal(sums.double(), torch.stack([y64.sum(red), (y64 * y64).sum(red)]))
    mean, var, rstd = conv3d_ops.bn_batch_stats(sums, n, EPS)
    m64 = y64.mean(red)
    v64 = (y64 - m64.view(1, -1, 1, 1, 1)).square().mean(red)
    room = 4 * 2.0 ** -53 * ((y64 * y64).mean(red) + m64 * m64)
    assert bool(((mean - m64).abs() <= 2.0 ** -52 * m64.abs()).all())
    assert bool(((var - v64).abs() <= room).all()), ((var - v64).abs() / room).max()
    assert bool(((rstd - (v64 + EPS).rsqrt()).abs() <= 1e-12 * rstd).all())


test_bn_variance_of_channels_with_a_large_mean_fp16 = fp16_twin(
    test_bn_variance_of_channels_with_a_large_mean)


CONSTANT_ROWS = {0: 3.0, 5: 0.0, 7: -2.0}     # interior pixel / token -> its value


def _slope64(v):
    return 0.5 * (1 + torch.erf(v * 2.0 ** -0.5)) + \
        v * torch.exp(-0.5 * v * v) * (2 * torch.pi) ** -0.5


@pytest.mark.parametrize('C', [64, 1024])
def test_ln_image_passes_with_constant_rows(C, flavour):
    """Pixels 0, 5 and 7 of a (1, C, 3, 4) image hold one integer on every channel (3, 0
    and -2; pixel 5 is the all-zero row of a region ReLU emptied), the others are
    Gaussian; C is a power of two.  Without GELU the row sum of C equal small integers is
    exact in fp32: mean = x, variance 0, rstd = eps^-1/2, xhat = 0 exactly.  With GELU in
    front the same holds for the zero row; for u = GELU(3), GELU(-2) a lane adds its 8 or
    16 copies of u one by one (the butterfly then only doubles), so the mean is u within
    16 2^-24 |u| and xhat is not 0 but at most m = 16 2^-24 |u| eps^-1/2 (4.4e-4 at u = 3):
    the conditioning of LayerNorm at variance 0, not an error of the kernel.
    Forward (``image_layernorm`` to an image and to tokens, ``image_gelu_layernorm``): beta,
    rounded to half for an image and EXACTLY for fp32 tokens; with GELU and u != 0 within
    half rounding plus gamma m.  Backward, four variants: dx = rstd (a - mean(a)) GELU'(x)
    with a = dout gamma against fp64 within half rounding; dbeta and sum dx within (K + 8)
    2^-24 sum |terms| as in test_ln_passes_against_fp64, dgamma within that plus the
    constant rows' |dout| m; nothing NaN."""
    shape = (1, C, 3, 4)
    B, _, Y, X = shape
    g = _gen(shape)
    x_val = (torch.randn(_cl(shape), generator=g) * 1.5 + 0.3).reshape(Y * X, C)
    for t, value in CONSTANT_ROWS.items():
        x_val[t] = value
    x = _grid('ln_image', shape, x_val.reshape(_cl(shape)))
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    x64 = x.interior().double()
    K = x.M
    rows = sorted(CONSTANT_ROWS)
    value = torch.tensor([CONSTANT_ROWS[t] for t in rows], dtype=torch.float64, device=DEV)
    beta_h = beta.to(half.dtype()).expand(len(rows), C)

    def const(t):
        return t.reshape(Y * X, -1)[rows]

    out = conv3d_ops.image_layernorm(x, gamma, beta, EPS)
    assert halo_is_zero(out) and torch.equal(const(out.interior()), beta_h)
    tok = conv3d_ops.image_layernorm(x, gamma, beta, EPS, tokens=True)
    assert bool(torch.isfinite(tok).all())
    assert torch.equal(const(tok), beta.expand(len(rows), C))
    out_g = conv3d_ops.image_gelu_layernorm(x, gamma, beta, EPS)
    assert halo_is_zero(out_g)
    m_gelu = 16 * U * F.gelu(value).abs() * EPS ** -0.5
    room = RTOL() * beta.double().abs() + 1.01 * gamma.double() * m_gelu[:, None]
    assert bool(((const(out_g.interior()).double() - beta.double()).abs() <= room).all())
    assert torch.equal(const(out_g.interior())[1], beta_h[1])          # the zero row: exact
    for gelu, o in ((False, out), (True, out_g)):
        want, _, _ = conv3d_ops.ln_forward_ref(x64, gamma.double(), beta.double(), EPS, gelu)
        assert bool(torch.isfinite(o.rows.float()).all())
        assert _within_half_rounding(o.interior().double(), want)

    dimg = _grid('ln_image', shape, torch.randn(_cl(shape), generator=g))
    dtok = torch.randn(B, Y * X, C, generator=g).to(DEV)
    red = [0, 1, 2]
    for gelu in (False, True):
        _, xhat, _ = conv3d_ops.ln_forward_ref(x64, gamma.double(), beta.double(), EPS, gelu)
        assert float(const(xhat).abs().max()) <= 1e-10
        slope = _slope64(value) if gelu else torch.ones_like(value)
        m = m_gelu if gelu else torch.zeros_like(value)
        for dout in (dimg, dtok):
            d64 = dout.double().view(B, Y, X, C) if torch.is_tensor(dout) else \
                dout.interior().double()
            dx64, dg64, db64 = conv3d_ops.ln_gelu_backward_ref(d64, x64, gamma.double(), EPS,
                                                               gelu)
            # the closed form at variance 0
            a = const(d64 * gamma.double())
            closed = EPS ** -0.5 * (a - a.mean(-1, keepdim=True)) * slope[:, None]
            assert float((const(dx64) - closed).abs().max()) <= 1e-9 * float(closed.abs().max())
            dx, sums = conv3d_ops.image_layernorm_bwd(dout, x, gamma, EPS, gelu_in=gelu)
            assert halo_is_zero(dx) and bool(torch.isfinite(dx.rows.float()).all())
            assert bool(torch.isfinite(sums).all())
            assert _within_half_rounding(dx.interior().double(), dx64)
            assert _within_half_rounding(const(dx.interior()).double(), const(dx64))
            want = torch.stack([dg64, db64, dx64.sum(red)])
            S = torch.stack([(d64 * xhat).abs().sum(red), d64.abs().sum(red),
                             dx64.abs().sum(red)])
            bound = (K + 8) * U * S
            bound[0] += (const(d64).abs() * m[:, None]).sum(0)
            assert bool(((sums.double() - want).abs() <= bound).all()), (gelu,)


test_ln_image_passes_with_constant_rows_fp16 = fp16_twin(test_ln_image_passes_with_constant_rows)


@pytest.mark.parametrize('d', [64, 1024])
def test_ln_tokens_backward_with_constant_rows(d, flavour):
    """``layernorm_f32_bwd`` (dout fp32 and half) on 12 token rows of which rows 0, 5 and 7
    hold one integer on every channel (3, 0, -2): dx = rstd (a - mean(a)) with rstd =
    eps^-1/2 against fp64 within 1e-5 of the row's RMS, the sums within (T + 8) 2^-24 sum
    |terms| (test_row_passes_against_fp64's criteria), nothing NaN."""
    T = 12
    g = _gen((T, d))
    x = torch.randn(T, d, generator=g) * 1.5 + 0.3
    for t, value in CONSTANT_ROWS.items():
        x[t] = value
    x = x.to(DEV)
    rows = sorted(CONSTANT_ROWS)
    gamma = (torch.rand(d, generator=g) + 0.5).to(DEV)
    dtok = torch.randn(T, d, generator=g).to(DEV)
    _, xhat, _ = conv3d_ops.ln_forward_ref(x.double(), gamma.double(),
                                           torch.zeros_like(gamma).double(), EPS)
    assert float(xhat[rows].abs().max()) == 0.0
    for dout in (dtok, dtok.to(half.dtype())):
        d64 = dout.double()
        dx64, dg64, db64 = conv3d_ops.ln_gelu_backward_ref(d64, x.double(), gamma.double(), EPS)
        a = (d64 * gamma.double())[rows]
        closed = EPS ** -0.5 * (a - a.mean(-1, keepdim=True))
        assert torch.allclose(dx64[rows], closed, rtol=1e-12, atol=0)
        dx, dg, db = vit_ops.layernorm_f32_bwd(dout, x, gamma, EPS)
        for v in (dx, dg, db):
            assert bool(torch.isfinite(v).all())
        rms = dx64.pow(2).mean(-1, keepdim=True).sqrt()
        assert bool(((dx.double() - dx64).abs() <= 1e-5 * rms).all())
        for got, want, S in ((dg, dg64, (d64 * xhat).abs().sum(0)), (db, db64, d64.abs().sum(0))):
            assert bool(((got.double() - want).abs() <= (T + 8) * U * S).all())


test_ln_tokens_backward_with_constant_rows_fp16 = fp16_twin(
    test_ln_tokens_backward_with_constant_rows)


@pytest.mark.parametrize('n', [8, 8 * 257])
@pytest.mark.parametrize('quick', [False, True], ids=['gelu', 'quickgelu'])
def test_gelu_pairs_at_large_arguments(quick, n, flavour):
    """+-30, +-100 and +- the largest finite half of the flavour, repeated over n elements
    (n = 8 * 257: one chunk falls in a second workgroup): the forward is y for positive
    arguments and -+0 for negative ones, the slope (``*_bwd`` with dh = 1) is 1 or 0, and
    nothing is NaN or inf.  The one argument at which they are neither: QuickGELU(-30) =
    -30 sigma(-51) = -2.0e-21 and its slope -3.4e-21 are normal bf16 numbers (they
    underflow to -0 in fp16); every result is compared with the fp64 function, within half
    rounding where that is not 0."""
    big = float(torch.finfo(half.dtype()).max)
    args = torch.tensor([30., -30., 100., -100., big, -big, 30., -100.])
    y = args.repeat(n // 8).to(half.dtype()).to(DEV)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) == big
    y64 = y.double()
    fwd, bwd = (vit_ops.quickgelu, vit_ops.quickgelu_bwd) if quick else \
        (vit_ops.gelu, vit_ops.gelu_bwd)
    if quick:
        want = y64 * torch.sigmoid(1.702 * y64)
        slope = vit_ops.quickgelu_bwd_ref(torch.ones_like(y64), y64)
    else:
        want = F.gelu(y64)
        slope = 0.5 * (1 + torch.erf(y64 * 2.0 ** -0.5)) + \
            y64 * torch.exp(-0.5 * y64 * y64) * (2 * torch.pi) ** -0.5
    # the facts of the fp64 functions, rounded to the flavour
    want_h, slope_h = want.to(half.dtype()), slope.to(half.dtype())
    small = (y == -30) & bool(quick and half.dtype() == torch.bfloat16)
    assert bool((((want_h != 0) & (want_h != y)) == small).all())
    assert bool((((slope_h != 0) & (slope_h != 1)) == small).all())
    assert bool((slope_h[y > 0] == 1).all()) and bool((want_h[y > 0] == y[y > 0]).all())
    got = fwd(y)
    got_slope = bwd(torch.ones_like(y), y)
    for res, ref in ((got, want), (got_slope, slope)):
        assert res.dtype == half.dtype() and bool(torch.isfinite(res).all())
        zero = ref.to(half.dtype()) == 0
        assert bool((res[zero] == 0).all())
        assert bool(((res.double() - ref).abs()[~zero] <= RTOL() * ref.abs()[~zero]).all())
    assert torch.equal(got[y > 0], y[y > 0])
    assert torch.equal(got_slope[y > 0], torch.ones_like(y[y > 0]))
    dh = torch.randn(n, generator=_gen((n,))).to(half.dtype()).to(DEV)
    got_d = bwd(dh, y)
    assert bool(torch.isfinite(got_d).all())
    assert torch.equal(got_d[y > 0], dh[y > 0])
    assert bool((got_d[(y < 0) & ~small] == 0).all())


test_gelu_pairs_at_large_arguments_fp16 = fp16_twin(test_gelu_pairs_at_large_arguments)
