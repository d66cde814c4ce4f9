"""The shared weight-gradient body (csrc/wgrad_kernel.h: ``linear_wgrad``,
``conv2d_k3_wgrad``, ``conv3d_k3_wgrad``; DESIGN sections 4k - 4m) on the MI355X at its
seams, shape by shape (tests/wgrad_seams.py; the CPU file asserts what makes each row a
seam): the 64-row slab and the zeroed tail of the linear case, the first split, uneven and
recomputed splits, more tiles than CUs, and the tile decomposition with nco != nci.

Yardsticks (none of them taken from the code under test):
 * fp64 results computed from the SAME half operands, with the hard bound of fp32 addition
   of exact products, rows 2^-24 sum |terms|, elementwise;
 * rocBLAS's fp32 product of the same rows, relative L2, with the factor 8 of the other
   weight-gradient tests;
 * integer operands, on which every summation order is exact: equality with fp64.
"""
import pytest
import torch

from tests import wgrad_seams as ws
from tests.helpers import flavour, fp16_twin  # noqa: F401
from veon_amd import conv3d_ops, half, vit_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_PACK = {'conv2d': conv3d_ops.pack_image, 'conv3d': conv3d_ops.pack}
_WGRAD = {'conv2d': conv3d_ops.conv2d_k3_wgrad, 'conv3d': conv3d_ops.conv3d_k3_wgrad}


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _draw(size, g, how, rectify=False):
    if how == 'integers':          # in [-4, 4], none zero
        return (torch.randint(1, 5, size, generator=g) *
                (2 * torch.randint(0, 2, size, generator=g) - 1)).float()
    t = torch.randn(size, generator=g)
    return t.relu() if rectify else t


def _operands(kind, shape, how):
    """(dy, x) as the wrapper of ``kind`` takes them.  'gauss': dy Gaussian, x a rectified
    Gaussian, as in the other weight-gradient tests; 'integers': both in [-4, 4] without a
    zero.  Convolutions: on EVERY interior voxel / pixel, so non-zero rows lie next to
    every face of the grid and a wrong tap offset cannot hide in zeros."""
    g = torch.Generator().manual_seed(sum(shape) + len(shape))
    if kind == 'linear':
        M, K, N = shape
        return (_draw((M, N), g, how).to(half.dtype()).to(DEV),
                _draw((M, K), g, how, True).to(half.dtype()).to(DEV))
    B, Cin, Cout, *spatial = shape
    dy = _draw((B, Cout, *spatial), g, how).to(half.dtype()).float().to(DEV)
    x = _draw((B, Cin, *spatial), g, how, True).to(half.dtype()).float().to(DEV)
    return _PACK[kind](dy), _PACK[kind](x)


def _call(kind, dy, x, out=None):
    return vit_ops.linear_wgrad(dy, x, out) if kind == 'linear' else _WGRAD[kind](dy, x, out)


def _tap_rows(kind, shape, dy, x):
    """[(index of the tap in dW[Cout][taps..][Cin], rows of dy, rows of x shifted by the
    tap's offset)]: the padded rows themselves, guard rows where row + off leaves the grid."""
    if kind == 'linear':
        return [((), dy, x)]
    spatial = shape[3:]
    Xp = spatial[-1] + 2
    Yp = spatial[-2] + 2
    taps = []
    for kz in range(3) if kind == 'conv3d' else (1,):
        for ky in range(3):
            for kx in range(3):
                off = ((kz - 1) * Yp + (ky - 1)) * Xp + (kx - 1)
                idx = (kz, ky, kx) if kind == 'conv3d' else (ky, kx)
                taps.append((idx, dy.rows, x.storage[x.guard + off:x.guard + off + x.M]))
    return taps


def _references(kind, shape, dy, x, blas=True):
    """fp64 dW, S = |dy|^T |x_shifted| (fp64) and rocBLAS's fp32 product."""
    M, Cin, Cout = ws.dims(kind, shape)
    full = (Cout,) + (3,) * {'linear': 0, 'conv2d': 2, 'conv3d': 3}[kind] + (Cin,)
    want = torch.empty(full, dtype=torch.float64, device=DEV)
    S = torch.empty_like(want)
    b32 = torch.empty(full, dtype=torch.float32, device=DEV) if blas else None
    for idx, d, xs in _tap_rows(kind, shape, dy, x):
        at = (slice(None),) + idx
        want[at] = d.double().t() @ xs.double()
        S[at] = d.double().abs().t() @ xs.double().abs()
        if blas:
            b32[at] = d.float().t() @ xs.float()
    return want, S, b32


@pytest.mark.parametrize('kind,shape', ws.SHAPES, ids=ws.IDS)
def test_seams_against_fp64(kind, shape, flavour):
    """|got - fp64| <= rows 2^-24 S elementwise (fp32 addition of exact products; rows = the
    M rows of the contraction, padded rows for the convolutions), and relative L2 error at
    most 8 x that of rocBLAS's fp32 product of the same rows (exactly 0 where rocBLAS's is).
    Measured on an MI355X, relative L2 kernel / rocBLAS fp32 (the kernel is below rocBLAS at
    every shape; M = 1 is a single exact product; the largest share of the elementwise
    bound is 0.078):
                shape                      bf16                 fp16
        linear  (1, 64, 64)                0.0e+00 / 0.0e+00    0.0e+00 / 0.0e+00
        linear  (63, 64, 64)               3.1e-08 / 3.4e-08    5.4e-08 / 8.9e-08
        linear  (64, 64, 64)               3.4e-08 / 3.9e-08    5.8e-08 / 9.6e-08
        linear  (65, 64, 64)               3.1e-08 / 3.6e-08    5.7e-08 / 8.9e-08
        linear  (960, 64, 64)              1.4e-07 / 1.6e-07    2.0e-07 / 3.8e-07
        linear  (961, 64, 64)              9.7e-08 / 1.5e-07    1.4e-07 / 3.9e-07
        linear  (1024, 64, 64)             1.0e-07 / 1.6e-07    1.5e-07 / 4.0e-07
        linear  (1025, 128, 256)           9.9e-08 / 1.6e-07    1.5e-07 / 3.9e-07
        linear  (1537, 64, 192)            1.0e-07 / 2.1e-07    1.5e-07 / 4.8e-07
        linear  (5760, 64, 64)             1.1e-07 / 5.0e-07    1.6e-07 / 9.5e-07
        linear  (70, 384, 320)             3.4e-08 / 3.7e-08    6.2e-08 / 9.6e-08
        conv2d  (2, 128, 256, 7, 5)        3.0e-08 / 3.2e-08    6.7e-08 / 8.5e-08
        conv2d  (1, 64, 192, 29, 31)       9.1e-08 / 1.4e-07    1.4e-07 / 3.6e-07
        conv2d  (1, 64, 64, 30, 30)        9.2e-08 / 1.5e-07    1.4e-07 / 3.7e-07
        conv2d  (1, 384, 320, 3, 5)        1.0e-08 / 1.0e-08    3.4e-08 / 3.8e-08
        conv3d  (2, 128, 256, 3, 7, 5)     5.0e-08 / 5.3e-08    1.0e-07 / 1.4e-07
        conv3d  (1, 192, 192, 2, 14, 30)   8.4e-08 / 1.2e-07    1.3e-07 / 3.0e-07
        conv3d  (1, 64, 64, 2, 14, 30)     8.6e-08 / 1.2e-07    1.4e-07 / 3.0e-07
        conv3d  (1, 384, 320, 1, 3, 5)     9.7e-09 / 1.0e-08    3.3e-08 / 3.8e-08"""
    dy, x = _operands(kind, shape, 'gauss')
    M, Cin, Cout = ws.dims(kind, shape)
    got = _call(kind, dy, x)
    want, S, blas = _references(kind, shape, dy, x)
    assert got.shape == want.shape and got.dtype == torch.float32
    e_k, e_b = _rel(got, want), _rel(blas, want)
    worst = float(((got.double() - want).abs() / (M * 2.0 ** -24 * S).clamp_min(1e-300)).max())
    print('wgrad seam %s %s %s: rel L2 kernel %.3e, rocBLAS fp32 %.3e; largest share of '
          'rows 2^-24 S %.3f' % (half.name(), kind, shape, e_k, e_b, worst))
    assert float(want.abs().max()) > 0
    assert bool(((got.double() - want).abs() <= M * 2.0 ** -24 * S).all())
    assert e_k <= 8 * e_b, (e_k, e_b)


test_seams_against_fp64_fp16 = fp16_twin(test_seams_against_fp64)


@pytest.mark.parametrize('kind,shape', ws.SHAPES, ids=ws.IDS)
def test_seams_on_integers_are_exact(kind, shape, flavour):
    """Operands are integers in [-4, 4], none zero: every product and every partial sum is
    an integer below 2^24 (16 rows < 2^24), so fp32 addition is exact in any order and the
    result EQUALS the fp64 one in both flavours.  A dropped, doubled or misplaced row, tap
    or tile shows outright."""
    dy, x = _operands(kind, shape, 'integers')
    got = _call(kind, dy, x)
    want, S, _ = _references(kind, shape, dy, x, blas=False)
    assert float(S.max()) < 2.0 ** 24 and float(want.abs().max()) > 0
    bad = int((got.double() != want).sum())
    assert bad == 0, '%d of %d entries differ' % (bad, want.numel())


test_seams_on_integers_are_exact_fp16 = fp16_twin(test_seams_on_integers_are_exact)


def _cached_workspace(kind, shape):
    """The wrapper's cached split-K workspace of this shape (created when absent)."""
    M, Cin, Cout = ws.dims(kind, shape)
    if kind == 'linear':
        nbytes = vit_ops.linear_wgrad_workspace_bytes(*shape)
        return conv3d_ops._workspace('linear_wgrad', nbytes, torch.device(DEV), *shape)
    B, _, _, *spatial = shape
    name, entry = {'conv3d': ('wgrad', conv3d_ops.wgrad_workspace_bytes),
                   'conv2d': ('wgrad2d', conv3d_ops.wgrad2d_workspace_bytes)}[kind]
    nbytes = entry(B, *spatial, Cin, Cout)
    return conv3d_ops._workspace(name, nbytes, torch.device(DEV), B, *spatial, Cin, Cout)


@pytest.mark.parametrize('kind,shape', ws.SHAPES, ids=ws.IDS)
def test_seams_leave_nothing_stale(kind, shape, flavour):
    """The cached split-K workspace and ``out`` are NaN before the call: the result is
    finite (every slab entry and every output is written before it is read) and bit-equal
    to a second call."""
    dy, x = _operands(kind, shape, 'gauss')
    first = _call(kind, dy, x)               # makes the wrapper cache its workspace
    known = len(conv3d_ops._WORKSPACES)
    cached = _cached_workspace(kind, shape)
    assert len(conv3d_ops._WORKSPACES) == known          # the wrapper's own entry, not a new one
    p = ws.plan_of(kind, shape)
    assert cached.numel() == p['split'] * first.numel()
    cached.fill_(float('nan'))
    out = torch.full_like(first, float('nan'))
    got = _call(kind, dy, x, out)
    assert got is out or got.data_ptr() == out.data_ptr()
    assert _cached_workspace(kind, shape) is cached      # the call used the filled tensor
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, first) and torch.equal(_call(kind, dy, x), first)


test_seams_leave_nothing_stale_fp16 = fp16_twin(test_seams_leave_nothing_stale)


@pytest.mark.parametrize('M', [1, 65, 961])
def test_linear_rows_beyond_m_contribute_nothing(M, flavour):
    """The operands are the leading M rows of larger allocations whose remaining rows are
    NaN: finite and bit-equal to exact-size copies, at one live row in the only slab, in
    the second slab, and in the last slab of the second split."""
    dy, x = _operands('linear', (M, 64, 64), 'gauss')
    big_dy = torch.full((M + 200, 64), float('nan'), dtype=half.dtype(), device=DEV)
    big_x = torch.full((M + 200, 64), float('nan'), dtype=half.dtype(), device=DEV)
    big_dy[:M] = dy
    big_x[:M] = x
    got = vit_ops.linear_wgrad(big_dy[:M], big_x[:M])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, vit_ops.linear_wgrad(dy, x))


test_linear_rows_beyond_m_contribute_nothing_fp16 = fp16_twin(
    test_linear_rows_beyond_m_contribute_nothing)
