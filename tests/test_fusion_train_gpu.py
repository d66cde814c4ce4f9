"""Native training of the lift's 2-D fusion (csrc/fusion_train.hip) on
the MI355X: the resize into channels-last rows and its gather-form adjoint, the dual
LayerNorm forward and backward, the join / split around the ReLU, and the
``CatFusionLift.hip_train`` switch against the module's own definition.  Every test here
calls a new wrapper or asserts on a new symbol's call count, so all of them fail on a tree
without the feature.

Yardsticks (none taken from the code under test): the fp64 references of
tests/fusion_train_refs.py on the fp32 filter tables; torch's fp32 autograd of the same
sequence on the same device; the module under ``torch.autocast`` with the flavour's half.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import fusion_train_refs as refs
from tests.helpers import flavour, fp16_twin  # noqa: F401
from veon_amd import _lib, fusion_ops, half, vit_ops
from veon_amd.models.semantic_net.fusion_layers import CatFusionLift

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RESIZE, ADJOINT, DUAL, DUALBWD = ('veon_fusion_resize_cat', 'veon_fusion_resize_adjoint',
                                  'veon_fusion_dual_ln', 'veon_fusion_dual_ln_bwd')
JOIN, SPLIT = 'veon_fusion_join', 'veon_fusion_relu_split'
WGRAD, COLSUM, GEMM = 'veon_linear_wgrad_bf16', 'veon_rows_colsum_bf16', 'veon_vit_gemm'
NEW = (RESIZE, ADJOINT, DUAL, DUALBWD, JOIN, SPLIT)
EPS = 1e-6
CASES = list(range(len(refs.MAP_CASES)))
WIDTHS = list(range(len(refs.WIDTHS)))
# backward tests: every width at map case 0, every other map case at the narrowest width
BWD = [(0, w) for w in WIDTHS] + [(c, 0) for c in CASES[1:]]


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    CatFusionLift.hip_train = False


def _rel(got, want):
    want = want.double().to(got.device)
    return ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()


def _counts(fn, names=NEW):
    before = dict(_lib.CALLS)
    fn()
    return tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in names)


_INPUTS = {}


def _inputs(case, width):
    """x1, x2 (CPU fp32) of a map case and a width, and its (size, C1, C2, out, N); made
    once and shared."""
    key = (case, width)
    if key not in _INPUTS:
        s1, s2, size = refs.MAP_CASES[case]
        C1, C2, out, N = refs.WIDTHS[width]
        g = torch.Generator().manual_seed(100 * case + width)
        x1 = torch.randn(N, C1, *s1, generator=g) * 1.5 + 0.3
        x2 = torch.randn(N, C2, *s2, generator=g) * 0.7 - 0.2
        _INPUTS[key] = (x1, x2, size, C1, C2, out, N)
    return _INPUTS[key]


# ------------------------------------------------------------------ resize + cat, forward
@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('case', CASES)
def test_resize_cat_against_fp64_on_the_fp32_tables(case, width, flavour):
    """rc elementwise within 8 * 2^-24 * sum_taps w |x| of the fp64 blend on the fp32 tables
    (four products and three additions in fp32, doubled for the order), every map case and
    width; an identity map is copied to the bit.  Measured on an MI355X: the largest error
    is 3.01 x 2^-24 of that sum (the kernels do not depend on the flavour)."""
    x1, x2, size, C1, C2, _, N = _inputs(case, width)
    assert _counts(lambda: fusion_ops.resize_cat(x1.to(DEV), x2.to(DEV), size),
                   (RESIZE,)) == (2,)
    got = fusion_ops.resize_cat(x1.to(DEV), x2.to(DEV), size)
    assert got.shape == (N * size[0] * size[1], C1 + C2) and got.dtype == torch.float32
    want = refs.resize_cat(x1, x2, size)
    scale = refs.resize_cat(x1, x2, size, absolute=True)
    err = (got.cpu().double() - want).abs()
    print('resize_cat case %d width %d: largest error %.2f x 2^-24 sum w|x|' %
          (case, width, float((err / scale.clamp_min(1e-300)).max()) * 2 ** 24))
    assert bool((err <= 8 * 2.0 ** -24 * scale).all())
    if case == 1:
        assert torch.equal(got.cpu(), want.float())


test_resize_cat_against_fp64_on_the_fp32_tables_fp16 = fp16_twin(
    test_resize_cat_against_fp64_on_the_fp32_tables)


# ------------------------------------------------------------------- dual LayerNorm, forward
def _key(t):
    """A half tensor's bit patterns as integers that order like the values (+0 == -0)."""
    b = t.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7fff))


def _ln_rows(M, C, seed):
    """Gaussian rows, rows with mean 100 and standard deviation 1, one constant row.  The
    constant is 3: partial sums of small integers are exact in fp32, so the mean is exact
    and the row normalises to exactly beta, as in fp64 (a constant whose sum rounds would be
    amplified by rstd = 1000 in any fp32 LayerNorm, torch's included)."""
    g = torch.Generator().manual_seed(seed)
    rc = torch.randn(M, C, generator=g) * 1.5 + 0.3
    rc[M // 2:] = torch.randn(M - M // 2, C, generator=g) + 100.0
    rc[M - 1] = 3.0
    return rc


def _ln_params(C, C2, g):
    return ((torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g) * 0.2,
            (torch.rand(C2, generator=g) + 0.5), torch.randn(C2, generator=g) * 0.2)


def _far_from_zero_params(C, C2, g):
    """gamma in [0.5, 1], |beta| in [6, 7] with random signs: |xhat| stays below 5.5 on these
    rows, so every output has a magnitude between 0.5 and 12.5 and none is the difference of
    two nearly equal terms."""
    def beta(n):
        return (6 + torch.rand(n, generator=g)) * (1 - 2 * torch.randint(0, 2, (n,), generator=g))
    return (0.5 + 0.5 * torch.rand(C, generator=g), beta(C),
            0.5 + 0.5 * torch.rand(C2, generator=g), beta(C2))


@pytest.mark.parametrize('width', WIDTHS)
def test_dual_layernorm_within_a_half_neighbour_of_fp64(width, flavour):
    """Every element of xn1 and xn2 equals the fp64 LayerNorm of the same fp32 rows rounded
    to the flavour's half, or one of that value's two neighbours: on Gaussian rows, rows of
    mean 100 and deviation 1 (where a one-pass variance fails) and a constant row (rstd =
    eps^-1/2, finite output, exactly beta).

    That statement rests on the fp32 arithmetic error being far below half an ulp of the
    half type, which holds where the output is not the difference of two nearly equal terms
    (xhat gamma against beta): an fp32 LayerNorm of any construction has an absolute error
    of some 2^-24 of the terms, which is many half ulps of an output of 1e-6.  So the
    neighbour check runs with parameters that keep every output away from zero
    (``_far_from_zero_params``), and a second pass with ordinary parameters (gamma in
    [0.5, 1.5], beta ~ 0.2 N) adds an absolute bound of this file's own, elementwise:
        |got - want| <= ulp_half(want) / 2 + 2^-20 (|xhat gamma| + |beta|)
                        + 2^-18 |mean| rstd |gamma|
    (half rounding; 16 roundings of the terms; the fp32 mean of up to 2432 values, 32 serial
    additions per lane and 6 butterfly steps, 64 x 2^-24 relative, scaled as xhat is).

    Measured on an MI355X: no element of the first pass is further than one neighbour; one
    neighbour off are 0, 0, 2 and 11 elements of 16 896, 28 160, 168 960 and 214 016 in bf16
    (8, 7, 54 and 81 in fp16); the second pass reaches 1.00 of its bound, which the half
    rounding term alone nearly fills."""
    C1, C2 = refs.WIDTHS[width][:2]
    C, M = C1 + C2, 88
    rc = _ln_rows(M, C, seed=width)
    gen = torch.Generator().manual_seed(40 + width)
    ulp = 2.0 ** (-7 if half.name() == 'bf16' else -10)
    for far in (True, False):
        g1, b1, g2, b2 = _far_from_zero_params(C, C2, gen) if far else _ln_params(C, C2, gen)
        d = [t.to(DEV) for t in (rc, g1, b1, g2, b2)]
        assert _counts(lambda: fusion_ops.dual_layernorm(d[0], C1, d[1], d[2], EPS, d[3],
                                                         d[4], EPS), (DUAL,)) == (1,)
        xn1, xn2 = fusion_ops.dual_layernorm(d[0], C1, d[1], d[2], EPS, d[3], d[4], EPS)
        assert xn1.shape == (M, C) and xn2.shape == (M, C2) and xn1.dtype == half.dtype()
        off = worst = 0
        for got, x, g, b in ((xn1, rc, g1, b1), (xn2, rc[:, C1:], g2, b2)):
            want, xhat, rstd = refs.layernorm(x, g, b, EPS)
            assert bool(torch.isfinite(got.float()).all())
            if far:
                assert float(want.abs().min()) > 0.5
                dist = (_key(got.cpu()) - _key(want.to(half.dtype()))).abs()
                off += int((dist > 0).sum())
                worst = max(worst, int(dist.max()))
            else:
                half_ulp = 0.5 * ulp * 2.0 ** torch.floor(torch.log2(want.abs().clamp_min(
                    2.0 ** -14)))
                mean = x.double().mean(-1, keepdim=True).abs()
                bound = half_ulp + 2.0 ** -20 * ((xhat * g.double()).abs() + b.double().abs()) \
                    + 2.0 ** -18 * mean * rstd * g.double().abs()
                err = (got.cpu().double() - want).abs()
                worst = max(worst, float((err / bound).max()))
                assert bool((err <= bound).all()), float((err / bound).max())
            # the constant row: xhat = 0 exactly, so the output is beta
            assert torch.equal(got[M - 1].cpu(), b.to(half.dtype()))
        if far:
            print('dual LN %s width %d: %d of %d elements one neighbour off, none further' %
                  (half.name(), width, off, M * (C + C2)))
            assert worst <= 1, worst
        else:
            print('dual LN %s width %d: ordinary parameters, largest error %.2f of the bound'
                  % (half.name(), width, worst))


test_dual_layernorm_within_a_half_neighbour_of_fp64_fp16 = fp16_twin(
    test_dual_layernorm_within_a_half_neighbour_of_fp64)


# ------------------------------------------- dual LayerNorm backward and the resize adjoint
def _backward_operands(case, width):
    x1, x2, size, C1, C2, _, N = _inputs(case, width)
    M = N * size[0] * size[1]
    g = torch.Generator().manual_seed(7 + 10 * case + width)
    dxn1 = torch.randn(M, C1 + C2, generator=g).to(half.dtype())
    dxn2 = torch.randn(M, C2, generator=g).to(half.dtype())
    g1, _, g2, _ = _ln_params(C1 + C2, C2, g)
    return x1, x2, size, C1, C2, N, M, dxn1, dxn2, g1, g2


def _native_backward(x1, x2, size, C1, dxn1, dxn2, g1, g2, nan_fill=False):
    """The wrappers' chain from the maps: resize_cat, dual_layernorm_bwd, both adjoints."""
    d = [t.to(DEV) for t in (x1, x2, dxn1, dxn2, g1, g2)]
    rc = fusion_ops.resize_cat(d[0], d[1], size)
    outs = dict(drc=torch.empty_like(rc), dx1=torch.empty_like(d[0]),
                dx2=torch.empty_like(d[1]))
    if nan_fill:
        for t in outs.values():
            t.fill_(float('nan'))
    drc, dg1, db1, dg2, db2 = fusion_ops.dual_layernorm_bwd(d[2], d[3], rc, C1, d[4], EPS,
                                                            d[5], EPS, out=outs['drc'])
    dx1 = fusion_ops.resize_adjoint(drc, x1.shape, size, 0, out=outs['dx1'])
    dx2 = fusion_ops.resize_adjoint(drc, x2.shape, size, C1, out=outs['dx2'])
    return dict(drc=drc, dg1=dg1, db1=db1, dg2=dg2, db2=db2, dx1=dx1, dx2=dx2)


@pytest.mark.parametrize('case,width', BWD)
def test_backward_against_fp64_with_torch_fp32_as_the_yardstick(case, width, flavour):
    """Relative L2 error e of drc, the four parameter sums, dx1 and dx2 against the fp64
    closed forms on the fp32 tables; yardstick: torch's fp32 autograd of the mirror
    sequence on the same device against the same fp64 result; e(kernel) <= 4 e(torch fp32)
    (two fp32 summation orders over up to 1408 terms, and a hardware rsqrt).  Map case 2
    runs with NaN-filled outputs: every element is written, finite, and exactly zero at
    the source pixels no token reads.

    Measured on an MI355X: the largest ratio e(kernel) / e(torch fp32) of the seven is between
    0.97 and 1.23 over the seven shapes and both flavours (1.23: dbeta2 at map case 0, width
    (384, 1024), fp16); the factor 4 did not have to move.  Pairs e(kernel) / e(torch fp32):
        map case 0, (384, 768), bf16   drc 6.9e-8 / 7.5e-8   dx1 6.3e-8 / 6.6e-8   dx2 8.8e-8 / 9.9e-8
                                       dgamma1 1.03e-7 / 1.02e-7   dgamma2 1.01e-7 / 9.9e-8
                                       dbeta1 1.1e-9 / 1.1e-9      dbeta2 3.7e-9 / 3.7e-9
        map case 2, (64, 64), fp16     drc 7.0e-8 / 7.7e-8   dx1 7.5e-8 / 6.9e-8   dx2 8.9e-8 / 9.7e-8
                                       dgamma1 9.5e-8 / 9.8e-8     dgamma2 1.10e-7 / 1.33e-7
                                       dbeta1 1.06e-8 / 9.6e-9     dbeta2 6.3e-9 / 8.9e-9
    (the full lists are what the test prints)."""
    x1, x2, size, C1, C2, N, M, dxn1, dxn2, g1, g2 = _backward_operands(case, width)
    n = _counts(lambda: _native_backward(x1, x2, size, C1, dxn1, dxn2, g1, g2))
    assert n == (2, 2, 0, 1, 0, 0), n
    got = _native_backward(x1, x2, size, C1, dxn1, dxn2, g1, g2, nan_fill=case == 2)
    rc = refs.resize_cat(x1, x2, size)
    drc, dg1, db1, dg2, db2 = refs.dual_layernorm_bwd(dxn1, dxn2, rc, C1, g1, EPS, g2, EPS)
    want = dict(drc=drc, dg1=dg1, db1=db1, dg2=dg2, db2=db2,
                dx1=refs.resize_adjoint(refs.maps(drc[:, :C1], N, *size), x1.shape),
                dx2=refs.resize_adjoint(refs.maps(drc[:, C1:], N, *size), x2.shape))
    yard = refs.mirror_backward(x1, x2, size, dxn1.float(), dxn2.float(), g1, EPS, g2, EPS,
                                torch.float32, DEV)
    worst = []
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32, k
        assert bool(torch.isfinite(got[k]).all()), k
        e_k, e_t = _rel(got[k], want[k]), _rel(yard[k], want[k])
        print('bwd %s case %d width %d %-4s e(kernel) %.3e  e(torch fp32) %.3e' %
              (half.name(), case, width, k, e_k, e_t))
        worst.append((e_k / max(e_t, 1e-30), k))
    print('largest e(kernel) / e(torch fp32): %.2f at %s' % max(worst))
    if case == 2:
        un = refs.untouched(x1.shape, size)
        assert bool(un.any()) and not bool(refs.untouched(x2.shape, size).any())
        assert bool((got['dx1'].cpu()[:, :, un] == 0).all())
        assert bool((want['dx1'][:, :, un] == 0).all())
    for ratio, k in worst:
        assert ratio <= 4, (k, ratio)


test_backward_against_fp64_with_torch_fp32_as_the_yardstick_fp16 = fp16_twin(
    test_backward_against_fp64_with_torch_fp32_as_the_yardstick)


# --------------------------------------------------------------------------- rows beyond M
def _in_nan_alloc(t, extra=37):
    big = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), float('nan'),
                     dtype=t.dtype, device=t.device)
    big[:t.shape[0]] = t
    return big[:t.shape[0]]


@pytest.mark.parametrize('width', [0, 2])
def test_rows_beyond_m_are_never_read(width, flavour):
    """Operands that are the leading rows of NaN-filled allocations give results equal to
    the bit to those of exact-size copies: all six kernels."""
    x1, x2, size, C1, C2, N, M, dxn1, dxn2, g1, g2 = _backward_operands(0, width)
    out = refs.WIDTHS[width][2]
    p1, p2 = out // 4, out - out // 4
    P1, P2 = -(-p1 // 64) * 64, -(-p2 // 64) * 64
    g = torch.Generator().manual_seed(5)
    d = [t.to(DEV) for t in (x1, x2, dxn1, dxn2, g1, g2)]
    b1, b2 = torch.zeros_like(d[4]), torch.zeros_like(d[5])
    y1 = torch.randn(M, P1, generator=g).relu().to(half.dtype()).to(DEV)
    y2 = torch.randn(M, P2, generator=g).relu().to(half.dtype()).to(DEV)
    dout = torch.randn(M, p1 + p2, generator=g).to(DEV)

    def chain(w):
        rc = fusion_ops.resize_cat(w(d[0]), w(d[1]), size)
        rc = w(rc)
        xn = fusion_ops.dual_layernorm(rc, C1, d[4], b1, EPS, d[5], b2, EPS)
        bw = fusion_ops.dual_layernorm_bwd(w(d[2]), w(d[3]), rc, C1, d[4], EPS, d[5], EPS)
        drc = w(bw[0])
        return (rc,) + xn + bw + (
            fusion_ops.resize_adjoint(drc, x1.shape, size, 0),
            fusion_ops.resize_adjoint(drc, x2.shape, size, C1),
            fusion_ops.join(w(y1), w(y2), p1, p2)) + fusion_ops.relu_split(
                w(dout), w(y1), w(y2), p1, p2)
    exact, sliced = chain(lambda t: t), chain(_in_nan_alloc)
    assert len(exact) == 13
    for i, (a, b) in enumerate(zip(exact, sliced)):
        assert bool(torch.isfinite(b.float()).all()), i
        assert torch.equal(a, b), i


test_rows_beyond_m_are_never_read_fp16 = fp16_twin(test_rows_beyond_m_are_never_read)


def test_join_and_split_are_exact(flavour):
    """join widens the first p columns of both half outputs; relu_split is dout where the
    stored output is positive, rounded to half, zero elsewhere and in the padding."""
    M, p1, p2, P1, P2 = 88, 16, 48, 64, 64
    g = torch.Generator().manual_seed(9)
    y1 = (torch.randn(M, P1, generator=g).relu() + 0).to(half.dtype()).to(DEV)
    y2 = torch.randn(M, P2, generator=g).relu().to(half.dtype()).to(DEV)
    dout = torch.randn(M, p1 + p2, generator=g).to(DEV)
    assert torch.equal(fusion_ops.join(y1, y2, p1, p2),
                       torch.cat([y1[:, :p1], y2[:, :p2]], 1).float())
    dy1, dy2 = fusion_ops.relu_split(dout, y1, y2, p1, p2)
    for dy, y, p, lo in ((dy1, y1, p1, 0), (dy2, y2, p2, p1)):
        want = torch.zeros_like(y)
        want[:, :p] = (dout[:, lo:lo + p] * (y[:, :p] > 0)).to(half.dtype())
        assert torch.equal(dy, want)
        assert bool((y[:, :p] > 0).any()) and bool((y[:, :p] == 0).any())


test_join_and_split_are_exact_fp16 = fp16_twin(test_join_and_split_are_exact)


# ------------------------------------------------------------------------------ the module
def _module(C1, C2, out, seed=3):
    torch.manual_seed(seed)
    mod = CatFusionLift(C1, C2, out)
    with torch.no_grad():
        for seq in (mod.input_proj_1, mod.input_proj_2):
            seq[0].weight.uniform_(0.5, 1.5)
            seq[0].bias.normal_(0, 0.2)
            seq[1].bias.normal_(0, 0.2)
    return mod.train()


def _step(mod, x1, x2, size, G, how, x2_grad=True, freeze=()):
    """One forward + backward of a copy of ``mod`` on the device: {name: tensor} of the
    output, dx1, dx2 and the eight parameter gradients.  Only 'native' runs with the switch
    on; 'fp32' and 'autocast' are the module's torch formulation."""
    m = copy.deepcopy(mod).to(DEV)
    for k, p in m.named_parameters():
        if any(k.startswith(f) for f in freeze):
            p.requires_grad_(False)
    a = x1.to(DEV).clone().requires_grad_(True)
    b = x2.to(DEV).clone().requires_grad_(x2_grad)
    CatFusionLift.hip_train = how == 'native'
    try:
        with torch.autocast('cuda', dtype=half.dtype(), enabled=how == 'autocast'):
            out = m(a, b, size)
        out.float().backward(G.to(DEV))
    finally:
        CatFusionLift.hip_train = False
    res = {'out': out.detach().float(), 'dx1': a.grad, 'dx2': b.grad}
    res.update({'grad:' + k: p.grad for k, p in m.named_parameters()})
    return res


def _decided_relu(mod, x1, x2, size):
    """1.0 where rounding the GEMM operands to the flavour's half cannot change the ReLU's
    decision, 0.0 elsewhere; fp32 on the CPU.  A pre-activation y = sum_k xn_k w_k + b computed
    from half operands is off by at most 2 u S, S = sum_k |xn_k w_k| + |b|, u the half's unit
    roundoff (two rounded operands per product); positions with |y| <= 4 u S (twice that) are
    undecided: there the native and the autocast run each flip the mask or not by chance,
    one flip among 88 x 16 outputs moves a gradient's relative error by a percent, and the
    comparison of the two errors would be a lottery.  3 to 13 % of the positions."""
    from tests.helpers import roundoff
    m = copy.deepcopy(mod).double()
    with torch.no_grad():
        r1, r2 = refs.resize(x1, size), refs.resize(x2, size)
        parts = []
        for seq, x in ((m.input_proj_1, torch.cat([r1, r2], 1)), (m.input_proj_2, r2)):
            xn = seq[0](x)
            S = F.conv2d(xn.abs(), seq[1].weight.abs(), seq[1].bias.abs())
            parts.append(seq[1](xn).abs() > 4 * roundoff() * S)
    return torch.cat(parts, 1).float()


@pytest.mark.parametrize('width', WIDTHS)
def test_module_matches_its_torch_formulation(width, flavour):
    """CatFusionLift(C1, C2, out) in training mode at map case 0, the switch on against the
    switch off (fp32 torch, the behaviour without it): output, dx1, dx2 and the eight
    parameter gradients, the upstream gradient a fixed random fp32 tensor that is zero at
    the positions ``_decided_relu`` leaves out (the output is compared everywhere); with e
    the relative L2 distance to the fp32 run, e(native) <= 2 e(autocast), the autocast run
    wrapping the module's forward in torch.autocast with the flavour's half (the yardstick
    and factor of test_native_blocks_in_place_on_the_path).

    Measured on an MI355X; the factor 2 did not have to move.  Largest e(native) /
    e(autocast) of the eleven, and the pairs of the output and dx1:
        (64, 64, 64)      bf16 0.91   out 2.7e-3 / 3.2e-3   dx1 3.0e-3 / 4.4e-3
        (64, 128, 256)    bf16 1.00
        (384, 768, 256)   bf16 1.00   out 2.8e-3 / 3.3e-3   dx1 2.7e-3 / 2.7e-3
        (384, 1024, 256)  bf16 1.00
        (64, 64, 64)      fp16 0.80   out 3.4e-4 / 5.8e-4   dx1 3.6e-4 / 5.0e-4
        (64, 128, 256) 0.79, (384, 768, 256) 0.74, (384, 1024, 256) 0.71 in fp16
    96.5, 95.3, 88.4 and 87.0 % of the outputs carry an upstream gradient in bf16.  With a
    plain random gradient the same runs gave ratios between 0.70 and 1.20 except
    (64, 64, 64) in bf16, 6.3: one ReLU flip among its 88 x 16 first-branch outputs, which the
    autocast run happened not to have (e 1.2e-2 against 1.9e-3, both far above the
    3e-3 of the roundings being compared)."""
    x1, x2, size, C1, C2, out, N = _inputs(0, width)
    mod = _module(C1, C2, out)
    decided = _decided_relu(mod, x1, x2, size)
    print('module %s width %d: %.1f %% of the outputs carry an upstream gradient' %
          (half.name(), width, 100 * float(decided.mean())))
    assert float(decided.mean()) > 0.75
    G = torch.randn(N, out, *size, generator=torch.Generator().manual_seed(21)) * decided
    ref = _step(mod, x1, x2, size, G, 'fp32')
    before = dict(_lib.CALLS)
    nat = _step(mod, x1, x2, size, G, 'native')
    n = tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in NEW + (WGRAD,))
    assert n == (2, 2, 2, 1, 1, 1, 2), n
    auto = _step(mod, x1, x2, size, G, 'autocast')
    assert set(nat) == set(ref) == set(auto) and len(ref) == 11
    assert nat['out'].shape == ref['out'].shape
    worst = []
    for k in sorted(ref):
        assert nat[k] is not None and nat[k].shape == ref[k].shape, k
        assert nat[k].dtype == torch.float32, k
        e_n, e_a = _rel(nat[k], ref[k]), _rel(auto[k], ref[k])
        print('module %s width %d %-28s e(native) %.3e  e(autocast) %.3e' %
              (half.name(), width, k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k))
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst))
    for ratio, k in worst:
        assert ratio <= 2, (k, ratio)


test_module_matches_its_torch_formulation_fp16 = fp16_twin(
    test_module_matches_its_torch_formulation)


def test_switch_and_call_counts(flavour):
    """Per step with the switch on: 2 resize launches, 2 dual LayerNorms (forward, and once
    more in backward for the weight gradients' operand), 1 dual LayerNorm backward, 2
    adjoint launches, 1 join, 1 split, 2 weight gradients, 2 column sums, 4 GEMMs.  Switch
    off: none.  A width the kernels do not take: none, and the torch result to the bit.  An
    x2 without a gradient: one adjoint launch fewer.  Frozen convs: no weight gradient, no
    column sum, no second dual LayerNorm."""
    names = NEW + (WGRAD, COLSUM, GEMM)
    x1, x2, size, C1, C2, out, N = _inputs(0, 0)
    mod = _module(C1, C2, out)
    G = torch.randn(N, out, *size, generator=torch.Generator().manual_seed(22))
    assert CatFusionLift.hip_train is False
    assert _counts(lambda: _step(mod, x1, x2, size, G, 'fp32'), names) == (0,) * 9
    assert _counts(lambda: _step(mod, x1, x2, size, G, 'native'), names) == \
        (2, 2, 2, 1, 1, 1, 2, 2, 4)
    res = {}
    assert _counts(lambda: res.update(_step(mod, x1, x2, size, G, 'native', x2_grad=False)),
                   names) == (2, 1, 2, 1, 1, 1, 2, 2, 4)
    assert res['dx2'] is None and res['dx1'] is not None
    frozen = ('input_proj_1.1', 'input_proj_2.1')
    assert _counts(lambda: res.update(_step(mod, x1, x2, size, G, 'native', freeze=frozen)),
                   names) == (2, 2, 1, 1, 1, 1, 0, 0, 4)
    assert res['grad:input_proj_1.1.weight'] is None
    assert res['grad:input_proj_1.0.weight'] is not None
    with torch.no_grad():                      # no autograd: the torch formulation
        CatFusionLift.hip_train = True
        m = copy.deepcopy(mod).to(DEV)
        assert _counts(lambda: m(x1.to(DEV), x2.to(DEV), size), names) == (0,) * 9
        CatFusionLift.hip_train = False
    # identity maps: torch's own resize backward adds with atomics and does not repeat itself
    # to the bit, so the fallback is compared where the torch path is deterministic
    i1, i2, isize = _inputs(1, 0)[:3]
    odd = _module(60, 64, 64)
    x60 = i1[:, :60].contiguous()
    on, off = {}, {}
    assert _counts(lambda: on.update(_step(odd, x60, i2, isize, G, 'native')), names) == (0,) * 9
    off.update(_step(odd, x60, i2, isize, G, 'fp32'))
    assert len(off) == 11
    for k in off:
        assert torch.equal(on[k], off[k]), k


def test_two_identical_steps_are_bit_equal(flavour):
    x1, x2, size, C1, C2, out, N = _inputs(0, 1)
    mod = _module(C1, C2, out)
    G = torch.randn(N, out, *size, generator=torch.Generator().manual_seed(23))
    a = _step(mod, x1, x2, size, G, 'native')
    b = _step(mod, x1, x2, size, G, 'native')
    assert len(a) == 11
    for k in a:
        assert torch.equal(a[k], b[k]), k


test_two_identical_steps_are_bit_equal_fp16 = fp16_twin(test_two_identical_steps_are_bit_equal)


def test_the_wrappers_capture_into_one_graph(flavour):
    """After a warm-up, the wrappers' forward + backward sequence (the six new kernels and
    the four GEMMs between them) on one stream is captured in one torch.cuda.graph; two
    replays give the eager run's results to the bit."""
    x1, x2, size, C1, C2, out, N = _inputs(0, 1)
    p1, p2 = out // 4, out - out // 4
    g = torch.Generator().manual_seed(31)
    M = N * size[0] * size[1]
    g1, b1, g2, b2 = (t.to(DEV) for t in _ln_params(C1 + C2, C2, g))
    w1 = (torch.randn(p1, C1 + C2, generator=g) * 0.05).to(half.dtype()).to(DEV)
    w2 = (torch.randn(p2, C2, generator=g) * 0.05).to(half.dtype()).to(DEV)
    w1t, w2t = w1.t().contiguous(), w2.t().contiguous()
    c1, c2 = torch.randn(p1, generator=g).to(DEV), torch.randn(p2, generator=g).to(DEV)
    dout = torch.randn(M, out, generator=g).to(DEV)
    a, b = x1.to(DEV), x2.to(DEV)

    def sequence():
        rc = fusion_ops.resize_cat(a, b, size)
        xn1, xn2 = fusion_ops.dual_layernorm(rc, C1, g1, b1, EPS, g2, b2, EPS)
        y1 = vit_ops.linear(xn1, w1, c1, vit_ops.EPI_AFFINE_RELU)
        y2 = vit_ops.linear(xn2, w2, c2, vit_ops.EPI_AFFINE_RELU)
        o = fusion_ops.join(y1, y2, p1, p2)
        dy1, dy2 = fusion_ops.relu_split(dout, y1, y2, p1, p2)
        bw = fusion_ops.dual_layernorm_bwd(vit_ops.linear(dy1, w1t), vit_ops.linear(dy2, w2t),
                                           rc, C1, g1, EPS, g2, EPS)
        return (o,) + bw + (fusion_ops.resize_adjoint(bw[0], a.shape, size, 0),
                            fusion_ops.resize_adjoint(bw[0], b.shape, size, C1))
    eager = [t.clone() for t in sequence()]            # the warm-up: tables, workspaces
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    before = dict(_lib.CALLS)
    with torch.cuda.graph(graph):
        static = sequence()
    assert tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in NEW) == (2, 2, 1, 1, 1, 1)
    for _ in range(2):
        for t in static:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert len(static) == len(eager) == 8
        for i, (s, e) in enumerate(zip(static, eager)):
            assert torch.equal(s, e), i


test_the_wrappers_capture_into_one_graph_fp16 = fp16_twin(
    test_the_wrappers_capture_into_one_graph)


# -------------------------------------------------------------------- in place on the path
def test_native_fusion_in_place_on_the_path(monkeypatch):
    """The tiny path of tests/test_path_golden.py (the set-up of
    tests/test_body_train_gpu.py::test_native_blocks_in_place_on_the_path) with the HSA
    network in training mode, ``fuse_ds_grad`` on the neck and ``CatFusionLift.hip_train``
    on: the layer's channels-last fp32 output reaches the pool as its feature rows without
    a copy (same ``data_ptr``, contiguous after the lift's permute, and
    ``prepare_feat_for_lifting``'s view works on it); the eight parameters of the fusion
    layer and every HSA parameter that receives a gradient get a finite non-zero one; and
    with e the relative L2 distance to the same step with the switch off (torch fp32),
    e(native) <= 2 e(autocast), autocast wrapping only the fusion layer.

    Measured on an MI355X (bf16): 62 parameters are compared; e(native) between 8.9e-3 and
    1.9e-2 on the eight of the fusion layer, e(autocast) between 1.2e-2 and 2.3e-2; the
    largest ratio is 1.44 (hsa.hsa_net_body.0.ff.conv1.bias).  The factor 2 did not have to
    move."""
    from tests.conftest import load_golden
    from tests.test_align_loss_gpu import _fixture
    from tests.test_path_golden import _build, _inputs as _path_inputs
    from veon_amd.models.semantic_net import occ_loss as occ_loss_mod
    from veon_amd.ops.bev_pool_v2 import bev_pool as bp
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=False)
    images, geom, metric = _path_inputs(g, DEV)
    gen = torch.Generator().manual_seed(50)
    C = net.ov_classifier_weight.shape[1]
    net.ov_classifier_weight = torch.nn.Parameter(torch.randn(25, C, generator=gen).to(DEV))
    _, inp = _fixture(torch.float32, DEV)
    B = images.shape[0]
    assert tuple(net.occ_size) == inp['occ_size']
    loss = occ_loss_mod.OccLossFB(grid_config=inp['grid_config'], high_conf_thr=0.3,
                                  stage2_start=2, priority=inp['priority'], ov_class_number=8)
    loss.epoch = 3
    args = (inp['voxel_semantics'][:B], inp['mask_camera'][:B],
            [t[:B] for t in inp['img_inputs']], inp['sem_seg_ds'][:B],
            inp['class_reflection'], loss)
    net.hsa.train()
    net.view_transformer.fuse_ds_grad = True
    dec = net.occ_decoder
    layer = dec.fusion_layers['layer_0']
    assert isinstance(layer, CatFusionLift)
    params = {'fusion2d.' + k: p for k, p in layer.named_parameters()}
    params.update({'hsa.' + k: p for k, p in net.hsa.named_parameters()})
    seen = {}

    def hook(mod, inputs, output):
        seen['out'] = output
    handle = layer.register_forward_hook(hook)
    pool = bp.bev_pool_v2_maxpool

    def spy(depth, feat, *a, **kw):
        seen['feat'] = feat
        return pool(depth, feat, *a, **kw)
    monkeypatch.setattr(bp, 'bev_pool_v2_maxpool', spy)

    def run(how):
        if how == 'autocast':
            def forward(*a, **kw):
                with torch.autocast('cuda', dtype=half.dtype()):
                    return CatFusionLift.forward(layer, *a, **kw).float()
            layer.forward = forward
        CatFusionLift.hip_train = how == 'native'
        net.zero_grad(set_to_none=True)
        before = dict(_lib.CALLS)
        try:
            with torch.enable_grad():
                out = net(images, geom, depth=metric, return_features=True)
                sum(net.occ_loss(out, *args).values()).backward()
        finally:
            CatFusionLift.hip_train = False
            layer.__dict__.pop('forward', None)
        return ({k: None if p.grad is None else p.grad.clone() for k, p in params.items()},
                tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in NEW + (WGRAD,)))

    ref, n_ref = run('fp32')
    nat, n_nat = run('native')
    out, feat = seen['out'], seen['feat']
    auto, n_auto = run('autocast')
    handle.remove()
    assert n_ref[:6] == (0,) * 6 and n_auto[:6] == (0,) * 6
    assert n_nat[:6] == (2, 2, 2, 1, 1, 1) and n_nat[6] - n_ref[6] == 2, (n_nat, n_ref)
    # no copy between the layer and the pool
    assert out.dtype == torch.float32 and out.permute(0, 2, 3, 1).is_contiguous()
    lifted = dec.prepare_feat_for_lifting(out).permute(0, 1, 3, 4, 2)
    assert lifted.is_contiguous() and lifted.data_ptr() == out.data_ptr()
    assert feat.is_contiguous() and feat.data_ptr() == out.data_ptr()
    assert feat.shape == lifted.shape
    ratios = []
    checked = 0
    for k in params:
        assert (nat[k] is None) == (ref[k] is None), k
        if ref[k] is None or (k.startswith('hsa.') and float(ref[k].abs().max()) == 0):
            continue
        checked += 1
        assert torch.isfinite(nat[k]).all() and nat[k].abs().max() > 0, k
        e_n, e_a = _rel(nat[k], ref[k]), _rel(auto[k], ref[k])
        print('path %-44s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        ratios.append((e_n / max(e_a, 1e-30), k))
    print('largest e(native) / e(autocast): %.2f at %s (%d parameters)' %
          (max(ratios) + (checked,)))
    assert checked > 8
    for ratio, k in ratios:
        assert ratio <= 2, (k, ratio)
