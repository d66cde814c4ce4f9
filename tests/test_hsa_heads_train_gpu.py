"""Native training of the HSA heads and token LayerNorms (csrc/linear_train.hip, DESIGN
section 4m) on the MI355X: the MFMA linear weight gradient, the column sum, the GELU pair,
the fp32 LayerNorm backward, and the three ``hip_train`` switches against the modules' own
definitions.  Every test here calls the new wrappers or asserts on their call counts, so
all of them fail on a tree without the feature.

Yardsticks (none of them taken from the code under test), those of
tests/test_hsa_train_gpu.py:
 * fp64 results computed from the SAME half-rounded operands;
 * hard bounds from fp32 addition: products of two half values are exact in fp32, so a
   K-term sum errs by at most K * 2^-24 * sum |terms|;
 * rocBLAS's fp32 product of the same operands (wgrad), torch under ``torch.autocast``
   with the flavour's half dtype (heads / blocks / path): measured errors of parent-commit
   code against the same exact result, with a stated factor on top.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import flavour, fp16_twin, half_tol, to_half  # noqa: F401
from veon_amd import _lib, conv3d_ops, half, vit_ops
from veon_amd.models.semantic_net.hsa_network import (AttnManipulateBlock, ConvBlock,
                                                      FeedForward, HighresSideAdaptorBlock)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WGRAD, COLSUM, LNBWD = 'veon_linear_wgrad_bf16', 'veon_rows_colsum_bf16', 'veon_layernorm_f32_bwd'
GELU, GELUBWD, GEMM = 'veon_gelu_bf16', 'veon_gelu_bwd_bf16', 'veon_vit_gemm'
NEW = (WGRAD, COLSUM, LNBWD, GELU, GELUBWD)
# (M, K, N): two slabs with a partial last one; mixed widths (narrow tile); wide tile with
# two splits and a partial last slab
SMALL = [(120, 64, 64), (70, 64, 128), (70, 128, 64), (1100, 128, 128)]
VEON = [(67584, 384, 384), (4224, 384, 2304)]


def _all_switches(value):
    ConvBlock.hip_train = value
    FeedForward.hip_train = value
    HighresSideAdaptorBlock.hip_train = value
    AttnManipulateBlock.hip_train = value


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _all_switches(False)


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _counts(fn, names=NEW):
    before = dict(_lib.CALLS)
    fn()
    return tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in names)


def _operands(M, K, N, seed):
    """dy: Gaussian; x: rectified Gaussian (an activation); both in the flavour's half."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(M, N, generator=g).to(half.dtype()).to(DEV)
    x = torch.randn(M, K, generator=g).relu().to(half.dtype()).to(DEV)
    return dy, x


# -------------------------------------------------------------- linear weight gradient
@pytest.mark.parametrize('M,K,N', SMALL + VEON)
def test_linear_wgrad_against_fp64(M, K, N, flavour):
    """(a) small shapes: |got - want| <= M 2^-24 S elementwise, S = |dy|^T |x| in fp64
    (fp32 addition of exact products).  (b) every shape: relative L2 error against fp64 at
    most 8 x that of rocBLAS's fp32 product of the same rows (two fp32 summation orders of
    identical exact products; the factor of the 2-D and 3-D tests).  Measured on an MI355X,
    relative L2 kernel / rocBLAS fp32 (the factor 8 did not have to move; the kernel is
    below rocBLAS at every shape):
        shape (M, K, N)            bf16                   fp16
        (120, 64, 64)              4.5e-8 / 5.1e-8        7.7e-8 / 1.3e-7
        (70, 64, 128)              3.5e-8 / 3.9e-8        6.3e-8 / 9.9e-8
        (70, 128, 64)              3.4e-8 / 3.6e-8        6.2e-8 / 9.8e-8
        (1100, 128, 128)           1.0e-7 / 1.7e-7        1.6e-7 / 4.0e-7
        (67584, 384, 384)          2.6e-7 / 1.1e-6        3.3e-7 / 1.8e-6
        (4224, 384, 2304)          1.5e-7 / 4.0e-7        2.1e-7 / 8.2e-7"""
    dy, x = _operands(M, K, N, seed=M + 3 * K + N)
    if (M, K, N) == SMALL[3]:
        # what this shape is here for: >= 2 splits, and a partial last slab
        assert vit_ops.linear_wgrad_workspace_bytes(M, K, N) >= 2 * N * K * 4
        assert M % 64 != 0
    assert _counts(lambda: vit_ops.linear_wgrad(dy, x), (WGRAD,)) == (1,)
    got = vit_ops.linear_wgrad(dy, x)
    assert got.shape == (N, K) and got.dtype == torch.float32
    want = vit_ops.linear_wgrad_ref(dy.double(), x.double())
    blas = vit_ops.linear_wgrad_ref(dy.float(), x.float())
    e_k, e_b = _rel(got, want), _rel(blas, want)
    print('linear wgrad %s %s: rel L2 kernel %.3e, rocBLAS fp32 %.3e' %
          (half.name(), (M, K, N), e_k, e_b))
    if (M, K, N) in SMALL:
        S = vit_ops.linear_wgrad_ref(dy.double().abs(), x.double().abs())
        assert bool(((got.double() - want).abs() <= M * 2.0 ** -24 * S).all())
    assert e_k <= 8 * e_b, (e_k, e_b)


test_linear_wgrad_against_fp64_fp16 = fp16_twin(test_linear_wgrad_against_fp64)


@pytest.mark.parametrize('M,K,N', [(70, 64, 128), (1100, 128, 128)])
def test_linear_wgrad_rows_beyond_m_contribute_nothing(M, K, N, flavour):
    """The operands are the leading M rows of larger allocations whose remaining rows are
    NaN: the result is finite and equal to the bit to that of exact-size copies (a tail
    that is summed, or a bound off by a row, would show; nothing out of bounds is read)."""
    dy, x = _operands(M, K, N, seed=11)
    big_dy = torch.full((M + 200, N), float('nan'), dtype=half.dtype(), device=DEV)
    big_x = torch.full((M + 200, K), float('nan'), dtype=half.dtype(), device=DEV)
    big_dy[:M] = dy
    big_x[:M] = x
    got = vit_ops.linear_wgrad(big_dy[:M], big_x[:M])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, vit_ops.linear_wgrad(dy, x))


test_linear_wgrad_rows_beyond_m_contribute_nothing_fp16 = fp16_twin(
    test_linear_wgrad_rows_beyond_m_contribute_nothing)


def test_linear_wgrad_and_colsum_are_bit_reproducible_at_the_large_shape():
    dy, x = _operands(*VEON[0], seed=2)
    assert torch.equal(vit_ops.linear_wgrad(dy, x), vit_ops.linear_wgrad(dy, x))
    assert torch.equal(vit_ops.colsum(dy), vit_ops.colsum(dy))


# ------------------------------------------------------------------------- row passes
def _within_half_rounding(got, want):
    rms = want.pow(2).mean().sqrt().item()
    tol = half_tol(2.0 ** -8, 2e-3)
    return bool(((got - want).abs() <= want.abs() * tol['rtol'] + tol['atol'] * rms).all())


# 384: 48 lanes of a wave hold the row, not a power of two; 576 and 1024: the
# two-chunks-per-lane kernel, with 8 and with all 64 lanes holding a second chunk
@pytest.mark.parametrize('T,d', [(240, 64), (70, 128), (45, 384), (16896, 384), (13, 576),
                                 (11, 1024)])
def test_row_passes_against_fp64(T, d, flavour):
    """colsum, gelu, gelu_bwd and layernorm_f32_bwd (dout as fp32 and as half) against the
    fp64 closed forms on the same inputs.  Elementwise half results within half rounding;
    dx (fp32) within 1e-5 of the row's RMS; sums within (T + 8) 2^-24 sum |terms| (T terms,
    and 8 for the fp32-rounded xhat factor of a term; the + 8 did not have to move).
    Measured on an MI355X: the largest error of any sum is 2.45 x 2^-24 sum |terms| (at
    (13, 576), bound 21; 2.44 at (11, 1024), bound 19; 1.33 at (45, 384), bound 53; 0.08 at
    (16 896, 384), bound 16 904), the largest dx error 1.2e-6 of the row's RMS, in both
    flavours."""
    g = torch.Generator().manual_seed(T + d)
    y = (torch.randn(T, d, generator=g) * 1.5 + 0.3).to(half.dtype()).to(DEV)
    dh = torch.randn(T, d, generator=g).to(half.dtype()).to(DEV)
    y64, dh64 = y.double(), dh.double()
    bound = (T + 8) * 2.0 ** -24

    assert _within_half_rounding(vit_ops.gelu(y).double(), F.gelu(y64))
    slope = 0.5 * (1 + torch.erf(y64 * 2.0 ** -0.5)) + \
        y64 * torch.exp(-0.5 * y64 * y64) * (2 * torch.pi) ** -0.5
    assert _within_half_rounding(vit_ops.gelu_bwd(dh, y).double(), dh64 * slope)

    got = vit_ops.colsum(dh)
    assert got.shape == (d,) and got.dtype == torch.float32
    err = (got.double() - dh64.sum(0)).abs()
    worst = float((err / dh64.abs().sum(0)).max()) * 2.0 ** 24
    assert bool((err <= bound * dh64.abs().sum(0)).all())

    x = (torch.randn(T, d, generator=g) * 1.5 + 0.3).to(DEV)
    gamma = (torch.rand(d, generator=g) + 0.5).to(DEV)
    dtok = torch.randn(T, d, generator=g).to(DEV)
    _, xhat, _ = conv3d_ops.ln_forward_ref(x.double(), gamma.double(),
                                           torch.zeros_like(gamma).double(), 1e-5)
    worst_dx = 0.0
    for dout in (dtok, dh):
        d64 = dout.double()
        dx64, dg64, db64 = conv3d_ops.ln_gelu_backward_ref(d64, x.double(), gamma.double(), 1e-5)
        dx, dg, db = vit_ops.layernorm_f32_bwd(dout, x, gamma, 1e-5)
        assert dx.dtype == torch.float32 and dx.shape == x.shape
        rms = dx64.pow(2).mean(-1, keepdim=True).sqrt()
        worst_dx = max(worst_dx, float(((dx.double() - dx64).abs() / rms).max()))
        assert bool(((dx.double() - dx64).abs() <= 1e-5 * rms).all())
        for got, want, S in ((dg, dg64, (d64 * xhat).abs().sum(0)), (db, db64, d64.abs().sum(0))):
            err = (got.double() - want).abs()
            worst = max(worst, float((err / S).max()) * 2.0 ** 24)
            assert bool((err <= bound * S).all())
    print('row passes %s %s: largest sum error %.2f x 2^-24 sum|terms| (bound %d), '
          'largest dx error %.2e of the row RMS' % (half.name(), (T, d), worst, T + 8, worst_dx))


test_row_passes_against_fp64_fp16 = fp16_twin(test_row_passes_against_fp64)


# ----------------------------------------------------- FeedForward against the module
def _head(dim, hidden, out, seed=3):
    torch.manual_seed(seed)
    ff = FeedForward(dim, hidden, out)
    with torch.no_grad():
        ff.net[0].weight.uniform_(0.5, 1.5)
        ff.net[0].bias.normal_(0, 0.2)
        for fc in (ff.net[1], ff.net[3]):
            fc.weight.copy_(to_half(fc.weight))
    return ff.train()


def _ff_step(ff, x, G, how, resized=None):
    """One forward + backward of a copy of ``ff`` (``resized``: (side, new) ->
    forward_resized): {name: tensor} of the output, the input gradient and the six
    parameter gradients.  Only 'native' runs with the switch on: every other run is the
    module's own (for forward_resized: un-reordered) definition."""
    ff = copy.deepcopy(ff)
    FeedForward.hip_train = how == 'native'
    if how == 'fp64':
        ff, x, G = ff.double().cpu(), x.double().cpu(), G.double().cpu()
    else:
        ff = ff.to(DEV)
    x = x.clone().requires_grad_(True)

    def call():
        return ff(x) if resized is None else ff.forward_resized(x, *resized)
    try:
        if how == 'autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                out = call()
        else:
            out = call()
        out.backward(G.to(out.dtype))
    finally:
        FeedForward.hip_train = False
    result = {'out': out.detach(), 'dx': x.grad}
    result.update({'grad:' + k: p.grad for k, p in ff.named_parameters()})
    return result


def _compare_ff_with_autocast(ff, x, G, exact_how, resized=None):
    """e = relative L2 error against the exact run; e(native) <= 2 e(autocast) for the
    output, dx and the six parameter gradients (both round the same operands to the same
    format and accumulate in fp32).

    Measured on an MI355X; the factor 2 did not have to move.  Largest
    e(native) / e(autocast) over the eight quantities, and the pairs e(native) / e(autocast)
    of the output and the input gradient:
        FeedForward(64, 64, 128)     bf16  1.00 (dx)               out 3.5e-3 / 3.5e-3  dx 3.6e-3 / 3.6e-3
        FeedForward(128, 128, 64)    bf16  1.00 (dx)               out 3.6e-3 / 3.6e-3  dx 3.5e-3 / 3.5e-3
        FeedForward(64, 64, 128)     fp16  1.00 (dx)               out 4.2e-4 / 4.2e-4  dx 4.3e-4 / 4.3e-4
        FeedForward(128, 128, 64)    fp16  1.00 (dx)               out 4.2e-4 / 4.3e-4  dx 4.4e-4 / 4.4e-4
        FeedForward(384, 384, 2304)  bf16  1.03 (grad net.0.bias)  out 3.6e-3 / 3.6e-3  dx 3.5e-3 / 3.5e-3
        FeedForward(384, 384, 2304)  fp16  1.01 (grad net.0.weight) out 4.4e-4 / 4.4e-4 dx 4.4e-4 / 4.4e-4
        forward_resized (64, 64, 128) bf16 1.17 (out)              out 3.4e-3 / 2.9e-3  dx 3.5e-3 / 3.5e-3
        forward_resized (64, 64, 128) fp16 1.23 (out)              out 4.0e-4 / 3.2e-4  dx 4.5e-4 / 4.5e-4
    (the full lists are what the test prints; the re-ordered forward_resized rounds the
    hidden map once more after the resize)."""
    exact = _ff_step(ff, x, G, exact_how, resized)
    before = dict(_lib.CALLS)
    nat = _ff_step(ff, x, G, 'native', resized)
    assert tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in NEW) == (2, 2, 1, 1, 1)
    auto = _ff_step(ff, x, G, 'autocast', resized)
    assert set(nat) == set(exact) == set(auto) and len(nat) == 8
    worst = []
    for k in sorted(exact):
        want = exact[k].to(DEV)
        assert nat[k] is not None and nat[k].shape == want.shape, k
        assert nat[k].dtype == torch.float32, k
        e_n, e_a = _rel(nat[k].to(DEV), want), _rel(auto[k].to(DEV), want)
        print('%-22s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k, e_n, e_a))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst)[:2])


def _ff_inputs(shape_in, shape_out, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape_in, generator=g).to(DEV) * 1.5 + 0.3,
            torch.randn(*shape_out, generator=g).to(DEV))


@pytest.mark.parametrize('dims,B,L', [((64, 64, 128), 2, 120), ((128, 128, 64), 2, 35)])
def test_feedforward_matches_the_module_definition(dims, B, L, flavour):
    """FeedForward(64, 64, 128) on 2 x 120 tokens and FeedForward(128, 128, 64) on 2 x 35 in
    training mode against the module's own definition in fp64 (CPU)."""
    ff = _head(*dims)
    x, G = _ff_inputs((B, L, dims[0]), (B, L, dims[2]), seed=7)
    _compare_ff_with_autocast(ff, x, G, 'fp64')


test_feedforward_matches_the_module_definition_fp16 = fp16_twin(
    test_feedforward_matches_the_module_definition)


def test_veon_feedforward_matches_the_module_definition(flavour):
    """FeedForward(384, 384, 2304) on 6 x (32 x 88) tokens; the yardstick is the fp32
    definition on the device (fp32's own error is some 1e4 below the half roundings being
    compared)."""
    ff = _head(384, 384, 2304)
    x, G = _ff_inputs((6, 32 * 88, 384), (6, 32 * 88, 2304), seed=8)
    _compare_ff_with_autocast(ff, x, G, 'fp32')


test_veon_feedforward_matches_the_module_definition_fp16 = fp16_twin(
    test_veon_feedforward_matches_the_module_definition)


def test_forward_resized_matches_the_unreordered_definition(flavour):
    """forward_resized with the switch on (hidden -> resize -> Linear on the surviving
    tokens) against the module's un-reordered definition (Linear on every token, then the
    resize) in fp64: FeedForward(64, 64, 128), side (8, 12) -> (2, 3).  The autocast run is
    the autocast of that same un-reordered definition."""
    ff = _head(64, 64, 128)
    x, G = _ff_inputs((2, 96, 64), (2, 128, 2, 3), seed=9)
    _compare_ff_with_autocast(ff, x, G, 'fp64', resized=((8, 12), (2, 3)))


test_forward_resized_matches_the_unreordered_definition_fp16 = fp16_twin(
    test_forward_resized_matches_the_unreordered_definition)


def test_switch_and_call_counts(flavour):
    """Per FeedForward step: 2 weight gradients, 2 column sums, 1 LayerNorm backward, one
    GELU and one GELU backward; 4 GEMMs (2 forward, 2 data gradients).  When neither the
    input nor the LayerNorm's parameters need a gradient, the first data-gradient GEMM and
    the LayerNorm backward are skipped; an input without a gradient alone skips neither
    (dgamma and dbeta come from that pass)."""
    names = NEW + (GEMM,)
    ff = _head(64, 64, 128).to(DEV)
    x = torch.randn(2, 120, 64, device=DEV)

    def step(m, needs_input_grad):
        def run():
            xi = x[..., :m.net[1].in_features].clone().requires_grad_(needs_input_grad)
            m(xi).sum().backward()
        return run
    assert FeedForward.hip_train is False
    assert _counts(step(ff, True), names) == (0, 0, 0, 0, 0, 0)   # the default: torch
    FeedForward.hip_train = True
    assert _counts(step(ff, True), names) == (2, 2, 1, 1, 1, 4)
    assert _counts(step(ff, False), names) == (2, 2, 1, 1, 1, 4)
    frozen = copy.deepcopy(ff)
    for p in frozen.net[0].parameters():
        p.requires_grad_(False)
    assert _counts(step(frozen, False), names) == (2, 2, 0, 1, 1, 3)
    ff.eval()                                           # eval mode keeps the inference path
    with torch.no_grad():
        assert _counts(lambda: ff(x), names) == (0, 0, 0, 0, 0, 0)
    odd = FeedForward(72, 72, 72).to(DEV).train()       # a width the kernels do not take
    x72 = torch.randn(2, 120, 72, device=DEV, requires_grad=True)
    assert _counts(lambda: odd(x72).sum().backward(), names) == (0, 0, 0, 0, 0, 0)


def test_two_identical_steps_are_bit_equal(flavour):
    ff = _head(64, 64, 128)
    x, G = _ff_inputs((2, 120, 64), (2, 120, 128), seed=12)
    a = _ff_step(ff, x, G, 'native')
    b = _ff_step(ff, x, G, 'native')
    for k in a:
        assert torch.equal(a[k], b[k]), k


test_two_identical_steps_are_bit_equal_fp16 = fp16_twin(test_two_identical_steps_are_bit_equal)


def test_an_optimizer_step_works(flavour):
    """Four native SGD steps lower an MSE loss monotonically; eval-mode inference with
    conv_dtype set afterwards (the existing native path, its half weights re-packed after
    train() / eval(): NativeCacheMixin) agrees with the torch definition within 2e-2."""
    ff = _head(64, 64, 128).to(DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 120, 64, generator=g).to(DEV)
    target = torch.randn(2, 120, 128, generator=g).to(DEV)
    opt = torch.optim.SGD(ff.parameters(), lr=0.1)
    FeedForward.hip_train = True
    before = _lib.CALLS.get(WGRAD, 0)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = F.mse_loss(ff(x), target)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    assert _lib.CALLS[WGRAD] - before == 8
    print('losses', losses)
    assert losses[3] < losses[2] < losses[1] < losses[0], losses
    ff.eval()
    with torch.no_grad():
        ff.conv_dtype = flavour
        n0 = _lib.CALLS.get(GEMM, 0)
        got = ff(x)
        assert _lib.CALLS.get(GEMM, 0) == n0 + 2
        ff.conv_dtype = None
        want = ff(x)
    rel = _rel(got, want)
    assert rel < 2e-2, rel


# --------------------------------------------------------------- token LayerNorm switch
def test_token_layernorm_switch_on_a_side_adaptor_block(flavour):
    """HighresSideAdaptorBlock(64, mlp_dim=64, neck_dim=64, pre_norm=True, use_add=True),
    one step on 2 x (10 x 12) tokens with an offset map, all switches on against all off
    (fp32): the gradients of pre_norm, ln_3, ln_4 and of the input within
    e(native) <= 2 e(autocast), the autocast run being the same block under
    torch.autocast.  Three LayerNorm backwards run natively.  Measured on an MI355X:
    e(native) / e(autocast) between 0.34 and 1.08 (pre_norm.bias in bf16, 3.6e-3 / 3.3e-3;
    dx 3.4e-3 / 3.8e-3 in bf16, 4.3e-4 / 9.9e-4 in fp16); ln_4.bias against its fp64 sum
    7.6e-8 / 7.8e-8.  The factor 2 did not have to move."""
    torch.manual_seed(5)
    blk = HighresSideAdaptorBlock(64, mlp_dim=64, neck_dim=64, pre_norm=True, use_add=True)
    with torch.no_grad():
        for ln in (blk.pre_norm, blk.ln_3, blk.ln_4):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.2)
    blk = blk.to(DEV).train()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 120, 64, generator=g).to(DEV)
    ext = torch.randn(2, 64, 3, 4, generator=g).to(DEV)
    G = torch.randn(2, 120, 64, generator=g).to(DEV)

    def step(how):
        b = copy.deepcopy(blk)
        xi = x.clone().requires_grad_(True)
        _all_switches(how == 'native')
        try:
            with torch.autocast('cuda', dtype=half.dtype(), enabled=how == 'autocast'):
                out = b(xi, None, ext, None, ext, (10, 12))
            out.float().backward(G)
        finally:
            _all_switches(False)
        res = {'dx': xi.grad}
        res.update({k: p.grad for k, p in b.named_parameters()
                    if k.split('.')[0] in ('pre_norm', 'ln_3', 'ln_4')})
        return res
    ref = step('fp32')
    # the gradient of ln_4.bias is the plain fp32 sum of G over the tokens in the fp32 and
    # in the autocast run (the same kernel on the same numbers: e(autocast) = 0 by
    # construction), so its yardstick is that sum in fp64
    ref['ln_4.bias'] = G.double().sum((0, 1))
    before = _lib.CALLS.get(LNBWD, 0)
    nat = step('native')
    assert _lib.CALLS.get(LNBWD, 0) == before + 3
    auto = step('autocast')
    assert len(ref) == 7
    for k in sorted(ref):
        e_n, e_a = _rel(nat[k], ref[k]), _rel(auto[k], ref[k])
        print('block %-16s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        assert e_n <= 2 * e_a, (k, e_n, e_a)


test_token_layernorm_switch_on_a_side_adaptor_block_fp16 = fp16_twin(
    test_token_layernorm_switch_on_a_side_adaptor_block)


# -------------------------------------------------------------------- in place on the path
def test_native_heads_and_layernorms_in_place_on_the_path():
    """The set-up of tests/test_hsa_train_gpu.py::test_native_convblocks_in_place_on_the_path
    (the tiny path, hsa_dim 64, the HSA network in training mode) with all four switches on:
    a finite gradient on every HSA parameter; with e the relative L2 distance to the same
    step with every switch off (torch fp32), e(native) <= 2 e(autocast), the autocast run
    wrapping the same modules (ConvBlocks and FeedForward heads; the token LayerNorms are
    fp32 under autocast too); and the new entry points' call counts: two heads (4 weight
    gradients, 4 column sums, 2 GELU pairs, 2 LayerNorm backwards) and seven token
    LayerNorms (pre_norm + ln_3 + ln_4, ln_3 + ln_4, ln_3 + ln_4).

    Measured on an MI355X (bf16): e(native) between 1.0e-3 and 1.3e-2 over the 54 HSA
    parameters, e(autocast) between 7.3e-3 and 1.8e-2; the largest ratio is 1.02
    (hsa_net_body.0.ln_3.weight).  The factor 2 did not have to move."""
    from tests.conftest import load_golden
    from tests.test_align_loss_gpu import _fixture
    from tests.test_path_golden import _build, _inputs
    from veon_amd.models.semantic_net import occ_loss as occ_loss_mod
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=False)
    images, geom, metric = _inputs(g, DEV)
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
    wrapped = [m for m in net.hsa.modules() if isinstance(m, (ConvBlock, FeedForward))]
    assert len(wrapped) == 5 and all(m.training for m in wrapped)
    params = dict(net.hsa.named_parameters())

    def autocast_of(m, name):
        inner = getattr(type(m), name)

        def call(*a, **kw):
            with torch.autocast('cuda', dtype=half.dtype()):
                return inner(m, *a, **kw).float()
        return call

    def run(how):
        if how == 'autocast':
            for m in wrapped:
                m.forward = autocast_of(m, 'forward')
                if isinstance(m, FeedForward):
                    m.forward_resized = autocast_of(m, 'forward_resized')
        _all_switches(how == 'native')
        net.zero_grad(set_to_none=True)
        before = dict(_lib.CALLS)
        try:
            with torch.enable_grad():
                out = net(images, geom, depth=metric, return_features=True)
                sum(net.occ_loss(out, *args).values()).backward()
        finally:
            _all_switches(False)
            for m in wrapped:
                m.__dict__.pop('forward', None)
                m.__dict__.pop('forward_resized', None)
        return ({k: None if p.grad is None else p.grad.clone() for k, p in params.items()},
                tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in NEW))

    ref, n_ref = run('fp32')
    nat, n_nat = run('native')
    auto, n_auto = run('autocast')
    assert n_ref == (0,) * 5 and n_auto == (0,) * 5
    assert n_nat == (4, 4, 2 + 7, 2, 2), n_nat
    ratios = []
    for k in params:
        assert nat[k] is not None and torch.isfinite(nat[k]).all(), k
        e_n, e_a = _rel(nat[k], ref[k]), _rel(auto[k], ref[k])
        print('path %-44s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        ratios.append((e_n / max(e_a, 1e-30), k))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(ratios))
