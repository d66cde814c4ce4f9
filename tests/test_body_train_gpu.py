"""Native training of the Conv3d body (csrc/conv3d_train.hip) on the
MI355X: the MFMA weight gradient, the data gradient through the forward kernel, the
train-mode BatchNorm passes, and ``ResBlock3D.hip_train`` against the module's own
definition.  Every test here calls the new wrappers or asserts on their call counts, so
all of them fail on a tree without the feature.

Yardsticks (none of them taken from the code under test):
 * fp64 results computed from the SAME half-rounded operands;
 * hard bounds from fp32 addition: products of two half values are exact in fp32, so a
   K-term sum errs by at most K * 2^-24 * sum |terms|;
 * rocBLAS's fp32 product of the same operands (wgrad), torch under ``torch.autocast``
   with the flavour's half dtype (block / body): measured errors of parent-commit code
   against the same fp64 result, with a stated factor on top.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import flavour, fp16_twin, half_tol, to_half  # noqa: F401
from tests.helpers import halo_is_zero as _halo_is_zero
from veon_amd import _lib, conv3d_ops, half
from veon_amd.models.semantic_net import AlignBody3D, ResBlock3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WGRAD, CONV = 'veon_conv3d_k3_wgrad_bf16', 'veon_conv3d_k3_bf16'
SMALL = [(2, 64, 64, 4, 10, 12), (2, 64, 128, 3, 7, 5), (2, 128, 64, 3, 7, 5)]
VEON = (1, 256, 256, 8, 100, 100)


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    ResBlock3D.hip_train = False


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _volumes(B, Cin, Cout, Z, Y, X, seed):
    """dy: Gaussian on EVERY interior voxel (so non-zero rows lie next to every face of
    the grid and a wrong tap offset cannot hide in zeros); x: rectified Gaussian."""
    g = torch.Generator().manual_seed(seed)
    dy = to_half(torch.randn(B, Cout, Z, Y, X, generator=g)).to(DEV)
    x = to_half(torch.randn(B, Cin, Z, Y, X, generator=g).relu()).to(DEV)
    return conv3d_ops.pack(dy), conv3d_ops.pack(x), dy, x


def _wgrad_references(dy, x):
    """fp64 dW, S = |dy|^T |x_shifted| (fp64) and rocBLAS's fp32 product, per tap, from
    the padded rows themselves (guard rows where row + off leaves the grid)."""
    B, Cin, Z, Y, X = x.shape
    Cout = dy.shape[1]
    want = torch.empty(Cout, 3, 3, 3, Cin, dtype=torch.float64, device=DEV)
    S = torch.empty_like(want)
    blas = torch.empty(Cout, 3, 3, 3, Cin, dtype=torch.float32, device=DEV)
    d64 = dy.rows.double()
    d32 = dy.rows.float()
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                off = ((kz - 1) * (Y + 2) + (ky - 1)) * (X + 2) + (kx - 1)
                xs = x.storage[x.guard + off:x.guard + off + x.M]
                want[:, kz, ky, kx] = d64.t() @ xs.double()
                S[:, kz, ky, kx] = d64.abs().t() @ xs.double().abs()
                blas[:, kz, ky, kx] = d32.t() @ xs.float()
    return want, S, blas


@pytest.mark.parametrize('B,Cin,Cout,Z,Y,X', SMALL + [VEON])
def test_wgrad_against_fp64(B, Cin, Cout, Z, Y, X, flavour):
    """(a) small shapes: |got - want| <= K 2^-24 S elementwise, K = padded rows (fp32
    addition of exact products).  (b) every shape: relative L2 error against fp64 at most
    8 x that of rocBLAS's fp32 product of the same operands (two fp32 summation orders
    of identical exact products; the factor is the issue's, from a CPU simulation of the
    MFMA order).  Measured on an MI355X, relative L2 kernel / rocBLAS fp32 (the factor 8
    did not have to move; the kernel is below rocBLAS at every shape):
        shape (B, Cin, Cout, Z, Y, X)    bf16                   fp16
        (2,  64,  64, 4,  10,  12)       6.9e-8 / 1.3e-7        1.1e-7 / 3.3e-7
        (2,  64, 128, 3,   7,   5)       4.9e-8 / 5.2e-8        1.0e-7 / 1.4e-7
        (2, 128,  64, 3,   7,   5)       5.0e-8 / 5.3e-8        1.0e-7 / 1.4e-7
        (1, 256, 256, 8, 100, 100)       6.5e-7 / 1.5e-6        7.4e-7 / 2.3e-6"""
    dyv, xv, dy, x = _volumes(B, Cin, Cout, Z, Y, X, seed=Cin + 3 * Cout + X)
    before = _lib.CALLS.get(WGRAD, 0)
    got = conv3d_ops.conv3d_k3_wgrad(dyv, xv)
    assert _lib.CALLS[WGRAD] == before + 1
    assert got.shape == (Cout, 3, 3, 3, Cin) and got.dtype == torch.float32
    want, S, blas = _wgrad_references(dyv, xv)
    e_k, e_b = _rel(got, want), _rel(blas, want)
    print('wgrad %s %s: rel L2 kernel %.3e, rocBLAS fp32 %.3e' %
          (half.name(), (B, Cin, Cout, Z, Y, X), e_k, e_b))
    if (B, Cin, Cout, Z, Y, X) != VEON:
        bound = xv.M * 2.0 ** -24 * S
        assert bool(((got.double() - want).abs() <= bound).all())
    assert e_k <= 8 * e_b, (e_k, e_b)


test_wgrad_against_fp64_fp16 = fp16_twin(test_wgrad_against_fp64)


def test_wgrad_is_the_conv_weight_gradient():
    """The tap convention: dW equals autograd's weight gradient of F.conv3d (fp64, CPU)."""
    B, Cin, Cout, Z, Y, X = SMALL[1]
    dyv, xv, dy, x = _volumes(B, Cin, Cout, Z, Y, X, seed=5)
    w = torch.zeros(Cout, Cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.cpu().double(), w, padding=1).backward(dy.cpu().double())
    got = conv3d_ops.conv3d_k3_wgrad(dyv, xv).permute(0, 4, 1, 2, 3).cpu()
    assert _rel(got, w.grad) < 1e-5


@pytest.mark.parametrize('B,Cin,Cout,Z,Y,X', SMALL + [VEON])
def test_dgrad_through_the_forward_kernel(B, Cin, Cout, Z, Y, X, flavour):
    """conv3d_k3(dy, pack_weight_dgrad(w)) against the input gradient in fp64 on the half
    operands (the transposed convolution), at the tolerance tests/test_conv3d_gpu.py
    states for a half-precision conv output."""
    g = torch.Generator().manual_seed(Cin + Cout + Y)
    dy = to_half(torch.randn(B, Cout, Z, Y, X, generator=g)).to(DEV)
    w = to_half(torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (27 * Cout) ** -0.5).to(DEV)
    if (B, Cin, Cout, Z, Y, X) == VEON:
        # no fp64 convolution on the device, and 283 GFLOP is too much for the CPU: the
        # same fp64 sum as 27 fp64 GEMMs over the padded rows of dy,
        # dx[m][ci] = sum_tap sum_co dy[m - off(tap)][co] w[co][ci][tap]
        dv = conv3d_ops.pack(dy)
        rows = torch.zeros(dv.M, Cin, dtype=torch.float64, device=DEV)
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    off = ((kz - 1) * (Y + 2) + (ky - 1)) * (X + 2) + (kx - 1)
                    src = dv.storage[dv.guard - off:dv.guard - off + dv.M]
                    rows += src.double() @ w[:, :, kz, ky, kx].double()
        want = rows.view(B, Z + 2, Y + 2, X + 2, Cin)[:, 1:-1, 1:-1, 1:-1] \
            .permute(0, 4, 1, 2, 3).float().contiguous()
    else:
        want = F.conv_transpose3d(dy.cpu().double(), w.cpu().double(), padding=1).float().to(DEV)
    wd = conv3d_ops.pack_weight_dgrad(w).to(half.dtype())
    out = conv3d_ops.conv3d_k3(conv3d_ops.pack(dy), wd)
    got = conv3d_ops.unpack(out)
    rms = want.pow(2).mean().sqrt().item()
    tol = half_tol(2.0 ** -7, 2e-3)
    assert bool(((got - want).abs() <= want.abs() * tol['rtol'] + tol['atol'] * rms).all())


test_dgrad_through_the_forward_kernel_fp16 = fp16_twin(test_dgrad_through_the_forward_kernel)


def _ncdhw(vol):
    return vol.interior().permute(0, 4, 1, 2, 3).double()


def _within_half_rounding(got, want):
    rms = want.pow(2).mean().sqrt().item()
    tol = half_tol(2.0 ** -8, 2e-3)
    return bool(((got - want).abs() <= want.abs() * tol['rtol'] + tol['atol'] * rms).all())


# the narrow and wide ones: one lane per row, idle threads, one row in flight (the 'bn' rows
# of tests/reduce_seams.py)
@pytest.mark.parametrize('B,C,Z,Y,X', [(2, 64, 4, 10, 12), (2, 128, 3, 7, 5), (1, 256, 8, 100, 100),
                                       (1, 8, 2, 3, 4), (1, 72, 2, 3, 4), (1, 1032, 1, 2, 3),
                                       (1, 2048, 1, 1, 2)])
def test_bn_passes_against_fp64(B, C, Z, Y, X, flavour):
    """Sums, normalise (+ identity, + ReLU) and the backward pass against the fp64 torch
    functions of tests/test_body_train.py on the same half inputs."""
    g = torch.Generator().manual_seed(C + X)
    y = conv3d_ops.pack((torch.randn(B, C, Z, Y, X, generator=g) * 1.5 + 0.3).to(DEV))
    ident = conv3d_ops.pack(torch.randn(B, C, Z, Y, X, generator=g).to(DEV))
    da = conv3d_ops.pack(torch.randn(B, C, Z, Y, X, generator=g).to(DEV))
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    n, eps = B * Z * Y * X, 1e-5
    y64 = _ncdhw(y)
    K = y.M

    sums = conv3d_ops.bn_sums(y)
    red = [0, 2, 3, 4]
    want = torch.stack([y64.sum(red), (y64 * y64).sum(red)])
    S = torch.stack([y64.abs().sum(red), (y64 * y64).sum(red)])
    assert bool(((sums.double() - want).abs() <= K * 2.0 ** -24 * S).all())

    mean, var, rstd = conv3d_ops.bn_batch_stats(sums, n, eps)
    for ident_v, relu in ((None, True), (ident, True), (None, False)):
        a64, m64, v64, r64 = conv3d_ops.bn_train_forward_ref(
            y64, gamma.double(), beta.double(), eps,
            None if ident_v is None else _ncdhw(ident_v), relu)
        assert _rel(mean, m64) < 1e-5 and _rel(rstd, r64) < 1e-5
        scale = (gamma.double() * rstd).float()
        shift = (beta.double() - mean * gamma.double() * rstd).float()
        a = conv3d_ops.bn_apply(y, scale, shift, ident=ident_v, relu=relu)
        assert _halo_is_zero(a)
        assert _within_half_rounding(_ncdhw(a), a64)

    # backward of BN + identity + ReLU, from the STORED activation (the mask's source)
    a = conv3d_ops.bn_apply(y, scale, shift, ident=ident, relu=True)
    a64, d64 = _ncdhw(a), _ncdhw(da)
    dy64, dg64, db64, dz64 = conv3d_ops.bn_train_backward_ref(d64, a64, y64, m64, r64,
                                                              gamma.double())
    bs = conv3d_ops.bn_bwd_sums(da, a, y, mean.float(), rstd.float())
    xhat = (y64 - m64.view(1, -1, 1, 1, 1)) * r64.view(1, -1, 1, 1, 1)
    want = torch.stack([db64, dg64])
    S = torch.stack([dz64.abs().sum(red), (dz64 * xhat).abs().sum(red)])
    # xhat is an fp32 value here (three roundings), not an exact product: K + 4
    assert bool(((bs.double() - want).abs() <= (K + 4) * 2.0 ** -24 * S).all())
    ca, cb, cc = conv3d_ops.bn_bwd_coefficients(bs, n, gamma, mean.float(), rstd.float())
    dyv, dzv = conv3d_ops.bn_bwd_apply(da, a, y, ca, cb, cc, want_dz=True)
    assert _halo_is_zero(dyv) and _halo_is_zero(dzv)
    assert _within_half_rounding(_ncdhw(dyv), dy64)
    assert torch.equal(_ncdhw(dzv), dz64)     # a selection of half values: exact


test_bn_passes_against_fp64_fp16 = fp16_twin(test_bn_passes_against_fp64)


# ------------------------------------------------------- block / body against the module
def _module(kind, width, depth, seed=3):
    torch.manual_seed(seed)
    mod = ResBlock3D(width, width) if kind == 'block' else AlignBody3D(width, depth)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
        if isinstance(m, torch.nn.Conv3d):
            m.weight.data = to_half(m.weight.data)
    return mod.train()


def _step(mod, x, G, how):
    """One forward + backward of a copy of ``mod``: {name: tensor} of the output, the
    input gradient, every parameter gradient and every BN buffer afterwards."""
    mod = copy.deepcopy(mod)
    ResBlock3D.hip_train = how == 'native'
    if how == 'fp64':
        mod, x, G = mod.double().cpu(), x.double().cpu(), G.double().cpu()
    else:
        mod = mod.to(DEV)
    x = x.clone().requires_grad_(True)
    if how == 'autocast':
        with torch.autocast('cuda', dtype=half.dtype()):
            out = mod(x)
    else:
        out = mod(x)
    out.backward(G.to(out.dtype))
    ResBlock3D.hip_train = False
    res = {'out': out.detach(), 'dx': x.grad}
    res.update({'grad:' + k: p.grad for k, p in mod.named_parameters()})
    res.update({'buf:' + k: b.detach() for k, b in mod.named_buffers()})
    return res


def _compare_with_autocast(mod, x, G, exact_how):
    """e = relative L2 error against the exact run; e(native) <= 2 e(autocast) for every
    quantity (both round the same operands to the same format and accumulate in fp32; the
    native path additionally rounds the stored conv output before BN and the gradient
    between blocks: at most about twice autocast's count of half roundings per conv).
    Where e(autocast) is exactly zero the native value must be equal.

    torch's autocast path does run for these modules on the device (MIOpen half convs),
    so the issue's fallback yardstick is not used.  Measured on an MI355X; the factor 2
    did not have to move.  Largest e(native) / e(autocast) over all quantities, and the
    pairs e(native) / e(autocast) of the output and the input gradient:
        ResBlock3D(64, 64)   bf16  1.16 (grad conv2.bn.weight)   out 2.8e-3 / 3.4e-3  dx 3.6e-2 / 4.0e-2
        AlignBody3D(64, 2)   bf16  1.09 (grad 1.conv2.bn.weight) out 4.2e-3 / 4.9e-3  dx 6.4e-2 / 6.8e-2
        ResBlock3D(64, 64)   fp16  1.09 (out)                    out 3.5e-4 / 3.3e-4  dx 8.5e-3 / 1.4e-2
        AlignBody3D(64, 2)   fp16  1.14 (1.conv2.bn.running_mean) out 5.3e-4 / 5.1e-4 dx 1.6e-2 / 2.0e-2
        AlignBody3D(256, 4)  bf16  1.10 (grad 0.conv2.bn.weight) out 6.8e-3 / 7.2e-3  dx 1.2e-1 / 1.2e-1
        AlignBody3D(256, 4)  fp16  1.19 (0.conv1.bn.running_var) out 8.5e-4 / 8.1e-4  dx 4.2e-2 / 4.3e-2
    (the full lists are what the test prints)."""
    exact = _step(mod, x, G, exact_how)
    before = dict(_lib.CALLS)
    nat = _step(mod, x, G, 'native')
    assert _lib.CALLS.get(WGRAD, 0) > before.get(WGRAD, 0)
    auto = _step(mod, x, G, 'autocast')
    assert set(nat) == set(exact) == set(auto)
    worst = []
    for k in sorted(exact):
        want = exact[k].to(DEV)
        assert nat[k] is not None and nat[k].shape == want.shape, k
        if not want.is_floating_point():
            assert torch.equal(nat[k].to(DEV), want), k
            continue
        e_n, e_a = _rel(nat[k].to(DEV), want), _rel(auto[k].to(DEV), want)
        print('%-46s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k, e_n, e_a))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst)[:2])


@pytest.mark.parametrize('kind', ['block', 'body'])
def test_block_and_body_match_the_module_definition(kind, flavour):
    """ResBlock3D(64, 64) / AlignBody3D(64, 2) in training mode, B = 2, 4 x 10 x 12,
    against the module's own definition in fp64 (CPU: no fp64 convolution on the device)."""
    mod = _module(kind, 64, 2)
    g = torch.Generator().manual_seed(7)
    x = to_half(torch.randn(2, 64, 4, 10, 12, generator=g)).to(DEV)
    G = torch.randn(2, 64, 4, 10, 12, generator=g).to(DEV)
    _compare_with_autocast(mod, x, G, 'fp64')


test_block_and_body_match_the_module_definition_fp16 = fp16_twin(
    test_block_and_body_match_the_module_definition)


def test_veon_body_matches_the_module_definition(flavour):
    """AlignBody3D(256, 4) on 1 x 8 x 100 x 100; the yardstick is the fp32 definition on
    the device (an fp64 Conv3d of 283 GFLOP is not something to wait for; fp32's own
    error is some 1e4 below the half roundings being compared)."""
    mod = _module('body', 256, 4)
    g = torch.Generator().manual_seed(8)
    x = to_half(torch.randn(1, 256, 8, 100, 100, generator=g).relu()).to(DEV)
    G = torch.randn(1, 256, 8, 100, 100, generator=g).to(DEV)
    _compare_with_autocast(mod, x, G, 'fp32')


test_veon_body_matches_the_module_definition_fp16 = fp16_twin(
    test_veon_body_matches_the_module_definition)


def _counts(fn):
    before = dict(_lib.CALLS)
    fn()
    return (_lib.CALLS.get(WGRAD, 0) - before.get(WGRAD, 0),
            _lib.CALLS.get(CONV, 0) - before.get(CONV, 0))


def test_switch_and_call_counts():
    body = _module('body', 64, 2).to(DEV)
    x = torch.randn(2, 64, 4, 10, 12, device=DEV)

    def step(needs_input_grad):
        def run():
            xi = x.clone().requires_grad_(needs_input_grad)
            body(xi).sum().backward()
        return run
    assert ResBlock3D.hip_train is False
    assert _counts(step(True)) == (0, 0)          # the default: torch, as before
    ResBlock3D.hip_train = True
    assert _counts(step(True)) == (4, 8)          # 4 forward + 4 data gradients
    assert _counts(step(False)) == (4, 7)         # the first block's input needs none
    body.eval()                                   # eval mode keeps the inference paths
    with torch.no_grad():
        assert _counts(lambda: body(x)) == (0, 4)
    other = ResBlock3D(64, 64).to(DEV).train()    # a conv bias is not the body's
    other.conv2.conv = torch.nn.Conv3d(64, 64, 3, 1, 1, bias=True).to(DEV)   # structure:
    assert _counts(lambda: other(x).sum().backward()) == (0, 0)              # torch


def test_two_identical_steps_are_bit_equal(flavour):
    mod = _module('body', 64, 2)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 64, 4, 10, 12, generator=g).to(DEV)
    G = torch.randn(2, 64, 4, 10, 12, generator=g).to(DEV)
    a, b = _step(mod, x, G, 'native'), _step(mod, x, G, 'native')
    for k in a:
        assert torch.equal(a[k], b[k]), k


test_two_identical_steps_are_bit_equal_fp16 = fp16_twin(test_two_identical_steps_are_bit_equal)


def test_wgrad_is_bit_reproducible_at_the_veon_shape():
    dyv, xv, _, _ = _volumes(*VEON, seed=2)
    a = conv3d_ops.conv3d_k3_wgrad(dyv, xv)
    b = conv3d_ops.conv3d_k3_wgrad(dyv, xv)
    assert torch.equal(a, b)


def test_an_optimizer_step_works():
    """Three native SGD steps lower an MSE loss; eval-mode inference afterwards (the
    existing native path, re-folded after train() / eval()) agrees with the torch
    definition in eval mode within the 1.5e-2 of the existing body test."""
    body = _module('body', 64, 2).to(DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 64, 4, 10, 12, generator=g).to(DEV)
    target = torch.randn(2, 64, 4, 10, 12, generator=g).relu().to(DEV)
    opt = torch.optim.SGD(body.parameters(), lr=0.05)
    ResBlock3D.hip_train = True
    before = _lib.CALLS.get(WGRAD, 0)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = F.mse_loss(body(x), target)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    assert _lib.CALLS[WGRAD] - before == 16
    assert losses[3] < losses[2] < losses[1] < losses[0], losses
    body.eval()
    with torch.no_grad():
        got = body(x)
        body.use_hip = False
        want = body(x)
    rel = _rel(got, want)
    assert rel < 1.5e-2, rel


def test_native_blocks_in_place_on_the_path():
    """The tiny path of tests/test_path_golden.py with the body's blocks in training mode,
    ``fuse_ds_grad`` on the neck and ``hip_train`` on the blocks: forward with
    return_features, occ_loss, backward.  Two weight gradients per block; finite non-zero
    gradients on the 2-D fusion layer in front of the lift and on every body parameter;
    and, with e the relative L2 distance to the same step with hip_train = False (torch
    fp32, the behaviour without the switch), e(native) <= 2 e(autocast), the autocast run
    wrapping only the body's blocks.

    Measured on an MI355X (bf16): e(native) between 1.6e-2 and 1.3e-1 over the 32
    parameters, e(autocast) between 2.1e-2 and 1.4e-1; the largest ratio is 1.16
    (body1.conv2.bn.weight, 7.2e-2 / 6.2e-2), and native is below autocast on 24 of the
    32.  The factor 2 did not have to move."""
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
    dec = net.occ_decoder
    blocks = list(dec.layers_3d_body)
    for blk in blocks:
        blk.train()
        assert blk.hip_supported()
    net.view_transformer.fuse_ds_grad = True
    params = {'fusion2d.' + k: p for k, p in dec.fusion_layers['layer_0'].named_parameters()}
    for i, blk in enumerate(blocks):
        params.update({'body%d.%s' % (i, k): p for k, p in blk.named_parameters()})
    buffers0 = [b.clone() for blk in blocks for b in blk.buffers()]

    def run(how):
        with torch.no_grad():      # every run starts from the same running statistics
            for b, b0 in zip([b for blk in blocks for b in blk.buffers()], buffers0):
                b.copy_(b0)
        if how == 'autocast':
            for blk in blocks:
                def forward(x, blk=blk):
                    with torch.autocast('cuda', dtype=half.dtype()):
                        return type(blk).forward(blk, x).float()
                blk.forward = forward
        ResBlock3D.hip_train = how == 'native'
        net.zero_grad(set_to_none=True)
        before = _lib.CALLS.get(WGRAD, 0)
        try:
            with torch.enable_grad():
                out = net(images, geom, depth=metric, return_features=True)
                sum(net.occ_loss(out, *args).values()).backward()
        finally:
            ResBlock3D.hip_train = False
            for blk in blocks:
                blk.__dict__.pop('forward', None)
        return {k: p.grad.clone() for k, p in params.items()}, _lib.CALLS.get(WGRAD, 0) - before

    ref, n_ref = run('fp32')
    nat, n_nat = run('native')
    auto, n_auto = run('autocast')
    assert n_ref == 0 and n_auto == 0 and n_nat == 2 * len(blocks)
    for k in params:
        assert torch.isfinite(nat[k]).all() and nat[k].abs().max() > 0, k
        e_n, e_a = _rel(nat[k], ref[k]), _rel(auto[k], ref[k])
        print('path %-34s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
