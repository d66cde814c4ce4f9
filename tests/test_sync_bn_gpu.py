"""The synchronised BatchNorm of the native training paths on the MI355X
(veon_amd/sync_bn.py, csrc/conv3d_train.hip): the fp64 stage two at the
seams of tests/reduce_seams.py, a batch split into "ranks" whose messages are added with
one torch ``+``, the coefficient kernels against the fp64 mirror, the three module-level
paths with ``nn.SyncBatchNorm`` against the same modules with plain BatchNorm3d, once
without a process group and once through a one-rank RCCL group, and the bad arguments.

Yardsticks (none of them taken from the code under test):
 * integer operands, on which every summation order is exact: equality with fp64 sums;
 * the fp64 mirror (``sync_bn.train_coeffs_ref`` / ``bwd_coeffs_ref``) fed fp64 sums of the
   same half-rounded volumes;
 * the existing un-synchronised passes on the same whole batch.
"""
import copy
import ctypes
import socket

import pytest
import torch
import torch.nn as nn

from tests import reduce_seams as rs
from tests.helpers import flavour, fp16_twin, halo_is_zero, to_half  # noqa: F401
from veon_amd import _lib, conv3d_ops, half, sync_bn
from veon_amd.models.semantic_net.align_net_body import (ConvModule3d, PredHead3DOcc,
                                                          ResBlock3D, _PackFn, _PredHead3D,
                                                          _UnpackFn, conv_module_train,
                                                          conv_module_train_ok)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
U = 2.0 ** -24                  # unit roundoff of fp32
ULP = 2.0 ** -23                # one fp32 ulp, relative
FILLS = ['interior', 'padded']
SPLIT = [(3, 64, 3, 5, 6), (3, 128, 2, 4, 4)]     # whole batch; "ranks" hold 2 + 1 samples


@pytest.fixture(autouse=True)
def _switches_off_afterwards():
    yield
    ResBlock3D.hip_train = False
    _PredHead3D.hip_train = False


def _gen(shape, salt=0):
    return torch.Generator().manual_seed(sum(shape) + 7 * len(shape) + salt)


def _ints(size, g):
    """Integers in [-4, 4], none zero."""
    return (torch.randint(1, 5, size, generator=g) *
            (2 * torch.randint(0, 2, size, generator=g) - 1)).float()


def _cl(shape):
    B, C, *spatial = shape
    return (B, *spatial, C)


def _grid(shape, values=None, fill='interior'):
    """A fresh zeroed PaddedVolume with ``values`` on its interior (B, Z, Y, X, C), or with
    fill='padded' on EVERY padded row (M, C), as tests/test_reduce_seams_gpu.py fills it."""
    grid = conv3d_ops.PaddedVolume(*shape, DEV)
    if values is not None:
        (grid.interior() if fill == 'interior' else grid.rows).copy_(values.to(DEV))
    return grid


def _size(shape, fill):
    return _cl(shape) if fill == 'interior' else (rs.plan_of('bn', shape)['M'], shape[1])


def _count(shape):
    B, C, Z, Y, X = shape
    return B * Z * Y * X


def _rows_sum(t):
    return t.sum(list(range(t.dim() - 1)))


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _nan_workspaces():
    for ws in conv3d_ops._WORKSPACES.values():
        ws.fill_(float('nan'))


# ============================================================ stage two, exact at the seams
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('shape', rs.shapes_of('bn'), ids=rs.ids_of('bn'))
def test_forward_stats_on_integers_are_exact(shape, fill, flavour):
    """Integers in [-4, 4] (the operands of test_bn_sums_on_integers_are_exact): both fp64
    sums EQUAL the fp64 sums of the rows, the last element is B Z Y X, and the buffer is
    bit-equal on a second call and from a NaN-filled workspace and output."""
    C = shape[1]
    y = _grid(shape, _ints(_size(shape, fill), _gen(shape)), fill)
    before = _lib.CALLS.get('veon_bn3d_sums_stats_bf16', 0)
    got = sync_bn.bn_sums_stats(y)
    assert _lib.CALLS['veon_bn3d_sums_stats_bf16'] == before + 1
    assert got.dtype == torch.float64 and tuple(got.shape) == (2 * C + 1,)
    y64 = y.rows.double()
    assert torch.equal(got[:C], _rows_sum(y64)) and torch.equal(got[C:2 * C], _rows_sum(y64 * y64))
    assert float(got[C:2 * C].min()) > 0
    assert float(got[2 * C]) == _count(shape)
    assert torch.equal(sync_bn.bn_sums_stats(y), got)
    _nan_workspaces()
    out = torch.full_like(got, float('nan'))
    assert sync_bn.bn_sums_stats(y, out=out) is out
    assert torch.equal(out, got)


test_forward_stats_on_integers_are_exact_fp16 = fp16_twin(test_forward_stats_on_integers_are_exact)


@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('mask', ['positive', 'masked'])
@pytest.mark.parametrize('shape', rs.shapes_of('bn'), ids=rs.ids_of('bn'))
def test_backward_stats_on_integers_are_exact(shape, mask, fill, flavour):
    """The operands of test_bn_bwd_sums_on_integers_are_exact (da, y integers, mean integer,
    rstd a power of two, a positive or masked): both fp64 sums EQUAL the fp64 ones, the
    fp32 copy equals them too, the count is B Z Y X; bit-equal again and from NaN."""
    C = shape[1]
    g = _gen(shape, 1)
    size = _size(shape, fill)
    da = _grid(shape, _ints(size, g), fill)
    y = _grid(shape, _ints(size, g), fill)
    a_val = torch.randint(1, 5, size, generator=g).float()
    if mask == 'masked':
        a_val = a_val * torch.randint(0, 2, size, generator=g)
    a = _grid(shape, a_val, fill)
    mean = torch.randint(-2, 3, (C,), generator=g).float().to(DEV)
    rstd = (2.0 ** torch.randint(-1, 2, (C,), generator=g).float()).to(DEV)
    got, sums = sync_bn.bn_bwd_sums_stats(da, a, y, mean, rstd)
    d64, a64, y64 = da.rows.double(), a.rows.double(), y.rows.double()
    dz = d64 * (a64 > 0)
    xhat = (y64 - mean.double()) * rstd.double()
    want = torch.stack([_rows_sum(dz), _rows_sum(dz * xhat)])
    assert float(_rows_sum((dz * xhat).abs()).max()) < 2.0 ** 23 and float(dz.abs().sum()) > 0
    assert torch.equal(got[:2 * C].view(2, C), want) and float(got[2 * C]) == _count(shape)
    assert sums.dtype == torch.float32 and torch.equal(sums.double(), want)
    again, sums_again = sync_bn.bn_bwd_sums_stats(da, a, y, mean, rstd)
    assert torch.equal(again, got) and torch.equal(sums_again, sums)
    _nan_workspaces()
    out = (torch.full_like(got, float('nan')), torch.full_like(sums, float('nan')))
    sync_bn.bn_bwd_sums_stats(da, a, y, mean, rstd, out=out)
    assert torch.equal(out[0], got) and torch.equal(out[1], sums)


test_backward_stats_on_integers_are_exact_fp16 = fp16_twin(
    test_backward_stats_on_integers_are_exact)


# ================================================================== a batch split in ranks
def _split(values):
    """(3, ...) channels-last values -> the whole batch and its "ranks" of 2 + 1 samples."""
    return values, (values[:2], values[2:])


def _vol(values):
    B, *spatial, C = values.shape
    return _grid((B, C, *spatial), values)


def _padded(vol):
    B, C, Z, Y, X = vol.shape
    return vol.rows.view(B, Z + 2, Y + 2, X + 2, C)


def _buffers(C, g):
    return ((torch.randn(C, generator=g) * 0.2).to(DEV),
            (torch.rand(C, generator=g) + 0.5).to(DEV),
            torch.zeros((), dtype=torch.int64, device=DEV))


@pytest.mark.parametrize('shape', SPLIT, ids=['x'.join(map(str, s)) for s in SPLIT])
def test_rank_split_on_integers_is_bit_equal(shape, flavour):
    """Three integer-valued samples as "ranks" of 2 + 1: the messages of the ranks, added
    with one torch ``+``, are BIT-EQUAL to the whole batch's in both directions; so are
    the coefficient vectors and buffers computed from either, the apply passes of each
    rank against its slice of the whole-batch run, and the ranks' fp32 (dbeta, dgamma) add
    to the whole batch's."""
    B, C, Z, Y, X = shape
    g = _gen(shape, 5)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    y_all, y_parts = _split(_ints(_cl(shape), g))
    whole, ranks = _vol(y_all), [_vol(v) for v in y_parts]
    s_whole = sync_bn.bn_sums_stats(whole)
    s_ranks = [sync_bn.bn_sums_stats(v) for v in ranks]
    assert [float(s[2 * C]) for s in s_ranks] == [2 * Z * Y * X, Z * Y * X]
    summed = s_ranks[0] + s_ranks[1]
    assert torch.equal(summed, s_whole) and float(summed[2 * C]) == B * Z * Y * X
    buf0 = _buffers(C, g)
    coeffs, bufs = [], []
    for stats in (s_whole, summed):
        rm, rv, nbt = (t.clone() for t in buf0)
        coeffs.append(sync_bn.bn_train_coeffs(stats, gamma, beta, EPS, 0.1, rm, rv, nbt))
        bufs.append((rm, rv, nbt))
    for p, q in zip(coeffs[0] + bufs[0], coeffs[1] + bufs[1]):
        assert torch.equal(p, q)
    assert int(bufs[1][2]) == 1 and not torch.equal(bufs[1][0], buf0[0])
    mean, rstd, scale, shift = coeffs[1]
    a_whole = conv3d_ops.bn_apply(whole, scale, shift, relu=True)
    a_ranks = [conv3d_ops.bn_apply(v, scale, shift, relu=True) for v in ranks]
    assert torch.equal(_padded(a_whole)[:2], _padded(a_ranks[0]))
    assert torch.equal(_padded(a_whole)[2:], _padded(a_ranks[1]))
    assert float(a_whole.rows.float().abs().max()) > 0

    # backward: integer da and mask, integer mean, rstd a power of two (exact terms)
    da_all, da_parts = _split(_ints(_cl(shape), g))
    m_all, m_parts = _split(torch.randint(0, 2, _cl(shape), generator=g).float())
    mu = torch.randint(-2, 3, (C,), generator=g).float().to(DEV)
    r = (2.0 ** torch.randint(-1, 2, (C,), generator=g).float()).to(DEV)
    d_whole, d_ranks = _vol(da_all), [_vol(v) for v in da_parts]
    k_whole, k_ranks = _vol(m_all), [_vol(v) for v in m_parts]
    b_whole, l_whole = sync_bn.bn_bwd_sums_stats(d_whole, k_whole, whole, mu, r)
    back = [sync_bn.bn_bwd_sums_stats(d, k, v, mu, r) for d, k, v in zip(d_ranks, k_ranks, ranks)]
    b_summed = back[0][0] + back[1][0]
    assert torch.equal(b_summed, b_whole)
    assert torch.equal(back[0][1] + back[1][1], l_whole) and float(l_whole.abs().max()) > 0
    c_whole = sync_bn.bn_bwd_coeffs(b_whole, gamma, mu, r)
    c_summed = sync_bn.bn_bwd_coeffs(b_summed, gamma, mu, r)
    for p, q in zip(c_whole, c_summed):
        assert torch.equal(p, q)
    dy_whole = conv3d_ops.bn_bwd_apply(d_whole, k_whole, whole, *c_summed)
    dy_ranks = [conv3d_ops.bn_bwd_apply(d, k, v, *c_summed)
                for d, k, v in zip(d_ranks, k_ranks, ranks)]
    assert torch.equal(_padded(dy_whole)[:2], _padded(dy_ranks[0]))
    assert torch.equal(_padded(dy_whole)[2:], _padded(dy_ranks[1]))
    assert halo_is_zero(dy_ranks[1]) and float(dy_whole.rows.float().abs().max()) > 0


test_rank_split_on_integers_is_bit_equal_fp16 = fp16_twin(test_rank_split_on_integers_is_bit_equal)


def _sums64(vol):
    v = vol.rows.double()
    return _rows_sum(v), _rows_sum(v * v)


def _message64(s0, s1, n):
    return torch.cat([s0, s1, torch.tensor([float(n)], dtype=torch.float64, device=DEV)])


def _within(tag, new, want):
    """A vector against its fp64 value: relative L2 error (the ``_rel`` of
    tests/test_body_train_gpu.py) below the 1e-5 that file puts on the existing statistics
    (tests/test_body_train_gpu.py:188, ``_rel(mean, m64) < 1e-5 and _rel(rstd, r64) <
    1e-5``)."""
    e_new = _rel(new, want)
    print('%-22s e(sync) %.3e' % (tag, e_new))
    assert e_new < 1e-5, (tag, e_new)
    return e_new


def _no_worse(tag, new, old, want):
    """``_within``, and not above the existing un-synchronised path's error on the same
    whole batch by more than one fp32 ulp (2^-23, relative): stage two in fp64 can only
    remove error."""
    e_new, e_old = _within(tag, new, want), _rel(old, want)
    print('%-22s e(plain) %.3e' % (tag, e_old))
    assert e_new <= e_old + ULP, (tag, e_new, e_old)


@pytest.mark.parametrize('offset', [False, True], ids=['plain', 'mean_offset'])
@pytest.mark.parametrize('momentum', [0.1, None])
@pytest.mark.parametrize('shape', SPLIT, ids=['x'.join(map(str, s)) for s in SPLIT])
def test_gaussian_rank_split_against_the_fp64_mirror(shape, momentum, offset, flavour):
    """Gaussian samples split 2 + 1, channel 3 constant (var == 0), two steps (momentum=None
    needs num_batches_tracked), optionally the conv bias of ``_BNReLUTrainFn`` as
    ``mean_offset`` (it enters running_mean only).  mean, rstd, scale, shift, ca, cb, cc and
    the running buffers against the fp64 mirror fed fp64 sums of the same half-rounded
    volumes:
     * from the ranks' added messages: within the 1e-5 of ``_within``;
     * from the whole batch's message, where stage one is bit for bit that of the existing
       path (``bn_sums`` + ``bn_batch_stats`` + ``bn_update_running``, ``bn_bwd_sums`` +
       ``bn_bwd_coefficients``) and only stage two and the algebra differ: additionally by
       the rule of ``_no_worse`` against that path."""
    B, C, Z, Y, X = shape
    n = B * Z * Y * X
    g = _gen(shape, 6)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    bias = (torch.randn(C, generator=g) * 0.5).to(DEV) if offset else None
    y_val = torch.randn(_cl(shape), generator=g) * 1.5 + 0.3
    y_val[..., 3] = 3.0
    y_all, y_parts = _split(y_val)
    whole, ranks = _vol(y_all), [_vol(v) for v in y_parts]
    assert [v.shape[0] for v in ranks] == [2, 1]
    buf0 = _buffers(C, g)
    rm, rv, nbt = (t.clone() for t in buf0)                        # the new path's, split
    rm_w, rv_w, nbt_w = (t.clone() for t in buf0)                  # ... on the whole batch
    rm64, rv64, nbt64 = buf0[0].double(), buf0[1].double(), buf0[2].clone()    # the mirror's
    plain = nn.BatchNorm3d(C, eps=EPS, momentum=momentum).to(DEV).train()     # the existing
    with torch.no_grad():
        plain.running_mean.copy_(buf0[0])
        plain.running_var.copy_(buf0[1])
    for step in range(2):
        stats = sync_bn.bn_sums_stats(ranks[0]) + sync_bn.bn_sums_stats(ranks[1])
        got = sync_bn.bn_train_coeffs(stats, gamma, beta, EPS, momentum, rm, rv, nbt, bias)
        parts = [_sums64(v) for v in ranks]
        stats64 = _message64(parts[0][0], parts[0][1], 2 * Z * Y * X) + \
            _message64(parts[1][0], parts[1][1], Z * Y * X)
        want = sync_bn.train_coeffs_ref(stats64, gamma, beta, EPS, momentum, rm64, rv64, nbt64,
                                        bias)
        mean_o, var_o, rstd_o = conv3d_ops.bn_batch_stats(conv3d_ops.bn_sums(whole), n, EPS)
        conv3d_ops.bn_update_running(
            plain, mean_o if bias is None else mean_o + bias.double(), var_o, n)
        scale_o = gamma.double() * rstd_o
        old = (mean_o.float(), rstd_o.float(), scale_o.float(),
               (beta.double() - mean_o * scale_o).float())
        got_w = sync_bn.bn_train_coeffs(sync_bn.bn_sums_stats(whole), gamma, beta, EPS,
                                        momentum, rm_w, rv_w, nbt_w, bias)
        for tag, p, pw, q, w in zip(('mean', 'rstd', 'scale', 'shift'), got, got_w, old, want):
            assert p.dtype == torch.float32
            _within(tag + ' (split)', p, w)
            _no_worse(tag, pw, q, w)
        _within('running_mean (split)', rm, rm64)
        _within('running_var (split)', rv, rv64)
        _no_worse('running_mean', rm_w, plain.running_mean, rm64)
        _no_worse('running_var', rv_w, plain.running_var, rv64)
        assert int(nbt) == int(nbt_w) == int(nbt64) == int(plain.num_batches_tracked) == step + 1
        # the constant channel: the sums are exact, so var == 0 and rstd = eps^-1/2
        assert float(got[0][3]) == 3.0
        assert abs(float(got[1][3]) - EPS ** -0.5) <= ULP * EPS ** -0.5
    if offset:      # the bias moved running_mean and nothing else
        rm2, rv2, nbt2 = (t.clone() for t in buf0)
        again = sync_bn.bn_train_coeffs(stats, gamma, beta, EPS, 0.1, rm2, rv2, nbt2, None)
        rm3, rv3, nbt3 = (t.clone() for t in buf0)
        with_b = sync_bn.bn_train_coeffs(stats, gamma, beta, EPS, 0.1, rm3, rv3, nbt3, bias)
        for p, q in zip(again, with_b):
            assert torch.equal(p, q)
        assert torch.equal(rv2, rv3)
        assert _rel(rm3 - rm2, 0.1 * bias) < 1e-5

    # backward, every path from the SAME fp32 mean and rstd and the stored activation
    mean, rstd, scale, shift = got
    a_whole = conv3d_ops.bn_apply(whole, scale, shift, relu=True)
    a_ranks = [conv3d_ops.bn_apply(v, scale, shift, relu=True) for v in ranks]
    da_all, da_parts = _split(to_half(torch.randn(_cl(shape), generator=g)))
    d_whole, d_ranks = _vol(da_all), [_vol(v) for v in da_parts]
    back = [sync_bn.bn_bwd_sums_stats(d, a, v, mean, rstd)
            for d, a, v in zip(d_ranks, a_ranks, ranks)]
    got_c = sync_bn.bn_bwd_coeffs(back[0][0] + back[1][0], gamma, mean, rstd)
    d64, a64, y64 = d_whole.rows.double(), a_whole.rows.double(), whole.rows.double()
    dz = d64 * (a64 > 0)
    xhat = (y64 - mean.double()) * rstd.double()
    want_c = sync_bn.bwd_coeffs_ref(_message64(_rows_sum(dz), _rows_sum(dz * xhat), n), gamma,
                                    mean, rstd)
    s_old = conv3d_ops.bn_bwd_sums(d_whole, a_whole, whole, mean, rstd)
    old_c = conv3d_ops.bn_bwd_coefficients(s_old, n, gamma, mean, rstd)
    got_cw = sync_bn.bn_bwd_coeffs(
        sync_bn.bn_bwd_sums_stats(d_whole, a_whole, whole, mean, rstd)[0], gamma, mean, rstd)
    for tag, p, pw, q, w in zip(('ca', 'cb', 'cc'), got_c, got_cw, old_c, want_c):
        _within(tag + ' (split)', p, w)
        _no_worse(tag, pw, q, w)
    # the local sums of the ranks are the parameter gradients: they add to the whole's
    local = back[0][1].double() + back[1][1].double()
    S = torch.stack([_rows_sum(dz.abs()), _rows_sum((dz * xhat).abs())])
    want_s = torch.stack([_rows_sum(dz), _rows_sum(dz * xhat)])
    # tests/test_body_train_gpu.py:205, plus the two roundings to fp32 of the ranks' sums
    assert bool(((local - want_s).abs() <= (whole.M + 4 + 2) * U * S).all())


test_gaussian_rank_split_against_the_fp64_mirror_fp16 = fp16_twin(
    test_gaussian_rank_split_against_the_fp64_mirror)


# ============================================================================ module level
def _init(mod, seed):
    torch.manual_seed(seed)
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
        if isinstance(m, nn.Conv3d):
            m.weight.data = to_half(m.weight.data)
            if m.bias is not None:
                m.bias.data.normal_(0, 0.5)
    return mod.train()


def _call_conv_module(cm, x):
    """A ConvModule3d as the temporal fusion runs it natively, else its own definition."""
    if x.is_cuda and ResBlock3D.hip_train:
        assert conv_module_train_ok(cm)
        xs, shape = conv_module_train(cm, _PackFn.apply(x), tuple(x.shape))
        return _UnpackFn.apply(xs, shape)
    return cm(x)


# kind -> (module, input shape, output channels, how to call it, number of BN modules)
def _case(kind):
    if kind == 'block':
        return _init(ResBlock3D(64, 64), 3), (2, 64, 3, 5, 6), 64, None, 2
    if kind == 'temporal':
        cm = ConvModule3d(128, 64, 3, 1, 1, bias=False, norm=True, act=True)
        return _init(cm, 4), (2, 128, 2, 4, 4), 64, _call_conv_module, 1
    return _init(PredHead3DOcc(256, 2), 5), (2, 256, 3, 5, 6), 2, None, 1


KINDS = ['block', 'temporal', 'head']


def _step(mod, x, G, how, call):
    """One forward + backward of a copy of ``mod``: {name: tensor} of the output, the
    input gradient, every parameter gradient and every buffer afterwards.  'sync': the
    copy converted by ``convert_sync_batchnorm`` on the native path."""
    mod = copy.deepcopy(mod)
    native = how in ('native', 'sync')
    if how == 'sync':
        mod = nn.SyncBatchNorm.convert_sync_batchnorm(mod)
        assert any(sync_bn.is_sync(m) for m in mod.modules())
    if how == 'fp64':
        mod, x, G = mod.double().cpu(), x.double().cpu(), G.double().cpu()
    else:
        mod = mod.to(DEV)
    mod.train()
    x = x.clone().requires_grad_(True)
    call = call or (lambda m, t: m(t))
    ResBlock3D.hip_train = _PredHead3D.hip_train = native
    try:
        if how == 'autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                out = call(mod, x)
        else:
            out = call(mod, x)
        out.backward(G.to(out.dtype).to(out.device))
    finally:
        ResBlock3D.hip_train = _PredHead3D.hip_train = False
    res = {'out': out.detach(), 'dx': x.grad}
    res.update({'grad:' + k: p.grad for k, p in mod.named_parameters()})
    res.update({'buf:' + k: b.detach() for k, b in mod.named_buffers()})
    return res


NEW_CALLS = ('veon_bn3d_sums_stats_bf16', 'veon_bn3d_bwd_sums_stats_bf16',
             'veon_bn_train_coeffs', 'veon_bn_bwd_coeffs')
OLD_CALLS = ('veon_bn3d_sums_bf16', 'veon_bn3d_bwd_sums_bf16')


def _sync_step(mod, x, G, call, n_bn, collectives):
    """The converted module's step, with the call counts that show which path it took:
    one launch of each new entry point per BN and direction, none of the plain sums, and
    ``collectives`` all-reduces."""
    before, reduced = dict(_lib.CALLS), sync_bn.ALL_REDUCE_CALLS
    res = _step(mod, x, G, 'sync', call)
    for name in NEW_CALLS:
        assert _lib.CALLS.get(name, 0) - before.get(name, 0) == n_bn, name
    for name in OLD_CALLS:
        assert _lib.CALLS.get(name, 0) == before.get(name, 0), name
    assert sync_bn.ALL_REDUCE_CALLS - reduced == collectives
    return res


def _inputs(kind):
    mod, shape, cout, call, n_bn = _case(kind)
    g = torch.Generator().manual_seed(7)
    x = to_half(torch.randn(*shape, generator=g).relu()).to(DEV)
    G = torch.randn(shape[0], cout, *shape[2:], generator=g).to(DEV)
    return mod, x, G, call, n_bn


@pytest.mark.parametrize('kind', KINDS)
def test_converted_modules_match_the_plain_native_path(kind, flavour):
    """One forward + backward step of a ResBlock3D, of a ConvModule3d as the temporal
    fusion runs it, and of a PredHead3DOcc, converted by ``convert_sync_batchnorm``, with no
    process group: output, input gradient, every parameter gradient and every buffer
    against the same module with plain BatchNorm3d on the existing native path.  The
    tolerance is the one tests/test_body_train_gpu.py puts between native and reference
    (``assert e_n <= 2 * e_a``, tests/test_body_train_gpu.py:288), e the relative L2
    distance to the module's own definition in fp64 and e_a that of torch under autocast:
    it holds for the converted module, and the distance between the converted and the
    plain native results is within it as well.  Integer buffers are equal."""
    assert not torch.distributed.is_initialized()
    mod, x, G, call, n_bn = _inputs(kind)
    exact = _step(mod, x, G, 'fp64', call)
    before = dict(_lib.CALLS)
    nat = _step(mod, x, G, 'native', call)
    for name in OLD_CALLS:
        assert _lib.CALLS.get(name, 0) - before.get(name, 0) == n_bn, name
    for name in NEW_CALLS:
        assert _lib.CALLS.get(name, 0) == before.get(name, 0), name
    syn = _sync_step(mod, x, G, call, n_bn, collectives=0)
    auto = _step(mod, x, G, 'autocast', call)
    assert set(syn) == set(nat) == set(exact) == set(auto)
    for k in sorted(exact):
        want = exact[k].to(DEV)
        assert syn[k] is not None and syn[k].shape == want.shape, k
        if not want.is_floating_point():
            assert torch.equal(syn[k], want) and torch.equal(syn[k], nat[k]), k
            continue
        assert bool(torch.isfinite(syn[k]).all()), k
        e_s, e_n, e_a = _rel(syn[k], want), _rel(nat[k], want), _rel(auto[k].to(DEV), want)
        d = _rel(syn[k], nat[k]) if float(nat[k].abs().max()) > 0 else \
            float(syn[k].abs().max())
        print('%-36s e(sync) %.3e  e(native) %.3e  e(autocast) %.3e  sync - native %.3e'
              % (k, e_s, e_n, e_a, d))
        assert e_s <= 2 * e_a, (k, e_s, e_a)
        assert d <= 2 * e_a, (k, d, e_a)


test_converted_modules_match_the_plain_native_path_fp16 = fp16_twin(
    test_converted_modules_match_the_plain_native_path)


@pytest.fixture
def one_rank_rccl_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % port, rank=0,
                            world_size=1, device_id=torch.device(DEV))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def test_converted_modules_through_a_one_rank_rccl_group(flavour, one_rank_rccl_group):
    """The same three steps with a process group: every BN issues one all-reduce of its
    fp64 device buffer per direction (counted in ``sync_bn.all_reduce``, the ResBlock's four
    also with an input that needs no gradient), and the sum over one rank changes no bit
    of any result against the run without a group's collective."""
    import torch.distributed as dist
    assert dist.is_initialized() and sync_bn.group_of(nn.SyncBatchNorm(8)) is one_rank_rccl_group
    probe = torch.arange(5, dtype=torch.float64, device=DEV)
    count = sync_bn.ALL_REDUCE_CALLS
    assert sync_bn.all_reduce(probe, one_rank_rccl_group) is probe
    assert sync_bn.ALL_REDUCE_CALLS == count + 1
    assert torch.equal(probe.cpu(), torch.arange(5, dtype=torch.float64))
    for kind in KINDS:
        mod, x, G, call, n_bn = _inputs(kind)
        with_group = _sync_step(mod, x, G, call, n_bn, collectives=2 * n_bn)
        real = sync_bn.group_of
        sync_bn.group_of = lambda bn: None          # the same step, no collective
        try:
            without = _sync_step(mod, x, G, call, n_bn, collectives=0)
        finally:
            sync_bn.group_of = real
        assert set(with_group) == set(without)
        for k in with_group:
            assert torch.equal(with_group[k], without[k]), (kind, k)
    # needs_input_grad does not change which BN collectives run
    blk = nn.SyncBatchNorm.convert_sync_batchnorm(_case('block')[0]).to(DEV).train()
    ResBlock3D.hip_train = True
    count = sync_bn.ALL_REDUCE_CALLS
    blk(torch.randn(2, 64, 3, 5, 6, device=DEV)).sum().backward()
    assert sync_bn.ALL_REDUCE_CALLS == count + 4


test_converted_modules_through_a_one_rank_rccl_group_fp16 = fp16_twin(
    test_converted_modules_through_a_one_rank_rccl_group)


# =========================================================================== bad arguments
def test_bad_arguments_are_refused():
    """Each new entry point returns VEON_ERR_BAD_ARG for C % 8 != 0, C > 2048, a null
    pointer and a misaligned pointer, and launches nothing (the buffers keep their NaN)."""
    lib = _lib.lib()
    BAD = 1
    C = 64
    shape = (1, C, 2, 3, 4)
    y = _grid(shape, _ints(_cl(shape), _gen(shape)))
    ws = conv3d_ops._bn_workspace(2048, DEV)
    stats = torch.full((2 * 2056 + 2,), float('nan'), dtype=torch.float64, device=DEV)
    vec = [torch.full((2056 + 1,), float('nan'), device=DEV) for _ in range(8)]
    sums = torch.full((2 * 2056 + 1,), float('nan'), device=DEV)
    nbt = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))

    def p(t, off=0):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + off)

    def fwd(yp=p(y.rows), sp=p(stats), wp=p(ws), c=C):
        return lib.veon_bn3d_sums_stats_bf16(yp, sp, wp, 1, c, 2, 3, 4, st)

    def bwd(dp=p(y.rows), ap=p(y.rows), yp=p(y.rows), mp=p(vec[0]), rp=p(vec[1]),
            sp=p(stats), fp=p(sums), wp=p(ws), c=C):
        return lib.veon_bn3d_bwd_sums_stats_bf16(dp, ap, yp, mp, rp, sp, fp, wp, 1, c, 2, 3, 4,
                                                 st)

    def train(sp=p(stats), gp=p(vec[0]), bp=p(vec[1]), op=None, rm=p(vec[2]), rv=p(vec[3]),
              nb=p(nbt), mp=p(vec[4]), rp=p(vec[5]), scp=p(vec[6]), shp=p(vec[7]), c=C):
        return lib.veon_bn_train_coeffs(sp, gp, bp, op, EPS, 0.1, rm, rv, nb, mp, rp, scp, shp,
                                        c, st)

    def back(sp=p(stats), gp=p(vec[0]), mp=p(vec[1]), rp=p(vec[2]), ap=p(vec[3]),
             bp=p(vec[4]), cp=p(vec[5]), c=C):
        return lib.veon_bn_bwd_coeffs(sp, gp, mp, rp, ap, bp, cp, c, st)

    for fn in (fwd, bwd, train, back):
        assert fn(c=60) == BAD and fn(c=2056) == BAD and fn(c=0) == BAD
        assert fn(sp=None) == BAD                      # null
        assert fn(sp=p(stats, 4)) == BAD               # fp64 buffer off its alignment
    assert fwd(yp=None) == BAD and fwd(wp=None) == BAD and fwd(yp=p(y.rows, 8)) == BAD
    assert bwd(dp=None) == BAD and bwd(ap=None) == BAD and bwd(mp=None) == BAD
    assert bwd(rp=None) == BAD and bwd(fp=None) == BAD and bwd(wp=None) == BAD
    assert bwd(dp=p(y.rows, 8)) == BAD and bwd(ap=p(y.rows, 2)) == BAD
    assert bwd(fp=p(sums, 2)) == BAD
    assert train(gp=None) == BAD and train(bp=None) == BAD and train(mp=None) == BAD
    assert train(rp=None) == BAD and train(scp=None) == BAD and train(shp=None) == BAD
    assert train(rm=None) == BAD and train(nb=None) == BAD        # running: all or none
    assert train(gp=p(vec[0], 2)) == BAD and train(nb=p(nbt, 4)) == BAD
    assert train(op=p(vec[4], 2)) == BAD
    assert back(gp=None) == BAD and back(mp=None) == BAD and back(rp=None) == BAD
    assert back(ap=None) == BAD and back(bp=None) == BAD and back(cp=None) == BAD
    assert back(cp=p(vec[5], 2)) == BAD
    torch.cuda.synchronize()
    for t in [stats, sums] + vec:
        assert bool(torch.isnan(t).all())
    assert int(nbt.sum()) == 0
