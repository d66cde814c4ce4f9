"""Host-side checks of the synchronised BatchNorm of the native training paths
(veon_amd/sync_bn.py): the C ABI additions, the torch mirror
``batch_norm_train`` against nn.BatchNorm3d in fp64, the group lookup, and the switch's
structure test on a converted block (plain torch, CPU)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from veon_amd import _lib, sync_bn
from veon_amd.models.semantic_net import ResBlock3D

_I, _P, _D = ctypes.c_int, ctypes.c_void_p, ctypes.c_double

# what the wrappers of veon_amd/sync_bn.py pass, stream last
WANT = {
    # y stats workspace | B C Z Y X | stream
    'veon_bn3d_sums_stats_bf16': (_I, [_P] * 3 + [_I] * 5 + [_P]),
    # da a y mean rstd stats sums workspace | B C Z Y X | stream
    'veon_bn3d_bwd_sums_stats_bf16': (_I, [_P] * 8 + [_I] * 5 + [_P]),
    # stats gamma beta mean_offset | eps momentum | running_mean running_var
    # num_batches_tracked mean rstd scale shift | C | stream
    'veon_bn_train_coeffs': (_I, [_P] * 4 + [_D] * 2 + [_P] * 7 + [_I] + [_P]),
    # stats gamma mean rstd ca cb cc | C | stream
    'veon_bn_bwd_coeffs': (_I, [_P] * 7 + [_I] + [_P]),
}


def test_header_and_libraries_carry_the_sync_bn_entry_points():
    from veon_amd import build
    build.build()
    declared = set(_lib.declared_symbols())
    for name, (restype, argtypes) in WANT.items():
        assert name in declared, name
        assert _lib._SIGNATURES[name] == (restype, argtypes), name
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        for name in WANT:
            assert hasattr(lib, name), (flavour, name)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2      # the additions are additive


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('identity', [False, True])
@pytest.mark.parametrize('momentum', [0.1, None])
def test_mirror_without_a_group_is_batchnorm3d(momentum, identity, relu):
    """``batch_norm_train(group=None)`` against autograd through nn.BatchNorm3d (+ identity)
    (+ ReLU) in fp64 over two steps (num_batches_tracked drives momentum=None): output, dx,
    dgamma, dbeta, the identity's gradient and the three buffers."""
    g = torch.Generator().manual_seed(1)
    C = 6
    bn = nn.BatchNorm3d(C, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.normal_(0, 0.2, generator=g)
        bn.running_mean.normal_(0, 0.2, generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    mine = copy.deepcopy(bn)
    shape = (2, C, 3, 4, 5)
    y = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    ident = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    y2, ident2 = (t.detach().clone().requires_grad_(True) for t in (y, ident))
    da = torch.randn(shape, generator=g, dtype=torch.float64)

    def close(p, q):
        return ((p - q).norm() / q.norm()).item() <= 1e-10
    for step in range(2):
        for t in (y, ident, y2, ident2, bn.weight, bn.bias, mine.weight, mine.bias):
            t.grad = None
        z = bn(y)
        z = z + ident if identity else z
        a = torch.relu(z) if relu else z
        a.backward(da)
        got = sync_bn.batch_norm_train(y2, mine, ident2 if identity else None, relu=relu,
                                       group=None)
        got.backward(da)
        assert close(got.detach(), a.detach()) and close(y2.grad, y.grad)
        assert close(mine.weight.grad, bn.weight.grad) and close(mine.bias.grad, bn.bias.grad)
        if identity:
            assert close(ident2.grad, ident.grad)
        else:
            assert ident2.grad is None
        assert close(mine.running_mean, bn.running_mean)
        assert close(mine.running_var, bn.running_var)
        assert int(mine.num_batches_tracked) == int(bn.num_batches_tracked) == step + 1


def test_is_sync_and_group_of():
    import torch.distributed as dist
    plain, sync = nn.BatchNorm3d(8), nn.SyncBatchNorm(8)
    assert not sync_bn.is_sync(plain) and sync_bn.is_sync(sync)
    assert sync_bn.is_sync(nn.SyncBatchNorm.convert_sync_batchnorm(nn.BatchNorm3d(8)))
    assert not dist.is_initialized()
    assert sync_bn.group_of(sync) is None and sync_bn.group_of(plain) is None
    marker = object()
    sync.process_group = marker
    assert sync_bn.group_of(sync) is marker
    # no group: no collective, the buffer comes back as it is
    before = sync_bn.ALL_REDUCE_CALLS
    stats = torch.arange(5, dtype=torch.float64)
    assert sync_bn.all_reduce(stats, None) is stats
    assert sync_bn.ALL_REDUCE_CALLS == before


def test_group_of_takes_the_default_group_once_initialised(tmp_path):
    """A one-rank gloo group in this process: ``group_of`` returns the default group, the
    collective is issued (and counted) although the world has one rank, and the mirror
    gives the same numbers as without a group."""
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='file://%s' % (tmp_path / 'rdv'), rank=0,
                            world_size=1)
    try:
        bn = nn.SyncBatchNorm(4).double().train()
        assert sync_bn.group_of(bn) is dist.group.WORLD
        own = dist.new_group([0])
        bn.process_group = own
        assert sync_bn.group_of(bn) is own
        bn.process_group = None
        g = torch.Generator().manual_seed(2)
        x = torch.randn(3, 4, 2, 2, 2, generator=g, dtype=torch.float64)
        ref = copy.deepcopy(bn)
        before = sync_bn.ALL_REDUCE_CALLS
        xa = x.clone().requires_grad_(True)
        out = sync_bn.batch_norm_train(xa, bn)
        out.sum().backward()
        assert sync_bn.ALL_REDUCE_CALLS == before + 2      # forward and backward
        xb = x.clone().requires_grad_(True)
        want = sync_bn.batch_norm_train(xb, ref, group=None)
        want.sum().backward()
        assert sync_bn.ALL_REDUCE_CALLS == before + 2
        assert torch.equal(out, want) and torch.equal(xa.grad, xb.grad)
        assert torch.equal(bn.running_var, ref.running_var)
    finally:
        dist.destroy_process_group()


def test_a_converted_block_keeps_the_native_structure():
    """``convert_sync_batchnorm`` swaps the BN modules and nothing the structure test of
    ``ResBlock3D.hip_train`` reads (nor that of the prediction heads and of the temporal
    fusion's ConvModule3d)."""
    from veon_amd.models.semantic_net.align_net_body import (ConvModule3d, PredHead3DOcc,
                                                               conv_module_train_ok)
    convert = nn.SyncBatchNorm.convert_sync_batchnorm
    blk = convert(ResBlock3D(64, 64)).train()
    assert sync_bn.is_sync(blk.conv1.bn) and sync_bn.is_sync(blk.conv2.bn)
    assert blk._train_structure_ok() and ResBlock3D(64, 64).train()._train_structure_ok()
    blk.conv2.bn.eval()
    assert not blk._train_structure_ok()
    head = convert(PredHead3DOcc(256, 2)).train()
    assert sync_bn.is_sync(head.occ_conv1.bn) and head._train_structure_ok()
    cm = convert(ConvModule3d(64, 64, 3, 1, 1, bias=False, norm=True, act=True)).train()
    assert sync_bn.is_sync(cm.bn) and conv_module_train_ok(cm)
    # without a ROCm volume the switch still leaves the torch definition in charge
    ResBlock3D.hip_train = True
    try:
        assert not convert(ResBlock3D(64, 64)).train()._hip_train_ok(torch.zeros(1, 64, 2, 3, 3))
    finally:
        ResBlock3D.hip_train = False
