"""CPU checks of the prediction heads' native training switch
(``_PredHead3D.hip_train``, veon_amd/models/semantic_net/align_net_body.py): the switch
changes nothing without a ROCm device, its gate, the moved autograd functions, the
hand-over kernels' host-only argument checks and the header."""
import ctypes
import inspect

import pytest
import torch

from veon_amd import _lib
from veon_amd.models import _train_fns
from veon_amd.models.semantic_net import align_net_body, temporal_fusion
from veon_amd.models.semantic_net.align_net_body import (PredHead3DOcc, PredHead3DSem,
                                                          ResBlock3D, _PredHead3D, run_blocks)

ENTRY_POINTS = ('veon_volume_unpack_cl_f32', 'veon_volume_sigm_bwd_pack_cl')


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _PredHead3D.hip_train = False
    ResBlock3D.hip_train = False


def test_header_declares_and_libraries_export_the_entry_points():
    from veon_amd import build
    build.build()
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    ptr, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib._SIGNATURES['veon_volume_unpack_cl_f32'] == (i, [ptr, ptr] + [i] * 6 + [ptr])
    assert _lib._SIGNATURES['veon_volume_sigm_bwd_pack_cl'] == (
        i, [ptr] * 4 + [i64] + [i] * 5 + [ptr])
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), (flavour, name)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2      # the additions are additive


def test_hand_over_kernels_refuse_bad_arguments_on_the_host():
    """The checks that run before any launch (no device needed)."""
    lib = _lib.lib()
    bad = 1                                      # VEON_ERR_BAD_ARG
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 64)
    unpack, spack = lib.veon_volume_unpack_cl_f32, lib.veon_volume_sigm_bwd_pack_cl
    assert unpack(None, p, 1, 8, 2, 1, 1, 1, None) == bad
    assert unpack(p, q, 1, 8, 9, 1, 1, 1, None) == bad          # C > Cp
    assert unpack(p, q, 1, 6, 2, 1, 1, 1, None) == bad          # Cp % 4
    assert unpack(p, q, 0, 8, 2, 1, 1, 1, None) == bad
    assert unpack(p, q, 1, 8, 2, 1, (1 << 20) + 1, 1, None) == bad
    st = (ctypes.c_int64 * 4)(64, 64, 64, 64)
    sp = ctypes.cast(st, ctypes.c_void_p)
    guard = int(lib.veon_conv3d_guard_rows(2, 3))
    assert spack(p, sp, p, q, guard + 1, 1, 64, 2, 2, 3, None) == bad     # not the grid's guard
    assert spack(p, sp, p, p, guard, 1, 64, 2, 2, 3, None) == bad         # aliased
    assert spack(p, sp, p, q, guard, 1, 62, 2, 2, 3, None) == bad         # C % 4
    assert spack(p, None, p, q, guard, 1, 64, 2, 2, 3, None) == bad
    short = (ctypes.c_int64 * 4)(64, 64, 64, 32)                          # rows overlap
    assert spack(p, ctypes.cast(short, ctypes.c_void_p), p, q, guard, 1, 64, 2, 2, 3,
                 None) == bad
    neg = (ctypes.c_int64 * 4)(64, -64, 64, 64)
    assert spack(p, ctypes.cast(neg, ctypes.c_void_p), p, q, guard, 1, 64, 2, 2, 3, None) == bad


def test_the_moved_functions_have_one_definition():
    assert temporal_fusion._rows_linear is _train_fns._rows_linear
    assert temporal_fusion._BNReLUTrainFn is _train_fns._BNReLUTrainFn
    assert align_net_body._rows_linear is _train_fns._rows_linear
    src = inspect.getsource(temporal_fusion)
    assert 'def _rows_linear' not in src and 'class _BNReLUTrainFn' not in src


def _heads(embed):
    torch.manual_seed(0)
    return PredHead3DOcc(embed, 2), PredHead3DSem(embed, 64)


def _run(head, x):
    x = x.clone().requires_grad_(True)
    out = head(x)
    out.square().sum().backward()
    res = {'out': out.detach(), 'dx': x.grad}
    res.update({'grad:' + k: p.grad for k, p in head.named_parameters()})
    res.update({'buf:' + k: b.detach().clone() for k, b in head.named_buffers()})
    return res


@pytest.mark.parametrize('which', [0, 1])
def test_switch_changes_nothing_on_the_cpu(which):
    x = torch.randn(2, 64, 2, 3, 5, generator=torch.Generator().manual_seed(1))
    assert _PredHead3D.hip_train is False
    off = _run(_heads(64)[which].train(), x)
    _PredHead3D.hip_train = True
    head = _heads(64)[which].train()
    assert head.hip_train is True and not head._hip_train_ok(x)
    on = _run(head, x)
    assert off.keys() == on.keys()
    for k in off:
        assert torch.equal(off[k], on[k]), k


def test_gate():
    _PredHead3D.hip_train = True
    x = torch.randn(1, 256, 1, 2, 2)
    for head in _heads(256):
        head.train()
        assert head._train_structure_ok()
        assert not head._hip_train_ok(x)                         # a CPU tensor
        assert not head._hip_train_ok((torch.zeros(4, 256), (1, 256, 1, 1, 1)))
        head.eval()
        assert not head._train_structure_ok() and not head._hip_train_ok(x)
        head.train()
        with torch.no_grad():
            assert not head._hip_train_ok(x)
    occ64, sem64 = _heads(64)
    assert not occ64.train()._train_structure_ok()               # middle width 16
    assert sem64.train()._train_structure_ok()
    assert not occ64._hip_train_ok(torch.randn(1, 64, 1, 2, 2))
    # a BN without running statistics, a feature width the GEMM does not divide
    occ, sem = _heads(256)
    occ.occ_conv1.bn = torch.nn.BatchNorm3d(64, track_running_stats=False)
    assert not occ.train()._train_structure_ok()
    assert not PredHead3DSem(256, 100).train()._train_structure_ok()
    # only the head that pads a narrow last conv to 64 rows may have one
    assert not PredHead3DSem(256, 8).train()._train_structure_ok()
    assert PredHead3DOcc(256, 8).train()._train_structure_ok()
    assert not PredHead3DOcc(256, 9).train()._train_structure_ok()
    _PredHead3D.hip_train = False
    assert not sem.train()._hip_train_ok(x)


def test_state_dict_keys_are_unchanged():
    occ, sem = _heads(256)
    assert list(occ.state_dict()) == [
        'occ_conv1.conv.weight', 'occ_conv1.bn.weight', 'occ_conv1.bn.bias',
        'occ_conv1.bn.running_mean', 'occ_conv1.bn.running_var',
        'occ_conv1.bn.num_batches_tracked', 'occ_conv2.conv.weight']
    assert [k for k in sem.state_dict() if 'bn' not in k] == [
        'occ_conv1.conv.weight', 'occ_conv1.conv.bias', 'occ_conv2.conv.weight',
        'occ_conv3.conv.weight']
    assert 'hip_train' not in vars(occ) and 'hip_train' not in vars(sem)


def test_run_blocks_default_is_unchanged_and_heads_take_a_plain_volume():
    torch.manual_seed(2)
    blocks = [ResBlock3D(8, 8).train() for _ in range(2)]
    x = torch.randn(1, 8, 2, 3, 3)
    a = run_blocks(blocks, x)
    for b in blocks:                              # the same batches again
        for m in b.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.reset_running_stats()
    b = run_blocks(blocks, x, return_storage=True)   # no native run: the fp32 volume
    assert torch.is_tensor(b) and torch.equal(a, b)
    assert 'return_storage' in inspect.signature(run_blocks).parameters
    assert inspect.signature(run_blocks).parameters['return_storage'].default is False
