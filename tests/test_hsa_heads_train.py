"""Host-side checks of the native training path of the HSA heads and token LayerNorms
(csrc/linear_train.hip): the C ABI additions, the linear weight
gradient's workspace plan, the torch references against fp64 autograd, and the three
switches (plain torch, CPU)."""
import copy
import ctypes

import torch
import torch.nn.functional as F

from veon_amd import _lib, conv3d_ops, vit_ops
from veon_amd.models.semantic_net.hsa_network import (AttnManipulateBlock, FeedForward,
                                                      HighresSideAdaptorBlock)

_I, _L, _P, _F = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float

# what the wrappers of veon_amd/vit_ops.py pass, stream last
WANT = {
    # M K N (host-only)
    'veon_linear_wgrad_workspace_bytes': (_L, [_I] * 3),
    # dy x dw workspace | workspace_bytes | M K N | stream
    'veon_linear_wgrad_bf16': (_I, [_P] * 4 + [_L] + [_I] * 3 + [_P]),
    'veon_rows_colsum_workspace_bytes': (_L, [_I]),
    # dy sums workspace | workspace_bytes | M N | stream
    'veon_rows_colsum_bf16': (_I, [_P] * 3 + [_L] + [_I] * 2 + [_P]),
    # y h | n | stream
    'veon_gelu_bf16': (_I, [_P] * 2 + [_L] + [_P]),
    # dh y dy | n | stream
    'veon_gelu_bwd_bf16': (_I, [_P] * 3 + [_L] + [_P]),
    'veon_layernorm_f32_bwd_workspace_bytes': (_L, [_I]),
    # dout | dout_half | x gamma dx sums workspace | bytes | T d | eps | stream
    'veon_layernorm_f32_bwd': (_I, [_P, _I] + [_P] * 5 + [_L] + [_I] * 2 + [_F] + [_P]),
}
NEW = [k for k in WANT if not k.endswith('workspace_bytes')]


def test_header_and_libraries_carry_the_head_training_entry_points():
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


def _plan(M, K, N):
    """(split, slabs per split) the rule of csrc/wgrad_kernel.h gives one workgroup per
    tile: 256 CUs / tiles splits, at least 8 slabs of 64 rows each, no empty split."""
    tile = 128 if K % 128 == 0 and N % 128 == 0 else 64
    tiles = (K // tile) * (N // tile)
    nsteps = (M + 63) // 64
    split = max(1, min(256 // tiles, nsteps // 8))
    sps = (nsteps + split - 1) // split
    return (nsteps + sps - 1) // sps, sps


def test_workspace_size_is_slabs_of_the_linear_weight_gradient():
    """split x N x K fp32, the split counts written out (and re-derived by ``_plan``, the
    rule restated here).  head_attn's first Linear, (67 584, 384, 384): 9 tiles of
    128 x 128, 256 // 9 = 28 splits of 38 slabs = 252 workgroups; its last Linear after the
    resize, (4 224, 384, 2304): 54 tiles, 4 splits = 216 workgroups."""
    wb = vit_ops.linear_wgrad_workspace_bytes
    for (M, K, N), split in [
            ((67584, 384, 384), 28),
            ((4224, 384, 2304), 4),
            ((120, 64, 64), 1),            # two slabs: one split below 16 slabs
            ((960, 64, 64), 1),            # 15 slabs; 16 is the first count with two splits
            ((961, 64, 64), 2),
            ((1100, 128, 128), 2),         # clamped by nsteps / 8 (18 slabs), wide tile
            ((70, 64, 128), 1),            # mixed widths: narrow tile
            ((4096, 1024, 2048), 2),       # 128 tiles: two splits fill the 256 CUs
            ((4096, 2048, 2048), 1),       # as many tiles as CUs
            ((4096, 2048, 4096), 1),       # more tiles than CUs
            ((44800, 64, 64), 78)]:        # 700 slabs: 256 -> 87 -> 9 per split, no empty split
        assert _plan(M, K, N)[0] == split, (M, K, N)
        assert wb(M, K, N) == split * N * K * 4, (M, K, N)
    for bad in [(70, 72, 64), (70, 64, 96), (70, 32, 64), (0, 64, 64), (-5, 64, 64),
                (70, 0, 64), (1 << 24, 64, 64),      # M * max(K, N) = 2^30: past the offsets
                (500000, 384, 2304)]:
        assert wb(*bad) == -1, bad
    assert wb((1 << 24) - 64, 64, 64) > 0
    lib = _lib.lib()
    assert lib.veon_layernorm_f32_bwd_workspace_bytes(384) % (2 * 384 * 4) == 0
    assert lib.veon_layernorm_f32_bwd_workspace_bytes(64) > 0
    assert lib.veon_layernorm_f32_bwd_workspace_bytes(72) == -1
    assert lib.veon_layernorm_f32_bwd_workspace_bytes(1088) == -1
    assert lib.veon_rows_colsum_workspace_bytes(2304) % (2304 * 4) == 0
    assert lib.veon_rows_colsum_workspace_bytes(12) == -1


def test_torch_references_equal_fp64_autograd():
    """``linear_wgrad_ref`` against autograd through F.linear, and
    ``conv3d_ops.ln_gelu_backward_ref`` against autograd through F.layer_norm, in fp64 to
    1e-12 / 1e-10."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 9, 24, generator=g, dtype=torch.float64)
    w = torch.randn(40, 24, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 9, 40, generator=g, dtype=torch.float64)
    F.linear(x, w).backward(dy)
    got = vit_ops.linear_wgrad_ref(dy, x)
    assert got.shape == w.shape
    assert ((got - w.grad).norm() / w.grad.norm()).item() <= 1e-12

    gamma = (torch.rand(24, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.zeros(24, dtype=torch.float64, requires_grad=True)
    xi = (x * 1.5 + 0.3).requires_grad_(True)
    dout = torch.randn(2, 9, 24, generator=g, dtype=torch.float64)
    F.layer_norm(xi, (24,), gamma, beta, 1e-5).backward(dout)
    dx, dg, db = conv3d_ops.ln_gelu_backward_ref(dout, xi.detach(), gamma.detach(), 1e-5)
    for p, q in ((dx, xi.grad), (dg, gamma.grad), (db, beta.grad)):
        assert ((p - q).norm() / q.norm()).item() <= 1e-10


def _switches(value):
    FeedForward.hip_train = value
    HighresSideAdaptorBlock.hip_train = value
    AttnManipulateBlock.hip_train = value


def _new_calls():
    return sum(_lib.CALLS.get(k, 0) for k in NEW)


def test_switches_are_off_by_default_and_cpu_and_eval_keep_the_torch_definition():
    """With the three switches on, a CPU module in training mode and an eval-mode module
    take today's code: identical results and gradients, no call of a new entry point."""
    assert FeedForward.hip_train is False
    assert HighresSideAdaptorBlock.hip_train is False
    assert AttnManipulateBlock.hip_train is False
    torch.manual_seed(4)
    ff = FeedForward(64, 64, 128).train()
    blk = HighresSideAdaptorBlock(64, mlp_dim=64, neck_dim=64, pre_norm=True, use_add=True)
    rear = AttnManipulateBlock(64, mlp_dim=64, clip_dim=64, heads=2, dim_head=16,
                               attn_layers=2, supp_dim=64, pre_norm=True)
    x = torch.randn(1, 12, 64)
    ext = torch.randn(1, 64, 2, 2)

    def run(switch, training):
        mods = [copy.deepcopy(m).train(training) for m in (ff, blk, rear)]
        xi = x.clone().requires_grad_(True)
        _switches(switch)
        try:
            assert not mods[0]._hip_train_ok(xi)
            with torch.set_grad_enabled(training):
                outs = [mods[0](xi), mods[0].forward_resized(xi, (3, 4), (2, 2)),
                        mods[1](xi, None, ext, None, ext, (3, 4))]
                outs += list(mods[2](xi, (3, 4), (2, 2))[1:])
            if training:
                sum(o.square().sum() for o in outs).backward()
        finally:
            _switches(False)
        grads = [xi.grad] + [p.grad for m in mods for p in m.parameters()]
        return [o.detach() for o in outs] + (grads if training else [])
    for training in (True, False):
        before = _new_calls()
        for p, q in zip(run(False, training), run(True, training)):
            assert torch.equal(p, q)
        assert _new_calls() == before
