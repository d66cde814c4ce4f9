"""Host-side checks of the training path of the fused lift + max-pool: the C ABI
additions, the neck's switch and the block-max helper (plain torch, CPU)."""
import ctypes

import numpy as np
import torch

from veon_amd import _lib, synthetic
from veon_amd.models import build_neck
from veon_amd.models.necks.lss_core import block_max

_I, _L, _P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p

# what the wrappers of veon_amd/ops/bev_pool_v2/bev_pool.py pass, stream last
WANT = {
    # c batch Z Y X dz dy dx | depth feat | feat_dtype | ranks_depth ranks_feat vstart out |
    # feat_elems | chunk_order winner | stream
    'veon_bev_pool_v2_fwd_rows_maxpool_winner':
        [_I] * 8 + [_P] * 2 + [_I] + [_P] * 4 + [_L] + [_P] * 2 + [_P],
    # n_points | table_len n_voxels | ranks_depth ranks_bev counts pvox | stream
    'veon_bev_pool_point_table': [_I] + [_L] * 2 + [_P] * 4 + [_P],
    # c n_images D HW batch Z Y X | pooled_grad winner pvox depth feat depth_grad feat_grad |
    # stream
    'veon_bev_pool_v2_bwd_rows_maxpool': [_I] * 8 + [_P] * 7 + [_P],
}


def test_header_and_library_carry_the_training_entry_points():
    from veon_amd import build
    build.build()
    declared = set(_lib.declared_symbols())
    for name, argtypes in WANT.items():
        assert name in declared, name
        restype, got = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int and got == argtypes, name
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        for name in WANT:
            assert hasattr(lib, name), (flavour, name)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2      # the additions are additive


def test_neck_switch_defaults_to_off():
    vt = build_neck(dict(type='LSSViewTransformerRaw', grid_config=synthetic.GRID_S2,
                         input_size=(256, 704), downsample=16, out_channels=8,
                         collapse_z=False, accelerate=False, ds_feat=[2, 2, 2]))
    assert vt.fuse_ds_grad is False
    assert vt.sync_free is False and vt.persistent_output is False


def _reference_block_max(vol, ds):
    """view_transformer_raw.py:549-553 without einops: blocks flattened in
    '(dz dh dw)' order, then torch.max(dim=-1).values."""
    dz, dh, dw = ds
    b, c, z, h, w = vol.shape
    x = vol.view(b, c, z // dz, dz, h // dh, dh, w // dw, dw)
    x = x.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(b, c, z // dz, h // dh, w // dw, -1)
    return torch.max(x, dim=-1).values


def _tie_volume():
    rng = np.random.default_rng(3)
    vol = rng.standard_normal((2, 3, 4, 6, 8))
    vol = np.maximum(vol, 0.0)                       # ReLU: zeros tie inside blocks
    vol[:, :, 0:2, 0:2, 0:2] = 0.0                   # an all-zero block
    vol[:, :, 0:2, 2:4, 0:2] = -1.0 - rng.random((2, 3, 2, 2, 2))   # all negative
    vol[:, :, 2:4, 0:2, 2:4] = 2.5                   # eight equal maxima
    vol[0, 0, 2, 4, 6] = vol[0, 0, 3, 5, 7] = 9.0    # two equal maxima, first and last
    vol[:, 1, 0:2, 4:6, 4:6] = -3.0                  # negative and all equal
    return torch.from_numpy(vol)


def test_block_max_first_max_is_the_reference_gradient():
    ds = (2, 2, 2)
    base = _tie_volume()
    w = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 3, 2, 3, 4)))
    grads, outs = {}, {}
    for key, fn in (('first', lambda v: block_max(v, ds, first_max=True)),
                    ('amax', lambda v: block_max(v, ds, first_max=False)),
                    ('default', lambda v: block_max(v, ds)),
                    ('reference', lambda v: _reference_block_max(v, ds)),
                    ('today', lambda v: v.view(2, 3, 2, 2, 3, 2, 4, 2).amax(dim=(3, 5, 7)))):
        v = base.clone().requires_grad_()
        out = fn(v)
        (out * w).sum().backward()
        outs[key], grads[key] = out.detach(), v.grad
    for key in outs:                                  # one forward, bit for bit
        assert torch.equal(outs[key], outs['today']), key
    assert torch.equal(grads['first'], grads['reference'])
    assert torch.equal(grads['amax'], grads['today'])
    assert torch.equal(grads['default'], grads['today'])
    # the case has ties: the two gradients differ
    assert not torch.equal(grads['first'], grads['amax'])
    # first-max: exactly one element of every block carries the gradient, the first
    g = grads['first'].view(2, 3, 2, 2, 3, 2, 4, 2).permute(0, 1, 2, 4, 6, 3, 5, 7) \
        .reshape(2, 3, 2, 3, 4, 8)
    assert ((g != 0).sum(-1) == 1).all()
    assert torch.equal(g.sum(-1), w)
    assert (g[:, :, 0, 0, 0, 0] == w[:, :, 0, 0, 0]).all()      # all-zero block: child 0
    assert (g[:, :, 1, 0, 1, 0] == w[:, :, 1, 0, 1]).all()      # eight equal: child 0
    assert g[0, 0, 1, 2, 3, 0] == w[0, 0, 1, 2, 3]              # 9.0 twice: the first
    # amax splits: the all-zero block gets an eighth everywhere
    a = grads['amax'].view(2, 3, 2, 2, 3, 2, 4, 2).permute(0, 1, 2, 4, 6, 3, 5, 7) \
        .reshape(2, 3, 2, 3, 4, 8)
    assert torch.allclose(a[:, :, 0, 0, 0], (w[:, :, 0, 0, 0] / 8).unsqueeze(-1).expand(2, 3, 8))


def test_cpu_torch_max_takes_the_first_of_equal_maxima():
    """The GPU tests take their expected winners from CPU torch.max(dim=-1): pin the
    tie rule they rely on against numpy's documented first-occurrence argmax."""
    rng = np.random.default_rng(5)
    x = rng.integers(-2, 3, size=(5000, 8)).astype(np.float32)
    x[::7] = 0.0
    x[1::7, 3] = -0.0
    idx = torch.max(torch.from_numpy(x), dim=-1).indices.numpy()
    assert np.array_equal(idx, np.argmax(x, axis=-1))
