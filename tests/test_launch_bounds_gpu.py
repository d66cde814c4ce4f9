"""Every native entry point between canary bands (tests/launch_guard.py).

One table of rows.  A row names an existing GPU test (module, function, arguments: its
smallest case and its smallest ragged one, each forced kernel variant once) or a small
local body, and the entry points it must launch.  The parametrised test runs the row
inside ``guarded()``: every tensor argument of every launch sits in exact-size memory
between two 4 KiB bands of 0xFF, so a store past an output or a workspace, a write
through a const pointer or a NaN / -1 read from beyond an input fails here, and the
reused test's own reference comparison runs on what the relocated launch computed.

The wrappers size their workspaces with the header's size functions and not a byte more
(``EXACT_SIZE`` names the row that runs each of them at exactly that size), so a size
function that promises too little shows as a touched band.

``veon_optim_update`` reaches parameters and EMA weights through its device record table
and ``veon_vit_block`` its weights through a host struct; the guard cannot move those, so
the two ``Arena`` tests at the end carve them out of canary memory.

tests/test_launch_guard.py (CPU) keeps the ledger: every stream-taking prototype of the
header is in a row here, in ``ARENA_DIRECT`` or in ``EXEMPT``.
"""
import copy
import functools
import importlib
import inspect

import pytest
import torch
from torch import nn

from tests.launch_guard import guarded
from veon_amd import _lib, half, optim, vit_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

V, C3, HM = 'tests.test_vit_ops_gpu', 'tests.test_conv3d_gpu', 'tests.test_half_mode_gpu'


class Row:
    def __init__(self, id, target, kwargs=None, entries=(), flavour='bf16'):
        self.id, self.target, self.kwargs = id, target, kwargs or {}
        self.entries, self.flavour = frozenset(entries), flavour


def _row(module, function, kwargs, entries, flavour='bf16', tag=None):
    if tag is None:
        tag = '-'.join(str(v).replace(' ', '') for v in kwargs.values()) \
            if isinstance(kwargs, dict) else ''
    rid = '%s.%s[%s]%s' % (module.rpartition('test_')[2], function.partition('test_')[2], tag,
                           '' if flavour == 'bf16' else '-fp16')
    return Row(rid, (module, function), kwargs, entries, flavour)


# ------------------------------------------------------------------ local bodies
def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _splitk(M, N, K, tile):
    """The split-K GEMM at the smallest ragged shape that takes ``tile`` (0: 192 x 192,
    1: 192 x 256), its slab exactly ``veon_vit_gemm_splitk_plan`` bytes: against the fp32
    product at the bound of test_vit_ops_gpu.test_gemm_splitk_residual."""
    import ctypes
    got_tile = ctypes.c_int(-1)
    need = _lib.lib().veon_vit_gemm_splitk_plan(M, N, K, ctypes.byref(got_tile))
    assert need > 0 and got_tile.value == tile
    a = _rand(M, K, seed=31).to(half.dtype())
    w = (_rand(N, K, seed=32) * K ** -0.5).to(half.dtype())
    bias, gamma, x = _rand(N, seed=33), _rand(N, seed=34) * 0.1, _rand(M, N, seed=35)
    slab = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    sync = torch.zeros(1024, dtype=torch.int32, device=DEV)
    got = vit_ops.linear_residual_splitk_(x.clone(), a, w, bias, gamma, (slab, sync))
    assert int(sync.abs().sum()) == 0
    ref = x + gamma * (a.float() @ w.float().t() + bias)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def _attention_bwd_exact(B, T, H, biased):
    """attention_bwd / attention_bias_bwd with ``workspace`` of exactly
    ``veon_vit_attention_bwd_workspace_bytes`` and ``lse`` of exactly
    ``veon_vit_attention_stats_len`` floats per row, under the guard: the same bits as the
    wrapper's own allocation gives outside it (the kernels use no atomics)."""
    dt, scale = half.dtype(), 0.125
    qkv = _rand(B, T, 3 * H * 64, seed=T).to(dt)
    dout = _rand(B, T, H * 64, seed=T + 1).to(dt)
    nbytes = int(_lib.lib().veon_vit_attention_bwd_workspace_bytes(B, T, H))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lse = torch.empty(B, H, vit_ops.attention_stats_len(T), dtype=torch.float32, device=DEV)
    if biased:
        bias = _rand(B, H, T - 1, T - 1, seed=T + 2)
        out, lse = vit_ops.attention_bias_fwd_lse(qkv, bias, H, scale, border=1, lse=lse)
        got = vit_ops.attention_bias_bwd(qkv, bias, out, dout, lse, H, scale, border=1,
                                         workspace=ws)
    else:
        out, lse = vit_ops.attention_fwd_lse(qkv, H, scale, lse=lse)
        got = (vit_ops.attention_bwd(qkv, out, dout, lse, H, scale, workspace=ws),)
    real, _lib.launch = _lib.launch, _lib.launch.__wrapped__       # the same, unguarded
    try:
        if biased:
            out2, lse2 = vit_ops.attention_bias_fwd_lse(qkv, bias, H, scale, border=1)
            want = vit_ops.attention_bias_bwd(qkv, bias, out2, dout, lse2, H, scale, border=1)
        else:
            out2, lse2 = vit_ops.attention_fwd_lse(qkv, H, scale)
            want = (vit_ops.attention_bwd(qkv, out2, dout, lse2, H, scale),)
    finally:
        _lib.launch = real
    assert torch.equal(out, out2) and torch.equal(lse[..., :T], lse2[..., :T])
    for g, w in zip(got, want):
        assert bool(torch.isfinite(g.float()).all()) and torch.equal(g, w)


def _image_dot(B, C, Y, X):
    """conv3d_ops.image_dot (1x1 conv C -> 1 of a padded image, fp32 accumulation) against
    fp64 on the same half operands.  Bound: a C-term fp32 dot product with a bias is off
    by at most (C + 2) 2^-24 (sum |x||w| + |bias|); relu is 1-Lipschitz and sigmoid
    1/4-Lipschitz, the sigmoid's own evaluation adds a few fp32 roundings of a value
    below 1 (8 x 2^-24 allowed)."""
    from veon_amd import conv3d_ops
    u = 2.0 ** -24
    x = _rand(B, C, Y, X, seed=C + X).to(half.dtype())
    w, bias = _rand(C, seed=C + 1) * C ** -0.5, 0.3
    img = conv3d_ops.pack_image(x.float())
    assert img.shape == (B, C, Y, X)
    dot = (x.double() * w.double().view(1, C, 1, 1)).sum(1, keepdim=True) + bias
    bound = (C + 2) * u * ((x.double().abs() * w.double().abs().view(1, C, 1, 1)).sum(
        1, keepdim=True) + abs(bias))
    for act, ref, extra in (('none', dot, 0.0), ('relu', dot.clamp_min(0), 0.0),
                            ('sigmoid', torch.sigmoid(dot), 8 * u)):
        got = conv3d_ops.image_dot(img, w, bias, act)
        assert got.shape == (B, 1, Y, X) and got.dtype == torch.float32
        assert bool(((got.double() - ref).abs() <= bound + extra).all()), act


def _volume_maxpool2(B, C, Z, Y, X):
    """veon_volume_maxpool2_f32 as VeonOccupancyPath._max_pool launches it, against
    view + amax bit for bit, NaN and -inf included (test_handover_gpu launches it past
    ``_lib.launch``, where the guard cannot see it)."""
    g = torch.Generator().manual_seed(5)
    vol = torch.randn(B, C, Z, Y, X, generator=g).to(DEV)
    vol[0, 0, 0, 0, 1] = float('nan')
    vol[0, -1, -1, -1, -1] = float('-inf')
    out = torch.empty(B, C, Z // 2, Y // 2, X // 2, device=DEV)
    _lib.launch('veon_volume_maxpool2_f32', vol.device, vol, out, B * C, Z, Y, X)
    want = vol.view(B, C, Z // 2, 2, Y // 2, 2, X // 2, 2).amax(dim=(3, 5, 7))
    assert torch.equal(torch.nan_to_num(out, nan=12345.0), torch.nan_to_num(want, nan=12345.0))
    assert bool(torch.isnan(out[0, 0, 0, 0, 0]))


def _lift_slab_family(C):
    """The slab pool kernels no wrapper launches any more (kept in the ABI for the
    reference's call sequence and the probes) and the padded max-pool below the row
    kernel's channel count, on a 20 x 20 x 4 grid, plan and row table at exactly
    veon_bev_pool_plan_ints / 2 (B Z Y + 1) ints.  The header's own statements are the
    references: fused == the scatter kernel into a zeroed volume, bit for bit; strided ==
    fused with the padding between the planes untouched; maxpool == the block max of
    fused; padded == maxpool rounded to half, halo zero."""
    from tests.helpers import halo_is_zero
    from tools._inputs import lift_case
    from veon_amd import conv3d_ops
    from veon_amd.ops.bev_pool_v2 import bev_pool as bp
    grid = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
            'depth': [1.0, 13.0, 1.0]}
    dev = torch.device(DEV)
    case = lift_case(grid, (64, 176), 2, C, DEV)
    depth, feat = case['depth'], case['feat_nhwc']
    rb, rd, rf, st, ln = (case[k] for k in ('rb', 'rd', 'rf', 'st', 'ln'))
    X, Y, Z = case['gsize']
    vpb, n = X * Y * Z, st.numel()
    bp.mark_sorted(st, int(rb[0]), int(rb[-1]))
    plan = bp.build_plan(rb, st, 1, vpb)
    assert plan.numel() == _lib.lib().veon_bev_pool_plan_ints(1, vpb)
    scatter = torch.zeros(vpb, C, device=DEV)
    _lib.launch('veon_bev_pool_v2_fwd', dev, C, n, depth, feat, rd, rf, rb, st, ln, scatter)
    want = scatter.t().contiguous()
    assert float(want.abs().sum()) > 0
    fused = torch.full((C, vpb), float('nan'), device=DEV)
    _lib.launch('veon_bev_pool_v2_fwd_fused', dev, C, n, 1, vpb, depth, feat, rd, rf, rb, st,
                ln, plan, fused, _lib.LAYOUT_BCZYX)
    assert torch.equal(fused, want)
    pad = 192
    strided = torch.full((C, vpb + pad), -7.0, device=DEV)
    _lib.launch('veon_bev_pool_v2_fwd_fused_strided', dev, C, n, 1, vpb, depth, feat,
                _lib.FEAT_F32, rd, rf, rb, st, ln, plan, strided, vpb + pad)
    assert torch.equal(strided[:, :vpb], want) and bool((strided[:, vpb:] == -7.0).all())
    rows = bp.build_row_table(rb, st, 1, vpb, X, attach=False)
    assert rows.numel() == 2 * (Z * Y + 1)
    pooled = torch.full((1, C, Z // 2, Y // 2, X // 2), float('nan'), device=DEV)
    _lib.launch('veon_bev_pool_v2_fwd_maxpool', dev, C, n, 1, Z, Y, X, 2, 2, 2, depth, feat,
                rd, rf, rb, st, ln, rows, pooled)
    assert torch.equal(pooled[0], want.view(C, Z // 2, 2, Y // 2, 2, X // 2, 2).amax((2, 4, 6)))
    vol = conv3d_ops.PaddedVolume(1, C, Z // 2, Y // 2, X // 2, dev)
    bp.bev_pool_v2_maxpool(depth, feat, rd, rf, rb, (1, Z, Y, X, C), st, ln, (2, 2, 2),
                           out_volume=vol)
    assert torch.equal(vol.interior().permute(0, 4, 1, 2, 3), pooled.to(half.dtype()))
    assert halo_is_zero(vol)


def _layernorm_padded(T, d, ld):
    """vit_ops.layernorm_padded (the side adapter's: LayerNorm over the first d of ld
    columns, zeros behind them; the padding of x is NaN and must not be read into the
    statistics) against F.layer_norm at the bound of test_vit_ops_gpu.test_layernorm."""
    from tests.helpers import half_tol
    x = torch.full((T, ld), float('nan'), device=DEV)
    x[:, :d] = _rand(T, d, seed=2, scale=3.0) + 0.5
    w, b = _rand(d, seed=3) * 0.1 + 1.0, _rand(d, seed=4) * 0.1
    got = vit_ops.layernorm_padded(x, w, b, d, eps=1e-6)
    assert got.dtype == half.dtype() and got.shape == (T, ld)
    ref = torch.nn.functional.layer_norm(x[:, :d], (d,), w, b, 1e-6)
    torch.testing.assert_close(got[:, :d].float(), ref, **half_tol(2 ** -8, 2e-3))
    assert float(got[:, d:].float().abs().sum()) == 0.0


# ------------------------------------------------------------------------ the table
GEMM = {'veon_vit_gemm'}
ATT = {'veon_vit_attention'}
ATT2 = {'veon_vit_attention_log2'}
T2, T3 = 'tests.test_hsa_train_gpu', 'tests.test_body_train_gpu'
TH, TV, TC = 'tests.test_hsa_heads_train_gpu', 'tests.test_vit_train_gpu', \
    'tests.test_clip_tail_train_gpu'
BN = {'veon_bn3d_sums_bf16', 'veon_bn3d_bwd_sums_bf16', 'veon_bn3d_apply_bf16',
      'veon_bn3d_bwd_apply_bf16'}
OPT = {'veon_optim_sumsq', 'veon_optim_clip_finish', 'veon_optim_update'}

ROWS = [
    # ---- ViT block kernels
    _row(V, 'test_cast_bf16_round_to_nearest_even', {}, {'veon_vit_cast_bf16'}),
    _row(V, 'test_layernorm', dict(T=3, d=100), {'veon_vit_layernorm'}),
    _row(V, 'test_gemm_bias_bf16', dict(M=1, N=4, K=64), GEMM),
    _row(V, 'test_gemm_bias_bf16', dict(M=64, N=128, K=64), GEMM),
    *[_row(V, 'test_gemm_every_big_tile_configuration', dict(cfg=c, M=257, N=520, K=64), GEMM)
      for c in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14)],
    *[_row(V, 'test_gemm_every_small_tile_instantiation', dict(tile=t, M=97, N=132, K=64), GEMM)
      for t in ((4, 2, 1), (4, 2, 2), (4, 4, 1), (4, 4, 2), (8, 2, 1))],
    _row(V, 'test_gemm_every_small_tile_instantiation', dict(tile=(4, 2, 1), M=1, N=4, K=64),
         GEMM),
    _row(V, 'test_gemm_every_small_tile_instantiation', dict(tile=(4, 4, 2), M=97, N=132, K=64),
         GEMM, 'fp16'),
    _row(V, 'test_gemm_every_big_tile_configuration', dict(cfg=8, M=257, N=520, K=64), GEMM,
         'fp16'),
    _row(V, 'test_gemm_layerscale_residual_inplace', {}, GEMM),
    Row('splitk[1025x2500x2048-tile0]', functools.partial(_splitk, 1025, 2500, 2048, 0),
        entries={'veon_vit_gemm_splitk'}),
    Row('splitk[1025x4036x2048-tile1]', functools.partial(_splitk, 1025, 4036, 2048, 1),
        entries={'veon_vit_gemm_splitk'}),
    *[_row(V, 'test_attention', dict(B=B, T=T, H=H, q_log2=q), ATT2 if q else ATT)
      for B, T, H in ((1, 65, 2), (3, 17, 3)) for q in (False, True)],
    _row(V, 'test_attention', dict(B=3, T=17, H=3, q_log2=False), ATT, 'fp16'),
    *[_row(V, 'test_attention_with_bias_and_masking', dict(q_log2=q), ATT2 if q else ATT)
      for q in (False, True)],
    *[_row(V, 'test_whole_block_call_equals_the_seven_ops',
           dict(act=a, with_gamma=g, with_bias=b, q_log2=q), {'veon_vit_block'})
      for a, g, b, q in ((vit_ops.EPI_GELU, True, False, True),
                         (vit_ops.EPI_QUICKGELU, False, True, False))],
    Row('layernorm_padded[3x48in64]', functools.partial(_layernorm_padded, 3, 48, 64),
        entries={'veon_vit_layernorm_padded'}),
    Row('layernorm_padded[5x100in128]', functools.partial(_layernorm_padded, 5, 100, 128),
        entries={'veon_vit_layernorm_padded'}),
    _row(V, 'test_layernorm_f32_add_nearest_is_the_torch_sequence',
         dict(B=1, L=38, d=128, YX=(5, 7), hw=(3, 3)), {'veon_layernorm_f32_add_nearest'}),
    _row(V, 'test_layernorm_f32_matches_torch', dict(T=7, d=128), {'veon_layernorm_f32'}),
    # ---- hand-over kernels
    _row('tests.test_handover_gpu', 'test_patchify_rows_are_the_conv_operand',
         dict(B=2, C=3, H=30, W=45, p=14, skip=1), {'veon_vit_patchify'}),
    *[_row('tests.test_handover_gpu', 'test_tokens_to_image_is_the_transposed_conv_pixel_shuffle',
           dict(s=s), {'veon_tokens_to_image'}) for s in (1, 2)],
    _row('tests.test_handover_gpu', 'test_image_subsample', dict(Y=7, X=5, step=2),
         {'veon_image_subsample'}),
    Row('volume_maxpool2[1x7x4x6x10]', functools.partial(_volume_maxpool2, 1, 7, 4, 6, 10),
        entries={'veon_volume_maxpool2_f32'}),
    Row('volume_maxpool2[2x3x2x2x34]', functools.partial(_volume_maxpool2, 2, 3, 2, 2, 34),
        entries={'veon_volume_maxpool2_f32'}),
    _row('tests.test_handover_gpu', 'test_sensor2keyego_kernel_equals_the_reference_algebra', {},
         {'veon_sensor2keyego'}),
    # ---- conv3d / conv2d forward on padded grids
    _row(C3, 'test_pack_unpack_round_trip_and_halo', {},
         {'veon_volume_pack_bf16', 'veon_volume_unpack_f32'}),
    _row(C3, 'test_conv3d_matches_torch', dict(B=1, Cin=64, Cout=136, Z=1, Y=1, X=1, mode='plain'),
         {'veon_conv3d_k3_bf16'}),
    _row(C3, 'test_conv3d_matches_torch',
         dict(B=1, Cin=64, Cout=64, Z=3, Y=5, X=7, mode='bn_resid_relu'), {'veon_conv3d_k3_bf16'}),
    _row(C3, 'test_conv3d_matches_torch',
         dict(B=1, Cin=64, Cout=64, Z=3, Y=5, X=7, mode='bn_relu'), {'veon_conv3d_k3_bf16'},
         'fp16'),
    *[_row(C3, 'test_conv2d_matches_torch',
           dict(B=1, Cin=64, Cout=64, Y=5, X=7, mode=m, dtype=d),
           {'veon_conv2d_k3_bf16', 'veon_image_pack_bf16', 'veon_image_unpack'})
      for m, d in (('bias_resid', torch.float32), ('bias_relu', torch.bfloat16))],
    _row(C3, 'test_conv2d_second_residual_and_relu_output', dict(B=1, C=64, Y=5, X=7),
         {'veon_conv2d_k3_bf16_ex'}),
    _row(C3, 'test_conv2d_stride2_matches_torch', dict(shape=(2, 64, 8, 5, 4)),
         {'veon_conv2d_k3s2_bf16'}),
    _row(C3, 'test_conv2d_stride2_matches_torch', dict(shape=(2, 64, 64, 9, 13)),
         {'veon_conv2d_k3s2_bf16'}),
    *[_row(C3, 'test_resize_bilinear_matches_interpolate', dict(size_in=i, size_out=o),
           {'veon_image_resize_bilinear'}) for i, o in (((4, 6), (8, 12)), ((5, 5), (1, 1)))],
    *[_row(C3, 'test_image_layernorm_matches_torch', dict(C=c, Y=y, X=x),
           {'veon_image_layernorm_bf16'}) for c, y, x in ((64, 3, 4), (520, 4, 4))],
    _row(C3, 'test_layernorm_tokens_to_padded_image_and_convblock_fusions', {},
         {'veon_layernorm_f32_to_padded'}),
    Row('image_dot[1x64x3x5]', functools.partial(_image_dot, 1, 64, 3, 5),
        entries={'veon_image_dot'}),
    Row('image_dot[2x32x5x7]', functools.partial(_image_dot, 2, 32, 5, 7),
        entries={'veon_image_dot'}),
    *[_row(C3, 'test_conv_every_tile_against_fp64', dict(tile=t, kernel=k),
           {'veon_conv3d_k3_bf16', 'veon_conv2d_k3_bf16'} |
           ({'veon_conv2d_k3s2_bf16'} if k == 'general' else set()))
      for t in ((3, 4, 7), (4, 4, 3), (4, 4, 4), (4, 2, 1), (4, 2, 2), (4, 2, 3), (4, 2, 4),
                (4, 3, 2), (4, 3, 3), (8, 1, 1), (8, 1, 2), (8, 1, 3), (8, 1, 4))
      for k in ('slab', 'general')],
    # ---- temporal fusion
    *[_row('tests.test_temporal_gpu', 'test_deform_attention_matches_torch',
           dict(B=B, C=C, heads=h, Z=Z, Y=Y, X=X), {'veon_deform_attention_bf16'})
      for B, C, h, Z, Y, X in ((1, 256, 4, 1, 1, 1), (1, 128, 4, 2, 5, 7), (1, 32, 1, 3, 4, 5))],
    _row('tests.test_temporal_gpu', 'test_warp_matches_align_after_lss', dict(shift=0.3),
         {'veon_volume_warp_bf16'}),
    _row('tests.test_temporal_gpu', 'test_zero_halo', {}, {'veon_volume_zero_halo_bf16'}),
    _row('tests.test_temporal_edges_gpu', 'test_warp_affine_matches_float64_algebra',
         lambda m: dict(gname=sorted(m.GRIDS)[0], family='rot3d', B=3), {'veon_warp_affine'},
         tag='rot3d-B3'),
    *[_row('tests.test_temporal_train_gpu', 'test_backward_holds_the_fp32_yardstick',
           dict(cid=c), {'veon_deform_attention_bwd_bf16', 'veon_deform_attention_bwd_dkv_bf16'})
      for c in ('layout-B1-hd32-h1-3x5x7', 'layout-B2-hd64-h4-2x4x4', 'len1-B2-hd32-h4-3x5x1')],
    # ---- training: weight gradients, BN and LN passes
    *[_row(T3, 'test_wgrad_against_fp64', dict(zip(('B', 'Cin', 'Cout', 'Z', 'Y', 'X'), s)),
           {'veon_conv3d_k3_wgrad_bf16'})
      for s in ((2, 64, 64, 4, 10, 12), (2, 64, 128, 3, 7, 5), (2, 128, 64, 3, 7, 5))],
    *[_row(T3, 'test_bn_passes_against_fp64', dict(zip(('B', 'C', 'Z', 'Y', 'X'), s)), BN)
      for s in ((1, 8, 2, 3, 4), (1, 72, 2, 3, 4), (2, 128, 3, 7, 5))],
    *[_row(T2, 'test_wgrad2d_against_fp64', dict(zip(('B', 'Cin', 'Cout', 'Y', 'X'), s)),
           {'veon_conv2d_k3_wgrad_bf16'})
      for s in ((2, 64, 64, 10, 12), (2, 64, 128, 7, 5), (2, 128, 64, 7, 5), (1, 128, 128, 3, 70))],
    *[_row(T2, 'test_ln_passes_against_fp64', dict(zip(('B', 'C', 'Y', 'X'), s)),
           {'veon_image_gelu_layernorm_bf16', 'veon_image_layernorm_bwd_bf16'})
      for s in ((1, 8, 3, 3), (1, 72, 3, 5), (1, 520, 3, 4))],
    *[_row(TH, 'test_linear_wgrad_against_fp64', dict(M=M, K=K, N=N), {'veon_linear_wgrad_bf16'})
      for M, K, N in ((120, 64, 64), (70, 64, 128), (70, 128, 64), (1100, 128, 128))],
    _row(TH, 'test_linear_wgrad_against_fp64', dict(M=70, K=64, N=128),
         {'veon_linear_wgrad_bf16'}, 'fp16'),
    *[_row(TH, 'test_row_passes_against_fp64', dict(T=T, d=d),
           {'veon_rows_colsum_bf16', 'veon_gelu_bf16', 'veon_gelu_bwd_bf16',
            'veon_layernorm_f32_bwd'}) for T, d in ((70, 128), (13, 576))],
    *[_row('tests.test_wgrad_seams_gpu', 'test_seams_against_fp64', dict(kind=k, shape=s),
           {'veon_%s_wgrad_bf16' % ('linear' if k == 'linear' else k + '_k3')})
      for k, s in (('linear', (1, 64, 64)), ('linear', (65, 64, 64)))],
    *[_row('tests.test_sync_bn_gpu', f, lambda m, kw=kw: dict(shape=m.rs.shapes_of('bn')[0],
                                                               fill=m.FILLS[0], **kw),
           e, tag='first')
      for f, kw, e in (('test_forward_stats_on_integers_are_exact', {},
                        {'veon_bn3d_sums_stats_bf16'}),
                       ('test_backward_stats_on_integers_are_exact', {'mask': 'masked'},
                        {'veon_bn3d_bwd_sums_stats_bf16'}))],
    _row('tests.test_sync_bn_gpu', 'test_rank_split_on_integers_is_bit_equal',
         dict(shape=(3, 128, 2, 4, 4)), {'veon_bn_train_coeffs', 'veon_bn_bwd_coeffs'}),
    _row('tests.test_sync_bn_gpu', 'test_gaussian_rank_split_against_the_fp64_mirror',
         dict(shape=(3, 64, 3, 5, 6), momentum=0.1, offset=True),
         {'veon_bn_train_coeffs', 'veon_bn_bwd_coeffs'}),
    # ---- attention for training
    *[_row(TV, 'test_forward_is_the_inference_kernel_and_lse_matches_fp64', dict(B=B, T=T, H=H),
           {'veon_vit_attention_fwd_lse'}) for B, T, H in ((1, 1, 1), (2, 65, 3))],
    *[_row(TV, 'test_backward_against_fp64', dict(B=B, T=T, H=H), {'veon_vit_attention_bwd'})
      for B, T, H in ((1, 1, 1), (2, 65, 3))],
    _row(TV, 'test_backward_against_fp64', dict(B=2, T=65, H=3), {'veon_vit_attention_bwd'},
         'fp16'),
    *[_row(TC, 'test_forward_against_fp64_and_the_unbiased_kernel', dict(B=B, T=T, H=H, border=b),
           {'veon_vit_attention_bias_fwd_lse'}) for B, T, H, b in ((1, 1, 1, 0), (2, 33, 2, 1))],
    *[_row(TC, 'test_backward_against_fp64', dict(B=B, T=T, H=H, border=b),
           {'veon_vit_attention_bias_bwd'}) for B, T, H, b in ((1, 2, 1, 1), (2, 66, 3, 1))],
    _row(TC, 'test_quickgelu_pair_against_fp64', {},
         {'veon_quickgelu_bf16', 'veon_quickgelu_bwd_bf16'}),
    Row('attention_bwd_exact[2x65x3]', functools.partial(_attention_bwd_exact, 2, 65, 3, False),
        entries={'veon_vit_attention_fwd_lse', 'veon_vit_attention_bwd'}),
    Row('attention_bias_bwd_exact[2x66x3]', functools.partial(_attention_bwd_exact, 2, 66, 3, True),
        entries={'veon_vit_attention_bias_fwd_lse', 'veon_vit_attention_bias_bwd'}),
    # ---- occupancy tails, evaluation, retrieval, 2-D maps
    _row('tests.test_occ_head_gpu', 'test_fused_tail_matches_the_op_sequence',
         dict(B=2, Q=5, low=(3, 7, 5), size=(6, 14, 10)), {'veon_occ_classify'}),
    _row('tests.test_occ_head_gpu', 'test_strided_inputs_are_read_in_place', {},
         {'veon_occ_classify'}),
    _row('tests.test_occ_eval_gpu', 'test_labels_equal_occ_classify_bit_for_bit',
         dict(name='small'), {'veon_occ_labels'}),
    _row('tests.test_occ_eval_gpu', 'test_fused_histogram_confusion_and_bincount_agree',
         dict(name='small'), {'veon_occ_labels', 'veon_occ_confusion'}),
    _row('tests.test_occ_eval_gpu', 'test_confusion_sizes', dict(n=257), {'veon_occ_confusion'}),
    *[_row('tests.test_occ_grouped_gpu', 'test_labels_and_merged_logits_equal_the_ungrouped_tail',
           dict(grid=g, K=5, layout=lay, bg_first=bg),
           {'veon_occ_labels_grouped', 'veon_occ_classify_grouped'})
      for g, lay, bg in (('x2', 'vec4', False), ('odd', 'scalar', True))],
    *[_row('tests.test_occ_fscore_gpu', 'test_tile_and_sample_seams', dict(X=X),
           {'veon_occ_fscore_counts'}) for X in (1, 17)],
    *[_row('tests.test_retrieval_gpu', 'test_kernel_odd_shapes',
           dict(low=(3, 7, 5), occ=(6, 14, 10), C=C, cv=cv), {'veon_occ_retrieve'})
      for C, cv in ((24, None), (20, 24))],
    *[_row('tests.test_align_loss_gpu', 'test_odd_shapes',
           dict(low=(3, 7, 5), occ=(6, 14, 10), C=C),
           {'veon_occ_align_fwd', 'veon_occ_align_bwd'}) for C in (24, 130)],
    *[_row('tests.test_align_select_gpu', f, {},
           {'veon_align_select_mark', 'veon_align_select_classify', 'veon_align_select_emit'})
      for f in ('test_seam_partial_last_workgroup', 'test_batch_of_two')],
    *[_row('tests.test_sem2d_gpu', 'test_maps_against_fp64', dict(name=n),
           {'veon_sem2d_ds', 'veon_sem2d_full'})
      for n in ('one_class_fractional_scale', 'fixture')],
    *[_row('tests.test_sem2d_gpu', 'test_labels_are_the_argmax_of_the_native_map',
           dict(name='fixture', grouped=g), {'veon_sem2d_labels'}) for g in (False, True)],
    # ---- losses, fusion, inputs, LiDAR render, optimiser
    _row('tests.test_depth_loss_gpu', 'test_shapes_and_depth_grids',
         dict(shape=(1, 1, 16, 48), bins=65, clipped=False),
         {'veon_depth_loss_rows', 'veon_depth_loss_reduce', 'veon_depth_loss_bwd'}),
    *[_row('tests.test_occ_bin_loss_gpu', 'test_matches_fp64_torch', dict(B=B, low=low, layout=lay),
           {'veon_occ_bin_loss_fwd', 'veon_occ_bin_loss_bwd'})
      for B, low, lay in ((1, (1, 1, 1), 'contiguous'), (2, (3, 5, 4), 'two_of_eight'),
                          (2, (1, 2, 3), 'channels_last'))],
    _row('tests.test_fusion_train_gpu', 'test_resize_cat_against_fp64_on_the_fp32_tables',
         dict(case=0, width=0), {'veon_fusion_resize_cat'}),
    _row('tests.test_fusion_train_gpu', 'test_dual_layernorm_within_a_half_neighbour_of_fp64',
         dict(width=0), {'veon_fusion_dual_ln'}),
    _row('tests.test_fusion_train_gpu',
         'test_backward_against_fp64_with_torch_fp32_as_the_yardstick', dict(case=0, width=0),
         {'veon_fusion_dual_ln_bwd', 'veon_fusion_resize_adjoint'}),
    _row('tests.test_fusion_train_gpu', 'test_join_and_split_are_exact', {},
         {'veon_fusion_join', 'veon_fusion_relu_split'}),
    _row('tests.test_image_inputs_gpu', 'test_prefilled_outputs_come_back_written', {},
         {'veon_image_resample_h', 'veon_image_resample_v_finish'}),
    _row('tests.test_image_inputs_gpu', 'test_depthanything_tail_within_bound', {},
         {'veon_image_cubic_norm'}),
    _row('tests.test_image_inputs_gpu', 'test_aligned_windows_take_both_kernels_to_the_same_bytes',
         {}, {'veon_image_resample_h', 'veon_image_resample_v_finish'}),
    *[_row('tests.test_lidar_depth_gpu', 'test_point_counts', dict(n=n),
           {'veon_lidar_depth_render'}) for n in (1, 65)],
    _row('tests.test_lidar_depth_gpu', 'test_batch_stride_and_downsample', {},
         {'veon_lidar_depth_render'}),
    _row('tests.test_optim_step_gpu', 'test_three_steps_equal_the_mirror_bit_for_bit',
         lambda m: dict(sizes=m.SEAMS), OPT, tag='seams'),
    _row('tests.test_head_train_gpu', 'test_unpack_cl_is_the_interior', dict(C=2, Cp=8),
         {'veon_volume_unpack_cl_f32'}),
    _row('tests.test_head_train_gpu', 'test_sigm_bwd_pack_cl_against_fp64',
         dict(layout='voxel_cosine'), {'veon_volume_sigm_bwd_pack_cl'}),
    # ---- the lift beyond what the arena modules launch directly
    _row('tests.test_bev_pool_gpu', 'test_kat_forward_backward_through_op', {},
         {'veon_bev_pool_v2_bwd'}),
    _row('tests.test_bev_pool_gpu', 'test_scatter_and_fused_bit_exact_small',
         dict(name='lss_small_b2'), {'veon_bev_pool_v2_fwd'}),
    _row('tests.test_bev_pool_gpu', 'test_odd_channel_counts_and_ragged_tiles', dict(C=3),
         {'veon_bev_pool_v2_fwd'}),
    *[Row('lift_slab_family[C%d]' % c, functools.partial(_lift_slab_family, c),
          entries={'veon_bev_pool_v2_fwd', 'veon_bev_pool_v2_fwd_fused',
                   'veon_bev_pool_v2_fwd_fused_strided', 'veon_bev_pool_v2_fwd_maxpool',
                   'veon_bev_pool_v2_fwd_maxpool_padded'}) for c in (16, 24)],
    *[_row('tests.test_pool_rows_gpu', 'test_rows_maxpool_random_structures_bit_exact',
           dict(C=c, dtype=d), {'veon_bev_pool_v2_fwd_rows_maxpool_ordered'})
      for c, d in ((4, torch.float32), (64, torch.bfloat16))],
    _row('tests.test_pool_rows_gpu', 'test_voxel_table_equals_searchsorted', {},
         {'veon_bev_pool_voxel_table'}),
    _row('tests.test_lift_train_gpu', 'test_op_random_lift_cases', dict(C=4),
         {'veon_bev_pool_v2_fwd_rows_maxpool_winner', 'veon_bev_pool_v2_bwd_rows_maxpool',
          'veon_bev_pool_point_table'}),
    _row('tests.test_lift_train_gpu', 'test_point_table_from_device_counts', {},
         {'veon_bev_pool_point_table'}),
    _row('tests.test_view_transformer_gpu', 'test_camera_matrices_kernel_matches_torch_inverse',
         {}, {'veon_camera_matrices'}),
    _row('tests.test_view_transformer_gpu', 'test_hip_prepare_fused_geometry_exact',
         dict(name='lss_small_b2'), {'veon_lss_prepare'}),
    _row('tests.test_view_transformer_gpu', 'test_fused_maxpool_bit_equal_to_two_step',
         dict(name='lss_small', mode='percall'), {'veon_lidar_coor', 'veon_lss_prepare'}),
    _row('tests.test_lift_prepare_edges_gpu',
         'test_sparse_entry_keeps_exactly_the_weights_at_or_above_eps', {},
         {'veon_lss_prepare_cameras_sparse'}),
    _row('tests.test_lift_prepare_edges_gpu',
         'test_twohot_entry_keeps_the_window_points_and_emits_compact_slots', dict(eps=0.0),
         {'veon_lss_prepare_cameras_twohot'}),
    _row(HM, 'test_pool_maxpool_into_padded_fp16_volume', {},
         {'veon_bev_pool_v2_fwd_rows_maxpool_ordered'}, 'fp16'),
]

# launched directly (``L.veon_*``) inside an Arena by the two older canary modules
ARENA_DIRECT = {
    'test_lift_bounds_gpu.py': [
        'veon_lss_prepare_cameras', 'veon_bev_pool_v2_fwd_rows',
        'veon_bev_pool_v2_fwd_rows_maxpool', 'veon_bev_pool_plan',
        'veon_bev_pool_v2_fwd_fused_ex', 'veon_bev_pool_row_table',
        'veon_bev_pool_v2_fwd_maxpool_ex', 'veon_downsample_depth', 'veon_two_hot_depth',
        'veon_feat_nchw_to_nhwc'],
    'test_depth_prep_edges_gpu.py': ['veon_two_hot_window'],
}
EXEMPT = {}

# size function -> a row that runs its kernel in a buffer of exactly that size: the local
# bodies pass one; the wrappers allocate what the function returns and nothing more
# (conv3d_ops._workspace, vit_ops.block_workspace, bev_pool.build_plan / build_voxel_table,
# lss_prepare_hip.prepare, align_select._workspace, occ_bin_loss.loss_forward)
EXACT_SIZE = {
    'veon_bev_pool_plan_ints': 'lift_slab_family[C16]',
    'veon_bev_pool_voxel_table_ints': 'pool_rows_gpu.voxel_table_equals_searchsorted[]',
    'veon_lss_prepare_workspace_bytes':
        'view_transformer_gpu.hip_prepare_fused_geometry_exact[lss_small_b2]',
    'veon_vit_gemm_splitk_plan': 'splitk[1025x2500x2048-tile0]',
    'veon_vit_block_workspace_bytes':
        'vit_ops_gpu.whole_block_call_equals_the_seven_ops[1-True-False-True]',
    'veon_conv3d_k3_wgrad_workspace_bytes': 'body_train_gpu.wgrad_against_fp64[2-64-128-3-7-5]',
    'veon_bn3d_sums_workspace_bytes': 'body_train_gpu.bn_passes_against_fp64[1-72-2-3-4]',
    'veon_conv2d_k3_wgrad_workspace_bytes': 'hsa_train_gpu.wgrad2d_against_fp64[2-64-128-7-5]',
    'veon_image_layernorm_bwd_workspace_bytes': 'hsa_train_gpu.ln_passes_against_fp64[1-72-3-5]',
    'veon_linear_wgrad_workspace_bytes':
        'hsa_heads_train_gpu.linear_wgrad_against_fp64[1100-128-128]',
    'veon_rows_colsum_workspace_bytes': 'hsa_heads_train_gpu.row_passes_against_fp64[13-576]',
    'veon_layernorm_f32_bwd_workspace_bytes':
        'hsa_heads_train_gpu.row_passes_against_fp64[13-576]',
    'veon_vit_attention_stats_len': 'attention_bwd_exact[2x65x3]',
    'veon_vit_attention_bwd_workspace_bytes': 'attention_bias_bwd_exact[2x66x3]',
    'veon_deform_attention_bwd_workspace_bytes':
        'temporal_train_gpu.backward_holds_the_fp32_yardstick[layout-B1-hd32-h1-3x5x7]',
    'veon_align_select_groups': 'align_select_gpu.seam_partial_last_workgroup[]',
    'veon_occ_bin_loss_workspace_bytes':
        'occ_bin_loss_gpu.matches_fp64_torch[2-(3,5,4)-two_of_eight]',
    'veon_fusion_dual_ln_bwd_workspace_bytes':
        'fusion_train_gpu.backward_against_fp64_with_torch_fp32_as_the_yardstick[0-0]',
}

_IDS = [r.id for r in ROWS]


def run_row(row):
    """-> the guard's log of one row."""
    if isinstance(row.target, tuple):
        module = importlib.import_module(row.target[0])
        fn = getattr(module, row.target[1])
        kwargs = row.kwargs(module) if callable(row.kwargs) else dict(row.kwargs)
        for v in vars(module).values():            # references cached by an earlier test
            if hasattr(v, 'cache_clear'):          # were computed outside the guard
                v.cache_clear()
    else:
        fn, kwargs = row.target, {}
    with half.use(row.flavour):
        if 'flavour' in inspect.signature(fn).parameters:
            kwargs['flavour'] = half.dtype()
        with guarded() as log:
            fn(**kwargs)
    return log


@pytest.mark.parametrize('row', ROWS, ids=_IDS)
def test_row_between_canary_bands(row):
    log = run_row(row)
    missing = sorted(row.entries - set(log))
    assert not missing, 'the row never launched %s (launched: %s)' % (missing, sorted(set(log)))
    assert not log.unguarded, log.unguarded
    print('%s: %d launches, %.0f us of guard per launch' % (
        row.id, len(log), 1e6 * (log.seconds - log.inner_seconds) / max(len(log), 1)))


# ------------------------------------------------ pointers the guard cannot move
class _ArenaBag(nn.Module):
    """tests.test_optim_step_gpu.Bag with every parameter a view carved out of an Arena:
    sizes around a chunk in two groups, a view one element into its slot (16-byte
    misaligned) and a frozen parameter (an EMA-only record)."""

    def __init__(self, ar, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        chunk = int(_lib.lib().veon_optim_chunk())
        assert chunk == optim.CHUNK

        def carve(n, lead=0, grad=True):
            t = ar.take(n + lead, torch.float32)[lead:]
            t.copy_(torch.randn(n, generator=g))
            return nn.Parameter(t, requires_grad=grad)
        self.first = nn.ParameterList([carve(chunk - 1), carve(chunk)])
        self.second = nn.ParameterList([carve(chunk + 1)])
        self.view = carve(chunk + 904, lead=1)
        self.frozen = carve(chunk + 1, grad=False)
        assert self.view.data_ptr() % 16 == 4

    def groups(self):
        return [dict(params=list(self.first) + [self.view]),
                dict(params=list(self.second), lr=3e-4, weight_decay=0.0)]

    def trained(self):
        return list(self.first) + [self.view] + list(self.second)


def test_optimizer_step_writes_stay_inside_parameters_and_ema_weights():
    """One FusedAdamW step with ModelEMA on parameters and EMA weights of chunk - 1, chunk
    and chunk + 1 elements (and the one-element-off view) carved out of a canary arena:
    equal to the CPU mirror (adamw_ema_step_torch) bit for bit, as
    test_optim_step_gpu.test_three_steps_equal_the_mirror_bit_for_bit, and no byte
    outside the tensors changed."""
    from tests import test_optim_step_gpu as m
    from tests.test_lift_bounds_gpu import Arena
    ar = Arena(1 << 20)
    bag = _ArenaBag(ar, 4)
    cbag = copy.deepcopy(bag).cpu()
    ema = optim.ModelEMA(bag, decay=0.999, updates=900)
    cema = optim.ModelEMA(cbag, decay=0.999, updates=900)
    held = dict(ema.ema.named_parameters())
    for i, (k, src, e) in enumerate(ema.pairs):          # the EMA weights into the arena
        t = ar.take(e.numel(), torch.float32).view_as(e)
        t.copy_(e)
        held[k].data = t
        ema.pairs[i] = (k, src, t)
    assert len(ema.pairs) == 5
    opt = optim.FusedAdamW(bag.groups(), max_norm=5.0, ema=ema, **m.HYPER)
    copt = optim.FusedAdamW(cbag.groups(), max_norm=5.0, ema=cema, **m.HYPER)
    torch.cuda.synchronize()
    ar.check()
    grads = m._grads(bag, 10)
    m._load(bag, opt, grads)
    m._load(cbag, copt, grads)
    n0 = dict(_lib.CALLS)
    opt.step()
    ema.update()
    assert all(_lib.CALLS.get(k, 0) == n0.get(k, 0) + 1 for k in m.NATIVE)
    m._feed_coefficient(copt, opt._scal)
    copt.step()
    cema.update()
    m._assert_same_state((bag, ema, opt), (cbag, cema, copt), 'arena step')
    for k, _, e in ema.pairs:
        assert e.data_ptr() == held[k].data_ptr()
    torch.cuda.synchronize()
    ar.check()


def test_vit_block_reads_and_writes_stay_inside_weights_carved_from_an_arena():
    """veon_vit_block with its residual stream, its workspace of exactly
    veon_vit_block_workspace_bytes and every weight of the host struct carved out of a
    canary arena: the same bits as on ordinary tensors, bands untouched."""
    from tests.test_lift_bounds_gpu import Arena
    torch.manual_seed(5)
    B, T, H = 2, 77, 2
    d, mlp = H * 64, 4 * H * 64
    ar = Arena(16 << 20)

    def carve(t):
        a = ar.take(t.numel(), t.dtype).view_as(t)
        a.copy_(t)
        return a

    def vec(n, s=1.0):
        return (torch.randn(n, device=DEV) * s).contiguous()

    def mat(n, k):
        return vit_ops.to_bf16(torch.randn(n, k, device=DEV) * k ** -0.5)
    n1, n2 = (vec(d, 0.1) + 1, vec(d, 0.1), 1e-6), (vec(d, 0.1) + 1, vec(d, 0.1), 1e-5)
    mats = [mat(3 * d, d), vec(3 * d, 0.1), mat(d, d), vec(d, 0.1), vec(d, 0.5)]
    mlps = [mat(mlp, d), vec(mlp, 0.1), mat(d, mlp), vec(d, 0.1), vec(d, 0.5)]
    bias = torch.randn(B, H, T, T, device=DEV)
    x0 = torch.randn(B * T, d, device=DEV)
    plain = vit_ops.BlockWeights(H, n1, *mats, n2, *mlps, vit_ops.EPI_GELU, q_log2=True)
    want = vit_ops.block_forward_(x0.clone(), plain, B, T,
                                  vit_ops.block_workspace(B, T, d, mlp, DEV), bias)
    c1, c2 = (carve(n1[0]), carve(n1[1]), n1[2]), (carve(n2[0]), carve(n2[1]), n2[2])
    inside = vit_ops.BlockWeights(H, c1, *[carve(t) for t in mats], c2,
                                  *[carve(t) for t in mlps], vit_ops.EPI_GELU, q_log2=True)
    n = int(_lib.lib().veon_vit_block_workspace_bytes(B, T, d, mlp))
    ws = ar.take(n, torch.uint8)
    ws[n - 4096:].zero_()
    got = vit_ops.block_forward_(carve(x0), inside, B, T, ws, carve(bias))
    torch.cuda.synchronize()
    ar.check()
    assert torch.equal(got, want)
