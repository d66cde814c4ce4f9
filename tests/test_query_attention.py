"""The recognition head's query cross-attention and the attention bias at the CLIP grid,
host side (no GPU): ``vit_ops.query_attention_ref`` (the yardstick of
tests/test_query_attention_gpu.py) against the mirror of the reference's attn_helper.py,
``MLPMaskDecoder.attn_bias_at`` against decode-then-resize, the extension header's ABI and
the switches."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden
from tests.test_side_adapter import CFG, _build, _clip_feats
from veon_amd import _lib, vit_ops
from veon_amd.build import INCLUDE
from veon_amd.models.semantic_net import ClipRecHead, semantic_branch_2d
from veon_amd.models.semantic_net import clip_blocks
from veon_amd.models.semantic_net.side_adapter import MLPMaskDecoder

EXT_HEADER = os.path.join(INCLUDE, 'ext', 'veon_hip_query.h')

# max |attn_bias_at - resize(decode)| <= BIAS_BOUND * max |resize(decode)|: four times the
# reassociation error measured for bilinear and bicubic (9.2e-7 of the range: 1.6e-5 on
# values up to 17.7).  Measured with this file's decoder (production widths, range about
# 2): at most 9.0e-7 of the range for 'avg', 9.0e-7 for bilinear, 8.1e-7 for bicubic.
BIAS_BOUND = 4e-6


# ------------------------------------------------------------------------- the mirror
def _attention_core(attn, query, key, mask):
    """``cross_attn_with_self_bias`` without its out_proj: an identity out_proj (the
    projection is the last thing it applies)."""
    D = attn.embed_dim
    saved = attn.out_proj.weight.data.clone(), attn.out_proj.bias.data.clone()
    attn.out_proj.weight.data.copy_(torch.eye(D))
    attn.out_proj.bias.data.zero_()
    try:
        return clip_blocks.cross_attn_with_self_bias(attn, query, key, key, attn_mask=mask)
    finally:
        attn.out_proj.weight.data.copy_(saved[0])
        attn.out_proj.bias.data.copy_(saved[1])


def _projections(attn, query, mem):
    """fp32 operands of ``query_attention_ref`` from the module's packed projection:
    q_qkv (N, Q, 3, H, hd) with q pre-scaled, mem_kv (N, L, 2, H, hd)."""
    D, H = attn.embed_dim, attn.num_heads
    hd = D // H
    w, b = attn.in_proj_weight, attn.in_proj_bias
    qp = F.linear(query, w, b).permute(1, 0, 2).reshape(query.shape[1], -1, 3, H, hd).clone()
    qp[:, :, 0] *= hd ** -0.5
    mp = F.linear(mem, w[D:], b[D:]).permute(1, 0, 2).reshape(mem.shape[1], -1, 2, H, hd)
    return qp, mp


@torch.no_grad()
def test_reference_function_is_the_core_of_the_mirror():
    torch.manual_seed(2)
    D, H, Q, L, N = 128, 2, 5, 11, 3
    attn = torch.nn.MultiheadAttention(D, H).eval()
    query, mem = torch.randn(Q, N, D), torch.randn(L, N, D)
    q_qkv, mem_kv = _projections(attn, query, mem)
    bias = torch.randn(N * H, Q, L)
    mask = torch.rand(N * H, Q, L) < 0.3
    as_bias = torch.zeros(N * H, Q, L).masked_fill(mask, float('-inf'))
    for m, b in ((bias, bias), (mask, as_bias), (None, None)):
        want = _attention_core(attn, query, mem, m).permute(1, 0, 2)       # (N, Q, D)
        got = vit_ops.query_attention_ref(
            q_qkv, mem_kv, H, None if b is None else b.view(N, H, Q, L), dtype=torch.float32)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    # the exp2-domain form of the operands gives the same result
    q2 = q_qkv.clone()
    q2[:, :, 0] *= vit_ops.LOG2E
    got = vit_ops.query_attention_ref(q2, mem_kv, H, bias.view(N, H, Q, L), q_log2=True,
                                      dtype=torch.float32)
    want = _attention_core(attn, query, mem, bias).permute(1, 0, 2)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    # key0: the first memory token dropped
    got = vit_ops.query_attention_ref(q_qkv, mem_kv, H, bias.view(N, H, Q, L)[..., 1:],
                                      key0=1, dtype=torch.float32)
    want = _attention_core(attn, query, mem[1:], bias[..., 1:]).permute(1, 0, 2)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    # every memory key masked: the queries' own v rows, exactly
    dead = torch.full((N, H, Q, L), float('-inf'))
    got = vit_ops.query_attention_ref(q_qkv, mem_kv, H, dead, dtype=torch.float32)
    assert torch.equal(got, q_qkv[:, :, 2].reshape(N, Q, D))
    want = _attention_core(attn, query, mem, torch.ones(N * H, Q, L, dtype=torch.bool))
    torch.testing.assert_close(got, want.permute(1, 0, 2), rtol=1e-5, atol=1e-6)


# -------------------------------------------------------------------- bias reordering
def _decoder(total_layers=1, rescale=True, seed=7):
    torch.manual_seed(seed)
    dec = MLPMaskDecoder(in_channels=24, total_heads=12, total_layers=total_layers,
                         embed_channels=256, mlp_channels=256, mlp_num_layers=3,
                         rescale_attn_bias=rescale).eval()
    with torch.no_grad():
        dec.attn_mlp.layers[-1].weight.mul_(3.0)
        dec.attn_mlp.layers[-1].bias.mul_(3.0)
        if rescale:
            dec.bias_scaling.weight.fill_(0.7)
            dec.bias_scaling.bias.fill_(-0.3)
    return dec, torch.randn(2, 7, 24), torch.randn(2, 24, 8, 12)


def _head(mode, heads=12, width=None):
    width = width or heads * 8
    blocks = [clip_blocks.ResidualAttentionBlock(width, heads)]
    return ClipRecHead(blocks, torch.nn.LayerNorm(width),
                       torch.nn.Parameter(torch.randn(width, 8)), downsample_method=mode)


@torch.no_grad()
@pytest.mark.parametrize('rescale', [True, False])
@pytest.mark.parametrize('size', [(4, 6), (5, 7), (8, 12)])
@pytest.mark.parametrize('mode', ['bilinear', 'bicubic', 'avg'])
def test_bias_at_the_target_grid_equals_decode_then_resize(mode, size, rescale):
    dec, query, x = _decoder(rescale=rescale)
    head = _head(mode)
    ref = head._build_attn_biases(dec(query, x)[1], size)[0]           # (B*heads, Q, h*w)
    got = dec.attn_bias_at(query, x, size, mode)
    assert got.shape == (2, 12, 7) + size
    scale = ref.abs().max().item()
    err = (got.reshape(ref.shape) - ref).abs().max().item()
    print('attn_bias_at %s %s: max |diff| %.3g of range %.3g (%.3g relative)'
          % (mode, size, err, scale, err / scale))
    assert err <= BIAS_BOUND * scale, (err, scale)
    # through forward, and passed through by the head
    preds, at = dec(query, x, bias_size=size, bias_mode=mode)
    assert torch.equal(preds, dec(query, x)[0])
    assert len(at) == 1 and torch.equal(at[0], got)
    assert torch.equal(head._build_attn_biases(at, size)[0], got.reshape(ref.shape))


@torch.no_grad()
def test_everything_else_takes_the_old_route():
    dec, query, x = _decoder()
    old = dec(query, x)[1]
    for mode in ('nearest', 'max', 'adaptive_max'):
        assert not dec.bias_at_ok(mode)
        new = dec(query, x, bias_size=(4, 6), bias_mode=mode)[1]
        assert len(new) == 1 and torch.equal(new[0], old[0])           # at the source grid
        with pytest.raises(ValueError):
            dec.attn_bias_at(query, x, (4, 6), mode)
    dec2, query, x = _decoder(total_layers=2)
    old = dec2(query, x)[1]
    new = dec2(query, x, bias_size=(4, 6), bias_mode='bilinear')[1]
    assert len(new) == 2 and all(torch.equal(a, b) for a, b in zip(new, old))
    with pytest.raises(ValueError):
        dec2.attn_bias_at(query, x, (4, 6), 'bilinear')


# ------------------------------------------------------------------------------- ABI
def test_extension_header_and_binding():
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    table = _lib._parse_header(EXT_HEADER)
    assert sorted(table) == ['veon_query_attention'] == _lib.ext_symbols()
    assert table['veon_query_attention'] == _lib._EXT_SIGNATURES['veon_query_attention'] == \
        (ci, [vp, vp, i64, vp, i64, i64, vp, ci, ci, ci, ci, ci, ci, vp])
    main = _lib._parse_header(os.path.join(INCLUDE, 'veon_hip.h'))
    assert _lib.declared_symbols() == sorted(main) == sorted(_lib._SIGNATURES)
    assert 'veon_query_attention' not in _lib.declared_symbols()
    # the guard's parser reads the same header (names and const-ness)
    from tests import launch_guard
    params = launch_guard.parse_params(EXT_HEADER)['veon_query_attention']
    assert [p[0] for p in params] == [
        'q_qkv', 'mem_kv', 'mem_token_stride', 'bias', 'bias_batch_stride',
        'bias_head_stride', 'out', 'B', 'Q', 'T', 'key0', 'H', 'q_log2', 'stream']
    assert [p[0] for p in params if p[2]] == ['q_qkv', 'mem_kv', 'bias']
    assert 'veon_query_attention' not in launch_guard.PARAMS


def test_both_libraries_export_the_extension_symbol():
    from veon_amd import build
    build.build()
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        assert hasattr(lib, 'veon_query_attention'), os.path.basename(path)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2                 # host-only calls, no GPU needed
        # a NULL operand is refused on the host, before anything is launched
        fn = lib.veon_query_attention
        fn.restype, fn.argtypes = _lib._EXT_SIGNATURES['veon_query_attention']
        assert fn(None, None, 128, None, 0, 0, None, 1, 1, 1, 0, 1, 0, None) == 1


def test_headers_under_ext_are_build_dependencies():
    from veon_amd import build
    assert EXT_HEADER in build._headers()


# -------------------------------------------------------------------------- switches
def test_switches_default_to_off():
    import inspect
    from veon_amd.models.veon_occ import VeonOccupancyPath
    assert ClipRecHead.hip_query is False
    assert VeonOccupancyPath.hip_rec_head is False
    assert inspect.signature(semantic_branch_2d).parameters['hip_query'].default is None
    assert inspect.signature(ClipRecHead.forward).parameters['hip_query'].default is None


@torch.no_grad()
def test_switch_on_the_cpu_changes_only_the_grid_of_the_bias():
    g = load_golden('side_adapter_tiny')
    trunk, head, net = _build(g)
    images = torch.from_numpy(g['images'])
    ov = torch.from_numpy(g['ov_classifier_weight'])
    feats = _clip_feats(trunk, images, CFG['clip_first_tail'])
    # the head alone: no ROCm device, so the switch changes nothing
    bias = net(images, feats)[1][0]
    off = head(feats, bias, normalize=True)
    head.hip_query = True
    assert torch.equal(head(feats, bias, normalize=True), off)
    assert torch.equal(head(feats, bias, normalize=True, hip_query=True), off)
    head.hip_query = False
    # the branch: the bias arrives at the CLIP grid, everything else as before
    want = semantic_branch_2d(net, head, ov, images, feats)
    calls = _lib.CALLS.get('veon_query_attention', 0)
    for via_attribute in (False, True):
        head.hip_query = via_attribute
        got = semantic_branch_2d(net, head, ov, images, feats,
                                 hip_query=None if via_attribute else True)
        head.hip_query = False
        assert set(got) == set(want)
        hw = tuple(feats[CFG['clip_first_tail']].shape[-2:])
        assert tuple(got['attn_biases'][0].shape[-2:]) == hw != \
            tuple(want['attn_biases'][0].shape[-2:])
        ref = head._build_attn_biases(want['attn_biases'], hw)[0]
        err = (got['attn_biases'][0].reshape(ref.shape) - ref).abs().max().item()
        assert err <= BIAS_BOUND * ref.abs().max().item(), err
        assert torch.equal(got['mask_preds'], want['mask_preds'])
        for k in ('mask_embs', 'mask_logits', 'sem_seg_ds', 'sem_embed_ds', 'sem_seg'):
            torch.testing.assert_close(got[k], want[k], rtol=1e-4, atol=1e-5)
    assert _lib.CALLS.get('veon_query_attention', 0) == calls
