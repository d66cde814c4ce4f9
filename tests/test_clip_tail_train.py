"""CPU side of the native training of the CLIP tail: the fp64 closed
forms the GPU tests use as references against torch's own autograd, the torch restatements
of ``vit_ops``, and the ``ResidualAttentionBlock.hip_train`` switch where it must change
nothing."""
import copy

import pytest
import torch

from tests import clip_tail_train_refs as refs
from veon_amd import vit_ops
from veon_amd.models.semantic_net.clip_blocks import (ClipRecHead, QuickGELU,
                                                       ResidualAttentionBlock)

SHAPES = [(1, 1, 1, 0), (1, 2, 1, 1), (2, 5, 2, 1), (1, 7, 3, 0)]


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    ResidualAttentionBlock.hip_train = False


def _autograd(qkv, bias, dout, H, border):
    """fp64 autograd of the plain formula softmax(scale q k^T + bias) v."""
    B, T = qkv.shape[:2]
    x = qkv.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    q, k, v = x.reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q * refs.SCALE) @ k.transpose(-2, -1) + refs.full_bias(b, B, H, T, border)
    out = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, H * 64)
    dx, db = torch.autograd.grad(out, (x, b), dout)
    return out.detach(), dx, db


@pytest.mark.parametrize('kind', refs.BIAS_KINDS)
@pytest.mark.parametrize('B,T,H,border', SHAPES)
def test_closed_forms_against_fp64_autograd(B, T, H, border, kind):
    """dq, dk, dv and dbias of the closed form (tests/clip_tail_train_refs.py) and of
    ``vit_ops.attention_bias_bwd_ref`` against fp64 autograd, some entries -inf, to 1e-12."""
    g = torch.Generator().manual_seed(100 * T + H)
    qkv, dout = refs.operands(B, T, H, g)
    bias = refs.mask_some_(refs.gram_bias(B, T, H, border, kind, g, torch.float64), border)
    if T - border >= 2 or (T - border == 1 and border):
        assert bool((bias == refs.NEG).any())
    out, dx, db = _autograd(qkv, bias, dout, H, border)
    assert not bool(torch.isnan(dx).any() | torch.isnan(db).any())
    got_out, _ = refs.forward(qkv, bias, H, border)
    dqkv, dense = refs.backward(qkv, bias, dout, H, border)
    assert dense.shape == (B, H, T - border, T - border)
    assert float((got_out - out).abs().max()) <= 1e-12
    assert float((dqkv - dx).abs().max()) <= 1e-12
    assert float((refs.reduce_dbias(dense, bias) - db).abs().max() if db.numel() else 0) <= 1e-12
    # the restatements of vit_ops, in fp64
    assert float((vit_ops.attention_bias_ref(qkv, bias, H, refs.SCALE, border) - out)
                 .abs().max()) <= 1e-12
    dqkv2, dense2 = vit_ops.attention_bias_bwd_ref(qkv, bias, dout, H, refs.SCALE, border)
    assert float((dqkv2 - dx).abs().max()) <= 1e-12
    assert dense2.shape == dense.shape
    assert float((dense2 - dense).abs().max() if dense.numel() else 0) <= 1e-12


def test_quickgelu_closed_form_against_fp64_autograd():
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(4, 64, generator=g) * 3).double().requires_grad_(True)
    dh = torch.randn(4, 64, generator=g).double()
    want, = torch.autograd.grad(QuickGELU()(y), y, dh)
    assert float((refs.quickgelu_bwd(dh, y.detach()) - want).abs().max()) <= 1e-12
    assert float((vit_ops.quickgelu_bwd_ref(dh, y.detach()) - want).abs().max()) <= 1e-12
    assert float((refs.quickgelu(y.detach()) - QuickGELU()(y).detach()).abs().max()) <= 1e-12


def test_a_fully_masked_query_has_zero_gradients():
    """Autograd gives NaN in a fully masked row (softmax of -inf alone) and, through dk and
    dv, everywhere in that (b, h); the closed forms define P = 0 there.  So: the zeros are
    asserted on their own, and every other (b, h) is compared with autograd as above; in the
    masked (b, h) the closed form must equal the same problem WITHOUT that query (its keys
    stay), which is what "contributes nothing" means."""
    B, T, H, border, dead_q = 2, 5, 2, 0, 3
    g = torch.Generator().manual_seed(11)
    qkv, dout = refs.operands(B, T, H, g)
    bias = refs.gram_bias(B, T, H, border, 'full', g, torch.float64)
    bias[1, 0, dead_q, :] = refs.NEG
    out, lse = refs.forward(qkv, bias, H, border)
    dqkv, dense = refs.backward(qkv, bias, dout, H, border)
    assert not bool(torch.isnan(out).any() | torch.isnan(dqkv).any() | torch.isnan(dense).any())
    assert float(lse[1, 0, dead_q]) == float('inf')
    assert float(out.view(B, T, H, 64)[1, dead_q, 0].abs().max()) == 0.0
    assert float(dqkv.view(B, T, 3, H, 64)[1, dead_q, 0, 0].abs().max()) == 0.0
    assert float(dense[1, 0, dead_q].abs().max()) == 0.0
    _, dx, db = _autograd(qkv, bias, dout, H, border)
    live = torch.ones(B, H, dtype=torch.bool)
    live[1, 0] = False
    dx5, d5 = dx.view(B, T, 3, H, 64), dqkv.view(B, T, 3, H, 64)
    assert bool(torch.isnan(dx5[1, :, :, 0]).any())
    for b in range(B):
        for h in range(H):
            if live[b, h]:
                assert float((d5[b, :, :, h] - dx5[b, :, :, h]).abs().max()) <= 1e-12
                assert float((dense[b, h] - db[b, h]).abs().max()) <= 1e-12
    # the masked (b, h) with the dead query's dout set to zero and one key opened for it:
    # that query then has dS = 0, so every other gradient must be what the closed form gave
    bias2 = bias.clone()
    bias2[1, 0, dead_q, 0] = 0.0
    dout2 = dout.clone()
    dout2.view(B, T, H, 64)[1, dead_q, 0] = 0
    _, dx2, db2 = _autograd(qkv, bias2, dout2, H, border)
    assert float((d5[1, :, :, 0] - dx2.view(B, T, 3, H, 64)[1, :, :, 0]).abs().max()) <= 1e-12
    assert float((dense[1, 0] - db2[1, 0]).abs().max()) <= 1e-12
    # vit_ops' restatement follows the same definition
    dqkv3, dense3 = vit_ops.attention_bias_bwd_ref(qkv, bias, dout, H, refs.SCALE, border)
    assert float((dqkv3 - dqkv).abs().max()) <= 1e-12
    assert float((dense3 - dense).abs().max()) <= 1e-12


def test_border_equals_the_head_built_zero_border():
    """``attention_bias_ref`` with border = 1 on the patch-to-patch matrix equals the same
    call on ``ClipRecHead.build_attn_bias``'s (B H, L + 1, L + 1) output with border = 0."""
    B, T, H = 2, 6, 3
    g = torch.Generator().manual_seed(5)
    qkv, _ = refs.operands(B, T, H, g, torch.float32)
    bias = refs.gram_bias(B, T, H, 1, 'full', g)
    a = vit_ops.attention_bias_ref(qkv, bias, H, refs.SCALE, border=1)
    b = vit_ops.attention_bias_ref(qkv, ClipRecHead.build_attn_bias(bias), H, refs.SCALE, border=0)
    assert torch.equal(a, b)


# --------------------------------------------------------------------------- the switch
def _block_step(blk, x, mask, G):
    blk = copy.deepcopy(blk)
    x = x.clone().requires_grad_(True)
    m = mask
    if mask is not None and mask.is_floating_point():
        m = mask.clone().requires_grad_(True)
    out = blk(x, attn_mask=m)
    out.backward(G)
    res = {'out': out.detach(), 'dx': x.grad}
    if m is not None and m.is_floating_point():
        res['dmask'] = m.grad
    res.update({k: p.grad for k, p in blk.named_parameters()})
    return res


def _cases():
    g = torch.Generator().manual_seed(21)
    L, N = 5, 2

    def mk(D, heads):
        torch.manual_seed(22)
        return ResidualAttentionBlock(D, heads), torch.randn(L, N, D, generator=g), \
            torch.randn(L, N, D, generator=g)
    plain = mk(128, 2) + (torch.randn(N * 2, L, L, generator=g),)
    boolm = mk(128, 2) + (torch.rand(L, L, generator=g) > 0.7,)
    boolm[3].fill_diagonal_(False)
    d96 = mk(96, 2) + (torch.randn(L, L, generator=g),)
    drop = mk(128, 2) + (None,)
    drop[0].attn.dropout = 0.1
    return {'plain': plain, 'bool mask': boolm, 'D = 96': d96, 'dropout': drop}


def test_switch_defaults_to_off_and_changes_nothing_on_the_cpu():
    """hip_train is False by default; set, a CPU block (also with a bool mask, D = 96, or
    dropout > 0) is rejected by ``_hip_train_ok`` and its output and every gradient are
    bit-equal to the switch off."""
    assert ResidualAttentionBlock.hip_train is False
    for name, (blk, x, G, mask) in _cases().items():
        torch.manual_seed(1)            # (dropout draws)
        off = _block_step(blk, x, mask, G)
        ResidualAttentionBlock.hip_train = True
        try:
            assert blk._hip_train_ok(x, mask) is False, name
            torch.manual_seed(1)
            on = _block_step(blk, x, mask, G)
        finally:
            ResidualAttentionBlock.hip_train = False
        assert set(on) == set(off)
        for k in off:
            assert torch.equal(on[k], off[k]), (name, k)
