"""Host-side checks of the native training path of the DINOv2 blocks
(csrc/attention_train.hip): the C ABI additions, the torch reference of
the attention backward against fp64 autograd, the LoRA pad packers, and the switch (plain
torch, CPU)."""
import copy
import ctypes

import pytest
import torch

from veon_amd import _lib, vit_ops
from veon_amd.models import _train_fns
from veon_amd.models.depth_anything.dinov2 import Attention, Block

_I, _L, _P, _F = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float

# what the wrappers of veon_amd/vit_ops.py pass, stream last
WANT = {
    # T (host-only)
    'veon_vit_attention_stats_len': (_L, [_I]),
    # qkv out lse | B T H head_dim | scale | stream
    'veon_vit_attention_fwd_lse': (_I, [_P] * 3 + [_I] * 4 + [_F] + [_P]),
    # B T H (host-only)
    'veon_vit_attention_bwd_workspace_bytes': (_L, [_I] * 3),
    # qkv out dout lse dqkv workspace | workspace_bytes | B T H head_dim | scale | stream
    'veon_vit_attention_bwd': (_I, [_P] * 6 + [_L] + [_I] * 4 + [_F] + [_P]),
}


def test_header_and_libraries_carry_the_attention_training_entry_points():
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
        stats_len = lib.veon_vit_attention_stats_len
        stats_len.restype, stats_len.argtypes = WANT['veon_vit_attention_stats_len']
        assert [stats_len(t) for t in (-3, 0, 1, 64, 65, 901)] == [0, 0, 64, 64, 128, 960]
        ws = lib.veon_vit_attention_bwd_workspace_bytes
        ws.restype, ws.argtypes = WANT['veon_vit_attention_bwd_workspace_bytes']
        assert ws(6, 901, 16) == 6 * 16 * 960 * 4 and ws(0, 5, 1) == -1 and ws(1, 5, 0) == -1


def test_switch_is_off_by_default_and_cpu_keeps_the_torch_definition():
    """With the switch on, a CPU block in training mode is bit-equal (output and every
    gradient) to the switch off, and no new entry point is called."""
    assert Block.hip_train is False
    torch.manual_seed(2)
    blk = Block(128, 2, init_values=1.0, lora_r=4).train()
    with torch.no_grad():
        for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            m.lora_B.normal_(0, 0.05)
    x = torch.randn(2, 9, 128)

    def run(switch):
        m = copy.deepcopy(blk)
        xi = x.clone().requires_grad_(True)
        Block.hip_train = switch
        try:
            assert not m._hip_train_ok(xi)
            out = m(xi)
            out.square().sum().backward()
        finally:
            Block.hip_train = False
        return [out.detach(), xi.grad] + [p.grad for p in m.parameters()]
    before = {k: _lib.CALLS.get(k, 0) for k in WANT}
    for a, b in zip(run(False), run(True)):
        assert (a is None and b is None) or torch.equal(a, b)
    assert {k: _lib.CALLS.get(k, 0) for k in WANT} == before


def test_attention_references_equal_fp64_autograd_of_the_module():
    """``attention_ref`` is the arithmetic of the module's ``Attention`` (between its two
    Linears), and ``attention_bwd_ref`` its fp64 autograd, to 1e-12."""
    g = torch.Generator().manual_seed(5)
    B, T, H, hd = 2, 11, 3, 8
    att = Attention(H * hd, num_heads=H).double()
    qkv = torch.randn(B, T, 3 * H * hd, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(B, T, H * hd, generator=g, dtype=torch.float64)
    # the module's own lines on a given qkv (attention.py:56-69)
    q, k, v = qkv.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    attn = ((q * att.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    out = (attn @ v).transpose(1, 2).reshape(B, T, H * hd)
    out.backward(dout)
    ref = vit_ops.attention_ref(qkv.detach(), H, att.scale)
    assert ((ref - out.detach()).norm() / out.detach().norm()).item() <= 1e-12
    got = vit_ops.attention_bwd_ref(qkv.detach(), dout, H, att.scale)
    assert got.shape == qkv.shape
    for i in range(3):
        a = got.view(B, T, 3, -1)[:, :, i]
        b = qkv.grad.view(B, T, 3, -1)[:, :, i]
        assert ((a - b).norm() / b.norm()).item() <= 1e-12, i


@pytest.mark.parametrize('r', [1, 4, 16, 64])
def test_lora_pad_packers(r):
    """A_pad [64, in]: A in rows 0..r-1; B_pad [out, 64]: scaling * B in columns 0..r-1;
    zeros elsewhere, so that B_pad A_pad = scaling * B A exactly as a product of padded
    matrices."""
    g = torch.Generator().manual_seed(r)
    A = torch.randn(r, 128, generator=g)
    Bm = torch.randn(192, r, generator=g)
    s = 1.0 / r
    a_pad, b_pad = _train_fns.lora_pad_a(A), _train_fns.lora_pad_b(Bm, s)
    assert a_pad.shape == (64, 128) and b_pad.shape == (192, 64)
    assert a_pad.dtype == b_pad.dtype == torch.float32
    assert torch.equal(a_pad[:r], A) and not a_pad[r:].any()
    assert torch.equal(b_pad[:, :r], Bm * s) and not b_pad[:, r:].any()
    x = torch.randn(5, 128, generator=g).double()
    want = (x @ A.double().t() @ Bm.double().t()) * s
    got = x @ a_pad.double().t() @ b_pad.double().t()
    assert ((got - want).norm() / want.norm()).item() <= 1e-7
    with pytest.raises(AssertionError):
        _train_fns.lora_pad_a(torch.zeros(65, 128))
