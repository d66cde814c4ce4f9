"""``veon_query_attention`` (include/ext/veon_hip_query.h) on the device, both half
flavours: the kernel against ``vit_ops.query_attention_ref`` in fp64 on the rounded operands
(that function is pinned to the mirror of the reference's attn_helper.py by
tests/test_query_attention.py), the seams of its running statistics, determinism, one run
between canary bands, the argument checks, and the recognition head / the 2-D branch with
the switch on."""
import os

import pytest
import torch

from tests import launch_guard
from tests.conftest import load_golden
from tests.helpers import flavour, fp16_twin, half_tol, named_init_  # noqa: F401
from tests.test_clip_blocks import _head_from_golden
from veon_amd import _lib, half, vit_ops
from veon_amd.build import INCLUDE
from veon_amd.graphs import GraphedCallable
from veon_amd.models.semantic_net import ClipRecHead, clip_blocks

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXT_HEADER = os.path.join(INCLUDE, 'ext', 'veon_hip_query.h')
# P is rounded to half before P.V, output half: the project's attention tolerance
ATT_TOL = (2 ** -7, 4e-3)
LN2 = 1.0 / vit_ops.LOG2E


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _operands(B, Q, Lk, H, key0, seed, q_log2, scale=0.5):
    """(q_qkv half [B, Q, 3, H, 64], mem_kv half [B, T, 2, H, 64]), T = key0 + Lk."""
    q = _rand(B, Q, 3, H, 64, seed=seed) * scale
    if q_log2:
        q[:, :, 0] *= vit_ops.LOG2E
    mem = _rand(B, key0 + Lk, 2, H, 64, seed=seed + 1) * scale
    return q.to(half.dtype()), mem.to(half.dtype())


def _check(q_qkv, mem_kv, H, bias, key0, q_log2, tol=ATT_TOL):
    got = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=key0, q_log2=q_log2)
    assert got.dtype == half.dtype() and got.shape == q_qkv.shape[:2] + (H * 64,)
    ref = vit_ops.query_attention_ref(q_qkv, mem_kv, H, bias, key0=key0, q_log2=q_log2,
                                      dtype=torch.float64)
    assert torch.isfinite(ref).all()
    torch.testing.assert_close(got.double(), ref, **half_tol(*tol))
    return got


SHAPES = [(1, 1, 1, 1, 0), (1, 16, 64, 1, 0), (2, 17, 65, 2, 1), (1, 5, 63, 3, 1),
          (2, 100, 176, 12, 1), (1, 100, 704, 12, 1), (3, 33, 130, 4, 0)]


@pytest.mark.parametrize('q_log2', [False, True])
@pytest.mark.parametrize('B,Q,Lk,H,key0', SHAPES)
def test_kernel_against_the_fp64_reference(B, Q, Lk, H, key0, q_log2, flavour):
    q_qkv, mem_kv = _operands(B, Q, Lk, H, key0, 11, q_log2)
    full = _rand(B, H, Q, Lk, seed=13)
    for bias in (None, full, full[:1].contiguous(), full[:, :1].contiguous(),
                 full[:1, :1].contiguous()):
        _check(q_qkv, mem_kv, H, bias, key0, q_log2)
    # broadcast axes given as zero strides of an expanded view
    _check(q_qkv, mem_kv, H, full[:1, :1].expand(B, H, Q, Lk), key0, q_log2)


test_kernel_against_the_fp64_reference_fp16 = fp16_twin(test_kernel_against_the_fp64_reference)


@pytest.mark.parametrize('q_log2', [False, True])
def test_memory_as_the_kv_part_of_a_packed_buffer(q_log2, flavour):
    """``mem_token_stride``: K/V of the memory read in place from a [B, T, 3, H, 64] qkv
    buffer (what a later reuse of the block's projection would hand over)."""
    B, Q, Lk, H, key0 = 2, 17, 65, 2, 1
    q_qkv, _ = _operands(B, Q, Lk, H, key0, 21, q_log2)
    packed = (_rand(B, key0 + Lk, 3, H, 64, seed=23) * 0.5).to(flavour)
    view = packed[:, :, 1:]
    assert not view.is_contiguous() and view.stride(1) == 3 * H * 64
    bias = _rand(B, H, Q, Lk, seed=24)
    before = _lib.CALLS.get('veon_query_attention', 0)
    got = _check(q_qkv, view, H, bias, key0, q_log2)
    assert _lib.CALLS['veon_query_attention'] == before + 1
    same = vit_ops.query_attention(q_qkv, view.contiguous(), H, bias, key0=key0,
                                   q_log2=q_log2)
    assert torch.equal(got, same)


test_memory_as_the_kv_part_of_a_packed_buffer_fp16 = fp16_twin(
    test_memory_as_the_kv_part_of_a_packed_buffer)


# ----------------------------------------------------------------------------- the seams
@pytest.mark.parametrize('q_log2', [False, True])
def test_masked_first_tile_then_live_scores_far_below_the_self_logit(q_log2, flavour):
    """Keys 0..63 masked, every live score about 300 log2 units below zero."""
    B, Q, Lk, H = 2, 37, 130, 2
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 31, q_log2)
    bias = _rand(B, H, Q, Lk, seed=33) * 2.0 - 210.0
    bias[..., :64] = float('-inf')
    _check(q_qkv, mem_kv, H, bias, 1, q_log2)


@pytest.mark.parametrize('live', [0.0, -210.0])
@pytest.mark.parametrize('q_log2', [False, True])
def test_live_keys_only_in_the_ragged_last_tile(q_log2, live, flavour):
    B, Q, Lk, H = 1, 21, 150, 3
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 35, q_log2)
    bias = _rand(B, H, Q, Lk, seed=37) * 2.0 + live
    bias[..., :128] = float('-inf')
    _check(q_qkv, mem_kv, H, bias, 1, q_log2)


@pytest.mark.parametrize('q_log2', [False, True])
def test_masked_middle_tile_then_a_rise_of_40(q_log2, flavour):
    """Live tile 0 near the reference, tile 1 masked, tile 2 forty log2 units higher (the
    reference moves after a masked tile), a ragged tail near zero again."""
    B, Q, Lk, H = 2, 33, 260, 2
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 0, 39, q_log2)
    bias = _rand(B, H, Q, Lk, seed=41)
    bias[..., 64:128] = float('-inf')
    bias[..., 128:192] += 40.0 * LN2
    _check(q_qkv, mem_kv, H, bias, 0, q_log2)
    # and in steps on both sides of the threshold, tile after tile
    steps = _rand(B, H, Q, Lk, seed=43)
    for t, rise in enumerate((0.0, 6.0, 15.0, 9.0, 40.0)):
        steps[..., 64 * t:64 * (t + 1)] += rise * LN2
    _check(q_qkv, mem_kv, H, steps, 0, q_log2)


def _with_self_logit(q_qkv, sign, q_log2):
    """The operands with q.k_q moved by about 1e4 (log2 units or more) in the direction of
    ``sign``: a component of 10 along e0 in q, of +-1000 in the query's own k row (both
    exact in either half type); the memory keys see only q's e0 component."""
    x = q_qkv.clone()
    x[:, :, 0, :, 0] = 10.0
    x[:, :, 1, :, 0] = sign * 1000.0
    return x


@pytest.mark.parametrize('q_log2', [False, True])
def test_self_logit_far_below_every_key_is_plain_attention(q_log2, flavour):
    B, Q, Lk, H = 2, 19, 100, 2
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 45, q_log2)
    q_qkv = _with_self_logit(q_qkv, -1.0, q_log2)
    bias = _rand(B, H, Q, Lk, seed=47)
    got = _check(q_qkv, mem_kv, H, bias, 1, q_log2)
    # attention over the memory keys alone
    x = q_qkv.double()
    q = x[:, :, 0].permute(0, 2, 1, 3)
    k, v = mem_kv.double()[:, 1:].permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-2, -1) * (LN2 if q_log2 else 1.0) + bias.double()
    plain = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, Q, H * 64)
    torch.testing.assert_close(got.double(), plain, **half_tol(*ATT_TOL))


@pytest.mark.parametrize('q_log2', [False, True])
def test_self_logit_far_above_every_key_gives_the_v_rows(q_log2, flavour):
    B, Q, Lk, H = 2, 19, 100, 2
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 49, q_log2)
    q_qkv = _with_self_logit(q_qkv, 1.0, q_log2)
    got = _check(q_qkv, mem_kv, H, _rand(B, H, Q, Lk, seed=51), 1, q_log2)
    assert torch.equal(got, q_qkv[:, :, 2].reshape(B, Q, H * 64))


@pytest.mark.parametrize('q_log2', [False, True])
def test_biases_of_plus_and_minus_fifty(q_log2, flavour):
    B, Q, Lk, H = 2, 40, 200, 3
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 53, q_log2)
    bias = torch.where(_rand(B, H, Q, Lk, seed=55) > 0, 50.0, -50.0)
    _check(q_qkv, mem_kv, H, bias, 1, q_log2)
    bias = bias + _rand(B, H, Q, Lk, seed=57)
    _check(q_qkv, mem_kv, H, bias, 1, q_log2)


@pytest.mark.parametrize('q_log2', [False, True])
def test_every_memory_key_masked_gives_the_v_rows_bit_for_bit(q_log2, flavour):
    B, Q, Lk, H = 2, 70, 150, 3
    q_qkv, mem_kv = _operands(B, Q, Lk, H, 1, 59, q_log2)
    bias = torch.full((B, H, Q, Lk), float('-inf'), device=DEV)
    got = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=1, q_log2=q_log2)
    assert torch.equal(got, q_qkv[:, :, 2].reshape(B, Q, H * 64))
    # some rows only: the others are ordinary rows
    some = _rand(B, H, Q, Lk, seed=61)
    dead = [0, 15, 16, 69]
    some[:, :, dead] = float('-inf')
    got = _check(q_qkv, mem_kv, H, some, 1, q_log2)
    assert torch.equal(got[:, dead], q_qkv[:, dead, 2].reshape(B, len(dead), H * 64))


for _t in (test_masked_first_tile_then_live_scores_far_below_the_self_logit,
           test_live_keys_only_in_the_ragged_last_tile,
           test_masked_middle_tile_then_a_rise_of_40,
           test_self_logit_far_below_every_key_is_plain_attention,
           test_self_logit_far_above_every_key_gives_the_v_rows,
           test_biases_of_plus_and_minus_fifty,
           test_every_memory_key_masked_gives_the_v_rows_bit_for_bit):
    globals()[_t.__name__ + '_fp16'] = fp16_twin(_t)


# ------------------------------------------------------- determinism, bands, arguments
def test_two_runs_are_bit_equal(flavour):
    B, Q, Lk, H, key0 = 2, 100, 176, 12, 1
    q_qkv, mem_kv = _operands(B, Q, Lk, H, key0, 63, True)
    bias = _rand(B, H, Q, Lk, seed=65)
    a = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=key0, q_log2=True)
    b = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=key0, q_log2=True)
    assert torch.equal(a, b)


test_two_runs_are_bit_equal_fp16 = fp16_twin(test_two_runs_are_bit_equal)


def test_one_run_between_canary_bands(monkeypatch, flavour):
    """Exact-size tensors, every operand between bands of 0xFF: the bands come back
    intact, the const operands unchanged (the guard raises otherwise), the result is the
    unguarded one."""
    monkeypatch.setattr(launch_guard, 'PARAMS',
                        {**launch_guard.PARAMS, **launch_guard.parse_params(EXT_HEADER)})
    B, Q, Lk, H, key0 = 2, 17, 65, 2, 1
    q_qkv, mem_kv = _operands(B, Q, Lk, H, key0, 67, True)
    bias = _rand(B, H, Q, Lk, seed=69)
    for t in (q_qkv, mem_kv, bias):
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
    want = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=key0, q_log2=True)
    with launch_guard.guarded() as log:
        got = vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=key0, q_log2=True)
    assert log == ['veon_query_attention'] and not log.unguarded
    assert torch.equal(got, want)
    _check(q_qkv, mem_kv, H, bias, key0, True)


test_one_run_between_canary_bands_fp16 = fp16_twin(test_one_run_between_canary_bands)


def test_bad_arguments_raise_and_launch_nothing(flavour):
    B, Q, T, H = 2, 5, 9, 2
    q_qkv, mem_kv = _operands(B, Q, T, H, 0, 71, False)
    bias = _rand(B, H, Q, T, seed=73)
    out = torch.full((B, Q, H * 64), 3.0, dtype=flavour, device=DEV)
    ts = 2 * H * 64
    good = [q_qkv, mem_kv, ts, bias, H * Q * T, Q * T, out, B, Q, T, 0, H, 0]
    _lib.launch('veon_query_attention', torch.device(DEV), *good)     # the list is valid
    out.fill_(3.0)
    odd = torch.empty(q_qkv.numel() + 8, dtype=flavour, device=DEV)[1:]
    bad = {'B': {7: 0}, 'Q': {8: 0}, 'T': {9: 0}, 'H': {11: 0}, 'negative Q': {8: -1},
           'key0 < 0': {10: -1}, 'key0 = T': {10: T}, 'stride < 2 H 64': {2: ts - 8},
           'stride % 8': {2: ts + 4}, 'null q': {0: None}, 'null mem': {1: None},
           'null out': {6: None}, 'misaligned q': {0: odd},
           'memory of 2^31 bytes': {2: 1 << 26, 9: 16},
           'queries of 2^31 bytes': {8: 1 << 22},
           'bias rows of 2^31 bytes': {8: 1 << 12, 9: (1 << 17) + 1, 10: 1}}
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(_lib.VeonHipError):
            _lib.launch('veon_query_attention', torch.device(DEV), *args)
    torch.cuda.synchronize()
    assert (out.float() == 3.0).all(), 'a refused call wrote the output'
    # the wrapper's own checks
    with pytest.raises(_lib.VeonHipError):
        vit_ops.query_attention(q_qkv.float(), mem_kv, H)
    with pytest.raises(_lib.VeonHipError):
        vit_ops.query_attention(q_qkv.cpu(), mem_kv.cpu(), H)
    with pytest.raises(_lib.VeonHipError):                             # head_dim 32
        vit_ops.query_attention(q_qkv, mem_kv, 2 * H)


test_bad_arguments_raise_and_launch_nothing_fp16 = fp16_twin(
    test_bad_arguments_raise_and_launch_nothing)


# ------------------------------------------------------------------------------- the head
@torch.no_grad()
def test_head_against_the_reference_vector(flavour):
    """tests/golden/clip_head_tiny.npz (the reference's own RecWithAttnbiasHead): width 64,
    one head, five blocks of which three are the tail, three queries.  The bound is the one
    test_rec_head_tail_blocks_on_mfma holds the same fixture to through the same number of
    half-precision blocks."""
    head, t = _head_from_golden(load_golden('clip_head_tiny'), DEV)
    first = int(t['first'])
    feats = {first: t['feat'], '%d_cls_token' % first: t['cls']}
    off = head(feats, [t['attn_bias']], normalize=True)
    before = _lib.CALLS.get('veon_query_attention', 0)
    head.hip_query = True
    sos = head(feats, [t['attn_bias']], normalize=True)
    # one call per TAIL block: the fixture has five blocks, the head owns those from
    # ``first`` = 2 on (test_rec_head_tail_blocks_on_mfma counts the same three)
    assert len(head.resblocks) == 3
    assert _lib.CALLS.get('veon_query_attention', 0) - before == len(head.resblocks)
    rel = ((sos - t['sos']).norm() / t['sos'].norm()).item()
    rel_off = ((off - t['sos']).norm() / t['sos'].norm()).item()
    print('clip_head_tiny sos: relative L2 %.3g native, %.3g with the switch off'
          % (rel, rel_off))
    assert rel < 2e-2, rel
    # clip_outputs are filled as without the switch
    outs_on, outs_off = {}, {}
    head(feats, [t['attn_bias']], normalize=True, clip_outputs=outs_on)
    head(feats, [t['attn_bias']], normalize=True, clip_outputs=outs_off, hip_query=False)
    assert set(outs_on) == set(outs_off)
    assert all(torch.equal(outs_on[k], outs_off[k]) for k in outs_on)


test_head_against_the_reference_vector_fp16 = fp16_twin(test_head_against_the_reference_vector)


@torch.no_grad()
def test_head_at_production_width(monkeypatch, flavour):
    """D 768, 12 heads, three tail blocks, 100 queries, 4 x 6 patches, two images.  Both
    errors against the fp64 run of the fp32 modules: the native query path, and the torch
    query path under autocast of the same half type (the same operands rounded to the same
    type; the factor 2 covers the other summation order and the half rounding of the
    weights -- the margin tests/test_optim_step.py gives torch's own error).
    Measured on MI355X (relative L2): bf16 native 2.99e-3, autocast 3.61e-3; fp16 native
    3.72e-4, autocast 4.59e-4."""
    D, heads, nblk, Q, hw, N = 768, 12, 3, 100, (4, 6), 2
    blocks = torch.nn.ModuleList(
        [clip_blocks.ResidualAttentionBlock(D, heads) for _ in range(nblk)])
    head = ClipRecHead(blocks, torch.nn.LayerNorm(D), torch.nn.Parameter(torch.zeros(D, 512)),
                       sos_token_num=Q)
    named_init_(head, 'rec_head_prod/')
    head.eval()
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(N, D, *hw, generator=g)
    cls = torch.randn(1, N, D, generator=g)
    bias = torch.randn(N, heads, Q, *hw, generator=g) * 3.0
    ref = head.double()({0: feat.double(), '0_cls_token': cls.double()}, [bias.double()])
    head = head.float().to(DEV)
    feats = {0: feat.to(DEV), '0_cls_token': cls.to(DEV)}

    def err(x):
        return ((x.double().cpu() - ref).norm() / ref.norm()).item()
    before = _lib.CALLS.get('veon_query_attention', 0)
    e_native = err(head(feats, [bias.to(DEV)], hip_query=True))
    assert _lib.CALLS.get('veon_query_attention', 0) - before == nblk
    layer = clip_blocks.cross_attn_layer

    def autocast_layer(*args):
        with torch.autocast('cuda', dtype=flavour):
            return layer(*args)
    monkeypatch.setattr(clip_blocks, 'cross_attn_layer', autocast_layer)
    e_autocast = err(head(feats, [bias.to(DEV)], hip_query=False))
    print('production-width head, %s: e_native %.3g, e_autocast %.3g'
          % (half.name(), e_native, e_autocast))
    assert e_native <= 2 * e_autocast, (e_native, e_autocast)


test_head_at_production_width_fp16 = fp16_twin(test_head_at_production_width)


# ------------------------------------------------------------------------------- the path
@torch.no_grad()
def test_path_with_the_native_recognition_head(flavour):
    """CLIP width 128 with 2 heads (head_dim 64).  With ``hip_rec_head`` the 2-D outputs
    stay within 3e-2 of the output range of the switch-off result
    (test_2d_branch_on_the_gpu's bound), ``mask_preds`` is equal, and the captured
    forward replays to the eager result bit for bit."""
    from veon_amd.models.veon_occ import VeonOccupancyPath
    grid = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
            'depth': [1.0, 13.0, 1.0]}
    torch.manual_seed(0)
    net = VeonOccupancyPath(
        input_size=(64, 96), num_cam=2, clip_width=128, clip_layers=4, clip_heads=2,
        clip_first_tail=2, clip_proj_dim=24, embed_dim=64, n_classes=5, occ_size=(4, 20, 20),
        hsa_dim=64, hsa_fusion_map=('0->1->1', '1->2->2'), grid_config=grid, bf16_heads=False,
        two_streams=False, clip_image=32,
        side_adapter=dict(image_size=64, width=48, depth=4, num_heads=3, num_queries=5,
                          fusion_map=('0->0', '1->1', '2->2'),
                          deep_supervision_idxs=(4,), embed_channels=16,
                          mlp_channels=24)).to(DEV).eval()
    images = torch.randn(1, 2, 3, 64, 96, device=DEV)
    off = net.forward_2d(images)
    before = _lib.CALLS.get('veon_query_attention', 0)
    net.hip_rec_head = True
    on = net.forward_2d(images)
    assert _lib.CALLS.get('veon_query_attention', 0) - before == 2     # two tail blocks
    assert set(on) == set(off)
    assert torch.equal(on['mask_preds'], off['mask_preds'])
    assert tuple(on['attn_biases'][0].shape) == (2, 2, 5, 2, 3)        # at the CLIP grid
    for k in ('mask_embs', 'mask_logits', 'sem_seg_ds', 'sem_embed_ds'):
        err = (on[k] - off[k]).abs().max().item()
        rng = max(1.0, off[k].abs().max().item())
        print('%s: max |on - off| %.3g of range %.3g' % (k, err, rng))
        assert err <= 3e-2 * rng, (k, err, rng)
    keys = ('mask_preds', 'mask_embs', 'mask_logits', 'sem_seg_ds', 'sem_embed_ds')
    graphed = GraphedCallable(lambda im: net.forward_2d(im), (images,))
    for _ in range(2):
        got = graphed(images)
        for k in keys:
            assert torch.equal(got[k], on[k]), k


test_path_with_the_native_recognition_head_fp16 = fp16_twin(
    test_path_with_the_native_recognition_head)
