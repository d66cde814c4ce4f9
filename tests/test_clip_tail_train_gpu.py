"""Native training of the CLIP tail (csrc/attention_train.hip with a dense additive bias,
DESIGN section 4t) on the MI355X: the biased attention forward with statistics, its
backward with dBias, ``ResidualAttentionBlock.hip_train`` and the recognition head's
``update_remaining_clip_feats`` under autograd.  Every test calls the new wrappers or the
switch, so all of them fail on a tree without the feature.

Yardsticks (none taken from the code under test):
 * fp64 closed forms (tests/clip_tail_train_refs.py, checked against fp64 autograd on the
   CPU) on the SAME half-rounded operands and the same fp32 bias;
 * torch's own half arithmetic of the same formula (``vit_ops.attention_bias_ref`` under
   autograd: q, k, v half, the bias fp32, added to the fp32-converted scores) and the
   unmodified modules under ``torch.autocast``, each measured against the same fp64
   result, with the project's factor 2: e(kernel) <= 2 e(torch);
 * the unbiased kernels (``attention_fwd_lse``) and the explicitly zero-bordered matrix,
   to the bit.

Shapes: 32 rows per wave, 128 per workgroup, 64-row streamed tiles, and odd bias row
strides (Tb = 65, 176, 199).
"""
import copy

import pytest
import torch

from tests import clip_tail_train_refs as refs
from tests.attention_train_refs import LSE_BOUND
from tests.helpers import flavour, fp16_twin  # noqa: F401
from veon_amd import _lib, half, vit_ops
from veon_amd.models.semantic_net.clip_blocks import ClipRecHead, ResidualAttentionBlock

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCALE = refs.SCALE
FWDB, BWDB = 'veon_vit_attention_bias_fwd_lse', 'veon_vit_attention_bias_bwd'
DS_ONLY = BWDB + ':ds_only'
WGRAD = 'veon_linear_wgrad_bf16'
WORKLOAD = (6, 177, 12, 1)
# (B, T, H, border) -> kind of bias
SHAPES = [(1, 1, 1, 0), (1, 1, 1, 1), (1, 2, 1, 1), (2, 33, 2, 1), (1, 64, 1, 0),
          (2, 66, 3, 1), (1, 129, 1, 0), (1, 200, 2, 1), WORKLOAD]
KIND = {(1, 200, 2, 1): 'heads'}       # head-broadcast: bias_sh = 0
HOSTILE = (2, 66, 3)


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    ResidualAttentionBlock.hip_train = False


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _counts(fn, names):
    before = dict(_lib.CALLS)
    fn()
    return tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in names)


def _operands(B, T, H, seed):
    """qkv as in tests/test_vit_train_gpu.py: N(0, 1) rounded to half, q below 2^-10 set to
    zero so that the scaled q is exact in fp16 too."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(half.dtype())
    q = qkv[:, :, 0]
    q[q.abs().float() < 2.0 ** -10] = 0
    dout = torch.randn(B, T, H * 64, generator=g).to(half.dtype())
    return qkv.view(B, T, 3 * H * 64).to(DEV), dout.to(DEV), g


def _torch_half(qkv, bias, dout, H, border):
    """(out, dqkv, dbias in the bias's shape) of the formula by torch's autograd in the
    flavour's half dtype, the bias fp32."""
    x = qkv.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    out = vit_ops.attention_bias_ref(x, b, H, SCALE, border)
    if b.numel() == 0:
        dx, = torch.autograd.grad(out, x, dout)
        return out.detach(), dx, torch.zeros_like(b)
    dx, db = torch.autograd.grad(out, (x, b), dout)
    return out.detach(), dx, db


_CASES = {}


def _case(B, T, H, border):
    """Operands, kernel results and references of one shape in the current flavour,
    computed once and shared (never modified) by the tests that need them."""
    key = (B, T, H, border, half.name())
    if key in _CASES:
        return _CASES[key]
    kind = KIND.get((B, T, H, border), 'full')
    qkv, dout, g = _operands(B, T, H, 1000 * B + 10 * T + H + border)
    bias = refs.gram_bias(B, T, H, border, kind, g).to(DEV)
    c = {'qkv': qkv, 'dout': dout, 'bias': bias, 'kind': kind}
    c['out'], c['lse'] = vit_ops.attention_bias_fwd_lse(qkv, bias, H, SCALE, border)
    c['dqkv'], c['dbias'] = vit_ops.attention_bias_bwd(qkv, bias, c['out'], dout, c['lse'], H,
                                                       SCALE, border)
    c['out64'], c['lse64'] = refs.forward(qkv.double(), bias.double(), H, border)
    c['dqkv64'], c['dbias64'] = refs.backward(qkv.double(), bias.double(), dout.double(), H,
                                              border)
    c['out_torch'], c['dqkv_torch'], c['dbias_torch'] = _torch_half(qkv, bias, dout, H, border)
    for k in [k for k in _CASES if k[:4] == WORKLOAD and key[:4] == WORKLOAD]:
        del _CASES[k]              # one workload case alive at a time
    _CASES[key] = c
    return c


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('B,T,H,border', SHAPES)
def test_forward_against_fp64_and_the_unbiased_kernel(B, T, H, border, flavour):
    """out within e(kernel) <= 2 e(torch half) of fp64, lse within LSE_BOUND; with a zero
    bias and no border, out and the live columns of lse are the unbiased kernel's to the
    bit; border = 1 is bit-equal to border = 0 on the explicitly zero-bordered matrix."""
    c = _case(B, T, H, border)
    Tp = vit_ops.attention_stats_len(T)
    assert c['out'].dtype == flavour and c['lse'].shape == (B, H, Tp)
    e_k, e_t = _rel(c['out'], c['out64']), _rel(c['out_torch'], c['out64'])
    err = (c['lse'][:, :, :T].double() - c['lse64']).abs().max().item()
    print('bias fwd %s %s: e(kernel) %.3e  e(torch) %.3e  lse max |err| %.3e (bound %.3e)' %
          (half.name(), (B, T, H, border), e_k, e_t, err, LSE_BOUND[flavour]))
    assert e_k <= 2 * e_t, (e_k, e_t)
    assert err <= LSE_BOUND[flavour], err
    zero = torch.zeros(B, H, T, T, device=DEV)
    out0, lse0 = vit_ops.attention_bias_fwd_lse(c['qkv'], zero, H, SCALE, 0)
    want, lse_w = vit_ops.attention_fwd_lse(c['qkv'], H, SCALE)
    assert torch.equal(out0, want) and torch.equal(lse0[..., :T], lse_w[..., :T])
    if border:
        padded = refs.full_bias(c['bias'], B, H, T, 1).contiguous()
        out1, lse1 = vit_ops.attention_bias_fwd_lse(c['qkv'], padded, H, SCALE, 0)
        assert torch.equal(out1, c['out']) and torch.equal(lse1[..., :T], c['lse'][..., :T])


test_forward_against_fp64_and_the_unbiased_kernel_fp16 = fp16_twin(
    test_forward_against_fp64_and_the_unbiased_kernel)


# ----------------------------------------------------------------------------- backward
def _check_gradients(c, B, T, H, border, tag):
    """dq, dk, dv and the dense dbias each within e(kernel) <= 2 e(torch half) of fp64.  At
    T = 1, P = 1 and dS = 0 exactly: dq, dk (and dbias) are held to the elementwise bound of
    tests/test_vit_train_gpu.py::test_backward_against_fp64, for the reason given there
    (dP and delta are two fp32 sums of the same 64 products in different orders:
    |dS| <= 2^-17 A, A = sum_d |dO_d v_d|).

    (1, 2, 1, 1) has a 1 x 1 bias matrix whose one dS is p_11 p_10 (dP_11 - dP_10) with
    p_10 about 1e-7 (the Gram diagonal is about 16): 1e-6 in fp64, below the fp32 spacing of
    dP_11 itself.  torch's fp32 softmax backward returns exactly 0 there (e = 1.000); the
    kernel measured 1.58 (bf16) and 1.00 (fp16).  It is held to the same rule as every
    other shape."""
    Tb = T - border
    for i, name in enumerate(('dq', 'dk', 'dv')):
        def third(t):
            return t.view(B, T, 3, H * 64)[:, :, i]
        if T == 1 and i < 2:
            assert float(third(c['dqkv64']).abs().max()) <= 1e-12     # zero but for fp64 order
            q_, k_, v_ = (c['qkv'].view(B, T, 3, H, 64)[:, :, j].double() for j in range(3))
            A = (c['dout'].view(B, T, H, 64).double() * v_).abs().sum(-1, keepdim=True)
            bound = 1.02 * SCALE * (k_ if i == 0 else q_).abs() * 2.0 ** -17 * A
            got = c['dqkv'].view(B, T, 3, H, 64)[:, :, i].double().abs()
            assert bool((got <= bound).all()), name
            continue
        e_k = _rel(third(c['dqkv']), third(c['dqkv64']))
        e_t = _rel(third(c['dqkv_torch']), third(c['dqkv64']))
        print('bias bwd %s %s %s %s: e(kernel) %.3e  e(torch) %.3e' %
              (tag, half.name(), (B, T, H, border), name, e_k, e_t))
        assert e_k <= 2 * e_t, (name, e_k, e_t)
    assert c['dbias'].shape == (B, H, Tb, Tb) and c['dbias'].dtype == torch.float32
    if Tb == 0:
        return
    if T == 1:
        assert float(c['dbias64'].abs().max()) <= 1e-12
        v_ = c['qkv'].view(B, T, 3, H, 64)[:, :, 2].double()
        A = (c['dout'].view(B, T, H, 64).double() * v_).abs().sum(-1)
        assert bool((c['dbias'].double().abs().view(B, H) <= 1.02 * 2.0 ** -17 * A.view(B, H)).all())
        return
    # the wrapper's view of it: summed over the broadcast axes, as torch's autograd sums
    got = refs.reduce_dbias(c['dbias'], c['bias'])
    want = refs.reduce_dbias(c['dbias64'], c['bias'])
    e_k, e_t = _rel(got, want), _rel(c['dbias_torch'], want)
    print('bias bwd %s %s %s dbias (%s): e(kernel) %.3e  e(torch) %.3e' %
          (tag, half.name(), (B, T, H, border), c['kind'], e_k, e_t))
    assert e_k <= 2 * e_t, ('dbias', e_k, e_t)


def _rerun_into_nan(c, H, border):
    """The same call with columns T.. of lse and of the workspace filled with large finite
    values of both signs, into NaN-filled dqkv and dbias: bit-equal to the clean run and no
    NaN left (every element is written, the padding is never read).  Then without dqkv
    (dbias bit-equal, counted as the dS-only form) and without dbias (dqkv bit-equal).
    The dS-only count is kept by the Python wrapper whenever it passes dqkv = NULL: it shows
    the wrapper's routing, not which kernels the C entry point then launches."""
    T = c['qkv'].shape[1]
    Tp = c['lse'].shape[-1]
    lse = c['lse'].clone()
    ws = torch.zeros_like(lse)
    fill = torch.tensor([1e30, -1e30, 3e38, -3e38], device=DEV).repeat(16)[:Tp - T]
    lse[:, :, T:] = fill
    ws[:, :, T:] = fill
    dqkv = torch.full_like(c['qkv'], float('nan'))
    dbias = torch.full_like(c['dbias'], float('nan'))
    args = (c['qkv'], c['bias'], c['out'], c['dout'], lse, H, SCALE, border)
    vit_ops.attention_bias_bwd(*args, dqkv=dqkv, dbias=dbias, workspace=ws)
    assert not bool(torch.isnan(dqkv).any()) and not bool(torch.isnan(dbias).any())
    assert torch.equal(dqkv, c['dqkv']) and torch.equal(dbias, c['dbias'])
    dbias.fill_(float('nan'))
    n = _counts(lambda: vit_ops.attention_bias_bwd(*args, dqkv=None, dbias=dbias,
                                                   workspace=ws.clone()), (BWDB, DS_ONLY))
    assert n == ((1, 1) if dbias.numel() else (0, 0))
    assert torch.equal(dbias, c['dbias'])
    dqkv.fill_(float('nan'))
    vit_ops.attention_bias_bwd(*args, dqkv=dqkv, dbias=None, workspace=ws)
    assert torch.equal(dqkv, c['dqkv'])


@pytest.mark.parametrize('B,T,H,border', SHAPES)
def test_backward_against_fp64(B, T, H, border, flavour):
    c = _case(B, T, H, border)
    assert c['dqkv'].dtype == flavour and c['dqkv'].shape == c['qkv'].shape
    _check_gradients(c, B, T, H, border, 'gram')
    _rerun_into_nan(c, H, border)


test_backward_against_fp64_fp16 = fp16_twin(test_backward_against_fp64)


def test_broadcast_biases_through_autograd(flavour):
    """``attention_bias_train`` with a head-broadcast (B, 1, Tb, Tb) bias given as an
    expanded view (zero stride), a (Tb, Tb) bias and a (B H, Tb, Tb) bias: the gradient
    comes back in the bias's own shape, within e <= 2 e(torch half) of fp64."""
    B, T, H, border = 2, 66, 3, 1
    Tb = T - border
    qkv, dout, g = _operands(B, T, H, 77)
    for kind in ('heads', 'matrix', 'flat'):
        bias = refs.gram_bias(B, T, H, border, 'full' if kind == 'flat' else kind, g).to(DEV)
        if kind == 'flat':
            bias = bias.reshape(B * H, Tb, Tb)
        b = bias.clone().requires_grad_(True)
        x = qkv.clone().requires_grad_(True)
        given = b.expand(B, H, Tb, Tb) if kind == 'heads' else b
        out = vit_ops.attention_bias_train(x, given, H, SCALE, border)
        out.backward(dout)
        assert b.grad.shape == bias.shape and b.grad.dtype == torch.float32
        d64, dense64 = refs.backward(qkv.double(), bias.double(), dout.double(), H, border)
        want = refs.reduce_dbias(dense64, bias)
        _, dx_t, db_t = _torch_half(qkv, bias, dout, H, border)
        e_k, e_t = _rel(b.grad, want), _rel(db_t, want)
        print('broadcast %s %s: dbias e(kernel) %.3e  e(torch) %.3e' % (kind, half.name(), e_k, e_t))
        assert e_k <= 2 * e_t, (kind, e_k, e_t)
        assert _rel(x.grad, d64) <= 2 * _rel(dx_t, d64)


test_broadcast_biases_through_autograd_fp16 = fp16_twin(test_broadcast_biases_through_autograd)


# -------------------------------------------------------------------------- hostile case
def _hostile(border):
    """(2, 66, 3): Gram bias with its diagonal scaled to about 60, keys 20..29 of every
    query masked, and query 40 of (b, h) = (1, 2) with every entry of its bias row masked.
    With border = 1 that query still sees the class token (bias 0 by index): it is live.
    With border = 0 the matrix is the zero-bordered one with that query's class-token
    entry masked too, so the query is FULLY masked: the header's contract applies."""
    B, T, H = HOSTILE
    qkv, dout, g = _operands(B, T, H, 4242)
    bias = refs.gram_bias(B, T, H, 1, 'full', g)
    idx = torch.arange(T - 1)
    bias[..., idx, idx] *= 60.0 / bias[..., idx, idx].mean()
    bias[..., :, 19:29] = refs.NEG
    bias[1, 2, 39, :] = refs.NEG
    if not border:
        bias = refs.full_bias(bias, B, H, T, 1).contiguous()
        bias[1, 2, 40, 0] = refs.NEG
    bias = bias.to(DEV)
    c = {'qkv': qkv, 'dout': dout, 'bias': bias, 'kind': 'full'}
    c['out'], c['lse'] = vit_ops.attention_bias_fwd_lse(qkv, bias, H, SCALE, border)
    c['dqkv'], c['dbias'] = vit_ops.attention_bias_bwd(qkv, bias, c['out'], dout, c['lse'], H,
                                                       SCALE, border)
    c['out64'], c['lse64'] = refs.forward(qkv.double(), bias.double(), H, border)
    c['dqkv64'], c['dbias64'] = refs.backward(qkv.double(), bias.double(), dout.double(), H,
                                              border)
    # e(torch) is torch's autograd in the half dtype, as at every other shape.  With
    # border = 1 nothing is NaN.  With border = 0 autograd is NaN throughout the (b, h) of
    # the fully masked query, so it runs on the problem with that query's dout zeroed and
    # one key opened for it (tests/test_clip_tail_train.py shows in fp64 that this is the
    # contract: the query then has dS = 0 and adds nothing to dk, dv); every other (b, h)
    # is untouched by that.  Its out row, v_0 there, is zero by the contract.
    if border:
        c['out_torch'], c['dqkv_torch'], c['dbias_torch'] = _torch_half(qkv, bias, dout, H, border)
        return c
    bias2, dout2 = bias.clone(), dout.clone()
    bias2[1, 2, 40, 0] = 0.0
    dout2.view(B, T, H, 64)[1, 40, 2] = 0
    c['out_torch'], c['dqkv_torch'], c['dbias_torch'] = _torch_half(qkv, bias2, dout2, H, border)
    c['out_torch'].view(B, T, H, 64)[1, 40, 2] = 0
    for k in ('out_torch', 'dqkv_torch', 'dbias_torch'):
        assert not bool(torch.isnan(c[k].float()).any()), k
    return c


@pytest.mark.parametrize('border', [1, 0])
def test_hostile_bias(border, flavour):
    B, T, H = HOSTILE
    c = _hostile(border)
    for k in ('out', 'lse', 'dqkv', 'dbias'):
        t = c[k][..., :T] if k == 'lse' else c[k]
        assert not bool(torch.isnan(t.float()).any()), k
    live = torch.ones(B, H, T, dtype=torch.bool, device=DEV)
    if not border:
        live[1, 2, 40] = False
        # the fully masked query: out row zero, lse +inf, dq row zero, dbias row zero
        assert float(c['lse'][1, 2, 40]) == float('inf')
        assert float(c['out'].view(B, T, H, 64)[1, 40, 2].float().abs().max()) == 0.0
        assert float(c['dqkv'].view(B, T, 3, H, 64)[1, 40, 0, 2].float().abs().max()) == 0.0
        assert float(c['dbias'][1, 2, 40].abs().max()) == 0.0
    assert bool(torch.isfinite(c['lse'][..., :T][live]).all())
    err = (c['lse'][..., :T].double() - c['lse64'])[live].abs().max().item()
    assert err <= LSE_BOUND[flavour], err
    # masked keys: exactly zero dbias (in the zero-bordered matrix the class token's own
    # row 0 is not masked)
    masked = c['dbias'][..., :, 19:29] if border else c['dbias'][..., 1:, 20:30]
    assert float(masked.abs().max()) == 0.0
    assert _rel(c['out'], c['out64']) <= 2 * _rel(c['out_torch'], c['out64'])
    # dk, dv of the masked (b, h) carry nothing of the dead query: part of the bound below
    _check_gradients(c, B, T, H, border, 'hostile')
    _rerun_into_nan(c, H, border)


test_hostile_bias_fp16 = fp16_twin(test_hostile_bias)


# ----------------------------------------------------------------- determinism, storage
def test_two_calls_at_the_workload_shape_are_bit_equal(flavour):
    B, T, H, border = WORKLOAD
    c = _case(*WORKLOAD)
    out, lse = vit_ops.attention_bias_fwd_lse(c['qkv'], c['bias'], H, SCALE, border)
    assert torch.equal(out, c['out']) and torch.equal(lse[..., :T], c['lse'][..., :T])
    dqkv, dbias = vit_ops.attention_bias_bwd(c['qkv'], c['bias'], out, c['dout'], lse, H, SCALE,
                                             border)
    assert torch.equal(dqkv, c['dqkv']) and torch.equal(dbias, c['dbias'])


test_two_calls_at_the_workload_shape_are_bit_equal_fp16 = fp16_twin(
    test_two_calls_at_the_workload_shape_are_bit_equal)


def test_attention_bias_train_saves_no_other_t_by_t_tensor(flavour):
    B, T, H, border = 2, 66, 3, 1
    c = _case(B, T, H, border)
    x = c['qkv'].clone().requires_grad_(True)
    b = c['bias'].clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.shape) or t,
                                                  lambda t: t):
        out = vit_ops.attention_bias_train(x, b, H, SCALE, border)
    assert sorted(tuple(s) for s in saved) == sorted(
        [(B, T, 3 * H * 64), (B, T, H * 64), (B, H, 128), (B, H, T - 1, T - 1)])
    out.backward(c['dout'])
    assert torch.equal(x.grad, c['dqkv']) and torch.equal(b.grad, c['dbias'])


# -------------------------------------------------------------------------------- block
def _round_weights_(mod, seed):
    """Non-trivial LayerNorm weights and biases, every matrix rounded to the half dtype so
    that the native and the autocast run see the same operands."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.startswith('ln_') and name.endswith('weight'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            if p.dim() >= 2:
                p.copy_(p.to(half.dtype()).float())
    return mod


def _block_step(blk, x, mask, G, how, x_grad=True, frozen=False):
    """One forward + backward of a copy of ``blk`` on x (L, N, D) with the additive mask
    (N, H, Lb, Lb): 'native' hands the mask over as it is; the torch runs build the
    (N H, L, L) mask the module takes (``ClipRecHead.build_attn_bias`` when bordered)."""
    blk = copy.deepcopy(blk)
    L = x.shape[0]
    ResidualAttentionBlock.hip_train = how == 'native'
    if how == 'fp64':
        blk, x, mask, G = blk.double().cpu(), x.double().cpu(), mask.double().cpu(), G.double().cpu()
    else:
        blk = blk.to(DEV)
    for p in blk.parameters():
        p.requires_grad_(not frozen)
    x = x.clone().requires_grad_(x_grad)
    m = mask.clone().requires_grad_(True)
    try:
        if how == 'native':
            out = blk(x, attn_mask=m)
        else:
            full = m.reshape(-1, L, L) if m.shape[-1] == L else ClipRecHead.build_attn_bias(m)
            if how == 'autocast':
                with torch.autocast('cuda', dtype=half.dtype()):
                    out = blk(x, attn_mask=full)
            else:
                out = blk(x, attn_mask=full)
        out.backward(G.to(out.dtype))
    finally:
        ResidualAttentionBlock.hip_train = False
    res = {'out': out.detach(), 'dx': x.grad, 'dmask': m.grad}
    res.update({'grad:' + k: p.grad for k, p in blk.named_parameters()})
    return res


def _block_case(D, heads, quick, border, seed=31):
    torch.manual_seed(seed)
    blk = _round_weights_(ResidualAttentionBlock(D, heads, quick_gelu=quick), seed + 1)
    L, N = 21, 2
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(L, N, D, generator=g).to(DEV)
    G = torch.randn(L, N, D, generator=g).to(DEV)
    mask = refs.gram_bias(N, L, heads, border, 'full', g).to(DEV)
    return blk, x, mask, G


@pytest.mark.parametrize('border', [1, 0])
@pytest.mark.parametrize('quick', [True, False])
@pytest.mark.parametrize('D,heads', [(128, 2), (768, 12)])
def test_block_matches_the_module_definition(D, heads, quick, border, flavour):
    """One training step of the block on 2 x 21 tokens with a Gram-shaped mask that requires
    a gradient, against an fp64 copy of the module: e(native) <= 2 e(autocast) for the
    output, dx, dmask and every parameter's gradient."""
    blk, x, mask, G = _block_case(D, heads, quick, border)
    exact = _block_step(blk, x, mask, G, 'fp64')
    n = _counts(lambda: exact.update(native=_block_step(blk, x, mask, G, 'native')),
                (FWDB, BWDB, DS_ONLY, WGRAD))
    assert n == (1, 1, 0, 4)
    nat = exact.pop('native')
    auto = _block_step(blk, x, mask, G, 'autocast')
    assert set(nat) == set(exact) == set(auto)
    worst = []
    for k in sorted(exact):
        want = exact[k].to(DEV)
        assert nat[k] is not None and nat[k].shape == want.shape and nat[k].dtype == torch.float32, k
        e_n, e_a = _rel(nat[k], want), _rel(auto[k], want)
        print('%-28s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst))


test_block_matches_the_module_definition_fp16 = fp16_twin(test_block_matches_the_module_definition)


def test_frozen_block_launches_no_weight_gradient(flavour):
    """Frozen weights: no weight gradient and no launch for one; when x needs no gradient
    either (the first tail block of the real step), the attention backward runs in its
    dS-only form (dqkv = None) and the mask's gradient is bit-equal to the full call's."""
    blk, x, mask, G = _block_case(128, 2, True, 1)
    res = {}
    n = _counts(lambda: res.update(a=_block_step(blk, x, mask, G, 'native', frozen=True)),
                (FWDB, BWDB, DS_ONLY, WGRAD))
    assert n == (1, 1, 0, 0)
    assert all(v is None for k, v in res['a'].items() if k.startswith('grad:'))
    n = _counts(lambda: res.update(b=_block_step(blk, x, mask, G, 'native', x_grad=False,
                                                 frozen=True)), (FWDB, BWDB, DS_ONLY, WGRAD))
    assert n == (1, 1, 1, 0)
    assert res['b']['dx'] is None and torch.equal(res['b']['dmask'], res['a']['dmask'])


# ------------------------------------------------------------------------ reference pin
def _head_step(how, seed=0):
    """``update_remaining_clip_feats`` of the head built from tests/golden/clip_head_tiny.npz
    under autograd, the three biases requiring a gradient -> (clip_feat_proj, [dbias])."""
    from tests.conftest import load_golden
    from tests.test_clip_blocks import _head_from_golden
    head, t = _head_from_golden(load_golden('clip_head_tiny'), 'cpu' if how == 'fp64' else DEV)
    if how == 'fp64':
        head = head.double()
        t = {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()}
    first = int(t['first'])
    outs = {first: t['feat'].clone(), '%d_cls_token' % first: t['cls'].clone()}
    attns = [t['attn_%d' % i].clone().requires_grad_(True) for i in range(3)]
    G = torch.randn(t['clip_feat_proj'].shape, generator=torch.Generator().manual_seed(5))
    ResidualAttentionBlock.hip_train = how == 'native'
    try:
        if how == 'autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                head.update_remaining_clip_feats(outs, t['offsets'], attns)
        else:
            head.update_remaining_clip_feats(outs, t['offsets'], attns)
        got = outs['clip_feat_proj']
        (got.to(G.dtype if how != 'fp64' else torch.float64)
         * G.to(got.device, torch.float64 if how == 'fp64' else G.dtype)).sum().backward()
    finally:
        ResidualAttentionBlock.hip_train = False
    return got.detach(), [a.grad for a in attns], t['clip_feat_proj']


def test_rec_head_tail_trains_natively(flavour):
    """The recognition head of the reference's own vectors with the switch on: the three
    tail blocks run ``veon_vit_attention_bias_fwd_lse`` (the patch-to-patch biases go in
    with border = 1, ``build_attn_bias`` is not called), clip_feat_proj is within the 2e-2
    relative L2 that ``test_rec_head_tail_blocks_on_mfma`` holds the inference kernels to,
    the bias gradients are within e(native) <= 2 e(autocast) of an fp64 run of the torch
    path, and two identical steps give bit-equal gradients.  Switch off: the same call
    makes no call to the new entry points."""
    res = {}
    n = _counts(lambda: res.update(nat=_head_step('native')), (FWDB, BWDB))
    assert n == (3, 3)
    got, grads, want = res['nat']
    rel = _rel(got, want.to(DEV))
    print('clip_feat_proj %s: relative L2 %.3e' % (half.name(), rel))
    assert rel < 2e-2, rel
    _, exact, _ = _head_step('fp64')
    n = _counts(lambda: res.update(auto=_head_step('autocast')), (FWDB, BWDB, DS_ONLY))
    assert n == (0, 0, 0)
    for i, (g_n, g_a, g_e) in enumerate(zip(grads, res['auto'][1], exact)):
        assert g_n.shape == g_e.shape and g_n.dtype == torch.float32
        e_n, e_a = _rel(g_n, g_e.to(DEV)), _rel(g_a, g_e.to(DEV))
        print('dbias %d %s: e(native) %.3e  e(autocast) %.3e' % (i, half.name(), e_n, e_a))
        assert e_n <= 2 * e_a, (i, e_n, e_a)
    _, again, _ = _head_step('native')
    for a, b in zip(grads, again):
        assert torch.equal(a, b)


test_rec_head_tail_trains_natively_fp16 = fp16_twin(test_rec_head_tail_trains_natively)


def test_switch_off_calls_no_new_entry_point(flavour):
    assert ResidualAttentionBlock.hip_train is False
    n = _counts(lambda: _head_step('torch'), (FWDB, BWDB, DS_ONLY, 'veon_quickgelu_bf16'))
    assert n == (0, 0, 0, 0)
    blk, x, mask, G = _block_case(128, 2, True, 1)
    n = _counts(lambda: _block_step(blk, x, mask, G, 'torch'), (FWDB, BWDB, DS_ONLY))
    assert n == (0, 0, 0)


def test_switch_on_still_rejects_what_the_kernels_do_not_take(flavour):
    """On the GPU with the switch on, where a plain block with a floating mask passes
    ``_hip_train_ok``: a bool mask, D = 96 (head dim 48) and dropout > 0 are each rejected
    and run torch's lines, with no call to the new entry points."""
    ResidualAttentionBlock.hip_train = True
    L, N = 5, 2
    g = torch.Generator().manual_seed(21)

    def mk(D):
        return (ResidualAttentionBlock(D, 2).to(DEV),
                torch.randn(L, N, D, generator=g).to(DEV).requires_grad_(True))
    blk, x = mk(128)
    assert blk._hip_train_ok(x, torch.randn(N * 2, L, L, generator=g).to(DEV)) is True
    assert blk._hip_train_ok(x, None) is True
    boolm = (torch.rand(L, L, generator=g) > 0.7).fill_diagonal_(False).to(DEV)
    drop, _ = mk(128)
    drop.attn.dropout = 0.1
    b96, x96 = mk(96)
    for name, b, t, m in (('bool mask', blk, x, boolm), ('dropout', drop, x, None),
                          ('D = 96', b96, x96, torch.randn(L, L, generator=g).to(DEV))):
        assert b._hip_train_ok(t, m) is False, name
        n = _counts(lambda: b(t, attn_mask=m).sum().backward(),
                    (FWDB, BWDB, 'veon_vit_attention_fwd_lse', 'veon_quickgelu_bf16'))
        assert n == (0, 0, 0, 0), name


def test_quickgelu_pair_against_fp64(flavour):
    """h and dy of the QuickGELU pair against fp64 from the same half values:
    e(kernel) <= 2 e(torch half)."""
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(130, 256, generator=g) * 2).to(half.dtype()).to(DEV)
    dh = torch.randn(130, 256, generator=g).to(half.dtype()).to(DEV)
    h64, d64 = refs.quickgelu(y.double()), refs.quickgelu_bwd(dh.double(), y.double())
    e_k, e_t = _rel(vit_ops.quickgelu(y), h64), _rel(refs.quickgelu(y), h64)
    assert e_k <= 2 * e_t, (e_k, e_t)
    e_k, e_t = _rel(vit_ops.quickgelu_bwd(dh, y), d64), _rel(refs.quickgelu_bwd(dh, y), d64)
    assert e_k <= 2 * e_t, (e_k, e_t)


test_quickgelu_pair_against_fp64_fp16 = fp16_twin(test_quickgelu_pair_against_fp64)
