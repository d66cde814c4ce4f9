"""Native training of the DINOv2 LoRA blocks (csrc/attention_train.hip)
on the MI355X: the attention forward with statistics, the attention backward, and
``Block.hip_train`` against the module's own definition.  Every test here calls the new
wrappers or the switch, so all of them fail on a tree without the feature.

Yardsticks (none of them taken from the code under test):
 * fp64 results computed from the SAME half-rounded operands;
 * the inference kernel (``vit_ops.attention``) for the training forward, to the bit;
 * torch's own half arithmetic of the same formula (attention) and the unmodified block
   under ``torch.autocast`` (blocks, encoder), each measured against the same fp64 result,
   with the project's factor 2 for "rounds the same quantities at the same places".

Shapes: the workgroup is 128 queries (dQ) / 128 keys (dK, dV), four waves of 32, and the
streamed tile is 64 rows, so the seams of the issue's table are the kernels' seams.
"""
import copy

import pytest
import torch

# LSE_BOUND, |lse - fp64| in log2 units, 2^-8 (bf16) / 2^-11 (fp16): stated once, next to the
# hostile cases that are held to it as well (tests/test_vit_train_hostile_gpu.py)
from tests.attention_train_refs import LSE_BOUND
from tests.helpers import flavour, fp16_twin, half_tol  # noqa: F401
from veon_amd import _lib, half, vit_ops
from veon_amd.models.depth_anything import dinov2
from veon_amd.models.depth_anything.dinov2 import Block, DinoVisionTransformer, LoRALinear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCALE = 0.125
FWD, BWD, WGRAD = 'veon_vit_attention_fwd_lse', 'veon_vit_attention_bwd', 'veon_linear_wgrad_bf16'
WORKLOAD = (6, 901, 16)
SHAPES = [(1, 1, 1),      # single token
          (1, 31, 1),     # under one tile
          (2, 33, 2),     # one past a wave's 32 rows
          (1, 64, 1),     # exact tile
          (2, 65, 3),     # one live row in the last streamed tile
          (1, 127, 2),    # one short of a 128-row workgroup
          (1, 129, 1),    # one past a 128-row workgroup
          (1, 200, 2),    # several tiles
          WORKLOAD]       # the workload's, computed once per flavour (_case)


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    Block.hip_train = False


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


def _counts(fn, names):
    before = dict(_lib.CALLS)
    fn()
    return tuple(_lib.CALLS.get(k, 0) - before.get(k, 0) for k in names)


_CASES = {}


def _case(B, T, H):
    """Operands, kernel results and references of one shape in the current flavour,
    computed once and shared (never modified) by the tests that need them.

    qkv: the raw output of a qkv Linear, N(0, 1) rounded to half.  q values below 2^-10 in
    magnitude are set to zero so that q / 8 is exact in fp16 too (no subnormal result):
    the premise of the bit-equality of the two forward forms."""
    key = (B, T, H, half.name())
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * B + 10 * T + H)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).to(half.dtype())
    q = qkv[:, :, 0]
    q[q.abs().float() < 2.0 ** -10] = 0
    qkv = qkv.view(B, T, 3 * H * 64).to(DEV)
    dout = torch.randn(B, T, H * 64, generator=g).to(half.dtype()).to(DEV)
    c = {'qkv': qkv, 'dout': dout}
    c['out'], c['lse'] = vit_ops.attention_fwd_lse(qkv, H, SCALE)
    # fp64 autograd of softmax(scale q k^T) v on the same half inputs
    x64 = qkv.double().requires_grad_(True)
    o64 = vit_ops.attention_ref(x64, H, SCALE)
    c['dqkv64'], = torch.autograd.grad(o64, x64, dout.double())
    q64, k64 = x64.detach().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)[:2]
    c['lse64'] = torch.logsumexp((q64 * SCALE) @ k64.transpose(-2, -1), -1) * vit_ops.LOG2E
    del x64, o64, q64, k64
    # the same formula by torch in the flavour's half dtype
    xh = qkv.clone().requires_grad_(True)
    c['dqkv_torch'], = torch.autograd.grad(vit_ops.attention_ref(xh, H, SCALE), xh, dout)
    del xh
    c['dqkv'] = vit_ops.attention_bwd(qkv, c['out'], dout, c['lse'], H, SCALE)
    if key[:3] != WORKLOAD:
        _CASES[key] = c
    else:                      # keep one workload case alive at a time
        for k in [k for k in _CASES if k[:3] == WORKLOAD]:
            del _CASES[k]
        _CASES[key] = c
    return c


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('B,T,H', SHAPES)
def test_forward_is_the_inference_kernel_and_lse_matches_fp64(B, T, H, flavour):
    """out is bit-equal to ``vit_ops.attention`` on the tensor with its q third times
    0.125 (a power of two: both forms round identically); lse against fp64 within 2^-8
    (bf16) / 2^-11 (fp16) log2 units."""
    c = _case(B, T, H)
    pre = c['qkv'].clone().view(B, T, 3, H, 64)
    pre[:, :, 0] *= SCALE
    assert torch.equal(pre[:, :, 0].float() * 8, c['qkv'].view(B, T, 3, H, 64)[:, :, 0].float())
    want = vit_ops.attention(pre.view(B, T, -1), H)
    assert c['out'].dtype == flavour and torch.equal(c['out'], want)
    Tp = vit_ops.attention_stats_len(T)
    assert Tp % 64 == 0 and T <= Tp < T + 64 and c['lse'].shape == (B, H, Tp)
    err = (c['lse'][:, :, :T].double() - c['lse64']).abs().max().item()
    print('lse %s %s: max |err| %.3e log2 units (bound %.3e)' %
          (half.name(), (B, T, H), err, LSE_BOUND[flavour]))
    assert err <= LSE_BOUND[flavour], err


test_forward_is_the_inference_kernel_and_lse_matches_fp64_fp16 = fp16_twin(
    test_forward_is_the_inference_kernel_and_lse_matches_fp64)


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize('B,T,H', SHAPES)
def test_backward_against_fp64(B, T, H, flavour):
    """Relative L2 error per third (dq, dk, dv) against fp64 autograd on the same half
    inputs: e(kernel) <= 2 e(torch), torch running the same formula in the half dtype.
    Then the same call with columns T.. of lse and of the workspace filled with large
    finite values of both signs, into a NaN-filled dqkv: bit-equal to the clean run and
    nothing of the fill left.

    A single token is the one case where a relative error is not defined: P = 1, so
    dS = P (dP - delta) and with it dq and dk are exactly zero in exact arithmetic (and in
    fp64, and in torch's half run, which subtracts a number from itself).  The kernel forms
    dP (matrix core) and delta (the delta pass) as two fp32 sums of the same 64 exact
    products dO_d v_d in different orders; each is within 64 * 2^-24 * A of the exact sum,
    A = sum_d |dO_d v_d|, so |dS| <= 2^-17 A and, after the half roundings of dS and of the
    result (and p within 2^-20 of 1), |dq_d| <= 1.02 * scale * |k_d| * 2^-17 * A, and dk
    the same with q_d.  There dq and dk are held to that bound elementwise; dv to
    e(kernel) <= 2 e(torch) as everywhere."""
    c = _case(B, T, H)
    assert c['dqkv'].dtype == flavour and c['dqkv'].shape == c['qkv'].shape
    for i, name in enumerate(('dq', 'dk', 'dv')):
        def third(t):
            return t.view(B, T, 3, H * 64)[:, :, i]
        if T == 1 and i < 2:
            assert float(third(c['dqkv64']).abs().max()) == 0.0
            q_, k_, v_ = (c['qkv'].view(B, T, 3, H, 64)[:, :, j].double() for j in range(3))
            A = (c['dout'].view(B, T, H, 64).double() * v_).abs().sum(-1, keepdim=True)
            other = k_ if i == 0 else q_
            bound = 1.02 * SCALE * other.abs() * 2.0 ** -17 * A
            got = c['dqkv'].view(B, T, 3, H, 64)[:, :, i].double().abs()
            print('attention bwd %s %s %s: max |%s| %.3e, largest share of the bound %.3f' %
                  (half.name(), (B, T, H), name, name, float(got.max()),
                   float((got / bound.clamp_min(1e-300)).max())))
            assert bool((got <= bound).all()), name
            continue
        e_k = _rel(third(c['dqkv']), third(c['dqkv64']))
        e_t = _rel(third(c['dqkv_torch']), third(c['dqkv64']))
        print('attention bwd %s %s %s: e(kernel) %.3e  e(torch) %.3e' %
              (half.name(), (B, T, H), name, e_k, e_t))
        assert e_k <= 2 * e_t, (name, e_k, e_t)
    Tp = c['lse'].shape[-1]
    lse = c['lse'].clone()
    ws = torch.zeros_like(lse)
    fill = torch.tensor([1e30, -1e30, 3e38, -3e38], device=DEV).repeat(16)[:Tp - T]
    lse[:, :, T:] = fill
    ws[:, :, T:] = fill
    dqkv = torch.full_like(c['qkv'], float('nan'))
    vit_ops.attention_bwd(c['qkv'], c['out'], c['dout'], lse, H, SCALE, dqkv=dqkv, workspace=ws)
    assert not bool(torch.isnan(dqkv).any())
    assert torch.equal(dqkv, c['dqkv'])


test_backward_against_fp64_fp16 = fp16_twin(test_backward_against_fp64)


def test_two_calls_at_the_workload_shape_are_bit_equal(flavour):
    c = _case(*WORKLOAD)
    H = WORKLOAD[2]
    out, lse = vit_ops.attention_fwd_lse(c['qkv'], H, SCALE)
    assert torch.equal(out, c['out']) and torch.equal(lse[..., :901], c['lse'][..., :901])
    assert torch.equal(vit_ops.attention_bwd(c['qkv'], out, c['dout'], lse, H, SCALE), c['dqkv'])


test_two_calls_at_the_workload_shape_are_bit_equal_fp16 = fp16_twin(
    test_two_calls_at_the_workload_shape_are_bit_equal)


def test_attention_train_saves_no_t_by_t_tensor(flavour):
    B, T, H = 2, 65, 3
    c = _case(B, T, H)
    x = c['qkv'].clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.shape) or t,
                                                  lambda t: t):
        out = vit_ops.attention_train(x, H, SCALE)
    assert sorted(tuple(s) for s in saved) == sorted([(B, T, 3 * H * 64), (B, T, H * 64),
                                                      (B, H, 128)])
    out.backward(c['dout'])
    assert torch.equal(x.grad, c['dqkv'])


# ------------------------------------------------------------------------------- blocks
def _round_weights_(mod, seed):
    """Non-trivial LayerNorm / LayerScale / bias values, random non-zero lora_B (at the zero
    init dA is exactly 0 and a ratio says nothing), and every matrix rounded to the half
    dtype, so that the native and the autocast run see the same operands."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith('lora_B'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif 'norm' in name and name.endswith('weight'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif name.endswith('gamma'):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            elif p.dim() == 2 and not name.endswith('lora_A'):
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            if p.dim() >= 2:
                p.copy_(p.to(half.dtype()).float())
    return mod


BLOCKS = {'lora4': lambda: Block(128, 2, init_values=1.0, lora_r=4),
          'full': lambda: Block(128, 2, lora_r=-1),     # every weight trainable
          'lora1': lambda: Block(64, 1, lora_r=1)}      # the Mlp has no LoRA (the `> 1` rule)


def _block(which):
    torch.manual_seed(3)
    return _round_weights_(BLOCKS[which](), seed=4).train()


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV), torch.randn(*shape, generator=g).to(DEV)


def _step(mod, x, G, how, call=None):
    """One forward + backward of a copy of ``mod``: {name: tensor} of the output, the input
    gradient and every parameter's gradient (None for a frozen one).  Only 'native' runs
    with the switch on; 'fp64' is the module's own definition on the CPU."""
    mod = copy.deepcopy(mod)
    Block.hip_train = how == 'native'
    if how == 'fp64':
        mod, x, G = mod.double().cpu(), x.double().cpu(), G.double().cpu()
    else:
        mod = mod.to(DEV)
    x = x.clone().requires_grad_(True)
    call = call or (lambda m, t: m(t))
    try:
        if how == 'autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                out = call(mod, x)
        else:
            out = call(mod, x)
        out.backward(G.to(out.dtype))
    finally:
        Block.hip_train = False
    result = {'out': out.detach(), 'dx': x.grad}
    result.update({'grad:' + k: p.grad for k, p in mod.named_parameters()})
    return result


def _compare_with_autocast(mod, x, G, call=None, only=None):
    """e = relative L2 error against the fp64 run of the module's own definition;
    e(native) <= 2 e(autocast) for the output, dx and every trainable parameter's gradient;
    frozen parameters get no gradient."""
    exact = _step(mod, x, G, 'fp64', call)
    nat = _step(mod, x, G, 'native', call)
    auto = _step(mod, x, G, 'autocast', call)
    assert set(nat) == set(exact) == set(auto)
    worst = []
    for k in sorted(exact):
        if exact[k] is None:
            assert nat[k] is None, k
            continue
        if only is not None and not only(k):
            continue
        want = exact[k].to(DEV)
        assert nat[k] is not None and nat[k].shape == want.shape, k
        assert nat[k].dtype == torch.float32, k
        e_n, e_a = _rel(nat[k], want), _rel(auto[k].to(DEV), want)
        print('%-34s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst))
    return nat


@pytest.mark.parametrize('which', sorted(BLOCKS))
def test_block_matches_the_module_definition(which, flavour):
    """One training step of the block on 2 x 65 tokens against the module's own definition
    in fp64; the autocast run is the unmodified block under torch.autocast."""
    blk = _block(which)
    x, G = _inputs((2, 65, blk.norm1.normalized_shape[0]), seed=7)
    before = dict(_lib.CALLS)
    nat = _compare_with_autocast(blk, x, G)
    assert _lib.CALLS.get(BWD, 0) - before.get(BWD, 0) == 1
    frozen = [k for k, v in nat.items() if v is None]
    lora = [m for m in blk.modules() if isinstance(m, LoRALinear) and m.r > 0]
    assert sorted(frozen) == sorted('grad:' + n + '.weight' for n, m in blk.named_modules()
                                    if m in lora)
    assert len(lora) == {'lora4': 4, 'full': 0, 'lora1': 2}[which]


test_block_matches_the_module_definition_fp16 = fp16_twin(test_block_matches_the_module_definition)


def test_call_counts(flavour, monkeypatch):
    """LoRA block: one attention forward + backward, no full-size weight gradient, eight
    rank-padded ones (two per LoRA Linear).  Fully trainable block: four full-size ones.
    Switch off: no new entry point is called and the step is bit-equal to plain torch."""
    shapes = []
    real = vit_ops.linear_wgrad

    def spy(dy, x, out=None):
        shapes.append((dy.shape[-1], x.shape[-1]))
        return real(dy, x, out)
    monkeypatch.setattr(vit_ops, 'linear_wgrad', spy)
    x, G = _inputs((2, 65, 128), seed=8)
    names = (FWD, BWD, WGRAD)
    assert Block.hip_train is False
    lora = _block('lora4')
    off = {}
    assert _counts(lambda: off.update(_step(lora, x, G, 'torch')), names) == (0, 0, 0)
    assert _counts(lambda: _step(lora, x, G, 'native'), names) == (1, 1, 8)
    assert sorted(shapes) == sorted([(384, 64), (64, 128), (128, 64), (64, 128),
                                     (512, 64), (64, 128), (128, 64), (64, 512)])
    del shapes[:]
    assert _counts(lambda: _step(_block('full'), x, G, 'native'), names) == (1, 1, 4)
    assert sorted(shapes) == sorted([(384, 128), (128, 128), (512, 128), (128, 512)])
    # eval mode and no_grad keep today's forward
    Block.hip_train = True
    blk = copy.deepcopy(lora).to(DEV)
    with torch.no_grad():
        assert _counts(lambda: blk(x), names) == (0, 0, 0)
    assert _counts(lambda: blk.eval()(x.clone().requires_grad_(True)), names) == (0, 0, 0)
    Block.hip_train = False

    def plain(m, t):     # the block's definition, written out
        t = t + m.ls1(m.attn(m.norm1(t)))
        return t + m.ls2(m.mlp(m.norm2(t)))
    want = _step(lora, x, G, 'torch', plain)
    for k in want:
        assert (want[k] is None and off[k] is None) or torch.equal(want[k], off[k]), k


# ------------------------------------------------------------------------ whole encoder
def _encoder():
    torch.manual_seed(5)
    enc = DinoVisionTransformer(img_size=112, patch_size=14, embed_dim=128, depth=2,
                                num_heads=2, init_values=1.0, lora_r=4)
    return _round_weights_(enc, seed=6).train()


def _taps(m, img):
    return torch.cat(m.get_intermediate_layers(img, 2), dim=-1)


def test_encoder_lora_gradients_and_optimizer_step(flavour):
    """A depth-2 encoder (d = 128, lora_r = 4, 2 x 65 tokens) through
    get_intermediate_layers under autograd: every LoRA gradient within
    e(native) <= 2 e(autocast) of fp64; two identical steps bit-equal (every output and
    gradient but those of ``patch_embed.proj``, torch's convolution backward); an AdamW step moves
    the LoRA parameters; .eval() merges and the native inference forward agrees with the
    torch eval forward (relative L2 <= 1e-2 in bf16, scaled by roundoff for fp16)."""
    enc = _encoder()
    g = torch.Generator().manual_seed(9)
    img = torch.randn(2, 3, 112, 112, generator=g).to(DEV)
    G = torch.randn(2, 64, 256, generator=g).to(DEV)
    before = dict(_lib.CALLS)
    a = _compare_with_autocast(enc, img, G, _taps, only=lambda k: 'lora' in k)
    assert _lib.CALLS.get(BWD, 0) - before.get(BWD, 0) == 2
    assert sum('lora' in k for k in a) == 16
    b = _step(enc, img, G, 'native', _taps)
    for k in a:
        if 'patch_embed.proj' in k:
            continue     # torch's own convolution backward (it stays torch): not bit-stable
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k

    enc = enc.to(DEV)
    lora = {k: p for k, p in enc.named_parameters() if 'lora' in k}
    old = {k: p.detach().clone() for k, p in lora.items()}
    opt = torch.optim.AdamW(lora.values(), lr=1e-2)
    Block.hip_train = True
    (_taps(enc, img) * G).sum().backward()
    Block.hip_train = False
    opt.step()
    for k, p in lora.items():
        assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        assert not torch.equal(p.detach(), old[k]), k
    enc.eval()
    assert all(m.merged for m in enc.modules() if isinstance(m, LoRALinear) and m.r > 0)
    with torch.no_grad():
        assert enc._use_hip(img)
        got = _taps(enc, img)
        enc.use_hip = False
        want = _taps(enc, img)
    rel = _rel(got, want)
    print('eval after the step %s: native vs torch relative L2 %.3e' % (half.name(), rel))
    assert rel <= half_tol(1e-2, 0)['rtol'], rel
    assert dinov2.Block.hip_train is False


test_encoder_lora_gradients_and_optimizer_step_fp16 = fp16_twin(
    test_encoder_lora_gradients_and_optimizer_step)
