"""The attention of training (csrc/attention_train.hip) on the MI355X
away from N(0, 1): saturated rows, one massive-activation token, a large common component
in v or in dout, a uniform softmax, and heads of one call in different regimes
(``operands`` of tests/attention_train_refs.py).  The backward rebuilds
p = exp2(s c - lse) from the stored lse without a clamp and subtracts delta, taken from the
half-rounded O, from dp: on these operands the subtraction cancels.

Yardsticks (none of them taken from the code under test):
 * the inference kernel for the forward, to the bit, and fp64 for lse (LSE_BOUND);
 * fp64 autograd on the same half operands, with torch's half autograd of the same
   formula measured against it: e(kernel) <= 2 e(torch), the project's rule, wherever a
   relative error is defined (``checks``);
 * the elementwise bound of ``attention_train_refs.elementwise_bound``, computed in fp64
   from the inputs, on every element of every case;
 * exact properties: slices do not see each other, a NaN stays in its slice, the backward
   is linear in dout to the bit (bf16).
The emulation (``attention_train_refs.emulate``, the kernel's rounding points in torch) is
printed next to the kernel: it separates "the formulation is this inaccurate here" from
"the kernel is wrong".
"""
import pytest
import torch

from tests import attention_train_refs as ar
from tests.helpers import flavour, fp16_twin  # noqa: F401
from veon_amd import half, vit_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCALE = ar.SCALE
_IDS = ['%s-%d' % c for c in ar.CASES]
_CASES = {}


def _case(name, T):
    """Operands, kernel results and references of one case in the current flavour, computed
    once and shared (never modified) by the tests that need them."""
    key = (name, T, half.name())
    if key in _CASES:
        return _CASES[key]
    H = ar.heads_of(name)
    qkv, dout = (t.to(DEV) for t in ar.operands(name, T, half.dtype()))
    c = {'H': H, 'qkv': qkv, 'dout': dout}
    c['out'], c['lse'] = vit_ops.attention_fwd_lse(qkv, H, SCALE)
    c['dqkv'] = vit_ops.attention_bwd(qkv, c['out'], dout, c['lse'], H, SCALE)
    c['parts'] = ar.fp64_parts(qkv, dout, H)
    c['torch'] = ar.autograd(qkv, dout, H, half.dtype())
    c['emu'] = ar.emulate(qkv, dout, H)
    _CASES[key] = c
    return c


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('name,T', ar.CASES, ids=_IDS)
def test_forward_on_hostile_data(name, T, flavour):
    """out is bit-equal to ``vit_ops.attention`` on the tensor with its q third times 0.125
    (exact: ``operands`` zeroes the q values that would go subnormal); lse is within
    LSE_BOUND of fp64 (the bound's derivation does not depend on the data); and out against
    fp64: e(kernel) <= 2 e(torch half), per head of 'mixed', where ``checks`` has a
    relative third.

    Measured on an MI355X: lse errs by at most 2.9e-5 log2 units in either flavour (onehot,
    where lse is about 100: fp32 roundoff), 1.5e-5 on big4, under 1e-5 elsewhere.  This is
    the test that found the lse of saturated rows outside its bound while the row sum was
    the matrix core's, of the half-rounded weights: 3.95e-3 (big4-65), 5.25e-3 (big4-129),
    4.69e-3 (mixed) against 2^-8 = 3.91e-3 in bf16, 5.8e-4 and 5.2e-4 against 2^-11 = 4.9e-4
    in fp16, the emulation at 1.8e-3 / 2.2e-4 (the largest weight of a row is
    rounded at up to 2^8, not at 1).  out, e(kernel) / e(torch): 0.09 - 0.12 on big4 and head
    0 of mixed, 0.51 - 0.65 on outlier8, doffset16 and head 1 of mixed, 0.97 - 1.00 on
    voffset8 and samekeys; e(emulation) equals e(kernel) to 4 % everywhere."""
    c = _case(name, T)
    H, B = c['H'], ar.B
    pre = c['qkv'].clone().view(B, T, 3, H, 64)
    pre[:, :, 0] *= SCALE
    assert torch.equal(pre[:, :, 0].float() * 8, c['qkv'].view(B, T, 3, H, 64)[:, :, 0].float())
    want = vit_ops.attention(pre.view(B, T, -1), H)
    assert c['out'].dtype == flavour and torch.equal(c['out'], want)
    assert bool(torch.isfinite(c['lse'][:, :, :T]).all())
    err = (c['lse'][:, :, :T].double() - c['parts']['lse']).abs().max().item()
    err_e = (c['emu'][1].double() - c['parts']['lse']).abs().max().item()
    print('lse %s %s-%d: max |err| kernel %.3e, emulation %.3e log2 units (bound %.3e)' %
          (half.name(), name, T, err, err_e, ar.LSE_BOUND[flavour]))
    assert err <= ar.LSE_BOUND[flavour], err
    rel_heads = sorted({h for h, _, kind in ar.checks(name) if kind == 'rel'},
                       key=lambda h: -1 if h is None else h)
    for head in rel_heads:
        o64 = ar.pick(c['parts']['O'], head)
        e_k = ar.rel_l2(ar.pick(ar.heads(c['out'], H), head), o64)
        e_t = ar.rel_l2(ar.pick(ar.heads(c['torch'][0], H), head), o64)
        e_e = ar.rel_l2(ar.pick(ar.heads(c['emu'][0], H), head), o64)
        print('attention fwd %s %s-%d head %s: e(kernel) %.3e  e(torch) %.3e  e(emulation) %.3e'
              % (half.name(), name, T, head, e_k, e_t, e_e))
        assert e_k <= 2 * e_t, (head, e_k, e_t)


test_forward_on_hostile_data_fp16 = fp16_twin(test_forward_on_hostile_data)


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize('name,T', ar.CASES, ids=_IDS)
def test_backward_on_hostile_data(name, T, flavour):
    """Nothing in dqkv is non-finite.  Where ``checks`` says 'rel' (big4, outlier8,
    voffset8, doffset16, heads 0 and 1 of mixed, dk and dv of samekeys): relative L2 per
    third against fp64 autograd on the same half operands, e(kernel) <= 2 e(torch half).

    Everywhere, the saturated rows (onehot, head 2 of mixed) and the exactly-zero dq of
    samekeys included, where a relative error is not defined (the true dq and dk are 1e-9 of
    the operands; the emulation's relative error is about 2e3): every element within
    ``elementwise_bound``.  With u = 2^-9 (bf16) / 2^-12 (fp16), eps_l = LSE_BOUND ln 2 and
    the fp64 P, O, dP, delta, dS:
        E_delta[i]  = (u + 64 2^-24) sum_d |dO[i,d] O[i,d]|        delta from the rounded O
        dS_err[i,j] = P[i,j] ((eps_l + 2u) |dP[i,j] - delta[i]| + 1.01 E_delta[i])
                      + 2^-25 in fp16: half the spacing of a subnormal stored ds
        |dq_err| <= scale dS_err @ |k|   + u |dq| + T 2^-24 scale (|dS| @ |k|)
        |dk_err| <= scale dS_err^T @ |q| + u |dk| + T 2^-24 scale (|dS|^T @ |q|)
        |dv_err| <= (eps_l + 2u) (P^T @ |dO|) + u |dv|
                      + 2^-25 sum_i |dO[i]| in fp16: the stored p is subnormal below 2^-14
    (p = exp2(s c - lse) errs by the error of lse; the products are linear in dS_err and
    add fp32 accumulation and the result's rounding).  No constant of it is fitted to the
    kernel; the CPU file holds the emulation to the same bound.

    Measured on an MI355X, e(kernel) / e(torch) / e(emulation) (saturated and degenerate
    thirds: the largest |kernel| and |fp64| entry instead) and the kernel's largest share
    of the bound; the emulation's share differs from the kernel's by at most 0.07.  The
    largest e(kernel) / e(torch) is 1.26 (outlier8-65 dq, fp16), the largest share 0.81:
      case              bf16                            fp16                            share bf16, fp16
      big4-65       dq  5.66e-03 / 3.22e-02 / 5.66e-03  8.85e-04 / 6.47e-03 / 8.86e-04  0.453, 0.431
      big4-65       dk  5.59e-03 / 3.34e-02 / 5.59e-03  8.45e-04 / 6.53e-03 / 8.46e-04  0.486, 0.539
      big4-65       dv  1.92e-03 / 1.23e-02 / 1.92e-03  2.49e-04 / 1.85e-03 / 2.49e-04  0.763, 0.740
      big4-129      dq  6.62e-03 / 4.86e-02 / 6.57e-03  8.13e-04 / 5.32e-03 / 8.16e-04  0.566, 0.472
      big4-129      dk  6.27e-03 / 4.71e-02 / 6.23e-03  7.87e-04 / 5.36e-03 / 7.85e-04  0.542, 0.518
      big4-129      dv  1.97e-03 / 1.63e-02 / 1.97e-03  2.51e-04 / 1.89e-03 / 2.51e-04  0.808, 0.773
      outlier8-65   dq  5.49e-03 / 5.46e-03 / 5.49e-03  8.22e-04 / 6.53e-04 / 8.22e-04  0.497, 0.594
      outlier8-65   dk  5.30e-03 / 5.53e-03 / 5.30e-03  7.50e-04 / 6.76e-04 / 7.50e-04  0.299, 0.319
      outlier8-65   dv  2.06e-03 / 2.81e-03 / 2.06e-03  2.46e-04 / 3.21e-04 / 2.46e-04  0.368, 0.422
      outlier8-129  dq  7.44e-03 / 7.18e-03 / 7.44e-03  9.55e-04 / 8.91e-04 / 9.53e-04  0.599, 0.673
      outlier8-129  dk  7.69e-03 / 7.15e-03 / 7.69e-03  9.12e-04 / 9.36e-04 / 9.14e-04  0.309, 0.364
      outlier8-129  dv  2.02e-03 / 2.44e-03 / 2.02e-03  2.88e-04 / 3.45e-04 / 2.88e-04  0.365, 0.336
      outlier8-200  dq  8.11e-03 / 7.12e-03 / 8.14e-03  8.91e-04 / 9.19e-04 / 8.89e-04  0.676, 0.583
      outlier8-200  dk  7.23e-03 / 7.07e-03 / 7.28e-03  9.06e-04 / 8.68e-04 / 8.94e-04  0.268, 0.252
      outlier8-200  dv  1.99e-03 / 2.85e-03 / 2.03e-03  2.53e-04 / 3.70e-04 / 2.53e-04  0.354, 0.303
      voffset8-65   dq  1.78e-02 / 1.99e-02 / 1.78e-02  2.30e-03 / 2.27e-03 / 2.31e-03  0.233, 0.298
      voffset8-65   dk  1.64e-02 / 2.03e-02 / 1.63e-02  2.09e-03 / 2.27e-03 / 2.10e-03  0.151, 0.142
      voffset8-65   dv  2.27e-03 / 3.82e-03 / 2.27e-03  2.90e-04 / 4.74e-04 / 2.90e-04  0.358, 0.352
      voffset8-129  dq  1.94e-02 / 2.10e-02 / 1.96e-02  2.54e-03 / 2.57e-03 / 2.51e-03  0.270, 0.230
      voffset8-129  dk  1.51e-02 / 2.11e-02 / 1.52e-02  1.94e-03 / 2.60e-03 / 1.91e-03  0.117, 0.121
      voffset8-129  dv  2.34e-03 / 4.10e-03 / 2.34e-03  2.97e-04 / 5.13e-04 / 2.97e-04  0.328, 0.344
      doffset16-129 dq  2.46e-03 / 4.83e-03 / 2.47e-03  3.04e-04 / 6.10e-04 / 3.04e-04  0.367, 0.383
      doffset16-129 dk  2.08e-03 / 3.69e-03 / 2.08e-03  2.57e-04 / 4.71e-04 / 2.57e-04  0.277, 0.262
      doffset16-129 dv  1.71e-03 / 1.78e-03 / 1.71e-03  2.15e-04 / 2.22e-04 / 2.15e-04  0.506, 0.530
      onehot-65     dq  |k| 1.5e-06, |fp64| 9.5e-12     |k| 4.1e-06, |fp64| 1.0e-11     0.000, 0.000
      onehot-65     dk  |k| 1.5e-06, |fp64| 9.3e-12     |k| 4.1e-06, |fp64| 9.8e-12     0.216, 0.000
      onehot-65     dv  |k| 4.1e+00, |fp64| 4.1e+00     |k| 4.1e+00, |fp64| 4.1e+00     0.000, 0.000
      onehot-129    dq  |k| 2.0e-06, |fp64| 2.7e-08     |k| 3.0e-06, |fp64| 2.8e-08     0.000, 0.002
      onehot-129    dk  |k| 2.0e-06, |fp64| 2.3e-08     |k| 3.0e-06, |fp64| 2.4e-08     0.285, 0.000
      onehot-129    dv  |k| 4.2e+00, |fp64| 4.2e+00     |k| 4.2e+00, |fp64| 4.2e+00     0.000, 0.000
      samekeys-129  dq  |k| 2.4e-03, |fp64| 5.9e-16     |k| 2.8e-04, |fp64| 5.8e-16     0.100, 0.095
      samekeys-129  dk  2.36e-03 / 3.30e-03 / 2.36e-03  2.93e-04 / 4.24e-04 / 2.93e-04  0.207, 0.204
      samekeys-129  dv  1.53e-03 / 1.53e-03 / 1.53e-03  2.32e-04 / 2.32e-04 / 2.32e-04  0.075, 0.100
      mixed-129 h0  dq  5.50e-03 / 4.12e-02 / 5.56e-03  6.87e-04 / 4.47e-03 / 7.00e-04  0.417, 0.411
      mixed-129 h0  dk  5.26e-03 / 4.10e-02 / 5.45e-03  6.65e-04 / 4.64e-03 / 6.76e-04  0.547, 0.503
      mixed-129 h0  dv  1.95e-03 / 1.57e-02 / 1.95e-03  2.51e-04 / 1.94e-03 / 2.51e-04  0.728, 0.733
      mixed-129 h1  dq  2.49e-03 / 4.75e-03 / 2.49e-03  3.05e-04 / 5.93e-04 / 3.05e-04  0.288, 0.311
      mixed-129 h1  dk  2.40e-03 / 4.65e-03 / 2.40e-03  2.96e-04 / 5.87e-04 / 2.96e-04  0.346, 0.279
      mixed-129 h1  dv  2.34e-03 / 4.24e-03 / 2.34e-03  2.94e-04 / 5.07e-04 / 2.94e-04  0.360, 0.305
      mixed-129 h2  dq  |k| 2.7e-06, |fp64| 8.2e-10     |k| 2.2e-06, |fp64| 8.0e-10     0.000, 0.000
      mixed-129 h2  dk  |k| 2.7e-06, |fp64| 7.2e-10     |k| 2.2e-06, |fp64| 6.9e-10     0.234, 0.000
      mixed-129 h2  dv  |k| 4.1e+00, |fp64| 4.1e+00     |k| 4.1e+00, |fp64| 4.1e+00     0.000, 0.000"""
    c = _case(name, T)
    H, parts = c['H'], c['parts']
    assert c['dqkv'].dtype == flavour and c['dqkv'].shape == c['qkv'].shape
    assert bool(torch.isfinite(c['dqkv']).all())
    got, tor, emu = (ar.thirds(t, H) for t in (c['dqkv'], c['torch'][1], c['emu'][2]))
    bounds = ar.elementwise_bound(parts, flavour)
    failed = []
    for head, i, kind in ar.checks(name):
        n = ar.THIRDS[i]
        share = ar.largest_share(got[i], parts[n], bounds[i], head)
        share_e = ar.largest_share(emu[i], parts[n], bounds[i], head)
        line = 'attention bwd %s %s-%d head %s %s:' % (half.name(), name, T, head, n)
        if kind == 'rel':
            want = ar.pick(parts[n], head)
            e_k, e_t, e_e = (ar.rel_l2(ar.pick(t[i], head), want) for t in (got, tor, emu))
            line += ' e(kernel) %.3e  e(torch) %.3e  e(emulation) %.3e;' % (e_k, e_t, e_e)
            if not e_k <= 2 * e_t:
                failed.append((n, head, 'relative', e_k, e_t))
        else:
            line += ' max |kernel| %.3e, max |fp64| %.3e;' % (
                float(ar.pick(got[i], head).abs().max()), float(ar.pick(parts[n], head).abs().max()))
        print(line + ' share of the bound: kernel %.3f, emulation %.3f' % (share, share_e))
        if not share <= 1.0:
            failed.append((n, head, 'bound', share))
    assert not failed, failed


test_backward_on_hostile_data_fp16 = fp16_twin(test_backward_on_hostile_data)


# --------------------------------------------------------------------- exact properties
MIXED = ('mixed', 129)


def _run(qkv, dout, H):
    out, lse = vit_ops.attention_fwd_lse(qkv, H, SCALE)
    return out, lse, vit_ops.attention_bwd(qkv, out, dout, lse, H, SCALE)


def _slices(c, out, lse, dqkv):
    """{(b, h): (out, lse[:T], dq, dk, dv)} of a joint call's results."""
    H, T = c['H'], c['qkv'].shape[1]
    o, g = ar.heads(out, H), ar.thirds(dqkv, H)
    return {(b, h): (o[b, h], lse[b, h, :T], g[0][b, h], g[1][b, h], g[2][b, h])
            for b in range(ar.B) for h in range(H)}


def test_slices_are_independent(flavour):
    """Each (b, h) slice of 'mixed' called alone as (1, T, 1): out, lse[..., :T] and the
    three thirds of dqkv are bit-equal to the joint call's.  The arithmetic of a workgroup
    depends on T alone, so any difference is an indexing error."""
    c = _case(*MIXED)
    H, T = c['H'], MIXED[1]
    joint = _slices(c, c['out'], c['lse'], c['dqkv'])
    x = c['qkv'].view(ar.B, T, 3, H, 64)
    for (b, h), want in joint.items():
        qkv1 = x[b:b + 1, :, :, h].contiguous().view(1, T, 192)
        dout1 = c['dout'].view(ar.B, T, H, 64)[b:b + 1, :, h].contiguous()
        out1, lse1, dqkv1 = _run(qkv1, dout1, 1)
        g1 = dqkv1.view(T, 3, 64)
        alone = (out1[0], lse1[0, 0, :T], g1[:, 0], g1[:, 1], g1[:, 2])
        for n, a, w in zip(('out', 'lse', 'dq', 'dk', 'dv'), alone, want):
            assert torch.equal(a, w), (b, h, n)


test_slices_are_independent_fp16 = fp16_twin(test_slices_are_independent)


def test_a_nan_does_not_travel(flavour):
    """v of (b = 0, h = 0) all NaN, and in a second run dout of that slice: every other
    (b, h) slice of out, lse and dqkv is bit-equal to the clean run.  NaN is data here."""
    c = _case(*MIXED)
    H, T = c['H'], MIXED[1]
    clean = _slices(c, c['out'], c['lse'], c['dqkv'])
    qkv = c['qkv'].clone()
    qkv.view(ar.B, T, 3, H, 64)[0, :, 2, 0] = float('nan')
    dout = c['dout'].clone()
    dout.view(ar.B, T, H, 64)[0, :, 0] = float('nan')
    for what, args in (('v', (qkv, c['dout'])), ('dout', (c['qkv'], dout))):
        got = _slices(c, *_run(*args, H))
        assert bool(torch.isnan(got[0, 0][2]).all()), what     # dq: it did arrive where it belongs
        for key in clean:
            if key == (0, 0):
                continue
            for n, a, w in zip(('out', 'lse', 'dq', 'dk', 'dv'), got[key], clean[key]):
                assert torch.equal(a, w), (what, key, n)


test_a_nan_does_not_travel_fp16 = fp16_twin(test_a_nan_does_not_travel)


def test_backward_is_linear_in_dout_to_the_bit(flavour):
    """attention_bwd(..., dout 2^k) is bit-equal to 2^k attention_bwd(..., dout) for
    k = +12 and -12: every rounding of the backward (delta, ds, the three results) is
    relative, and bf16 has fp32's exponent range, so nothing leaves it."""
    if flavour == torch.float16:
        pytest.skip('fp16: ds of the saturated head is subnormal (about 1e-6), its rounding '
                    'is absolute, and dout 2^12 overflows: the property is bf16\'s')
    c = _case(*MIXED)
    for k in (12, -12):
        f = 2.0 ** k
        dout = c['dout'] * f
        assert torch.equal(dout.float(), c['dout'].float() * f)
        got = vit_ops.attention_bwd(c['qkv'], c['out'], dout, c['lse'], c['H'], SCALE)
        want = c['dqkv'] * f
        assert torch.equal(want.float(), c['dqkv'].float() * f)
        assert torch.equal(got, want), k


test_backward_is_linear_in_dout_to_the_bit_fp16 = fp16_twin(
    test_backward_is_linear_in_dout_to_the_bit)
