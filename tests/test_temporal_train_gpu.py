"""The backward of the deformable attention (csrc/temporal_train.hip) and the native
training step of the temporal fusion built on it.

Reference: fp64 CPU autograd of ``TemporalDeformable.attend`` (the definition) on the same
half-rounded operands.  Yardstick: the same ``attend`` under torch autograd in fp32 on the
device (tanh in fp32), its gradients rounded to the half dtype.  Condition, per gradient:
relative L2 error e(native) <= 2 e(yardstick) -- the project's factor for "rounds the same
quantities at the same places".  Every numeric test prints both errors (run with -s) and
has an fp16 twin.

doff leaves out the entries (voxel, head, sample) tests/temporal_train_refs.doff_keep_mask
names: a coordinate within 2^-10 voxel of a node, where fp32 and fp64 may floor
differently; at most 2 % (asserted here, and on the CPU for every input of this file).
With zero offsets on a cube every coordinate IS a node and exactly representable in fp32
(-1 + 2i/4, then (g + 1) * 0.5 * 4 = i without rounding), so both precisions floor alike
and nothing is left out there.
"""
import contextlib
import copy
import functools

import pytest
import torch

from tests import temporal_train_refs as tr
from tests.helpers import flavour, fp16_twin, named_init_, roundoff, to_half  # noqa: F401
from veon_amd import _lib, conv3d_ops, half
from veon_amd.models.semantic_net import temporal_fusion as tfm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = {tr.case_id(c): c for c in tr.GPU_CASES}
DKV = 'veon_deform_attention_bwd_dkv_bf16'


def _pack(t):
    return conv3d_ops.pack(t.to(DEV))


def _native(kv, q, off, dout, heads, **kw):
    dkv, dq, doff = conv3d_ops.deform_attention_bwd(_pack(kv), _pack(q), _pack(off),
                                                    _pack(dout), heads, **kw)
    return dkv, dq, doff


@functools.lru_cache(maxsize=None)
def _case(cid, flavour_name):
    """Inputs, fp64 reference, half-rounded fp32 yardstick and native result of one case,
    computed once per flavour and left unchanged."""
    name, B, hd, heads, zyx, seed, kw = CASES[cid]
    kv, q, off, dout = tr.inputs(B, hd, heads, zyx, seed, **kw)
    ref = tr.attend_autograd(kv, q, off, dout, heads)[1:]
    yard = tr.attend_autograd(kv, q, off, dout, heads, dtype=torch.float32, device=DEV)[1:]
    yard = tuple(g.to(half.dtype()).double().cpu() for g in yard)
    vols = _native(kv, q, off, dout, heads)
    nat = tuple(conv3d_ops.unpack(v).double().cpu() for v in vols)
    return (kv, q, off, dout), ref, yard, nat, vols


def _halo_is_zero(vol):
    B, C, Z, Y, X = vol.shape
    halo = vol.rows.view(B, Z + 2, Y + 2, X + 2, C).clone()
    halo[:, 1:-1, 1:-1, 1:-1] = 0
    assert float(halo.float().abs().sum()) == 0.0


def _hold(tag, nat, yard, ref, mask=None):
    en, ey = tr.rel_l2(nat, ref, mask), tr.rel_l2(yard, ref, mask)
    print('%s: native %.3e yardstick %.3e ratio %.2f' % (tag, en, ey, en / max(ey, 1e-300)))
    assert bool(torch.isfinite(nat).all()), tag
    assert en <= 2 * ey, (tag, en, ey)


def _check(cid, which=('dkv', 'dq', 'doff'), exclude=True):
    name, B, hd, heads, zyx, seed, kw = CASES[cid]
    (kv, q, off, dout), ref, yard, nat, vols = _case(cid, half.name())
    noff = heads * 24
    for i, g in enumerate(('dkv', 'dq', 'doff')):
        _halo_is_zero(vols[i])
        if g not in which:
            continue
        mask = None
        n, y, r = nat[i], yard[i], ref[i]
        if g == 'doff':
            n, y, r = n[:, :noff], y[:, :noff], r[:, :noff]
            if exclude:
                mask = tr.doff_keep_mask(off, heads, zyx)
                share = 1.0 - mask.double().mean().item()
                print('%s: %.2f %% of doff left out' % (cid, 100 * share))
                assert share <= 0.02
        _hold('%s %s' % (cid, g), n, y, r, mask)


def _ids(*names):
    return [cid for cid, c in CASES.items() if c[0] in names]


@pytest.mark.parametrize('cid', _ids('layout', 'box', 'len1', 'qscale', 'randn'))
def test_backward_holds_the_fp32_yardstick(cid):
    _check(cid)


test_backward_holds_the_fp32_yardstick_fp16 = fp16_twin(test_backward_holds_the_fp32_yardstick)


@pytest.mark.parametrize('cid', _ids('surplus'))
def test_surplus_offset_channels(cid):
    """8 NaN surplus offset channels: the same bits as the tight call, and the surplus
    columns of doff exactly zero."""
    _check(cid)
    name, B, hd, heads, zyx, seed, kw = CASES[cid]
    (kv, q, off, dout), _, _, nat, vols = _case(cid, half.name())
    noff = heads * 24
    assert off.shape[1] == noff + 8 and bool(torch.isnan(off[:, noff:]).all())
    tight = _native(kv, q, off[:, :noff].contiguous(), dout, heads)
    assert torch.equal(tight[0].rows, vols[0].rows) and torch.equal(tight[1].rows, vols[1].rows)
    wide = vols[2].rows.view(-1, noff + 8)
    assert torch.equal(wide[:, :noff], tight[2].rows)
    assert float(wide[:, noff:].float().abs().sum()) == 0.0


test_surplus_offset_channels_fp16 = fp16_twin(test_surplus_offset_channels)


@pytest.mark.parametrize('cid', _ids('zero'))
def test_zero_offsets_on_a_cube(cid):
    """Every sample on a node: doff and dkv under the condition (nothing left out, see the
    module docstring).  dq is zero in exact arithmetic; the eight da_s are bitwise equal
    and the softmax weights within 2^-22 of 1/8, so per voxel and head
    |dq| <= 2^-16 hd^-0.5 max_s |dOut.V_s| max_s |K_s|_inf."""
    _check(cid, which=('dkv', 'doff'), exclude=False)
    name, B, hd, heads, zyx, seed, kw = CASES[cid]
    (kv, q, off, dout), _, _, nat, _ = _case(cid, half.name())
    Z, Y, X = zyx
    assert Z == X
    # the sample of voxel (z, y, x) sits on the row (z' = x, y, x' = z)
    rows = kv.double().transpose(2, 4).reshape(B, heads, 2, hd, Z, Y, X)
    K, V = rows[:, :, 0], rows[:, :, 1]
    da = (dout.double().view(B, heads, hd, Z, Y, X) * V).sum(2)
    bound = 2.0 ** -16 * hd ** -0.5 * da.abs() * K.abs().amax(2)
    dq = nat[1].view(B, heads, hd, Z, Y, X).abs()
    ratio = (dq / bound.unsqueeze(2).clamp_min(1e-300)).max().item()
    print('%s dq: largest |dq| / bound %.3g' % (cid, ratio))
    assert ratio <= 1.0


test_zero_offsets_on_a_cube_fp16 = fp16_twin(test_zero_offsets_on_a_cube)


@pytest.mark.parametrize('cid', _ids('saturated'))
def test_saturated_offsets(cid):
    """Offsets +-8: tanh' ~ 4.5e-7.  dq and dkv under the condition; doff finite and at
    most 1e-3 of the randn case's largest entry at the same shape and seed (the fp64
    ratio is about 1e-6)."""
    _check(cid, which=('dkv', 'dq'))
    _, _, _, nat, _ = _case(cid, half.name())
    _, _, _, nat_r, _ = _case(cid.replace('saturated', 'randn'), half.name())
    assert bool(torch.isfinite(nat[2]).all())
    big, small = nat_r[2].abs().max().item(), nat[2].abs().max().item()
    print('%s: max |doff| %.3e against %.3e (randn)' % (cid, small, big))
    assert small <= 1e-3 * big


test_saturated_offsets_fp16 = fp16_twin(test_saturated_offsets)


# ----------------------------------------------------------------------- structure
def _storages(cid, grads=(True, True, True)):
    name, B, hd, heads, zyx, seed, kw = CASES[cid]
    kv, q, off, dout = tr.inputs(B, hd, heads, zyx, seed, **kw)
    vols = [_pack(t) for t in (kv, q, off)]
    st = [v.storage.clone().requires_grad_(g) for v, g in zip(vols, grads)]
    return vols, st, _pack(dout), heads, vols[1].shape


@pytest.mark.parametrize('cid', ['layout-B1-hd32-h4-3x5x7', 'layout-B2-hd64-h2-2x4x4'])
def test_training_op_forward_and_autograd(cid):
    """The forward of the training op is the inference kernel bit for bit; autograd
    returns what ``deform_attention_bwd`` returns; a second backward gives equal bits."""
    vols, st, dout, heads, shape = _storages(cid)
    want = conv3d_ops.deform_attention(*vols, heads)
    got = conv3d_ops.deform_attention_train(*st, heads, shape)
    assert torch.equal(got.detach(), want.storage)
    grads = torch.autograd.grad(got, st, dout.storage)
    direct = conv3d_ops.deform_attention_bwd(*vols, dout, heads)
    again = conv3d_ops.deform_attention_bwd(*vols, dout, heads)
    for g, d, a in zip(grads, direct, again):
        assert torch.equal(g, d.storage) and torch.equal(d.storage, a.storage)


test_training_op_forward_and_autograd_fp16 = fp16_twin(test_training_op_forward_and_autograd)


@pytest.mark.parametrize('cid', ['layout-B1-hd32-h2-3x5x7', 'len1-B2-hd64-h1-3x1x7'])
def test_backward_overwrites_every_element(cid):
    """NaN-filled dkv / dq / doff buffers: no NaN is left and the halos are zero."""
    vols, _, dout, heads, _ = _storages(cid)
    outs = [v.like() for v in vols]
    for o in outs:
        o.rows.fill_(float('nan'))
    conv3d_ops.deform_attention_bwd(*vols, dout, heads, out=tuple(outs))
    for o in outs:
        assert not bool(torch.isnan(o.rows.float()).any())
        _halo_is_zero(o)


test_backward_overwrites_every_element_fp16 = fp16_twin(test_backward_overwrites_every_element)


def test_no_dkv_kernel_when_kv_needs_no_gradient():
    vols, st, dout, heads, shape = _storages('layout-B1-hd32-h4-3x5x7', (False, True, True))
    out = conv3d_ops.deform_attention_train(*st, heads, shape)
    before = _lib.CALLS.get(DKV, 0)
    dq, doff = torch.autograd.grad(out, st[1:], dout.storage)
    assert _lib.CALLS.get(DKV, 0) == before
    vols2, st2, _, _, _ = _storages('layout-B1-hd32-h4-3x5x7')
    out2 = conv3d_ops.deform_attention_train(*st2, heads, shape)
    full = torch.autograd.grad(out2, st2, dout.storage)
    assert _lib.CALLS.get(DKV, 0) == before + 1
    assert torch.equal(full[1], dq) and torch.equal(full[2], doff)


test_no_dkv_kernel_when_kv_needs_no_gradient_fp16 = fp16_twin(
    test_no_dkv_kernel_when_kv_needs_no_gradient)


# ------------------------------------------------------------------------- modules
# Reference: the module's own definition in fp64 on the CPU.  Yardstick: the unmodified
# module (switches off) under torch.autocast in the flavour's dtype on the device.
# Condition per tensor (output, input gradients, parameter gradients, BN buffers):
# e(native) <= 2 e(autocast), relative L2.  Two gradients are zero in exact arithmetic
# (out_proj.bias, key_value_proj.bias) and are held to bounds of their own, see below.
ZYX = (3, 5, 7)


@contextlib.contextmanager
def _switches(on):
    old = tfm.TemporalDeformable.hip_train, tfm.TemporalFusionMultiFrame.hip_train
    tfm.TemporalDeformable.hip_train = tfm.TemporalFusionMultiFrame.hip_train = on
    try:
        yield
    finally:
        tfm.TemporalDeformable.hip_train, tfm.TemporalFusionMultiFrame.hip_train = old


def _module(kind, C, seed, T=1):
    torch.manual_seed(seed)
    mod = tfm.TemporalDeformable(C) if kind == 'deform' else tfm.TemporalFusionMultiFrame(C, seqs=T)
    named_init_(mod, kind, seed)
    with torch.no_grad():        # offsets of the order of a voxel, as a trained module has
        for m in mod.modules():
            if isinstance(m, tfm.TemporalDeformable):
                m.offset_conv[2].weight.mul_(4.0)
    return mod.train()


def _step(mod, run, tensors, needs, dout, dtype, device, autocast=None):
    """One training step of a fresh copy of ``mod`` -> {name: float64 CPU tensor}."""
    mod = copy.deepcopy(mod).to(device=device, dtype=dtype).train()
    ins = [t.detach().to(device=device, dtype=dtype).requires_grad_(n)
           for t, n in zip(tensors, needs)]
    ctx = torch.autocast('cuda', dtype=autocast) if autocast else contextlib.nullcontext()
    with ctx:
        out = run(mod, ins)
    out.backward(dout.to(device=device, dtype=out.dtype))
    res = {'out': out.detach()}
    for i, (t, n) in enumerate(zip(ins, needs)):
        if n:
            res['d input %d' % i] = t.grad
        else:
            assert t.grad is None                  # a past frame gets no gradient
    for k, p in mod.named_parameters():
        res['d ' + k] = p.grad
    for k, b in mod.named_buffers():
        res['buffer ' + k] = b
    return {k: v.detach().double().cpu() for k, v in res.items()}, mod


def _hold_module(tag, mod, run, tensors, needs, seed):
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(tensors[0].shape, generator=g)
    hooked = {}
    ref_mod = copy.deepcopy(mod)

    def keep(name):
        def hook(m, i, o):
            o.register_hook(lambda gr: hooked.setdefault(name, []).append(gr.detach().clone()))
        return hook
    for m in ref_mod.modules():
        if isinstance(m, tfm.TemporalDeformable):
            m.out_proj.register_forward_hook(keep('dy'))
            m.key_value_proj.register_forward_hook(keep('dkv'))
    ref, _ = _step(ref_mod, run, tensors, needs, dout, torch.float64, 'cpu')
    with _switches(False):
        yard, _ = _step(mod, run, tensors, needs, dout, torch.float32, DEV, autocast=half.dtype())
    before = dict(_lib.CALLS)
    with _switches(True):
        nat, _ = _step(mod, run, tensors, needs, dout, torch.float32, DEV)
    ran = {k for k, v in _lib.CALLS.items() if v > before.get(k, 0)}
    assert {'veon_deform_attention_bwd_bf16', DKV, 'veon_conv3d_k3_wgrad_bf16',
            'veon_linear_wgrad_bf16', 'veon_bn3d_bwd_apply_bf16'} <= ran, ran
    assert set(nat) == set(ref) == set(yard)
    worst = 0.0
    for k in sorted(ref):
        if k.endswith('num_batches_tracked'):
            assert torch.equal(nat[k], ref[k])
            continue
        if k.endswith('out_proj.bias') and k.startswith('d '):
            # exact gradient zero: the sum over the n voxels of dy.  A path that sums
            # half-rounded dy may be off by the roundings: <= roundoff * sum |dy|
            bound = roundoff() * sum(d.abs().sum(dim=(0, 2, 3, 4)) for d in hooked['dy'])
            assert float(ref[k].abs().max()) <= 1e-9
            ratio = (nat[k].abs() / bound).max().item()
            print('%s %s: |g| / bound %.3g' % (tag, k, ratio))
            assert ratio <= 1.0
            continue
        if k.endswith('key_value_proj.bias') and k.startswith('d '):
            # also zero in exact arithmetic: a constant added to every key moves all 8
            # logits alike, one added to every value passes through the softmax weights
            # (they sum to one) and out_proj as a per-channel constant, which train-mode
            # BN removes.  A relative error against zero is undefined: both paths are
            # measured against the size of what they sum, sum_v |dkv[v, c]| (fp64)
            size = sum(d.abs().sum(dim=(0, 2, 3, 4)) for d in hooked['dkv'])
            assert float(ref[k].abs().max()) <= 1e-9 * float(size.max())
            en, ey = (nat[k].norm() / size.norm()).item(), (yard[k].norm() / size.norm()).item()
        else:
            en, ey = tr.rel_l2(nat[k], ref[k]), tr.rel_l2(yard[k], ref[k])
        worst = max(worst, en / max(ey, 1e-300))
        print('%s %-55s native %.3e autocast %.3e ratio %.2f' % (tag, k, en, ey, en / max(ey, 1e-300)))
        assert bool(torch.isfinite(nat[k]).all()), k
        assert en <= 2 * ey, (tag, k, en, ey)
    print('%s: largest ratio %.2f' % (tag, worst))


def test_temporal_deformable_training_step():
    C, B = 128, 2
    mod = _module('deform', C, 3)
    g = torch.Generator().manual_seed(4)
    prev, curr = (to_half(torch.randn(B, C, *ZYX, generator=g)) for _ in range(2))
    _hold_module('deform', mod, lambda m, ins: m(ins[0], ins[1]), [prev, curr], [True, True], 5)


test_temporal_deformable_training_step_fp16 = fp16_twin(test_temporal_deformable_training_step)


@pytest.mark.parametrize('T', [1, 2])
def test_temporal_fusion_training_step(T):
    C, B = 128, 2
    mod = _module('fusion', C, 6 + T, T)
    g = torch.Generator().manual_seed(7 + T)
    frames = [to_half(torch.randn(B, C, *ZYX, generator=g)) for _ in range(T + 1)]
    _hold_module('fusion T=%d' % T, mod, lambda m, ins: m(ins[0], ins[1:]), frames,
                 [True] + [False] * T, 8 + T)


test_temporal_fusion_training_step_fp16 = fp16_twin(test_temporal_fusion_training_step)


def test_decoder_in_training_mode_with_the_switches():
    """AlignNetOcc3D(num_temporal=2) in training mode (forward only): switches on against
    switches off, held to twice the error of the switches-off run with the temporal
    fusion under autocast.  The shape of tests/test_temporal_gpu.py's decoder."""
    from tests.conftest import load_golden
    from tests.test_temporal_gpu import _decoder, _randomise
    t = {k: torch.from_numpy(v).to(DEV) for k, v in load_golden('align_net_tiny').items()}
    torch.manual_seed(5)
    net = _decoder(256, 1)
    _randomise(net.cpu(), torch.Generator().manual_seed(5))
    net = net.to(DEV).train()
    metas = [t['s2e'], t['e2g'], t['intr'], t['pr'], t['pt'], t['bda'][None]]
    clip = {1: t['clip1'], 2: t['clip2']}
    sem_feat = torch.zeros(2, 8, 4, 11, device=DEV)
    g = torch.Generator().manual_seed(6)
    prev = to_half(torch.randn(1, 256, 2, 10, 10, generator=g)).to(DEV)

    def run():
        with torch.no_grad():
            return net(sem_feat, clip, [t['supp']], t['metric'], metas, [prev])
    with _switches(False):
        want = run()
        plain = net.temporal_fusion.forward

        def under_autocast(*a):
            with torch.autocast('cuda', dtype=half.dtype()):
                return plain(*a).float()
        net.temporal_fusion.forward = under_autocast
        yard = run()
        del net.temporal_fusion.forward
    before = _lib.CALLS.get('veon_deform_attention_bf16', 0)
    with _switches(True):
        got = run()
    assert _lib.CALLS.get('veon_deform_attention_bf16', 0) == before + 2
    assert set(got) == set(want)
    for key in sorted(want):
        en, ey = tr.rel_l2(got[key], want[key]), tr.rel_l2(yard[key], want[key])
        print('decoder %s: native %.3e autocast %.3e ratio %.2f' % (key, en, ey, en / ey))
        assert en <= 2 * ey, (key, en, ey)


test_decoder_in_training_mode_with_the_switches_fp16 = fp16_twin(
    test_decoder_in_training_mode_with_the_switches)
