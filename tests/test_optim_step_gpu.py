"""GPU tests of csrc/optim_step.hip through veon_amd/optim.py, in both library flavours.

The yardstick is the torch mirror ON THE CPU (IEEE division and square root, no
contraction), never the code under test; the kernels must equal it bit for bit: the norm
in the kernels' summation order, and p / exp_avg / exp_avg_sq / EMA over three steps when
the mirror is fed the coefficient the finish kernel wrote.  Tensors are no larger than one
chunk + 1; the seams are the sizes around a chunk, an unaligned view (element accesses), a
padded arena slot before a full one, two groups, and more chunks than the finish workgroup
has threads."""
import copy
import math
import warnings

import pytest
import torch
from torch import nn

from tests import optim_refs as refs
from veon_amd import _lib, half, optim
from veon_amd.models.semantic_net import ResBlock3D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = optim.CHUNK
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SEAMS = [1, 3, C, 0, C - 1, C + 1]      # 3 is padded to 4 and followed by a full chunk
MANY = [C] * 258 + [5, C + 1]           # 261 chunks > 256 finish threads
NATIVE = ('veon_optim_sumsq', 'veon_optim_clip_finish', 'veon_optim_update')


@pytest.fixture(autouse=True, params=['bf16', 'fp16'])
def flavour(request):
    with half.use(request.param):
        yield request.param


class Bag(nn.Module):
    """Parameters of the given sizes in two halves (the optimizer's two groups), one
    parameter that is a view one element into its storage, a frozen parameter, a floating
    and an integer buffer."""

    def __init__(self, sizes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.first = nn.ParameterList([nn.Parameter(torch.randn(n, generator=g))
                                       for n in sizes[:len(sizes) // 2]])
        self.second = nn.ParameterList([nn.Parameter(torch.randn(n, generator=g))
                                        for n in sizes[len(sizes) // 2:]])
        self.view = nn.Parameter(torch.randn(C + 905, generator=g)[1:])
        self.frozen = nn.Parameter(torch.randn(C + 1, generator=g), requires_grad=False)
        self.register_buffer('stat', torch.randn(C - 1, generator=g))
        self.register_buffer('count', torch.tensor(7))

    def groups(self):
        return [dict(params=list(self.first) + [self.view]),
                dict(params=list(self.second), lr=3e-4, weight_decay=0.0)]

    def trained(self):
        return list(self.first) + [self.view] + list(self.second)


def _bag(sizes, seed, device):
    """The bag on ``device``; the view parameter stays a view one element in."""
    bag = Bag(sizes, seed)
    if device != 'cpu':
        whole = torch.cat([bag.view.detach().new_zeros(1), bag.view.detach()])
        bag.view = nn.Parameter(whole.to(device)[1:])
        bag.first = nn.ParameterList([nn.Parameter(p.detach().to(device)) for p in bag.first])
        bag.second = nn.ParameterList([nn.Parameter(p.detach().to(device)) for p in bag.second])
        bag.frozen = nn.Parameter(bag.frozen.detach().to(device), requires_grad=False)
        bag.stat = bag.stat.to(device)
        bag.count = bag.count.to(device)
    assert bag.view.data_ptr() % 16 == 4 and bag.view.is_contiguous()
    return bag


def _grads(bag, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [refs.wide_grads(tuple(p.shape), g) * scale for p in bag.trained()]


def _pair(sizes, max_norm=5.0, with_ema=True, seed=0):
    """The same bag, EMA and optimizer on the device and on the CPU."""
    out = []
    for device in (DEV, 'cpu'):
        bag = _bag(sizes, seed, device)
        ema = optim.ModelEMA(bag, decay=0.999, updates=900) if with_ema else None
        opt = optim.FusedAdamW(bag.groups(), max_norm=max_norm, ema=ema, **HYPER)
        out.append((bag, ema, opt))
    return out


def _load(bag, opt, grads):
    opt.zero_grad()
    for p, g in zip(bag.trained(), grads):
        p.grad.add_(g.to(p.device))


def _feed_coefficient(cpu_opt, scal):
    """The CPU mirror steps with the norm and coefficient the finish kernel wrote."""
    cpu_opt._scal.copy_(scal.cpu())
    cpu_opt.clip_grad_norm_ = lambda: cpu_opt._norm


def _differences(got, want):
    """'' when equal to the bit, else where and by how much they differ."""
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().reshape(-1)
    if bad.numel() == 0:
        return ''
    i = int(bad[0])
    return '%d of %d differ, first at %d: %r against %r, largest |difference| %.3e' % (
        bad.numel(), got.numel(), i, float(got[i]), float(want[i]),
        float((got.double() - want.double()).abs().nan_to_num(float('inf')).max()))


def _assert_same_state(dev, cpu, what):
    """Every arena element (padding included), parameter and EMA entry, bit for bit."""
    (bag, ema, opt), (cbag, cema, copt) = dev, cpu
    found = {}
    for name in ('_grad_arena', '_m_arena', '_v_arena'):
        found[name] = _differences(getattr(opt, name), getattr(copt, name))
    for (k, p), q in zip(bag.named_parameters(), cbag.parameters()):
        found[k] = _differences(p, q)
    if ema is not None:
        for (k, v), w in zip(ema.ema.state_dict().items(), cema.ema.state_dict().values()):
            found['ema ' + k] = _differences(v.float(), w.float())
    found = {k: v for k, v in found.items() if v}
    assert not found, (what, found)


def _padding_mask(opt):
    mask = torch.ones(opt._numel, dtype=torch.bool)
    for _, _, p, off in opt._slots:
        mask[off:off + p.numel()] = False
    return mask


def test_chunk_constant_is_the_kernels():
    assert _lib.lib().veon_optim_chunk() == optim.CHUNK


@pytest.mark.parametrize('sizes', [SEAMS, MANY], ids=['seams', 'many_chunks'])
def test_norm_equals_the_mirror_in_the_kernels_order(sizes):
    (bag, _, opt), (cbag, _, copt) = _pair(sizes, with_ema=False)
    assert (opt._partials.numel() > optim.FINISH_THREADS) == (sizes is MANY)
    grads = _grads(bag, 1)
    _load(bag, opt, grads)
    n0 = dict(_lib.CALLS)
    got = opt.clip_grad_norm_()
    assert all(_lib.CALLS.get(k, 0) == n0.get(k, 0) + 1 for k in NATIVE[:2])
    assert got is opt.grad_norm
    arena = opt._grad_arena.cpu()
    want_partials = optim.chunk_partials_torch(arena)
    assert torch.equal(opt._partials.cpu(), want_partials)
    want, coef = optim.grad_norm_torch(arena, 5.0)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(opt._scal.cpu(), torch.stack([want, coef]))
    exact = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    assert abs(float(got) - exact) <= (optim.NORM_CHAIN + 1) * 2.0 ** -24 * exact


@pytest.mark.parametrize('sizes', [SEAMS, MANY], ids=['seams', 'many_chunks'])
def test_three_steps_equal_the_mirror_bit_for_bit(sizes):
    dev, cpu = _pair(sizes)
    (bag, ema, opt), (cbag, cema, copt) = dev, cpu
    assert len(opt._slots) == len(sizes) + 1
    mask = _padding_mask(opt)
    assert mask.any()
    _assert_same_state(dev, cpu, 'before')
    for step in range(3):
        # step 1 is clipped hard, step 2 is below max_norm, step 0 in between
        grads = _grads(bag, 10 + step, scale=(1.0, 10.0, 1e-4)[step])
        _load(bag, opt, grads)
        _load(cbag, copt, grads)
        with torch.no_grad():                     # the buffers move too, as under BN
            bag.stat.add_(0.25)
            cbag.stat.add_(0.25)
        n0 = dict(_lib.CALLS)
        opt.step()
        ema.update()
        assert all(_lib.CALLS.get(k, 0) == n0.get(k, 0) + 1 for k in NATIVE)
        coef = float(opt._coef)
        assert (coef == 1.0) == (step == 2), (step, coef)
        _feed_coefficient(copt, opt._scal)
        copt.step()
        cema.update()
        _assert_same_state(dev, cpu, 'step %d' % step)
        for name in ('_grad_arena', '_m_arena', '_v_arena'):
            assert not getattr(opt, name).cpu()[mask].any(), (step, name)
    assert ema.updates == 903 and int(ema.ema.count) == 7
    assert opt._steps == [3, 3]


def test_without_clipping_is_one_launch_and_equals_the_mirror():
    dev, cpu = _pair(SEAMS, max_norm=None)
    (bag, ema, opt), (cbag, cema, copt) = dev, cpu
    for step in range(2):
        grads = _grads(bag, 20 + step)
        _load(bag, opt, grads)
        _load(cbag, copt, grads)
        n0 = dict(_lib.CALLS)
        opt.step()
        copt.step()
        assert [_lib.CALLS.get(k, 0) - n0.get(k, 0) for k in NATIVE] == [0, 0, 1]
    assert opt.grad_norm is None
    _assert_same_state(dev, cpu, 'no clipping')


def test_model_ema_alone_is_one_launch_and_equals_the_reference_lines():
    bag = _bag(SEAMS, 3, DEV)
    ema = optim.ModelEMA(bag, decay=0.999, updates=10560)
    want = {k: v.cpu().clone() for k, v in bag.state_dict().items()}
    with torch.no_grad():
        for t in bag.state_dict().values():
            if t.dtype.is_floating_point:
                t.add_(1.5)
    n0 = dict(_lib.CALLS)
    ema.update(None, bag)
    assert [_lib.CALLS.get(k, 0) - n0.get(k, 0) for k in NATIVE] == [0, 0, 1]
    d = refs.reference_decay(0.999, 10561)
    for k, v in want.items():
        if v.dtype.is_floating_point:
            refs.reference_ema_lines(v, d, bag.state_dict()[k].cpu())
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v.cpu(), want[k]), k


@pytest.mark.parametrize('case', ['above', 'below', 'nan'])
def test_finish_coefficient(case):
    (bag, _, opt), _ = _pair(SEAMS, max_norm={'above': 1e9, 'below': 0.5, 'nan': 5.0}[case],
                             with_ema=False)
    before = [p.detach().clone() for p in bag.trained()]
    grads = _grads(bag, 30)
    if case == 'nan':
        grads[2][17] = float('nan')
    _load(bag, opt, grads)
    opt.step()
    norm, coef = opt._scal.cpu()
    want_norm, want_coef = optim.grad_norm_torch(opt._grad_arena.cpu(), opt.max_norm)
    if case == 'nan':
        assert math.isnan(float(norm)) and math.isnan(float(coef))
        assert all(torch.isnan(p).all() for p in bag.trained() if p.numel())
        return
    assert torch.equal(norm, want_norm) and torch.equal(coef, want_coef)
    if case == 'above':
        assert float(coef) == 1.0
    else:
        assert float(coef) == float(torch.tensor(0.5) / (norm + torch.tensor(1e-6))) < 1.0
    assert all(torch.isfinite(p).all() and not torch.equal(p.detach(), b)
               for p, b in zip(bag.trained(), before) if p.numel())


def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    # torch's warning of a synchronising operation; the one-time notice that the mode is a
    # prototype (raised by set_sync_debug_mode itself, first use in a process) is not one
    found = [w for w in rec if 'called a synchroniz' in str(w.message).lower()]
    for w in found:
        print('synchronising call at %s:%d: %s' % (w.filename, w.lineno, w.message))
    return len(found)


def test_steady_state_makes_three_native_calls_and_no_synchronising_one():
    """One iteration (zero_grad, gradient adds, step, update) under
    torch.cuda.set_sync_debug_mode('warn'): no synchronising call, three native calls, no
    allocation.  Reading ``grad_norm`` is the one synchronising call, which also shows that
    the mode is live."""
    (bag, ema, opt), _ = _pair(MANY)
    grads = [g.to(DEV) for g in _grads(bag, 40)]

    def iteration():
        opt.zero_grad()
        for p, g in zip(bag.trained(), grads):
            p.grad.add_(g)
        opt.step()
        ema.update()

    iteration()
    allocated = torch.cuda.memory_allocated()
    n0 = dict(_lib.CALLS)
    n_sync = _sync_warnings(iteration)
    live = _sync_warnings(lambda: float(opt.grad_norm))
    print('synchronisation warnings: step %d, reading grad_norm %d' % (n_sync, live))
    assert n_sync == 0 and live == 1
    assert [_lib.CALLS.get(k, 0) - n0.get(k, 0) for k in NATIVE] == [1, 1, 1]
    assert torch.cuda.memory_allocated() == allocated


def test_two_identical_runs_are_bit_equal():
    runs = []
    for _ in range(2):
        (bag, ema, opt), _ = _pair(MANY)
        for step in range(2):
            _load(bag, opt, _grads(bag, 50 + step))
            opt.step()
            ema.update()
        runs.append([opt._scal.clone(), opt._m_arena, opt._v_arena]
                    + [p.detach() for p in bag.parameters()]
                    + [v for v in ema.ema.state_dict().values()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_step_after_a_native_backward_against_torch_and_fp64():
    """One ResBlock3D(64, 64) trained natively: FusedAdamW(max_norm, ema) after its
    backward, against clip_grad_norm_ + torch.optim.AdamW(foreach=False) + the reference's
    EMA lines on a deep copy that is handed the same gradients, both measured against the
    fp64 restatement: e(kernel) <= 2 e(torch) for p, exp_avg, exp_avg_sq and the EMA
    (e = max |x - fp64| / max |fp64| over all parameters)."""
    torch.manual_seed(5)
    block = ResBlock3D(64, 64).to(DEV).train()
    twin = copy.deepcopy(block)
    ema = optim.ModelEMA(block, decay=0.999, updates=4000)
    twin_ema = {k: v.clone() for k, v in twin.state_dict().items()}
    opt = optim.FusedAdamW(block.parameters(), max_norm=1e-3, ema=ema, **HYPER)
    topt = torch.optim.AdamW(twin.parameters(), foreach=False, **HYPER)
    x = torch.randn(2, 64, 4, 10, 12, device=DEV)
    ResBlock3D.hip_train = True
    try:
        n0 = _lib.CALLS.get('veon_conv3d_k3_wgrad_bf16', 0)
        opt.zero_grad()
        block(x).square().mean().backward()
        assert _lib.CALLS.get('veon_conv3d_k3_wgrad_bf16', 0) > n0
    finally:
        ResBlock3D.hip_train = False
    params, twins = list(block.parameters()), list(twin.parameters())
    assert all(p.grad is v for p, v in zip(params, opt._views))
    grads = [p.grad.clone() for p in params]
    assert all(g.abs().sum() > 0 for g in grads)
    ref = refs.Fp64Step([p.cpu() for p in params], [p.cpu() for p in params])
    for q, g in zip(twins, grads):
        q.grad = g.clone()
    # the buffers after the forward are the model's state the EMA reads
    twin.load_state_dict({k: v for k, v in block.state_dict().items() if 'running' in k
                          or 'num_batches' in k}, strict=False)
    tnorm = torch.nn.utils.clip_grad_norm_(twins, 1e-3)
    opt.step()
    ema.update()
    topt.step()
    d = refs.reference_decay(0.999, 4001)
    for k, v in twin_ema.items():
        if v.dtype.is_floating_point:
            refs.reference_ema_lines(v, d, twin.state_dict()[k])
    ref.step([g.cpu() for g in grads], max_norm=1e-3, d=d, **HYPER)
    assert float(opt.grad_norm) > 1e-3
    assert abs(float(opt.grad_norm) - ref.norm) <= (optim.NORM_CHAIN + 1) * 2.0 ** -24 * ref.norm
    print('norm: kernel %.9g torch %.9g fp64 %.9g' % (float(opt.grad_norm), float(tnorm), ref.norm))
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])  # noqa: E731
    names = [k for k, _ in block.named_parameters()]
    got_ema, want_ema = ema.ema.state_dict(), twin_ema
    sd = opt.state_dict()['state']
    for what, mine, theirs, want in (
            ('p', params, twins, ref.p),
            ('m', [sd[i]['exp_avg'] for i in range(len(params))],
             [topt.state[q]['exp_avg'] for q in twins], ref.m),
            ('v', [sd[i]['exp_avg_sq'] for i in range(len(params))],
             [topt.state[q]['exp_avg_sq'] for q in twins], ref.v),
            ('ema', [got_ema[k] for k in names], [want_ema[k] for k in names], ref.e)):
        e_kernel = refs.scaled_error(cat(mine), cat(want))
        e_torch = refs.scaled_error(cat(theirs), cat(want))
        print('%s: e_kernel %.3e e_torch %.3e' % (what, e_kernel, e_torch))
        assert e_kernel <= 2 * e_torch, (what, e_kernel, e_torch)
    # the EMA-only entries (BatchNorm statistics) follow the reference lines to the bit
    for k in got_ema:
        if k not in names:
            assert torch.equal(got_ema[k], want_ema[k]), k


def test_entries_the_kernel_cannot_take_follow_the_reference_lines():
    """A half buffer and a non-contiguous fp32 buffer on the device: ModelEMA alone and
    under FusedAdamW sends them through the reference's two lines, the rest through the
    kernel; both equal the lines run on the same tensors."""
    for fused in (False, True):
        torch.manual_seed(11)
        model = nn.Linear(8, 8).to(DEV)
        model.register_buffer('halves', torch.randn(37, device=DEV).half())
        model.register_buffer('strided', torch.randn(6, 5, device=DEV).t())
        ema = optim.ModelEMA(model, decay=0.999, updates=500)
        opt = optim.FusedAdamW(model.parameters(), ema=ema, **HYPER) if fused else None
        want = {k: v.clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            for t in model.state_dict().values():
                t.add_(0.5)
        n0 = _lib.CALLS.get(NATIVE[2], 0)
        if fused:
            opt.step()          # zero gradients: p moves by the weight decay alone
        ema.update(None, model)
        assert _lib.CALLS.get(NATIVE[2], 0) == n0 + 1
        d = refs.reference_decay(0.999, 501)
        for k, v in want.items():
            refs.reference_ema_lines(v, d, model.state_dict()[k])
        for k, v in ema.ema.state_dict().items():
            assert torch.equal(v, want[k]), (fused, k)
