"""CPU tests of veon_amd/optim.py: the torch mirrors of csrc/optim_step.hip against the
reference's EMA lines (bit for bit) and an fp64 restatement of clip + AdamW (within twice
torch's own fp32 error), the norm's summation order against its derived bound, and the host
logic of FusedAdamW / ModelEMA / MEGVIIEMAHook.  The yardsticks are tests/optim_refs.py."""
import copy
import math
import types

import pytest
import torch
from torch import nn

from tests import optim_refs as refs
from veon_amd import _lib, optim

HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def test_symbols_are_declared():
    names = _lib.declared_symbols()
    for s in ('veon_optim_chunk', 'veon_optim_sumsq', 'veon_optim_clip_finish',
              'veon_optim_update'):
        assert s in names


# ------------------------------------------------------------------ EMA
def test_ema_mirror_equals_the_reference_lines_bit_for_bit():
    g = torch.Generator().manual_seed(0)
    n = 200000
    model, ema = torch.randn(n, generator=g), torch.randn(n, generator=g)
    want = ema.clone()
    d = refs.reference_decay(0.999, 10561)
    refs.reference_ema_lines(want, d, model)
    optim.adamw_ema_step_torch(model, None, None, None, ema, None, None, optim.ema_scalars(d))
    assert torch.equal(ema, want)


def test_model_ema_follows_the_reference_over_updates_with_a_changing_decay():
    """ModelEMA on a module with a buffer and a frozen parameter, five updates while the
    model moves: every floating entry equals the reference loop's, bit for bit; the integer
    buffer stays at its copy; track='changing' leaves the frozen parameter out."""
    torch.manual_seed(1)
    model = nn.Sequential(nn.Linear(7, 5), nn.BatchNorm1d(5), nn.Linear(5, 3))
    model[2].weight.requires_grad_(False)
    ema = optim.ModelEMA(model, decay=0.999, updates=3)
    changing = optim.ModelEMA(model, decay=0.999, updates=3, track='changing')
    assert '2.weight' in [k for k, _, _ in ema.pairs]
    assert '2.weight' not in [k for k, _, _ in changing.pairs]
    assert '1.running_mean' in [k for k, _, _ in changing.pairs]
    want = {k: v.clone() for k, v in copy.deepcopy(model).state_dict().items()}
    for it in range(5):
        with torch.no_grad():
            for t in model.state_dict().values():
                if t.dtype.is_floating_point:
                    t.add_(torch.randn_like(t))
        ema.update(None, model)
        d = refs.reference_decay(0.999, 3 + it + 1)
        for k, v in want.items():
            if v.dtype.is_floating_point:
                refs.reference_ema_lines(v, d, model.state_dict()[k])
    assert ema.updates == 8
    got = ema.ema.state_dict()
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert not any(p.requires_grad for p in ema.ema.parameters())
    assert not ema.ema.training


# ------------------------------------------------------------------ AdamW against fp64
SHAPES = [(3000,), (17, 129), (1,), (4097,)]


@pytest.mark.parametrize('max_norm', [None, 1e9, 5.0])
def test_adamw_mirror_within_twice_torch_error_against_fp64(max_norm):
    """Gradients Gaussian times 10^k, k in -4 .. 1; after 1, 3, 20 and 100 steps, for each
    of p, exp_avg and exp_avg_sq: e = max |x - fp64| / max |fp64| of the mirror (FusedAdamW
    on the CPU) is at most twice that of clip_grad_norm_ + torch.optim.AdamW(foreach=False)
    in fp32.  max_norm = 5 bites (the norm is in the thousands), 1e9 does not."""
    g = torch.Generator().manual_seed(2)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    ours = [nn.Parameter(t.clone()) for t in init]
    theirs = [nn.Parameter(t.clone()) for t in init]
    opt = optim.FusedAdamW(ours, max_norm=max_norm, **HYPER)
    topt = torch.optim.AdamW(theirs, foreach=False, **HYPER)
    ref = refs.Fp64Step(init)
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
    worst = 0.0
    for step in range(1, 101):
        grads = [refs.wide_grads(s, g) for s in SHAPES]
        opt.zero_grad()
        for p, q, gr in zip(ours, theirs, grads):
            p.grad.add_(gr)            # accumulates into the bound view, as autograd does
            q.grad = gr.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        opt.step()
        topt.step()
        ref.step(grads, max_norm=max_norm, **HYPER)
        if step not in (1, 3, 20, 100):
            continue
        if max_norm is not None:
            assert (ref.norm > max_norm) == (max_norm == 5.0)
        sd = opt.state_dict()['state']
        for name, mine, torchs, want in (
                ('p', ours, theirs, ref.p),
                ('m', [sd[i]['exp_avg'] for i in range(len(ours))],
                 [topt.state[q]['exp_avg'] for q in theirs], ref.m),
                ('v', [sd[i]['exp_avg_sq'] for i in range(len(ours))],
                 [topt.state[q]['exp_avg_sq'] for q in theirs], ref.v)):
            e_mirror = refs.scaled_error(cat(mine), cat(want))
            e_torch = refs.scaled_error(cat(torchs), cat(want))
            print('max_norm %s step %3d %s: e_mirror %.3e e_torch %.3e ratio %.2f'
                  % (max_norm, step, name, e_mirror, e_torch, e_mirror / e_torch))
            worst = max(worst, e_mirror / e_torch)
            assert e_mirror <= 2 * e_torch, (step, name, e_mirror, e_torch)
    print('largest ratio %.2f' % worst)


# ------------------------------------------------------------------ norm
@pytest.mark.parametrize('n', [1, optim.CHUNK - 1, optim.CHUNK + 1, 300 * optim.CHUNK + 5])
def test_norm_mirror_within_its_derived_bound(n):
    """Every squared element is rounded once and then passes through at most NORM_CHAIN
    fp32 additions (16 in its lane, 6 butterfly steps, 4 waves), all terms non-negative:
    the sum of squares is within (NORM_CHAIN + 1) * 2^-24 relative (first order) of the
    exact one; the fp64 finish adds 2^-53 per addition.  The square root halves that and
    the rounding to fp32 adds 2^-24, which stays below the same bound.  300 chunks: more
    partials than the finish workgroup has threads."""
    g = torch.Generator().manual_seed(n)
    x = refs.wide_grads((n,), g)
    got = float(optim.grad_norm_torch(x))
    want = math.sqrt(float((x.double() ** 2).sum()))
    bound = (optim.NORM_CHAIN + 1) * 2.0 ** -24
    rel = abs(got - want) / want
    print('n %d: norm %.9g fp64 %.9g rel %.3e bound %.3e' % (n, got, want, rel, bound))
    assert rel <= bound


def test_norm_mirror_layout_constants_match_the_chain():
    per_lane = optim.CHUNK // optim.FINISH_THREADS
    assert optim.CHUNK % (4 * optim.FINISH_THREADS) == 0
    assert optim.NORM_CHAIN == per_lane + int(math.log2(64)) + optim.FINISH_THREADS // 64


def test_finish_mirror_coefficient():
    part = torch.tensor([9.0, 16.0])
    norm, coef = optim.finish_torch(part, 10.0)
    assert float(norm) == 5.0 and float(coef) == 1.0
    norm, coef = optim.finish_torch(part, 2.5)
    assert float(coef) == float(torch.tensor(2.5) / (torch.tensor(5.0) + torch.tensor(1e-6)))
    norm, coef = optim.finish_torch(torch.tensor([9.0, float('nan')]), 2.5)
    assert math.isnan(float(norm)) and math.isnan(float(coef))


def test_one_nan_gradient_element_makes_every_stepped_parameter_nan():
    """As clip_grad_norm_(error_if_nonfinite=False) + AdamW: the NaN norm gives a NaN
    coefficient, which reaches every element of every parameter."""
    g = torch.Generator().manual_seed(3)
    ours = [nn.Parameter(torch.randn(5, generator=g)), nn.Parameter(torch.randn(3, 4, generator=g))]
    theirs = [nn.Parameter(p.detach().clone()) for p in ours]
    opt = optim.FusedAdamW(ours, max_norm=5.0, **HYPER)
    topt = torch.optim.AdamW(theirs, foreach=False, **HYPER)
    for p, q in zip(ours, theirs):
        gr = torch.randn(p.shape, generator=g)
        p.grad.copy_(gr)
        q.grad = gr.clone()
    ours[1].grad[2, 1] = float('nan')
    theirs[1].grad[2, 1] = float('nan')
    torch.nn.utils.clip_grad_norm_(theirs, 5.0)
    opt.step()
    topt.step()
    assert math.isnan(float(opt.grad_norm))
    for p, q in zip(ours, theirs):
        assert torch.isnan(q).all() and torch.isnan(p).all()


# ------------------------------------------------------------------ state dict
def _two_group_model(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 2))


def _groups(model):
    return [dict(params=list(model[0].parameters())),
            dict(params=list(model[1].parameters()), lr=3e-4, weight_decay=0.0)]


def _train(model, opt, steps, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        opt.zero_grad()
        model(torch.randn(4, 6, generator=g)).square().sum().backward()
        opt.step()


def test_state_dict_round_trip_with_torch_adamw_both_ways():
    """Two steps in one class, the state handed to the other, two more steps in both: the
    parameters agree to the few ulps the two fp32 sequences differ by, and the step
    counts carry over."""
    for first in ('fused', 'torch'):
        a, b = _two_group_model(4), _two_group_model(4)
        fused = optim.FusedAdamW(_groups(a), **HYPER)
        plain = torch.optim.AdamW(_groups(b), foreach=False, **HYPER)
        src, dst = (fused, plain) if first == 'fused' else (plain, fused)
        _train(a if first == 'fused' else b, src, 2, 5)
        (b if first == 'fused' else a).load_state_dict(
            (a if first == 'fused' else b).state_dict())
        dst.load_state_dict(copy.deepcopy(src.state_dict()))
        sd = fused.state_dict()
        assert sorted(sd['state']) == [0, 1, 2, 3]
        for st in sd['state'].values():
            assert sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] and float(st['step']) == 2.0
        assert sd['param_groups'][1]['lr'] == 3e-4 and sd['param_groups'][1]['weight_decay'] == 0.0
        _train(a, fused, 2, 6)
        _train(b, plain, 2, 6)
        assert fused._steps == [4, 4]
        assert all(float(plain.state[p]['step']) == 4.0 for p in b.parameters())
        for p, q in zip(a.parameters(), b.parameters()):
            torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-7)
        for i, q in enumerate(b.parameters()):
            torch.testing.assert_close(fused.state_dict()['state'][i]['exp_avg'],
                                       plain.state[q]['exp_avg'], rtol=1e-5, atol=1e-9)


def test_state_dict_is_empty_before_the_first_step():
    opt = optim.FusedAdamW(_two_group_model(7).parameters(), **HYPER)
    assert opt.state_dict()['state'] == {}


# ------------------------------------------------------------------ argument errors
@pytest.mark.parametrize('flag', ['amsgrad', 'maximize', 'capturable', 'differentiable'])
def test_unsupported_flags_raise(flag):
    with pytest.raises(ValueError, match=flag):
        optim.FusedAdamW([nn.Parameter(torch.zeros(3))], **{flag: True})


def test_bad_parameters_raise():
    with pytest.raises(ValueError, match='fp32'):
        optim.FusedAdamW([nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match='contiguous'):
        optim.FusedAdamW([nn.Parameter(torch.zeros(3, 4).t())])
    with pytest.raises(ValueError, match='at most 8'):
        optim.FusedAdamW([dict(params=[nn.Parameter(torch.zeros(2))]) for _ in range(9)])
    optim.FusedAdamW([dict(params=[nn.Parameter(torch.zeros(2))]) for _ in range(8)])
    with pytest.raises(ValueError, match='max_norm'):
        optim.FusedAdamW([nn.Parameter(torch.zeros(3))], max_norm=0.0)
    with pytest.raises(ValueError, match='track'):
        optim.ModelEMA(nn.Linear(2, 2), track='some')
    opt = optim.FusedAdamW([nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError, match='constructor'):
        opt.add_param_group(dict(params=[nn.Parameter(torch.zeros(2))]))
    with pytest.raises(ValueError, match='max_norm'):
        opt.clip_grad_norm_()


# ------------------------------------------------------------------ gradient binding
def test_gradients_stay_bound_and_a_replaced_one_is_noticed():
    model = _two_group_model(8)
    opt = optim.FusedAdamW(_groups(model), max_norm=5.0, **HYPER)
    bound = [p.grad for p in model.parameters()]
    assert all(b is not None for b in bound)
    x = torch.randn(4, 6)
    model(x).square().sum().backward()
    once = [b.clone() for b in bound]
    model(x).square().sum().backward()
    for p, b, o in zip(model.parameters(), bound, once):
        assert p.grad is b
        assert torch.equal(b, o + o)           # accumulated in place
        assert b.data_ptr() >= opt._grad_arena.data_ptr()
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is b and not b.any() for p, b in zip(model.parameters(), bound))
    model.zero_grad(set_to_none=True)
    with pytest.raises(ValueError, match=r'parameter 0 of group 0.*attach_grads'):
        opt.step()
    model(x).square().sum().backward()          # fresh tensors, not the views
    with pytest.raises(ValueError, match='attach_grads'):
        opt.step()
    fresh = [p.grad.clone() for p in model.parameters()]
    opt.attach_grads()
    for p, b, f in zip(model.parameters(), bound, fresh):
        assert p.grad is b and torch.equal(b, f)
    opt.step()
    assert opt._steps == [2, 2]


def test_untouched_parameter_is_stepped_with_a_zero_gradient():
    used, unused = nn.Parameter(torch.ones(3)), nn.Parameter(torch.ones(2))
    opt = optim.FusedAdamW([used, unused], **HYPER)
    used.square().sum().backward()
    opt.step()
    assert torch.equal(unused.detach(), torch.full((2,), 1.0).mul_(
        torch.tensor(1 - 1e-4 * 1e-2, dtype=torch.float32)))


def test_fused_ema_equals_step_then_reference_ema():
    """FusedAdamW(ema=...) followed by update() (which only counts) leaves the EMA model
    where an unfused FusedAdamW step followed by the reference loop leaves it, bit for
    bit: trained entries, the frozen parameter and the buffers."""
    torch.manual_seed(9)
    a = nn.Sequential(nn.Linear(6, 5), nn.BatchNorm1d(5), nn.Linear(5, 2))
    a[2].bias.requires_grad_(False)
    b = copy.deepcopy(a)
    ema = optim.ModelEMA(a, decay=0.999, updates=40)
    want = {k: v.clone() for k, v in b.state_dict().items()}
    fused = optim.FusedAdamW([p for p in a.parameters() if p.requires_grad], max_norm=1.0,
                             ema=ema, **HYPER)
    plain = optim.FusedAdamW([p for p in b.parameters() if p.requires_grad], max_norm=1.0,
                             **HYPER)
    g = torch.Generator().manual_seed(10)
    for it in range(3):
        x = torch.randn(8, 6, generator=g)
        for model, opt in ((a, fused), (b, plain)):
            opt.zero_grad()
            model(x).square().sum().backward()
            opt.step()
        ema.update(None, a)
        d = refs.reference_decay(0.999, 40 + it + 1)
        for k, v in want.items():
            if v.dtype.is_floating_point:
                refs.reference_ema_lines(v, d, b.state_dict()[k])
    assert ema.updates == 43
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v, want[k]), k


# ------------------------------------------------------------------ hook
def test_hook_restores_every_process_group_and_follows_the_runner(tmp_path):
    model = nn.Sequential(nn.Linear(4, 4), nn.SyncBatchNorm(4), nn.SyncBatchNorm(4))

    class NoCopy:
        def __deepcopy__(self, memo):
            raise AssertionError('a process group was deep-copied')
    groups = [NoCopy(), NoCopy()]
    model[1].process_group, model[2].process_group = groups
    wrapped = nn.Module()
    wrapped.module = model
    runner = types.SimpleNamespace(model=wrapped, epoch=2, work_dir=str(tmp_path),
                                   logger=None)
    hook = optim.MEGVIIEMAHook(init_updates=7, decay=0.99)
    hook.before_run(runner)
    assert model[1].process_group is groups[0] and model[2].process_group is groups[1]
    assert runner.ema_model.ema[1].process_group is None
    assert runner.ema_model.updates == 7
    assert runner.ema_model.decay(2000) == 0.99 * (1 - math.exp(-1))
    with torch.no_grad():
        model[0].weight.add_(1.0)
    before = runner.ema_model.ema[0].weight.clone()
    hook.after_train_iter(runner)
    assert runner.ema_model.updates == 8
    assert not torch.equal(runner.ema_model.ema[0].weight, before)
    hook.after_train_epoch(runner)
    saved = torch.load(str(tmp_path / 'epoch_3_ema.pth'))
    assert saved['epoch'] == 2 and saved['updates'] == 8
    assert torch.equal(saved['state_dict']['0.weight'], runner.ema_model.ema[0].weight)
    resumed = optim.MEGVIIEMAHook(resume=str(tmp_path / 'epoch_3_ema.pth'))
    resumed.before_run(runner)
    assert runner.ema_model.updates == 8
    assert torch.equal(runner.ema_model.ema[0].weight, saved['state_dict']['0.weight'])


def test_a_moved_parameter_or_another_model_is_noticed():
    """The record table holds addresses: a parameter or buffer whose storage was replaced
    after construction, and an update() handed another model, raise instead of reading
    the old memory."""
    model = nn.Sequential(nn.Linear(3, 3), nn.BatchNorm1d(3))
    ema = optim.ModelEMA(model, decay=0.99)
    opt = optim.FusedAdamW(model.parameters(), ema=ema, **HYPER)
    opt.step()
    ema.update(None, model)
    with pytest.raises(ValueError, match='another model'):
        ema.update(None, nn.Linear(3, 3))
    assert ema.updates == 1
    model[1].running_mean = torch.zeros(3)
    with pytest.raises(ValueError, match='1.running_mean'):
        opt.step()
    with pytest.raises(ValueError, match='1.running_mean'):
        optim.ModelEMA.update(ema)
    other = nn.Linear(3, 3)
    opt2 = optim.FusedAdamW(other.parameters(), **HYPER)
    other.weight.data = other.weight.data.clone()
    with pytest.raises(ValueError, match='parameter 0 of group 0.*no longer lives'):
        opt2.step()
