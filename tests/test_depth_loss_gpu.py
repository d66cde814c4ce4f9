"""GPU checks of the native depth pre-training loss (csrc/depth_loss.hip through
veon_amd.depth_loss, ``LSSViewTransformerRaw.depth_pretrain_loss`` and
``VeonDepthPretrain(hip_train=True)``).

Exact: d and t against ``depth_ops.downsample_depth`` to the bit; winner positions, zero
pixels, valid / foreground flags and label bins against the fp64 closed form of
tests/depth_loss_refs.py, the non-zero pattern of the gradient against the CPU mirror's
(the builder keeps every label 1e-4 away from a bin boundary, so fp32 and fp64 take the
same bin).

Accuracy, the yardstick of tests/test_align_loss_gpu.py: with the closed form in fp64 as
the truth and the torch fp32 sequence (``depth_pretrain_loss_torch``) on the same device as
reference, e_nat <= 2 e_ref + floor for each loss, for depth_error and, element by
element, for the gradient map (e_ref the largest error of the reference over the map).
Both are fp32 evaluations of the same terms in different orders and either may be the
luckier, hence the 2.  ``floor`` guards e_ref ~ 0 and is an error model of the form
(addends + K) * 2^-24 * sum |terms|, evaluated in fp64, u = 2^-24:

  depth_error    (n + 2) u mean|d - t|: n addends, one subtraction, one division.
  loss_depth_zoe with w_i = d loss / d g_i = [(g_i - m)/(n - 1) + 0.15 m/n]/sqrt(Dg):
                 (n + 8) u sum_i |w_i| (|log d_i| + |log t_i| + |m|): g_i carries the
                 rounding of two logf relative to their own size, not to g_i; sums of n.
  its gradient   (n + 8) u [(L_i + |m| + mean_j L_j)/(n - 1) + 0.15 |m|/n]/(sqrt(Dg) d_i),
                 L_i = |log d_i| + |log t_i| >= |g_i|: the same roundings through
                 (g_i - m), the mean and sqrt(Dg).
  loss_depth_ce  row = sum_k a_k of D log addends; a gap carries 2 roundings relative to
                 |gap| <= 16 and expf one more in absolute terms, which reach the row
                 through d row / d gap_k = q_k = p_k (e_k - S):
                 0.05/max(1, n_fg) (D + 1 + 8) u sum_fg [sum_k |a_k| + sum_k |q_k| (|gap_k| + 1)].
  its gradient   sum_k q_k (-gamma sign): p_k and S are themselves (D+1)-term sums, so
                 each addend is good to (2 (D + 1) + K) u of gamma p_k (|e_k| + sum_j p_j
                 |e_j|), K = 48 = 2 * 16 (the gap roundings at |gap| <= 16 moving every
                 p) + 16 (expf, logf, divisions):
                 0.05/max(1, n_fg) (2 (D + 1) + 48) u gamma sum_k p_k (|e_k| + sum_j p_j |e_j|).

A combined gradient w_zoe zoe + w_ce ce gets the weighted sum of the two floors plus one
rounding of the result."""
import pytest
import torch

from tests import depth_loss_refs as refs
from veon_amd import _lib, depth_loss, depth_ops
from veon_amd.models import VeonDepthPretrain, build_neck
from veon_amd.models.depth_anything import DepthAnythingV2Adaptor

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
SHAPES = [(1, 2, 32, 64), (1, 1, 16, 48), (2, 6, 64, 176)]       # at label scale 16
SCALES = [(8, 16), (4, 8), (16, 16)]
ENTRY_POINTS = ('veon_depth_loss_rows', 'veon_depth_loss_reduce', 'veon_depth_loss_bwd')
W_ZOE, W_CE = 0.7, 1.3


def floors(cf, depth, gt, grid, sp, sg, gamma=4.0):
    """The module docstring's floors in fp64 -> dict(loss_depth_zoe, loss_depth_ce,
    depth_error (floats), zoe_grad, ce_grad (maps shaped as depth))."""
    D, lo, step = refs.grid_bins(grid)
    d, t, valid, fg = cf['d'], cf['t'], cf['valid'], cf['fg']
    n, n_fg = float(cf['n']), max(1.0, float(cf['n_fg']))
    L = (torch.log(d + 1e-7).abs() + torch.log(t + 1e-7).abs()) * valid
    g = (torch.log(d + 1e-7) - torch.log(t + 1e-7)) * valid
    m = g.sum() / n
    sq = cf['sqrt_Dg']
    w = (((g - m) / (n - 1) + 0.15 * m / n) / sq).abs() * valid
    f_zoe = float((n + 8) * U * (w * (L + m.abs())).sum())
    zrow = (n + 8) * U * ((L + m.abs() + L.sum() / n) / (n - 1) + 0.15 * m.abs() / n) \
        / (sq * (d + 1e-7)) * valid
    c = depth_loss.bin_centers(D, lo, step).double()
    gap = (-gamma * (d[:, None] - c[None, :]).abs()).clamp_min(-16.0)
    p = torch.softmax(gap, 1)
    y = torch.zeros_like(p).scatter_(1, cf['label_bin'][:, None], 1.0)
    keep = torch.ones_like(p)
    keep[:, D] = 0
    a = (y * torch.log(p) + (1 - y) * torch.log(1 - p)).abs() * keep
    e = ((p - y) / (p * (1 - p)).clamp_min(1e-12) * keep)
    S = (p * e).sum(1, keepdim=True)
    q = (p * (e - S)).abs()
    wce = 0.05 / n_fg
    f_ce = float(wce * (D + 1 + 8) * U * ((a.sum(1) + (q * (gap.abs() + 1)).sum(1)) * fg).sum())
    crow = wce * (2 * (D + 1) + 48) * U * gamma * \
        (p * (e.abs() + (p * e.abs()).sum(1, keepdim=True))).sum(1) * fg
    f_err = float((n + 2) * U * cf['depth_error'])

    def scatter(row):
        out = torch.zeros_like(refs.blocks(depth.double(), sp))
        out.scatter_(1, cf['winner'][:, None], row[:, None])
        return refs.unblocks(out, depth.shape, sp)
    return dict(loss_depth_zoe=f_zoe, loss_depth_ce=f_ce, depth_error=f_err,
                zoe_grad=scatter(zrow), ce_grad=scatter(crow))


def native_with_grad(depth, gt, grid, sp, sg, w_zoe=W_ZOE, w_ce=W_CE):
    D, lo, step = refs.grid_bins(grid)
    leaf = depth.detach().to(DEV).clone().requires_grad_(True)
    out = depth_loss.depth_pretrain_loss(leaf, gt.to(DEV), D, lo, step, sp, sg)
    (w_zoe * out['loss_depth_zoe'] + w_ce * out['loss_depth_ce']).backward()
    return {k: v.detach() for k, v in out.items()}, leaf.grad


_CASES = {}


def case(shape, bins, scales, clipped):
    """Inputs, fp64 closed form, floors, CPU and device fp32 mirrors of one case, computed
    once and shared (nothing in it is modified afterwards)."""
    key = (shape, bins, scales, clipped)
    if key not in _CASES:
        B, N, H, W = shape
        sp, sg = scales
        grid = refs.GRIDS[bins]
        depth, gt = refs.make_inputs(5, B, N, H * sg // 16, W * sg // 16, grid, sp, sg, clipped)
        cf = refs.closed_form(depth, gt, grid, sp, sg, w_zoe=W_ZOE, w_ce=W_CE)
        _CASES[key] = dict(
            depth=depth, gt=gt, grid=grid, sp=sp, sg=sg, cf=cf,
            floors=floors(cf, depth, gt, grid, sp, sg),
            cpu32=refs.mirror_with_grad(depth, gt, grid, sp, sg, w_zoe=W_ZOE, w_ce=W_CE),
            dev32=refs.mirror_with_grad(depth, gt, grid, sp, sg, device=DEV, w_zoe=W_ZOE,
                                        w_ce=W_CE))
    return _CASES[key]


def check_case(c, what):
    depth, gt, grid, sp, sg, cf, fl = (c[k] for k in ('depth', 'gt', 'grid', 'sp', 'sg', 'cf',
                                                      'floors'))
    D, lo, step = refs.grid_bins(grid)
    n0 = dict(_lib.CALLS)
    out, grad = native_with_grad(depth, gt, grid, sp, sg)
    for name in ENTRY_POINTS:
        assert _lib.CALLS.get(name, 0) == n0.get(name, 0) + 1, name
    # ---- exact: the row records
    rec = depth_loss.unpack_rows(depth_loss.loss_rows(depth.to(DEV), gt.to(DEV), D, lo, step,
                                                      sp, sg))
    assert torch.equal(rec['d'], depth_ops.downsample_depth(depth.to(DEV), sp).reshape(-1))
    assert torch.equal(rec['t'], depth_ops.downsample_depth(gt.to(DEV), sg).reshape(-1))
    for k in ('winner', 'winner_zero', 'label_bin', 'valid', 'fg'):
        assert torch.equal(rec[k].cpu().long(), cf[k].long()), k
    # winner positions.  A row whose d lies beyond the last centre has the same slope sign
    # on every bin, so its ce gradient is sum_k q_k = 0 up to rounding: only the zoe term
    # makes its winner non-zero, and the patterns are compared where that term is alive
    live = refs.blocks(torch.zeros_like(depth), sp)
    live.scatter_(1, cf['winner'][:, None], (~cf['winner_zero']).float()[:, None])
    live = refs.unblocks(live, depth.shape, sp) != 0
    assert not grad.cpu()[~live].any() and torch.isfinite(grad).all()
    if not cf['clipped']:
        _, cpu_grad = c['cpu32']
        assert torch.equal(grad.cpu() != 0, cpu_grad != 0)
        assert torch.equal(grad.cpu() != 0, cf['grad'] != 0)
    # ---- accuracy: e_nat <= 2 e_ref + floor
    ref_out, ref_grad = c['dev32']
    for k in ('loss_depth_zoe', 'loss_depth_ce', 'depth_error'):
        e_nat = abs(float(out[k].double().cpu()) - float(cf[k]))
        e_ref = abs(float(ref_out[k].double().cpu()) - float(cf[k]))
        print('%s %s: %.7g  e_nat %.3e  e_ref %.3e  floor %.3e'
              % (what, k, float(cf[k]), e_nat, e_ref, fl[k]))
        assert e_nat <= 2 * e_ref + fl[k], (k, e_nat, e_ref, fl[k])
    g64 = cf['grad']
    floor = W_ZOE * fl['zoe_grad'] + W_CE * fl['ce_grad'] + U * g64.abs()
    err_nat = (grad.cpu().double() - g64).abs()
    err_ref = (ref_grad.cpu().double() - g64).abs()
    # a device min may break the planted tie otherwise than the contract: leave those
    # elements out of the reference's error
    same = (ref_grad.cpu() != 0) == (g64 != 0)
    e_nat, e_ref = float(err_nat.max()), float((err_ref * same).max())
    over = float((err_nat - floor).max())
    print('%s grad: max %.3e  e_nat %.3e  e_ref %.3e  max floor %.3e'
          % (what, float(g64.abs().max()), e_nat, e_ref, float(floor.max())))
    assert over <= 2 * e_ref, (over, e_nat, e_ref)
    if cf['clipped']:
        _, zgrad = native_with_grad(depth, gt, grid, sp, sg, w_zoe=1.0, w_ce=0.0)
        assert not zgrad.any()                   # the zoe part is exactly 0
        assert float(out['loss_depth_zoe']) == 2.0


@pytest.mark.parametrize('clipped', [False, True])
@pytest.mark.parametrize('bins', sorted(refs.GRIDS))
@pytest.mark.parametrize('shape', SHAPES)
def test_shapes_and_depth_grids(shape, bins, clipped):
    check_case(case(shape, bins, (8, 16), clipped), 'rows %s D+1 %d clipped %d'
               % (shape, bins, clipped))


@pytest.mark.parametrize('scales', SCALES[1:])
@pytest.mark.parametrize('shape', SHAPES)
def test_scale_pairs(shape, scales):
    check_case(case(shape, 89, scales, False), 'rows %s scales %s' % (shape, scales))
    check_case(case(shape, 60, scales, True), 'rows %s scales %s clipped' % (shape, scales))


def _native(depth, gt, grid, sp=8, sg=16, **kw):
    D, lo, step = refs.grid_bins(grid)
    return depth_loss.depth_pretrain_loss(depth, gt, D, lo, step, sp, sg, **kw)


def test_no_foreground_row():
    """every label beyond the last centre: loss_depth_ce is exactly 0 with zero gradient"""
    grid = refs.GRIDS[64]
    depth, gt = refs.make_inputs(5, 1, 2, 32, 64, grid, plant=False)
    gt = torch.where(gt > 0, gt + 60.0, gt).to(DEV)
    leaf = depth.to(DEV).requires_grad_(True)
    out = _native(leaf, gt, grid)
    assert float(out['loss_depth_ce']) == 0.0 and out['loss_depth_zoe'] > 0
    grad, = torch.autograd.grad(out['loss_depth_ce'], leaf)
    assert not grad.any()


@pytest.mark.parametrize('n_valid', [0, 1])
def test_fewer_than_two_valid_rows(n_valid):
    """the forward returns what the torch formulation returns, NaN included (1e-5
    relative on what is finite: the bound of this project's fp32 mirrors)"""
    grid = refs.GRIDS[89]
    depth, gt = refs.make_inputs(5, 1, 2, 32, 64, grid, plant=False)
    keep = refs.blocks(gt, 16).clone()
    keep[n_valid:] = 0
    gt = refs.unblocks(keep, gt.shape, 16).contiguous()
    D, lo, step = refs.grid_bins(grid)
    want = depth_loss.depth_pretrain_loss_torch(depth.to(DEV), gt.to(DEV), D, lo, step)
    got = _native(depth.to(DEV), gt.to(DEV), grid)
    assert torch.isnan(want['loss_depth_zoe']) and torch.isnan(got['loss_depth_zoe'])
    assert bool(torch.isnan(want['depth_error'])) == bool(torch.isnan(got['depth_error'])) \
        == (n_valid == 0)
    for k in ('loss_depth_ce', 'depth_error'):
        if not torch.isnan(want[k]):
            assert abs(float(got[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), k


def test_repeatable_and_every_element_written():
    c = case(SHAPES[2], 89, (8, 16), False)
    depth, gt, grid = c['depth'].to(DEV), c['gt'].to(DEV), c['grid']
    D, lo, step = refs.grid_bins(grid)
    a_out, a_grad = native_with_grad(depth, gt, grid, 8, 16)
    b_out, b_grad = native_with_grad(depth, gt, grid, 8, 16)
    assert all(torch.equal(a_out[k], b_out[k]) for k in a_out) and torch.equal(a_grad, b_grad)
    # the low-level backward into a poisoned buffer
    rec = depth_loss.loss_rows(depth, gt, D, lo, step)
    out, coef = depth_loss.loss_reduce(rec)
    gz = torch.tensor(W_ZOE, device=DEV)
    gc = torch.tensor(W_CE, device=DEV)
    buf = torch.full(depth.shape, float('nan'), device=DEV)
    got = depth_loss.loss_backward(rec, coef, depth.shape, 8, gz, gc, out=buf)
    assert got is buf and not torch.isnan(buf).any() and torch.equal(buf, a_grad)
    buf.fill_(float('nan'))
    depth_loss.loss_backward(rec, coef, depth.shape, 8, None, gc, out=buf)
    assert not torch.isnan(buf).any()


def test_selected_losses():
    c = case(SHAPES[0], 89, (8, 16), False)
    depth, gt, grid = c['depth'].to(DEV), c['gt'].to(DEV), c['grid']
    both = _native(depth, gt, grid)
    for zoe, ce in [(False, False), (True, False), (False, True)]:
        out = _native(depth, gt, grid, zoe=zoe, ce=ce)
        assert set(out) == {k for k, on in (('loss_depth_zoe', zoe), ('loss_depth_ce', ce),
                                            ('depth_error', True)) if on}
        assert all(torch.equal(out[k], both[k]) for k in out)


def test_unsupported_inputs_are_refused():
    grid = refs.GRIDS[89]
    depth, gt = (t.to(DEV) for t in refs.make_inputs(5, 1, 2, 32, 64, grid))
    with pytest.raises(_lib.VeonHipError):
        _native(depth.double(), gt.double(), grid)
    with pytest.raises(_lib.VeonHipError):
        _native(depth.transpose(2, 3), gt.transpose(2, 3), grid)
    with pytest.raises(_lib.VeonHipError):
        _native(depth[..., :24], gt, grid)                        # w mismatch (and strided)
    with pytest.raises(_lib.VeonHipError):
        _native(depth[:, :, :12].contiguous(), gt, grid)          # H not a multiple of 8
    rec = torch.empty(16, 8, device=DEV)
    for bad in [dict(Hp=12), dict(sp=3), dict(Hg=48), dict(D=0)]:
        a = dict(BN=2, Hp=16, Wp=32, sp=8, Hg=32, Wg=64, sg=16, D=88)
        a.update(bad)
        with pytest.raises(_lib.VeonHipError):
            _lib.launch('veon_depth_loss_rows', depth.device, a['BN'], a['Hp'], a['Wp'], a['sp'],
                        a['Hg'], a['Wg'], a['sg'], a['D'], 1.0, 0.5, 4.0, depth, gt, rec)


def test_graph_capture_forward_and_backward():
    """forward + backward captured in one graph on a side stream, upstream gradients as
    device tensors: the replay is bit-equal to eager and follows the inputs in place, so
    nothing in the path reads the device back"""
    grid = refs.GRIDS[89]
    D, lo, step = refs.grid_bins(grid)
    first = refs.make_inputs(5, 1, 2, 32, 64, grid)
    second = refs.make_inputs(6, 1, 2, 32, 64, grid, clipped=True)
    depth = first[0].to(DEV).requires_grad_(True)
    gt = first[1].to(DEV)
    gz, gc = torch.tensor(W_ZOE, device=DEV), torch.tensor(W_CE, device=DEV)

    def step_fn():
        out = depth_loss.depth_pretrain_loss(depth, gt, D, lo, step)
        grad, = torch.autograd.grad([out['loss_depth_zoe'], out['loss_depth_ce']], depth,
                                    [gz, gc])
        return out['loss_depth_zoe'], out['loss_depth_ce'], out['depth_error'], grad

    def eager():
        return [t.detach().clone() for t in step_fn()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step_fn()                                                  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    want = eager()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        held = step_fn()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, want))
    with torch.no_grad():
        depth.copy_(second[0])
        gt.copy_(second[1])
        gz.fill_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in held]
    want = eager()
    assert float(want[0]) == 2.0 and not torch.equal(want[3], torch.zeros_like(want[3]))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_veon_depth_pretrain_hip_train():
    torch.manual_seed(0)
    grid = refs.GRIDS[89]
    model = VeonDepthPretrain(
        depth_estimator=DepthAnythingV2Adaptor('vits', lora_r=4, max_depth=40.0),
        img_view_transformer=build_neck(dict(
            type='LSSViewTransformerRaw',
            grid_config={'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0],
                         'z': [-1.0, 3.0, 1.0], 'depth': list(grid)},
            input_size=(32, 64), out_channels=8, collapse_z=False)),
        hip_train=True)
    est = dict(model.depth_estimator.named_parameters())
    with torch.no_grad():
        for n, p in est.items():
            if n.endswith('lora_B'):             # zero-initialised: would hide lora_A's gradient
                p.normal_(0, 0.02)
    model.to(DEV).train()
    assert all(b.hip_train for b in model.depth_estimator.pretrained.blocks)
    g = torch.Generator().manual_seed(1)
    _, gt = refs.make_inputs(5, 1, 2, 32, 64, grid, plant=False)
    seen = {}
    vt = model.img_view_transformer
    inner = vt.depth_pretrain_loss

    def recorder(depth, gt_depth, *a):
        seen['depth'], seen['gt'] = depth.detach().clone(), gt_depth.detach().clone()
        return inner(depth, gt_depth, *a)
    vt.depth_pretrain_loss = recorder
    n0 = dict(_lib.CALLS)
    losses = model.forward_train(img_inputs=[torch.zeros(1, 2, 3, 32, 64, device=DEV)],
                                 depth_img_inputs=torch.randn(1, 2, 3, 56, 112,
                                                              generator=g).to(DEV),
                                 gt_depth=gt.to(DEV))
    sum(losses.values()).backward()
    for name in ENTRY_POINTS:
        assert _lib.CALLS.get(name, 0) == n0.get(name, 0) + 1, name
    assert set(losses) == {'loss_depth_zoe', 'loss_depth_ce'}
    assert tuple(seen['depth'].shape) == (1, 2, 16, 32)
    D, lo, step = refs.grid_bins(grid)
    want = depth_loss.depth_pretrain_loss(seen['depth'], seen['gt'], D, lo, step)
    assert all(torch.equal(losses[k].detach(), want[k]) for k in losses)
    assert torch.equal(model.avg_depth_error, want['depth_error']) and model.nonce == 1
    frozen = {n for n in est if n.startswith('pretrained.') and 'lora' not in n}
    unused = {n for n in est if n.startswith('depth_head.scratch.refinenet4.resConfUnit1.')}
    assert all(est[n].grad is None for n in frozen)
    for n in set(est) - frozen - unused:
        assert est[n].grad is not None and torch.isfinite(est[n].grad).all() \
            and est[n].grad.any(), n
