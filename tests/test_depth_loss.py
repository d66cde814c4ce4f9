"""CPU checks of the depth pre-training loss (veon_amd/depth_loss.py, the
``LSSViewTransformerRaw`` methods and ``VeonDepthPretrain``):

(a) the torch mirror reproduces every case of tests/golden/depth_loss_tiny.npz (the
    reference's own ``downsample_depth`` + ``get_depth_loss_own`` and autograd), losses and
    gradient, to 1e-5 relative: the bound this project pins its fp32 CPU mirrors at;
(b) the closed form of tests/depth_loss_refs.py equals fp64 autograd of the mirror to
    1e-12 absolute on the gradient map (terms are O(1) sums of <= 90 addends);
(c) the tie goes to (0, 0); zeroed pixels and invalid rows get exactly 0;
(d) the header declares the three entry points and both libraries export them;
(e) ``VeonDepthPretrain`` freezes exactly the non-LoRA ``pretrained.*`` parameters and a
    CPU forward_train + backward gives gradients to exactly the others."""
import ctypes

import pytest
import torch

from tests import depth_loss_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, depth_loss
from veon_amd.models import VeonDepthPretrain, build_neck
from veon_amd.models.depth_anything import DepthAnythingV2Adaptor

RTOL = 1e-5
ENTRY_POINTS = ('veon_depth_loss_rows', 'veon_depth_loss_reduce', 'veon_depth_loss_bwd')


def view_transformer(grid):
    return build_neck(dict(type='LSSViewTransformerRaw',
                           grid_config={'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0],
                                        'z': [-1.0, 3.0, 1.0], 'depth': list(grid)},
                           input_size=(32, 64), out_channels=8, collapse_z=False))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('case', ['unclipped', 'clipped'])
@pytest.mark.parametrize('zoe,ce', [(False, False), (False, True), (True, False), (True, True)])
def test_mirror_reproduces_the_reference(case, zoe, ce):
    gold = load_golden('depth_loss_tiny')
    grid = tuple(float(v) for v in gold['grid'])
    sp, sg = int(gold['pred_scale']), int(gold['gt_scale'])
    vt = view_transformer(grid)
    assert vt.D == refs.grid_bins(grid)[0]
    depth = torch.from_numpy(gold[case + '_depth']).requires_grad_(True)
    gt = torch.from_numpy(gold[case + '_gt_depth'])
    tag = '%s_z%dc%d_' % (case, zoe, ce)
    # the class methods, as forward_train strings them together
    pred_ds, gt_ds = vt.downsample_depth(depth, sp), vt.downsample_depth(gt, sg)
    losses = vt.get_depth_loss_own(gt_ds, pred_ds, zoe=zoe, ce=ce)
    assert set(losses) == {k for k, on in (('loss_depth_zoe', zoe), ('loss_depth_ce', ce)) if on}
    for k, v in losses.items():
        assert rel(v.detach(), gold[tag + k]) <= RTOL, (k, float(v), float(gold[tag + k]))
    if losses:
        grad, = torch.autograd.grad(sum(losses.values()), depth)
        assert rel(grad, gold[tag + 'grad']) <= RTOL
        assert torch.equal(grad != 0, torch.from_numpy(gold[tag + 'grad']) != 0)
    # and the one-call form (the CPU path of depth_pretrain_loss)
    D, lo, step = refs.grid_bins(grid)
    out = depth_loss.depth_pretrain_loss(depth, gt, D, lo, step, sp, sg, zoe=zoe, ce=ce)
    assert set(out) == set(losses) | {'depth_error'}
    assert not out['depth_error'].requires_grad
    assert rel(out['depth_error'], gold[case + '_depth_error']) <= RTOL
    for k in losses:
        assert rel(out[k].detach(), gold[tag + k]) <= RTOL
    if zoe and ce:
        both = vt.depth_pretrain_loss(depth, gt, sp, sg)
        assert all(torch.equal(both[k], out[k]) for k in out)


@pytest.mark.parametrize('clipped', [False, True])
@pytest.mark.parametrize('sp,sg', [(8, 16), (4, 8), (16, 16)])
@pytest.mark.parametrize('bins', sorted(refs.GRIDS))
def test_closed_form_is_fp64_autograd_of_the_mirror(bins, sp, sg, clipped):
    grid = refs.GRIDS[bins]
    depth, gt = refs.make_inputs(5, 1, 2, 2 * sg, 4 * sg, grid, sp, sg, clipped)
    cf = refs.closed_form(depth, gt, grid, sp, sg, w_zoe=0.7, w_ce=1.3)
    out, grad = refs.mirror_with_grad(depth, gt, grid, sp, sg, dtype=torch.float64,
                                      w_zoe=0.7, w_ce=1.3)
    assert cf['clipped'] == clipped and cf['n'] >= 2 and cf['n_fg'] >= 1
    err = float((grad - cf['grad']).abs().max())
    print('D+1 %d (%d, %d) clipped %d: max|closed - autograd| %.2e' % (bins, sp, sg, clipped, err))
    assert err <= 1e-12
    for k in ('loss_depth_zoe', 'loss_depth_ce', 'depth_error'):
        assert abs(float(out[k]) - float(cf[k])) <= 1e-12 * max(1.0, abs(float(cf[k])))
    if clipped:
        assert not cf['zoe_grad'].any()


def test_ties_zero_pixels_and_invalid_rows():
    grid, sp, sg = refs.GRIDS[89], 8, 16
    depth, gt = refs.make_inputs(5, 1, 2, 32, 64, grid, sp, sg)
    _, grad = refs.mirror_with_grad(depth, gt, grid, sp, sg)
    gb, pb = refs.blocks(grad, sp), refs.blocks(depth, sp)
    row = {name: r for r, name in enumerate(refs.PLANTED)}
    # two equal minima at (0,0) and (1,1): the gradient goes to (0,0) alone
    r = row['pred_tie']
    assert pb[r, 0] == pb[r, sp + 1] == pb[r].min()
    assert gb[r, 0] != 0 and not gb[r, 1:].any()
    # zeroed pixels get exactly 0, the smallest non-zero pixel gets the gradient
    r = row['pred_zeros']
    assert (pb[r] == 0).sum() > 1 and not gb[r][pb[r] == 0].any()
    assert gb[r].nonzero().flatten().tolist() == \
        [int(torch.where(pb[r] == 0, torch.full_like(pb[r], 1e5), pb[r]).argmin())]
    # an all-zero block: d is the constant 1e5
    assert not gb[row['pred_all_zero_label_9224_9']].any()
    # invalid rows (all-zero label block, label 9225): neither loss reaches them
    assert not gb[row['label_all_zero']].any() and not gb[row['label_9225']].any()
    # valid but not foreground rows still get the zoe gradient
    assert gb[row['label_beyond']].any() and gb[row['label_over_500']].any()
    assert (gb != 0).sum(1).max() == 1


def test_header_declares_and_libraries_export_the_entry_points():
    from veon_amd import build
    build.build()
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    ptr, i = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES['veon_depth_loss_reduce'] == (i, [ctypes.c_int64, ptr, ptr, ptr, ptr])
    assert _lib._SIGNATURES['veon_depth_loss_bwd'] == (i, [i] * 4 + [ptr] * 6)
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), (flavour, name)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2      # the additions are additive


def test_unsupported_shapes_are_refused():
    D, lo, step = refs.grid_bins(refs.GRIDS[89])
    ok = torch.rand(1, 2, 16, 32) + 1
    for depth, gt, sp, sg in [(ok, torch.rand(1, 2, 32, 48), 8, 16),      # w mismatch
                              (torch.rand(1, 2, 12, 32), torch.rand(1, 2, 32, 64), 8, 16),
                              (ok, torch.rand(1, 2, 32, 64), 3, 6),
                              (ok, torch.rand(1, 3, 32, 64), 8, 16)]:
        with pytest.raises(ValueError):
            depth_loss.depth_pretrain_loss(depth, gt, D, lo, step, sp, sg)
    with pytest.raises(_lib.VeonHipError):        # the native entry has no CPU path
        depth_loss.loss_rows(ok, torch.rand(1, 2, 32, 64), D, lo, step)


def test_veon_depth_pretrain_freezes_and_trains_the_right_parameters():
    torch.manual_seed(0)
    model = VeonDepthPretrain(
        depth_estimator=DepthAnythingV2Adaptor('vits', lora_r=4, max_depth=40.0),
        img_view_transformer=dict(type='LSSViewTransformerRaw',
                                  grid_config={'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0],
                                               'z': [-1.0, 3.0, 1.0], 'depth': [1.0, 45.0, 0.5]},
                                  input_size=(32, 64), out_channels=8, collapse_z=False))
    assert (model.pred_depth_scale, model.gt_depth_scale, model.hip_train) == (8, 16, False)
    est = dict(model.depth_estimator.named_parameters())
    frozen = {n for n in est if n.startswith('pretrained.') and 'lora' not in n}
    assert frozen and {n for n, p in est.items() if not p.requires_grad} == frozen
    assert any('lora' in n for n in est) and any(n.startswith('depth_head.') for n in est)
    for p in model.parameters():                  # train() re-applies the rule
        p.requires_grad = True
    model.train()
    assert {n for n, p in est.items() if not p.requires_grad} == frozen
    # LoRA's B matrices start at zero, which would hide the A matrices' gradient
    with torch.no_grad():
        for n, p in est.items():
            if n.endswith('lora_B'):
                p.normal_(0, 0.02)
    g = torch.Generator().manual_seed(1)
    _, gt = refs.make_inputs(5, 1, 2, 32, 64, refs.GRIDS[89], plant=False)
    losses = model.forward_train(img_inputs=[torch.zeros(1, 2, 3, 32, 64)],
                                 depth_img_inputs=torch.randn(1, 2, 3, 56, 112, generator=g),
                                 gt_depth=gt)
    assert set(losses) == {'loss_depth_zoe', 'loss_depth_ce'}
    assert all(torch.isfinite(v) for v in losses.values())
    assert model.nonce == 1 and model.avg_depth_error.dim() == 0 and model.avg_depth_error > 0
    sum(losses.values()).backward()
    with_grad = {n for n, p in est.items() if p.grad is not None}
    # the DPT head's deepest fusion block has one input, so its first residual unit is
    # never called (in the reference's DPT as well): trainable, but outside the graph
    unused = {n for n in est if n.startswith('depth_head.scratch.refinenet4.resConfUnit1.')}
    assert len(unused) == 4 and with_grad == set(est) - frozen - unused
    assert all(torch.isfinite(est[n].grad).all() and est[n].grad.any() for n in with_grad)
