"""CPU checks of the feature-alignment training loss: the mirrors
(veon_amd/models/semantic_net/occ_loss.py) against the reference's own ``Proj2Dto3DLoss``
recorded in tests/golden/align_loss_tiny.npz (tools/gen_golden_align_loss.py), losses,
gradient and per-camera entry counts; the primitive's CPU path (veon_amd/align_loss.py)
against a direct fp64 evaluation and ``torch.autograd.gradcheck``; argument refusals; the
header's new entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden
from veon_amd import _lib
from veon_amd.align_loss import voxel_cosine
from veon_amd.models.semantic_net.occ_loss import OccLossFB, Proj2Dto3DLoss

CASES = ('open', 'mixed', 'stage2')


def fixture_inputs(g, dtype, device='cpu'):
    """The recorded inputs as the mirrors take them (float tensors in ``dtype``)."""
    def t(a):
        a = torch.from_numpy(np.asarray(a))
        return (a.to(dtype) if a.is_floating_point() else a).to(device)
    gc = g['grid_config']
    return dict(
        feat_low=t(g['feat_low']), bin_low=t(g['bin_low']), sem_seg_ds=t(g['sem_seg_ds']),
        table=t(g['ov_classifier_weight']), voxel_semantics=t(g['voxel_semantics']),
        mask_camera=t(g['mask_camera']), img_inputs=[t(g['img_inputs_%d' % i]) for i in range(11)],
        class_reflection=[int(v) for v in g['class_reflection']],
        priority=[float(v) for v in g['priority']], occ_size=tuple(int(v) for v in g['occ_size']),
        grid_config={k: [float(v) for v in gc[i]] for i, k in enumerate(('x', 'y', 'z', 'depth'))})


def build_loss(g, inp, case):
    loss = OccLossFB(grid_config=inp['grid_config'], high_conf_thr=float(g[case + '_high_conf_thr']),
                     stage2_start=int(g['stage2_start']), priority=inp['priority'],
                     ov_class_number=int(g[case + '_ov_class_number']))
    loss.epoch = int(g[case + '_epoch'])
    return loss


def selection(loss, inp, feat=None):
    """The entry lists the loss trains on (Proj2Dto3DLoss.select on the masked labels)."""
    labels = loss.masked_labels(inp['voxel_semantics'], inp['mask_camera'])
    return loss.proj2dto3dloss.select(
        inp['feat_low'] if feat is None else feat, inp['sem_seg_ds'], inp['img_inputs'], labels,
        inp['class_reflection'], inp['table'], inp['occ_size'])


def run_case(g, inp, case):
    """-> (loss dict, the loss module, d (det + soft) / d feat_low, per-camera counts
    (3, B, n_cam))"""
    loss = build_loss(g, inp, case)
    feat = inp['feat_low'].clone().requires_grad_(True)
    labels_before = inp['voxel_semantics'].clone()
    results = dict(feat_occ=feat, bin_occ=inp['bin_low'], occ_size=inp['occ_size'],
                   sem_seg_ds=inp['sem_seg_ds'], class_reflection=inp['class_reflection'],
                   ov_classifier_weight=inp['table'])
    out = loss(inp['voxel_semantics'], inp['mask_camera'], results, inp['img_inputs'],
               prev_img_inputs=[])
    assert torch.equal(inp['voxel_semantics'], labels_before)      # the caller's labels stay
    sel = selection(loss, inp)
    counts = torch.stack([torch.stack([s[k] for s in sel]) for k in ('det', 'soft', 'ignored')])
    total = sum(v / w for v, w in ((out.get('loss_featalign_det_c_0'), loss.loss_featalign_det_weight),
                                   (out.get('loss_featalign_soft_c_0'), loss.loss_featalign_soft_weight))
                if v is not None)
    grad, = torch.autograd.grad(total, feat)
    return out, loss, grad, counts.cpu()


def test_fixture_covers_every_branch():
    g = load_golden('align_loss_tiny')
    cnt = g['stage2_counts']
    assert cnt[0].sum() > 0 and cnt[1].sum() > 0 and cnt[2].sum() > 0
    assert int(g['stage2_shared_voxels']) > 0
    assert g['mixed_counts'][2].sum() == 0 and g['open_counts'][0].sum() == 1
    assert float(g['open_loss_det']) == 0.0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('case', CASES)
def test_mirror_matches_reference_fixture(case, dtype):
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, dtype)
    out, loss, grad, counts = run_case(g, inp, case)
    assert np.array_equal(counts.numpy(), g[case + '_counts'])
    ov = int(g[case + '_ov_class_number'])
    assert ('loss_featalign_det_c_0' in out) == (ov != 17)
    assert 'loss_featalign_soft_c_0' in out and 'loss_binocc_c_0' in out
    if ov != 17:
        np.testing.assert_allclose(float(out['loss_featalign_det_c_0'].detach()) / loss.loss_featalign_det_weight,
                                   float(g[case + '_loss_det']), atol=1e-5)
    np.testing.assert_allclose(float(out['loss_featalign_soft_c_0'].detach()) / loss.loss_featalign_soft_weight,
                               float(g[case + '_loss_soft']), atol=1e-5)
    np.testing.assert_allclose(float(out['loss_binocc_c_0']) / loss.loss_voxel_ce_weight,
                               float(g['loss_binocc']), atol=1e-5)
    ref = g[case + '_grad'].astype(np.float64)
    scale = np.abs(ref).max()
    assert scale > 0
    np.testing.assert_allclose(grad.double().numpy() / scale, ref / scale, atol=1e-5)


def test_proj_loss_direct_call_and_empty_selection():
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, torch.float32)
    loss = Proj2Dto3DLoss(grid_config=inp['grid_config'], ov_class_number=8,
                          priority=inp['priority'])
    free = torch.full_like(inp['voxel_semantics'], 17)
    feat = inp['feat_low'].clone().requires_grad_(True)
    det, soft = loss(feat, inp['sem_seg_ds'], None, inp['img_inputs'], voxel_semantics=free,
                     class_reflection=inp['class_reflection'],
                     ov_classifier_weight=inp['table'], occ_size=inp['occ_size'])
    assert float(det) == 0.0 and float(soft) == 0.0


def direct(feat, voxels, labels, table, occ, eps, batch):
    """cos_i by the definition, fp64, one entry at a time"""
    f_up = F.interpolate(feat[batch:batch + 1].double(), tuple(occ), mode='trilinear',
                         align_corners=False)[0]
    out = []
    for (x, y, z), k in zip(voxels.tolist(), labels.tolist()):
        f, t = f_up[:, z, y, x], table[k].double()
        out.append((f @ t) / (f.norm().clamp_min(eps) * t.norm().clamp_min(eps)))
    return torch.stack(out)


def edge_entries(occ, n, K, seed, dup=4):
    Z, Y, X = occ
    g = torch.Generator().manual_seed(seed)
    pts = [(x, y, z) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    rnd = torch.stack([torch.randint(0, s, (n,), generator=g) for s in (X, Y, Z)], 1)
    for axis, size in enumerate((X, Y, Z)):
        for v in (0, size - 1):
            f = rnd[:6].clone()
            f[:, axis] = v
            pts += [tuple(r) for r in f.tolist()]
    pts += [tuple(r) for r in rnd.tolist()]
    pts += pts[5:5 + dup] * 2                      # repeats, with other labels
    vox = torch.tensor(pts, dtype=torch.int32)
    return vox, torch.randint(0, K, (vox.shape[0],), generator=g).to(torch.int32)


@pytest.mark.parametrize('low,occ', [((2, 5, 5), (4, 10, 10)), ((3, 7, 5), (6, 14, 10)),
                                     ((2, 5, 9), (5, 11, 20))])
def test_cpu_voxel_cosine_matches_direct_fp64(low, occ):
    g = torch.Generator().manual_seed(sum(low))
    B, C, K = 2, 12, 5
    feat = torch.randn((B, C) + low, generator=g, dtype=torch.float64)
    feat[1, :, 0, 0, :2] = 0.0                      # a region of zeros
    feat[1, :, 1, 1, :2] *= 1e-8                    # and one below the clamp
    table = torch.randn(K, C, generator=g, dtype=torch.float64) * \
        torch.tensor([1e-3, 1.0, 40.0, 1.0, 0.0], dtype=torch.float64)[:, None]
    vox, lab = edge_entries(occ, 30, K, 1)
    for batch in (0, 1):
        cos = voxel_cosine(feat, vox, lab, table, occ, batch=batch)
        assert cos.shape == (vox.shape[0],) and cos.dtype == torch.float64
        torch.testing.assert_close(cos, direct(feat, vox, lab, table, occ, 1e-6, batch),
                                   rtol=0, atol=1e-12)
    cl = feat.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)   # channels-last
    torch.testing.assert_close(voxel_cosine(cl, vox, lab, table, occ, batch=1), cos, rtol=0,
                               atol=1e-15)


def test_cpu_gradient_below_the_clamp_is_autograds():
    """f = (3e-7, 4e-7), t = (3, 4), eps 1e-6: the gradient flows through the norm although
    the clamp is active (ATen clamps under a no-grad guard): u/n - (<f,u>/n^2) f/|f| =
    (3e5, 4e5), half the naive u/eps."""
    feat = torch.zeros(1, 2, 1, 1, 1, dtype=torch.float64)
    feat[0, :, 0, 0, 0] = torch.tensor([3e-7, 4e-7], dtype=torch.float64)
    feat.requires_grad_(True)
    table = torch.tensor([[3.0, 4.0]], dtype=torch.float64)
    vox = torch.zeros(1, 3, dtype=torch.int32)
    cos = voxel_cosine(feat, vox, torch.zeros(1, dtype=torch.int32), table, (1, 1, 1))
    cos.sum().backward()
    f = feat.detach()[0, :, 0, 0, 0]
    n, u = 1e-6, table[0] / 5.0
    want = u / n - (f @ u) / n ** 2 * f / f.norm()
    torch.testing.assert_close(feat.grad[0, :, 0, 0, 0], want, rtol=1e-9, atol=0)


def test_cpu_gradcheck():
    g = torch.Generator().manual_seed(3)
    low, occ, C, K = (2, 3, 2), (4, 6, 4), 4, 3
    feat = torch.randn((2, C) + low, generator=g, dtype=torch.float64, requires_grad=True)
    table = torch.randn(K, C, generator=g, dtype=torch.float64)
    vox, lab = edge_entries(occ, 6, K, 4)
    assert torch.autograd.gradcheck(
        lambda f: voxel_cosine(f, vox, lab, table, occ, batch=1), (feat,), eps=1e-6, atol=1e-6)


def test_empty_entry_list():
    feat = torch.randn(1, 4, 2, 2, 2, requires_grad=True)
    cos = voxel_cosine(feat, torch.zeros(0, 3, dtype=torch.int32),
                       torch.zeros(0, dtype=torch.int32), torch.randn(3, 4), (4, 4, 4))
    assert cos.shape == (0,)
    cos.sum().backward()
    assert torch.equal(feat.grad, torch.zeros_like(feat))


def test_bad_arguments_refused():
    feat = torch.randn(1, 4, 2, 2, 2)
    table = torch.randn(3, 4)
    occ = (4, 4, 4)
    ok_v = torch.tensor([[0, 0, 0]], dtype=torch.int32)
    ok_l = torch.tensor([0], dtype=torch.int32)
    for v in ([[4, 0, 0]], [[0, -1, 0]], [[0, 0, 4]]):
        with pytest.raises(ValueError):
            voxel_cosine(feat, torch.tensor(v, dtype=torch.int32), ok_l, table, occ)
    for lab in (-1, 3):
        with pytest.raises(ValueError):
            voxel_cosine(feat, ok_v, torch.tensor([lab], dtype=torch.int32), table, occ)
    with pytest.raises(ValueError):          # the table gets no gradient: refuse, not ignore
        voxel_cosine(feat, ok_v, ok_l, table.clone().requires_grad_(True), occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v, ok_l, torch.randn(3, 5), occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v, ok_l, table, occ, batch=1)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v[:, :2], ok_l, table, occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v, ok_l[:0], table, occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v.float(), ok_l, table, occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat[0], ok_v, ok_l, table, occ)


def test_header_declares_the_entry_points():
    names = _lib.declared_symbols()
    assert 'veon_occ_align_fwd' in names and 'veon_occ_align_bwd' in names
    assert len(_lib._SIGNATURES['veon_occ_align_fwd'][1]) == 21
    assert len(_lib._SIGNATURES['veon_occ_align_bwd'][1]) == 24
