"""The label-only tail and the confusion-matrix kernels (csrc/occ_tail.hip, csrc/occ_eval.hip).

Labels: bit-equal to the labels of ``conv3d_ops.occ_classify`` (same code, library built
without FMA contraction) on every case of tests/edge_refs.py, in both instantiations and
with strided occupancy logits; and equal to the float64 reference outside its undecided
set, under the cap the existing edge tests hold ``occ_classify`` to.
Histograms: integer counts, so everything is compared exactly -- the fused histogram,
``confusion`` of the same labels (uint8 and int64) and numpy's bincount under the
reference's rule (mmdet3d/datasets/occ_metrics.py:78-147)."""
import functools

import numpy as np
import pytest
import torch

from tests import edge_refs as er
from veon_amd import _lib, conv3d_ops
from veon_amd.occ_eval import OccMiouMetric, confusion, occ_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = sorted(n for n, c in er.OCC_CASES.items() if c[1] <= 254)


def _channels_last(x):
    """(B,Q,z,y,x) -> the same values as a channels-last view of 16-byte rows (the VEC4
    instantiation); the surplus floats are NaN."""
    B, Q, z, y, xx = x.shape
    row = (Q + 3) // 4 * 4
    rows = torch.full((B, z, y, xx, row), float('nan'), device=x.device)
    rows[..., :Q] = x.permute(0, 2, 3, 4, 1)
    return rows[..., :Q].permute(0, 4, 1, 2, 3)


def _strided_bin(bin_d):
    """The occupancy logits as a channel slice of a transposed volume."""
    B, _, z, y, x = bin_d.shape
    wide = torch.full((B, z, 8, y, x), float('nan'), device=bin_d.device)
    wide[:, :, :2] = bin_d.transpose(1, 2)
    strided = wide.transpose(1, 2)[:, :2]
    assert strided.stride(0) == 4 * bin_d.stride(0) and strided.stride(2) == 8 * y * x
    return strided


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(sem_low, bin_low on the device, size, the labels of occ_classify as uint8), once
    per case and never written."""
    if name == 'integer':
        sem_low, bin_low, size = er.occ_integer_inputs()
    elif name == 'special':
        sem_low, bin_low, size, _ = er.occ_special_inputs()
    else:
        sem_low, bin_low, size = er.occ_inputs(name)
    sem_d, bin_d = sem_low.to(DEV), bin_low.to(DEV)
    want = conv3d_ops.occ_classify(sem_d, bin_d, size)[2]
    assert int(want.min()) >= 0 and int(want.max()) <= sem_low.shape[1]
    return sem_d, bin_d, size, want.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _truth(name, seed=0):
    """Seeded ground truth in [0, n_cl) with ~10 % 255 and a mask with ~30 % zeros, on
    the device, shaped as the labels."""
    sem_d, _, size, want = _inputs(name)
    n_cl = sem_d.shape[1] + 1
    g = torch.Generator().manual_seed(1000 + seed)
    gt = torch.randint(0, n_cl, want.shape, generator=g, dtype=torch.uint8)
    gt[torch.rand(want.shape, generator=g) < 0.1] = 255
    mask = (torch.rand(want.shape, generator=g) >= 0.3).to(torch.uint8)
    return gt.to(DEV), mask.to(DEV), n_cl


def _bincount(labels, gt, mask, n_cl):
    """hist_info after add_batch's masking, in numpy (occ_metrics.py:94-101, 123-125)."""
    lab, g = labels.cpu().numpy().reshape(-1), gt.cpu().numpy().reshape(-1)
    k = g < n_cl
    if mask is not None:
        k &= mask.cpu().numpy().reshape(-1) != 0
    return torch.from_numpy(np.bincount(n_cl * g[k].astype(int) + lab[k].astype(int),
                                        minlength=n_cl ** 2).reshape(n_cl, n_cl))


def _hist(n_cl):
    return torch.zeros((n_cl, n_cl), dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------ labels
@pytest.mark.parametrize('name', CASES + ['integer', 'special'])
def test_labels_equal_occ_classify_bit_for_bit(name):
    sem_d, bin_d, size, want = _inputs(name)
    forms = {'scalar': (sem_d, bin_d), 'vec4': (_channels_last(sem_d), bin_d),
             'strided bin': (sem_d, _strided_bin(bin_d)),
             'vec4, strided bin': (_channels_last(sem_d), _strided_bin(bin_d))}
    assert forms['vec4'][0].stride(1) == 1 and forms['vec4'][0].data_ptr() % 16 == 0
    for key, (s, b) in forms.items():
        got = occ_labels(s, b, size)
        assert got.dtype == torch.uint8 and got.shape == want.shape, key
        assert torch.equal(got, want), (name, key, int((got != want).sum()))
        # ... and of the very call it is compared with
        assert torch.equal(got, conv3d_ops.occ_classify(s, b, size)[2].to(torch.uint8)), key


@pytest.mark.parametrize('name', CASES)
def test_labels_against_the_float64_reference(name):
    sem_d, bin_d, size, _ = _inputs(name)
    Q = sem_d.shape[1]
    r = er.occ_tail_ref(sem_d.cpu(), bin_d.cpu(), size)
    und = r.undecided()
    share = und.double().mean().item()
    for form, s in (('scalar', sem_d), ('vec4', _channels_last(sem_d))):
        occ = occ_labels(s, bin_d, size).cpu().long()
        differ = (occ != r.labels).permute(0, 3, 2, 1)
        print('%s %s: undecided share %.2e, labels differing %d'
              % (name, form, share, int(differ.sum())))
        assert share < er.UNDECIDED_CAP, (name, share)
        assert not bool((differ & ~und).any()), (name, form, int((differ & ~und).sum()))
        assert int(occ.min()) >= 0 and int(occ.max()) <= Q


# --------------------------------------------------------------------------- histogram
# Zo 6, 5, 9 (byte stores), 4, 8 and 16 (4-, 8- and 16-byte stores)
@pytest.mark.parametrize('name', ['small', 'ragged', 'q40', 'veon', 'equal', 'q17'])
def test_fused_histogram_confusion_and_bincount_agree(name):
    sem_d, bin_d, size, want = _inputs(name)
    gt, mask, n_cl = _truth(name)
    fused = _hist(n_cl)
    labels = occ_labels(_channels_last(sem_d), bin_d, size, gt, mask, fused)
    assert torch.equal(labels, want)
    ref = _bincount(labels, gt, mask, n_cl)
    assert 0 < int(ref.sum()) < labels.numel() and int((ref > 0).sum()) > 1
    assert torch.equal(fused.cpu(), ref), name
    scalar = _hist(n_cl)
    occ_labels(sem_d, bin_d, size, gt, mask, scalar)
    assert torch.equal(scalar, fused)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pred in (labels, labels.long()):
        assert torch.equal(confusion(pred, gt, mask, n_cl, flag=flag).cpu(), ref), pred.dtype
    assert int(flag) == 0


def test_histogram_seams():
    sem_d, bin_d, size, want = _inputs('q17')
    gt, mask, n_cl = _truth('q17')
    n = want.numel()
    # no mask
    h = _hist(n_cl)
    occ_labels(sem_d, bin_d, size, gt, None, h)
    assert torch.equal(h.cpu(), _bincount(want, gt, None, n_cl))
    assert torch.equal(confusion(want, gt, None, n_cl), h)
    # a second call doubles it exactly; hist is accumulated into, never cleared
    once = h.clone()
    occ_labels(sem_d, bin_d, size, gt, None, h)
    assert torch.equal(h, 2 * once)
    # mask all zero: the given histogram is untouched
    marked = torch.arange(n_cl * n_cl, device=DEV).view(n_cl, n_cl)
    h = marked.clone()
    assert torch.equal(occ_labels(sem_d, bin_d, size, gt, torch.zeros_like(mask), h), want)
    assert torch.equal(h, marked)
    assert torch.equal(confusion(want, gt, torch.zeros_like(mask), n_cl, h), marked)
    # ground truth all 255
    occ_labels(sem_d, bin_d, size, torch.full_like(gt, 255), mask, h)
    assert torch.equal(confusion(want, torch.full_like(gt, 255), mask, n_cl, h), marked)
    # ground truth and mask one byte off every alignment: byte accesses, same counts
    off = [torch.empty(n + 1, dtype=torch.uint8, device=DEV)[1:].view(want.shape) for _ in 'gm']
    off[0].copy_(gt), off[1].copy_(mask)
    assert off[0].data_ptr() % 4 == 1
    h = _hist(n_cl)
    assert torch.equal(occ_labels(sem_d, bin_d, size, off[0], off[1], h), want)
    assert torch.equal(h.cpu(), _bincount(want, gt, mask, n_cl))
    assert torch.equal(confusion(want, off[0], off[1], n_cl), h)
    assert torch.equal(confusion(want.long(), off[0], off[1], n_cl), h)
    # gt without hist, hist without gt, a mask alone: refused
    for bad in ((gt, None, None), (None, None, _hist(n_cl)), (None, mask, None)):
        with pytest.raises(_lib.VeonHipError):
            occ_labels(sem_d, bin_d, size, *bad)


def test_every_voxel_in_one_bin():
    B, Q, low, size = 2, 5, (3, 7, 5), (6, 14, 10)
    sem = torch.zeros(B, Q, *low, device=DEV)
    sem[:, 2] = 1.0
    binv = torch.zeros(B, 2, *low, device=DEV)
    binv[:, 0] = 1.0
    n = B * size[0] * size[1] * size[2]
    gt = torch.full((B, size[2], size[1], size[0]), 3, dtype=torch.uint8, device=DEV)
    h = _hist(Q + 1)
    labels = occ_labels(sem, binv, size, gt, None, h)
    assert bool((labels == 2).all())
    want = torch.zeros_like(h)
    want[3, 2] = n
    assert torch.equal(h, want)
    assert torch.equal(confusion(labels, gt, None, Q + 1), want)
    assert torch.equal(confusion(labels.long(), gt, None, Q + 1), want)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 99991])
def test_confusion_sizes(n):
    n_cl = 18
    g = torch.Generator().manual_seed(n)
    pred = torch.randint(0, n_cl, (n,), generator=g, dtype=torch.uint8)
    gt = torch.randint(0, n_cl, (n,), generator=g, dtype=torch.uint8)
    gt[torch.rand(n, generator=g) < 0.1] = 255
    mask = (torch.rand(n, generator=g) >= 0.3).to(torch.uint8)
    mask[0] = 1
    gt[0] = 4
    want = confusion(pred, gt, mask, n_cl)                     # torch.bincount on the CPU
    assert torch.equal(want, _bincount(pred, gt, mask, n_cl))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for p in (pred, pred.long()):
        got = confusion(p.to(DEV), gt.to(DEV), mask.to(DEV), n_cl, flag=flag)
        assert torch.equal(got.cpu(), want), (n, p.dtype)
        assert torch.equal(confusion(p.to(DEV), gt.to(DEV), None, n_cl).cpu(),
                           _bincount(pred, gt, None, n_cl))
    assert int(flag) == 0
    # a counted prediction out of range: in no bin, and the flag is up
    for p, value in ((pred.clone(), n_cl), (pred.long(), -1), (pred.long(), 1 << 40)):
        hit = int(want[4, int(pred[0])])
        p[0] = value
        got = confusion(p.to(DEV), gt.to(DEV), mask.to(DEV), n_cl, flag=flag.zero_())
        assert int(flag) == 1
        assert int(got[4, int(pred[0])]) == hit - 1 and int(got.sum()) == int(want.sum()) - 1
    # ... but not where the voxel does not count
    p = pred.clone()
    p[0] = 200
    gt2 = gt.clone()
    gt2[0] = 255
    confusion(p.to(DEV), gt2.to(DEV), mask.to(DEV), n_cl, flag=flag.zero_())
    assert int(flag) == 0


def test_more_than_64_classes_are_refused():
    pred = torch.zeros(16, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.VeonHipError, match='status 1'):
        confusion(pred, pred, None, n_cl=65)
    confusion(pred, pred, None, n_cl=64)
    sem = torch.randn(1, 64, 2, 3, 4, device=DEV)
    binv = torch.randn(1, 2, 2, 3, 4, device=DEV)
    gt = torch.zeros((1, 8, 6, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.VeonHipError, match='status 1'):
        occ_labels(sem, binv, (4, 6, 8), gt, None, _hist(65))
    occ_labels(sem[:, :63], binv, (4, 6, 8), gt, None, _hist(64))
    occ_labels(sem, binv, (4, 6, 8))                           # labels alone: Q <= 254


def test_two_runs_are_identical():
    sem_d, bin_d, size, _ = _inputs('veon')
    gt, mask, n_cl = _truth('veon')
    runs = []
    for _ in range(2):
        h = _hist(n_cl)
        labels = occ_labels(_channels_last(sem_d), bin_d, size, gt, mask, h)
        runs.append((labels, h, confusion(labels, gt, mask, n_cl)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_metric_on_the_device_equals_the_cpu_metric():
    sem_d, bin_d, size, want = _inputs('q17')
    gt, mask, n_cl = _truth('q17')
    dev_m = OccMiouMetric(num_classes=n_cl, device=DEV)
    cpu_m = OccMiouMetric(num_classes=n_cl, device='cpu')
    for m in (dev_m, cpu_m):
        m.add_batch(want, gt.cpu().numpy(), None, mask.bool())
        m.add_batch(want.long().cpu(), gt.long(), None, mask)
    assert dev_m.hist.is_cuda and torch.equal(dev_m.hist.cpu(), cpu_m.hist)
    assert dev_m.miou() == cpu_m.miou() and dev_m.cnt == 2


# ---------------------------------------------------------------------- path and graph
def _tiny_path():
    from veon_amd.models.veon_occ import VeonOccupancyPath
    grid = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
            'depth': [1.0, 13.0, 1.0]}
    torch.manual_seed(0)
    net = VeonOccupancyPath(input_size=(64, 176), num_cam=2, clip_width=64, clip_layers=4,
                            clip_heads=1, clip_first_tail=2, clip_proj_dim=64, embed_dim=64,
                            n_classes=5, occ_size=(4, 20, 20), hsa_dim=64,
                            hsa_fusion_map=('0->1->1', '1->2->2'), grid_config=grid,
                            two_streams=False, clip_image=64).to(DEV).eval()
    bin_low = torch.randn(1, 2, 2, 10, 10, device=DEV)
    feat = torch.randn(1, 64, 2, 10, 10, device=DEV)
    return net, bin_low, feat


def test_path_tail_labels_only_uses_the_label_kernel():
    net, bin_low, feat = _tiny_path()
    with torch.no_grad():
        full = net._classify(bin_low, feat)
        before = dict(_lib.CALLS)
        only = net._classify(bin_low, feat, labels_only=True)
        after = dict(_lib.CALLS)
        feats = net._classify(bin_low, feat, return_features=True, labels_only=True)
    assert after.get('veon_occ_labels', 0) == before.get('veon_occ_labels', 0) + 1
    assert after.get('veon_occ_classify', 0) == before.get('veon_occ_classify', 0)
    assert set(only) == {'occ_pred_cls'} and set(feats) == {'occ_pred_cls', 'feat_low', 'bin_low'}
    assert only['occ_pred_cls'].dtype == torch.uint8
    assert torch.equal(only['occ_pred_cls'].long(), full['occ_pred_cls'])
    assert len(only['occ_pred_cls'].unique()) > 2


def test_tail_with_fused_histogram_in_a_graph():
    from veon_amd.graphs import GraphedCallable
    net, bin_low, feat = _tiny_path()
    m = OccMiouMetric(num_classes=6, device=DEV)
    g = torch.Generator().manual_seed(3)
    gt = torch.randint(0, 6, (1, 20, 20, 4), generator=g, dtype=torch.uint8).to(DEV)
    mask = (torch.rand((1, 20, 20, 4), generator=g) >= 0.3).to(torch.uint8).to(DEV)
    with torch.no_grad():
        labels = net._classify(bin_low, feat, labels_only=True,
                               count=(gt, mask, m.hist))['occ_pred_cls']
    single = m.hist.clone()
    assert torch.equal(single.cpu(), _bincount(labels, gt, mask, 6)) and int(single.sum()) > 0

    def tail(b, f):
        return net._classify(b, f, labels_only=True, count=(gt, mask, m.hist))['occ_pred_cls']
    graphed = GraphedCallable(tail, (bin_low, feat))     # (its warm-up calls count too)
    m.reset()
    for _ in range(3):
        out = graphed(bin_low, feat)
    assert torch.equal(out, labels)
    assert torch.equal(m.hist, 3 * single)


@torch.no_grad()
def test_evaluate_fuses_the_histogram_into_the_native_tail():
    """The whole tiny native path (tests/golden/path_tiny): evaluate() is one
    veon_occ_labels call (no veon_occ_classify, no veon_occ_confusion), returns the
    default forward's labels and adds their confusion matrix to the metric."""
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=True)
    images, geom, depth = _inputs(g, DEV)
    n_cl = net.ov_classifier_weight.shape[0] + 1
    full = net(images, geom, depth=depth)
    gen = torch.Generator().manual_seed(4)
    shape = full['occ_pred_cls'].shape
    gt = torch.randint(0, n_cl, shape, generator=gen)
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    mask = torch.rand(shape, generator=gen) >= 0.3
    m = OccMiouMetric(num_classes=n_cl, device=DEV)
    before = dict(_lib.CALLS)
    labels = net.evaluate(images, geom, gt.numpy(), mask.to(DEV), m, depth=depth)
    after = dict(_lib.CALLS)
    assert after.get('veon_occ_labels', 0) == before.get('veon_occ_labels', 0) + 1
    for other in ('veon_occ_classify', 'veon_occ_confusion'):
        assert after.get(other, 0) == before.get(other, 0), other
    assert labels.dtype == torch.uint8 and torch.equal(labels.long(), full['occ_pred_cls'])
    assert m.cnt == images.shape[0]
    want = _bincount(labels, gt.to(torch.uint8), mask, n_cl)
    assert torch.equal(m.hist.cpu(), want) and 0 < int(want.sum()) < labels.numel()
    only = net(images, geom, depth=depth, labels_only=True)
    assert set(only) == {'occ_pred_cls'} and torch.equal(only['occ_pred_cls'], labels)


def test_more_tiles_than_the_grid_bound():
    """Zo = 64 makes tiles of 16 x 1 columns: 130 * 17 = 2210 of them, more than the 2048
    blocks of the grid, so blocks stride over two tiles each and flush once."""
    B, Q, low, size = 1, 3, (7, 13, 26), (64, 130, 260)
    g = torch.Generator().manual_seed(21)
    sem = (torch.randn(B, Q, *low, generator=g) * 3).to(DEV)
    binv = torch.randn(B, 2, *low, generator=g).to(DEV)
    shape = (B, size[2], size[1], size[0])
    gt = torch.randint(0, Q + 1, shape, generator=g, dtype=torch.uint8)
    gt[torch.rand(shape, generator=g) < 0.1] = 255
    gt, mask = gt.to(DEV), (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8).to(DEV)
    want = conv3d_ops.occ_classify(sem, binv, size)[2].to(torch.uint8)
    h = _hist(Q + 1)
    for s in (sem, _channels_last(sem)):
        assert torch.equal(occ_labels(s, binv, size, gt, mask, h), want)
    assert torch.equal(h.cpu(), 2 * _bincount(want, gt, mask, Q + 1))


@torch.no_grad()
@pytest.mark.parametrize('device', [None, 'cuda', 'cuda:0'])
def test_metric_on_the_default_device_works_with_evaluate_and_add_batch(device):
    """``device=None`` and ``device='cuda'`` (no index) name the device the images are on:
    evaluate() accepts the metric, add_batch gives the same matrix."""
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=True)
    images, geom, depth = _inputs(g, DEV)
    n_cl = net.ov_classifier_weight.shape[0] + 1
    m = OccMiouMetric(num_classes=n_cl, device=device)
    assert m.device == m.hist.device == images.device and m.device.index == 0
    gen = torch.Generator().manual_seed(6)
    shape = (images.shape[0], net.occ_size[2], net.occ_size[1], net.occ_size[0])
    gt = torch.randint(0, n_cl, shape, generator=gen, dtype=torch.uint8)
    mask = torch.rand(shape, generator=gen) >= 0.3
    labels = net.evaluate(images, geom, gt, mask, m, depth=depth)
    want = _bincount(labels, gt, mask, n_cl)
    assert torch.equal(m.hist.cpu(), want) and int(want.sum()) > 0
    m.add_batch(labels, gt.numpy(), None, mask.to(DEV))
    assert torch.equal(m.hist.cpu(), 2 * want) and m.cnt == 2 * images.shape[0]
    m.count_miou()
