"""The F-score kernel (csrc/occ_fscore.hip) against the torch mirror on the CPU, which
tests/test_occ_fscore.py holds to the reference's recorded results and to a float64 brute
force.  Everything is an integer count, so everything is compared exactly."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.test_occ_fscore import MODES, check_against_fixture, config_kw, fill
from veon_amd import _lib
from veon_amd.occ_eval import (DEFAULT_REACH, OccFScoreMetric, OccMiouMetric,
                               fscore_counts, fscore_reach)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VOID, FREE = (17, 255), 17
R2, R3 = fscore_reach(0.9), fscore_reach(1.3)
# every voxel of the own column, most of the four neighbours': the spread past the word
TALL = (1, np.array([[-1, 40, -1], [40, 63, 40], [-1, 40, -1]], np.int32))
TABLES = {'default': (DEFAULT_REACH, DEFAULT_REACH), 'r2': (R2, fscore_reach(0.45)),
          'r3': (R3, R2), 'tall': (TALL, DEFAULT_REACH)}
assert (DEFAULT_REACH[0], R2[0], R3[0]) == (1, 2, 3)


def volume(shape, seed, density=0.1):
    """Seeded (pred, gt, mask) uint8 on the CPU: mostly free, ~5 % of the ground truth
    255, ~30 % of the mask 0."""
    g = torch.Generator().manual_seed(seed)
    def labels():
        lab = torch.randint(0, 17, shape, generator=g, dtype=torch.uint8)
        lab[torch.rand(shape, generator=g) >= density] = FREE
        return lab
    pred, gt = labels(), labels()
    gt[torch.rand(shape, generator=g) < 0.05] = 255
    mask = (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8)
    return pred, gt, mask


def agree(pred, gt, mask, tables=TABLES['default'], void=VOID):
    """Kernel counts == mirror counts; -> the counts."""
    kw = dict(void=void, reach_acc=tables[0], reach_cmpl=tables[1])
    want = fscore_counts(pred, gt, mask, **kw)
    before = _lib.CALLS.get('veon_occ_fscore_counts', 0)
    got = fscore_counts(pred.to(DEV), gt.to(DEV), None if mask is None else mask.to(DEV), **kw)
    assert _lib.CALLS.get('veon_occ_fscore_counts', 0) == before + 1
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), (tuple(pred.shape), got.cpu().tolist(), want.tolist())
    return want


# ------------------------------------------------------------------------------- seams
@pytest.mark.parametrize('X', [1, 15, 16, 17, 33])
def test_tile_and_sample_seams(X):
    """Voxels at the last column of sample b and the first of b + 1, at y = Y - 1 of one x
    row and y = 0 of the next: neighbours in memory, not in the grid.  A halo that leaks
    across a sample or wraps with the flat index changes a count."""
    Z = 5
    for Y, B in itertools.product([1, 15, 16, 17, 33], [1, 3]):
        pred = torch.full((B, X, Y, Z), FREE, dtype=torch.uint8)
        gt = pred.clone()
        pred[:, X - 1, Y - 1, :] = 1        # the last column of every sample ...
        gt[:, 0, 0, :] = 2                  # ... and the first
        for x in range(4, X - 5, 2):        # (clear of the two corner columns)
            gt[:, x, Y - 1, 1] = 3          # the end of an x row ...
            pred[:, x + 1, 0, 1] = 4        # ... and the start of the next
        for name in ('default', 'r3'):
            planted = agree(pred, gt, None, TABLES[name])
            if X == 33 and Y == 33:         # nothing planted is near anything
                assert planted[:, 2:].tolist() == [[0, 0]] * B, name
                assert int(planted[0, 0]) == Z + 12 and int(planted[0, 1]) == Z + 12
        noise = volume((B, X, Y, Z), 100 * X + Y)
        both = (torch.where(pred != FREE, pred, noise[0]), torch.where(gt != FREE, gt, noise[1]))
        for name in ('default', 'r2', 'r3'):
            agree(both[0], both[1], noise[2], TABLES[name])
            agree(both[0], both[1], None, TABLES[name])


@pytest.mark.parametrize('Z', [1, 7, 16, 17, 32, 63, 64])
def test_z_seams(Z):
    """Voxels at z = 0 and z = Z - 1: the spread past both ends of the word, and the
    64-bit word itself at Z = 64."""
    shape = (2, 18, 17, Z)
    pred, gt, mask = volume(shape, Z, density=0.05)
    pred[:, 3, 4, 0], gt[:, 3, 5, Z - 1] = 1, 1
    pred[:, 9, 9, Z - 1], gt[:, 10, 9, 0] = 1, 1
    pred[1, 17, 16, Z - 1], gt[0, 0, 0, 0] = 1, 1
    mask[:, 3, 4:6], mask[:, 9:11, 9] = 1, 1
    for name in TABLES:
        c = agree(pred, gt, mask, TABLES[name])
        assert int(c[:, 0].min()) > 0 and int(c[:, 1].min()) > 0
        agree(pred, gt, None, TABLES[name])
    # two isolated voxels a whole column apart: near only under the tall table
    pred, gt = torch.full(shape, FREE, dtype=torch.uint8), torch.full(shape, FREE, dtype=torch.uint8)
    pred[:, 5, 5, 0], gt[:, 5, 5, Z - 1] = 1, 1
    assert agree(pred, gt, None, TABLES['tall']).tolist() == [[1, 1, 1, int(Z <= 2)]] * 2
    if Z > 4:
        assert agree(pred, gt, None, TABLES['r3']).tolist() == [[1, 1, 0, 0]] * 2


@pytest.mark.parametrize('name', ['default', 'r2', 'r3'])
def test_every_offset(name):
    """One predicted and one ground-truth voxel per sample, one sample per integer offset
    with |d| <= 3 on every axis (across the tile seam at 16): the hit is what the table
    says."""
    acc, cmpl = TABLES[name]
    offsets = list(itertools.product(range(-3, 4), repeat=3))
    shape = (len(offsets), 20, 20, 8)
    pred, gt = torch.full(shape, FREE, dtype=torch.uint8), torch.full(shape, FREE, dtype=torch.uint8)

    def near(reach, dx, dy, dz):
        R, table = reach
        return int(abs(dx) <= R and abs(dy) <= R and abs(dz) <= table[dx + R, dy + R])
    want = []
    for b, (dx, dy, dz) in enumerate(offsets):
        pred[b, 15, 15, 3] = 0
        gt[b, 15 + dx, 15 + dy, 3 + dz] = 0
        want.append([1, 1, near(acc, dx, dy, dz), near(cmpl, -dx, -dy, -dz)])
    assert agree(pred, gt, None, (acc, cmpl)).tolist() == want
    hits = sum(w[2] for w in want)
    assert hits == {'default': 19, 'r2': 57, 'r3': 147}[name]      # |d|^2 <= 2, 5, 10


def test_extremes():
    for shape in [(2, 17, 19, 16), (1, 5, 6, 64), (1, 1, 1, 1)]:
        n = shape[1] * shape[2] * shape[3]
        full = torch.zeros(shape, dtype=torch.uint8)
        free = torch.full(shape, FREE, dtype=torch.uint8)
        ones, zeros = torch.ones(shape, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8)
        for name in ('default', 'r3', 'tall'):
            t = TABLES[name]
            assert agree(full, full, None, t).tolist() == [[n, n, n, n]] * shape[0]
            assert agree(full, full, ones, t).tolist() == [[n, n, n, n]] * shape[0]
            assert agree(free, free, None, t).tolist() == [[0, 0, 0, 0]] * shape[0]
            assert agree(full, free, None, t).tolist() == [[n, 0, 0, 0]] * shape[0]
            assert agree(free, torch.full(shape, 255, dtype=torch.uint8), None, t).tolist() \
                == [[0, 0, 0, 0]] * shape[0]
            assert agree(full, full, zeros, t).tolist() == [[0, 0, 0, 0]] * shape[0]
    # another void set: 0 is void, 17 and 255 are not
    pred, gt, mask = volume((2, 9, 20, 16), 5)
    c = agree(pred, gt, mask, void=(0,))
    assert int(c[:, 0].min()) > int(0.5 * mask[0].sum())


# -------------------------------------------------------------------------- load paths
def _off_by_one(t):
    """The same values one byte off every alignment, on the device."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 4 == 1 and buf.is_contiguous()
    return buf


@pytest.mark.parametrize('Z', [5, 8, 12, 16, 24, 48])
def test_load_paths(Z):
    """Z = 16 and 48: 16-byte loads; 8 and 24: 8 bytes; 12: 4 bytes; 5: bytes -- and bytes
    again for tensors one byte off alignment.  uint8 and int64 predictions."""
    shape = (2, 19, 21, Z)
    pred, gt, mask = volume(shape, 300 + Z)
    want = agree(pred, gt, mask, TABLES['r2'])
    assert torch.equal(agree(pred.long(), gt, mask, TABLES['r2']), want)
    kw = dict(reach_acc=TABLES['r2'][0], reach_cmpl=TABLES['r2'][1])
    d = [t.to(DEV) for t in (pred, gt, mask)]
    assert all(t.data_ptr() % 16 == 0 for t in d)
    for k in range(3):                       # each tensor alone off alignment, then all
        args = list(d)
        args[k] = _off_by_one(d[k])
        assert torch.equal(fscore_counts(*args, **kw).cpu(), want), k
    off = [_off_by_one(t) for t in d]
    assert torch.equal(fscore_counts(*off, **kw).cpu(), want)
    assert torch.equal(fscore_counts(d[0].long(), off[1], off[2], **kw).cpu(), want)
    assert torch.equal(fscore_counts(off[0], off[1], None, **kw).cpu(),
                       fscore_counts(pred, gt, None, **kw))
    # int64 labels outside a byte are occupied, whatever their low byte says
    wide = pred.long()
    occupied = wide != FREE
    wide[occupied] = torch.tensor([-1, 300, 256 + 17, 1 << 40, -(1 << 40) + 255, 3])[
        torch.arange(int(occupied.sum())) % 6]
    assert torch.equal(agree(wide, gt, mask, TABLES['r2']), want)


def test_more_tiles_than_the_grid_bound():
    """47 x 47 tiles of one sample, 2209 > the 2048 blocks of the grid: blocks take a
    second tile.  And the same with three samples, where the second tile of a block
    belongs to another sample."""
    pred, gt, mask = volume((1, 737, 739, 3), 77, density=0.05)
    c = agree(pred, gt, mask)
    assert 0 < int(c[0, 2]) < int(c[0, 0])
    pred, gt, mask = volume((3, 430, 420, 2), 78, density=0.05)      # 3 * 27 * 27 = 2187
    c = agree(pred, gt, mask, TABLES['r2'])
    assert len({tuple(r) for r in c.tolist()}) == 3


def test_out_accumulates_and_two_runs_are_identical():
    pred, gt, mask = (t.to(DEV) for t in volume((3, 33, 35, 16), 9))
    once = fscore_counts(pred, gt, mask)
    assert torch.equal(fscore_counts(pred, gt, mask), once)
    marked = torch.arange(12, device=DEV).view(3, 4)
    out = marked.clone()
    assert fscore_counts(pred, gt, mask, out=out) is out
    assert torch.equal(out, marked + once)
    fscore_counts(pred, gt, mask, out=out)
    assert torch.equal(out, marked + 2 * once)
    # a view of a larger buffer, as the metric passes it; one sample as (X, Y, Z)
    buf = torch.zeros((8, 4), dtype=torch.int64, device=DEV)
    fscore_counts(pred, gt, mask, out=buf[2:5])
    assert torch.equal(buf[2:5], once) and int(buf[:2].abs().sum() + buf[5:].abs().sum()) == 0
    assert torch.equal(fscore_counts(pred[1], gt[1], mask[1]), once[1:2])
    # the inputs are never written
    want = volume((3, 33, 35, 16), 9)
    for got, kept in zip((pred, gt, mask), want):
        assert torch.equal(got.cpu(), kept)


def test_bad_arguments_are_refused():
    pred = torch.zeros((1, 4, 4, 65), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.VeonHipError, match='Z'):
        fscore_counts(pred, pred)
    ok = torch.zeros((1, 4, 4, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='R must be'):
        fscore_counts(ok, ok, reach_acc=(4, np.zeros((9, 9), np.int32)))
    with pytest.raises(ValueError, match='reaches'):
        fscore_counts(ok, ok, reach_cmpl=(0, np.array([[64]], np.int32)))
    with pytest.raises(_lib.VeonHipError, match='device'):
        fscore_counts(ok, ok.cpu())


def test_graph_replay():
    """``fscore_counts(..., out=)`` in one captured graph on one stream: the replay
    equals eager and follows in-place changes of its inputs (the tables and the void
    words travel in the launch itself)."""
    shape = (2, 20, 17, 16)
    first, second = volume(shape, 31), volume(shape, 32)
    pred, gt, mask = (t.to(DEV) for t in first)
    kw = dict(reach_acc=TABLES['r2'][0], reach_cmpl=TABLES['r2'][1])
    out = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    fscore_counts(pred, gt, mask, out=out, **kw)          # eager, also the warm-up
    eager = out.clone()
    assert torch.equal(eager.cpu(), fscore_counts(*first, **kw))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fscore_counts(pred, gt, mask, out=out, **kw)
    out.zero_()
    graph.replay()
    assert torch.equal(out, eager)
    graph.replay()
    assert torch.equal(out, 2 * eager)                    # it adds, replay after replay
    for t, new in zip((pred, gt, mask), second):
        t.copy_(new)
    out.zero_()
    graph.replay()
    want = fscore_counts(*second, **kw)
    assert torch.equal(out.cpu(), want) and not torch.equal(want, eager.cpu())


# ------------------------------------------------------------------------------ metric
@functools.lru_cache(maxsize=None)
def _gold():
    from tests.test_occ_fscore import GOLDEN
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('device', [None, 'cuda', 'cuda:0'])
def test_metric_on_the_device_equals_the_cpu_metric_and_the_fixture(device):
    gold = _gold()
    for cfg, mode in itertools.product(sorted(gold['configs']), sorted(MODES)):
        def metric_of(n, device=device):
            m = OccFScoreMetric(device=device, **config_kw(gold, cfg), **MODES[mode])
            return fill(m, gold, samples=range(n))
        dev_m, cpu_m = metric_of(4), metric_of(4, 'cpu')
        assert dev_m.device == dev_m.counts.device == torch.device(DEV)
        assert np.array_equal(dev_m.sample_counts(), cpu_m.sample_counts())
        assert dev_m.count_fscore() == cpu_m.count_fscore()
        if device == 'cuda:0':
            check_against_fixture(metric_of, gold, cfg, mode)
    # tensors on the device, batches, int64 predictions; more samples than the buffer holds
    m = OccFScoreMetric(device=device, use_image_mask=True)
    before = _lib.CALLS.get('veon_occ_fscore_counts', 0)
    for _ in range(5):
        m.add_batch(torch.from_numpy(gold['pred']).to(DEV).long(), gold['gt'], None,
                    torch.from_numpy(gold['mask_camera']).to(DEV))
    assert _lib.CALLS.get('veon_occ_fscore_counts', 0) == before + 5
    assert m.cnt == 20
    assert np.array_equal(m.sample_counts(), np.tile(gold['default_image_counts'], (5, 1)))
    m.reset()
    assert m.cnt == 0 and m.sample_counts().shape == (0, 4)


@torch.no_grad()
def test_evaluate_with_both_metrics_on_the_native_path():
    """The whole tiny native path (tests/golden/path_tiny): with a list of both metrics
    evaluate() returns the same labels, leaves the mIoU metric's ``hist`` and ``cnt`` as
    a run with that metric alone leaves them -- still one veon_occ_labels call with the
    histogram fused, no veon_occ_confusion -- and gives the F-score metric the counts of
    ``add_batch`` on the returned labels."""
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=True)
    images, geom, depth = _inputs(g, DEV)
    n_cl = net.ov_classifier_weight.shape[0] + 1
    void = (n_cl - 1, 255)
    gen = torch.Generator().manual_seed(4)
    shape = (images.shape[0], net.occ_size[2], net.occ_size[1], net.occ_size[0])
    gt = torch.randint(0, n_cl, shape, generator=gen)
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    mask = torch.rand(shape, generator=gen) >= 0.3
    net.evaluate(images, geom, gt, mask, OccMiouMetric(num_classes=n_cl, device=DEV),
                 depth=depth)      # (whatever the path prepares once is prepared now)
    alone = OccMiouMetric(num_classes=n_cl, device=DEV)
    before = dict(_lib.CALLS)
    want = net.evaluate(images, geom, gt.numpy(), mask.to(DEV), alone, depth=depth)
    single = {k: v - before.get(k, 0) for k, v in _lib.CALLS.items() if v != before.get(k, 0)}
    assert single['veon_occ_labels'] == 1 and 'veon_occ_fscore_counts' not in single
    miou = OccMiouMetric(num_classes=n_cl, device=DEV)
    f_mask = OccFScoreMetric(void=void, use_image_mask=True, device=DEV)
    f_all = OccFScoreMetric(void=void, device=DEV)
    before = dict(_lib.CALLS)
    labels = net.evaluate(images, geom, gt.numpy(), mask.to(DEV), [miou, f_mask, f_all],
                          depth=depth)
    listed = {k: v - before.get(k, 0) for k, v in _lib.CALLS.items() if v != before.get(k, 0)}
    assert listed == dict(single, veon_occ_fscore_counts=2)      # the same calls, and two
    assert labels.dtype == torch.uint8 and torch.equal(labels, want)
    assert torch.equal(miou.hist, alone.hist) and miou.cnt == alone.cnt == shape[0]
    assert int(miou.hist.sum()) > 0
    for m, mk in ((f_mask, mask), (f_all, None)):
        by_hand = OccFScoreMetric(void=void, use_image_mask=mk is not None, device=DEV)
        by_hand.add_batch(labels, gt, None, mk)
        assert m.cnt == by_hand.cnt == shape[0]
        assert np.array_equal(m.sample_counts(), by_hand.sample_counts())
        cpu = fscore_counts(labels.cpu(), miou.labels_u8(gt).cpu(),
                            None if mk is None else mk.to(torch.uint8), void)
        assert np.array_equal(m.sample_counts(), cpu.numpy())
    assert int(f_all.sample_counts()[:, 0].min()) > 0
    # an F-score metric alone; a tuple
    only = OccFScoreMetric(void=void, device=DEV)
    assert torch.equal(net.evaluate(images, geom, gt, None, only, depth=depth), want)
    assert np.array_equal(only.sample_counts(), f_all.sample_counts())
    assert torch.equal(net.evaluate(images, geom, gt, mask, (only,), depth=depth), want)
    assert only.cnt == 2 * shape[0]
    with pytest.raises(ValueError, match='lives on'):
        net.evaluate(images, geom, gt, mask, [miou, OccFScoreMetric(void=void, device='cpu')],
                     depth=depth)
    assert torch.equal(miou.hist, alone.hist)          # refused before anything was counted
