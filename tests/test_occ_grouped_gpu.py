"""The grouped tails (csrc/occ_tail.hip) on the MI355X.

Yardstick: the EXISTING ``conv3d_ops.occ_classify`` on all K rows, then torch's maximum
over each run of rows and the lowest channel that attains the maximum.  The kernels blend
every row with the same code (occ_interp.h, no FMA contraction), so labels are compared
exactly and merged logits as values (NaN where the yardstick has NaN)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from veon_amd import _lib, conv3d_ops
from veon_amd.occ_eval import confusion, occ_labels, occ_labels_grouped

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 2
# (z, y, x) of the head -> (Zo, Yo, Xo): x2 with Zo = 6; no multiple, Xo = 17 past the
# 16-column tile, Zo = 5 (both: 1-byte stores); Zo = 16 (16-byte stores)
GRIDS = {'x2': ((3, 5, 7), (6, 10, 14)), 'odd': ((2, 3, 5), (5, 7, 17)),
         'z16': ((4, 3, 5), (16, 6, 10))}


def _table(K, bg_first):
    """(group, n_merged): runs of seeded lengths and the background row, a run of its
    own, last; ``bg_first``: the background run feeds channel 0 (SemanticKITTI)."""
    if K == 1:
        return [0], 1
    rng = np.random.RandomState(K)
    group, ch = [], 0
    while len(group) < K - 1:
        group += [ch] * min(int(rng.randint(1, 6)), K - 1 - len(group))
        ch += 1
    group.append(ch)
    n = ch + 1
    if bg_first:
        group = [(g + 1) % n for g in group]
    return group, n


@functools.lru_cache(maxsize=None)
def _inputs(grid, K, bg_first):
    """Seeded low-resolution logits on the device, never written: rows c and c + 1 across
    the first run boundary identical (a tie of two merged channels), one NaN and one +inf
    corner value in different samples."""
    low, size = GRIDS[grid]
    group, n_merged = _table(K, bg_first)
    g = torch.Generator().manual_seed(100 * K + len(grid))
    sem = torch.randn(B, K, *low, generator=g) * 3
    binv = torch.randn(B, 2, *low, generator=g)
    if K > 1:
        c = next(i for i in range(K - 1) if group[i] != group[i + 1])
        sem[:, c + 1] = sem[:, c]
    sem[0, 3 % K, 0, 0, 0] = float('nan')
    sem[1, K - 1, -1, -1, -1] = float('inf')
    return sem.to(DEV), binv.to(DEV), size, group, n_merged


def _channels_last(x):
    """The same values as a channels-last view of padded 16-byte rows (VEC4); the surplus
    floats are NaN."""
    Bn, Q, z, y, xx = x.shape
    row = (Q + 3) // 4 * 4
    rows = torch.full((Bn, z, y, xx, row), float('nan'), device=x.device)
    rows[..., :Q] = x.permute(0, 2, 3, 4, 1)
    return rows[..., :Q].permute(0, 4, 1, 2, 3)


def _strided(x):
    """The same values as every second channel of an NCDHW volume (the scalar path)."""
    wide = torch.full((x.shape[0], 2 * x.shape[1]) + tuple(x.shape[2:]), float('nan'),
                      device=x.device)
    wide[:, ::2] = x
    view = wide[:, ::2]
    assert view.stride(1) == 2 * x.stride(1) and view.stride(4) == 1
    return view


LAYOUTS = {'vec4': _channels_last, 'scalar': _strided}


def _yardstick(sem, binv, size, group, n_merged, free_label):
    K = sem.shape[1]
    up, bin_up, cls = conv3d_ops.occ_classify(sem.contiguous(), binv, size)
    merged = [None] * n_merged
    left = 0
    while left < K:
        right = left
        while right + 1 < K and group[right + 1] == group[left]:
            right += 1
        merged[group[left]] = torch.max(up[:, left:right + 1], dim=1).values
        left = right + 1
    merged = torch.stack(merged, dim=1)
    top = merged.max(dim=1, keepdim=True).values
    index = torch.arange(n_merged, device=sem.device).view(1, -1, 1, 1, 1)
    first = torch.where(merged == top, index, torch.full_like(index, n_merged)).amin(dim=1)
    first = first.permute(0, 3, 2, 1)
    labels = torch.where(cls == K, torch.full_like(cls, free_label), first)
    return merged, bin_up, labels


def _same_values(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan])


CASES = [(grid, K, layout, bg_first) for grid in GRIDS for K in (1, 5, 61)
         for layout in LAYOUTS for bg_first in ((False, True) if K > 1 else (False,))]


@pytest.mark.parametrize('grid, K, layout, bg_first', CASES)
def test_labels_and_merged_logits_equal_the_ungrouped_tail(grid, K, layout, bg_first):
    sem, binv, size, group, n_merged = _inputs(grid, K, bg_first)
    free = n_merged - 1 if not bg_first else 0
    want_merged, want_bin, want = _yardstick(sem, binv, size, group, n_merged, free)
    view = LAYOUTS[layout](sem)
    before = dict(_lib.CALLS)
    merged, bin_up, cls = conv3d_ops.occ_classify_grouped(view, binv, size, group, n_merged,
                                                          free)
    labels = occ_labels_grouped(view, binv, size, group, n_merged, free)
    for name in ('veon_occ_classify_grouped', 'veon_occ_labels_grouped'):
        assert _lib.CALLS.get(name, 0) == before.get(name, 0) + 1
    assert cls.dtype == torch.int64 and labels.dtype == torch.uint8
    assert cls.shape == labels.shape == (B, size[2], size[1], size[0])
    assert torch.equal(cls, want) and torch.equal(labels.long(), want)
    assert torch.equal(bin_up, want_bin)
    assert merged.shape == (B, n_merged) + tuple(size) and _same_values(merged, want_merged)
    # the special values reached the outputs: NaN and +inf merged logits exist, their
    # voxels are free, and other voxels are kept
    assert bool(torch.isnan(merged).any()) and bool(torch.isposinf(merged).any())
    bad = (torch.isnan(merged).any(1) | torch.isposinf(merged).any(1)).permute(0, 3, 2, 1)
    assert bool((cls[bad] == free).all())
    kept = (want != free) if K > 1 and not bg_first else ~bad
    assert bool(kept.any())


@functools.lru_cache(maxsize=None)
def _identity_case(K, Zo):
    """Seeded logits on the (2, 3, 5) grid and what the UNGROUPED tails make of them at
    (Zo, 7, 10) (non-integer ratios in y and x), computed once and never written: one row
    NaN in a few voxels, one voxel all -inf; gt with 255s, a mask and their histogram."""
    size = (Zo, 7, 10)
    g = torch.Generator().manual_seed(1000 * K + Zo)
    sem = torch.randn(B, K, 2, 3, 5, generator=g) * 3
    binv = torch.randn(B, 2, 2, 3, 5, generator=g)
    for b, z, y, x in ((0, 0, 1, 2), (1, 1, 0, 0), (1, 0, 2, 4)):
        sem[b, 2, z, y, x] = float('nan')
    sem[0, :, 1, 2, 3] = float('-inf')
    shape = (B, size[2], size[1], size[0])
    gt = torch.randint(0, K + 1, shape, generator=g, dtype=torch.uint8)
    gt[torch.rand(shape, generator=g) < 0.1] = 255
    mask = (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8).to(DEV)
    sem, binv, gt = sem.to(DEV), binv.to(DEV), gt.to(DEV)
    rows, bin_up, cls = conv3d_ops.occ_classify(sem, binv, size)
    hist = torch.zeros((K + 1, K + 1), dtype=torch.int64, device=DEV)
    labels = occ_labels(sem, binv, size, gt, mask, hist)
    assert torch.equal(labels.long(), cls) and int(hist.sum()) > 0
    assert bool(torch.isnan(rows).any()) and bool(torch.isneginf(rows).all(1).any())
    assert bool((cls == K).any()) and bool((cls < K).any())
    return sem, binv, size, gt, mask, rows, bin_up, cls, labels, hist


@pytest.mark.parametrize('Zo', [16, 8, 4, 5])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('K', [5, 8])
def test_the_identity_table_gives_the_ungrouped_tails(K, layout, Zo):
    """group = range(K): every row is a run of its own, so both grouped kernels must give
    what ``occ_classify`` / ``occ_labels`` give, bit for bit (the merged logits are compared
    as bit patterns: NaN rows included) -- the four kernels share one voxel body.  K = 5
    and 8: a 16-byte step with and without surplus floats; Zo = 16, 8, 4, 5: the four widths
    of the tile writer."""
    sem, binv, size, gt, mask, rows, bin_up, cls, labels, hist = _identity_case(K, Zo)
    view = LAYOUTS[layout](sem)
    table = (list(range(K)), K, K)
    merged, got_bin, got_cls = conv3d_ops.occ_classify_grouped(view, binv, size, *table)
    assert torch.equal(got_cls, cls) and torch.equal(got_bin, bin_up)
    assert torch.equal(merged.view(torch.int32), rows.view(torch.int32))
    assert torch.equal(occ_labels_grouped(view, binv, size, *table), labels)
    got_hist = torch.zeros_like(hist)
    assert torch.equal(occ_labels_grouped(view, binv, size, *table, gt, mask, got_hist),
                       labels)
    assert torch.equal(got_hist, hist)


@pytest.mark.parametrize('group', [[0, 1], [1, 0], [2, 0, 0, 1]])
def test_a_tie_goes_to_the_lowest_merged_channel(group):
    """Identical rows in every group: all merged channels are equal everywhere, so every
    kept voxel is labelled 0, whichever run feeds channel 0."""
    g = torch.Generator().manual_seed(3)
    row = torch.randn(B, 1, 2, 3, 5, generator=g)
    sem = row.expand(B, len(group), 2, 3, 5).contiguous().to(DEV)
    binv = torch.randn(B, 2, 2, 3, 5, generator=g).to(DEV)
    n, free = max(group) + 1, 7
    for layout in LAYOUTS.values():
        merged, _, cls = conv3d_ops.occ_classify_grouped(layout(sem), binv, (5, 7, 17), group,
                                                         n, free)
        assert all(torch.equal(merged[:, 0], merged[:, c]) for c in range(n))
        assert set(cls.unique().tolist()) == {0, free}
        assert torch.equal(occ_labels_grouped(layout(sem), binv, (5, 7, 17), group, n,
                                              free).long(), cls)


def test_a_free_label_of_its_own():
    sem, binv, size, group, n_merged = _inputs('odd', 5, False)
    _, _, want = _yardstick(sem, binv, size, group, n_merged, 40)
    assert bool((want == 40).any()) and bool((want < n_merged).any())
    for layout in LAYOUTS.values():
        assert torch.equal(occ_labels_grouped(layout(sem), binv, size, group, n_merged,
                                              40).long(), want)
        assert torch.equal(conv3d_ops.occ_classify_grouped(layout(sem), binv, size, group,
                                                           n_merged, 40)[2], want)


@pytest.mark.parametrize('grid', sorted(GRIDS))
def test_fused_histogram_equals_confusion_of_the_labels(grid):
    """gt with 255s and a mask; n_cl = max(n_merged, free_label + 1); two calls add up."""
    sem, binv, size, group, n_merged = _inputs(grid, 61, False)
    for free in (n_merged - 1, 40):
        n_cl = max(n_merged, free + 1)
        shape = (B, size[2], size[1], size[0])
        g = torch.Generator().manual_seed(7)
        gt = torch.randint(0, n_cl, shape, generator=g, dtype=torch.uint8)
        gt[torch.rand(shape, generator=g) < 0.1] = 255
        mask = (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8).to(DEV)
        gt = gt.to(DEV)
        plain = occ_labels_grouped(sem, binv, size, group, n_merged, free)
        for m in (mask, None):
            hist = torch.zeros((n_cl, n_cl), dtype=torch.int64, device=DEV)
            want = confusion(plain, gt, m, n_cl)
            assert int(want.sum()) > 0 and int(want[:, free].sum()) > 0
            for layout in LAYOUTS.values():
                got = occ_labels_grouped(layout(sem), binv, size, group, n_merged, free, gt,
                                         m, hist)
                assert torch.equal(got, plain)
            assert torch.equal(hist, 2 * want)


def test_the_entry_points_refuse_what_the_header_excludes():
    sem, binv, size, group, n_merged = _inputs('x2', 5, False)
    args = (sem, _lib.strides(sem), 5)
    tail = (binv, _lib.strides(binv), B, 3, 5, 7, 6, 10, 14)
    out = torch.empty((B, 14, 10, 6), dtype=torch.uint8, device=DEV)
    for bad, n in (([0, 1, 0, 2, 2], 3), ([0, 0, 1, 1, 1], 3), ([0, 0, 1, 3, 3], 3)):
        with pytest.raises(_lib.VeonHipError):
            _lib.launch('veon_occ_labels_grouped', sem.device, *args,
                        _lib.host_array(bad, ctypes.c_uint8), n, n - 1, *tail,
                        out, None, None, None)
    with pytest.raises(ValueError):
        occ_labels_grouped(sem, binv, size, [0, 1, 0, 2, 2], 3, 2)


def test_graph_replay_equals_eager():
    from veon_amd.graphs import GraphedCallable
    sem, binv, size, group, n_merged = _inputs('odd', 61, True)
    view = _channels_last(sem)
    shape = (B, size[2], size[1], size[0])
    gt = (torch.arange(int(np.prod(shape)), device=DEV) % n_merged).to(torch.uint8).view(shape)
    hist = torch.zeros((n_merged, n_merged), dtype=torch.int64, device=DEV)

    def tails(s, b):
        merged, bin_up, cls = conv3d_ops.occ_classify_grouped(s, b, size, group, n_merged, 0)
        labels = occ_labels_grouped(s, b, size, group, n_merged, 0, gt, None, hist)
        return merged, bin_up, cls, labels

    eager = [t.clone() for t in tails(view, binv)]
    want_hist = hist.clone()
    graphed = GraphedCallable(tails, (view, binv), clone=False)
    hist.zero_()
    out = graphed.run()
    torch.cuda.synchronize()
    assert _same_values(out[0], eager[0])
    assert all(torch.equal(a, b) for a, b in zip(out[1:], eager[1:]))
    assert torch.equal(hist, want_hist) and int(hist.sum()) == gt.numel()
