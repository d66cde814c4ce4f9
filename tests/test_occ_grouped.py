"""The grouped tail's torch mirror (also its CPU path) against the reference's own
``_merge_classes_prob`` + ``simple_test`` lines (tools/gen_golden_open_vocab.py), and the
host checks of the group table."""
import pytest
import torch

from tests.conftest import load_golden
from veon_amd import conv3d_ops
from veon_amd.align_select import group_ids
from veon_amd.occ_eval import (confusion, group_table, occ_grouped_reference,
                               occ_labels_grouped)


def _case():
    g = load_golden('open_vocab_tiny')
    gid, runs = group_ids(g['class_reflection'])
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    return t, tuple(int(v) for v in g['size']), gid + [runs], runs + 1, runs


def test_mirror_equals_the_recorded_reference():
    t, size, group, n_merged, free = _case()
    merged, bin_up, labels = occ_grouped_reference(t['sem_low'], t['bin_low'], size, group,
                                                   n_merged, free)
    assert torch.equal(merged, t['merged']) and torch.equal(labels, t['labels'])
    assert bin_up.shape == (1, 2) + size
    # the recorded case holds a tie of two channels (decided for the lower one), free
    # voxels and every other label
    assert set(labels.unique().tolist()) == {0, 2, 3, 4}
    # the wrappers on the CPU are the mirror
    m2, b2, l2 = conv3d_ops.occ_classify_grouped(t['sem_low'], t['bin_low'], size, group,
                                                 n_merged, free)
    assert torch.equal(m2, merged) and torch.equal(b2, bin_up) and torch.equal(l2, labels)
    gt = (labels % 3).to(torch.uint8)
    hist = torch.zeros((n_merged, n_merged), dtype=torch.int64)
    l8 = occ_labels_grouped(t['sem_low'], t['bin_low'], size, group, n_merged, free, gt,
                            None, hist)
    assert l8.dtype == torch.uint8 and torch.equal(l8.long(), labels)
    assert torch.equal(hist, confusion(l8, gt, None, n_merged))


def test_background_first_and_another_free_label():
    t, size, group, n_merged, free = _case()
    moved = [(g + 1) % n_merged for g in group]      # background -> channel 0
    merged, _, labels = occ_grouped_reference(t['sem_low'], t['bin_low'], size, moved,
                                              n_merged, 9)
    assert torch.equal(merged[:, 1:], t['merged'][:, :-1])
    assert torch.equal(merged[:, 0], t['merged'][:, -1])
    kept = labels != 9
    assert bool(kept.any()) and bool((~kept).any())
    first = torch.where(merged == merged.max(1, keepdim=True).values,
                        torch.arange(n_merged).view(1, -1, 1, 1, 1), n_merged).amin(1)
    assert torch.equal(labels[kept], first.permute(0, 3, 2, 1)[kept])


@pytest.mark.parametrize('group, n_merged, free', [
    ([0, 1, 0], 2, 2),                    # a split run
    ([0, 0, 1, 1, 0], 2, 2),              # the same, longer
    ([0, 1, 2, 1], 3, 3),                 # a channel used twice
    ([0] * 257, 1, 1),                    # K > 256
    (list(range(65)), 65, 65),            # n_merged > 64
    ([0, 1], 3, 3),                       # a channel without rows
    ([0, 2], 2, 2),                       # a channel out of range
    ([0, 1], 2, 256),                     # a label that is no byte
])
def test_bad_group_tables_raise_value_error(group, n_merged, free):
    with pytest.raises(ValueError):
        group_table(group, n_merged, free)
    K = len(group)
    sem, binv = torch.zeros(1, K, 1, 1, 1), torch.zeros(1, 2, 1, 1, 1)
    with pytest.raises(ValueError):
        occ_labels_grouped(sem, binv, (2, 2, 2), group, n_merged, free)
    with pytest.raises(ValueError):
        conv3d_ops.occ_classify_grouped(sem, binv, (2, 2, 2), group, n_merged, free)


def test_table_limits_are_inclusive():
    assert len(group_table([0] * 256, 1, 0)) == 256
    assert group_table(list(range(64)), 64, 63, with_hist=True) == list(range(64))
    with pytest.raises(ValueError):       # the histogram's side is max(n_merged, free + 1)
        group_table([0, 1], 2, 64, with_hist=True)
    assert group_table([0, 1], 2, 64) == [0, 1]
    with pytest.raises(ValueError):       # one entry per logit row
        group_table([0, 1], 2, 2, K=3)
