"""``build_vocabulary`` against the triples the reference's own
``_add_vocabulary_nuscenes`` lines returned (tools/gen_golden_open_vocab.py)."""
import json
import os

import torch

from tests.conftest import GOLD
from veon_amd.vocabulary import build_vocabulary, group_ids, lowest_argmax, merge_runs


def _doc():
    with open(os.path.join(GOLD, 'open_vocab_tiny.json')) as f:
        return json.load(f)


def test_equals_the_recorded_reference_triples():
    doc = _doc()
    assert len(doc['cases']) == 2 and len(doc['templates']) == 14
    for case in doc['cases']:
        voc, detailed, reflection = build_vocabulary(case['words'], doc['categories'])
        assert voc == case['vocabulary']
        assert detailed == case['detailed_description']
        assert reflection == case['class_reflection']
        assert len(voc) == len(detailed) == len(reflection)


def test_group_ids_has_seventeen_runs():
    doc = _doc()
    voc, _, reflection = build_vocabulary([], doc['categories'])
    gid, runs = group_ids(reflection)
    assert runs == 17 == len(doc['categories']) and gid == reflection and len(voc) == 66
    # three words of the user's in front: three classes more, 'car' no longer in its category
    voc, _, reflection = build_vocabulary(doc['cases'][1]['words'], doc['categories'])
    assert group_ids(reflection)[1] == 20 and voc[:3] == ['traffic light', 'car', 'zebra crossing']
    assert voc.count('car') == 1


def test_user_words_are_deduplicated_in_order():
    voc, detailed, reflection = build_vocabulary(
        [' B ', 'a', 'b', '', 'A', 'c'], [{'category': 'x', 'detailed_items': [['a'], ['d', 'long d']]}])
    assert voc == ['b', 'a', 'c', 'd'] and reflection == [0, 1, 2, 3]
    assert detailed == ['b', 'a', 'c', "d, in detail 'long d'"]


def test_merge_runs_and_lowest_argmax_on_a_hand_written_table():
    """Three runs over five rows at four positions: a plain one, a tie of channels 1 and 2
    (the lower wins), a NaN in run 0 (it sticks; no channel attains a NaN maximum: n) and
    -inf rows."""
    nan, inf = float('nan'), float('inf')
    group = [0, 0, 1, 2, 2]
    rows = torch.tensor([[[1., 0., nan, -inf],
                          [3., 1., 7., -inf],
                          [2., 4., 1., -1.],
                          [0., 4., 2., -2.],
                          [-1., 2., 3., -inf]]])
    merged = merge_runs(rows, group, 3)
    want = torch.tensor([[[3., 1., nan, -inf],
                          [2., 4., 1., -1.],
                          [0., 4., 3., -2.]]])
    torch.testing.assert_close(merged, want, rtol=0, atol=0, equal_nan=True)
    cls, top = lowest_argmax(merged)
    assert cls.tolist() == [[0, 1, 3, 1]] and cls.dtype == torch.int64
    torch.testing.assert_close(top, torch.tensor([[[3., 4., nan, -1.]]]), rtol=0, atol=0,
                               equal_nan=True)
    # trailing dims of any number: the same table as a (1, 5, 2, 2) volume
    cls4, _ = lowest_argmax(merge_runs(rows.view(1, 5, 2, 2), group, 3))
    assert cls4.tolist() == [[[0, 1], [3, 1]]]


def test_group_ids_numbers_runs_in_order_of_appearance():
    assert group_ids([3, 3, 7, 3]) == ([0, 0, 1, 2], 3)
    assert group_ids([]) == ([], 0)
