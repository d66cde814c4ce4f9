"""``build_vocabulary`` against the triples the reference's own
``_add_vocabulary_nuscenes`` lines returned (tools/gen_golden_open_vocab.py)."""
import json
import os

from tests.conftest import GOLD
from veon_amd.align_select import group_ids
from veon_amd.vocabulary import build_vocabulary


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
