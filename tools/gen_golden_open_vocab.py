#!/usr/bin/env python
"""Fixtures of the open-vocabulary path: tests/golden/open_vocab_tiny.npz + .json.

    python tools/gen_golden_open_vocab.py        (CPU; needs the reference tree)

Nothing of the reference is imported as a module (its entry module pulls in detectron2):
the two methods ``_add_vocabulary_nuscenes`` and ``_merge_classes_prob`` of
mmdet3d/models/semantic_net/san_in_veon_entry_temporal.py and the label lines of
``VeonTemporal.simple_test`` (mmdet3d/models/detectors/veon_temporal.py:220-229) are lifted
from the files with ``ast`` at generation time, unmodified, and run on a stand-in ``self``.
Data only:

open_vocab_tiny.json
    categories   the reference's nuScenes-brief list (vocabulary/nuscenes_vol.py) as
                 [{"category", "detailed_items": [[brief] | [brief, detail], ...]}]
    templates    its "vild" template list (clip_utils/utils.py)
    cases        for two lists of user words: the words, and the (vocabulary,
                 detailed_description, class_reflection) its lines return for them (the
                 words prepared as prepare_vocabulary :94-98 does, but de-duplicated in
                 order: ``list(set(...))`` has no order to record)
open_vocab_tiny.npz   one tail case
    sem_low (1, 9, 2, 3, 4), bin_low (1, 2, 2, 3, 4) fp32; class_reflection (8,);
    size (3,) = (4, 6, 8); merged (1, 5, 4, 6, 8): _merge_classes_prob of the trilinearly
    upsampled rows; labels (1, 8, 6, 4) int64: the simple_test lines on it (free = 17 is
    replaced by ``free_label`` = 4, the background channel of THIS case, after the fact)"""
import ast
import json
import os
import runpy
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('VEON_REFERENCE', '/root/reference')
SEM = os.path.join(REF, 'mmdet3d', 'models', 'semantic_net')
OUT = os.path.join(ROOT, 'tests', 'golden', 'open_vocab_tiny')
WORD_LISTS = [[], ['Traffic Light ', 'car', '', 'traffic light', 'zebra crossing']]


def lift_methods(path, cls, names, namespace):
    """The named methods of class ``cls`` in ``path``, compiled from their own AST."""
    with open(path) as f:
        tree = ast.parse(f.read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    defs = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(defs) == len(names)
    for d in defs:
        d.returns = None      # (annotations name typing symbols that are not needed)
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, 'exec'), namespace)
    return [namespace[n] for n in names]


def lift_lines(path, cls, method, first, last):
    """The statements of ``cls.method`` on lines [first, last], compiled as a block."""
    with open(path) as f:
        tree = ast.parse(f.read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == method)
    stmts = [s for s in fn.body if first <= s.lineno and s.end_lineno <= last]
    assert stmts and stmts[0].lineno == first and stmts[-1].end_lineno == last
    return compile(ast.Module(body=stmts, type_ignores=[]), path, 'exec')


def main():
    voc = runpy.run_path(os.path.join(SEM, 'vocabulary', 'nuscenes_vol.py'))
    kitti = runpy.run_path(os.path.join(SEM, 'vocabulary', 'semkitti_vol.py'))
    with open(os.path.join(SEM, 'clip_utils', 'utils.py')) as f:
        utils = ast.parse(f.read())
    templates = next(ast.literal_eval(n.value) for n in utils.body
                     if isinstance(n, ast.Assign) and n.targets[0].id == 'PREDEFINED_TEMPLATES')
    ns = dict(List=list, torch=torch, NUSCENES_CLASSES=voc['NUSCENES_CLASSES'],
              NUSCENES_CLASSES_BRIEF=voc['NUSCENES_CLASSES_BRIEF'],
              SEMKITTI_CLASSES_BRIEF=kitti['SEMKITTI_CLASSES_BRIEF'])
    add_voc, merge = lift_methods(os.path.join(SEM, 'san_in_veon_entry_temporal.py'),
                                  'SANInVeonEntryTemporal',
                                  ['_add_vocabulary_nuscenes', '_merge_classes_prob'], ns)
    cases = []
    for words in WORD_LISTS:
        prepared = list(dict.fromkeys(w.lower().strip() for w in words))
        prepared = [w for w in prepared if w != '']
        v, d, r = add_voc(None, list(prepared), list(prepared),
                          list(range(len(prepared))), 'nuscenes_brief')
        cases.append(dict(words=words, vocabulary=v, detailed_description=d,
                          class_reflection=r))
    doc = dict(categories=[dict(category=c['category'],
                                detailed_items=[list(i) for i in c['detailed_items']])
                           for c in voc['NUSCENES_CLASSES_BRIEF']],
               templates=templates['vild'], cases=cases)
    with open(OUT + '.json', 'w') as f:
        json.dump(doc, f, indent=1)

    torch.manual_seed(24)
    reflection = [0, 0, 1, 2, 2, 2, 3, 3]
    size = (4, 6, 8)
    sem_low = torch.randn(1, len(reflection) + 1, 2, 3, 4)
    sem_low[0, 1] = sem_low[0, 2]          # equal rows in two groups: a tie of channels
    bin_low = torch.randn(1, 2, 2, 3, 4)
    up = F.interpolate(sem_low, size=size, mode='trilinear', align_corners=False)
    this = types.SimpleNamespace(class_reflection=reflection, mode='nuscenes')
    merged, _ = merge(this, up, 1, torch.zeros(len(reflection) + 1, 1))
    block = lift_lines(os.path.join(REF, 'mmdet3d', 'models', 'detectors', 'veon_temporal.py'),
                       'VeonTemporal', 'simple_test', 220, 229)
    env = dict(torch=torch, self=this, semantic_results=dict(
        sem_occ=merged, bin_occ=F.interpolate(bin_low, size=size, mode='trilinear',
                                              align_corners=False)))
    exec(block, env)
    labels = env['occ_pred_cls']
    free = merged.shape[1] - 1
    sel = env['sel_tag'].permute(0, 3, 2, 1)
    assert bool((labels[~sel] == 17).all()) and int(labels[sel].max()) <= free
    labels = torch.where(sel, labels, torch.full_like(labels, free))
    np.savez(OUT + '.npz', sem_low=sem_low.numpy(), bin_low=bin_low.numpy(),
             class_reflection=np.array(reflection), size=np.array(size),
             merged=merged.numpy(), labels=labels.numpy())
    print('wrote', OUT + '.json', OUT + '.npz', 'K2 =', len(cases[0]['vocabulary']))


if __name__ == '__main__':
    sys.exit(main())
