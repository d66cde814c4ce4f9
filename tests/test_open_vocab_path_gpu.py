"""``VeonOccupancyPath.set_vocabulary`` on the tiny native path of the path tests: the
grouped tails, evaluation and prompt retrieval; and a path without it unchanged."""
import functools

import pytest
import torch

from tests import clip_text_refs as refs
from tests.conftest import load_golden
from tests.test_path_golden import _build, _inputs
from veon_amd import _lib, conv3d_ops
from veon_amd.models.semantic_net import classifier_logits_low
from veon_amd.models.semantic_net.clip_text import OvClassifier
from veon_amd.occ_eval import OccMiouMetric, confusion, occ_grouped_reference
from veon_amd.retrieval import retrieve_points

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WORDS = 'a photo of the car sedan bus tree road grass there is in scene cone'.split()
VOCABULARY = ['car', 'sedan', 'bus', 'tree', 'grass', 'road']
REFLECTION = [0, 0, 0, 1, 1, 2]                   # three merged classes (+ background)


class _WordTokenizer:
    def __call__(self, texts):
        out = torch.zeros((len(texts), 12), dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [62] + [1 + WORDS.index(w) for w in t.split()] + [63]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def _classifier():
    enc = refs.tower(embed_dim=24, ctx=12, vocab=64, width=64, heads=1, layers=1, seed=5)
    return OvClassifier(enc.to(DEV), _WordTokenizer(),
                        ('a photo of a {}', 'there is the {} in the scene')).to(DEV)


@functools.lru_cache(maxsize=None)
def _path():
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=True)
    plain = _build(g, DEV, native=True)
    clf = _classifier()
    net.set_vocabulary(clf, VOCABULARY, REFLECTION)
    return net, plain, clf, _inputs(g, DEV)


@torch.no_grad()
def test_labels_only_equals_the_torch_composition():
    net, _, clf, (images, geom, depth) = _path()
    assert tuple(net.ov_vocab_weight.shape) == (7, 24) and net.vocabulary_version == 1
    assert torch.equal(net.ov_vocab_weight, clf.classifier_weight(VOCABULARY))
    before = dict(_lib.CALLS)
    out = net(images, geom, depth=depth, labels_only=True, return_features=True)
    after = dict(_lib.CALLS)
    assert after.get('veon_occ_labels_grouped', 0) == before.get('veon_occ_labels_grouped', 0) + 1
    assert after.get('veon_occ_labels', 0) == before.get('veon_occ_labels', 0)
    low = classifier_logits_low(net.ov_vocab_weight, out['feat_low']).float()
    group, labels = [0, 0, 0, 1, 1, 2, 3], out['occ_pred_cls']
    assert labels.dtype == torch.uint8 and labels.shape == (1, 20, 20, 4)
    # the composition a user has without the grouped tail: all seven rows upsampled by the
    # ungrouped kernel, torch's maximum over each run, the first maximum -- exactly equal
    up, _, cls = conv3d_ops.occ_classify(low, out['bin_low'].float(), net.occ_size)
    merged = torch.stack([up[:, 0:3].amax(1), up[:, 3:5].amax(1), up[:, 5], up[:, 6]], dim=1)
    first = torch.where(merged == merged.amax(1, keepdim=True),
                        torch.arange(4, device=DEV).view(1, -1, 1, 1, 1), 4).amin(1)
    want = torch.where(cls == 7, torch.full_like(cls, 3), first.permute(0, 3, 2, 1))
    assert torch.equal(labels.long(), want)
    # and the ATen form (F.interpolate) agrees wherever fp32 rounding cannot decide
    m2, bin_up, want2 = occ_grouped_reference(low, out['bin_low'], net.occ_size, group, 4, 3)
    top2 = m2.topk(2, dim=1).values
    near = ((top2[:, 0] - top2[:, 1]).abs() <= 1e-5 * top2[:, 0].abs().clamp(min=1.0))
    near |= (torch.softmax(bin_up, 1)[:, 0] - 0.5).abs() <= 1e-6
    decided = ~near.permute(0, 3, 2, 1)
    assert float(decided.float().mean()) > 0.99
    assert torch.equal(labels.long()[decided], want2[decided])
    assert len(labels.unique()) >= 2
    full = net(images, geom, depth=depth)
    assert full['sem_occ'].shape == (1, 4, 4, 20, 20)
    assert torch.equal(full['occ_pred_cls'], labels.long())
    assert after.get('veon_occ_classify', 0) == before.get('veon_occ_classify', 0)


@torch.no_grad()
def test_evaluate_counts_the_merged_classes():
    net, _, _, (images, geom, depth) = _path()
    gen = torch.Generator().manual_seed(4)
    shape = (1, 20, 20, 4)
    gt = torch.randint(0, 4, shape, generator=gen)
    gt[torch.rand(shape, generator=gen) < 0.1] = 255
    mask = torch.rand(shape, generator=gen) >= 0.3
    with pytest.raises(ValueError):
        net.evaluate(images, geom, gt, mask.to(DEV), OccMiouMetric(num_classes=8, device=DEV),
                     depth=depth)
    m = OccMiouMetric(num_classes=4, device=DEV)
    before = dict(_lib.CALLS)
    labels = net.evaluate(images, geom, gt.numpy(), mask.to(DEV), m, depth=depth)
    after = dict(_lib.CALLS)
    assert after.get('veon_occ_labels_grouped', 0) == before.get('veon_occ_labels_grouped', 0) + 1
    assert after.get('veon_occ_confusion', 0) == before.get('veon_occ_confusion', 0)
    want = confusion(labels, gt.to(torch.uint8).to(DEV), mask.to(torch.uint8).to(DEV), 4)
    assert torch.equal(m.hist, want) and 0 < int(want.sum()) < labels.numel()
    assert torch.equal(labels, net(images, geom, depth=depth, labels_only=True)['occ_pred_cls'])


@torch.no_grad()
def test_retrieve_by_prompts():
    net, plain, clf, (images, geom, depth) = _path()
    out = net(images, geom, depth=depth, return_features=True)
    g = torch.Generator().manual_seed(2)
    pts = torch.stack([torch.randint(0, 20, (30,), generator=g),
                       torch.randint(0, 20, (30,), generator=g),
                       torch.randint(0, 4, (30,), generator=g)], dim=1).int().to(DEV)
    prompts = ['bus', 'cone', 'tree']
    emb = clf.retrieval_embedding(prompts)
    assert emb.shape == (3, 24)
    score, prob = net.retrieve(out, pts, prompts=prompts)
    want_score, want_prob = retrieve_points(out['feat_low'], out['bin_low'], pts, emb,
                                            net.occ_size)
    assert torch.equal(score, want_score) and torch.equal(prob, want_prob)
    with pytest.raises(ValueError):
        net.retrieve(out, pts)
    with pytest.raises(RuntimeError):
        plain.retrieve(out, pts, prompts=prompts)


@torch.no_grad()
def test_a_path_without_a_vocabulary_is_unchanged():
    """The twin built from the same fixture never saw ``set_vocabulary``: the ungrouped
    kernels, its own 5 + 1 classes, and outputs equal to a path built before the other
    one's vocabulary was set."""
    net, plain, _, (images, geom, depth) = _path()
    before = dict(_lib.CALLS)
    out = plain(images, geom, depth=depth)
    only = plain(images, geom, depth=depth, labels_only=True)
    after = dict(_lib.CALLS)
    assert after.get('veon_occ_classify', 0) == before.get('veon_occ_classify', 0) + 1
    assert after.get('veon_occ_labels', 0) == before.get('veon_occ_labels', 0) + 1
    for name in ('veon_occ_classify_grouped', 'veon_occ_labels_grouped'):
        assert after.get(name, 0) == before.get(name, 0)
    assert out['sem_occ'].shape == (1, 5, 4, 20, 20) and plain.ov_vocab_weight is None
    assert torch.equal(only['occ_pred_cls'].long(), out['occ_pred_cls'])
    fresh = _build(load_golden('path_tiny'), DEV, native=True)
    again = fresh(images, geom, depth=depth)
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert sorted(plain.state_dict()) == sorted(net.state_dict())
