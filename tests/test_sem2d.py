"""The fused 2-D semantic tail (veon_amd/sem2d.py) on the CPU: its torch mirrors against
the maps the reference's own classes recorded (tests/golden/side_adapter_tiny.npz), the
label rules against a hand-written loop, the argument checks, the opt-in wiring and the
C ABI.  Tolerances: tests/sem2d_refs.py."""
import os

import pytest
import torch

from tests import sem2d_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, sem2d


def _fixture():
    g = load_golden('side_adapter_tiny')
    return {k: torch.from_numpy(g[k]) for k in ('mask_logits', 'mask_embs', 'mask_preds',
                                                'sem_seg_ds', 'sem_embed_ds', 'sem_seg')}


def test_mirrors_reproduce_the_recorded_maps():
    f = _fixture()
    logits, embs, preds = f['mask_logits'], f['mask_embs'], f['mask_preds']
    size = tuple(f['sem_seg'].shape[-2:])
    B, Q, K, C, h, w, H, W = refs.SHAPES['fixture']
    assert (tuple(logits.shape), tuple(embs.shape), tuple(preds.shape), size) == \
        ((B, Q, K + 1), (B, Q, C), (B, Q, h, w), (H, W))
    seg_ds, emb_ds = sem2d.semantic_maps_ds(logits, embs, preds)       # CPU: the mirrors
    seg = sem2d.semantic_map(logits, preds, size)
    tol_k, tol_c = refs.class_bound(logits, preds), refs.bound(embs, preds)
    for name, got, tol in (('sem_seg_ds', seg_ds, tol_k), ('sem_embed_ds', emb_ds, tol_c),
                           ('sem_seg', seg, tol_k)):
        ratio = refs.excess(got, f[name], tol, factor=2.0)
        print(name, 'mirror vs fixture: %.3f of 2 * bound' % ratio)
        assert ratio <= 1.0, (name, ratio)
    r_ds, r_emb, r_seg = refs.ref64(logits, embs, preds, size)
    for name, ref in (('sem_seg_ds', r_ds), ('sem_embed_ds', r_emb), ('sem_seg', r_seg)):
        err = float((ref - f[name].double()).abs().max())
        print(name, 'fp64 vs fixture: %.3g' % err)
        assert err <= 2.1e-7, (name, err)
        ratio = refs.excess(ref, f[name], tol_c if name == 'sem_embed_ds' else tol_k)
        assert ratio <= 1.0, (name, ratio)      # the fixture itself is within the bound
    assert sem2d.semantic_maps_ds(logits, None, preds)[1] is None


def test_mirror_error_is_a_small_share_of_the_bound():
    """torch's own fp32 tail against fp64 on every shape of the GPU tests stays within half
    the bound: an fp32 implementation as good as torch's, but with other roundings, fits."""
    for name, shape in refs.SHAPES.items():
        logits, embs, preds = refs.random_inputs(shape, refs.SEED)
        size = shape[-2:]
        r_ds, r_emb, r_seg = refs.ref64(logits, embs, preds, size, name in refs.ATEN_INDEX)
        seg_ds, emb_ds = sem2d.semantic_maps_ds_torch(logits, embs, preds)
        seg = sem2d.semantic_map_torch(logits, preds, size)
        tol_k, tol_c = refs.class_bound(logits, preds), refs.bound(embs, preds)
        ratios = (refs.excess(seg_ds, r_ds, tol_k), refs.excess(emb_ds, r_emb, tol_c),
                  refs.excess(seg, r_seg, tol_k))
        print(name, 'torch fp32 vs fp64, share of the bound: %.3f %.3f %.3f' % ratios)
        assert max(ratios) <= 0.5, (name, ratios)


def test_label_statistics_of_the_gpu_cases():
    """What tests/test_sem2d_gpu.py asserts of the native labels holds for torch's fp32
    labels on the same inputs: they differ from fp64's only at pixels whose fp64 top-two
    margin is within 2 * max_c bound, and at most 0.5 % of the pixels have such a margin."""
    for name, shape in refs.SHAPES.items():
        if name == 'fixture':
            continue
        logits, embs, preds = refs.random_inputs(shape, refs.SEED)
        size = shape[-2:]
        group, n_merged = (refs.GROUP_67_17, 17) if shape[2] == 67 else (None, None)
        ref_seg = refs.ref64(logits, None, preds, size, name in refs.ATEN_INDEX)[2]
        labels = sem2d.semantic_labels(logits, preds, size, group, n_merged)
        want = sem2d.labels_of_map(ref_seg, group, n_merged)
        margin = refs.top_two_margin(ref_seg, group, n_merged)
        tol = refs.class_bound(logits, preds).max(dim=1).values[:, None, None]
        close = margin <= 2.0 * tol
        print(name, 'torch labels differ at %d pixels, %.4f %% have a small margin'
              % (int((labels != want).sum()), 100 * float(close.double().mean())))
        assert not ((labels != want) & ~close).any()
        assert float(close.double().mean()) <= 0.005


def test_grouped_labels_equal_a_loop_with_an_exact_tie():
    """K = 7 rows in three groups; at one pixel two groups attain the maximum exactly
    (the lowest channel wins), at another two rows of one group tie."""
    torch.manual_seed(3)
    sem = torch.rand(2, 7, 5, 6)
    group, n_merged = [0, 0, 1, 1, 1, 2, 2], 3
    sem[0, :, 1, 2] = torch.tensor([0.1, 0.2, 0.9, 0.3, 0.4, 0.9, 0.5])    # groups 1 and 2 tie
    sem[1, :, 4, 5] = torch.tensor([0.7, 0.7, 0.1, 0.2, 0.3, 0.4, 0.5])    # inside group 0
    sem[1, :, 0, 0] = torch.tensor([0.5, 0.1, 0.2, 0.5, 0.1, 0.5, 0.1])    # all three tie
    got = sem2d.labels_of_map(sem, group, n_merged)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 5, 6)
    assert torch.equal(got, refs.loop_labels(sem, group, n_merged))
    assert got[0, 1, 2] == 1 and got[1, 4, 5] == 0 and got[1, 0, 0] == 0
    plain = sem2d.labels_of_map(sem)
    assert torch.equal(plain, refs.loop_labels(sem, None, None))
    assert plain[0, 1, 2] == 2 and plain[1, 0, 0] == 0
    # through the public call: labels of the mirror's map
    shape = (2, 6, 7, 3, 3, 4, 9, 10)
    logits, _, preds = refs.random_inputs(shape, seed=5)
    labels = sem2d.semantic_labels(logits, preds, (9, 10), group, n_merged)
    want = refs.loop_labels(sem2d.semantic_map_torch(logits, preds, (9, 10)), group, n_merged)
    assert torch.equal(labels, want)


def test_nan_proposal_gives_ignore_label_where_the_map_is_nan():
    shape = (2, 6, 4, 3, 3, 5, 12, 20)
    logits, _, preds = refs.random_inputs(shape, seed=7)
    preds[1, 2, 1, 3] = float('nan')
    sem = sem2d.semantic_map(logits, preds, (12, 20))
    nan = torch.isnan(sem).any(dim=1)
    assert nan.any() and not nan[0].any() and not nan.all()
    assert torch.equal(nan[1], refs.touched((12, 20), (3, 5), 1, 3))
    assert torch.equal(torch.isnan(sem).all(dim=1), nan)        # every row of such a pixel
    for kw in (dict(), dict(group=[0, 0, 1, 2], n_merged=3), dict(ignore_label=200)):
        labels = sem2d.semantic_labels(logits, preds, (12, 20), **kw)
        ignore = kw.get('ignore_label', 255)
        assert torch.equal(labels == ignore, nan), kw
        assert int(labels[~nan].max()) < 4


def test_argument_checks():
    B, Q, K = 2, 5, 4
    logits, preds = torch.zeros(B, Q, K + 1), torch.zeros(B, Q, 3, 4)
    embs = torch.zeros(B, Q, 6)
    size = (6, 8)
    with pytest.raises(ValueError):                                   # Q = 257
        sem2d.semantic_map(torch.zeros(1, 257, 3), torch.zeros(1, 257, 2, 2), size)
    with pytest.raises(ValueError):                                   # K + 1 = 257
        sem2d.semantic_map(torch.zeros(1, 4, 257), torch.zeros(1, 4, 2, 2), size)
    with pytest.raises(ValueError):
        sem2d.semantic_labels(torch.zeros(1, 4, 257), torch.zeros(1, 4, 2, 2), size)
    with pytest.raises(ValueError):
        sem2d.semantic_maps_ds(torch.zeros(1, 257, 3), None, torch.zeros(1, 257, 2, 2))
    # the limits themselves are accepted
    assert tuple(sem2d.semantic_map(torch.zeros(1, 256, 256), torch.zeros(1, 256, 1, 1),
                                    (2, 3)).shape) == (1, 255, 2, 3)
    for bad_preds in (torch.zeros(B + 1, Q, 3, 4), torch.zeros(B, Q + 1, 3, 4)):
        with pytest.raises(ValueError):
            sem2d.semantic_map(logits, bad_preds, size)
        with pytest.raises(ValueError):
            sem2d.semantic_maps_ds(logits, embs, bad_preds)
        with pytest.raises(ValueError):
            sem2d.semantic_labels(logits, bad_preds, size)
    for bad_embs in (torch.zeros(B + 1, Q, 6), torch.zeros(B, Q + 1, 6)):
        with pytest.raises(ValueError):
            sem2d.semantic_maps_ds(logits, bad_embs, preds)
    for group, n_merged in (([0, 1, 0, 2], 3),          # a split run
                            ([0, 0, 1, 3], 3),          # a channel out of range
                            ([0, 0, 1, 1], 3),          # a channel without a row
                            ([0, 1, 2], 3),             # not K entries
                            ([0, 0, 1, 2], None)):      # no n_merged
        with pytest.raises(ValueError):
            sem2d.semantic_labels(logits, preds, size, group, n_merged)
    with pytest.raises(ValueError):
        sem2d.semantic_labels(logits, preds, size, ignore_label=256)
    with pytest.raises(ValueError):
        sem2d.semantic_map(logits, preds, (0, 8))


def test_a_caller_with_gradients_keeps_the_torch_lines():
    shape = (1, 4, 3, 5, 2, 3, 6, 7)
    logits, embs, preds = refs.random_inputs(shape, seed=2)
    preds.requires_grad_(True)
    seg_ds, emb_ds = sem2d.semantic_maps_ds(logits, embs, preds)
    seg = sem2d.semantic_map(logits, preds, (6, 7))
    (seg_ds.sum() + emb_ds.sum() + seg.sum()).backward()
    assert preds.grad is not None and torch.isfinite(preds.grad).all()
    assert sem2d.semantic_labels(logits, preds, (6, 7)).dtype == torch.uint8


def _network():
    from tests.test_side_adapter import CFG, _build, _clip_feats
    g = load_golden('side_adapter_tiny')
    trunk, head, net = _build(g)
    images = torch.from_numpy(g['images'])
    ov = torch.from_numpy(g['ov_classifier_weight'])
    with torch.no_grad():
        feats = _clip_feats(trunk, images, CFG['clip_first_tail'])
    return net, head, ov, images, feats


@torch.no_grad()
def test_branch_with_the_native_tail_is_unchanged_on_the_cpu():
    from veon_amd.models.semantic_net import semantic_branch_2d
    net, head, ov, images, feats = _network()
    default = semantic_branch_2d(net, head, ov, images, feats)
    native = semantic_branch_2d(net, head, ov, images, feats, native_tail=True)
    assert set(native) == set(default)
    for k, v in default.items():
        if k in ('attn_biases', 'san_features'):
            assert all(torch.equal(a, b) for a, b in zip(v, native[k])), k
        else:
            assert torch.equal(v, native[k]), k
    ds_only = semantic_branch_2d(net, head, ov, images, feats, native_tail=True, full=False)
    assert set(ds_only) == set(default) - {'sem_seg'}
    assert torch.equal(ds_only['sem_seg_ds'], default['sem_seg_ds'])
    lab = semantic_branch_2d(net, head, ov, images, feats, native_tail=True, labels=True)
    assert set(lab) == set(default) | {'labels_2d'}
    assert lab['labels_2d'].dtype == torch.uint8
    assert tuple(lab['labels_2d'].shape) == (2, 64, 96)
    assert torch.equal(lab['labels_2d'].long(), default['sem_seg'].argmax(dim=1))
    for kw in (dict(full=False), dict(labels=True)):
        with pytest.raises(ValueError):                 # the torch lines know neither
            semantic_branch_2d(net, head, ov, images, feats, **kw)


@torch.no_grad()
def test_path_switch():
    from veon_amd.models.veon_occ import VeonOccupancyPath
    assert VeonOccupancyPath.hip_tail_2d is False
    grid = {'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0], 'z': [-1.0, 3.0, 1.0],
            'depth': [1.0, 13.0, 1.0]}
    torch.manual_seed(0)
    net = VeonOccupancyPath(
        input_size=(64, 96), num_cam=2, clip_width=64, clip_layers=4, clip_heads=2,
        clip_first_tail=3, clip_proj_dim=24, embed_dim=64, n_classes=5, occ_size=(4, 20, 20),
        hsa_dim=64, hsa_fusion_map=('0->1->1', '1->2->2'), grid_config=grid, bf16_heads=False,
        two_streams=False, clip_image=32,
        side_adapter=dict(image_size=64, width=48, depth=4, num_heads=3, num_queries=5,
                          fusion_map=('0->0', '1->1', '2->2', '3->3'),
                          deep_supervision_idxs=(4,), embed_channels=16,
                          mlp_channels=24)).eval()
    images = torch.randn(1, 2, 3, 64, 96)
    default = net.forward_2d(images)
    with pytest.raises(ValueError):
        net.forward_2d(images, labels=True)
    net.hip_tail_2d = True
    out = net.forward_2d(images, labels=True)
    assert set(out) == set(default) | {'labels_2d'}
    for k in ('sem_seg_ds', 'sem_embed_ds', 'sem_seg', 'mask_logits'):
        assert torch.equal(out[k], default[k]), k
    assert tuple(out['labels_2d'].shape) == (2, 64, 96)
    assert torch.equal(out['labels_2d'].long(), default['sem_seg'].argmax(dim=1))
    assert 'sem_seg' not in net.forward_2d(images, full=False)
    # (forward(with_2d=True) lifts, which has no CPU path: tests/test_sem2d_gpu.py)


def test_header_declares_the_entry_points():
    names = ('veon_sem2d_ds', 'veon_sem2d_full', 'veon_sem2d_labels')
    with open(os.path.join(_lib.INCLUDE, 'veon_hip.h')) as f:
        header = f.read()
    for name in names:
        assert 'int %s(' % name in header
        assert name in _lib.declared_symbols()
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is _lib._C_TYPES['int']
        assert argtypes[-1] is _lib.ctypes.c_void_p          # the stream goes last
    assert len(_lib._SIGNATURES['veon_sem2d_full'][1]) == 12
    assert '#define VEON_ABI_VERSION 2' in header
    assert header.count('san_in_veon_temporal.py:176-186, 240-255') >= 1
