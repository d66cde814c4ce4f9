"""The fused 2-D semantic tail (csrc/sem2d.hip through veon_amd/sem2d.py) on the GPU
against fp64 restatements of the reference's lines.  Shapes, inputs and tolerances:
tests/sem2d_refs.py."""
import functools

import pytest
import torch

from tests import sem2d_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, sem2d

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = sorted(refs.SHAPES)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (host), the fp64 maps and the tolerances of one shape; never modified."""
    shape = refs.SHAPES[name]
    if name == 'fixture':
        g = load_golden('side_adapter_tiny')
        logits, embs, preds = (torch.from_numpy(g[k])
                               for k in ('mask_logits', 'mask_embs', 'mask_preds'))
    else:
        logits, embs, preds = refs.random_inputs(shape, refs.SEED)
    size = tuple(shape[-2:])
    r_ds, r_emb, r_seg = refs.ref64(logits, embs, preds, size, name in refs.ATEN_INDEX)
    return dict(logits=logits, embs=embs, preds=preds, size=size, ref_ds=r_ds, ref_emb=r_emb,
                ref_seg=r_seg, tol_k=refs.class_bound(logits, preds),
                tol_c=refs.bound(embs, preds))


def _native(case):
    logits, embs, preds = (case[k].to(DEV) for k in ('logits', 'embs', 'preds'))
    before = dict(_lib.CALLS)
    seg_ds, emb_ds = sem2d.semantic_maps_ds(logits, embs, preds)
    seg = sem2d.semantic_map(logits, preds, case['size'])
    for name in ('veon_sem2d_ds', 'veon_sem2d_full'):
        assert _lib.CALLS.get(name, 0) == before.get(name, 0) + 1, name
    return seg_ds, emb_ds, seg


@pytest.mark.parametrize('name', NAMES)
def test_maps_against_fp64(name):
    case = _case(name)
    B, Q, K, C, h, w, H, W = refs.SHAPES[name]
    seg_ds, emb_ds, seg = _native(case)
    assert tuple(seg_ds.shape) == (B, K, h, w) and tuple(emb_ds.shape) == (B, C, h, w)
    assert tuple(seg.shape) == (B, K, H, W)
    ratios = (refs.excess(seg_ds, case['ref_ds'], case['tol_k']),
              refs.excess(emb_ds, case['ref_emb'], case['tol_c']),
              refs.excess(seg, case['ref_seg'], case['tol_k']))
    print(name, 'native vs fp64, share of the bound: %.3f %.3f %.3f' % ratios)
    assert max(ratios) <= 1.0, ratios
    again = _native(case)
    for a, b in zip((seg_ds, emb_ds, seg), again):
        assert torch.equal(a, b)
    only_seg, none = sem2d.semantic_maps_ds(case['logits'].to(DEV), None,
                                            case['preds'].to(DEV))
    assert none is None and torch.equal(only_seg, seg_ds)


def test_maps_against_the_recorded_fixture():
    g = load_golden('side_adapter_tiny')
    case = _case('fixture')
    for name, got, tol in zip(('sem_seg_ds', 'sem_embed_ds', 'sem_seg'), _native(case),
                              (case['tol_k'], case['tol_c'], case['tol_k'])):
        ratio = refs.excess(got, torch.from_numpy(g[name]), tol, factor=2.0)
        print(name, 'native vs fixture: %.3f of 2 * bound' % ratio)
        assert ratio <= 1.0, (name, ratio)


def test_saturated_proposals_weigh_exactly_one_and_zero():
    """mask_preds = +-1e4: the sigmoid is exactly 1 or 0 (no NaN from the overflowing
    exponential).  With one sign per proposal every pixel of an image then holds the same
    sum, bit for bit, at both resolutions; its tolerance against fp64 has no argument term
    (max|mask_preds| -> 0: a saturated sigmoid does not feel its argument's rounding)."""
    shape = B, Q, K, C, h, w, H, W = refs.SHAPES['production_q_odd_source']
    logits, embs, _ = refs.random_inputs(shape, refs.SEED)
    g = torch.Generator().manual_seed(1)
    sign = torch.where(torch.rand(B, Q, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    preds = (1e4 * sign).expand(B, Q, h, w).contiguous()
    case = dict(logits=logits, embs=embs, preds=preds, size=(H, W))
    seg_ds, emb_ds, seg = _native(case)
    for t in (seg_ds, emb_ds, seg):
        assert torch.isfinite(t).all()
    assert torch.equal(seg_ds, seg_ds[:, :, :1, :1].expand_as(seg_ds))
    assert torch.equal(emb_ds, emb_ds[:, :, :1, :1].expand_as(emb_ds))
    assert torch.equal(seg, seg_ds[:, :, :1, :1].expand_as(seg))
    r_ds, r_emb, r_seg = refs.ref64(logits, embs, preds, (H, W))
    assert refs.excess(seg, r_seg, refs.class_bound(logits, preds, max_pred=0.0)) <= 1.0
    assert refs.excess(emb_ds, r_emb, refs.bound(embs, preds, max_pred=0.0)) <= 1.0
    # every proposal off: exactly zero; signs that differ from pixel to pixel: still finite
    off = dict(case, preds=torch.full((B, Q, h, w), -1e4))
    for t in _native(off):
        assert torch.equal(t, torch.zeros_like(t))
    mixed = torch.where(torch.rand(B, Q, h, w, generator=g) < 0.5, -1e4, 1e4)
    m_ds, m_emb, m_seg = _native(dict(case, preds=mixed))
    assert torch.isfinite(m_ds).all() and torch.isfinite(m_emb).all()
    assert torch.isfinite(m_seg).all()
    assert refs.excess(m_ds, refs.ref64(logits, embs, mixed, (H, W))[0],
                       refs.class_bound(logits, mixed, max_pred=0.0)) <= 1.0


@pytest.mark.parametrize('name', ['production_q_odd_source', 'one_class_fractional_scale'])
def test_nan_proposal_reaches_exactly_the_pixels_that_tap_it(name):
    shape = B, Q, K, C, h, w, H, W = refs.SHAPES[name]
    logits, embs, preds = refs.random_inputs(shape, refs.SEED)
    b, q, y, x = B - 1, Q // 2, h - 1, w // 2
    preds[b, q, y, x] = float('nan')
    seg_ds, emb_ds, seg = _native(dict(logits=logits, embs=embs, preds=preds, size=(H, W)))
    want = torch.zeros(B, H, W, dtype=torch.bool)
    want[b] = refs.touched((H, W), (h, w), y, x)
    assert want.any() and not want[b].all()
    assert torch.equal(torch.isnan(seg).cpu(), want[:, None].expand(B, K, H, W))
    want_ds = torch.zeros(B, h, w, dtype=torch.bool)
    want_ds[b, y, x] = True
    assert torch.equal(torch.isnan(seg_ds).cpu(), want_ds[:, None].expand(B, K, h, w))
    assert torch.equal(torch.isnan(emb_ds).cpu(), want_ds[:, None].expand(B, C, h, w))
    labels = sem2d.semantic_labels(logits.to(DEV), preds.to(DEV), (H, W), ignore_label=200)
    assert torch.equal((labels == 200).cpu(), want)


def _group_of(name):
    return (refs.GROUP_67_17, 17) if refs.SHAPES[name][2] == 67 else (None, None)


@pytest.mark.parametrize('grouped', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_labels_are_the_argmax_of_the_native_map(name, grouped):
    group, n_merged = _group_of(name) if grouped else (None, None)
    if grouped and group is None:
        K = refs.SHAPES[name][2]         # every shape has a grouped case: runs of r rows
        r = max(2, -(-K // 64))
        group, n_merged = [c // r for c in range(K)], -(-K // r)
    case = _case(name)
    logits, preds = case['logits'].to(DEV), case['preds'].to(DEV)
    seg = sem2d.semantic_map(logits, preds, case['size'])
    before = _lib.CALLS.get('veon_sem2d_labels', 0)
    labels = sem2d.semantic_labels(logits, preds, case['size'], group, n_merged)
    assert _lib.CALLS.get('veon_sem2d_labels', 0) == before + 1
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (seg.shape[0],) + case['size']
    assert torch.equal(labels, sem2d.labels_of_map(seg, group, n_merged))
    assert torch.equal(labels, sem2d.semantic_labels(logits, preds, case['size'], group,
                                                     n_merged))


@pytest.mark.parametrize('name', NAMES)
def test_labels_against_fp64(name):
    """A label may differ from fp64's only where fp64's two best (merged) channels are
    closer than the two maps may be wrong together, 2 * max_c bound; and such pixels are
    rare (at most 0.5 %), so the first condition is not empty talk."""
    case = _case(name)
    group, n_merged = _group_of(name)
    logits, preds = case['logits'].to(DEV), case['preds'].to(DEV)
    labels = sem2d.semantic_labels(logits, preds, case['size'], group, n_merged).cpu()
    want = sem2d.labels_of_map(case['ref_seg'], group, n_merged)
    margin = refs.top_two_margin(case['ref_seg'], group, n_merged)
    close = margin <= 2.0 * case['tol_k'].max(dim=1).values[:, None, None]
    share = float(close.double().mean())
    differ = labels != want
    print(name, 'labels differ from fp64 at %d pixels, %.4f %% have a small margin'
          % (int(differ.sum()), 100 * share))
    assert not (differ & ~close).any()
    assert share <= 0.005, share


def test_peak_memory_stays_below_the_tensor_that_must_not_exist():
    B, Q, K, h, w, H, W = 2, 100, 17, 8, 8, 128, 128
    logits, _, preds = refs.random_inputs((B, Q, K, 1, h, w, H, W), refs.SEED)
    logits, preds = logits.to(DEV), preds.to(DEV)

    def rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del out
        return peak - base

    sem2d.semantic_map(logits, preds, (H, W))                   # warm-up
    r_map = rise(lambda: sem2d.semantic_map(logits, preds, (H, W)))
    r_lab = rise(lambda: sem2d.semantic_labels(logits, preds, (H, W)))
    r_torch = rise(lambda: sem2d.semantic_map_torch(logits, preds, (H, W)))
    print('peak rise: map %d, labels %d, torch tail %d bytes' % (r_map, r_lab, r_torch))
    assert r_map < B * Q * H * W * 4
    assert r_lab < B * K * H * W * 4
    assert r_torch >= B * Q * H * W * 4       # what the torch lines form


def test_graph_capture_replays_with_fresh_inputs():
    shape = refs.SHAPES['production_q_odd_source']
    size = tuple(shape[-2:])
    first = [t.to(DEV) for t in refs.random_inputs(shape, refs.SEED)]
    second = [t.to(DEV) for t in refs.random_inputs(shape, refs.SEED + 1)]
    third = [t.to(DEV) for t in refs.random_inputs(shape, refs.SEED + 2)]
    static = [t.clone() for t in first]

    def step(inp):
        logits, embs, preds = inp
        return sem2d.semantic_maps_ds(logits, embs, preds) + (
            sem2d.semantic_map(logits, preds, size),
            sem2d.semantic_labels(logits, preds, size))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)                                               # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step(static)
    for fresh in (second, third):
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for a, b in zip(got, step(fresh)):
            assert torch.equal(a, b)
    assert not torch.equal(got[2], step(first)[2])


@torch.no_grad()
def test_branch_with_the_native_tail():
    from tests.test_side_adapter import CFG, _build, _clip_feats
    from veon_amd.models.semantic_net import semantic_branch_2d
    g = load_golden('side_adapter_tiny')
    trunk, head, net = (m.to(DEV) for m in _build(g))
    images = torch.from_numpy(g['images']).to(DEV)
    ov = torch.from_numpy(g['ov_classifier_weight']).to(DEV)
    feats = _clip_feats(trunk, images, CFG['clip_first_tail'])
    default = semantic_branch_2d(net, head, ov, images, feats)
    before = dict(_lib.CALLS)
    native = semantic_branch_2d(net, head, ov, images, feats, native_tail=True, labels=True)
    for name in ('veon_sem2d_ds', 'veon_sem2d_full', 'veon_sem2d_labels'):
        assert _lib.CALLS.get(name, 0) == before.get(name, 0) + 1, name
    assert set(native) == set(default) | {'labels_2d'}
    logits, embs, preds = (default[k].cpu() for k in ('mask_logits', 'mask_embs', 'mask_preds'))
    tol_k, tol_c = refs.class_bound(logits, preds), refs.bound(embs, preds)
    for k, tol in (('sem_seg_ds', tol_k), ('sem_embed_ds', tol_c), ('sem_seg', tol_k)):
        assert native[k].shape == default[k].shape
        ratio = refs.excess(native[k], default[k], tol, factor=2.0)
        print(k, 'native tail vs torch tail: %.3f of 2 * bound' % ratio)
        assert ratio <= 1.0, (k, ratio)
    for k in ('mask_preds', 'mask_embs', 'mask_logits'):
        assert torch.equal(native[k], default[k]), k
    for k in ('attn_biases', 'san_features'):
        assert all(torch.equal(a, b) for a, b in zip(native[k], default[k])), k
    assert torch.equal(native['labels_2d'], sem2d.labels_of_map(native['sem_seg']))


@torch.no_grad()
def test_path_returns_2d_labels():
    from veon_amd import synthetic
    from veon_amd.models.veon_occ import VeonOccupancyPath
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
                          mlp_channels=24)).to(DEV).eval()
    images = torch.randn(1, 2, 3, 64, 96, device=DEV)
    metas = [t.to(DEV) for t in synthetic.rig_inputs(synthetic.make_rig(1, 2, (64, 96)))]
    plain = net(images, metas, with_2d=True)
    assert '2d_labels' not in plain
    net.hip_tail_2d = True
    before = _lib.CALLS.get('veon_sem2d_labels', 0)
    out = net(images, metas, with_2d=True)
    assert _lib.CALLS.get('veon_sem2d_labels', 0) == before + 1
    assert set(out) == set(plain) | {'2d_labels'}
    assert out['2d_labels'].dtype == torch.uint8
    assert tuple(out['2d_labels'].shape) == (2, 64, 96)
    assert torch.equal(out['2d_labels'], sem2d.labels_of_map(out['2d_sem_seg']))
    two_d = net.forward_2d(images, full=False, labels=True)
    assert 'sem_seg' not in two_d and tuple(two_d['labels_2d'].shape) == (2, 64, 96)
