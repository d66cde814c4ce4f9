"""GPU checks of the native LiDAR depth render (csrc/lidar_depth.hip through
``veon_amd.lidar_depth.multiview_depth``), every comparison against the torch mirror or the
fp64 oracle on the CPU.

Image-point mode (``lidar2img=None``) does no arithmetic beyond ``u / downsample``, so the
result is bit-equal to the mirror's.  In projection mode the seam cases use matrices whose
products are exact in fp32 (small integers and powers of two), bit-equal again; the
``margin_case`` of tests/lidar_depth_refs.py keeps every pair 0.05 pixels from a rounding
seam, so the occupied pixels must be the fp64 oracle's, and each depth lies within
8 * 2^-24 * sum |terms| of its own dot product: three products and three sums round at
most four times, doubled for the post_rot row (``oracle``'s ``bound``, per point)."""
import math

import pytest
import torch
import torch.nn as nn

from tests import lidar_depth_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, depth_loss, lidar_depth
from veon_amd.depth_ops import downsample_depth_torch
from veon_amd.models import VeonDepthPretrain, build_neck

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LO, HI = refs.GRID[:2]
ENTRY = 'veon_lidar_depth_render'
NAN, INF = float('nan'), float('inf')


def to_dev(t):
    if isinstance(t, (list, tuple)):
        return [to_dev(v) for v in t]
    return None if t is None else t.to(DEV)


def native(points, mats, h, w, rng=(LO, HI), **kw):
    """One native call -> the CPU copy of its result."""
    n0 = _lib.CALLS.get(ENTRY, 0)
    mats = [to_dev(m) for m in mats] if mats is not None else [None] * 3
    out = lidar_depth.multiview_depth(to_dev(points), *mats, h, w, rng, **kw)
    assert _lib.CALLS.get(ENTRY, 0) == n0 + 1
    return out.cpu()


def mirror(points, mats, h, w, rng=(LO, HI), **kw):
    mats = mats if mats is not None else [None] * 3
    return lidar_depth.multiview_depth_torch(points, *mats, h, w, rng, **kw)


def check_image_points(points, h, w, **kw):
    got, want = native(points, None, h, w, **kw), mirror(points, None, h, w, **kw)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    return got


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize('case', sorted(refs.FIXTURES))
def test_reference_fixtures(case):
    golden = load_golden('lidar_depth_tiny')
    h, w = (int(v) for v in golden[case + '_size'])
    got = check_image_points(torch.from_numpy(golden[case + '_points'])[None], h, w)
    assert int((got != 0).sum()) == golden[case + '_index'].shape[0]


# ------------------------------------------------------------------ collisions
def test_collisions_exact_minimum_in_any_order():
    g = torch.Generator().manual_seed(2)
    n, h, w = 4096, 8, 16
    pix = torch.tensor([[0.0, 0.0], [15.0, 7.0], [7.0, 3.0], [8.0, 3.0]])
    which = torch.randint(0, 4, (n,), generator=g)
    d = LO + (HI - LO) * torch.rand(n, generator=g, dtype=torch.float64)
    pts = torch.cat([pix[which] + (torch.rand(n, 2, generator=g) - 0.5) * 0.9,
                     d.to(torch.float32)[:, None]], 1)
    got = check_image_points(pts[None], h, w)
    assert int((got != 0).sum()) == 4
    for k, (x, y) in enumerate(pix.long().tolist()):
        assert float(got[0, 0, y, x]) == float(pts[which == k, 2].min())
    for seed in (3, 4):
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
        assert torch.equal(native(pts[perm][None], None, h, w), got)


# ------------------------------------------------------------------ seams
HALVES_X = (-0.5, 0.5, 1.5, 2.5, 14.5, 15.5)
HALVES_Y = (-0.5, 0.5, 1.5, 2.5, 6.5, 7.5)


def range_ends():
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    zero = torch.tensor(0.0)
    return [LO, float(torch.nextafter(lo, zero)), float(torch.nextafter(hi, zero)), HI]


def test_half_integers_round_to_even():
    """one point per half-integer, each with a depth of its own"""
    h, w = 8, 16
    rows = [[x, 3.0, 2.0 + i] for i, x in enumerate(HALVES_X)] + \
           [[5.0, y, 10.0 + i] for i, y in enumerate(HALVES_Y)]
    got = check_image_points(torch.tensor(rows)[None], h, w)
    want = torch.zeros(h, w)
    want[3, 0] = 2.0            # -0.5 -> -0.0 and 0.5 -> 0.0: pixel 0, the nearer of 2, 3
    want[3, 2] = 4.0            # 1.5, 2.5 -> 2
    want[3, 14] = 6.0           # 14.5 -> 14; 15.5 -> 16 is outside
    want[0, 5] = 10.0
    want[2, 5] = 12.0
    want[6, 5] = 14.0           # 6.5 -> 6; 7.5 -> 8 is outside
    assert torch.equal(got[0, 0], want)


def test_seams_of_the_filter():
    h, w = 8, 16
    ends = range_ends()
    rows = [[x, y, d] for x in HALVES_X for y in HALVES_Y for d in ends]
    for bad in (NAN, INF, -INF, 1e30, -1e30):
        rows += [[bad, 3.0, 5.0], [3.0, bad, 5.0], [3.0, 3.0, bad], [bad, bad, bad]]
    pts = torch.tensor(rows)
    got = check_image_points(pts[None], h, w)
    # lo is kept, its predecessor is not; hi is not kept, its predecessor is
    assert float(got[0, 0, 0, 0]) == LO and set(got.unique().tolist()) == {0.0, LO}
    only = torch.tensor([[4.0, 4.0, ends[1]], [5.0, 4.0, ends[3]], [6.0, 4.0, ends[2]]])
    got = check_image_points(only[None], h, w)
    assert got[0, 0, 4, 4:7].tolist() == [0.0, 0.0, ends[2]]


def exact_rig():
    """Two cameras whose arithmetic is exact in fp32 on small dyadic inputs: lidar2img =
    [I | t] and a permuted, sign-flipped variant; post_rot scales by powers of two and
    feeds the depth into u (the full 3 x 3 is used); integer post_tran."""
    l2i = torch.tensor([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
                        [[0.0, 2.0, 0.0, 1.0], [2.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]]])
    rot = torch.tensor([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
                        [[0.5, 0.0, 0.25], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]]])
    tran = torch.tensor([[0.0, 0.0, 0.0], [1.0, -2.0, 0.0]])
    return [l2i[None], rot[None], tran[None]]


def test_projection_seams():
    """z = 0, z < 0, NaN and huge rows in projection mode; camera 1 looks along -z"""
    h, w = 8, 16
    rows = [[3.0, 2.0, 0.0], [0.0, 0.0, 0.0], [-3.0, -2.0, 0.0],          # z = 0: inf, NaN
            [6.0, 4.0, 2.0], [-6.0, -4.0, -2.0],                           # (3, 2) at d = +-2
            [1.0, 1.0, 2.0], [3.0, 5.0, 2.0], [-1.0, 1.0, 2.0],            # halves of camera 0
            [2.0, 4.0, -2.0], [8.0, 2.0, -4.0], [8.0, 24.0, -8.0],         # camera 1
            [3.0, 3.0, LO], [3.0 * HI, 3.0 * HI, HI], [4.0, 4.0, -LO],
            [NAN, 1.0, 2.0], [1.0, NAN, 2.0], [1.0, 1.0, NAN], [INF, 1.0, 2.0],
            [1.0, 1.0, INF], [1e30, 1e30, 2.0], [1e30, 1.0, 1e30], [1.0, 1.0, -INF]]
    pts = torch.tensor(rows)[None]
    mats = exact_rig()
    got, want = native(pts, mats, h, w), mirror(pts, mats, h, w)
    assert torch.equal(got, want)
    # camera 0: (3, 2), (0, 0) twice, (2, 2), (3, 3); camera 1, which sees the z < 0 points
    # only: (4, 2) at 2 m, (3, 6) at 4 m, (6, 2) at 8 m
    assert float(got[0, 0, 2, 3]) == 2.0 and int((got[0, 0] != 0).sum()) == 4
    want1 = torch.zeros(h, w)
    want1[2, 4], want1[6, 3], want1[2, 6] = 2.0, 4.0, 8.0
    assert torch.equal(got[0, 1], want1)


# ------------------------------------------------------------------ sizes and inputs
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_point_counts(n):
    h, w = 16, 32
    got = check_image_points(refs.fixture_points(30 + n, h, w, n)[None], h, w)
    assert tuple(got.shape) == (1, 1, h, w) and (n > 0 or not bool(got.any()))


def test_batch_stride_and_downsample():
    """B = 3 with an all-NaN sample in the middle, 5-float rows read in place, downsample 2"""
    h, w, n = 32, 64, 300
    g = torch.Generator().manual_seed(9)
    pts = torch.full((3, n, 5), 1e9)
    pts[:, :, 3:] = torch.randn(3, n, 2, generator=g) * 100     # never read
    pts[0, :, :3] = refs.fixture_points(40, h, w, n)
    pts[1, :, :3] = NAN
    pts[2, :, :3] = refs.fixture_points(41, h, w, n)
    got = check_image_points(pts, h, w, downsample=2)
    assert tuple(got.shape) == (3, 1, 16, 32)
    assert int((got[1] != 0).sum()) == 0 and bool((got[0] != 0).any()) and \
        bool((got[2] != 0).any()) and not torch.equal(got[0], got[2])
    assert torch.equal(got[2:], check_image_points(pts[2:, :, :3].contiguous(), h, w,
                                                   downsample=2))
    check_image_points(pts, h, w, downsample=2, block=4)


# ------------------------------------------------------------------ projection
@pytest.fixture(scope='module')
def margin():
    case = refs.margin_case(3, n=2000)
    ora = refs.oracle(case['points'], case['lidar2img'], case['post_rots'], case['post_trans'],
                      case['height'], case['width'], case['lo'], case['hi'])
    return case, ora


def test_projection_against_the_fp64_oracle(margin):
    case, ora = margin
    mats = [case['lidar2img'], case['post_rots'], case['post_trans']]
    got = native(case['points'], mats, case['height'], case['width'])
    assert torch.equal(got != 0, ora['depth'] != 0)
    assert int((got != 0).sum()) == 2000
    err = (got.double() - ora['depth']).abs()
    worst = float((err / ora['bound'].clamp_min(1e-30)).max())
    print('margin_case: largest error / bound = %.3f' % worst)
    assert bool((err <= ora['bound']).all()), worst
    # two samples of unequal length as a list: NaN padding, B = 2
    p = case['points'][0]
    mats2 = [m.expand(2, *m.shape[1:]).contiguous() for m in mats]
    both = native([p[:1203], p[1203:]], mats2, case['height'], case['width'])
    # every point has a pixel of its own: the two samples' maps are disjoint
    assert torch.equal(torch.where(both[0] != 0, both[0], both[1])[None], got)
    assert int((both[0] != 0).sum()) == 1203 and int((both[1] != 0).sum()) == 797


# ------------------------------------------------------------------ block
@pytest.fixture(scope='module')
def block_full():
    h, w = 32, 96
    pts = refs.fixture_points(50, h, w, 700)[None]
    return pts, h, w, native(pts, None, h, w)


def empty_to_zero(t):
    return torch.where(t == 1e5, torch.zeros_like(t), t)


@pytest.mark.parametrize('block', [2, 4, 8, 16])
def test_block_equals_downsampled_full_map(block_full, margin, block):
    pts, h, w, full = block_full
    got = native(pts, None, h, w, block=block)
    assert tuple(got.shape) == (1, 1, h // block, w // block)
    assert torch.equal(got, empty_to_zero(downsample_depth_torch(full, block)))
    case, _ = margin
    mats = [case['lidar2img'], case['post_rots'], case['post_trans']]
    full2 = native(case['points'], mats, case['height'], case['width'])
    got2 = native(case['points'], mats, case['height'], case['width'], block=block)
    assert torch.equal(got2, empty_to_zero(downsample_depth_torch(full2, block)))


# ------------------------------------------------------------------ poison and capture
def test_every_element_is_written():
    h, w = 32, 96
    pts = refs.fixture_points(50, h, w, 700)[None].to(DEV)
    for block in (1, 16):
        out = torch.full((1, 1, h // block, w // block), NAN, device=DEV)
        res = lidar_depth.multiview_depth(pts, None, None, None, h, w, (LO, HI), block=block,
                                          out=out)
        assert res is out and bool(torch.isfinite(out).all())
        assert torch.equal(out.cpu(), mirror(pts.cpu(), None, h, w, block=block))
    none = torch.full((2, 0, 3), 0.0, device=DEV)
    out = torch.full((2, 1, h, w), NAN, device=DEV)
    lidar_depth.multiview_depth(none, None, None, None, h, w, (LO, HI), out=out)
    assert not bool(out.any())


def test_graph_capture_follows_the_point_buffer(margin):
    case, _ = margin
    h, w = case['height'], case['width']
    mats = [case[k].to(DEV) for k in ('lidar2img', 'post_rots', 'post_trans')]
    first = case['points']
    second = refs.margin_case(4, n=2000)['points']
    pts = first.to(DEV)
    out = torch.empty((1, 2, h // 16, w // 16), device=DEV)

    def step():
        return lidar_depth.multiview_depth(pts, *mats, h, w, (LO, HI), block=16, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                     # warm-up
    torch.cuda.current_stream().wait_stream(side)
    want_first = step().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    out.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_first)
    pts.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert not torch.equal(got, want_first)
    assert torch.equal(got, step())
    assert torch.equal(got.cpu(), empty_to_zero(downsample_depth_torch(
        native(second, mats, h, w), 16)))


def test_unsupported_inputs_are_refused():
    h, w = 16, 32
    pts = refs.fixture_points(1, h, w, 64)[None].to(DEV)
    with pytest.raises(_lib.VeonHipError):
        lidar_depth.multiview_depth(pts.double(), None, None, None, h, w, (LO, HI))
    with pytest.raises(_lib.VeonHipError):
        lidar_depth.multiview_depth(pts.expand(2, 64, 3)[:, ::2], None, None, None, h, w,
                                    (LO, HI))
    with pytest.raises(_lib.VeonHipError):          # matrices left on the host
        lidar_depth.multiview_depth(pts, *[m[:, :1] for m in exact_rig()], h, w, (LO, HI))
    with pytest.raises(_lib.VeonHipError):
        lidar_depth.multiview_depth(pts, None, None, None, h, w, (LO, HI),
                                    out=torch.empty(1, 1, h, w + 1, device=DEV))
    with pytest.raises(ValueError):
        lidar_depth.multiview_depth(pts, None, None, None, h, w, (0.0, HI))


# ------------------------------------------------------------------ loss equality
def test_block_map_gives_the_same_loss_bits():
    """2 x 64 x 96 labels: (block map, gt_scale 1) against (full map, gt_scale 16)"""
    h, w = 64, 96
    pts = torch.stack([refs.fixture_points(60, h, w, 90), refs.fixture_points(61, h, w, 90)])
    full = lidar_depth.multiview_depth(pts.to(DEV), None, None, None, h, w, (LO, HI))
    small = lidar_depth.multiview_depth(pts.to(DEV), None, None, None, h, w, (LO, HI), block=16)
    assert 0 < int((small == 0).sum()) < small.numel()
    full, small = full.reshape(1, 2, h, w), small.reshape(1, 2, h // 16, w // 16)
    g = torch.Generator().manual_seed(8)
    base = (1.0 + 40.0 * torch.rand(1, 2, h // 2, w // 2, generator=g)).to(DEV)
    res = []
    for gt, scale in ((full, 16), (small, 1)):
        depth = base.clone().requires_grad_(True)
        out = depth_loss.depth_pretrain_loss(depth, gt, 88, LO, 0.5, 8, scale)
        (0.7 * out['loss_depth_zoe'] + 1.3 * out['loss_depth_ce']).backward()
        res.append((out, depth.grad))
    for k in ('loss_depth_zoe', 'loss_depth_ce', 'depth_error'):
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert torch.equal(res[0][1], res[1][1]) and bool(res[0][1].any())


# ------------------------------------------------------------------ wiring
class _StubEstimator(nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(1.5))

    def forward(self, x):
        return {'metric_depth': 2.0 + self.scale * x[:, 0].abs() * 10.0}


def test_forward_train_renders_the_block_map(margin):
    case, _ = margin
    h, w = case['height'], case['width']
    eye = torch.eye(4).expand(1, 2, 4, 4).contiguous()
    le2g = torch.cat([case['lidar2img'], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(1, 2, 1, 4)], 2)
    img_inputs = (torch.zeros(1, 2, 3, h, w, device=DEV), None, None,
                  torch.eye(3).expand(1, 2, 3, 3).contiguous(), case['post_rots'],
                  case['post_trans'], None, eye, le2g, eye, eye)
    depth_in = torch.randn(1, 2, 3, h // 2, w // 2,
                           generator=torch.Generator().manual_seed(5)).to(DEV)
    mats = [case['lidar2img'], case['post_rots'], case['post_trans']]
    full = native(case['points'], mats, h, w).to(DEV)
    res = []
    for kw in (dict(gt_depth=full), dict(points=case['points']),
               dict(points=[case['points'][0].to(DEV)])):
        model = VeonDepthPretrain(
            _StubEstimator(),
            build_neck(dict(type='LSSViewTransformerRaw',
                            grid_config={'x': [-10.0, 10.0, 1.0], 'y': [-10.0, 10.0, 1.0],
                                         'z': [-1.0, 3.0, 1.0], 'depth': list(refs.GRID)},
                            input_size=(h, w), out_channels=8, collapse_z=False)),
            hip_train=True).to(DEV)
        seen = {}
        inner = model.img_view_transformer.depth_pretrain_loss

        def recorder(depth, gt_depth, sp, sg, inner=inner, seen=seen):
            seen['gt'], seen['sg'] = tuple(gt_depth.shape), sg
            return inner(depth, gt_depth, sp, sg)
        model.img_view_transformer.depth_pretrain_loss = recorder
        n0 = _lib.CALLS.get(ENTRY, 0)
        losses = model.forward_train(img_inputs, depth_in, **kw)
        sum(losses.values()).backward()
        rendered = _lib.CALLS.get(ENTRY, 0) - n0
        res.append((losses, model.depth_estimator.scale.grad.clone(),
                    model.avg_depth_error.clone(), seen, rendered))
    assert res[0][3] == dict(gt=(1, 2, h, w), sg=16) and res[0][4] == 0
    for losses, grad, err, seen, rendered in res[1:]:
        assert seen == dict(gt=(1, 2, h // 16, w // 16), sg=1) and rendered == 1
        for k in ('loss_depth_zoe', 'loss_depth_ce'):
            assert torch.equal(losses[k], res[0][0][k]), k
        assert torch.equal(grad, res[0][1]) and torch.equal(err, res[0][2])
    assert math.isfinite(float(res[0][2]))
