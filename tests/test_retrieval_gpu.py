"""GPU checks of the native point retrieval (csrc/occ_retrieval.hip via
veon_amd.retrieval.retrieve_points): the kernel against the reference sequence
(trilinear upsample, gather, F.cosine_similarity; san_in_veon_temporal.py:195-200,
268-273) restated in fp64 on the SAME stored operands (the half rows upcast), its
edge cases, determinism and graph capture, and the path level against the reference
chain's low-resolution features of tests/golden/path_tiny.npz."""
import pytest
import torch
import torch.nn.functional as F

from veon_amd import _lib, conv3d_ops, half
from veon_amd.retrieval import average_precision, retrieve_points

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL = 2e-5     # fp32 accumulation of C <= 768 products, against fp64


def grid_points(occ, n, seed):
    """all 8 grid corners, points on all 6 faces, random points, 3 duplicates"""
    Z, Y, X = occ
    g = torch.Generator().manual_seed(seed)
    pts = [(x, y, z) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    face = torch.stack([torch.randint(0, X, (64,), generator=g),
                        torch.randint(0, Y, (64,), generator=g),
                        torch.randint(0, Z, (64,), generator=g)], 1)
    for axis, size in enumerate((X, Y, Z)):
        for v in (0, size - 1):
            f = face.clone()
            f[:, axis] = v
            pts += [tuple(int(a) for a in r) for r in f]
    rnd = torch.stack([torch.randint(0, X, (n,), generator=g),
                       torch.randint(0, Y, (n,), generator=g),
                       torch.randint(0, Z, (n,), generator=g)], 1)
    pts += [tuple(int(a) for a in r) for r in rnd]
    pts += pts[8:11]
    return torch.tensor(pts, dtype=torch.int32)


def oracle(feat5, bin5, pts, emb, occ, batch=0):
    """The reference sequence in fp64 on the device: (score (Q,P), bin_prob (P))."""
    x, y, z = pts.long().to(feat5.device).T
    f_up = F.interpolate(feat5[batch:batch + 1].double(), tuple(occ), mode='trilinear',
                         align_corners=False)[0]
    f = f_up[:, z, y, x]
    del f_up
    e = emb.double().to(feat5.device)
    score = (e @ f) / (f.norm(dim=0).clamp_min(1e-8)[None] * e.norm(dim=1).clamp_min(1e-8)[:, None])
    prob = None
    if bin5 is not None:
        b_up = F.interpolate(bin5[batch:batch + 1].double(), tuple(occ), mode='trilinear',
                             align_corners=False)[0]
        prob = torch.softmax(b_up[:, z, y, x], 0)[0]
    return score, prob


def half_volume(B, C, low, seed, cv=None):
    """a PaddedVolume of sem-head-like values (sigmoid - 0.5) and its stored operand
    as (B, C, z, y, x) fp32 (the half values upcast exactly)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.sigmoid(2 * torch.randn((B, cv or C) + tuple(low), generator=g)) - 0.5
    vol = conv3d_ops.pack(x.to(DEV))
    stored = vol.interior().permute(0, 4, 1, 2, 3)[:, :C].float()
    return vol, stored


def bin_logits(B, low, seed):
    g = torch.Generator().manual_seed(seed)
    return (3 * torch.randn((B, 2) + tuple(low), generator=g)).to(DEV)


def prompts(Q, C, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-3, 2, Q)[:, None] if Q > 1 else torch.ones(1, 1)
    return (torch.randn(Q, C, generator=g) * scale).to(DEV)


def check(got, want, atol=ATOL):
    s, p = got
    rs, rp = want
    err = (s.double() - rs).abs().max().item()
    assert err <= atol, err
    if rp is not None:
        errp = (p.double() - rp).abs().max().item()
        assert errp <= atol, errp
    return err


@torch.no_grad()
def test_kernel_veonb_shape_vs_fp64_sequence():
    low, occ, C = (8, 100, 100), (16, 200, 200), 512
    vol, stored = half_volume(1, C, low, 0)
    binl = bin_logits(1, low, 1)
    pts = grid_points(occ, 40000, 2).to(DEV)
    n0 = _lib.CALLS.get('veon_occ_retrieve', 0)
    for Q in (1, 17, 64):
        emb = prompts(Q, C, Q)
        got = retrieve_points(vol, binl, pts, emb, occ)
        err = check(got, oracle(stored, binl, pts, emb, occ))
        print('VEON-B Q=%d: max |score - fp64| %.2e' % (Q, err))
    assert _lib.CALLS['veon_occ_retrieve'] == n0 + 3     # the native op ran


@torch.no_grad()
@pytest.mark.parametrize('low,occ', [((3, 7, 5), (6, 14, 10)), ((2, 5, 9), (5, 11, 20))])
@pytest.mark.parametrize('C,cv', [(512, None), (768, None), (24, None), (20, 24)])
def test_kernel_odd_shapes(low, occ, C, cv):
    """vector path (C % 8 == 0) and the scalar tail (C = 20 of 24-channel rows)"""
    vol, stored = half_volume(1, C, low, C, cv)
    binl = bin_logits(1, low, 3)
    pts = grid_points(occ, 300, 4).to(DEV)
    emb = prompts(5, C, 6)
    check(retrieve_points(vol, binl, pts, emb, occ), oracle(stored, binl, pts, emb, occ))


@torch.no_grad()
def test_kernel_fp32_strided_and_batch():
    low, occ, C = (3, 7, 5), (6, 14, 10), 64
    g = torch.Generator().manual_seed(7)
    cl = torch.randn((2,) + low + (C,), generator=g).to(DEV)      # channels-last fp32
    feats = [cl.permute(0, 4, 1, 2, 3),
             torch.randn((2, 2 * C) + low, generator=g).to(DEV)[:, ::2],   # strided channels
             torch.randn((2, C, 9, 9, 9), generator=g).to(DEV)[:, :, 1:4, 1:8, 2:7]]
    binl = torch.randn((2, 4) + low, generator=g).to(DEV)[:, 1:3]       # strided bin
    pts = grid_points(occ, 300, 8).to(DEV)
    emb = prompts(3, C, 9)
    for f in feats:
        for batch in (0, 1):
            check(retrieve_points(f, binl, pts, emb, occ, batch),
                  oracle(f, binl, pts, emb, occ, batch))
    # the half rows, B = 2, batch = 1
    vol, stored = half_volume(2, 512, low, 10)
    emb = prompts(2, 512, 11)
    check(retrieve_points(vol, binl, pts, emb, occ, batch=1),
          oracle(stored, binl, pts, emb, occ, batch=1))
    s, p = retrieve_points(vol, None, pts, emb, occ, batch=1)
    assert p is None


@torch.no_grad()
def test_kernel_fp16_flavour():
    with half.use('fp16'):
        for low, occ, C in (((8, 100, 100), (16, 200, 200), 512), ((2, 5, 9), (5, 11, 20), 768),
                            ((3, 7, 5), (6, 14, 10), 24)):
            vol, stored = half_volume(1, C, low, C + 1)
            assert vol.rows.dtype == torch.float16
            binl = bin_logits(1, low, 12)
            pts = grid_points(occ, 5000, 13).to(DEV)
            for Q in (1, 17):
                emb = prompts(Q, C, 14)
                check(retrieve_points(vol, binl, pts, emb, occ),
                      oracle(stored, binl, pts, emb, occ))


@torch.no_grad()
def test_out_of_range_nan_others_bit_identical_and_deterministic():
    low, occ, C = (8, 100, 100), (16, 200, 200), 512
    vol, _ = half_volume(1, C, low, 20)
    binl = bin_logits(1, low, 21)
    pts = grid_points(occ, 3000, 22).to(DEV)
    bad = torch.tensor([[-1, 0, 0], [200, 5, 5], [5, 200, 5], [5, 5, 16], [0, -7, 0],
                        [0, 0, -1]], dtype=torch.int32, device=DEV)
    mixed = torch.cat([pts[:1000], bad, pts[1000:]])
    emb = prompts(17, C, 23)
    s, p = retrieve_points(vol, binl, pts, emb, occ)
    s2, p2 = retrieve_points(vol, binl, mixed, emb, occ)
    assert torch.isnan(s2[:, 1000:1006]).all() and torch.isnan(p2[1000:1006]).all()
    keep = torch.ones(mixed.shape[0], dtype=torch.bool, device=DEV)
    keep[1000:1006] = False
    assert torch.equal(s2[:, keep], s) and torch.equal(p2[keep], p)
    assert torch.isfinite(s).all() and torch.isfinite(p).all()
    # two launches: bit-identical
    s3, p3 = retrieve_points(vol, binl, pts, emb, occ)
    assert torch.equal(s3, s) and torch.equal(p3, p)


@torch.no_grad()
def test_bad_arguments_refused():
    low, occ = (2, 5, 9), (5, 11, 20)
    vol, _ = half_volume(1, 24, low, 30)
    pts = grid_points(occ, 10, 31).to(DEV)
    with pytest.raises(ValueError):      # more channels than the rows hold
        retrieve_points(vol, None, pts, prompts(1, 32, 0), occ)
    with pytest.raises(_lib.VeonHipError):   # Q = 0: the C ABI refuses it (status 1)
        retrieve_points(vol, None, pts, torch.zeros(0, 24, device=DEV), occ)
    with pytest.raises(_lib.VeonHipError):   # batch outside [0, B): the C ABI as well
        import ctypes
        s5 = ctypes.c_int64 * 5
        emb = prompts(1, 24, 0)
        st = _lib.lib().veon_occ_retrieve(
            _lib.ptr(vol.rows), 1, ctypes.cast(s5(24, 1, 24, 24, 24), ctypes.c_void_p), 24,
            None, None, 1, 2, 5, 9, 5, 11, 20, _lib.ptr(pts), pts.shape[0], 1, _lib.ptr(emb),
            1, _lib.ptr(emb), _lib.ptr(emb), None, None)
        _lib.check(st, 'veon_occ_retrieve')


@torch.no_grad()
def test_graph_capture_of_retrieve_equals_eager():
    from veon_amd.graphs import GraphedCallable
    low, occ, C = (8, 100, 100), (16, 200, 200), 512
    vol, _ = half_volume(1, C, low, 40)
    binl = bin_logits(1, low, 41)
    pts = grid_points(occ, 20000, 42).to(DEV)
    emb = prompts(17, C, 43)
    graphed = GraphedCallable(lambda p, e: retrieve_points(vol, binl, p, e, occ), (pts, emb))
    pts2 = grid_points(occ, 20000, 44).to(DEV)
    emb2 = prompts(17, C, 45)
    gs, gp = graphed(pts2, emb2)
    es, ep = retrieve_points(vol, binl, pts2, emb2, occ)
    assert torch.equal(gs, es) and torch.equal(gp, ep)


# ---------------------------------------------------------------- path level

def _native_path():
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=True)
    return g, net, _inputs(g, DEV)


@torch.no_grad()
@pytest.mark.parametrize('flavour', ['bf16', 'fp16'])
def test_path_scores_match_reference_chain(flavour):
    """Scores from forward(return_features=True) + retrieve against the same sequence
    on the reference chain's own low-resolution features (feat_occ_lowres /
    bin_occ_lowres of path_tiny).

    Bound.  For unit e, |cos(f, e) - cos(f', e)| <= |f/|f| - f'/|f'|| <= 2 |f - f'| / |f|.
    The native features differ from the reference's by (i) their storage rounding,
    relative u = 2^-8 (bf16) / 2^-11 (fp16) per element, and (ii) the path's error
    upstream of the head, which tests/test_path_golden.py bounds at 6e-3 relative L2
    on the class logits (a per-voxel linear map of these features).  The interpolation
    is a convex combination, so neither grows.  Per point: 2 (u + 6e-3) on the RMS
    over the points; single points with a small |f| may exceed it, so the maximum is
    held to 4x that.  The occupancy probability is a 1-Lipschitz function of the
    difference of the two logits (softmax slope <= 1/4 per logit): the bin_occ bound
    of test_path_golden, 5e-3 of the logit range, times 2 x 1/4 -> range * 2.5e-3."""
    with half.use(flavour):
        g, net, (images, geom, metric) = _native_path()
        out = net(images, geom, depth=metric, return_features=True)
        assert isinstance(out['feat_low'], conv3d_ops.PaddedVolume)
        occ = net.occ_size
        pts = grid_points(occ, 1500, 50).to(DEV)
        emb = prompts(4, 24, 51)
        s, p = net.retrieve(out, pts, emb)
    ref_f = torch.from_numpy(g['feat_occ_lowres']).to(DEV)
    ref_b = torch.from_numpy(g['bin_occ_lowres']).to(DEV)
    rs, rp = oracle(ref_f, ref_b, pts, emb, occ)
    u = 2.0 ** -8 if flavour == 'bf16' else 2.0 ** -11
    bound = 2 * (u + 6e-3)
    d = (s.double() - rs).abs()
    rms, mx = d.pow(2).mean().sqrt().item(), d.max().item()
    b_range = (ref_b.max() - ref_b.min()).item()
    dp = (p.double() - rp).abs().max().item()
    print('%s path_tiny retrieval: rms %.3e max %.3e (bound %.3e / %.3e); bin_prob %.3e '
          '(bound %.3e)' % (flavour, rms, mx, bound, 4 * bound, dp, 2.5e-3 * b_range))
    assert rms <= bound and mx <= 4 * bound, (rms, mx, bound)
    assert dp <= 2.5e-3 * b_range, (dp, b_range)

    # AP: labels = top decile of the reference scores (AP of the reference = 1).  Only
    # points whose reference score lies within the max deviation of the decile threshold
    # can change side; each such point can cost at most one rank among the positives,
    # so AP(native) >= 1 - 2 * ambiguous / positives.
    for q in range(emb.shape[0]):
        thr = torch.quantile(rs[q], 0.9)
        labels = (rs[q] > thr).long()
        npos = int(labels.sum())
        ambiguous = int(((rs[q] - thr).abs() <= mx).sum())
        ap_ref = average_precision(labels, rs[q])
        ap = average_precision(labels, s[q])
        assert ap_ref == pytest.approx(1.0)
        assert ap >= ap_ref - 2.0 * ambiguous / npos - 1e-12, (q, ap, ambiguous, npos)


@torch.no_grad()
def test_path_default_keys_bit_identical():
    _, net, (images, geom, metric) = _native_path()
    a = net(images, geom, depth=metric)
    a = {k: v.clone() for k, v in a.items()}
    b = net(images, geom, depth=metric, return_features=False)
    c = net(images, geom, depth=metric, return_features=True)
    assert set(a) == set(b) == {'bin_occ', 'sem_occ', 'occ_pred_cls'}
    assert set(c) == set(a) | {'feat_low', 'bin_low'}
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


@torch.no_grad()
def test_graph_captured_forward_retrieval_equals_eager():
    from veon_amd.graphs import GraphedCallable
    _, net, (images, geom, metric) = _native_path()
    occ = net.occ_size
    pts = grid_points(occ, 1500, 60).to(DEV)
    emb = prompts(3, 24, 61)
    graphed = GraphedCallable(
        lambda im: net(im, geom, depth=metric, return_features=True), (images,))
    vol = graphed.static_out['feat_low']
    storage = vol.storage.data_ptr()
    g = torch.Generator().manual_seed(62)
    for _ in range(2):
        new = images + 0.1 * torch.randn(images.shape, generator=g).to(DEV)
        out = graphed(new)
        assert out['feat_low'] is vol and vol.storage.data_ptr() == storage
        gs, gp = net.retrieve(out, pts, emb)
        gs, gp = gs.clone(), gp.clone()
        eager = net(new, geom, depth=metric, return_features=True)
        es, ep = net.retrieve(eager, pts, emb)
        assert torch.equal(gs, es) and torch.equal(gp, ep)
