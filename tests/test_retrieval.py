"""CPU checks of the open-vocabulary point retrieval (veon_amd/retrieval.py): the
torch fallback of ``retrieve_points`` against the reference sequence restated in fp64
(upsample, gather, cosine; san_in_veon_temporal.py:195-200, 268-273), the AP against
sklearn, the voxel indices against a restatement of RetrievalForPointsIndices
(datasets/pipelines/loading.py:990-1012), and the path's output keys."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from veon_amd.retrieval import (average_precision, points_to_voxel_indices,
                                pop3d_retrieval, retrieve_points)


def restated(feat, bin_low, points, emb, occ_size, batch=0):
    """The reference sequence, fp64, one point at a time for the cosine."""
    f_up = F.interpolate(feat[batch:batch + 1].double(), tuple(occ_size), mode='trilinear',
                         align_corners=False)[0]
    b_up = F.interpolate(bin_low[batch:batch + 1].double(), tuple(occ_size),
                         mode='trilinear', align_corners=False)[0]
    e = emb.double()
    P, Q = points.shape[0], e.shape[0]
    score = torch.empty(Q, P, dtype=torch.float64)
    prob = torch.empty(P, dtype=torch.float64)
    for p in range(P):
        x, y, z = (int(v) for v in points[p])
        f = f_up[:, z, y, x]
        for q in range(Q):
            score[q, p] = (f @ e[q]) / (max(f.norm().item(), 1e-8) * max(e[q].norm().item(), 1e-8))
        prob[p] = torch.softmax(b_up[:, z, y, x], 0)[0]
    return score, prob


def grid_points(occ_size, n_random, g, dup=3):
    """every corner, points on every face, random interior points, duplicates"""
    Z, Y, X = occ_size
    pts = [(x, y, z) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    for _ in range(4):
        rx, ry, rz = (int(torch.randint(0, n, (1,), generator=g)) for n in (X, Y, Z))
        pts += [(0, ry, rz), (X - 1, ry, rz), (rx, 0, rz), (rx, Y - 1, rz),
                (rx, ry, 0), (rx, ry, Z - 1)]
    for _ in range(n_random):
        pts.append(tuple(int(torch.randint(0, n, (1,), generator=g)) for n in (X, Y, Z)))
    pts += pts[:dup]
    return torch.tensor(pts, dtype=torch.int32)


@pytest.mark.parametrize('low,occ', [((2, 5, 5), (4, 10, 10)),      # ratio 2
                                     ((3, 7, 5), (6, 14, 10)),
                                     ((2, 5, 9), (5, 11, 20)),      # ratios not 2
                                     ((3, 4, 6), (7, 9, 13))])
def test_cpu_retrieve_matches_reference_sequence_fp64(low, occ):
    g = torch.Generator().manual_seed(sum(low) + sum(occ))
    B, C, Q = 2, 12, 3
    feat = torch.randn((B, C) + low, generator=g, dtype=torch.float64)
    bin_low = torch.randn((B, 2) + low, generator=g, dtype=torch.float64)
    emb = torch.randn(Q, C, generator=g, dtype=torch.float64) * torch.tensor([[1e-3], [1.0], [40.0]],
                                                                             dtype=torch.float64)
    pts = grid_points(occ, 20, g)
    for batch in (0, 1):
        s, p = retrieve_points(feat, bin_low, pts, emb, occ, batch)
        rs, rp = restated(feat, bin_low, pts, emb, occ, batch)
        assert s.shape == (Q, pts.shape[0]) and p.shape == (pts.shape[0],)
        torch.testing.assert_close(s, rs, rtol=0, atol=1e-12)
        torch.testing.assert_close(p, rp, rtol=0, atol=1e-12)
    # duplicate points score the same (torch's vectorised cosine: up to rounding)
    n = pts.shape[0]
    torch.testing.assert_close(s[:, n - 3:], s[:, :3], rtol=0, atol=1e-15)


def test_cpu_retrieve_zero_feature_scores_zero_and_outside_is_nan():
    low, occ = (2, 3, 4), (4, 6, 8)
    feat = torch.randn((1, 8) + low, dtype=torch.float64)
    feat[:, :, 1, 2, 3] = 0.0       # the top corner voxel: its upsampled feature is 0
    bin_low = torch.randn((1, 2) + low, dtype=torch.float64)
    emb = torch.randn(2, 8, dtype=torch.float64)
    pts = torch.tensor([[7, 5, 3], [0, 0, 0], [8, 0, 0], [0, -1, 0], [0, 0, 4]],
                       dtype=torch.int32)
    s, p = retrieve_points(feat, bin_low, pts, emb, occ)
    assert torch.equal(s[:, 0], torch.zeros(2, dtype=torch.float64))    # as torch gives
    ref = F.cosine_similarity(
        F.interpolate(feat, occ, mode='trilinear', align_corners=False)[0][:, 3, 5, 7][None],
        emb, dim=1)
    assert torch.equal(ref, torch.zeros(2, dtype=torch.float64))
    assert torch.isfinite(s[:, 1]).all() and torch.isfinite(p[:2]).all()
    assert torch.isnan(s[:, 2:]).all() and torch.isnan(p[2:]).all()


def test_cpu_retrieve_fp32_and_no_bin():
    low, occ = (2, 4, 4), (4, 8, 8)
    feat = torch.randn((1, 16) + low)
    emb = torch.randn(1, 16)
    pts = grid_points(occ, 10, torch.Generator().manual_seed(1))
    s, p = retrieve_points(feat, None, pts, emb, occ)
    assert p is None and s.dtype == torch.float32
    rs, _ = restated(feat, torch.zeros((1, 2) + low), pts, emb, occ)
    torch.testing.assert_close(s.double(), rs, rtol=0, atol=2e-6)
    with pytest.raises(ValueError):
        retrieve_points(feat, None, pts, torch.randn(1, 15), occ)
    with pytest.raises(ValueError):
        retrieve_points(feat, None, pts, emb, occ, batch=1)


def _ap_cases():
    rng = np.random.default_rng(0)
    yield rng.integers(0, 2, 500), rng.standard_normal(500)             # random
    yield rng.integers(0, 2, 400), rng.integers(0, 5, 400) / 4.0        # heavy ties
    y = np.zeros(300, int)
    y[17] = 1
    yield y, rng.standard_normal(300)                                   # one positive
    yield y, np.round(rng.standard_normal(300), 1)                      # one positive, ties
    yield np.ones(50, int), rng.standard_normal(50)                     # all positive
    yield np.zeros(50, int), rng.standard_normal(50)                    # no positive


def test_average_precision_equals_sklearn():
    metrics = pytest.importorskip('sklearn.metrics')
    import warnings
    for y, s in _ap_cases():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')      # sklearn warns when there is no positive
            want = metrics.average_precision_score(y, s)
        got = average_precision(torch.from_numpy(y), torch.from_numpy(s))
        assert got == pytest.approx(float(want), rel=1e-12, abs=1e-12), (got, want)
    assert average_precision(torch.zeros(10), torch.randn(10)) == 0.0


def test_pop3d_retrieval_dict():
    metrics = pytest.importorskip('sklearn.metrics')
    rng = np.random.default_rng(3)
    y, s = rng.integers(0, 2, 200), rng.standard_normal(200).astype(np.float32)
    vis = np.sort(rng.choice(200, 80, replace=False))
    out = pop3d_retrieval(torch.from_numpy(s), None, torch.from_numpy(y), vis)
    assert set(out) == {'map', 'map_visible'}
    assert out['map'] == pytest.approx(metrics.average_precision_score(y, s), rel=1e-12)
    assert out['map_visible'] == pytest.approx(
        metrics.average_precision_score(y[vis], s[vis]), rel=1e-12)


def restated_indices(points_lidar, lidar2lidarego, grid_config):
    """loading.py:990-1012 in numpy (the grid size from the grid config)."""
    pts = torch.as_tensor(points_lidar)[:, :3]
    pts = pts[:, :3].matmul(lidar2lidarego[:3, :3].T) + lidar2lidarego[:3, 3]
    xg, yg, zg = grid_config['x'], grid_config['y'], grid_config['z']
    X, Y, Z = (round((xg[1] - xg[0]) / xg[2]), round((yg[1] - yg[0]) / yg[2]),
               round((zg[1] - zg[0]) / zg[2]))
    xi = np.floor((pts[:, 0] - xg[0]) / xg[2])
    yi = np.floor((pts[:, 1] - yg[0]) / yg[2])
    zi = np.floor((pts[:, 2] - zg[0]) / zg[2])
    xi = np.where(xi > X - 1, X - 1, xi)
    yi = np.where(yi > Y - 1, Y - 1, yi)
    zi = np.where(zi > Z - 1, Z - 1, zi)
    ind = np.stack([xi, yi, zi], axis=1)
    ind = np.where(ind < 0, 0, ind)
    return np.uint(ind).astype(np.int32), (Z, Y, X)


def test_points_to_voxel_indices_matches_reference():
    grid = {'x': [-40.0, 40.0, 0.4], 'y': [-40.0, 40.0, 0.4], 'z': [-1.0, 5.4, 0.4]}
    g = torch.Generator().manual_seed(5)
    pts = torch.cat([torch.rand(2000, 4, generator=g) * torch.tensor([100.0, 100.0, 10.0, 1.0])
                     - torch.tensor([50.0, 50.0, 3.0, 0.0]),          # many outside: clamped
                     torch.tensor([[-40.0, -40.0, -1.0, 0.0], [39.99, 39.99, 5.39, 0.0]])])
    m = torch.eye(4)
    m[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    m[:3, 3] = torch.tensor([0.9, -0.2, 1.8])
    want, occ = restated_indices(pts, m, grid)
    got = points_to_voxel_indices(pts, m, grid, occ)
    assert got.dtype == torch.int32
    assert np.array_equal(got.numpy(), want)
    assert (got.min(0).values >= 0).all()
    assert (got.max(0).values <= torch.tensor([occ[2] - 1, occ[1] - 1, occ[0] - 1])).all()


def test_forward_default_keys_unchanged_on_cpu():
    from tests.test_path_golden import _build, _inputs
    from tests.conftest import load_golden
    from oracle import lss_torch
    g = load_golden('path_tiny')
    net = _build(g, 'cpu', native=False)
    vt = net.view_transformer

    def cpu_view_transform(input, depth, tran_feat):   # the lift: CPU oracle
        B, N, C, H, W = input[0].shape
        grid = (vt.grid_lower_bound, vt.grid_interval, vt.grid_size)
        cams = (input[1], input[3], input[4], input[5], input[6])
        return lss_torch.lift(vt.frustum, grid, cams, depth.view(B, N, -1, H, W),
                              tran_feat.view(B, N, C, H, W))
    vt.view_transform = cpu_view_transform
    images, geom, metric = _inputs(g, 'cpu')
    with torch.no_grad():
        out = net(images, geom, depth=metric)
        out2 = net(images, geom, depth=metric, return_features=False)
        out3 = net(images, geom, depth=metric, return_features=True)
    assert set(out) == set(out2) == {'bin_occ', 'sem_occ', 'occ_pred_cls'}
    for k in out:
        assert torch.equal(out[k], out2[k]) and torch.equal(out[k], out3[k])
    assert set(out3) == set(out) | {'feat_low', 'bin_low'}
    assert tuple(out3['feat_low'].shape) == (1, 24, 2, 10, 10)
    assert tuple(out3['bin_low'].shape) == (1, 2, 2, 10, 10)
    # the path's retrieve == the CPU op on the returned features
    pts = grid_points(net.occ_size, 30, torch.Generator().manual_seed(2))
    emb = torch.randn(2, 24)
    s, p = net.retrieve(out3, pts, emb)
    s2, p2 = retrieve_points(out3['feat_low'], out3['bin_low'], pts, emb, net.occ_size)
    assert torch.equal(s, s2) and torch.equal(p, p2)
