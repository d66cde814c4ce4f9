"""Inputs and an fp64 oracle for the LiDAR depth render (veon_amd/lidar_depth.py,
csrc/lidar_depth.hip).

``fixture_points``   the seeded image points of tests/golden/lidar_depth_tiny.npz
                     (tools/gen_golden_lidar_depth.py): uniform over the map plus a
                     10-pixel margin all round, depth uniform in [0, 60).
``tie_pixels``       the pixels at which the reference's result is not defined: two kept
                     points of different depth share the smallest fp32 sort key
                     ``rank + depth / 100`` (loading.py:750-751), so an unstable argsort
                     chooses between them.
``oracle``           projection, rounding, filter and minimum in fp64 on the fp32 inputs,
                     with each pair's distance to the nearest decision seam and the
                     rounding bound of its depth.
``margin_case``      points back-projected in fp64 through a two-camera rig so that, after
                     rounding to fp32, every (point, camera) pair keeps 0.05 pixels to the
                     nearest rounding seam and 0.005 m to both range ends, or falls out by
                     as much.  An fp32 projection errs by a few 2^-24 x |u|, about 4e-4
                     pixels at |u| <= 1600, and cannot cross that margin: fp32 and fp64
                     must occupy the same pixels.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
GRID = (1.0, 45.0, 0.5)
SEAM_MARGIN, RANGE_MARGIN = 0.05, 0.005
FIXTURES = {'a': dict(seed=11, height=32, width=88, n=4000),
            'b': dict(seed=12, height=512, width=1408, n=20000)}


def fixture_points(seed, height, width, n):
    """-> (n, 3) fp32 image points (u, v, d)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, 3, generator=g, dtype=torch.float64)
    scale = torch.tensor([width + 20.0, height + 20.0, 60.0], dtype=torch.float64)
    shift = torch.tensor([-10.0, -10.0, 0.0], dtype=torch.float64)
    return (r * scale + shift).to(torch.float32)


def tie_pixels(points, height, width, lo, hi, downsample=1):
    """points (P, 3) fp32 image points -> (tie (H, W) bool, {flat pixel: sorted tied
    depths}, occupied (H, W) bool, multi (H, W) bool: two or more kept points), with the
    reference's own fp32 arithmetic for the key."""
    height, width = height // downsample, width // downsample
    coor = torch.round(points[:, :2] / downsample)
    depth = points[:, 2]
    kept = (coor[:, 0] >= 0) & (coor[:, 0] < width) & (coor[:, 1] >= 0) & \
        (coor[:, 1] < height) & (depth < hi) & (depth >= lo)
    coor, depth = coor[kept], depth[kept]
    ranks = coor[:, 0] + coor[:, 1] * width                      # fp32, exact below 2^24
    key = (ranks + depth / 100.).numpy()
    pix = ranks.to(torch.long).numpy()
    d = depth.numpy()
    n = height * width
    count = np.bincount(pix, minlength=n)
    min_key = np.full(n, np.inf, np.float32)
    np.minimum.at(min_key, pix, key)
    first = key == min_key[pix]
    d_lo, d_hi = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
    np.minimum.at(d_lo, pix[first], d[first])
    np.maximum.at(d_hi, pix[first], d[first])
    tie = d_hi > d_lo
    tied = {int(p): sorted(set(d[first & (pix == p)].tolist())) for p in np.nonzero(tie)[0]}
    shape = (height, width)
    return (torch.from_numpy(tie.reshape(shape)), tied,
            torch.from_numpy((count > 0).reshape(shape)),
            torch.from_numpy((count > 1).reshape(shape)))


def oracle(points, lidar2img, post_rots, post_trans, height, width, lo, hi, downsample=1):
    """fp64 on the given (fp32) inputs.  points (B, P, >=3), lidar2img (B, N, 3, 4),
    post_rots (B, N, 3, 3), post_trans (B, N, 3) -> dict(
      depth (B, N, H, W) fp64: the smallest kept depth, 0 where none;
      bound (B, N, H, W): the largest rounding bound 8 u sum |terms| among the pixel's kept
        points, for the dot product that forms the depth (the q.z row's four terms scaled
        by |post_rot[2][2]|, the two other post_rot products and post_tran[2]);
      robust (B, N, P) bool: the pair keeps SEAM_MARGIN pixels to every rounding seam and
        RANGE_MARGIN metres to both range ends, or is out of the image or the range by as
        much;
      kept (B, N, P) bool)."""
    H, W = height // downsample, width // downsample
    p = points[..., :3].double()[:, None, :, None, :]                 # B 1 P 1 3
    M = lidar2img.double()[:, :, None]                                # B N 1 3 4
    R = post_rots.double()[:, :, None]                                # B N 1 3 3
    T = post_trans.double()[:, :, None]                               # B N 1 3
    q = (M[..., :3] * p).sum(-1) + M[..., 3]                          # B N P 3
    abs_qz = (M[..., 2, :3].abs() * p[..., 0, :].abs()).sum(-1) + M[..., 2, 3].abs()
    v = torch.stack([q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], q[..., 2]], -1)
    r = (R * v[..., None, :]).sum(-1) + T
    x, y, d = r[..., 0] / downsample, r[..., 1] / downsample, r[..., 2]
    bound = 8 * U * (R[..., 2, 2].abs() * abs_qz + (R[..., 2, 0] * v[..., 0]).abs()
                     + (R[..., 2, 1] * v[..., 1]).abs() + T[..., 2].abs())
    cx, cy = torch.round(x), torch.round(y)
    kept = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (d < hi) & (d >= lo)

    def seam(t):
        return ((t - torch.floor(t)) - 0.5).abs()

    def inside(t, n):
        return (t >= -0.5 + SEAM_MARGIN) & (t <= n - 0.5 - SEAM_MARGIN)

    def outside(t, n):
        return ~((t > -0.5 - SEAM_MARGIN) & (t < n - 0.5 + SEAM_MARGIN))     # NaN: outside
    d_in = (d >= lo + RANGE_MARGIN) & (d <= hi - RANGE_MARGIN)
    d_out = (d <= lo - RANGE_MARGIN) | (d >= hi + RANGE_MARGIN)
    robust = d_out | (torch.isfinite(x) & outside(x, W)) | (torch.isfinite(y) & outside(y, H)) \
        | (inside(x, W) & inside(y, H) & d_in & (seam(x) >= SEAM_MARGIN)
           & (seam(y) >= SEAM_MARGIN))
    B, N, P = kept.shape
    cell = torch.where(kept, cy * W + cx, torch.zeros_like(cx)).long().reshape(B * N, P)
    inf = torch.full_like(d, float('inf')).reshape(B * N, P)
    depth = torch.full((B * N, H * W), float('inf'), dtype=torch.float64)
    depth.scatter_reduce_(1, cell, torch.where(kept.reshape(B * N, P), d.reshape(B * N, P), inf),
                          'amin')
    bmap = torch.zeros((B * N, H * W), dtype=torch.float64)
    bmap.scatter_reduce_(1, cell, torch.where(kept, bound, torch.zeros_like(bound))
                         .reshape(B * N, P), 'amax')
    depth = torch.where(torch.isinf(depth), torch.zeros_like(depth), depth)
    return dict(depth=depth.reshape(B, N, H, W), bound=bmap.reshape(B, N, H, W), robust=robust,
                kept=kept)


def margin_rig(height, width):
    """Two cameras back to back (yaw 20 and 200 degrees), about 0.5 m apart (what one
    sees is behind the other), intrinsics for a ``width``-wide image before the post
    transform; post_rot = 0.88 x a 5-degree in-plane rotation, a post_tran; all fp64 ->
    (lidar2img (2, 4, 4), post_rots (2, 3, 3), post_trans (2, 3))."""
    f = 0.9 * width
    a = math.radians(5.0)
    l2i = torch.zeros(2, 4, 4, dtype=torch.float64)
    for n, (yaw, tx) in enumerate(((20.0, 0.25), (200.0, -0.25))):
        c, s = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
        cam2lidar = torch.eye(4, dtype=torch.float64)
        # columns: camera x (right), y (down), z (forward) in the lidar frame (x fwd, y left)
        cam2lidar[:3, :3] = torch.tensor([[s, 0.0, c], [-c, 0.0, s], [0.0, -1.0, 0.0]],
                                         dtype=torch.float64)
        cam2lidar[:3, 3] = torch.tensor([tx, 0.03 * (n + 1), 0.4], dtype=torch.float64)
        k = torch.eye(4, dtype=torch.float64)
        k[:3, :3] = torch.tensor([[f, 0.0, 0.57 * width + n], [0.0, f, 0.31 * width - n],
                                  [0.0, 0.0, 1.0]], dtype=torch.float64)
        l2i[n] = k @ torch.inverse(cam2lidar)
    rot = torch.eye(3, dtype=torch.float64)
    rot[:2, :2] = 0.88 * torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]],
                                      dtype=torch.float64)
    post_rots = torch.stack([rot, rot])
    post_trans = torch.tensor([[-3.5, -7.25, 0.0], [2.75, -5.5, 0.0]], dtype=torch.float64)
    return l2i, post_rots, post_trans


def margin_case(seed, n=2000, height=128, width=352, grid=GRID):
    """-> dict(points (1, n, 3), lidar2img (1, 2, 3, 4), post_rots (1, 2, 3, 3), post_trans
    (1, 2, 3), all fp32; height, width, lo, hi).  Every point is aimed at a pixel of its
    own of one camera (no two points share a pixel), at most 0.4 pixels from its centre,
    with a depth at least 0.01 m inside the range; the asserts below verify, in fp64 on the
    rounded inputs, the margins the module docstring states."""
    lo, hi = float(grid[0]), float(grid[1])
    g = torch.Generator().manual_seed(seed)
    l2i, post_rots, post_trans = margin_rig(height, width)
    per_cam = [n - n // 2, n // 2]
    pts = []
    for c in range(2):
        m = per_cam[c]
        pix = torch.randperm(height * width, generator=g)[:m]
        off = (torch.rand(m, 2, generator=g, dtype=torch.float64) * 2 - 1) * 0.4
        uv = torch.stack([(pix % width).double(), (pix // width).double()], 1) + off
        d = lo + 0.01 + torch.rand(m, generator=g, dtype=torch.float64) * (hi - lo - 0.02)
        # undo the post transform (its third row and column are the identity's), then
        # the perspective division, then lidar2img
        uv = (uv - post_trans[c, :2]) @ torch.inverse(post_rots[c, :2, :2]).T
        hom = torch.cat([uv * d[:, None], d[:, None], torch.ones(m, 1, dtype=torch.float64)], 1)
        pts.append((hom @ torch.inverse(l2i[c]).T)[:, :3])
    points = torch.cat(pts)[torch.randperm(n, generator=g)]
    case = dict(points=points.to(torch.float32)[None].contiguous(),
                lidar2img=l2i[None, :, :3, :].to(torch.float32).contiguous(),
                post_rots=post_rots[None].to(torch.float32).contiguous(),
                post_trans=post_trans[None].to(torch.float32).contiguous(),
                height=height, width=width, lo=lo, hi=hi)
    ora = oracle(case['points'], case['lidar2img'], case['post_rots'], case['post_trans'],
                 height, width, lo, hi)
    assert bool(ora['robust'].all()), 'a pair of margin_case is within the margin of a seam'
    assert int(ora['kept'].sum()) == n and int((ora['depth'] > 0).sum()) == n, \
        'every point of margin_case is kept once, in a pixel of its own'
    return case
