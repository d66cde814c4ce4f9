"""Exact CPU references of the index half of the lift (csrc/lss_prepare.hip) and the
inputs of its edge tests.  A plain module: nothing device-specific, no fixtures.
tests/test_lift_refs.py pins every function here on the CPU before the GPU module
(tests/test_lift_prepare_edges_gpu.py) relies on them, and checks every builder's
promises on the very inputs that module uses.

Every promise a builder makes is an ``assert`` inside it: a case cannot silently
degenerate into one that no longer reaches the seam it was built for.

The seams (constants of csrc/lss_prepare.hip, restated here as the cases' geometry):
  * the two-kernel scan works on blocks of 1024 bins (256 threads x 4 bins) and emits
    one plan entry per 64 bins;
  * ``k_voxel_keys`` issues one histogram atomic per run of equal keys inside a
    64-lane wave of a 256-thread block over the points of one camera;
  * ``k_rank_in_bin`` stages at most 3072 sorted slots per 256-slot block.
"""
import numpy as np
import torch

from veon_amd import lss_prepare

SCAN_BLOCK = 1024   # bins per scan block
TILE = 64           # voxel ranks per plan tile
WAVE = 64
BLOCK = 256         # points per workgroup of the key kernel, slots per rank block
RANK_SPAN = 3072    # slots a rank block stages in LDS

_EMPTY = tuple(np.zeros(0, np.int32) for _ in range(5))


def _grid_t(lower, interval, gsize):
    return tuple(torch.as_tensor(np.asarray(v, dtype=np.float32)) for v in
                 (lower, interval, gsize))


# ------------------------------------------------------------------------- references
def prepare_ref(coor, lower, interval, gsize, keep=None):
    """The five int32 arrays (ranks_bev, ranks_depth, ranks_feat, interval_starts,
    interval_lengths) of ``lss_prepare.voxel_pooling_prepare_v2_torch`` on CPU fp32
    ``coor`` (B,N,D,H,W,3), as numpy; five empty arrays when nothing is kept.

    Points with ``keep == False`` and points with any non-finite coordinate are removed
    EXPLICITLY: their coordinates are replaced by a point 1000 voxels below the grid
    before the call, so the rule does not depend on how the host converts NaN to int64.
    """
    coor = torch.as_tensor(coor).detach().cpu().float().clone()
    lower, interval, gsize = _grid_t(lower, interval, gsize)
    drop = ~torch.isfinite(coor).all(-1)
    if keep is not None:
        keep = torch.as_tensor(np.asarray(keep)).bool().reshape(coor.shape[:-1])
        drop |= ~keep
    coor[drop] = lower - 1000.0 * interval
    out = lss_prepare.voxel_pooling_prepare_v2_torch(coor, lower, interval, gsize)
    if out[0] is None:
        return _EMPTY
    return tuple(t.numpy().astype(np.int32) for t in out)


def vstart_ref(ranks_bev, n_bins):
    """The dense voxel table: voxel v owns the sorted points [vstart[v], vstart[v+1])."""
    return np.searchsorted(np.asarray(ranks_bev), np.arange(n_bins + 1),
                           'left').astype(np.int32)


def plan_ref(ranks_bev, starts, B, vpb):
    """(B * vpb/64, 4) int32: for every tile of 64 consecutive voxel ranks of one batch
    element {first interval, #intervals, first point, #points} -- the contract stated
    above ``veon_bev_pool_plan`` in include/veon_hip.h.  An empty tile carries the
    interval / point count before it and zero lengths."""
    assert vpb % TILE == 0
    rb = np.asarray(ranks_bev)
    irank = rb[np.asarray(starts)] if len(starts) else np.zeros(0, rb.dtype)
    edges = np.arange(B * vpb // TILE + 1) * TILE
    iv = np.searchsorted(irank, edges, 'left')
    pt = np.searchsorted(rb, edges, 'left')
    return np.stack((iv[:-1], np.diff(iv), pt[:-1], np.diff(pt)), 1).astype(np.int32)


def twohot_keep_and_slot(win, D, H, W, K):
    """From the ``win`` words of ``veon_two_hot_window`` (host copy, any shape ending in
    2, pixels in (b,n,h,w) order): the keep mask and the compact ``ranks_depth`` value of
    every frustum point, both flat in POINT order (b,n,d,h,w), as the comment above
    ``veon_lss_prepare_cameras_twohot`` states them:
      keep  = k in [q0, q0+nq)  or  (tail kept and k outside [k0, k0+nk))
      slot  = pix*K + (1 + k - k0 if k in [k0, k0+nk) else 0)."""
    w = np.asarray(win).astype(np.int64).reshape(-1, H * W, 2)     # (BN, HW, 2)
    x, y = w[..., 0] & 0xffffffff, w[..., 1] & 0xffffffff          # the raw 32-bit words
    k0, nk = (x & 0xffff)[:, None], (x >> 16)[:, None]
    q0, nq = (y & 0xffff)[:, None], ((y >> 16) & 0x7fff)[:, None]
    tail = ((y >> 31) & 1).astype(bool)[:, None]
    k = np.arange(D).reshape(1, D, 1)
    inwin = (k >= k0) & (k < k0 + nk)
    keep = ((k >= q0) & (k < q0 + nq)) | (tail & ~inwin)           # (BN, D, HW)
    pix = np.arange(w.shape[0] * H * W).reshape(-1, 1, H * W)
    slot = pix * K + np.where(inwin, 1 + k - k0, 0)
    return keep.reshape(-1), slot.reshape(-1).astype(np.int32)


# --------------------------------------------------------------------------- axis rig
def axis_rig(xs, cams, shifts, B):
    """A rig that drives any 1-D voxel histogram through the camera entry: frustum
    (D=1, H=1, W=len(xs), 3) with ds = [1.0], ys = [0.0]; identity cam2imgs, post_rots,
    bda, zero post_trans, identity sensor2ego apart from the x translation ``shifts``
    (per camera, or (B, cams)).  Every product is by 0 or 1, so the coordinate of point
    (b, n, 0, 0, w) is exactly (fp32(xs[w] + shifts[b, n]), 0, 1).  xs must be finite.
    -> dict(frustum, sensor2ego, cam2imgs, post_rots, post_trans, bda), CPU fp32."""
    xs = np.asarray(xs, dtype=np.float32)
    assert xs.ndim == 1 and xs.size > 0 and np.isfinite(xs).all()
    sh = np.broadcast_to(np.asarray(shifts, dtype=np.float32), (B, cams))
    frustum = torch.zeros(1, 1, xs.size, 3)
    frustum[..., 0] = torch.from_numpy(xs)
    frustum[..., 2] = 1.0
    s2e = torch.eye(4).repeat(B, cams, 1, 1)
    s2e[:, :, 0, 3] = torch.from_numpy(sh.copy())
    eye3 = torch.eye(3).repeat(B, cams, 1, 1)
    return dict(frustum=frustum, sensor2ego=s2e, cam2imgs=eye3.clone(),
                post_rots=eye3.clone(), post_trans=torch.zeros(B, cams, 3),
                bda=torch.eye(3).repeat(B, 1, 1))


def axis_grid(X, lower=0.0, step=1.0):
    """The X x 1 x 1 grid of an axis rig: y = 0 and z = 1 sit in the middle of the one
    voxel of their axis.  -> (lower, interval, gsize) fp32 tensors."""
    return _grid_t([lower, -0.5, 0.5], [step, 1.0, 1.0], [X, 1, 1])


def rig_coor(rig):
    """CPU coordinates (B,N,D,H,W,3) of a rig dict: ``lss_prepare``'s own torch path
    (camera_matrices + lidar_coor_from_matrices_torch)."""
    pri, comb, trans = lss_prepare.camera_matrices(rig['sensor2ego'], rig['cam2imgs'],
                                                   rig['post_rots'])
    return lss_prepare.lidar_coor_from_matrices_torch(
        rig['frustum'], pri, rig['post_trans'], comb, trans, rig['bda'])


def _axis_case(name, xs, cams, shifts, B, X):
    """One axis-rig case + the global bin of every point (-1 = dropped), by integer
    arithmetic on the half-integer coordinates the builders use."""
    xs = np.asarray(xs, dtype=np.float64)
    sh = np.broadcast_to(np.asarray(shifts, dtype=np.float64), (B, cams))
    x = xs[None, None, :] + sh[:, :, None]                          # (B, N, W)
    assert np.all(x * 2 == np.round(x * 2)) and np.all(x != np.round(x)), \
        'builders place every point in the middle of a unit voxel'
    assert np.abs(x).max() < 2 ** 20                                # exact in fp32
    local = np.floor(x).astype(np.int64)
    bins = np.where((local >= 0) & (local < X),
                    local + np.arange(B).reshape(B, 1, 1) * X, -1)
    rig = axis_rig(xs, cams, shifts, B)
    return dict(name=name, rig=rig, grid=axis_grid(X), B=B, vpb=X,
                dims=(B, cams, 1, 1, xs.size), bins=bins.reshape(-1))


# ------------------------------------------------------------------------ face table
def _face_values(lo, step, size):
    f = np.float32
    lo, step = f(lo), f(step)
    up = f(lo + f(size) * step)
    below = f(lo - step)
    return [
        ('lower', lo, True),
        ('lower-step/2', f(lo - step / f(2)), True),       # trunc toward zero: voxel 0
        ('lower-0.49step', f(lo - f(0.49) * step), True),
        ('lower-step', below, False),                      # exactly -1
        ('nextafter(lower-step,+inf)', np.nextafter(below, f(np.inf)), None),
        ('upper', up, False),
        ('nextafter(upper,-inf)', np.nextafter(up, f(-np.inf)), None),
        ('+0.0', f(0.0), None),
        ('-0.0', f(-0.0), None),
        ('nan', f(np.nan), False),
        ('+inf', f(np.inf), False),
        ('-inf', f(-np.inf), False),
        ('+1e30', f(1e30), False),
        ('-1e30', f(-1e30), False),
        ('+3e9step', f(f(3e9) * step), False),
        ('-3e9step', f(f(-3e9) * step), False),
    ]


def float_verdict(coor, lower, interval, gsize):
    """Kept / dropped of every point by float32 numpy arithmetic alone -- the voxel
    index stays a float (np.trunc), no float -> integer conversion anywhere: finite,
    and 0 <= trunc((c - lower) / step) < size on every axis."""
    c = np.asarray(coor, dtype=np.float32)
    lo, st, sz = (np.asarray(v, dtype=np.float32) for v in (lower, interval, gsize))
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.trunc((c - lo) / st)
        return (np.isfinite(c) & (v >= 0) & (v < sz)).all(-1)


def face_table():
    """Coordinates exactly on, and one ulp beside, the voxel faces, plus every kind of
    non-finite and huge value, per axis with the other two axes in the middle of a
    voxel; one point with all three coordinates NaN; the table once per batch element
    (B = 2).  Power-of-two steps: voxel centres and faces are exact.
    -> dict(coor (2,1,1,1,P,3), grid, labels, expect): ``expect[i]`` is the stated
    verdict of point i (True kept / False dropped / None: decided by fp32 rounding,
    ``float_verdict`` is the authority)."""
    lower = np.array([-2.0, 0.0, 1.0], np.float32)
    step = np.array([0.5, 0.25, 2.0], np.float32)
    size = np.array([8, 4, 2], np.float32)                 # 64 voxels: one plan tile
    mid = lower + step * np.array([3.5, 1.5, 1.5], np.float32)
    rows, labels, expect = [], [], []
    for a in range(3):
        for name, v, verdict in _face_values(lower[a], step[a], size[a]):
            p = mid.copy()
            p[a] = v
            rows.append(p)
            labels.append('xyz'[a] + ':' + name)
            expect.append(verdict)
    rows.append(np.full(3, np.nan, np.float32))
    labels.append('all:nan')
    expect.append(False)
    pts = np.stack(rows).astype(np.float32)
    coor = np.stack((pts, pts)).reshape(2, 1, 1, 1, len(rows), 3)
    grid = _grid_t(lower, step, size)
    kept = float_verdict(pts, lower, step, size)
    for i, e in enumerate(expect):
        assert e is None or bool(kept[i]) == e, labels[i]
    for a in range(3):
        on_axis = np.array([l.startswith('xyz'[a] + ':') for l in labels])
        assert kept[on_axis].any() and (~kept[on_axis]).any(), a
    # -0.0 is kept on every axis (the reference's run kept it); NaN, inf, 1e30 never
    assert all(kept[labels.index(a + ':-0.0')] for a in 'xyz')
    assert float_verdict(mid[None], lower, step, size).all()
    return dict(coor=torch.from_numpy(coor), grid=grid, labels=labels * 2,
                expect=expect * 2, B=2, vpb=64)


# ------------------------------------------------------------------------ scan seams
SCAN_GRIDS = [(1, 64), (1, 960), (1, 1024), (1, 1088), (1, 2048), (1, 2112), (1, 3136),
              (2, 1088), (1, 15), (2, 189)]


def scan_cases(B, X):
    """Axis-rig cases of the grid X x 1 x 1 with B batch elements: occupancy patterns
    aimed at the 1024-bin seams of the two-kernel scan, the last bin and ``vstart[n]``,
    and a batch boundary inside a scan block (B = 2: batch element 1 is shifted by 64
    voxels, so its occupancy differs and its top bins fall off the grid)."""
    n_bins = B * X
    shifts = np.zeros((B, 1)) if B == 1 else np.array([[0.0], [64.0]])
    out = []

    def add(name, bins_local, extra=()):
        # extra: local voxel positions outside the grid (dropped points between kept ones)
        xs = np.array(list(bins_local) + list(extra), dtype=np.float64) + 0.5
        c = _axis_case('%dx%d-%s' % (B, X, name), xs, 1, shifts, B, X)
        c['n_bins'] = n_bins
        out.append(c)
        return c

    far = [-500, X + 500, X + 507, -400]                  # dropped under either shift
    c = add('bin0', [0, 0, 0], far[:1])
    assert set(c['bins'][c['bins'] >= 0]) == ({0} if B == 1 else {0, X + 64})
    c = add('last', [X - 1, X - 1], far[:2])
    assert set(c['bins'][c['bins'] >= 0]) == {X - 1}      # batch 1: shifted off the grid
    if n_bins > SCAN_BLOCK:
        s = SCAN_BLOCK
        c = add('seam', [s, s - 1, s - 1, s, s], far[:1])
        assert {s - 1, s} <= set(c['bins'])
    c = add('once', list(range(X - 1, -1, -1)))            # descending: the sort works
    kept = c['bins'][c['bins'] >= 0]
    assert np.unique(kept).size == kept.size
    assert kept.size == (X if B == 1 else 2 * X - 64) and n_bins - 1 in kept
    c = add('second', list(range(0, X, 2)) + list(range(0, X, 2)))
    kept = c['bins'][c['bins'] >= 0]
    assert (kept[kept < X] % 2 == 0).all() and np.bincount(kept).max() == 2
    c = add('none', [], far)
    assert (c['bins'] < 0).all()
    if B == 2:
        # the batch boundary lies inside a scan block and both sides of it are occupied
        assert X % SCAN_BLOCK != 0 and X // SCAN_BLOCK == (X + 64) // SCAN_BLOCK
        once = out[-3]['bins']
        assert X - 1 in once and X + 64 in once
    return out


# ------------------------------------------------------------- wave-aggregated atomics
def run_cases():
    """Two cameras, two batch elements, W = 700 points per camera (700 % 256 = 188,
    700 % 64 = 60: tail lanes exist) on a 64 x 1 x 1 grid.  Along w: runs of one voxel of
    lengths 1, 2, 63, 64, 65, 200 that cross lane-64 and lane-256 boundaries, runs broken
    by one dropped point, a dropped run between two runs of the same voxel, a voxel that
    comes back later.  The cameras are shifted against each other, so every voxel
    receives runs from several workgroups.
    -> dict(rig, grid, coor, coor_nan, ...): ``coor_nan`` = the same coordinates with
    every second dropped point made NaN (for the coordinate entry)."""
    DROP = -100
    segs = [(25, 1), (26, 2), (27, 63), (28, 64), (29, 65), (30, 200),
            (31, 25), (DROP, 1), (31, 39),                    # a run broken by one point
            (32, 30), (DROP, 30), (32, 30),                   # a dropped run inside a voxel
            (23, 63), (27, 64),                               # lower voxel; voxel 27 again
            (33, 13), (DROP, 1), (33, 9)]
    vox = np.concatenate([np.full(n, v) for v, n in segs])
    W = 700
    assert vox.size == W and W % BLOCK == 188 and W % WAVE == 60
    lens = {n for v, n in segs if v != DROP}
    assert {1, 2, 63, 64, 65, 200} <= lens
    start = np.cumsum([0] + [n for _, n in segs])
    crosses = lambda m: [(a, b) for (v, n), a, b in zip(segs, start[:-1], start[1:])  # noqa: E731
                         if v != DROP and a // m != (b - 1) // m]
    assert len(crosses(WAVE)) >= 6 and len(crosses(BLOCK)) >= 1
    # the dropped run straddles a workgroup boundary; the 64-run is not wave-aligned
    d0 = int(start[10])
    assert d0 // BLOCK != (d0 + 29) // BLOCK and start[3] % WAVE != 0
    B, N, X = 2, 2, 64
    shifts = np.array([[0.0, 2.0], [1.0, -3.0]])
    c = _axis_case('runs', vox + 0.5, N, shifts, B, X)
    bins = c['bins'].reshape(B, N, W)
    assert (bins[vox[None, None].repeat(B, 0).repeat(N, 1) == DROP] < 0).all()
    assert (bins[:, :, vox != DROP] >= 0).all()
    # a voxel is fed by more than one camera
    assert np.intersect1d(bins[0, 0], bins[0, 1]).size > 3
    coor = rig_coor(c['rig'])
    assert torch.equal(coor[..., 0].reshape(B, N, W),
                       torch.from_numpy((vox[None, None] + 0.5 + shifts[:, :, None])
                                        .astype(np.float32)))
    assert bool((coor[..., 1] == 0).all()) and bool((coor[..., 2] == 1).all())
    coor_nan = coor.clone()
    dropped = np.flatnonzero(c['bins'] < 0)
    flat = coor_nan.view(-1, 3)
    flat[torch.from_numpy(dropped[::2]), 0] = float('nan')
    flat[torch.from_numpy(dropped[1::4]), 2] = float('nan')
    c.update(coor=coor, coor_nan=coor_nan, n_bins=B * X)
    return c


# ------------------------------------------------------------------ long bins (rank pass)
LONG_BINS = [255, 256, 257, 3071, 3072, 3073, 4000]


def long_bin_cases(L):
    """Sorted layout: a 100-point voxel, ONE voxel of L points, 300 single-point voxels
    (grid 320 x 1 x 1, one batch element, 4 cameras).  Which point index falls into
    which voxel is a seeded random permutation over all cameras, so the arrival order in
    a voxel is not index order and the rank pass has to establish it.
    -> dict(coor (1,4,1,1,W,3), grid, L, ...)."""
    N, X = 4, 320
    A, LONG, FIRST_SINGLE, SINGLES = 2, 3, 4, 300
    n_kept = 100 + L + SINGLES
    W = -(-(n_kept + 37) // N)                          # some dropped points as well
    P = N * W
    vox = np.full(P, -7, np.int64)
    perm = np.random.RandomState(1234 + L).permutation(P)
    vox[perm[:100]] = A
    vox[perm[100:100 + L]] = LONG
    vox[perm[100 + L:n_kept]] = FIRST_SINGLE + np.arange(SINGLES)
    long_pts = np.flatnonzero(vox == LONG)
    assert long_pts.size == L
    assert np.unique(long_pts // W).size == N             # spread over all cameras
    assert (np.diff(perm[100:100 + L]) < 0).any()         # not handed out in index order
    coor = np.zeros((P, 3), np.float32)
    coor[:, 0] = vox + 0.5
    coor[:, 2] = 1.0
    grid = axis_grid(X)
    rb, rd, rf, st, ln = prepare_ref(coor.reshape(1, N, 1, 1, W, 3), *grid)
    assert ln.max() == L and ln[1] == L and ln[0] == 100 and (ln[2:] == 1).all()
    assert rb.size == n_kept and st.size == 2 + SINGLES
    lo, end = 0, 100 + L                                  # block 0 starts in voxel A
    if L >= RANK_SPAN:
        # the long voxel overruns the staged span of the block it starts in, and the
        # first single-point voxels share a 256-slot block with its end
        assert int(st[1]) // BLOCK == 0 and end > lo + RANK_SPAN
        assert end % BLOCK != 0 and (end - 1) // BLOCK == end // BLOCK
    return dict(name='long%d' % L, coor=torch.from_numpy(coor.reshape(1, N, 1, 1, W, 3)),
                grid=grid, L=L, B=1, vpb=X, n_bins=X)
