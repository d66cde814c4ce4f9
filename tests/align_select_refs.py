"""Helpers of the entry-selection tests (no tests here): a synthetic rig and data builder
in the style of tools/gen_golden_align_loss.py, parametrised by grid, cameras and image
size; the fp64 margin of every discrete decision of the selection per (camera, voxel)
pair; and ``protect``, which frees every voxel with a decision below its margin so that an
fp32 implementation and the fp64 oracle take the same decisions everywhere.

Margins (those of the fixture generator's ``margins``), with U = 2^-24:
    100 * 16 * U * max(H, W) px    the four image bounds, for points not robustly behind
                                   the near plane
    100 * 16 * U * depth_hi        the two depth bounds
    100 * 4 * U * max|logit|       the three top-2 gaps of the sampled logits
    100 * (C + 8) * U * |f||t|     the stage-2 top-2 gaps
    100 * (C + 8) * U              |cos - thr|
Condition, not measurement: ``protect`` may free at most 1 % of the labelled voxels of a
case (asserted on the host before anything touches a device)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
REFLECTION = [0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 14, 15, 16, 16]
PRIORITY = [1.0, 3.0, 2.5, 1.5, 4.0, 2.0, 3.5, 5.0, 1.2, 2.2, 1.0, 0.5, 0.8, 0.6, 0.7, 1.1, 0.9]
N_CLS = 17
CAP = 0.01

# name -> what make_case builds.  occ = (Z, Y, X); image = (H, W); sem = the 2-D map's size.
# Workgroups of the mark kernel hold 256 pairs and its scan takes 1024 totals per pass:
#   seam_partial  4 * 10*38*46 = 69 920 pairs = 273 * 256 + 32: the last workgroup is partial
#   seam_scan     2 * 16*100*100 = 320 000 pairs = 1 250 workgroups > 1 024: two scan passes
SPECS = {
    'seam_partial': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(20, 36), seed=0),
    'seam_scan': dict(occ=(16, 100, 100), n_cam=2, image=(20, 36), sem=(10, 18), seed=1),
    'blind_middle': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(20, 36), seed=2,
                         blind=(1,)),
    'blind_last': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(20, 36), seed=3,
                       blind=(3,)),
    'batch2': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(20, 36), seed=4, B=2),
    'stage2': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(20, 36), seed=5, C=16,
                   thr=0.5, epoch=3),
    'small_map': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(7, 11), seed=6),
    'in_place': dict(occ=(10, 38, 46), n_cam=4, image=(20, 36), sem=(9, 17), seed=7, C=16,
                     thr=0.5, epoch=3),
}


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def grid_config(occ):
    """A 20 m square around the ego vehicle in cubic voxels, z from -1 m, depth 1-12 m."""
    Zo, Yo, Xo = occ
    step = 20.0 / max(Xo, Yo)
    return {'x': [-step * Xo / 2, step * Xo / 2, step], 'y': [-step * Yo / 2, step * Yo / 2, step],
            'z': [-1.0, -1.0 + step * Zo, step], 'depth': [1.0, 12.0, 0.5]}


def make_rig(seed, B, n_cam, image, blind=()):
    """n_cam cameras looking outward, yaw 2 pi / n_cam apart with overlapping fields of
    view; the post rotation mixes depth into u and v a little (its third row and column
    are not those of the identity).  A ``blind`` camera is lifted above the grid and turned
    to look straight up: every voxel is behind it.  fp32, the reference's img_inputs order."""
    H, W = image
    r = np.random.RandomState(seed)
    base = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]])
    cam2camego = np.zeros((B, n_cam, 4, 4))
    camego2global = np.zeros((B, n_cam, 4, 4))
    lidarego2global = np.zeros((B, n_cam, 4, 4))
    intrins = np.zeros((B, n_cam, 3, 3))
    post_rots = np.zeros((B, n_cam, 3, 3))
    post_trans = np.zeros((B, n_cam, 3))
    for b in range(B):
        ego = rot(2, r.uniform(-3, 3))
        ego[:3, 3] = r.uniform(-50, 50, 3)
        for c in range(n_cam):
            yaw = c * 2 * np.pi / n_cam + r.uniform(-0.2, 0.2)
            m = rot(2, yaw) @ rot(1, r.uniform(-0.05, 0.05)) @ base
            m[:3, 3] = r.uniform(-0.5, 0.5, 3) + [0, 0, 1.0]
            if c in blind:
                m = rot(1, np.pi / 2) @ base
                m[:3, 3] = [0, 0, 10.0]
            cam2camego[b, c] = m
            drift = rot(2, r.uniform(-0.01, 0.01))
            drift[:3, 3] = r.uniform(-0.2, 0.2, 3)
            camego2global[b, c] = ego @ drift
            lidarego2global[b, c] = ego
            f = W / 2.4 + r.uniform(-0.5, 0.5)
            intrins[b, c] = [[f, 0, (W - 1) / 2 + r.uniform(-1, 1)],
                             [0, f, (H - 1) / 2 + r.uniform(-1, 1)], [0, 0, 1]]
            s = r.uniform(0.9, 1.1)
            pr = np.diag([s, s, 1.0])
            pr[0, 2], pr[1, 2] = r.uniform(-0.02, 0.02, 2)
            pr[2, 0], pr[2, 1] = r.uniform(-0.002, 0.002, 2)
            pr[2, 2] = r.uniform(0.98, 1.02)
            post_rots[b, c] = pr
            post_trans[b, c] = [r.uniform(-2, 2), r.uniform(-2, 2), r.uniform(-0.05, 0.05)]
    t = lambda a: torch.from_numpy(a.astype(np.float32))     # noqa: E731
    eye = torch.eye(4).repeat(B, n_cam, 1, 1)
    return [torch.zeros(B, n_cam, 3, H, W), eye.clone(), eye.clone(), t(intrins), t(post_rots),
            t(post_trans), torch.eye(3).repeat(B, 1, 1), eye.clone(), t(lidarego2global),
            t(cam2camego), t(camego2global)]


def group_ids():
    gid, cur = [], -1
    for i, v in enumerate(REFLECTION):
        if i == 0 or v != REFLECTION[i - 1]:
            cur += 1
        gid.append(cur)
    return torch.tensor(gid)


def top2_gap(values):
    if values.shape[0] < 2:
        return values.new_full(values.shape[1:], float('inf'))
    t = values.topk(2, dim=0).values
    return t[0] - t[1]


def group_max(values, gid):
    return torch.stack([values[gid == k].max(0).values for k in range(int(gid.max()) + 1)])


def centres64(case):
    gc = case['grid_config']
    Zo, Yo, Xo = case['occ_size']
    ax = [torch.arange(n, dtype=torch.float64) * gc[k][2] + (gc[k][0] + gc[k][2] / 2)
          for n, k in ((Xo, 'x'), (Yo, 'y'), (Zo, 'z'))]
    return torch.stack(torch.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)


def project64(rig, b, c, xyz):
    """(u, v, depth) of the voxel centres in camera c of sample b, fp64"""
    d = torch.float64
    k = torch.eye(4, dtype=d)
    k[:3, :3] = rig[3][b, c].to(d)
    m = k @ torch.inverse(rig[10][b, c].to(d) @ rig[9][b, c].to(d)) @ rig[8][b, c].to(d)
    p = xyz @ m[:3, :3].T + m[:3, 3]
    p = torch.cat([p[:, :2] / p[:, 2:3], p[:, 2:3]], 1)
    return (p @ rig[4][b, c].to(d).T + rig[5][b, c].to(d)).T


def padded_corner_samples(case):
    """Number of kept (camera, voxel) pairs of sample 0 whose bilinear footprint on the
    2-D map reaches outside it (a zero-padded corner is sampled), fp64."""
    rig, gc = case['img_inputs'], case['grid_config']
    H, W = rig[0].shape[-2:]
    hs, ws = case['sem_seg_ds'].shape[-2:]
    lab = case['voxel_semantics'].masked_fill(case['mask_camera'] == 0, 255)[0].reshape(-1).long()
    cand = (lab >= 0) & (lab < N_CLS)
    xyz, n = centres64(case), 0
    for c in range(rig[3].shape[1]):
        u, v, z = project64(rig, 0, c, xyz)
        keep = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z < gc['depth'][1]) & \
            (z >= gc['depth'][0]) & cand
        ix = (u[keep] / ((W - 1) / 2) * ws - 1) / 2
        iy = (v[keep] / ((H - 1) / 2) * hs - 1) / 2
        n += int(((ix < 0) | (ix > ws - 1) | (iy < 0) | (iy > hs - 1)).sum())
    return n


def unsafe_voxels(case, labels):
    """(B, X*Y*Z) bool: voxels with a decision below its margin in ANY camera, fp64.
    ``labels``: the masked labels (B, X, Y, Z)."""
    d = torch.float64
    rig, sem_seg, gc = case['img_inputs'], case['sem_seg_ds'], case['grid_config']
    Zo, Yo, Xo = case['occ_size']
    H, W = rig[0].shape[-2:]
    B, n_cam = rig[3].shape[:2]
    gid = group_ids()
    xyz = centres64(case)
    lo, hi = gc['depth'][0], gc['depth'][1]
    tol_px, tol_z = 100 * 16 * U * max(H, W), 100 * 16 * U * hi
    tol_l = 100 * 4 * U * float(sem_seg.abs().max())
    stage2 = case['epoch'] >= case['stage2_start']
    unsafe = torch.zeros(B, Xo * Yo * Zo, dtype=torch.bool)
    for b in range(B):
        gt_all = labels[b].reshape(-1).long()
        cand = (gt_all < N_CLS) & (gt_all >= 0)
        seen = torch.zeros_like(cand)
        for c in range(n_cam):
            u, v, z = project64(rig, b, c, xyz)
            keep = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z < hi) & (z >= lo) & cand
            front = cand & (z >= lo - tol_z)
            near = torch.stack([u.abs(), (u - (W - 1)).abs(), v.abs(), (v - (H - 1)).abs()]).min(0).values
            unsafe[b] |= front & ~(near >= tol_px)               # NaN counts as unsafe
            unsafe[b] |= cand & ~(torch.minimum((z - lo).abs(), (z - hi).abs()) >= tol_z)
            idx = keep.nonzero()[:, 0]
            if not idx.numel():
                continue
            seen |= keep
            gt = gt_all[idx]
            xy = torch.stack([u[idx] / ((W - 1) / 2) - 1, v[idx] / ((H - 1) / 2) - 1], -1)
            logit = F.grid_sample(sem_seg[b, c][None].to(d), xy[None, None], mode='bilinear',
                                  align_corners=False)[0, :, 0]
            bad = (top2_gap(logit) < tol_l) | (top2_gap(group_max(logit, gid)) < tol_l)
            in_group = gid[:, None] == gt[None]
            restr = torch.where(in_group, logit, torch.full_like(logit, float('-inf')))
            bad |= (in_group.sum(0) > 1) & (top2_gap(restr) < tol_l)
            unsafe[b, idx[bad]] = True
        if stage2 and seen.any():
            idx = seen.nonzero()[:, 0]
            C = case['feat_low'].shape[1]
            f_up = F.interpolate(case['feat_low'][b:b + 1].to(d), (Zo, Yo, Xo), mode='trilinear',
                                 align_corners=False)[0]
            f = f_up.permute(3, 2, 1, 0).reshape(-1, C)[idx]            # (x, y, z) order
            tab = case['table'].to(d)[:-1]
            dots = f @ tab.T
            scale = f.norm(dim=1, keepdim=True) * tab.norm(dim=1)[None]
            tol_d = 100 * (C + 8) * U * scale.max(1).values
            bad = (top2_gap(dots.T) < tol_d) | (top2_gap(group_max(dots.T, gid)) < tol_d)
            cos = F.cosine_similarity(f, tab[dots.argmax(1)], dim=1, eps=1e-6)
            bad |= (cos - case['high_conf_thr']).abs() < 100 * (C + 8) * U
            unsafe[b, idx[bad]] = True
    return unsafe


def protect(case):
    """The case with every unsafe voxel's label set to free (17); asserts the 1 % cap.
    -> (case, number freed, number of labelled voxels)"""
    masked = case['voxel_semantics'].masked_fill(case['mask_camera'] == 0, 255)
    unsafe = unsafe_voxels(case, masked).reshape(masked.shape)
    labelled = int(((masked.long() >= 0) & (masked.long() < N_CLS)).sum())
    freed = int((unsafe & (masked.long() >= 0) & (masked.long() < N_CLS)).sum())
    assert freed <= CAP * labelled, 'protect frees %d of %d labelled voxels' % (freed, labelled)
    out = dict(case)
    out['voxel_semantics'] = case['voxel_semantics'].masked_fill(unsafe, N_CLS)
    return out, freed, labelled


def make_case(name, label_dtype=torch.uint8, protected=True):
    """The inputs of case ``name`` of SPECS as ``tests.test_align_loss.selection`` takes
    them (fp32 on the CPU), plus ``high_conf_thr``, ``epoch``, ``stage2_start``."""
    spec = SPECS[name]
    occ, n_cam, B, C = spec['occ'], spec['n_cam'], spec.get('B', 1), spec.get('C', 4)
    Zo, Yo, Xo = occ
    g = torch.Generator().manual_seed(100 + spec['seed'])
    low = tuple(v // 2 for v in occ)
    K2 = len(REFLECTION)
    labels = torch.randint(0, N_CLS, (B, Xo, Yo, Zo), generator=g)
    kind = torch.rand((B, Xo, Yo, Zo), generator=g)
    labels[kind < 0.45] = N_CLS
    labels[kind > 0.95] = 255
    case = dict(
        feat_low=torch.randn((B, C) + low, generator=g),
        bin_low=torch.randn((B, 2) + low, generator=g),
        sem_seg_ds=2.0 * torch.randn((B, n_cam, K2) + tuple(spec['sem']), generator=g),
        table=torch.randn(K2 + 1, C, generator=g),
        voxel_semantics=labels.to(label_dtype),
        mask_camera=(torch.rand((B, Xo, Yo, Zo), generator=g) > 0.1).to(torch.uint8),
        img_inputs=make_rig(spec['seed'], B, n_cam, spec['image'], spec.get('blind', ())),
        class_reflection=list(REFLECTION), priority=list(PRIORITY), occ_size=occ,
        grid_config=grid_config(occ), high_conf_thr=spec.get('thr', 0.985),
        epoch=spec.get('epoch', 0), stage2_start=2)
    if protected:
        case, freed, labelled = protect(case)
        case['freed'], case['labelled'] = freed, labelled
    return case


def to_device(case, device, dtype=torch.float32):
    def t(a):
        if not isinstance(a, torch.Tensor):
            return a
        return (a.to(dtype) if a.is_floating_point() else a).to(device)
    out = {k: t(v) for k, v in case.items()}
    out['img_inputs'] = [t(a) for a in case['img_inputs']]
    return out
