"""fp64 CPU references of the sampling kernels (csrc/temporal.hip, csrc/occ_tail.hip)
and the inputs of their edge tests.  A plain module: nothing device-specific, no
fixtures.  tests/test_edge_refs.py pins every function here on the CPU before the GPU
modules (tests/test_temporal_edges_gpu.py, tests/test_occ_head_edges_gpu.py) rely on
them, and proves every stated cap on the very inputs those modules use.

Operands are what the kernels see: volumes rounded to the flavour's half dtype,
matrices rounded to fp32; everything after that is float64.
"""
import contextlib
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

from veon_amd import half
from veon_amd.models.semantic_net import temporal_fusion as tfm


def half_round(x):
    """Round to the flavour's half dtype, widen to float64, on the CPU."""
    return x.detach().cpu().to(half.dtype()).double()


@contextlib.contextmanager
def _float64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


# ----------------------------------------------------------------------- temporal
def warp_ref(occ, cur2glob, prev2glob, grid_config, ds):
    """``temporal_fusion.align_after_lss`` (the mirror tests/test_temporal.py pins to
    the reference's vectors) in float64 on the CPU: volume rounded to half, matrices
    rounded to fp32 and widened, voxel centres formed in float64."""
    mats = [m.detach().cpu().float().double() for m in (cur2glob, prev2glob)]
    mats = [m[:, None] if m.dim() == 3 else m for m in mats]
    with _float64_default():
        return tfm.align_after_lss(half_round(occ), mats, grid_config, ds)


def attend_ref(mod, kv, q, off):
    """``TemporalDeformable.attend`` in float64 on the CPU on half-rounded operands,
    ``tanh`` in float64; ``off`` holds the RAW offsets (surplus channels ignored).
    Heads are independent, so they run one at a time (VEON's shape would otherwise
    need a 2.6 GB sample tensor)."""
    nh, S, hd = mod.num_heads, mod.num_samples, mod.head_dim
    one = copy.copy(mod)
    one.num_heads, one.channels = 1, hd
    kv, q = half_round(kv), half_round(q)
    off = torch.tanh(half_round(off[:, :nh * S * 3]))
    outs = []
    for h in range(nh):
        outs.append(one.attend(kv[:, h * 2 * hd:(h + 1) * 2 * hd].contiguous(),
                               q[:, h * hd:(h + 1) * hd].contiguous(),
                               off[:, h * S * 3:(h + 1) * S * 3].contiguous()))
    return torch.cat(outs, dim=1)


def rot_xyz(roll=0.0, pitch=0.0, yaw=0.0):
    """float64 rotation Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    cy, sy = math.cos(yaw), math.sin(yaw)
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], np.float64)
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], np.float64)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], np.float64)
    return rz @ ry @ rx


def pose(rot, trans):
    """4x4 float64 rigid transform from a 3x3 block and a translation."""
    m = np.eye(4)
    m[:3, :3] = np.asarray(rot, np.float64)
    m[:3, 3] = np.asarray(trans, np.float64)
    return m


def affine_ref(cur2glob, prev2glob, first, step):
    """S^-1 inv(prev) cur S in numpy float64 on the fp32-rounded matrices (S: voxel
    index -> metric, diag(step) and the first centre) -> (B, 3, 4) float64."""
    cur = np.asarray(cur2glob, np.float32).astype(np.float64).reshape(-1, 4, 4)
    prev = np.asarray(prev2glob, np.float32).astype(np.float64).reshape(-1, 4, 4)
    S = np.eye(4)
    S[:3, :3] = np.diag(np.asarray(step, np.float64))
    S[:3, 3] = np.asarray(first, np.float64)
    Si = np.linalg.inv(S)
    return np.stack([(Si @ np.linalg.inv(p) @ c @ S)[:3] for c, p in zip(cur, prev)])


# --------------------------------------------------------------------- occupancy tail
EPS32 = 2.0 ** -24
VALUE_BOUND = 8 * EPS32     # x blend(|logits|): a depth-3 nest of fp32 multiplies and adds


def _axis(n_in, n_out, fused=False):
    """ATen's area_pixel_compute_source_index (align_corners=False) in float32:
    -> i0, i1 (int64) and lambda0, lambda1 (fp32 values widened to float64).
    ``fused``: scale*(dst+0.5)-0.5 as ONE fused multiply-add, which is what a build with
    floating-point contraction makes of it (ATen's CPU kernels); the library is built
    with contraction off and rounds the product first (the default here).  The two
    differ by one float32 ulp of the source index at a few indices of ratios that are
    not binary fractions."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    if fused:       # the product of two float32 is exact in float64: one rounding
        src = (np.float64(scale) * (dst + np.float32(0.5)).astype(np.float64) - 0.5)
        src = src.astype(np.float32)
    else:
        src = scale * (dst + np.float32(0.5)) - np.float32(0.5)
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return (torch.from_numpy(i0), torch.from_numpy(i1),
            torch.from_numpy(l0.astype(np.float64)), torch.from_numpy(l1.astype(np.float64)))


def _blend(x, size, fused=False):
    """The 8-corner blend of x (B,C,z,y,x float64) in float64, nested x, y, z."""
    (z0, z1, lz0, lz1), (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = (
        _axis(n, m, fused) for n, m in zip(x.shape[2:], size))
    x = lx0 * x[..., x0] + lx1 * x[..., x1]
    x = ly0[:, None] * x[..., y0, :] + ly1[:, None] * x[..., y1, :]
    return lz0[:, None, None] * x[:, :, z0] + lz1[:, None, None] * x[:, :, z1]


def corner_touch(mask_low, size):
    """bool (B,Z,Y,X): output voxels whose 8-corner set holds a marked low-resolution
    voxel (``mask_low`` (B,z,y,x) bool), whatever the weights."""
    (z0, z1, _, _), (y0, y1, _, _), (x0, x1, _, _) = (
        _axis(n, m) for n, m in zip(mask_low.shape[1:], size))
    out = torch.zeros((mask_low.shape[0],) + tuple(size), dtype=torch.bool)
    for zi in (z0, z1):
        for yi in (y0, y1):
            for xi in (x0, x1):
                out |= mask_low[:, zi][:, :, yi][:, :, :, xi]
    return out


class OccTail:
    """What ``occ_tail_ref`` returns (all float64 / int64 CPU tensors):
    sem (B,Q,Z,Y,X), bin (B,2,Z,Y,X), sem_abs / bin_abs (the same blend of |logits|),
    labels (B,X,Y,Z) by the kernel's stated rule, sem_margin (fp64 top-2 gap of the
    class logits; inf for Q = 1) and bin_margin (|o0 - o1|), both (B,Z,Y,X)."""

    def undecided(self):
        """bool (B,Z,Y,X): voxels where a label may differ from ``labels``: one of the
        margins is at most twice the value bound (the largest over the classes, resp.
        over the two occupancy logits, at that voxel)."""
        sb = VALUE_BOUND * self.sem_abs.max(dim=1).values
        bb = VALUE_BOUND * self.bin_abs.max(dim=1).values
        return (self.sem_margin <= 2 * sb) | (self.bin_margin <= 2 * bb)


def occ_tail_ref(sem_low, bin_low, size, fused_index=False):
    """The fused tail in float64 on fp32 lambdas (``_axis``; ``fused_index`` selects the
    contracted source index of ATen's CPU build instead of the library's)."""
    size = tuple(int(v) for v in size)
    sem_low, bin_low = sem_low.detach().cpu().double(), bin_low.detach().cpu().double()
    r = OccTail()
    f = fused_index
    r.sem, r.bin = _blend(sem_low, size, f), _blend(bin_low, size, f)
    r.sem_abs, r.bin_abs = _blend(sem_low.abs(), size, f), _blend(bin_low.abs(), size, f)
    Q = sem_low.shape[1]
    vmax = r.sem.max(dim=1, keepdim=True).values
    idx = torch.arange(Q).view(1, Q, 1, 1, 1)
    cls = torch.where(r.sem == vmax, idx, torch.full_like(idx, Q)).min(dim=1).values
    scored = ~torch.isnan(r.sem).any(dim=1) & torch.isfinite(vmax[:, 0])
    keep = scored & (r.bin[:, 0] > r.bin[:, 1])
    cls = torch.where(keep, cls.clamp(max=Q - 1), torch.full_like(cls, Q))
    r.labels = cls.permute(0, 3, 2, 1).contiguous()
    if Q > 1:
        top = r.sem.topk(2, dim=1).values
        r.sem_margin = top[:, 0] - top[:, 1]
    else:
        r.sem_margin = torch.full_like(r.bin[:, 0], float('inf'))
    r.bin_margin = (r.bin[:, 0] - r.bin[:, 1]).abs()
    return r


def aten_tail(sem_low, bin_low, size):
    """ATen's own op sequence (``reference()`` of tests/test_occ_head_gpu.py) in fp32 on
    the CPU: the stand-in for the kernel where the caps are proved, and the source of
    the expected labels around special values."""
    sem_low, bin_low = sem_low.detach().cpu().float(), bin_low.detach().cpu().float()
    size = tuple(int(v) for v in size)
    sem = F.interpolate(sem_low, size=size, mode='trilinear', align_corners=False)
    binv = F.interpolate(bin_low, size=size, mode='trilinear', align_corners=False)
    score, cls = torch.softmax(sem, dim=1).max(dim=1)
    keep = (score > 0.0) & (torch.softmax(binv, dim=1)[:, 0] > 0.5)
    occ = torch.where(keep, cls, torch.full_like(cls, sem.shape[1]))
    return sem, binv, occ.permute(0, 3, 2, 1).contiguous()


def plain_fp32_tail(sem_low, bin_low, size):
    """The kernel's own arithmetic in numpy float32 (no contraction anywhere: the plain
    source index, the nest az.l0*(ay.l0*(ax.l0*p + ax.l1*p) + ...) + az.l1*(...), first
    maximum, softmax(o)[0] > 0.5): the CPU stand-in that shares the source-index
    rounding of the reference the GPU tests use."""
    size = tuple(int(v) for v in size)

    def nest(x):
        x = x.detach().cpu().float().numpy()
        (z0, z1, lz0, lz1), (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = (
            tuple(t.numpy() for t in _axis(n, m)) for n, m in zip(x.shape[2:], size))
        lz0, lz1, ly0, ly1, lx0, lx1 = (v.astype(np.float32) for v in (lz0, lz1, ly0, ly1, lx0, lx1))
        x = lx0 * x[..., x0] + lx1 * x[..., x1]
        x = ly0[:, None] * x[..., y0, :] + ly1[:, None] * x[..., y1, :]
        x = lz0[:, None, None] * x[:, :, z0] + lz1[:, None, None] * x[:, :, z1]
        assert x.dtype == np.float32
        return x
    sem, binv = nest(sem_low), nest(bin_low)
    Q = sem.shape[1]
    with np.errstate(invalid='ignore', over='ignore'):
        cls = sem.argmax(axis=1)                           # first maximum
        vmax = sem.max(axis=1)
        scored = ~np.isnan(sem).any(axis=1) & np.isfinite(vmax)
        om = np.maximum(binv[:, 0], binv[:, 1])
        e0, e1 = np.exp(binv[:, 0] - om), np.exp(binv[:, 1] - om)
        keep = scored & (e0 / (e0 + e1) > np.float32(0.5))
    occ = np.where(keep, cls, Q).transpose(0, 3, 2, 1)
    return torch.from_numpy(sem), torch.from_numpy(binv), torch.from_numpy(np.ascontiguousarray(occ))


# The cases of tests/test_occ_head_edges_gpu.py: name -> (B, Q, low (z,y,x), size).
OCC_CASES = {
    'veon':      (1, 17, (8, 100, 100), (16, 200, 200)),     # the three existing triples
    'small':     (2, 5, (3, 7, 5), (6, 14, 10)),
    'ragged':    (8, 40, (2, 5, 9), (5, 11, 20)),
    'down':      (1, 17, (6, 9, 10), (3, 5, 7)),
    'equal':     (2, 17, (4, 9, 11), (4, 9, 11)),
    'z1':        (1, 5, (1, 5, 9), (4, 10, 18)),
    'y1':        (1, 17, (4, 1, 9), (8, 6, 18)),
    'x1':        (1, 4, (4, 5, 1), (8, 10, 5)),
    'q1':        (1, 1, (3, 7, 5), (6, 14, 10)),
    'q4':        (2, 4, (3, 7, 5), (6, 14, 10)),
    'q5':        (1, 5, (4, 10, 12), (8, 20, 24)),
    'q17':       (1, 17, (4, 10, 12), (8, 20, 24)),
    'q40':       (1, 40, (4, 10, 12), (9, 21, 25)),
}
UNDECIDED_CAP = 1e-3


def occ_inputs(name):
    """The random logits of one case: 3 N(0,1) class logits, N(0,1) occupancy logits."""
    B, Q, low, size = OCC_CASES[name]
    g = torch.Generator().manual_seed(sorted(OCC_CASES).index(name) + 100)
    sem_low = torch.randn(B, Q, *low, generator=g) * 3
    bin_low = torch.randn(B, 2, *low, generator=g)
    return sem_low, bin_low, size


INTEGER_CASE = (2, 17, (4, 10, 12), (8, 20, 24))


def occ_integer_inputs():
    """Integer-valued logits in [-4, 4] at a 2x ratio: lambdas 0, 0.25, 0.75, 1 and
    integers are exact through the whole nest in fp32, so nothing is undecided; ties of
    the maximum and o0 == o1 both occur."""
    B, Q, low, size = INTEGER_CASE
    g = torch.Generator().manual_seed(7)
    sem_low = torch.randint(-4, 5, (B, Q) + low, generator=g).float()
    bin_low = torch.randint(-4, 5, (B, 2) + low, generator=g).float()
    return sem_low, bin_low, size


SPECIAL_CASE = (1, 5, (4, 6, 7), (8, 12, 14))


def occ_special_inputs():
    """Random logits with hand-placed special values -> (sem_low, bin_low, size,
    mask_low): ``mask_low`` (B,z,y,x) marks the low-resolution voxels that hold one."""
    B, Q, low, size = SPECIAL_CASE
    g = torch.Generator().manual_seed(9)
    sem_low = torch.randn(B, Q, *low, generator=g) * 3
    bin_low = torch.randn(B, 2, *low, generator=g)
    nan, inf = float('nan'), float('inf')
    sem_low[0, 2, 0, 0, 0] = nan                      # NaN in one class, at a corner
    sem_low[0, 1, 1, 2, 3] = nan                      # ... and inside
    sem_low[0, 3, 2, 4, 1] = inf                      # +inf in one class
    lo = sem_low[0, :, 3, 1, 5].argmin()
    sem_low[0, lo, 3, 1, 5] = -inf                    # -inf in a non-maximal class
    sem_low[0, :, 1, 5, 6] = -inf                     # -inf in every class of a voxel
    sem_low[0, :, 3, 5, 0] = -inf                     # ... at a corner of the volume
    bin_low[0, 0, 0, 3, 3] = nan
    bin_low[0, 1, 2, 0, 6] = nan
    bin_low[0, 0, 3, 3, 2] = inf
    bin_low[0, 1, 0, 5, 1] = inf
    bin_low[0, 0, 2, 2, 4] = -inf
    bin_low[0, 1, 1, 0, 0] = -inf
    mask = ~torch.isfinite(sem_low).all(dim=1) | ~torch.isfinite(bin_low).all(dim=1)
    return sem_low, bin_low, size, mask


# ------------------------------------------------------------------ depth preparation
# Inputs of tests/test_depth_prep_edges_gpu.py (the reference there is the C oracle).
DEPTH_BN = 2
DEPTH_PARAMS = [(59, 1.0, 1.0, 4.0), (118, 1.0, 0.5, 4.0), (30, 2.0, 2.0, 1.0),
                (8, 1.0, 1.0, 0.5),        # the window covers every bin: K = D + 1
                (59, 1.0, 1.0, 64.0)]      # at most one or two bins unclamped
DEPTH_SIZES = [(3, 5), (16, 44), (1, 257)]


def depth_centres(D, lo, step):
    off = np.float32(np.float64(lo) + np.float64(step) / 2.0)
    return (np.arange(D + 1, dtype=np.float32) * np.float32(step) + off).astype(np.float32)


def depth_targets(D, lo, step, gamma):
    """The block minima the map is built around, with the kind of each:
    0 zero block, 1 uniform (every logit clamped), 2 other."""
    c = depth_centres(D, lo, step)
    reach = np.float32(16.0) / np.float32(gamma)
    vals, kinds = [], []

    def add(v, kind=2):
        vals.extend(np.atleast_1d(np.asarray(v, np.float32)).tolist())
        kinds.extend([kind] * np.atleast_1d(v).size)
    add(0.0, 0)                                                  # a whole block of zeros
    add(c)                                                       # on every centre
    add((c[:-1] + c[1:]) / np.float32(2))                               # on every midpoint
    lo_edge, hi_edge = c[0] - reach, c[-1] + reach               # exact: binary fractions
    add([np.float32(lo) - reach - np.float32(1), lo_edge - np.float32(0.5), lo_edge - np.float32(40)], 1)
    add([hi_edge + np.float32(0.5), hi_edge + np.float32(3), np.float32(1e4)], 1)
    for edge in (lo_edge, hi_edge):                              # just inside / outside
        add([np.nextafter(edge, np.float32(-1e9)), edge, np.nextafter(edge, np.float32(1e9))])
    g = np.random.default_rng(D)
    add(g.uniform(c[0] - reach, c[-1] + reach, 24).astype(np.float32))
    vals, kinds = np.asarray(vals, np.float32), np.asarray(kinds)
    # a uniform target must really clamp every bin, any other non-zero one must not
    far = np.abs(vals[:, None] - c[None]).min(1) * np.float32(gamma) > 16
    assert np.array_equal(far[kinds == 1], np.ones((kinds == 1).sum(), bool))
    keep = (vals != 0) | (kinds == 0)                            # 0.0 means "missing"
    return vals[keep], kinds[keep]


def depth_map(h, w, ds, params):
    """(1, DEPTH_BN, h*ds, w*ds) fp32 whose block minima cycle through ``depth_targets``; the
    target sits at each of the ds*ds positions in turn, its neighbours are zeros (a
    single non-zero pixel), larger values, or a mix."""
    vals, kinds = depth_targets(*params)
    n = DEPTH_BN * h * w
    idx = np.arange(n) % len(vals)
    tgt, kind = vals[idx], kinds[idx]
    g = np.random.default_rng(h * 1000 + w + ds)
    blocks = np.zeros((n, ds * ds), np.float32)
    fill = (np.maximum(tgt, 0)[:, None] + 1 + g.uniform(0, 5, (n, ds * ds))).astype(np.float32)
    style = (np.arange(n) // len(vals)) % 3          # 0: zeros, 1: larger, 2: mixed
    mixed = g.uniform(size=(n, ds * ds)) < 0.5
    blocks = np.where((style == 1)[:, None] | ((style == 2)[:, None] & mixed), fill, blocks)
    pos = np.arange(n) % (ds * ds)
    blocks[np.arange(n), pos] = tgt
    blocks[kind == 0] = 0                            # whole blocks of zeros
    want_min = np.where(kind == 0, np.float32(1e5), tgt).astype(np.float32)
    m = blocks.reshape(DEPTH_BN, h, w, ds, ds).transpose(0, 1, 3, 2, 4).reshape(1, DEPTH_BN, h * ds, w * ds)
    return np.ascontiguousarray(m), want_min.reshape(1, DEPTH_BN, h, w), kind.reshape(1, DEPTH_BN, h, w)
