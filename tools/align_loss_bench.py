#!/usr/bin/env python
"""Forward + backward of the feature-alignment primitive (veon_amd.align_loss.
voxel_cosine) at the VEON shapes: native against two torch formulations, in the same
process, alternating.

    python tools/align_loss_bench.py [--rounds 5] [--steps 10] [--quick]

VEON-B (C = 512) and VEON-L (C = 768), low-resolution volume (8, 100, 100) -> grid
(16, 200, 200), N in {40 000, 200 000} entries, drawn uniformly over the grid or from a
thin slab (surface-like, heavy stencil overlap), K = 18 table rows.  Features in both
layouts that matter: ``cl`` = channels-last rows (the kernels' vector path) and ``ncdhw``
(what the torch heads of the training path produce: the any-stride scalar path, plus
autograd's layout copy of the channels-last gradient).  Structures:
    native    csrc/occ_align_loss.hip in both directions
    upsample  the reference formulation: F.interpolate to the grid, gather, cosine
    gather8   the cheap torch formulation: index_select of the 8 corner rows, blend,
              cosine; autograd's backward is index_add_ onto the low-resolution rows
Per case and structure: ms per step (device events over ``--steps`` back-to-back steps)
as median [min .. max] over ``--rounds`` alternating rounds, and the rise of
torch.cuda.max_memory_allocated over one step.  N is an assumption: how many entries a
real Occ3D sample yields is not known here; the two values bracket "non-free voxels
seen by a camera".  Needs a ROCm device.  Kernel-level times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this tool with ``--quick``."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd.align_loss import voxel_cosine  # noqa: E402

LOW, OCC, K, EPS = (8, 100, 100), (16, 200, 200), 18, 1e-6


def entries(kind, n, seed, dev):
    Z, Y, X = OCC
    g = torch.Generator().manual_seed(seed)
    if kind == 'uniform':
        vox = torch.stack([torch.randint(0, s, (n,), generator=g) for s in (X, Y, Z)], 1)
    else:
        vox = torch.stack([torch.randint(0, X, (n,), generator=g),
                           Y // 3 + torch.randint(0, 12, (n,), generator=g),
                           Z // 2 + torch.randint(0, 2, (n,), generator=g)], 1)
    lab = torch.randint(0, K, (n,), generator=g)
    return vox.to(torch.int32).to(dev), lab.to(torch.int32).to(dev)


def upsample(feat, vox, lab, table):
    v = vox.long()
    f_up = F.interpolate(feat, OCC, mode='trilinear', align_corners=False)[0]
    return F.cosine_similarity(f_up[:, v[:, 2], v[:, 1], v[:, 0]].T, table[lab.long()], dim=1,
                               eps=EPS)


def axis(dst, n_in, n_out):
    src = ((dst.float() + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0
    return i0, i1, 1 - l1, l1


def gather8(feat, vox, lab, table):
    rows = feat[0].permute(1, 2, 3, 0).reshape(-1, feat.shape[1])       # (zyx, C)
    z, y, x = LOW
    ax = [axis(vox[:, k].long(), n, m) for k, n, m in ((2, z, OCC[0]), (1, y, OCC[1]), (0, x, OCC[2]))]
    f = 0
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                idx = (ax[0][a] * y + ax[1][b]) * x + ax[2][c]
                w = ax[0][2 + a] * ax[1][2 + b] * ax[2][2 + c]
                f = f + w[:, None] * rows.index_select(0, idx)
    return F.cosine_similarity(f, table[lab.long()], dim=1, eps=EPS)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps     # ms


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise / 1e6        # MB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 3 steps (profiler run)')
    a = ap.parse_args()
    rounds, steps = (2, 3) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('align_loss_bench: no ROCm device')
    dev = 'cuda:0'
    print('device %s; %d rounds of %d steps, structures alternating' % (
        torch.cuda.get_device_name(0), rounds, steps))
    print('low %s -> grid %s, K = %d; upsampled volume %.1f MB (C = 512) / %.1f MB (C = 768)'
          % (LOW, OCC, K, 512 * 640000 * 4 / 1e6, 768 * 640000 * 4 / 1e6))
    print('%-4s %-6s %-8s %-7s %-9s | %28s | %9s' % ('C', 'layout', 'entries', 'N', 'structure',
                                                     'ms/step median [min .. max]', 'peak MB'))
    structures = (('native', lambda f, v, l, t: voxel_cosine(f, v, l, t, OCC, EPS)),
                  ('gather8', gather8), ('upsample', upsample))
    for C, layout in ((512, 'cl'), (512, 'ncdhw'), (768, 'cl'), (768, 'ncdhw')):
        g = torch.Generator().manual_seed(C)
        feat = (torch.sigmoid(2 * torch.randn((1,) + LOW + (C,), generator=g)) - 0.5).to(dev)
        feat = feat.permute(0, 4, 1, 2, 3)                 # channels-last rows
        if layout == 'ncdhw':
            feat = feat.contiguous()
        table = torch.randn(K, C, generator=g).to(dev)
        for kind in ('uniform', 'slab'):
            for n in (40000, 200000):
                vox, lab = entries(kind, n, n + C, dev)
                gout = torch.randn(n, generator=g).to(dev)
                fns = {}
                for name, fn in structures:
                    def step(fn=fn):
                        leaf = feat.detach().requires_grad_()
                        fn(leaf, vox, lab, table).backward(gout)
                        return leaf.grad
                    fns[name] = step
                ref = fns['upsample']()
                for name in fns:       # warm-up and a sanity check of the structure
                    got = fns[name]()
                    err = float((got - ref).abs().max() / ref.abs().max())
                    assert err < 1e-3, (name, err)
                    fns[name]()
                times = {name: [] for name in fns}
                for _ in range(rounds):
                    for name in fns:
                        times[name].append(timed(fns[name], steps))
                for name in fns:
                    t = times[name]
                    print('%-4d %-6s %-8s %-7d %-9s | %9.3f [%8.3f .. %8.3f] | %9.1f' % (
                        C, layout, kind, n, name, statistics.median(t), min(t), max(t),
                        peak_rise(fns[name])))
                med = {k: statistics.median(v) for k, v in times.items()}
                print('%-38s native / gather8 = %.3f, native / upsample = %.3f' % (
                    '', med['native'] / med['gather8'], med['native'] / med['upsample']))


if __name__ == '__main__':
    main()
