#!/usr/bin/env python
"""Point retrieval on the occupancy path: the native kernel (csrc/occ_retrieval.hip,
reading the low-resolution half rows) against the torch formulation of the reference
(fp32 trilinear upsample of the whole feature volume, gather, F.cosine_similarity;
san_in_veon_temporal.py:195-200, 268-273).

    python tools/retrieval_bench.py [--iters 200] [--quick]

Shapes: VEON-B (C = 512) and VEON-L (C = 768), (8,100,100) -> (16,200,200), P in
{35 k, 200 k} uniform random points, Q in {1, 17}.  Per case: mean time per launch
from device events over ``--iters`` warm back-to-back launches, and the rise of
torch.cuda.max_memory_allocated over one call above what was allocated before it.
Kernel-level times come from a separate ``rocprofv3 --kernel-trace --stats`` run of
this tool with ``--quick``."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import conv3d_ops  # noqa: E402
from veon_amd.retrieval import retrieve_points  # noqa: E402

LOW, OCC = (8, 100, 100), (16, 200, 200)


def torch_formulation(feat32, pts, emb):
    """the reference: upsample the full volume, gather the points, cosine per prompt"""
    f_up = F.interpolate(feat32, OCC, mode='trilinear', align_corners=False)[0]
    x, y, z = pts.long().T
    f = f_up[:, z, y, x]                                    # (C, P)
    return torch.stack([F.cosine_similarity(f, e[:, None], dim=0) for e in emb])


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3     # us


def peak_rise(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise / 2 ** 20        # MiB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--quick', action='store_true', help='20 launches per case (profiler run)')
    a = ap.parse_args()
    iters = 20 if a.quick else a.iters
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    print('device %s, %d launches per case' % (torch.cuda.get_device_name(0), iters))
    print('%-7s %4s %7s %3s | %10s %10s %8s | %10s %10s' % (
        'shape', 'C', 'P', 'Q', 'kernel us', 'torch us', 'speed-up', 'kernel MiB',
        'torch MiB'))
    for name, C in (('VEON-B', 512), ('VEON-L', 768)):
        x = torch.sigmoid(2 * torch.randn((1, C) + LOW, generator=g)) - 0.5
        vol = conv3d_ops.pack(x.to(dev))
        binl = torch.randn((1, 2) + LOW, generator=g).to(dev)
        feat32 = vol.interior().permute(0, 4, 1, 2, 3).float().contiguous()   # (1,C,z,y,x)
        for P in (35000, 200000):
            pts = torch.stack([torch.randint(0, n, (P,), generator=g)
                               for n in (OCC[2], OCC[1], OCC[0])], 1).to(torch.int32).to(dev)
            for Q in (1, 17):
                emb = torch.randn(Q, C, generator=g).to(dev)

                def kern():
                    return retrieve_points(vol, binl, pts, emb, OCC)

                def ref():
                    return torch_formulation(feat32, pts, emb)
                # same answer (bf16 operands on both sides, fp32 vs fp32)
                err = (kern()[0] - ref()).abs().max().item()
                tk, tr = timed(kern, iters), timed(ref, iters)
                mk, mr = peak_rise(kern), peak_rise(ref)
                print('%-7s %4d %7d %3d | %10.1f %10.1f %7.1fx | %10.2f %10.1f   (max |diff| %.1e)'
                      % (name, C, P, Q, tk, tr, tr / tk, mk, mr, err))
        del vol, feat32
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
