#!/usr/bin/env python
"""The LiDAR depth labels of one training step (veon_amd.lidar_depth) at the VEON shape: 6
cameras of the synthetic rig (veon_amd/synthetic.py), 512 x 1408 images, one sweep of
34 720 points in 5-float rows, depth range [1, 45).

    python tools/lidar_depth_bench.py [--rounds 5] [--window 0.5] [--quick]

In one process, alternating per round:

    native b1    ``multiview_depth`` (csrc/lidar_depth.hip) at block 1: six full maps
    native b16   the same at block 16: the 6 x 32 x 88 values the loss reads
    mirror       ``multiview_depth_torch`` on the same device (full maps)
    host         the reference's host sequence (loading.py:735-759, :811-821) restated with
                 its sort, per camera, on the host cores (torch's default thread count)
    h2d          the copy of the six full maps (17.3 MB, pinned) to the device, which the
                 host sequence needs on top

Microseconds per call as median [min .. max] over ``--rounds`` rounds; device structures
are timed with device events around a window of back-to-back calls that lasts at least
``--window`` seconds, the host sequence with the wall clock over a few calls (``--quick``:
2 rounds of 50 ms).  Needs a ROCm device."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import lidar_depth, synthetic  # noqa: E402

H, W, CAMS, POINTS, STRIDE = 512, 1408, 6, 34720, 5
LO, HI = 1.0, 45.0


def make_inputs(seed=0):
    """-> points (1, P, 5), lidar2img (1, 6, 3, 4), post_rots, post_trans on the CPU."""
    rig = synthetic.make_rig(batch=1, n_cams=CAMS, input_size=(H, W))
    lidar2ego = torch.eye(4)
    lidar2ego[:3, 3] = torch.tensor([0.94, 0.0, 1.84])
    l2le = lidar2ego.expand(1, CAMS, 4, 4).contiguous()
    lidar2img = lidar_depth.compose_lidar2img(l2le, rig['ego2global'], rig['sensor2ego'],
                                              rig['ego2global'], rig['intrins'])
    g = torch.Generator().manual_seed(seed)
    r = 2.0 + 50.0 * torch.rand(POINTS, generator=g) ** 2
    az = 2 * math.pi * torch.rand(POINTS, generator=g)
    el = torch.deg2rad(-30.0 + 40.0 * torch.rand(POINTS, generator=g))
    pts = torch.zeros(1, POINTS, STRIDE)
    pts[0, :, 0] = r * torch.cos(el) * torch.cos(az)
    pts[0, :, 1] = r * torch.cos(el) * torch.sin(az)
    pts[0, :, 2] = r * torch.sin(el)
    pts[0, :, 3] = torch.rand(POINTS, generator=g) * 255
    return pts, lidar2img, rig['post_rots'], rig['post_trans']


def host_sequence(points, lidar2img, post_rots, post_trans):
    """The reference's per-camera host steps with its sort key -> (6, H, W)."""
    maps = []
    for c in range(CAMS):
        m = lidar2img[0, c]
        p = points[0, :, :3].matmul(m[:3, :3].T) + m[:3, 3].unsqueeze(0)
        p = torch.cat([p[:, :2] / p[:, 2:3], p[:, 2:3]], 1)
        p = p.matmul(post_rots[0, c].T) + post_trans[0, c:c + 1, :]
        depth_map = torch.zeros((H, W), dtype=torch.float32)
        coor = torch.round(p[:, :2])
        depth = p[:, 2]
        kept = (coor[:, 0] >= 0) & (coor[:, 0] < W) & (coor[:, 1] >= 0) & (coor[:, 1] < H) & \
            (depth < HI) & (depth >= LO)
        coor, depth = coor[kept], depth[kept]
        ranks = coor[:, 0] + coor[:, 1] * W
        order = (ranks + depth / 100.).argsort()
        coor, depth, ranks = coor[order], depth[order], ranks[order]
        first = torch.ones(coor.shape[0], dtype=torch.bool)
        first[1:] = ranks[1:] != ranks[:-1]
        coor, depth = coor[first].to(torch.long), depth[first]
        depth_map[coor[:, 1], coor[:, 0]] = depth
        maps.append(depth_map)
    return torch.stack(maps)


def timed_device(fn, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps     # us


def timed_host(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='seconds per timed window')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 50 ms')
    a = ap.parse_args()
    rounds, window = (2, 0.05) if a.quick else (a.rounds, a.window)
    if not torch.cuda.is_available():
        sys.exit('lidar_depth_bench: no ROCm device')
    dev = 'cuda:0'
    cpu = make_inputs()
    pts, l2i, rots, trans = (t.to(dev).contiguous() for t in cpu)
    out1 = torch.empty((1, CAMS, H, W), device=dev)
    out16 = torch.empty((1, CAMS, H // 16, W // 16), device=dev)
    pinned = torch.zeros((CAMS, H, W)).pin_memory()
    landing = torch.empty((CAMS, H, W), device=dev)
    fns = {
        'native b1': lambda: lidar_depth.multiview_depth(pts, l2i, rots, trans, H, W, (LO, HI),
                                                         out=out1),
        'native b16': lambda: lidar_depth.multiview_depth(pts, l2i, rots, trans, H, W, (LO, HI),
                                                          block=16, out=out16),
        'mirror': lambda: lidar_depth.multiview_depth_torch(pts, l2i, rots, trans, H, W,
                                                            (LO, HI)),
        'host': lambda: host_sequence(*cpu),
        'h2d': lambda: landing.copy_(pinned, non_blocking=True),
    }
    # the structures compute the same maps (the mirror to rounding; the host sequence up to
    # its ties)
    full, small, mir = fns['native b1']().clone(), fns['native b16']().clone(), fns['mirror']()
    host = fns['host']().to(dev)[None]
    occupied = int((full != 0).sum())
    print('device %s; %d rounds, windows of >= %.2f s, structures alternating; host threads %d'
          % (torch.cuda.get_device_name(0), rounds, window, torch.get_num_threads()))
    print('%d points, %d x %d x %d maps: %d occupied pixels, %d of %d block-16 values occupied'
          % (POINTS, CAMS, H, W, occupied, int((small != 0).sum()), small.numel()))
    for name, other in (('mirror', mir), ('host sequence', host)):
        print('native against the %s: occupancy differs on %d pixels, depth bits on %d, '
              'largest |difference| %.3e m'
              % (name, int(((full != 0) != (other != 0)).sum()), int((full != other).sum()),
                 float((full - other).abs().max())))
    steps = {}
    for name, fn in fns.items():
        timer = timed_host if name == 'host' else timed_device
        fn()
        steps[name] = max(3 if name == 'host' else 10, math.ceil(window * 1e6 / timer(fn, 3)))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append((timed_host if name == 'host' else timed_device)(fn, steps[name]))
    print('%-11s | %34s | %8s' % ('structure', 'us/call median [min .. max]', 'calls'))
    for name, t in times.items():
        print('%-11s | %12.1f [%9.1f .. %9.1f] | %8d'
              % (name, statistics.median(t), min(t), max(t), steps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    print('every native b1 round below every mirror round: %s (max %.1f against min %.1f)'
          % ('yes' if max(times['native b1']) < min(times['mirror']) else 'no',
             max(times['native b1']), min(times['mirror'])))
    print('every native b16 round below every mirror round: %s (max %.1f against min %.1f)'
          % ('yes' if max(times['native b16']) < min(times['mirror']) else 'no',
             max(times['native b16']), min(times['mirror'])))
    print('block 16 against block 1: %.1f us saved per call (%.3f of block 1)'
          % (med['native b1'] - med['native b16'], med['native b16'] / med['native b1']))
    print('host sequence + h2d against native b16: %.1f us against %.1f us'
          % (med['host'] + med['h2d'], med['native b16']))


if __name__ == '__main__':
    main()
