#!/usr/bin/env python
"""Forward + backward of the depth pre-training loss (veon_amd.depth_loss) at the VEON
shapes: native (csrc/depth_loss.hip) against the reference's torch sequence
(``depth_pretrain_loss_torch``) on the same device, in the same process, alternating.

    python tools/depth_loss_bench.py [--rounds 5] [--window 0.5] [--quick]

6 cameras, LiDAR depth at 256 x 704 and 512 x 1408 (about 10 % of the pixels hit),
predictions at half that size, scales 8 / 16, depth grid [1, 45, 0.5] (D = 88): 4224 and
16896 rows.  One step = the loss dict and depth_error from the two full-resolution maps,
then the gradient of loss_depth_zoe + loss_depth_ce with respect to the prediction.
Per size and structure: microseconds per step (device events around a window of
back-to-back steps that lasts at least ``--window`` seconds) as median [min .. max] over
``--rounds`` alternating rounds, and the device kernel launches of one step as the torch
profiler counts them (``--quick``: 2 rounds of 50 ms and no launch count, for a separate
``rocprofv3 --kernel-trace --stats`` run).  The torch sequence is the baseline because it
is what a user had to write before; it synchronises the host four times per step, the
native path never.  Needs a ROCm device."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import depth_loss  # noqa: E402

GRID = (1.0, 45.0, 0.5)
D, LO, STEP = 88, GRID[0], GRID[2]
SP, SG, CAMS = 8, 16, 6


def make_inputs(Hg, Wg, seed, dev):
    g = torch.Generator().manual_seed(seed)
    h, w = Hg // SG, Wg // SG
    target = 2.0 + 40.0 * torch.rand(1, CAMS, h, w, generator=g)
    up = lambda t, s: t.repeat_interleave(s, 2).repeat_interleave(s, 3)     # noqa: E731
    gt = up(target, SG) + 2.0 * torch.rand(1, CAMS, Hg, Wg, generator=g)
    gt = gt * (torch.rand(1, CAMS, Hg, Wg, generator=g) < 0.1)
    pred = up(target, SP) * (1 + 0.15 * torch.randn(1, CAMS, h * SP, w * SP, generator=g)) \
        + 3.0 * torch.rand(1, CAMS, h * SP, w * SP, generator=g)
    return pred.clamp_min(0.05).to(dev), gt.to(dev)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps     # us


def launches(fn):
    """Device kernels of one step, by the torch profiler; None when it cannot say."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events()
                if str(getattr(e, 'device_type', '')).endswith('CUDA') and e.name
                and not e.name.lower().startswith(('memcpy', 'memset')))
        return n or None
    except Exception as exc:          # the count is a by-product, the timing is the point
        print('launch count unavailable: %s' % exc)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='seconds per timed window')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 50 ms (profiler run)')
    a = ap.parse_args()
    rounds, window = (2, 0.05) if a.quick else (a.rounds, a.window)
    if not torch.cuda.is_available():
        sys.exit('depth_loss_bench: no ROCm device')
    dev = 'cuda:0'
    print('device %s; %d rounds, windows of >= %.2f s, structures alternating'
          % (torch.cuda.get_device_name(0), rounds, window))
    print('%-10s %-6s %-9s | %30s | %8s | %8s' % ('labels', 'rows', 'structure',
                                                  'us/step median [min .. max]', 'steps',
                                                  'launches'))
    for Hg, Wg in ((256, 704), (512, 1408)):
        pred, gt = make_inputs(Hg, Wg, Hg, dev)
        fns = {}
        for name, fn in (('native', depth_loss.depth_pretrain_loss),
                         ('torch', depth_loss.depth_pretrain_loss_torch)):
            def step(fn=fn):
                leaf = pred.detach().requires_grad_()
                out = fn(leaf, gt, D, LO, STEP, SP, SG)
                (out['loss_depth_zoe'] + out['loss_depth_ce']).backward()
                return out, leaf.grad
            fns[name] = step
        (ref, ref_grad), (got, got_grad) = fns['torch'](), fns['native']()
        for k in ref:                      # the two structures compute the same thing
            assert abs(float(got[k].detach()) - float(ref[k].detach())) <= 1e-4 * abs(float(ref[k].detach())), k
        assert float((got_grad - ref_grad).abs().max()) <= 1e-4 * float(ref_grad.abs().max())
        steps = {}
        for name in fns:                   # warm-up, and the window's length in steps
            fns[name]()
            steps[name] = max(10, math.ceil(window * 1e6 / timed(fns[name], 20)))
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name in fns:
                times[name].append(timed(fns[name], steps[name]))
        for name in fns:
            t = times[name]
            n = None if a.quick else launches(fns[name])
            print('%-10s %-6d %-9s | %10.1f [%8.1f .. %8.1f] | %8d | %8s'
                  % ('%dx%d' % (Hg, Wg), CAMS * (Hg // SG) * (Wg // SG), name,
                     statistics.median(t), min(t), max(t), steps[name],
                     'n/a' if n is None else n))
        med = {k: statistics.median(v) for k, v in times.items()}
        print('%-28s native / torch = %.3f' % ('', med['native'] / med['torch']))


if __name__ == '__main__':
    main()
