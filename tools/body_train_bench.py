#!/usr/bin/env python
"""Training step of the Conv3d body (AlignBody3D forward + backward, train-mode BN) at
the VEON shape: B = 1, 256 channels, 8 x 100 x 100 voxels, four ResBlock3D.  Three
structures in one process, alternating rounds:

    torch fp32      what a training step runs without the switch (nn.Conv3d / BatchNorm3d)
    torch autocast  the same modules under torch.autocast with the build's half dtype
    native          ResBlock3D.hip_train = True (csrc/conv3d_train.hip)
    native syncbn   (with --sync-bn) a copy of the body converted by
                    nn.SyncBatchNorm.convert_sync_batchnorm, hip_train = True: the
                    synchronised statistics interval (veon_amd/sync_bn.py) in ONE process
                    with no process group, so without a collective

    python tools/body_train_bench.py [--rounds 5] [--steps 5] [--quick] [--only native]
                                     [--sync-bn]

Per structure: ms per step (forward + backward, input gradient included, device events
over ``--steps`` back-to-back steps) as median [min .. max] over ``--rounds`` alternating
rounds -- the spread is the yardstick for the comparison -- and the rise of
torch.cuda.max_memory_allocated over one step above the resident inputs.  Needs a ROCm
device.  Kernel-level times come from a separate ``rocprofv3 --kernel-trace --stats``
run of this tool with ``--quick`` (and ``--only native`` for the native kernels alone)."""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import half  # noqa: E402
from veon_amd.models.semantic_net import AlignBody3D, ResBlock3D  # noqa: E402

STRUCTURES = ('torch fp32', 'torch autocast', 'native')
SYNC = 'native syncbn'


def step_fn(body, x, gout, structure):
    def step():
        ResBlock3D.hip_train = structure in ('native', SYNC)
        xi = x.detach().requires_grad_()
        if structure == 'torch autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                out = body(xi)
        else:
            out = body(xi)
        out.backward(gout.to(out.dtype))
        ResBlock3D.hip_train = False
        return xi.grad
    return step


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
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 2 steps (profiler run)')
    ap.add_argument('--only', choices=STRUCTURES + (SYNC,), default=None)
    ap.add_argument('--sync-bn', action='store_true',
                    help='add the structure "native, SyncBatchNorm-converted"')
    a = ap.parse_args()
    if a.only == SYNC:
        a.sync_bn = True
    rounds, steps = (2, 2) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('body_train_bench: no ROCm device')
    dev = 'cuda:0'
    torch.manual_seed(0)
    body = AlignBody3D(256, 4).to(dev).train()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(1, 256, 8, 100, 100, generator=gen).relu().to(dev)   # a lifted volume
    gout = torch.randn(1, 256, 8, 100, 100, generator=gen).to(dev)
    # --only X --sync-bn: X and the converted structure alternate
    names = [a.only] if a.only else list(STRUCTURES)
    if a.sync_bn and SYNC not in names:
        names.append(SYNC)
    print('device %s; %s operands; %d rounds of %d steps, structures alternating' % (
        torch.cuda.get_device_name(0), half.name(), rounds, steps))
    print('AlignBody3D(256, 4), training mode, input 1 x 256 x 8 x 100 x 100 (%.1f MB fp32)'
          % (x.numel() * 4 / 1e6))
    bodies = {n: body for n in names}
    if SYNC in names:
        assert not torch.distributed.is_initialized()      # no group: no collective
        bodies[SYNC] = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(body))
    fns = {n: step_fn(bodies[n], x, gout, n) for n in names}
    for n in names:          # warm-up: MIOpen's algorithm search, workspaces, allocator
        for _ in range(2):
            fns[n]()
    times = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            times[n].append(timed(fns[n], steps))
    peaks = {n: peak_rise(fns[n]) for n in names}
    print('%-15s | %30s | %10s' % ('structure', 'ms/step median [min .. max]', 'peak MB'))
    for n in names:
        t = times[n]
        print('%-15s | %9.3f [%8.3f .. %8.3f] | %10.1f' % (
            n, statistics.median(t), min(t), max(t), peaks[n]))
    med = {n: statistics.median(t) for n, t in times.items()}
    if 'native' in med and SYNC in med:
        spread = {n: max(times[n]) - min(times[n]) for n in ('native', SYNC)}
        print('%s - native = %+.3f ms (%.3f of native); spread of the rounds: native %.3f ms, '
              '%s %.3f ms' % (SYNC, med[SYNC] - med['native'], med[SYNC] / med['native'],
                              spread['native'], SYNC, spread[SYNC]))
    if 'native' in med:
        for n in names:
            if n not in ('native', SYNC):
                print('native / %s = %.3f; spread of the rounds: %s %.3f ms, native %.3f ms'
                      % (n, med['native'] / med[n], n, max(times[n]) - min(times[n]),
                         max(times['native']) - min(times['native'])))


if __name__ == '__main__':
    main()
