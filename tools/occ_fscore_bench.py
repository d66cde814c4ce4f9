#!/usr/bin/env python
"""The F-score step at the VEON shape, (1, 200, 200, 16) uint8 labels, at about 3 % and
about 10 % occupied voxels, in one process, the structures alternating within every
round.

    python tools/occ_fscore_bench.py [--rounds 5] [--window 0.5] [--out FILE]

    fscore_counts      the kernel (csrc/occ_fscore.hip) with the reference's default
                       thresholds: a halo of one column, reaches 1 / 1 / 0
    fscore_counts R=0  the same kernel with a one-entry table of reach 0: no halo, the own
                       column only -- what phase 1 (loads and bit-packing), the
                       reduction and the launch cost without the neighbourhood
    torch mirror       ``fscore_counts_torch`` on the device: pad, shift, OR, sum
    confusion          the mIoU kernel on the same volume in the same run: it reads the
                       same bytes, so it is the floor to compare against

Microseconds per call from device events around windows of back-to-back calls (at least
``--window`` seconds each), as median [min .. max] over ``--rounds`` rounds.  A difference
counts when the [min .. max] ranges do not overlap.  The reference's own step
(``Metric_FScore.add_batch``: two KD-trees per sample on the host, occ_metrics.py:
190-233) is not run here -- this tool needs neither the reference tree nor sklearn; it
took 0.11 to 0.12 s per sample at this shape and 3 % occupancy on the CPU of a development
machine, NOT on the machine of the GPU.  Needs a ROCm device."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import occ_eval  # noqa: E402

SHAPE, N_CL = (1, 200, 200, 16), 18
OWN_COLUMN = (0, np.zeros((1, 1), np.int32))
REFERENCE_HOST_STEP_S = (0.11, 0.12)


def make_inputs(dev, density, seed):
    g = torch.Generator().manual_seed(seed)

    def labels():
        lab = torch.randint(0, 17, SHAPE, generator=g, dtype=torch.uint8)
        lab[torch.rand(SHAPE, generator=g) >= density] = 17
        return lab
    pred, gt = labels(), labels()
    gt[torch.rand(SHAPE, generator=g) < 0.05] = 255
    mask = (torch.rand(SHAPE, generator=g) >= 0.3).to(torch.uint8)
    return pred.to(dev), gt.to(dev), mask.to(dev)


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls     # us


def verdict(a, b):
    if max(a) < min(b):
        return 'below, ranges apart'
    if min(a) > max(b):
        return 'above, ranges apart'
    return 'ranges overlap: no difference shown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='seconds per timed window')
    ap.add_argument('--out', help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('occ_fscore_bench: no ROCm device')
    dev = 'cuda:0'
    lines = ['device %s; labels %s uint8; %d rounds, device events over windows of >= %.2f s, '
             'alternating' % (torch.cuda.get_device_name(0), SHAPE, a.rounds, a.window)]
    for occupied, seed in ((0.03, 0), (0.10, 1)):
        # (the mask voids 30 % of the labelled voxels again)
        pred, gt, mask = make_inputs(dev, occupied / 0.7, seed)
        out = torch.zeros((SHAPE[0], 4), dtype=torch.int64, device=dev)
        hist = torch.zeros((N_CL, N_CL), dtype=torch.int64, device=dev)
        void, reach = (17, 255), occ_eval.DEFAULT_REACH
        fns = {
            'fscore_counts': lambda: occ_eval.fscore_counts(pred, gt, mask, out=out),
            'fscore_counts R=0': lambda: occ_eval.fscore_counts(
                pred, gt, mask, reach_acc=OWN_COLUMN, reach_cmpl=OWN_COLUMN, out=out),
            'torch mirror': lambda: occ_eval.fscore_counts_torch(pred, gt, mask, void, reach,
                                                                 reach),
            'confusion': lambda: occ_eval.confusion(pred, gt, mask, N_CL, hist),
        }
        counts = occ_eval.fscore_counts(pred, gt, mask)
        assert torch.equal(counts, fns['torch mirror']())        # the same counts
        assert torch.equal(counts.cpu(), occ_eval.fscore_counts(pred.cpu(), gt.cpu(), mask.cpu()))
        calls = {}
        for name, fn in fns.items():       # warm-up, and the window's length in calls
            fn()
            calls[name] = max(5, math.ceil(a.window * 1e6 / timed(fn, 5)))
        times = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                times[name].append(timed(fn, calls[name]))
        n = pred[0].numel()
        lines.append('')
        lines.append('occupied: prediction %.1f %%, ground truth %.1f %% of %d voxels; counts %s'
                     % (100.0 * int(counts[0, 0]) / n, 100.0 * int(counts[0, 1]) / n, n,
                        counts[0].tolist()))
        lines.append('%-18s | %30s | %7s' % ('structure', 'us/call median [min .. max]', 'calls'))
        for name, t in times.items():
            lines.append('%-18s | %10.1f [%8.1f .. %8.1f] | %7d'
                         % (name, statistics.median(t), min(t), max(t), calls[name]))
        med = {k: statistics.median(v) for k, v in times.items()}
        for name, other in (('fscore_counts', 'confusion'), ('fscore_counts R=0', 'confusion'),
                            ('fscore_counts', 'fscore_counts R=0'),
                            ('fscore_counts', 'torch mirror')):
            lines.append('%-18s / %-17s = %.3f (%s)' % (name, other, med[name] / med[other],
                                                         verdict(times[name], times[other])))
        lines.append("%-18s / the reference's host step of %.2f .. %.2f s (a development "
                     "machine's CPU, not this machine's) = %.1e .. %.1e"
                     % ('fscore_counts', REFERENCE_HOST_STEP_S[0], REFERENCE_HOST_STEP_S[1],
                        med['fscore_counts'] * 1e-6 / REFERENCE_HOST_STEP_S[1],
                        med['fscore_counts'] * 1e-6 / REFERENCE_HOST_STEP_S[0]))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
