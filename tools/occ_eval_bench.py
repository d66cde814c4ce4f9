#!/usr/bin/env python
"""The tail of the occupancy path and the mIoU step at the VEON shape: B 1, Q 17,
(8, 100, 100) -> (16, 200, 200), the class logits as the path hands them over (the
channels-last interior of the classifier GEMM's padded rows), in one process, the
structures alternating within every round.

    python tools/occ_eval_bench.py [--rounds 7] [--window 0.3] [--out FILE]

    occ_classify       the tail as it was: upsampled logits (48 MB) + int64 labels
    occ_labels         the label-only tail: uint8 labels (640 KB), nothing else
    occ_labels + hist  the same with the confusion matrix fused in
    confusion          the confusion matrix of existing uint8 labels
    confusion int64    ... of occ_classify's int64 labels
    host step          the reference's per-sample step restated: labels
                       ``.cpu().numpy().astype(np.uint8)``, boolean-mask selection of
                       prediction and ground truth, ``np.bincount``
                       (veon_temporal.py:241, occ_metrics.py:94-101, 123-125)

Microseconds per call: a host clock around a window of back-to-back calls (at least
``--window`` seconds) that ends in a device synchronise, as median [min .. max] over
``--rounds`` rounds.  The yardstick of the two label kernels is ``occ_classify`` in the
same run; a difference counts when the [min .. max] ranges do not overlap.  Needs a ROCm
device."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import conv3d_ops, occ_eval  # noqa: E402

B, Q, LOW, SIZE = 1, 17, (8, 100, 100), (16, 200, 200)
N_CL = Q + 1


def make_inputs(dev):
    g = torch.Generator().manual_seed(0)
    z, y, x = LOW
    rows = torch.randn(B, z + 2, y + 2, x + 2, 24, generator=g).to(dev) * 3
    sem = rows[:, 1:-1, 1:-1, 1:-1, :Q].permute(0, 4, 1, 2, 3)
    binv = torch.randn(B, 2, z, y, x, generator=g).to(dev)
    shape = (B, SIZE[2], SIZE[1], SIZE[0])
    gt = torch.randint(0, N_CL, shape, generator=g, dtype=torch.uint8)
    gt[torch.rand(shape, generator=g) < 0.1] = 255
    mask = (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8)
    return sem, binv, gt.to(dev), mask.to(dev)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls     # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window')
    ap.add_argument('--out', help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('occ_eval_bench: no ROCm device')
    dev = 'cuda:0'
    sem, binv, gt, mask = make_inputs(dev)
    hist = torch.zeros((N_CL, N_CL), dtype=torch.int64, device=dev)
    labels64 = conv3d_ops.occ_classify(sem, binv, SIZE)[2]
    labels8 = occ_eval.occ_labels(sem, binv, SIZE)
    assert torch.equal(labels8, labels64.to(torch.uint8))       # the same labels
    gt_np, mask_np = gt.cpu().numpy(), mask.cpu().numpy().astype(bool)

    def host_step():
        pred = labels64.cpu().numpy().astype(np.uint8)
        p, t = pred[mask_np], gt_np[mask_np]
        k = (t >= 0) & (t < N_CL)
        return np.bincount(N_CL * t[k].astype(int) + p[k].astype(int),
                           minlength=N_CL ** 2).reshape(N_CL, N_CL)

    fns = {
        'occ_classify': lambda: conv3d_ops.occ_classify(sem, binv, SIZE),
        'occ_labels': lambda: occ_eval.occ_labels(sem, binv, SIZE),
        'occ_labels + hist': lambda: occ_eval.occ_labels(sem, binv, SIZE, gt, mask, hist),
        'confusion': lambda: occ_eval.confusion(labels8, gt, mask, N_CL, hist),
        'confusion int64': lambda: occ_eval.confusion(labels64, gt, mask, N_CL, hist),
        'host step': host_step,
    }
    want = torch.from_numpy(host_step())                        # ... and the same counts
    for name in ('occ_labels + hist', 'confusion', 'confusion int64'):
        hist.zero_()
        fns[name]()
        assert torch.equal(hist.cpu(), want), name
    calls = {}
    for name, fn in fns.items():       # warm-up, and the window's length in calls
        fn()
        calls[name] = max(5, math.ceil(a.window * 1e6 / timed(fn, 5)))
    times = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, calls[name]))
    lines = ['device %s; B %d, Q %d, %s -> %s; %d rounds, windows of >= %.2f s, alternating'
             % (torch.cuda.get_device_name(0), B, Q, LOW, SIZE, a.rounds, a.window),
             '%-18s | %30s | %7s' % ('structure', 'us/call median [min .. max]', 'calls')]
    for name, t in times.items():
        lines.append('%-18s | %10.1f [%8.1f .. %8.1f] | %7d'
                     % (name, statistics.median(t), min(t), max(t), calls[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    for name in ('occ_labels', 'occ_labels + hist'):
        if max(times[name]) < min(times['occ_classify']):
            verdict = 'below, ranges apart'
        elif min(times[name]) > max(times['occ_classify']):
            verdict = 'above, ranges apart'
        else:
            verdict = 'ranges overlap: no difference shown'
        lines.append('%-18s / occ_classify = %.3f (%s)'
                     % (name, med[name] / med['occ_classify'], verdict))
    lines.append('%-18s / host step    = %.4f' % ('occ_labels + hist',
                                                   med['occ_labels + hist'] / med['host step']))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
