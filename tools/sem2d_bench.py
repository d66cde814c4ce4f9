#!/usr/bin/env python
"""The fused 2-D semantic tail (veon_amd/sem2d.py) against the torch tail it replaces, at
the VEON shape: six 512 x 1408 images, Q = 100 proposals at 32 x 88, C = 512, for K = 17
merged classes and K = 67 detailed rows (merged to 17 for the grouped labels).

    python tools/sem2d_bench.py [--rounds 5] [--window 0.3] [--out FILE]

    semantic_map       sem_seg (B,K,H,W) in one pass
    torch map          F.interpolate(mask_preds) -> sigmoid -> einsum: the default tail
    semantic_labels    uint8 labels only (grouped 67 -> 17 at K = 67)
    torch labels       torch map, run maxima, arg-max
    semantic_maps_ds   sem_seg_ds + sem_embed_ds in one launch
    torch maps_ds      softmax, sigmoid, two einsums

Microseconds per call: a host clock around a window of back-to-back calls (at least
``--window`` seconds) that ends in a device synchronise; the structures alternate within
every round, every round is printed, then median [min .. max].  Peak memory: the rise of
``torch.cuda.max_memory_allocated`` over one call.  Needs a ROCm device."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veon_amd import sem2d  # noqa: E402

B, Q, C, LOW, SIZE = 6, 100, 512, (32, 88), (512, 1408)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls     # us


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def measure(fns, rounds, window):
    calls, rises = {}, {}
    for name, fn in fns.items():       # warm-up, and the window's length in calls
        fn()
        calls[name] = max(3, math.ceil(window * 1e6 / timed(fn, 3)))
        rises[name] = peak_rise(fn)
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, calls[name]))
    lines = ['%-18s | %10.1f [%9.1f .. %9.1f] | %5d | %9.1f MB | %s'
             % (name, statistics.median(t), min(t), max(t), calls[name], rises[name] / 1e6,
                ' '.join('%.1f' % v for v in t)) for name, t in times.items()]
    return lines, times


def part(K, dev, rounds, window):
    g = torch.Generator().manual_seed(K)
    logits = (4.0 * torch.randn(B, Q, K + 1, generator=g)).to(dev)
    embs = torch.randn(B, Q, C, generator=g).to(dev)
    preds = (6.0 * torch.randn(B, Q, *LOW, generator=g)).to(dev)
    group, n_merged = ([c * 17 // K for c in range(K)], 17) if K > 17 else (None, None)
    fns = {
        'semantic_map': lambda: sem2d.semantic_map(logits, preds, SIZE),
        'torch map': lambda: sem2d.semantic_map_torch(logits, preds, SIZE),
        'semantic_labels': lambda: sem2d.semantic_labels(logits, preds, SIZE, group, n_merged),
        'torch labels': lambda: sem2d.semantic_labels_torch(logits, preds, SIZE, group,
                                                            n_merged),
        'semantic_maps_ds': lambda: sem2d.semantic_maps_ds(logits, embs, preds),
        'torch maps_ds': lambda: sem2d.semantic_maps_ds_torch(logits, embs, preds),
    }
    agree = float((fns['semantic_labels']() == fns['torch labels']()).float().mean())
    err = float((fns['semantic_map']() - fns['torch map']()).abs().max())
    rows, times = measure(fns, rounds, window)
    lines = ['-- B %d, Q %d, K %d, C %d, %s -> %s; max |native - torch| of sem_seg %.2e, labels '
             'equal on %.6f of the pixels' % (B, Q, K, C, LOW, SIZE, err, agree)] + rows
    names = list(fns)
    for nat, ref in zip(names[0::2], names[1::2]):
        below = max(times[nat]) < min(times[ref])
        lines.append('%-18s / %-14s = %.4f; every native round below every torch round: %s'
                     % (nat, ref, statistics.median(times[nat]) / statistics.median(times[ref]),
                        'yes' if below else 'NO'))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window')
    ap.add_argument('--out', help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('sem2d_bench: no ROCm device')
    dev = 'cuda:0'
    lines = ['device %s; %d rounds, windows of >= %.2f s, alternating'
             % (torch.cuda.get_device_name(0), a.rounds, a.window),
             '%-18s | %34s | %5s | %12s | rounds (us/call)'
             % ('structure', 'us/call median [min .. max]', 'calls', 'peak rise')]
    with torch.no_grad():
        for K in (17, 67):
            lines += part(K, dev, a.rounds, a.window)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
