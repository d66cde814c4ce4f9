#!/usr/bin/env python
"""Training step (forward + backward, parameters and the current frame's input requiring
gradients, train-mode BN) of the temporal fusion at the VEON shape, B = 1, 256 channels,
8 x 100 x 100 voxels:

    deform   one TemporalDeformable(256): both inputs require gradients
    fusion   TemporalFusionMultiFrame(256, seqs=1) with one past frame (no gradient)

Three structures in one process, alternating rounds:

    torch fp32      the definition (F.grid_sample on a (B*heads*8, 2*hd, D, H, W) copy)
    torch autocast  the same modules under torch.autocast with the build's half dtype
    native          TemporalDeformable.hip_train = TemporalFusionMultiFrame.hip_train = True
                    (csrc/temporal_train.hip); absent on a tree without the switches

    python tools/temporal_train_bench.py [--rounds 5] [--steps 3] [--quick]
                                         [--only native] [--workload fusion]

Per workload and structure: ms per step as median [min .. max] over ``--rounds``
alternating rounds (device events over ``--steps`` back-to-back steps) -- the spread is the
yardstick for the comparison -- and the rise of torch.cuda.max_memory_allocated over one
step above the resident inputs.  Then the two new kernels alone at that shape (device
events around ``conv3d_ops.deform_attention_bwd`` without and with the dKV gather) and
their share of the native fusion step, which backs two of them.  Needs a ROCm device."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import conv3d_ops, half  # noqa: E402
from veon_amd.models.semantic_net import temporal_fusion as tfm  # noqa: E402

STRUCTURES = ('torch fp32', 'torch autocast', 'native')
SHAPE = (1, 256, 8, 100, 100)
HAS_NATIVE = hasattr(tfm.TemporalFusionMultiFrame, 'hip_train')


def set_switches(on):
    if HAS_NATIVE:
        tfm.TemporalDeformable.hip_train = tfm.TemporalFusionMultiFrame.hip_train = on


def step_fn(mod, run, tensors, needs, gout, structure):
    def step():
        set_switches(structure == 'native')
        for p in mod.parameters():
            p.grad = None
        ins = [t.detach().requires_grad_(n) for t, n in zip(tensors, needs)]
        if structure == 'torch autocast':
            with torch.autocast('cuda', dtype=half.dtype()):
                out = run(mod, ins)
        else:
            out = run(mod, ins)
        out.backward(gout.to(out.dtype))
        set_switches(False)
        return ins[0].grad
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


def bench(tag, mod, run, tensors, needs, gout, names, rounds, steps):
    fns = {n: step_fn(mod, run, tensors, needs, gout, n) for n in names}
    for n in names:          # warm-up: MIOpen's algorithm search, workspaces, allocator
        for _ in range(2):
            fns[n]()
    times = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            times[n].append(timed(fns[n], steps))
    peaks = {n: peak_rise(fns[n]) for n in names}
    print('%-7s %-15s | %33s | %10s' % ('', 'structure', 'ms/step median [min .. max]', 'peak MB'))
    for n in names:
        t = times[n]
        print('%-7s %-15s | %10.3f [%9.3f .. %9.3f] | %10.1f' % (
            tag, n, statistics.median(t), min(t), max(t), peaks[n]))
    med = {n: statistics.median(t) for n, t in times.items()}
    if 'native' in med:
        for n in names:
            if n != 'native':
                print('%s: native / %s = %.3f; spread of the rounds: %s %.3f ms, native %.3f ms'
                      % (tag, n, med['native'] / med[n], n, max(times[n]) - min(times[n]),
                         max(times['native']) - min(times['native'])))
    return med


def kernel_times(dev, rounds, steps, fusion_ms):
    B, C, Z, Y, X = SHAPE
    gen = torch.Generator().manual_seed(3)
    vol = lambda c, s=1.0: conv3d_ops.pack((torch.randn(B, c, Z, Y, X, generator=gen) * s).to(dev))  # noqa: E731
    kv, q, off, dout = vol(2 * C), vol(C), vol(128, 1.5), vol(C)
    outs = (kv.like(), q.like(), off.like())
    vox = lambda: conv3d_ops.deform_attention_bwd(kv, q, off, dout, 4, need_dkv=False, out=outs)  # noqa: E731
    both = lambda: conv3d_ops.deform_attention_bwd(kv, q, off, dout, 4, out=outs)  # noqa: E731
    fwd = lambda: conv3d_ops.deform_attention(kv, q, off, 4, out=outs[1])  # noqa: E731
    for f in (vox, both, fwd):
        f()
    t = {k: statistics.median(timed(f, max(steps, 5)) for _ in range(rounds))
         for k, f in (('vox', vox), ('both', both), ('fwd', fwd))}
    dkv = t['both'] - t['vox']
    print('kernels at %s, 4 heads, 128 offset channels (median of %d rounds):' % (SHAPE, rounds))
    print('  forward gather                         %8.3f ms' % t['fwd'])
    print('  per-voxel backward (+ two halo passes) %8.3f ms' % t['vox'])
    print('  dKV gather (both - per-voxel)          %8.3f ms' % dkv)
    if fusion_ms:
        print('  share of the native fusion step (two calls each): per-voxel %.1f %%, dKV %.1f %%'
              % (200 * t['vox'] / fusion_ms, 200 * dkv / fusion_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 2 steps')
    ap.add_argument('--only', choices=STRUCTURES, default=None)
    ap.add_argument('--workload', choices=('deform', 'fusion'), default=None)
    a = ap.parse_args()
    rounds, steps = (2, 2) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('temporal_train_bench: no ROCm device')
    dev = 'cuda:0'
    names = [a.only] if a.only else list(STRUCTURES)
    if not HAS_NATIVE:
        names = [n for n in names if n != 'native']
    print('device %s; %s operands; %d rounds of %d steps, structures alternating%s' % (
        torch.cuda.get_device_name(0), half.name(), rounds, steps,
        '' if HAS_NATIVE else '; this tree has no native training path'))
    gen = torch.Generator().manual_seed(1)
    frames = [torch.randn(*SHAPE, generator=gen).relu().to(dev) for _ in range(2)]
    gout = torch.randn(*SHAPE, generator=gen).to(dev)
    fusion_ms = None
    if a.workload in (None, 'deform'):
        torch.manual_seed(0)
        mod = tfm.TemporalDeformable(256).to(dev).train()
        bench('deform', mod, lambda m, ins: m(ins[0], ins[1]), frames, [True, True], gout,
              names, rounds, steps)
    if a.workload in (None, 'fusion'):
        torch.manual_seed(0)
        mod = tfm.TemporalFusionMultiFrame(256, seqs=1).to(dev).train()
        med = bench('fusion', mod, lambda m, ins: m(ins[0], ins[1:]), frames, [True, False],
                    gout, names, rounds, steps)
        fusion_ms = med.get('native')
    if HAS_NATIVE and 'native' in names:
        kernel_times(dev, rounds, steps, fusion_ms)


if __name__ == '__main__':
    main()
