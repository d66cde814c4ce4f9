#!/usr/bin/env python
"""Training step of the HSA network (forward + backward) at the VEON shape: 6 cameras,
512 x 1408 images, 8 x 8 patches -> 64 x 176 tokens of 384 channels.  Three subjects,
three structures each, in one process in alternating rounds:

    block    one ConvBlock(384, 384) on 6 x (64 x 176) tokens with ``residual``
    head     FeedForward(384, 384, 2304) on 6 x (64 x 176) tokens through
             ``forward_resized`` to 16 x 44 (head_attn of the AttnManipulateBlock)
    network  HighresSideAdaptorNetwork.build() on 6 x 3 x 512 x 1408 (``--small``:
             256 x 704), random gradients seeded on ``attns`` and ``supp``

    torch fp32      what a training step runs without the switches (nn.Conv2d / Linear /
                    LayerNorm)
    torch autocast  the same modules under torch.autocast with the build's half dtype
    native          every ``hip_train`` switch on: ConvBlock (csrc/conv2d_train.hip),
                    FeedForward and the blocks' token LayerNorms (csrc/linear_train.hip)

``--subject wgrad`` times the linear weight gradient alone at the heads' two shapes.

    python tools/hsa_train_bench.py [--rounds 5] [--steps 5] [--quick] [--small]
                                    [--only native] [--subject block]

Per structure: ms per step (forward + backward, input gradient included, device events
over ``--steps`` back-to-back steps) as median [min .. max] over ``--rounds`` alternating
rounds -- the spread is the yardstick for the comparison -- and the rise of
torch.cuda.max_memory_allocated over one step above the resident inputs.  Needs a ROCm
device.  Kernel-level times come from a separate ``rocprofv3 --kernel-trace --stats``
run of this tool with ``--quick --only native``."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import half  # noqa: E402
from veon_amd.models.semantic_net.hsa_network import (  # noqa: E402
    AttnManipulateBlock, ConvBlock, FeedForward, HighresSideAdaptorBlock,
    HighresSideAdaptorNetwork)

STRUCTURES = ('torch fp32', 'torch autocast', 'native')
SUBJECTS = ('block', 'head', 'network')
SWITCHED = (ConvBlock, FeedForward, HighresSideAdaptorBlock, AttnManipulateBlock)


def _set_native(on):
    for cls in SWITCHED:
        cls.hip_train = on


def _run(structure, forward, backward):
    def step():
        _set_native(structure == 'native')
        try:
            if structure == 'torch autocast':
                with torch.autocast('cuda', dtype=half.dtype()):
                    out = forward()
            else:
                out = forward()
            return backward(out)
        finally:
            _set_native(False)
    return step


def block_subject(dev, gen):
    blk = ConvBlock(384, 384).to(dev).train()
    x = torch.randn(6, 64 * 176, 384, generator=gen).to(dev)
    res = torch.randn(6, 64 * 176, 384, generator=gen).to(dev)
    gout = torch.randn(6, 64 * 176, 384, generator=gen).to(dev)
    state = {}

    def forward():
        state['x'] = x.detach().requires_grad_()
        return blk(state['x'], (64, 176), residual=res)

    def backward(out):
        out.backward(gout.to(out.dtype))
        return state['x'].grad
    return 'ConvBlock(384, 384), training mode, 6 x (64 x 176) tokens + residual', \
        forward, backward, blk


def head_subject(dev, gen):
    ff = FeedForward(384, 384, 2304).to(dev).train()
    x = torch.randn(6, 64 * 176, 384, generator=gen).to(dev)
    gout = torch.randn(6, 2304, 16, 44, generator=gen).to(dev)
    state = {}

    def forward():
        state['x'] = x.detach().requires_grad_()
        return ff.forward_resized(state['x'], (64, 176), (16, 44))

    def backward(out):
        ff.zero_grad(set_to_none=True)
        out.backward(gout.to(out.dtype))
        return state['x'].grad
    return 'FeedForward(384, 384, 2304), training mode, 6 x (64 x 176) tokens, ' \
        'forward_resized to 16 x 44', forward, backward, ff


def wgrad_times(dev, gen, iters=20):
    """The linear weight gradient alone (kernel + reduce, device events over ``iters``
    back-to-back calls after two warm-ups) and its share of the 2.5 PFLOP/s bf16 peak."""
    from veon_amd import vit_ops
    print('linear weight gradient, %d calls back to back' % iters)
    for M, K, N in ((67584, 384, 384), (4224, 384, 2304)):
        dy = torch.randn(M, N, generator=gen).to(half.dtype()).to(dev)
        x = torch.randn(M, K, generator=gen).to(half.dtype()).to(dev)
        out = torch.empty(N, K, device=dev)
        for _ in range(2):
            vit_ops.linear_wgrad(dy, x, out)
        ms = sorted(timed(lambda: vit_ops.linear_wgrad(dy, x, out), iters) for _ in range(5))
        tflops = 2.0 * M * K * N / (ms[2] * 1e-3) / 1e12
        print('(M, K, N) = (%6d, %4d, %4d) | %8.4f ms median [%8.4f .. %8.4f] | %7.1f TFLOP/s'
              ' | %5.1f %% of peak' % (M, K, N, ms[2], ms[0], ms[-1], tflops, tflops / 25.0))


def network_subject(dev, gen, small):
    size = (256, 704) if small else (512, 1408)
    net = HighresSideAdaptorNetwork.build(input_size=size).to(dev).train()
    image = torch.randn(6, 3, *size, generator=gen).to(dev)
    h, w = size[0] // 32, size[1] // 32          # CLIP's token grid on the half-size image
    clip = {i: torch.randn(6, 768, h, w, generator=gen).to(dev) for i in (1, 3, 6, 9)}
    state = {}

    def forward():
        return net(image, clip)

    def backward(out):
        _, attns, supp = out
        if 'g' not in state:     # random gradients on both outputs, drawn once
            state['g'] = (torch.randn(attns.shape, generator=gen).to(dev),
                          torch.randn(supp.shape, generator=gen).to(dev))
        ga, gs = state['g']
        net.zero_grad(set_to_none=True)
        torch.autograd.backward([attns, supp], [ga.to(attns.dtype), gs.to(supp.dtype)])
        return net.patch_embed.proj.weight.grad
    return 'HighresSideAdaptorNetwork.build(), training mode, image 6 x 3 x %d x %d' % size, \
        forward, backward, net


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


def measure(title, forward, backward, names, rounds, steps):
    print(title)
    fns = {n: _run(n, forward, backward) for n in names}
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
    if 'native' in med:
        for n in names:
            if n != 'native':
                print('native / %s = %.3f; spread of the rounds: %s %.3f ms, native %.3f ms'
                      % (n, med['native'] / med[n], n, max(times[n]) - min(times[n]),
                         max(times['native']) - min(times['native'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 2 steps (profiler run)')
    ap.add_argument('--small', action='store_true', help='network on 256 x 704 images')
    ap.add_argument('--only', choices=STRUCTURES, default=None)
    ap.add_argument('--subject', choices=SUBJECTS + ('wgrad',), default=None)
    a = ap.parse_args()
    rounds, steps = (2, 2) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('hsa_train_bench: no ROCm device')
    dev = 'cuda:0'
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    names = [a.only] if a.only else list(STRUCTURES)
    print('device %s; %s operands; %d rounds of %d steps, structures alternating' % (
        torch.cuda.get_device_name(0), half.name(), rounds, steps))
    for subject in ([a.subject] if a.subject else SUBJECTS):
        if subject == 'wgrad':
            wgrad_times(dev, gen)
            continue
        if subject == 'block':
            title, forward, backward, keep = block_subject(dev, gen)
        elif subject == 'head':
            title, forward, backward, keep = head_subject(dev, gen)
        else:
            title, forward, backward, keep = network_subject(dev, gen, a.small)
        measure(title, forward, backward, names, rounds, steps)
        del forward, backward, keep
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
