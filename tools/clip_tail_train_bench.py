#!/usr/bin/env python
"""Training step through the CLIP tail (forward + backward) at the two VEON shapes:
(N, T, H, D) = (6, 177, 12, 768) for 256 x 704 images and (6, 705, 12, 768) for 512 x 1408
(11 x 16 and 22 x 32 patch tokens + the class token).  Three subjects, three structures
each, in one process in alternating rounds:

    attention   softmax(scale q k^T + bias) v alone on a raw qkv tensor, the patch-to-patch
                bias (N, H, T - 1, T - 1) requiring a gradient; once with qkv requiring one
                too and once without (``dqkv = None``: the dS-only backward).  The two torch
                structures of this subject are NOT the parent path: they run the
                restatement ``vit_ops.attention_bias_ref`` (matmul, softmax, matmul under
                autograd) on fp32 and on half tensors, after ``build_attn_bias``
    block       one ResidualAttentionBlock(768, 12), trainable, x and the bias requiring
                gradients
    head        ClipRecHead.update_remaining_clip_feats with three tail blocks, frozen block
                weights, biases E E^T formed by torch.matmul from E (N, H, T - 1, 32) that
                requires a gradient (the Gram matmul and its backward are inside the timed
                step, in torch in every structure), the trunk's tokens without a gradient
                and the two feature offsets (N, T - 1, 768) with one, as the HSA network
                hands them over.  (Without offsets nothing but the mask of the first block
                needs a gradient, and torch's fused attention backward raises on that:
                "shape '[72, 177]' is invalid for input of size 0".)

    torch fp32      block, head: the path without the switch, ``build_attn_bias`` +
                    nn.MultiheadAttention in fp32; attention: the restatement in fp32
    torch autocast  block, head: the same under torch.autocast with the build's half dtype;
                    attention: the restatement on half q, k, v
    native          ``ResidualAttentionBlock.hip_train`` on (csrc/attention_train.hip)

    python tools/clip_tail_train_bench.py [--rounds 5] [--steps 5] [--quick]
                                          [--only native] [--subject block] [--tokens 177]

Per structure: ms per step (device events over ``--steps`` back-to-back steps) as median
[min .. max] over ``--rounds`` alternating rounds -- the spread is the yardstick for the
comparison -- and the rise of torch.cuda.max_memory_allocated over one step above the
resident inputs and weights, the gradients the step returns included (those of the step
before are dropped first).  Needs a ROCm device.  Kernel-level times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this tool with ``--quick --only native``."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import half, vit_ops  # noqa: E402
from veon_amd.models.semantic_net.clip_blocks import (  # noqa: E402
    ClipRecHead, ResidualAttentionBlock)

STRUCTURES = ('torch fp32', 'torch autocast', 'native')
SUBJECTS = ('attention', 'attention-ds', 'block', 'head')
GRIDS = {177: (11, 16), 705: (22, 32)}
N, H, D = 6, 12, 768
SCALE = 0.125


def _run(structure, forward, backward):
    def step():
        ResidualAttentionBlock.hip_train = structure == 'native'
        try:
            if structure == 'torch autocast':
                with torch.autocast('cuda', dtype=half.dtype()):
                    out = forward(structure)
            else:
                out = forward(structure)
            return backward(out)
        finally:
            ResidualAttentionBlock.hip_train = False
    return step


def _gram(T, gen, dev):
    E = torch.randn(N, H, T - 1, 32, generator=gen) * 0.5 ** 0.5
    return E.to(dev)


def attention_subject(dev, gen, T, qkv_grad):
    qkv32 = torch.randn(N, T, 3 * D, generator=gen).to(dev)
    qkvh = qkv32.to(half.dtype())
    E = _gram(T, gen, dev)
    bias = (E @ E.transpose(-2, -1)).contiguous()
    gout = torch.randn(N, T, D, generator=gen).to(dev)
    state = {}

    def forward(structure):
        state['b'] = bias.detach().requires_grad_()
        x = (qkv32 if structure == 'torch fp32' else qkvh).detach().requires_grad_(qkv_grad)
        state['x'] = x
        if structure == 'native':
            return vit_ops.attention_bias_train(x, state['b'], H, SCALE, border=1)
        full = ClipRecHead.build_attn_bias(state['b']).view(N, H, T, T)
        return vit_ops.attention_bias_ref(x, full, H, SCALE)

    def backward(out):
        out.backward(gout.to(out.dtype))
        return state['b'].grad
    return 'attention with bias, (N, T, H) = (%d, %d, %d), qkv %s; torch = the restatement ' \
        'attention_bias_ref' % (
            N, T, H, 'requires a gradient' if qkv_grad else 'needs no gradient (dS only)'), \
        forward, backward, state.clear


def block_subject(dev, gen, T):
    blk = ResidualAttentionBlock(D, H).to(dev)
    x = torch.randn(T, N, D, generator=gen).to(dev)
    E = _gram(T, gen, dev)
    bias = (E @ E.transpose(-2, -1)).contiguous()
    gout = torch.randn(T, N, D, generator=gen).to(dev)
    state = {}

    def forward(structure):
        state['x'] = x.detach().requires_grad_()
        state['b'] = bias.detach().requires_grad_()
        if structure == 'native':
            return blk(state['x'], attn_mask=state['b'])
        return blk(state['x'], attn_mask=ClipRecHead.build_attn_bias(state['b']))

    def backward(out):
        blk.zero_grad(set_to_none=True)
        out.backward(gout.to(out.dtype))
        return state['x'].grad

    def clear():
        state.clear()
        blk.zero_grad(set_to_none=True)
    return 'ResidualAttentionBlock(%d, %d), trainable, %d x %d tokens' % (D, H, N, T), \
        forward, backward, clear


def head_subject(dev, gen, T):
    hw = GRIDS[T]
    blocks = torch.nn.ModuleList([ResidualAttentionBlock(D, H) for _ in range(3)])
    head = ClipRecHead(blocks, torch.nn.LayerNorm(D), torch.nn.Parameter(torch.randn(D, 512)
                                                                         * D ** -0.5))
    head = head.to(dev)
    for p in head.parameters():
        p.requires_grad_(False)
    feat = torch.randn(N, D, *hw, generator=gen).to(dev)
    cls = torch.randn(1, N, D, generator=gen).to(dev)
    Es = [_gram(T, gen, dev) for _ in range(3)]
    offs = (torch.randn(2, N, T - 1, D, generator=gen) * 0.1).to(dev)
    gout = torch.randn(N, 512, *hw, generator=gen).to(dev)
    state = {}

    def forward(structure):
        state['E'] = [e.detach().requires_grad_() for e in Es]
        attns = [e @ e.transpose(-2, -1) for e in state['E']]
        outs = {0: feat, '0_cls_token': cls}
        state['o'] = offs.detach().requires_grad_()
        head.update_remaining_clip_feats(outs, state['o'], attns, keep_layers=())
        return outs['clip_feat_proj']

    def backward(out):
        out.backward(gout.to(out.dtype))
        return state['E'][0].grad
    return 'ClipRecHead.update_remaining_clip_feats, 3 frozen blocks, Gram biases with a ' \
        'gradient, %d x (%d x %d + 1) tokens' % ((N,) + hw), forward, backward, state.clear


def timed(fn, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps     # ms


def peak_rise(fn, clear):
    """Rise of the peak over one step above what is resident before it.  ``clear`` drops the
    previous step's leaves and their gradients first, so that the gradients this step
    allocates count."""
    clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise / 1e6        # MB


def measure(title, forward, backward, clear, names, rounds, steps):
    print(title)
    fns = {n: _run(n, forward, backward) for n in names}
    for n in names:          # warm-up: library algorithm searches, workspaces, allocator
        for _ in range(2):
            fns[n]()
    times = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            times[n].append(timed(fns[n], steps))
    peaks = {n: peak_rise(fns[n], clear) for n in names}
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
    ap.add_argument('--only', choices=STRUCTURES, default=None)
    ap.add_argument('--subject', choices=SUBJECTS, default=None)
    ap.add_argument('--tokens', type=int, choices=sorted(GRIDS), default=None)
    a = ap.parse_args()
    rounds, steps = (2, 2) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('clip_tail_train_bench: no ROCm device')
    dev = 'cuda:0'
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    names = [a.only] if a.only else list(STRUCTURES)
    print('device %s; %s operands; %d rounds of %d steps, structures alternating' % (
        torch.cuda.get_device_name(0), half.name(), rounds, steps))
    for T in ([a.tokens] if a.tokens else sorted(GRIDS)):
        for subject in ([a.subject] if a.subject else SUBJECTS):
            if subject == 'attention':
                title, forward, backward, clear = attention_subject(dev, gen, T, True)
            elif subject == 'attention-ds':
                title, forward, backward, clear = attention_subject(dev, gen, T, False)
            elif subject == 'block':
                title, forward, backward, clear = block_subject(dev, gen, T)
            else:
                title, forward, backward, clear = head_subject(dev, gen, T)
            measure(title, forward, backward, clear, names, rounds, steps)
            clear()
            del forward, backward, clear
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
