#!/usr/bin/env python
"""Training step of the DepthAnythingV2 encoder (DINOv2 ViT-L with LoRA, forward +
backward) at the VEON shape: 6 images of 901 tokens.  Three subjects:

    attention  the attention forward + backward alone at B6 T901, H16 and H12: the native
               kernels (csrc/attention_train.hip) against torch's half
               scaled_dot_product_attention and against the explicit
               softmax(q k^T) v formulation of the module under torch.autocast
    block      one ViT-L block, Block(1024, 16, init_values=1.0, lora_r=16)
    encoder    DINOv2Adaptor('vitl', lora_r=16): 24 blocks on 6 x 3 x 238 x 742 images
               (17 x 53 patches + class token = 901 tokens), get_intermediate_layers

and three structures for the last two, in one process in alternating rounds:

    torch fp32      what a training step runs without the switch
    torch autocast  the same modules under torch.autocast with the build's half dtype
    native          ``Block.hip_train`` on

    python tools/vit_train_bench.py [--rounds 5] [--steps 5] [--quick] [--only native]
                                    [--subject block] [--depth 24]

Per structure: ms per step (device events over ``--steps`` back-to-back steps) as median
[min .. max] over ``--rounds`` alternating rounds -- the spread is the yardstick for the
comparison -- and the rise of torch.cuda.max_memory_allocated over one step above the
resident inputs.  On a tree without the switch "native" is torch fp32 and the attention
subject is skipped.  Needs a ROCm device.  Kernel-level times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this tool with ``--quick --only native``."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import half, vit_ops  # noqa: E402
from veon_amd.models.depth_anything.dinov2 import Block, DINOv2Adaptor  # noqa: E402

STRUCTURES = ('torch fp32', 'torch autocast', 'native')
SUBJECTS = ('attention', 'block', 'encoder')
B, T = 6, 901


def _run(structure, forward, backward):
    def step():
        Block.hip_train = structure == 'native'
        try:
            if structure == 'torch autocast':
                with torch.autocast('cuda', dtype=half.dtype()):
                    out = forward()
            else:
                out = forward()
            return backward(out)
        finally:
            Block.hip_train = False
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


def table(title, fns, rounds, steps, ratio_to='native'):
    """``fns``: {name: step}.  Warm-up, alternating rounds, one table."""
    print(title)
    names = list(fns)
    for n in names:
        for _ in range(2):
            fns[n]()
    times = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            times[n].append(timed(fns[n], steps))
    peaks = {n: peak_rise(fns[n]) for n in names}
    print('%-24s | %30s | %10s' % ('structure', 'ms/step median [min .. max]', 'peak MB'))
    for n in names:
        t = times[n]
        print('%-24s | %9.3f [%8.3f .. %8.3f] | %10.1f' % (
            n, statistics.median(t), min(t), max(t), peaks[n]))
    med = {n: statistics.median(t) for n, t in times.items()}
    if ratio_to in med:
        for n in names:
            if n != ratio_to:
                print('%s / %s = %.3f; spread of the rounds: %s %.3f ms, %s %.3f ms'
                      % (ratio_to, n, med[ratio_to] / med[n], n, max(times[n]) - min(times[n]),
                         ratio_to, max(times[ratio_to]) - min(times[ratio_to])))
    return med


def attention_subject(dev, gen, rounds, steps):
    if not hasattr(vit_ops, 'attention_bwd'):
        print('attention: this tree has no native attention backward; skipped')
        return
    scale = 0.125
    for H in (16, 12):
        qkv = torch.randn(B, T, 3 * H * 64, generator=gen).to(half.dtype()).to(dev)
        dout = torch.randn(B, T, H * 64, generator=gen).to(half.dtype()).to(dev)
        ws = torch.empty(B, H, vit_ops.attention_stats_len(T), device=dev)
        dqkv = torch.empty_like(qkv)

        def native():
            out, lse = vit_ops.attention_fwd_lse(qkv, H, scale)
            return vit_ops.attention_bwd(qkv, out, dout, lse, H, scale, dqkv=dqkv, workspace=ws)

        def sdpa():
            x = qkv.detach().requires_grad_()
            q, k, v = x.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
            o = F.scaled_dot_product_attention(q, k, v, scale=scale)
            o.transpose(1, 2).reshape(B, T, H * 64).backward(dout)
            return x.grad

        def explicit():
            x = qkv.detach().float().requires_grad_()
            with torch.autocast('cuda', dtype=half.dtype()):
                o = vit_ops.attention_ref(x, H, scale)
            o.backward(dout.to(o.dtype))
            return x.grad
        med = table('attention forward + backward, B%d T%d H%d, head dim 64' % (B, T, H),
                    {'native': native, 'torch half SDPA': sdpa,
                     'explicit softmax autocast': explicit}, rounds, steps)
        # forward 4 B H T^2 64 flop, backward 10 B H T^2 64 (five products of the same size)
        tflops = 14.0 * B * H * T * T * 64 / (med['native'] * 1e-3) / 1e12
        print('native: %.1f TFLOP/s of products, %.1f %% of the 2.5 PFLOP/s bf16 peak'
              % (tflops, tflops / 25.0))


def block_subject(dev, gen):
    blk = Block(1024, 16, init_values=1.0, lora_r=16).to(dev).train()
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith('lora_B'):
                p.normal_(0, 0.02)
    x = torch.randn(B, T, 1024, generator=gen).to(dev)
    gout = torch.randn(B, T, 1024, generator=gen).to(dev)
    state = {}

    def forward():
        state['x'] = x.detach().requires_grad_()
        return blk(state['x'])

    def backward(out):
        blk.zero_grad(set_to_none=True)
        out.backward(gout.to(out.dtype))
        return state['x'].grad
    return 'Block(1024, 16, init_values=1.0, lora_r=16), training mode, %d x %d tokens' \
        % (B, T), forward, backward, blk


def encoder_subject(dev, gen, depth):
    enc = DINOv2Adaptor('vitl', lora_r=16)
    if depth < len(enc.blocks):
        enc.blocks = enc.blocks[:depth]
    enc = enc.to(dev).train()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith('lora_B'):
                p.normal_(0, 0.02)
    img = torch.randn(B, 3, 238, 742, generator=gen).to(dev)
    n = len(enc.blocks)
    taps = [n // 4 - 1 if n >= 4 else 0, n // 2 - 1 if n >= 2 else 0, 3 * n // 4 - 1, n - 1]
    taps = sorted(set(t for t in taps if t >= 0))
    state = {}

    def forward():
        return enc.get_intermediate_layers(img, taps, return_class_token=True)

    def backward(outs):
        flat = [t for pair in outs for t in pair]
        if 'g' not in state:
            state['g'] = [torch.randn(t.shape, generator=gen).to(dev) for t in flat]
        enc.zero_grad(set_to_none=True)
        torch.autograd.backward(flat, [g.to(t.dtype) for g, t in zip(state['g'], flat)])
        return enc.blocks[0].attn.qkv.lora_A.grad
    return "DINOv2Adaptor('vitl', lora_r=16), %d blocks, training mode, images %d x 3 x 238 x " \
        '742 (%d tokens), taps %s' % (n, B, T, taps), forward, backward, enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 2 steps (profiler run)')
    ap.add_argument('--only', choices=STRUCTURES, default=None)
    ap.add_argument('--subject', choices=SUBJECTS, default=None)
    ap.add_argument('--depth', type=int, default=24, help='blocks of the encoder subject')
    a = ap.parse_args()
    rounds, steps = (2, 2) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('vit_train_bench: no ROCm device')
    dev = 'cuda:0'
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    names = [a.only] if a.only else list(STRUCTURES)
    print('device %s; %s operands; %d rounds of %d steps, structures alternating; '
          'Block.hip_train %s' % (torch.cuda.get_device_name(0), half.name(), rounds, steps,
                                  'present' if 'hip_train' in vars(Block) else 'ABSENT'))
    for subject in ([a.subject] if a.subject else SUBJECTS):
        if subject == 'attention':
            attention_subject(dev, gen, rounds, steps)
            continue
        if subject == 'block':
            title, forward, backward, keep = block_subject(dev, gen)
        else:
            title, forward, backward, keep = encoder_subject(dev, gen, a.depth)
        table(title, {n: _run(n, forward, backward) for n in names}, rounds, steps)
        del forward, backward, keep
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
