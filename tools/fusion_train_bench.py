#!/usr/bin/env python
"""Forward + backward of the lift's 2-D fusion layer (``CatFusionLift``) at the VEON shape,
with the native switch (``CatFusionLift.hip_train``) on and off, in the same process,
alternating.

    python tools/fusion_train_bench.py [--rounds 5] [--steps 10] [--fp16] [--quick]

x1 (6, 384, 64, 176) and x2 (6, 768, 16, 44), both resized to 32 x 88, out = 256: 16 896
tokens of 1152 channels.  Both inputs and all eight parameters ask for a gradient; the
upstream gradient is a fixed channels-last fp32 tensor, as the lift's backward hands it
over.  Variants:
    native    the switch on (csrc/fusion_train.hip)
    off       the switch off, fp32: the parent path
    autocast  the switch off under ``torch.autocast`` in the flavour's half dtype
Per variant: ms per step (device events around ``--steps`` back-to-back steps) as median
[min .. max] over ``--rounds`` alternating rounds, and the rise of
torch.cuda.max_memory_allocated over one step.  Run the command twice and compare the
medians: a gap below the spread between the two runs is no gap.  Needs a ROCm device."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decoder_tail_train_bench import alternate  # noqa: E402
from veon_amd import half  # noqa: E402
from veon_amd.models.semantic_net.fusion_layers import CatFusionLift  # noqa: E402

X1, X2, SIZE, OUT = (6, 384, 64, 176), (6, 768, 16, 44), (32, 88), 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--fp16', action='store_true', help='the fp16 flavour of the library')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 3 steps (profiler run)')
    a = ap.parse_args()
    rounds, steps = (2, 3) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('fusion_train_bench: no ROCm device')
    dev = 'cuda:0'
    torch.manual_seed(0)
    mod = CatFusionLift(X1[1], X2[1], OUT).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn(X1, generator=g).to(dev), torch.randn(X2, generator=g).to(dev)
    G = torch.randn((X1[0],) + SIZE + (OUT,), generator=g).to(dev).permute(0, 3, 1, 2)
    params = list(mod.parameters())

    def step(on, autocast=False):
        CatFusionLift.hip_train = on
        for p in params:
            p.grad = None
        a1, a2 = x1.detach().requires_grad_(), x2.detach().requires_grad_()
        with torch.autocast('cuda', dtype=half.dtype(), enabled=autocast):
            out = mod(a1, a2, SIZE)
        out.float().backward(G)
        CatFusionLift.hip_train = False
        return a1.grad, a2.grad

    with half.use(torch.float16 if a.fp16 else torch.bfloat16):
        print('device %s; flavour %s; %d rounds of %d steps (%d steps per variant), variants '
              'alternating' % (torch.cuda.get_device_name(0), half.name(), rounds, steps,
                               rounds * steps))
        print('CatFusionLift(%d, %d, %d), %s + %s -> %s: the resized rows are %.0f MB in fp32'
              % (X1[1], X2[1], OUT, X1, X2, SIZE,
                 X1[0] * SIZE[0] * SIZE[1] * (X1[1] + X2[1]) * 4 / 1e6))
        print('%-10s | %28s | %9s' % ('variant', 'ms/step median [min .. max]', 'peak MB'))
        med = alternate({'native': lambda: step(True), 'off': lambda: step(False),
                         'autocast': lambda: step(False, autocast=True)}, rounds, steps)
        print('%-10s native / off = %.3f, native / autocast = %.3f' % (
            '', med['native'] / med['off'], med['native'] / med['autocast']))


if __name__ == '__main__':
    main()
