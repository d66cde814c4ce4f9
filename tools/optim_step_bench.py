#!/usr/bin/env python
"""The parameter update of one training iteration (veon_amd.optim) on the parameter sets of
the VEON-L occupancy path: gradient-norm clip (max_norm 5) + AdamW (lr 1e-4, weight decay
1e-2) + the weight EMA of MEGVIIEMAHook over every floating state_dict entry.

    python tools/optim_step_bench.py [--rounds 5] [--window 0.3] [--quick] [--out FILE]

Parameter sets (modules built as the model builds them, synthetic gradients):

    body+heads   AlignBody3D(256, 4) + PredHead3DOcc(256, 2) + PredHead3DSem(256, 768)
    hsa          HighresSideAdaptorNetwork.build(dim 384, CLIP width 1024, 3 fusion steps)
    dinov2-lora  DINOv2Adaptor('vitl', lora_r=16): only lora_A / lora_B train, the frozen
                 rest is EMA-only
    all          the three together

In one process, alternating per round:

    native          FusedAdamW(max_norm=5, ema=ModelEMA(model)).step() + ema.update()
    foreach+loop    clip_grad_norm_ + torch.optim.AdamW (its default on a device: foreach)
                    + the reference's EMA loop (three torch ops per entry)
    fused+loop      the same with AdamW(fused=True)
    foreach+feach   clip_grad_norm_ + AdamW + the EMA as two torch._foreach calls
    fused+feach     the same with AdamW(fused=True): the strongest torch sequence

Microseconds per iteration, wall clock around a window of back-to-back iterations that ends
in a device synchronise (the torch sequences are bound by their launches, so the host is
part of what is measured), as median [min .. max] over the rounds; kernel launches per
iteration counted by torch.profiler in one extra iteration; bytes against the floor of 36 B
per trained element (read g, p, m, v, e; write p, m, v, e) and 12 B per EMA-only element.
The native step reads the gradients a second time for the norm (4 B per trained element on
top of the floor).  All five structures step the same parameters from the same gradients,
the views of the native optimizer's arena; their norm (below 1) is below max_norm,
so ``clip_grad_norm_`` of the torch sequences multiplies them by exactly 1 and every
structure sees the same gradients in every iteration, while the parameters drift.  Needs a
ROCm device."""
import argparse
import copy
import math
import os
import statistics
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import optim  # noqa: E402

HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
MAX_NORM, DECAY = 5.0, 0.999
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                   'r23_optim_step_bench.txt')


def body_heads():
    from veon_amd.models.semantic_net.align_net_body import (AlignBody3D, PredHead3DOcc,
                                                             PredHead3DSem)
    return nn.ModuleDict(dict(body=AlignBody3D(256, 4), occ=PredHead3DOcc(256, 2),
                              sem=PredHead3DSem(256, 768)))


def hsa():
    from veon_amd.models.semantic_net.hsa_network import HighresSideAdaptorNetwork
    return HighresSideAdaptorNetwork.build(
        dim=384, clip_dim=1024, mlp_dim=384, input_size=(256, 704),
        fusion_map=('0->3->6', '1->9->12', '2->15->18'), manip_supp_dim=384, num_heads=16,
        manip_attn_layers=6)


def dinov2_lora():
    from veon_amd.models.depth_anything.dinov2 import DINOv2Adaptor
    enc = DINOv2Adaptor('vitl', lora_r=16)
    for n, p in enc.named_parameters():
        p.requires_grad_('lora_' in n)
    return enc


SETS = {'body+heads': lambda: body_heads(), 'hsa': lambda: hsa(),
        'dinov2-lora': lambda: dinov2_lora(),
        'all': lambda: nn.ModuleDict(dict(a=body_heads(), b=hsa(), c=dinov2_lora()))}


class LoopEMA:
    """The reference's ModelEMA.update (ema.py:48-59) on a deep copy."""

    def __init__(self, model, foreach):
        self.ema = copy.deepcopy(model).eval()
        self.model, self.updates, self.foreach = model, 0, foreach
        pairs = [(v, model.state_dict()[k]) for k, v in self.ema.state_dict().items()
                 if v.dtype.is_floating_point]
        self.e, self.m = [a for a, _ in pairs], [b for _, b in pairs]

    def update(self):
        with torch.no_grad():
            self.updates += 1
            d = DECAY * (1 - math.exp(-self.updates / 2000))
            if self.foreach:
                torch._foreach_mul_(self.e, d)
                torch._foreach_add_(self.e, self.m, alpha=1.0 - d)
                return
            msd = self.model.state_dict()
            for k, v in self.ema.state_dict().items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1.0 - d) * msd[k].detach()


def torch_iteration(params, opt, ema):
    def run():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        ema.update()
    return run


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def launches(fn):
    """(number, names) of the device activities torch.profiler records in one iteration
    (kernels, and memsets or copies if there are any); (None, []) when it records none."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return (len(names) or None), names


def bench_set(name, rounds, window, emit):
    dev = 'cuda:0'
    torch.manual_seed(0)
    model = SETS[name]().to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    ema = optim.ModelEMA(model, decay=DECAY)
    native = optim.FusedAdamW(params, max_norm=MAX_NORM, ema=ema, **HYPER)
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:                     # p.grad: the bound view (the padding stays zero)
        p.grad.copy_(torch.randn(p.shape, device=dev, generator=g) * 1e-4)
    counts = native.counts()
    n_train, n_rest = counts['trained'], counts['ema_only']
    floor = 36 * n_train + 12 * n_rest

    def native_iteration():
        native.step()
        ema.update()

    fns = {'native': native_iteration}
    for label, kw, foreach_ema in (('foreach+loop', {}, False), ('fused+loop', {'fused': True}, False),
                                   ('foreach+feach', {}, True), ('fused+feach', {'fused': True}, True)):
        opt = torch.optim.AdamW(params, **HYPER, **kw)
        fns[label] = torch_iteration(params, opt, LoopEMA(model, foreach_ema))
    emit('')
    emit('== %s: %d trained tensors (%.2f M elements), %d state_dict entries EMA-only (%.2f M '
         'elements); %d records; floor %.1f MB per iteration'
         % (name, len(params), n_train / 1e6, counts['ema_only_entries'], n_rest / 1e6,
            counts['records'], floor / 1e6))
    steps, count = {}, {}
    for label, fn in fns.items():
        fn()
        fn()
        steps[label] = max(5, math.ceil(window * 1e6 / timed(fn, 3)))
        count[label], names = launches(fn)
        if label == 'native':
            native_names = names
    times = {label: [] for label in fns}
    for _ in range(rounds):
        for label, fn in fns.items():
            times[label].append(timed(fn, steps[label]))
    emit('%-14s | %34s | %-40s | %9s | %9s' % ('structure', 'us/iteration median [min .. max]',
                                               'rounds', 'launches', 'floor GB/s'))
    for label, t in times.items():
        emit('%-14s | %12.1f [%9.1f .. %9.1f] | %-40s | %9s | %9.0f'
             % (label, statistics.median(t), min(t), max(t), ' '.join('%.0f' % v for v in t),
                count[label] if count[label] is not None else 'n/m',
                floor / statistics.median(t) / 1e3))
    emit('device activities of a native iteration: %s' % ', '.join(native_names))
    best = min((k for k in times if k != 'native'), key=lambda k: statistics.median(times[k]))
    emit('strongest torch sequence: %s; every native round below every round of it: %s '
         '(native max %.1f, its min %.1f); ratio of medians %.2f'
         % (best, 'yes' if max(times['native']) < min(times[best]) else 'no',
            max(times['native']), min(times[best]),
            statistics.median(times[best]) / statistics.median(times['native'])))
    emit('native moves %.1f MB (floor + the norm pass): %.0f GB/s at its median'
         % ((floor + 4 * counts['arena']) / 1e6,
            (floor + 4 * counts['arena']) / statistics.median(times['native']) / 1e3))
    assert torch.isfinite(native.grad_norm).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 50 ms')
    ap.add_argument('--sets', default=','.join(SETS))
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    rounds, window = (2, 0.05) if a.quick else (a.rounds, a.window)
    if not torch.cuda.is_available():
        sys.exit('optim_step_bench: no ROCm device')
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit('device %s; %d rounds, windows of >= %.2f s, structures alternating; wall clock ending '
         'in a synchronise; clip max_norm %g, AdamW %s, EMA decay %g'
         % (torch.cuda.get_device_name(0), rounds, window, MAX_NORM, HYPER, DECAY))
    for name in a.sets.split(','):
        bench_set(name, rounds, window, emit)
        torch.cuda.empty_cache()
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
