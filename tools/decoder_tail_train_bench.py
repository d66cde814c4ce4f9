#!/usr/bin/env python
"""Forward + backward of the decoder tail of the occupancy training step at the VEON
shape: both prediction heads and the three terms of ``OccLossFB.loss_voxel``, with the
native switches (``_PredHead3D.hip_train``, ``OccLossFB.hip_train``) on and off, in the
same process, alternating.

    python tools/decoder_tail_train_bench.py [--rounds 5] [--steps 10] [--fp16] [--quick]

B = 1, 256 channels on 8 x 100 x 100, ``clip_outdim`` 512 and 768, occupancy grid
(16, 200, 200), N = 40 000 alignment entries drawn as tools/align_loss_bench.py draws
them (the discrete selection of ``Proj2Dto3DLoss`` is replaced by that fixed list: it is
the same no-grad code in every variant).  Variants:
    on        switches on; the heads read the body's padded half storage, as they do
              behind a run of native ``ResBlock3D`` s
    on+pack   switches on; the heads are given an fp32 volume and pack it themselves
    off       switches off, fp32: the parent path (MIOpen 1x1x1 convs + BatchNorm3d)
    autocast  switches off under ``torch.autocast`` in the flavour's half dtype
``bin_occ_loss`` alone ((1, 2, 8, 100, 100) -> (16, 200, 200)) is timed against the torch
sequence as well.  Per variant: ms per step (device events around ``--steps`` back-to-back
steps, at least 50 in all) as median [min .. max] over ``--rounds`` alternating rounds, and
the rise of torch.cuda.max_memory_allocated over one step.  Needs a ROCm device."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from align_loss_bench import entries, peak_rise, timed  # noqa: E402
from veon_amd import conv3d_ops, half  # noqa: E402
from veon_amd.models.semantic_net.align_net_body import (PredHead3DOcc, PredHead3DSem,  # noqa: E402
                                                          _PredHead3D)
from veon_amd.models.semantic_net.occ_loss import OccLossFB  # noqa: E402
from veon_amd.occ_bin_loss import bin_occ_loss, bin_occ_loss_torch  # noqa: E402

LOW, OCC, EMBED, N, K = (8, 100, 100), (16, 200, 200), 256, 40000, 18


def report(name, times, rise):
    print('%-10s | %9.3f [%8.3f .. %8.3f] | %9.1f' % (name, statistics.median(times), min(times),
                                                     max(times), rise))


def alternate(fns, rounds, steps):
    for fn in fns.values():          # warm-up: allocator, workspaces, MIOpen's choices
        fn()
        fn()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, steps))
    for name, fn in fns.items():
        report(name, times[name], peak_rise(fn))
    return {name: statistics.median(t) for name, t in times.items()}


def tail_case(clip_outdim, rounds, steps, dev):
    torch.manual_seed(clip_outdim)
    occ_head = PredHead3DOcc(EMBED, 2).to(dev).train()
    sem_head = PredHead3DSem(EMBED, clip_outdim).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, EMBED) + LOW, generator=g).relu().to(dev)
    storage = conv3d_ops.pack(x).storage
    table = torch.randn(K, clip_outdim, generator=g).to(dev)
    vox, lab = entries('uniform', N, N + clip_outdim, dev)
    sel = [dict(voxels=vox, labels=lab, weights=torch.full((N,), 1.0 / N, device=dev),
                n_det=N // 2)]
    labels = torch.randint(0, 19, (1,) + OCC[::-1], generator=g).to(torch.uint8).to(dev)
    labels[0, :10] = 255
    loss = OccLossFB(grid_config=None, priority=[1.0] * 17, ov_class_number=8).to(dev)
    loss.proj2dto3dloss.select = lambda *a, **k: sel
    loss._bin_weights_on(torch.device(dev))
    meta = dict(sem_seg_ds=None, img_inputs=None, class_reflection=None,
                ov_classifier_weight=table)
    params = list(occ_head.parameters()) + list(sem_head.parameters())

    def step(on, from_storage=False, autocast=False):
        _PredHead3D.hip_train = loss.hip_train = on
        for p in params:
            p.grad = None
        if from_storage:
            leaf = storage.detach().requires_grad_()
            inp = (leaf, tuple(x.shape))
        else:
            leaf = x.detach().requires_grad_()
            inp = leaf
        with torch.autocast('cuda', dtype=half.dtype(), enabled=autocast):
            bin_low, feat = occ_head(inp), sem_head(inp)
        out = loss.loss_voxel(dict(feat_occ=feat.float(), bin_occ=bin_low, occ_size=OCC), labels,
                              meta, 'c_0')
        sum(out.values()).backward()
        _PredHead3D.hip_train = loss.hip_train = False
        return leaf.grad

    print('clip_outdim %d: feat_occ %.0f MB in fp32' % (clip_outdim,
                                                       clip_outdim * 80000 * 4 / 1e6))
    return alternate({'on': lambda: step(True, True), 'on+pack': lambda: step(True),
                      'off': lambda: step(False), 'autocast': lambda: step(False, autocast=True)},
                     rounds, steps)


def loss_case(rounds, steps, dev):
    g = torch.Generator().manual_seed(2)
    logits = (3 * torch.randn((1, 2) + LOW, generator=g)).to(dev)
    labels = torch.randint(0, 19, (1,) + OCC[::-1], generator=g).to(torch.uint8).to(dev)
    labels[0, :10] = 255
    cw = torch.tensor([1.0, 0.5], device=dev)

    def step(fn):
        leaf = logits.detach().requires_grad_()
        fn(leaf, labels, cw, OCC).backward()
        return leaf.grad
    print('bin_occ_loss alone, (1, 2, 8, 100, 100) -> (16, 200, 200)')
    return alternate({'native': lambda: step(bin_occ_loss), 'torch': lambda: step(bin_occ_loss_torch)},
                     rounds, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--fp16', action='store_true', help='the fp16 flavour of the library')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 3 steps (profiler run)')
    a = ap.parse_args()
    rounds, steps = (2, 3) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('decoder_tail_train_bench: no ROCm device')
    dev = 'cuda:0'
    with half.use(torch.float16 if a.fp16 else torch.bfloat16):
        print('device %s; flavour %s; %d rounds of %d steps (%d steps per variant), variants '
              'alternating' % (torch.cuda.get_device_name(0), half.name(), rounds, steps,
                               rounds * steps))
        print('%-10s | %28s | %9s' % ('variant', 'ms/step median [min .. max]', 'peak MB'))
        med = loss_case(rounds, steps, dev)
        print('%-10s native / torch = %.3f' % ('', med['native'] / med['torch']))
        for clip_outdim in (512, 768):
            med = tail_case(clip_outdim, rounds, steps, dev)
            print('%-10s on / off = %.3f, on / autocast = %.3f, on+pack / off = %.3f' % (
                '', med['on'] / med['off'], med['on'] / med['autocast'],
                med['on+pack'] / med['off']))


if __name__ == '__main__':
    main()
