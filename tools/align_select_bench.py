#!/usr/bin/env python
"""The entry selection of the feature-alignment loss (``Proj2Dto3DLoss.select``) at the
VEON shape: the torch mirror against the native selection (``hip_select``), in the same
process, alternating.

    python tools/align_select_bench.py [--rounds 5] [--steps 10] [--quick]

B = 1, the six-camera rig of veon_amd/synthetic.py at 512 x 1408, GRID_VEON (200 x 200 x 16
voxels, 3.84 M (camera, voxel) pairs, depth 1-45 m).  Labels are drawn so that the number
of kept entries lands near 40 000 and near 200 000, the two entry counts of
tools/align_loss_bench.py: the share of labelled voxels is target / (kept entries with
every voxel labelled).  ``sem_seg_ds`` has 24 two-dimensional classes merged into 17 on a
32 x 88 map (the image over 16: the side adapter's mask resolution -- an assumption of this
tool, as is the class count; the cost of the native classify step is linear in both).
``feat_low`` is (1, 512, 8, 100, 100) in channels-last rows.  Stage 2 off and on (threshold
0.985: on random features nothing is confident, the work is the same).

Per case and structure: ms per call of ``select`` (device events around ``--steps``
back-to-back calls, so the host's waits for the device are inside the window) as median
[min .. max] over ``--rounds`` alternating rounds, the number of kept entries and the rise
of torch.cuda.max_memory_allocated over one call.  Last: one whole ``OccLossFB.loss_voxel``
forward + backward (``hip_train`` on, C = 512) with the real selection in both settings.
Needs a ROCm device.  Kernel-level times come from a separate ``rocprofv3 --kernel-trace
--stats`` run of this tool with ``--quick``."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _inputs  # noqa: E402,F401  (puts the repository root on sys.path)
from align_loss_bench import peak_rise, timed  # noqa: E402
from veon_amd import synthetic  # noqa: E402
from veon_amd.models.semantic_net.occ_loss import OccLossFB  # noqa: E402

LOW, OCC, SIZE, SEM, C = (8, 100, 100), (16, 200, 200), (512, 1408), (32, 88), 512
REFLECTION = [0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 14, 15, 16, 16]
PRIORITY = [1.0, 3.0, 2.5, 1.5, 4.0, 2.0, 3.5, 5.0, 1.2, 2.2, 1.0, 0.5, 0.8, 0.6, 0.7, 1.1, 0.9]


def make_inputs(dev):
    rig = synthetic.make_rig(1, 6, SIZE)
    eye = torch.eye(4).repeat(1, 6, 1, 1)
    t = lambda a: a.to(dev)     # noqa: E731
    images = torch.zeros(1).expand(1, 6, 3, *SIZE)          # only its size is read
    img_inputs = [images, t(eye), t(eye), t(rig['intrins']), t(rig['post_rots']),
                  t(rig['post_trans']), t(rig['bda']), t(eye), t(eye.clone()),
                  t(rig['sensor2ego']), t(rig['ego2global'])]
    g = torch.Generator().manual_seed(0)
    sem = (2.0 * torch.randn((1, 6, len(REFLECTION)) + SEM, generator=g)).to(dev)
    feat = (torch.sigmoid(2 * torch.randn((1,) + LOW + (C,), generator=g)) - 0.5).to(dev)
    table = torch.randn(len(REFLECTION) + 1, C, generator=g).to(dev)
    bin_low = (3 * torch.randn((1, 2) + LOW, generator=g)).to(dev)
    return img_inputs, sem, feat.permute(0, 4, 1, 2, 3), table, bin_low


def draw_labels(share, seed, dev, ignored=0.03):
    """``share`` of the voxels labelled, ``ignored`` of them 255, the rest free"""
    g = torch.Generator().manual_seed(seed)
    Zo, Yo, Xo = OCC
    labels = torch.randint(0, 17, (1, Xo, Yo, Zo), generator=g)
    kind = torch.rand((1, Xo, Yo, Zo), generator=g)
    labels[kind >= share] = 17
    labels[kind > 1 - ignored] = 255
    return labels.to(torch.uint8).to(dev)


def alternate(fns, rounds, steps):
    for fn in fns.values():
        fn()
        fn()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--quick', action='store_true', help='2 rounds of 3 steps (profiler run)')
    a = ap.parse_args()
    rounds, steps = (2, 3) if a.quick else (a.rounds, a.steps)
    if not torch.cuda.is_available():
        sys.exit('align_select_bench: no ROCm device')
    dev = 'cuda:0'
    img_inputs, sem, feat, table, bin_low = make_inputs(dev)
    loss = OccLossFB(grid_config=synthetic.GRID_VEON, priority=PRIORITY, ov_class_number=8,
                     high_conf_thr=0.985, stage2_start=2, hip_train=True)
    mod = loss.proj2dto3dloss

    def select(on, labels):
        mod.hip_select = on
        return mod.select(feat, sem, img_inputs, labels, REFLECTION, table, OCC)

    def kept(sel):
        return int(sel['det'].sum() + sel['soft'].sum() + sel['ignored'].sum()) - 1

    mod.epoch = 0
    everything = kept(select(True, draw_labels(2.0, 1, dev, 0.0))[0])
    print('device %s; %d rounds of %d calls, structures alternating' % (
        torch.cuda.get_device_name(0), rounds, steps))
    print('grid %s, 6 cameras at %s: %d pairs, %d in view; sem_seg_ds %s x %d classes'
          % (OCC, SIZE, 6 * 640000, everything, SEM, len(REFLECTION)))
    print('%-7s %-8s %-9s | %28s | %9s' % ('stage 2', 'kept', 'structure',
                                           'ms/call median [min .. max]', 'peak MB'))
    for target in (40000, 200000):
        labels = draw_labels(target / everything, target, dev)
        for stage2 in (False, True):
            mod.epoch = 3 if stage2 else 0
            a_, b_ = select(False, labels)[0], select(True, labels)[0]
            # unprotected data: an fp32 near-tie may fall differently in the two structures
            same = a_['voxels'].shape == b_['voxels'].shape and a_['n_det'] == b_['n_det'] and \
                torch.equal(a_['voxels'], b_['voxels']) and torch.equal(a_['labels'], b_['labels'])
            n = kept(b_)
            print('%-7s %-8d lists of the two structures identical: %s' % (
                'on' if stage2 else 'off', n, 'yes' if same else 'no (%d / %d entries)' % (
                    a_['voxels'].shape[0], b_['voxels'].shape[0])))
            fns = {'torch': lambda: select(False, labels), 'native': lambda: select(True, labels)}
            times = alternate(fns, rounds, steps)
            for name, fn in fns.items():
                t = times[name]
                print('%-7s %-8d %-9s | %9.3f [%8.3f .. %8.3f] | %9.1f' % (
                    'on' if stage2 else 'off', n, name, statistics.median(t), min(t), max(t),
                    peak_rise(fn)))
            print('%-27s native / torch = %.3f' % ('', statistics.median(times['native'])
                                                    / statistics.median(times['torch'])))

    # the whole loss step with the real selection
    labels = draw_labels(40000 / everything, 40000, dev)
    mod.epoch = 3
    meta = dict(sem_seg_ds=sem, img_inputs=img_inputs, class_reflection=REFLECTION,
                ov_classifier_weight=table)

    def step(on):
        mod.hip_select = on
        leaf = feat.detach().requires_grad_()
        b = bin_low.detach().requires_grad_()
        out = loss.loss_voxel(dict(feat_occ=leaf, bin_occ=b, occ_size=OCC), labels, meta, 'c_0')
        sum(out.values()).backward()
        return leaf.grad

    print('OccLossFB.loss_voxel forward + backward (hip_train on, stage 2 on, C = %d), '
          'selection included' % C)
    fns = {'torch': lambda: step(False), 'native': lambda: step(True)}
    times = alternate(fns, rounds, steps)
    for name, fn in fns.items():
        t = times[name]
        print('%-7s %-8s %-9s | %9.3f [%8.3f .. %8.3f] | %9.1f' % (
            'on', '~40000', name, statistics.median(t), min(t), max(t), peak_rise(fn)))
    print('%-27s native / torch = %.3f' % ('', statistics.median(times['native'])
                                            / statistics.median(times['torch'])))


if __name__ == '__main__':
    main()
