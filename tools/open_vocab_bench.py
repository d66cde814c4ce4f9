#!/usr/bin/env python
"""The open-vocabulary additions at the VEON shape, in one process, the structures
alternating within every round.

    python tools/open_vocab_bench.py [--rounds 5] [--window 0.3] [--out FILE]

(a) The text tower (ViT-B/16's: width 512, 8 heads, 12 layers, seeded weights) in both half
    flavours, on the fixture vocabulary (tests/golden/open_vocab_tiny.json: 66 descriptions)
    x its 14 templates = 924 prompts, and on one prompt.  No BPE file is at hand, so a
    prompt's length is its number of words + 2 (SOT, EOT), a LOWER bound of its token count:
        native trimmed     ``encode_text`` as it runs by default (L = max(eot) + 1)
        native untrimmed   ``trim=False``: all 77 positions
        mirror fp32        the torch form on the device, 77 positions (what open_clip runs)
    Tokens are host tensors, as the tokenizer returns them.
(b) The grouped tail, B 1, (8, 100, 100) -> (16, 200, 200), K = 67 rows in 17 runs + the
    background row (n_merged 18), the logits as the path hands them over (channels-last
    interior of the classifier GEMM's padded rows):
        occ_labels_grouped          uint8 labels only
        occ_labels_grouped + hist   with the confusion matrix fused in
        occ_classify_grouped        int64 labels + occupancy pair + 18 merged channels
        torch sequence              what a user has without them: F.interpolate of the K
                                    rows, maximum per run, both softmaxes, arg-max, where
        occ_labels (18 rows)        the ungrouped label tail on 18 rows, as context

Microseconds per call: a host clock around a window of back-to-back calls (at least
``--window`` seconds) that ends in a device synchronise, as median [min .. max] over
``--rounds`` rounds.  Needs a ROCm device."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veon_amd import conv3d_ops, half, occ_eval  # noqa: E402
from veon_amd.align_select import group_ids  # noqa: E402
from veon_amd.models.semantic_net.clip_text import ClipTextEncoder  # noqa: E402
from veon_amd.vocabulary import build_vocabulary  # noqa: E402

LOW, SIZE = (8, 100, 100), (16, 200, 200)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls     # us


def measure(fns, rounds, window):
    calls = {}
    for name, fn in fns.items():       # warm-up, and the window's length in calls
        fn()
        calls[name] = max(3, math.ceil(window * 1e6 / timed(fn, 3)))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, calls[name]))
    return ['%-28s | %10.1f [%9.1f .. %9.1f] | %6d'
            % (name, statistics.median(t), min(t), max(t), calls[name])
            for name, t in times.items()], {k: statistics.median(v) for k, v in times.items()}


def prompt_tokens(prompts, ctx=77, vocab=49408):
    g = torch.Generator().manual_seed(0)
    out = torch.zeros((len(prompts), ctx), dtype=torch.long)
    for i, p in enumerate(prompts):
        n = min(len(p.split()), ctx - 2)
        out[i, 0] = vocab - 2
        out[i, 1:1 + n] = torch.randint(1, vocab - 2, (n,), generator=g)
        out[i, 1 + n] = vocab - 1
    return out


def tower_part(dev, rounds, window):
    with open(os.path.join(ROOT, 'tests', 'golden', 'open_vocab_tiny.json')) as f:
        doc = json.load(f)
    _, detailed, _ = build_vocabulary([], doc['categories'])
    prompts = [t.format(d) for t in doc['templates'] for d in detailed]
    sets = {'%d prompts' % len(prompts): prompt_tokens(prompts),
            '1 prompt': prompt_tokens(['a photo of a traffic cone'])}
    lines = []
    for dtype in (torch.bfloat16, torch.float16):
        with half.use(dtype):
            torch.manual_seed(0)
            enc = ClipTextEncoder.from_preset('ViT-B/16').to(dev).eval()
            for label, tok in sets.items():
                L = int(tok.argmax(-1).max()) + 1
                fns = {'native trimmed (L = %d)' % L: lambda: enc.encode_text(tok),
                       'native untrimmed (77)': lambda: enc.encode_text(tok, trim=False),
                       'mirror fp32 (77)': lambda: enc.encode_text(tok, trim=False,
                                                                   native=False)}
                rows, med = measure(fns, rounds, window)
                names = list(fns)
                lines.append('-- text tower, %s, %s' % (half.name(), label))
                lines += rows
                lines.append('trimmed / untrimmed = %.3f, trimmed / mirror = %.3f'
                             % (med[names[0]] / med[names[1]], med[names[0]] / med[names[2]]))
    return lines


def tail_part(dev, rounds, window):
    with open(os.path.join(ROOT, 'tests', 'golden', 'open_vocab_tiny.json')) as f:
        doc = json.load(f)
    reflection = build_vocabulary([], doc['categories'])[2]
    gid, runs = group_ids(reflection)
    group, n_merged, free = gid + [runs], runs + 1, runs
    K = len(group)
    g = torch.Generator().manual_seed(0)
    z, y, x = LOW
    rows = torch.randn(1, z + 2, y + 2, x + 2, (K + 7) // 8 * 8, generator=g).to(dev) * 3
    sem = rows[:, 1:-1, 1:-1, 1:-1, :K].permute(0, 4, 1, 2, 3)
    binv = torch.randn(1, 2, z, y, x, generator=g).to(dev)
    shape = (1, SIZE[2], SIZE[1], SIZE[0])
    gt = torch.randint(0, n_merged, shape, generator=g, dtype=torch.uint8)
    gt[torch.rand(shape, generator=g) < 0.1] = 255
    gt, mask = gt.to(dev), (torch.rand(shape, generator=g) >= 0.3).to(torch.uint8).to(dev)
    hist = torch.zeros((n_merged, n_merged), dtype=torch.int64, device=dev)
    bounds = [(i, i + gid[i:].count(gid[i])) for i in range(len(gid))
              if i == 0 or gid[i] != gid[i - 1]] + [(K - 1, K)]

    def torch_sequence():
        up = F.interpolate(sem, size=SIZE, mode='trilinear', align_corners=False)
        merged = torch.cat([up[:, a:b].amax(1, keepdim=True) for a, b in bounds], dim=1)
        bin_up = F.interpolate(binv, size=SIZE, mode='trilinear', align_corners=False)
        score, cls = torch.softmax(merged, dim=1).max(dim=1)
        keep = (score > 0.0) & (torch.softmax(bin_up, dim=1)[:, 0] > 0.5)
        return torch.where(keep, cls, torch.full_like(cls, free)).permute(0, 3, 2, 1) \
            .contiguous().to(torch.uint8)

    labels = occ_eval.occ_labels_grouped(sem, binv, SIZE, group, n_merged, free)
    assert torch.equal(conv3d_ops.occ_classify_grouped(sem, binv, SIZE, group, n_merged,
                                                       free)[2], labels.long())
    agree = float((torch_sequence() == labels).float().mean())
    sem18 = sem[:, :18]
    fns = {
        'occ_labels_grouped': lambda: occ_eval.occ_labels_grouped(sem, binv, SIZE, group,
                                                                  n_merged, free),
        'occ_labels_grouped + hist': lambda: occ_eval.occ_labels_grouped(
            sem, binv, SIZE, group, n_merged, free, gt, mask, hist),
        'occ_classify_grouped': lambda: conv3d_ops.occ_classify_grouped(
            sem, binv, SIZE, group, n_merged, free),
        'torch sequence': torch_sequence,
        'occ_labels (18 rows)': lambda: occ_eval.occ_labels(sem18, binv, SIZE),
    }
    rows_, med = measure(fns, rounds, window)
    lines = ['-- grouped tail, B 1, %s -> %s, K %d, n_merged %d; labels equal to the torch '
             "sequence's on %.4f of the voxels" % (LOW, SIZE, K, n_merged, agree)]
    lines += rows_
    for name in list(fns)[:3]:
        lines.append('%-28s / torch sequence = %.4f' % (name, med[name] / med['torch sequence']))
    lines.append('%-28s / occ_labels (18 rows) = %.3f'
                 % ('occ_labels_grouped', med['occ_labels_grouped'] / med['occ_labels (18 rows)']))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window')
    ap.add_argument('--out', help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('open_vocab_bench: no ROCm device')
    dev = 'cuda:0'
    lines = ['device %s; %d rounds, windows of >= %.2f s, alternating'
             % (torch.cuda.get_device_name(0), a.rounds, a.window),
             '%-28s | %34s | %6s' % ('structure', 'us/call median [min .. max]', 'calls')]
    with torch.no_grad():
        lines += tower_part(dev, a.rounds, a.window)
        lines += tail_part(dev, a.rounds, a.window)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
