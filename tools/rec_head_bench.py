#!/usr/bin/env python
"""The recognition head of the 2-D branch with its native query path
(``ClipRecHead.hip_query`` / ``VeonOccupancyPath.hip_rec_head``) against the path it
replaces, in the same run: six cameras, 100 queries, CLIP ViT-B/16 widths, for 512 x 1408
and for 256 x 704 images, in both half flavours.

    python tools/rec_head_bench.py [--rounds 5] [--window 0.3] [--out FILE]

    forward_2d off / on      VeonOccupancyPath.forward_2d, ``hip_rec_head`` off / on
    head off, side grid      ClipRecHead.forward as today: bias at the side adapter's grid,
                             resized by the head, torch query path
    head off, clip grid      the torch query path on a bias already at the CLIP grid
    head on, clip grid       the native query path (nine launches per tail block)
    bias decode+resize       MLPMaskDecoder.forward, then the head's resize of B*heads*Q maps
    bias at clip grid        MLPMaskDecoder.forward(bias_size=...): attn_bias_at
    query_attention          veon_query_attention alone (B 6, H 12, Q 100, full bias)
    query_attention_ref      the same arithmetic in torch, in half on the device

Microseconds per call: a host clock around a window of back-to-back calls (at least
``--window`` seconds) that ends in a device synchronise; the structures of a group
alternate within every round, every round is printed, then median [min .. max].  Peak
memory: the rise of ``torch.cuda.max_memory_allocated`` over one call.  Needs a ROCm
device; one process, at most 16 host threads; run it under a ``timeout``."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veon_amd import half, vit_ops  # noqa: E402

B, Q = 6, 100


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
    """Rows of the table for one group of structures, and their per-round times."""
    calls, rises = {}, {}
    for name, fn in fns.items():       # warm-up, and the window's length in calls
        fn()
        calls[name] = max(3, math.ceil(window * 1e6 / timed(fn, 3)))
        rises[name] = peak_rise(fn)
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, calls[name]))
    lines = ['%-22s | %10.1f [%9.1f .. %9.1f] | %5d | %9.1f MB | %s'
             % (name, statistics.median(t), min(t), max(t), calls[name], rises[name] / 1e6,
                ' '.join('%.1f' % v for v in t)) for name, t in times.items()]
    return lines, times


def verdict(times, new, old):
    below = max(times[new]) < min(times[old])
    return ('%-22s / %-22s = %.4f; every round of the first below every round of the second: %s'
            % (new, old, statistics.median(times[new]) / statistics.median(times[old]),
               'yes' if below else 'NO'))


def part(size, dev, rounds, window):
    from veon_amd.models.semantic_net import ClipRecHead
    from veon_amd.models.veon_occ import VeonOccupancyPath
    torch.manual_seed(0)
    net = VeonOccupancyPath(input_size=size, num_cam=B, side_adapter=True).to(dev).eval()
    head, side = net.clip_rec_head, net.side_adapter_network
    images = torch.randn(1, B, 3, *size, device=dev)
    lines = ['-- %s, %d x %d x %d images' % (half.name(), B, size[0], size[1])]

    def fwd(on):
        net.hip_rec_head = on
        try:
            return net.forward_2d(images)
        finally:
            net.hip_rec_head = False
    rows, t = measure({'forward_2d off': lambda: fwd(False),
                       'forward_2d on': lambda: fwd(True)}, rounds, window)
    lines += rows + [verdict(t, 'forward_2d on', 'forward_2d off')]

    # the head alone, on the CLIP features and the decoder's biases of these images
    img = images.flatten(0, 1)
    x = torch.nn.functional.interpolate(img, scale_factor=0.5, mode='bilinear',
                                        align_corners=False)
    outs, hw = net.clip_trunk(x, last_layer_idx=net.clip_first_tail)
    feats = {}
    for i, tok in enumerate(outs):
        ClipRecHead._save(feats, i, tok, hw)
    feature = side.forward_features(img, feats)[0][-1]
    dec = side.mask_decoder
    mode = head.downsample_method
    side_bias = dec(**feature)[1]
    clip_bias = dec(**feature, bias_size=hw, bias_mode=mode)[1]
    lines.append('   CLIP grid %s, bias at the side grid %s, at the CLIP grid %s'
                 % (hw, tuple(side_bias[0].shape), tuple(clip_bias[0].shape)))
    rows, t = measure({
        'head off, side grid': lambda: head(feats, side_bias, normalize=True, hip_query=False),
        'head off, clip grid': lambda: head(feats, clip_bias, normalize=True, hip_query=False),
        'head on, clip grid': lambda: head(feats, clip_bias, normalize=True, hip_query=True),
    }, rounds, window)
    lines += rows + [verdict(t, 'head on, clip grid', 'head off, clip grid'),
                     verdict(t, 'head on, clip grid', 'head off, side grid')]
    rows, t = measure({
        'bias decode+resize': lambda: head._build_attn_biases(dec(**feature)[1], hw),
        'bias at clip grid': lambda: head._build_attn_biases(
            dec(**feature, bias_size=hw, bias_mode=mode)[1], hw),
    }, rounds, window)
    lines += rows + [verdict(t, 'bias at clip grid', 'bias decode+resize')]

    # the kernel alone at the head's shape
    H, Lk = head.resblocks[0].attn.num_heads, hw[0] * hw[1]
    g = torch.Generator().manual_seed(1)
    q_qkv = (torch.randn(B, Q, 3, H, 64, generator=g) * 0.5).to(dev).to(half.dtype())
    mem_kv = (torch.randn(B, Lk + 1, 2, H, 64, generator=g) * 0.5).to(dev).to(half.dtype())
    bias = torch.randn(B, H, Q, Lk, generator=g).to(dev)
    rows, t = measure({
        'query_attention': lambda: vit_ops.query_attention(q_qkv, mem_kv, H, bias, key0=1,
                                                           q_log2=True),
        'query_attention_ref': lambda: vit_ops.query_attention_ref(
            q_qkv, mem_kv, H, bias, key0=1, q_log2=True, dtype=half.dtype()),
    }, rounds, window)
    lines += ['   kernel alone: B %d, H %d, Q %d, Lk %d' % (B, H, Q, Lk)] + rows + \
        [verdict(t, 'query_attention', 'query_attention_ref')]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.3, help='seconds per timed window')
    ap.add_argument('--out', help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('rec_head_bench: no ROCm device')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = 'cuda:0'
    lines = ['device %s; %d rounds, windows of >= %.2f s, alternating'
             % (torch.cuda.get_device_name(0), a.rounds, a.window),
             '%-22s | %34s | %5s | %12s | rounds (us/call)'
             % ('structure', 'us/call median [min .. max]', 'calls', 'peak rise')]
    with torch.no_grad():
        for dtype in (torch.bfloat16, torch.float16):
            with half.use(dtype):
                for size in ((512, 1408), (256, 704)):
                    lines += part(size, dev, a.rounds, a.window)
                    torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
