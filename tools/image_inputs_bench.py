#!/usr/bin/env python
"""The camera inputs of one sample (veon_amd.image_inputs) at the VEON shape: six decoded
900 x 1600 frames -> ``imgs`` 6 x 3 x 512 x 1408 (resize to 792 x 1408, window from row 280,
``mmlab``), and the depth branch 256 x 704 (``midas``) or 252 x 700 (``depthanythingv2``).

    python tools/image_inputs_bench.py [--rounds 5] [--window 0.5] [--quick]

In one process, alternating per round:

    native            ``prepare_images`` (csrc/image_inputs.hip), ``imgs`` only: 2 launches
    native +midas     with the depth branch, midas: 4 launches
    native +dav2      with the depth branch, depthanythingv2: 5 launches
    h pass, v finish, depth h, depth v midas, cubic tail    the launches one by one
    mirror, mirror +midas   ``prepare_images_torch`` on the same device
    host x1, host x6  where Pillow is installed: the reference's host sequence (resize,
                      crop, numpy normalisation, depth resize, midas) per camera, on one
                      thread and on six of the usable cores
    h2d               the copy of the 52 MB fp32 ``imgs`` (pinned) the host sequence needs

Microseconds per call as median [min .. max] over ``--rounds`` rounds; device structures
are timed with device events around a window of back-to-back calls that lasts at least
``--window`` seconds, the host sequence with the wall clock (``--quick``: 2 rounds of
50 ms).  Needs a ROCm device."""
import argparse
import math
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veon_amd import _lib, image_inputs as ii  # noqa: E402

CAMS, H, W = 6, 900, 1600
RESIZE_DIMS, CROP, FH, FW, DH, DW = (1408, 792), (0, 280, 1408, 792), 512, 1408, 256, 704
# the 235 / 347 ms of the issue: the Pillow / numpy sequence for six cameras in two runs on
# one thread of the development machine, without JPEG decoding
DEVELOPMENT_HOST_MS = (235, 347)


def make_frames(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (1, CAMS, H, W, 3), generator=g, dtype=torch.uint8)


def host_camera(Image, frame):
    """One camera of the reference's sequence -> (imgs plane, depth plane) as numpy."""
    mean, std = (np.array(v, np.float32) for v in ii.NORMS['mmlab'])
    img = Image.fromarray(frame).resize(RESIZE_DIMS).crop(CROP)
    x = np.array(img).astype(np.float32)[..., ::-1]
    x = ((x - mean) * (1 / np.float64(std)).astype(np.float32)).transpose(2, 0, 1)
    d = (np.array(img.resize((DW, DH))) / 255.).astype(np.float32)[..., ::-1]
    d = ((d - np.float32(0.5)) * np.float32(2)).transpose(2, 0, 1)
    return np.ascontiguousarray(x), np.ascontiguousarray(d)


def timed_device(fn, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps     # us


def timed_host(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5, help='seconds per timed window')
    ap.add_argument('--quick', action='store_true', help='2 rounds of 50 ms')
    a = ap.parse_args()
    rounds, window = (2, 0.05) if a.quick else (a.rounds, a.window)
    if not torch.cuda.is_available():
        sys.exit('image_inputs_bench: no ROCm device')
    dev = torch.device('cuda:0')
    cpu = make_frames()
    frames = cpu.to(dev)
    kw = dict(resize_dims=RESIZE_DIMS, crop=CROP, flip=False, norm='mmlab')
    midas = dict(kw, depth_size=(DH, DW), depth_norm='midas')
    dav2 = dict(kw, depth_size=(DH, DW), depth_norm='depthanythingv2')
    full = ii.prepare_images(frames, return_canvas=True, **dav2)
    out = {k: torch.empty_like(v) for k, v in full.items()}
    out_midas = dict(out, depth_img_inputs=torch.empty((1, CAMS, 3, DH, DW), device=dev))
    canvas, depth_u8 = full['canvas'].view(CAMS, FH, FW, 3), full['depth_canvas'].view(
        CAMS, DH, DW, 3)

    # the launches one by one, on the tensors of the whole call
    r0, r1 = ii._needed_rows(H, RESIZE_DIMS[1], CROP[1], CROP[3])
    bx, kx = ii.device_coeffs(W, RESIZE_DIMS[0], dev)
    by, ky = ii.device_coeffs(H, RESIZE_DIMS[1], dev)
    dbx, dkx = ii.device_coeffs(FW, DW, dev)
    dby, dky = ii.device_coeffs(FH, DH, dev)
    tmp = torch.empty((CAMS, r1 - r0, RESIZE_DIMS[0], 3), dtype=torch.uint8, device=dev)
    dtmp = torch.empty((CAMS, FH, DW, 3), dtype=torch.uint8, device=dev)
    win, dwin = ii._windows([CROP], [False]), ii._windows([(0, 0, DW, DH)], [False])
    lut, dlut = ii.device_lut('mmlab', dev), ii.device_lut('midas', dev)
    src = frames.view(CAMS, H, W, 3)
    fns = {
        'native': lambda: ii.prepare_images(frames, out=out, **kw),
        'native +midas': lambda: ii.prepare_images(frames, out=out_midas, **midas),
        'native +dav2': lambda: ii.prepare_images(frames, out=out, **dav2),
        'h pass': lambda: _lib.launch('veon_image_resample_h', dev, src, CAMS, H, W,
                                      RESIZE_DIMS[0], r0, r1 - r0, bx, kx, kx.shape[1], tmp),
        'v finish': lambda: _lib.launch('veon_image_resample_v_finish', dev, tmp, CAMS, r1 - r0,
                                        RESIZE_DIMS[0], r0, RESIZE_DIMS[1], by, ky, ky.shape[1],
                                        win, FH, FW, lut, 1, out['canvas'], out['imgs']),
        'depth h': lambda: _lib.launch('veon_image_resample_h', dev, canvas, CAMS, FH, FW, DW, 0,
                                       FH, dbx, dkx, dkx.shape[1], dtmp),
        'depth v midas': lambda: _lib.launch('veon_image_resample_v_finish', dev, dtmp, CAMS, FH,
                                             DW, 0, DH, dby, dky, dky.shape[1], dwin, DH, DW,
                                             dlut, 1, None, out_midas['depth_img_inputs']),
        'cubic tail': lambda: _lib.launch('veon_image_cubic_norm', dev, depth_u8, CAMS, DH, DW,
                                          252, 700, 1, *ii.DEPTHANYTHING_MEAN,
                                          *ii.DEPTHANYTHING_STD, out['depth_img_inputs']),
        'mirror': lambda: ii.prepare_images_torch(frames, **kw),
        'mirror +midas': lambda: ii.prepare_images_torch(frames, **midas),
    }
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        arrays = [cpu[0, n].numpy() for n in range(CAMS)]
        pool = ThreadPoolExecutor(CAMS)
        fns['host x1'] = lambda: [host_camera(Image, f) for f in arrays]
        fns['host x6'] = lambda: list(pool.map(lambda f: host_camera(Image, f), arrays))
    pinned = torch.zeros((CAMS, 3, FH, FW)).pin_memory()
    landing = torch.empty((CAMS, 3, FH, FW), device=dev)
    fns['h2d'] = lambda: landing.copy_(pinned, non_blocking=True)

    mir = ii.prepare_images_torch(frames, return_canvas=True, **midas)
    nat = ii.prepare_images(frames, return_canvas=True, **midas)
    print('device %s; %d rounds, windows of >= %.2f s, structures alternating; host threads %d'
          % (torch.cuda.get_device_name(0), rounds, window, torch.get_num_threads()))
    print('%d frames %d x %d -> %d x %d (rows %d .. %d of the frame read), depth %d x %d'
          % (CAMS, H, W, FH, FW, r0, r1 - 1, DH, DW))
    print('native against the mirror: ' + ', '.join(
        '%s differs on %d' % (k, int((nat[k] != mir[k]).sum())) for k in sorted(mir)))
    if Image is not None:
        x, d = host_camera(Image, cpu[0, 0].numpy())
        print('native against the host sequence, camera 0: imgs differs on %d, depth on %d'
              % (int((nat['imgs'][0, 0].cpu() != torch.from_numpy(x)).sum()),
                 int((nat['depth_img_inputs'][0, 0].cpu() != torch.from_numpy(d)).sum())))
    else:
        print('Pillow is not installed here: the host sequence is not timed; on one thread of '
              'the development machine it took %d and %d ms in two runs (not this machine)'
              % DEVELOPMENT_HOST_MS)
    steps = {}
    for name, fn in fns.items():
        host = name.startswith('host')
        timer = timed_host if host else timed_device
        fn()
        steps[name] = max(2 if host else 10, math.ceil(window * 1e6 / timer(fn, 2)))
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            timer = timed_host if name.startswith('host') else timed_device
            times[name].append(timer(fn, steps[name]))
    print('%-14s | %36s | %8s' % ('structure', 'us/call median [min .. max]', 'calls'))
    for name, t in times.items():
        print('%-14s | %12.1f [%10.1f .. %10.1f] | %8d'
              % (name, statistics.median(t), min(t), max(t), steps[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    for nat_name, mir_name in (('native', 'mirror'), ('native +midas', 'mirror +midas')):
        print('every %s round below every %s round: %s (max %.1f against min %.1f)'
              % (nat_name, mir_name,
                 'yes' if max(times[nat_name]) < min(times[mir_name]) else 'no',
                 max(times[nat_name]), min(times[mir_name])))
    imgs_bytes = CAMS * 3 * FH * FW * 4
    depth_bytes = CAMS * 3 * DH * DW * 4
    read_bytes = CAMS * (r1 - r0) * W * 3
    print('native: %.1f MB of imgs written in %.1f us = %.0f GB/s of output; with %.1f MB of '
          'frame rows read, %.0f GB/s in all'
          % (imgs_bytes / 1e6, med['native'], imgs_bytes / med['native'] / 1e3,
             read_bytes / 1e6, (imgs_bytes + read_bytes) / med['native'] / 1e3))
    print('native +midas: %.1f MB of imgs + depth inputs written in %.1f us = %.0f GB/s of '
          'output' % ((imgs_bytes + depth_bytes) / 1e6, med['native +midas'],
                      (imgs_bytes + depth_bytes) / med['native +midas'] / 1e3))
    if Image is not None:
        print('host sequence x6 + h2d against native +midas: %.1f us against %.1f us'
              % (med['host x6'] + med['h2d'], med['native +midas']))


if __name__ == '__main__':
    main()
