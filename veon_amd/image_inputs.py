"""The camera inputs of VEON: the pipeline step ``PrepareImageInputs``
(mmdet3d/datasets/pipelines/loading.py:1073-1329) from decoded uint8 frames: Pillow's
``Image.resize`` (8-bit bicubic with antialiasing) bit for bit, the crop window, the
optional flip, the normalised ``imgs``, the depth branch's ``depth_img_inputs`` and the
``post_rots`` / ``post_trans`` the lift reads.

Pillow's 8-bit resampling is integer arithmetic on coefficient tables that depend on the
two sizes alone (``resize_coeffs``); ``pil_resize_torch`` restates it in integer torch ops
on any device, and on a ROCm device ``prepare_images`` runs it natively
(csrc/image_inputs.hip: the horizontal pass of the rows the window needs, then the vertical
pass fused with window, flip and normalisation).  The reference's normalisations of the
transformed image (``mmlab``, ``clipsan``, ``midas``) are functions of a byte: the host
tabulates them in the reference's arithmetic (``norm_lut``), the kernel looks them up.

Unpinned, because the packages are absent where this was written: mmcv's ``imnormalize``
(restated from its source as one fp32 subtraction and one fp32 multiplication), OpenCV's
``INTER_CUBIC`` of the depthanythingv2 branch (``cubic_norm_torch`` states the definition
used) and pyquaternion's rotation matrix (``quaternion_rotation_matrix``).

Not supported (``ValueError``): ``rotate != 0`` (no VEON config uses it) and a crop window
that leaves the resized image (Pillow pads it with zeros)."""
import math

import numpy as np
import torch

from . import _lib, depth_cache

PRECISION_BITS = 22                # Pillow's 32 - 8 - 2
MAX_WINDOWS = _lib.IMAGE_MAX_WINDOWS

NORMS = {
    'mmlab': ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
    'clipsan': ((122.7709, 116.7460, 104.0937), (68.5005, 66.6322, 70.3232)),
}
DEPTHANYTHING_MEAN, DEPTHANYTHING_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# host tables per (in, out); device copies per (in, out, device) and (norm, device);
# UPLOADS counts the host-to-device copies (in steady state a call makes none)
_COEFFS, _DEVICE_COEFFS, _DEVICE_LUTS = {}, {}, {}
UPLOADS = 0


# ------------------------------------------------------------------ Pillow's tables
def _bicubic(x):
    """Pillow's ``bicubic_filter`` (a = -0.5) in its operation order, float64."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resize_coeffs(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for one axis of a bicubic
    resize of the whole image, in C double order -> (bounds (out, 2), kk (out, ksize)),
    int32 CPU tensors: first tap and tap count of every output index, and the coefficients
    in 22-bit fixed point rounded half away from zero (0 beyond the count).  Cached."""
    key = (int(in_size), int(out_size))
    if key in _COEFFS:
        return _COEFFS[key]
    n_in, n_out = key
    if n_in <= 0 or n_out <= 0:
        raise ValueError('sizes must be positive, got %d -> %d' % key)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)       # (int): truncates
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, _bicubic(((x + xmin[:, None]) - center[:, None] + 0.5) / fs), 0.0)
    ww = np.zeros(n_out, np.float64)
    for t in range(ksize):                                                  # index order
        ww = ww + w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    one = float(1 << PRECISION_BITS)
    kk = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one))
    kk = np.where(live, kk, 0.0).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    _COEFFS[key] = (torch.from_numpy(bounds), torch.from_numpy(kk))
    return _COEFFS[key]


def device_coeffs(in_size, out_size, device):
    """``resize_coeffs`` on ``device``, uploaded once per (in, out, device)."""
    global UPLOADS
    device = torch.device(device)
    if device.type == 'cpu':
        return resize_coeffs(in_size, out_size)
    key = (int(in_size), int(out_size), str(device))
    tab = _DEVICE_COEFFS.get(key)
    if tab is None:
        bounds, kk = resize_coeffs(in_size, out_size)
        tab = _DEVICE_COEFFS[key] = (bounds.to(device), kk.to(device))
        UPLOADS += 2
    return tab


# ------------------------------------------------------------------ normalisation tables
def _norm_spec(norm):
    """-> (hashable key, mean, std) of a byte-table normalisation."""
    if isinstance(norm, str):
        if norm == 'midas':
            return norm, None, None
        if norm not in NORMS:
            raise ValueError('unknown normalisation %r' % (norm,))
        return (norm,) + NORMS[norm]
    mean, std = (tuple(float(v) for v in t) for t in norm)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError('mean and std must have three entries')
    return (mean, std), mean, std


def norm_lut(norm):
    """The table lut[c][u] (3, 256) fp32 of output channel c at byte u, in the reference's
    arithmetic.  ``mmlab`` / ``clipsan`` / (mean, std): mmcv's ``imnormalize`` on the fp32
    image, ``(f32(u) - f32(mean[c])) * f32(1 / f64(f32(std[c])))``.  ``midas``
    (loading.py:1037-1045): the same on ``f32(f64(u) / 255.)`` with mean = std = 0.5.  The
    channel swap (``to_rgb=True`` on an image that is RGB already) is the reader's."""
    _, mean, std = _norm_spec(norm)
    if mean is None:
        x = (np.arange(256, dtype=np.float64) / 255.).astype(np.float32)
        mean, std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
    else:
        x = np.arange(256, dtype=np.float32)
    mean32, std32 = np.array(mean, np.float32), np.array(std, np.float32)
    stdinv = (1 / np.float64(std32)).astype(np.float32)
    lut = (x[None, :] - mean32[:, None]) * stdinv[:, None]
    assert lut.dtype == np.float32
    return torch.from_numpy(lut)


def device_lut(norm, device):
    global UPLOADS
    device = torch.device(device)
    key = (_norm_spec(norm)[0], str(device))
    lut = _DEVICE_LUTS.get(key)
    if lut is None:
        lut = norm_lut(norm).to(device)
        if device.type != 'cpu':
            UPLOADS += 1
        _DEVICE_LUTS[key] = lut
    return lut


def apply_lut_torch(img_u8, lut):
    """img (..., h, w, 3) uint8, lut (3, 256) -> (..., 3, h, w) fp32 with the reference's
    channel swap: output channel c reads input channel 2 - c."""
    idx = img_u8.long()
    return torch.stack([lut[c][idx[..., 2 - c]] for c in range(3)], -3)


# ------------------------------------------------------------------ torch mirror
def _pass_torch(img, bounds, kk, dim, first_row=0):
    """One resampling pass of Pillow along ``dim`` of a uint8 tensor, in int32."""
    n_in = img.shape[dim]
    shape = [1] * img.dim()
    shape[dim] = bounds.shape[0]
    acc = None
    for t in range(kk.shape[1]):
        idx = (bounds[:, 0].long() - first_row + t).clamp_(0, n_in - 1)   # kk = 0 past the count
        term = img.index_select(dim, idx).to(torch.int32) * kk[:, t].reshape(shape)
        acc = term + (1 << (PRECISION_BITS - 1)) if acc is None else acc + term
    return (acc >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def _needed_rows(n_in, n_out, y0, y1):
    """Source rows [r0, r1) the vertical pass of output rows [y0, y1) reads."""
    if n_in == n_out:
        return y0, y1
    bounds = resize_coeffs(n_in, n_out)[0]
    return int(bounds[y0, 0]), int(bounds[y1 - 1, 0]) + int(bounds[y1 - 1, 1])


def _resize_rows(img, size, y0, y1):
    """Rows [y0, y1) of ``Image.resize(size)``: img (..., H, W, 3) uint8."""
    H, W = img.shape[-3:-1]
    newW, newH = size
    r0, r1 = _needed_rows(H, newH, y0, y1)
    out = img[..., r0:r1, :, :]
    if newW != W:                                   # a pass that keeps its size is skipped
        out = _pass_torch(out, *device_coeffs(W, newW, img.device), dim=out.dim() - 2)
    if newH != H:
        bounds, kk = device_coeffs(H, newH, img.device)
        out = _pass_torch(out, bounds[y0:y1], kk[y0:y1], dim=out.dim() - 3, first_row=r0)
    return out


def pil_resize_torch(img_u8, size):
    """``Image.resize(size)`` of an RGB image (BICUBIC, the whole image): img (..., H, W, 3)
    uint8 on any device, size = (W', H') -> (..., H', W', 3) uint8, equal to Pillow byte
    for byte.  Horizontal pass first, rounded to a byte, then the vertical pass."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() < 3 or img_u8.shape[-1] != 3:
        raise ValueError('expected a uint8 (..., H, W, 3) image')
    return _resize_rows(img_u8, size, 0, int(size[1]))


def _check_window(resize_dims, crop, rotate=0):
    newW, newH = (int(v) for v in resize_dims)
    x0, y0, x1, y1 = (int(v) for v in crop)
    if rotate != 0:
        raise ValueError('rotate = %s: only rotate = 0 is supported' % (rotate,))
    if newW <= 0 or newH <= 0 or x1 <= x0 or y1 <= y0:
        raise ValueError('empty resize %s or crop %s' % (resize_dims, crop))
    if x0 < 0 or y0 < 0 or x1 > newW or y1 > newH:
        raise ValueError('the crop %s leaves the resized image %dx%d (Pillow would pad with '
                         'zeros; not supported)' % (tuple(crop), newW, newH))
    return newW, newH, x0, y0, x1, y1


def transform_core_torch(img_u8, resize_dims, crop, flip, rotate=0):
    """``img_transform_core`` (:1140-1147): resize, crop, flip -> (..., fH, fW, 3) uint8."""
    newW, newH, x0, y0, x1, y1 = _check_window(resize_dims, crop, rotate)
    out = _resize_rows(img_u8, (newW, newH), y0, y1)[..., x0:x1, :]
    return out.flip(-2) if flip else out


def depthanything_size(h, w, target=252, multiple=14):
    """``Resize.get_size`` of transform_depthanything.py as ``depthanythingNormalize``
    configures it (keep_aspect_ratio, lower_bound, multiples of 14) -> (oh, ow)."""
    scale = max(target / h, target / w)

    def constrain(x):
        y = int(np.round(x / multiple) * multiple)
        return y if y >= target else int(np.ceil(x / multiple) * multiple)
    return constrain(scale * h), constrain(scale * w)


def cubic_weights_torch(n_in, n_out, device=None):
    """The four-tap cubic of the module docstring for one axis -> (taps (out, 4) long,
    clamped to the image; weights (out, 4) fp32, each operation rounded once)."""
    d = torch.arange(n_out, dtype=torch.float64, device=device)
    f = ((d + 0.5) * (n_in / n_out) - 0.5).to(torch.float32)
    s = torch.floor(f)
    t = f - s
    A = -0.75
    w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
    w1 = ((A + 2) * t - (A + 3)) * t * t + 1
    u = 1 - t
    w2 = ((A + 2) * u - (A + 3)) * u * u + 1
    w3 = 1 - w0 - w1 - w2
    taps = (s.long()[:, None] + torch.arange(-1, 3, device=device)).clamp_(0, n_in - 1)
    return taps, torch.stack([w0, w1, w2, w3], 1)


def cubic_norm_torch(img_u8, out_size=None, mean=DEPTHANYTHING_MEAN, std=DEPTHANYTHING_STD,
                     dtype=torch.float32):
    """``depthanythingNormalize`` (:1048-1069): img (..., h, w, 3) uint8 -> (..., 3, oh, ow)
    ``dtype``: swap, / 255, cubic resize to ``out_size`` (``depthanything_size``), then
    (x - mean) / std.  The cubic is OpenCV's INTER_CUBIC as far as it can be stated without
    the package (unpinned): scale = in / out in double, fx = f32((dx + 0.5) scale - 0.5),
    four fp32 weights with A = -0.75, taps sx - 1 .. sx + 2 clamped, rows first (taps summed
    left to right), then columns."""
    h, w = img_u8.shape[-3:-1]
    oh, ow = out_size if out_size is not None else depthanything_size(h, w)
    dev = img_u8.device
    x = img_u8.flip(-1).movedim(-1, -3).to(dtype) / 255
    tx, wx = cubic_weights_torch(w, ow, dev)
    ty, wy = cubic_weights_torch(h, oh, dev)
    wx, wy = wx.to(dtype), wy.to(dtype)
    rows = None
    for k in range(4):
        term = x.index_select(-1, tx[:, k]) * wx[:, k]
        rows = term if rows is None else rows + term
    out = None
    for k in range(4):
        term = rows.index_select(-2, ty[:, k]) * wy[:, k, None]
        out = term if out is None else out + term
    m = torch.tensor(mean, dtype=torch.float32, device=dev).to(dtype)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32, device=dev).to(dtype)[:, None, None]
    return (out - m) / s


def _per_camera(crop, flip, N):
    """-> (crops, flips): lists of one entry, or of N."""
    crops = [tuple(int(v) for v in c) for c in crop] if isinstance(crop[0], (tuple, list)) \
        else [tuple(int(v) for v in crop)]
    flips = [bool(f) for f in flip] if isinstance(flip, (tuple, list)) else [bool(flip)]
    n = max(len(crops), len(flips))
    if n > 1:
        crops = crops * n if len(crops) == 1 else crops
        flips = flips * n if len(flips) == 1 else flips
        if len(crops) != N or len(flips) != N:
            raise ValueError('crop and flip must be one value or one per camera (%d), got %d '
                             'and %d' % (N, len(crops), len(flips)))
        if N > MAX_WINDOWS:
            raise ValueError('at most %d cameras per call with per-camera windows, got %d'
                             % (MAX_WINDOWS, N))
    sizes = set((c[2] - c[0], c[3] - c[1]) for c in crops)
    if len(sizes) != 1:
        raise ValueError('the crop windows must have one size, got %s' % sorted(sizes))
    return crops, flips


def _check_frames(frames, resize_dims, crop, flip, rotate, depth_norm):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or \
            frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError('frames must be a contiguous uint8 (B, N, H, W, 3) tensor')
    if depth_norm not in (None, 'midas', 'depthanythingv2'):
        raise ValueError('unknown depth normalisation %r' % (depth_norm,))
    crops, flips = _per_camera(crop, flip, frames.shape[1])
    for c in crops:
        _check_window(resize_dims, c, rotate)
    return crops, flips


def prepare_images_torch(frames, resize_dims, crop, flip=False, norm='mmlab', depth_size=None,
                         depth_norm=None, return_canvas=False, rotate=0):
    """The mirror of ``prepare_images`` in torch ops on the device of ``frames``."""
    crops, flips = _check_frames(frames, resize_dims, crop, flip, rotate, depth_norm)
    N = frames.shape[1]
    if len(crops) == 1:
        canvas = transform_core_torch(frames, resize_dims, crops[0], flips[0])
    else:
        canvas = torch.stack([transform_core_torch(frames[:, n], resize_dims, crops[n], flips[n])
                              for n in range(N)], 1)
    res = {'imgs': apply_lut_torch(canvas, device_lut(norm, frames.device))}
    if return_canvas:
        res['canvas'] = canvas
    if depth_norm is not None:
        dh, dw = depth_size if depth_size is not None else canvas.shape[-3:-1]
        depth = pil_resize_torch(canvas, (int(dw), int(dh)))
        if depth_norm == 'midas':
            res['depth_img_inputs'] = apply_lut_torch(depth, device_lut('midas', frames.device))
        else:
            res['depth_img_inputs'] = cubic_norm_torch(depth)
        if return_canvas:
            res['depth_canvas'] = depth
    return res


# ------------------------------------------------------------------ native path
def _windows(crops, flips):
    win = _lib.ImageWindows()
    win.n = len(crops)
    for i, (c, f) in enumerate(zip(crops, flips)):
        win.x0[i], win.y0[i], win.flip[i] = c[0], c[1], int(f)
    return win


def _out_tensor(out, key, shape, dtype, dev):
    t = None if out is None else out.get(key)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or \
            t.device != dev:
        raise _lib.VeonHipError('out[%r] must be a contiguous %s tensor of shape %s on %s'
                                % (key, dtype, tuple(shape), dev))
    return t


def _native_resample(src, resize_dims, crops, flips, lut, canvas, planes):
    """src (BN, H, W, 3) uint8 on a ROCm device -> the windows of its resize, into ``canvas``
    (BN, fH, fW, 3) uint8 and / or ``planes`` (BN, 3, fH, fW) fp32 through ``lut``."""
    dev = src.device
    BN, H, W = (int(v) for v in src.shape[:3])
    newW, newH = resize_dims
    fW, fH = crops[0][2] - crops[0][0], crops[0][3] - crops[0][1]
    r0, r1 = H, 0
    for c in crops:
        a, b = _needed_rows(H, newH, c[1], c[3])
        r0, r1 = min(r0, a), max(r1, b)
    Hs, Ws, row0 = H, W, 0
    if newW != W:
        bx, kx = device_coeffs(W, newW, dev)
        tmp = torch.empty((BN, r1 - r0, newW, 3), dtype=torch.uint8, device=dev)
        _lib.launch('veon_image_resample_h', dev, src, BN, H, W, newW, r0, r1 - r0, bx, kx,
                    int(kx.shape[1]), tmp)
        src, Hs, Ws, row0 = tmp, r1 - r0, newW, r0
    by, ky, ksize = None, None, 0
    if newH != H:
        by, ky = device_coeffs(H, newH, dev)
        ksize = int(ky.shape[1])
    _lib.launch('veon_image_resample_v_finish', dev, src, BN, Hs, Ws, row0, newH, by, ky,
                ksize, _windows(crops, flips), fH, fW, lut, 1, canvas, planes)


def prepare_images(frames, resize_dims, crop, flip=False, norm='mmlab', depth_size=None,
                   depth_norm=None, return_canvas=False, out=None, rotate=0):
    """Decoded camera frames -> the network's image inputs.

    frames (B, N, H, W, 3) uint8, contiguous.  resize_dims = (newW, newH), crop = (x0, y0,
    x1, y1) inside the resized image and ``flip``: ``sample_augmentation``'s, one value or
    one per camera (windows of one size).  norm: 'mmlab', 'clipsan' or (mean, std).
    depth_norm 'midas' or 'depthanythingv2' adds the depth branch at depth_size = (dh, dw)
    (``data_config['depth_input_size']``; None: the window's size).

    -> dict: ``imgs`` (B, N, 3, fH, fW) fp32; ``depth_img_inputs`` (B, N, 3, dh, dw) fp32
    (252 x 700 from 256 x 704 for depthanythingv2); with ``return_canvas`` also ``canvas``
    (B, N, fH, fW, 3) uint8, the transformed image, and ``depth_canvas``, its depth resize.
    ``out``: a dict of preallocated results by the same keys.

    ROCm tensors: native, every element written, nothing uploaded in steady state (tables
    cached per sizes and device, windows passed by value), no host synchronisation,
    capturable.  Anything else: ``prepare_images_torch``."""
    crops, flips = _check_frames(frames, resize_dims, crop, flip, rotate, depth_norm)
    resize_dims = (int(resize_dims[0]), int(resize_dims[1]))
    if not frames.is_cuda:
        res = prepare_images_torch(frames, resize_dims, crop, flip, norm, depth_size,
                                   depth_norm, return_canvas)
        for k, v in (out or {}).items():
            if k in res:
                res[k] = v.copy_(res[k])
        return res
    dev = frames.device
    B, N, H, W = (int(v) for v in frames.shape[:4])
    fW, fH = crops[0][2] - crops[0][0], crops[0][3] - crops[0][1]
    need_canvas = return_canvas or depth_norm is not None
    res = {'imgs': _out_tensor(out, 'imgs', (B, N, 3, fH, fW), torch.float32, dev)}
    canvas = _out_tensor(out, 'canvas', (B, N, fH, fW, 3), torch.uint8, dev) \
        if need_canvas else None
    _native_resample(frames.view(B * N, H, W, 3), resize_dims, crops, flips,
                     device_lut(norm, dev), canvas, res['imgs'])
    if return_canvas:
        res['canvas'] = canvas
    if depth_norm is None:
        return res
    dh, dw = (int(v) for v in depth_size) if depth_size is not None else (fH, fW)
    cubic = depth_norm == 'depthanythingv2'
    oh, ow = depthanything_size(dh, dw) if cubic else (dh, dw)
    depth = _out_tensor(out, 'depth_img_inputs', (B, N, 3, oh, ow), torch.float32, dev)
    depth_u8 = canvas
    if (dh, dw) != (fH, fW) or not cubic:
        keep = cubic or return_canvas
        depth_u8 = _out_tensor(out, 'depth_canvas', (B, N, dh, dw, 3), torch.uint8, dev) \
            if keep else None
        _native_resample(canvas.view(B * N, fH, fW, 3), (dw, dh), [(0, 0, dw, dh)], [False],
                         None if cubic else device_lut('midas', dev), depth_u8,
                         None if cubic else depth)
    if cubic:
        _lib.launch('veon_image_cubic_norm', dev, depth_u8, B * N, dh, dw, oh, ow, 1,
                    *DEPTHANYTHING_MEAN, *DEPTHANYTHING_STD, depth)
    if return_canvas:
        res['depth_canvas'] = depth_u8
    res['depth_img_inputs'] = depth
    return res


# ------------------------------------------------------------------ augmentation
def sample_augmentation(data_config, H, W, is_train, flip=None, scale=None, rng=None):
    """``PrepareImageInputs.sample_augmentation`` (:1160-1186) op for op -> (resize,
    resize_dims, crop, flip, rotate).  ``rng``: a ``numpy.random`` generator or the module
    itself (the default); the draws keep the reference's order."""
    rng = np.random if rng is None else rng
    fH, fW = data_config['input_size']
    if is_train:
        resize = float(fW) / float(W)
        resize += rng.uniform(*data_config['resize'])
        resize_dims = (int(W * resize), int(H * resize))
        newW, newH = resize_dims
        crop_h = int((1 - rng.uniform(*data_config['crop_h'])) * newH) - fH
        crop_w = int(rng.uniform(0, max(0, newW - fW)))
        crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
        flip = data_config['flip'] and rng.choice([0, 1])
        rotate = rng.uniform(*data_config['rot'])
    else:
        resize = float(fW) / float(W)
        if scale is not None:
            resize += scale
        else:
            resize += data_config.get('resize_test', 0.0)
        resize_dims = (int(W * resize), int(H * resize))
        newW, newH = resize_dims
        crop_h = int((1 - np.mean(data_config['crop_h'])) * newH) - fH
        crop_w = int(max(0, newW - fW) / 2)
        crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
        flip = False if flip is None else flip
        rotate = 0
    return resize, resize_dims, crop, flip, rotate


def post_homography(post_rot, post_tran, resize, crop, flip, rotate):
    """The post-homography lines of ``img_transform`` (:1124-1136) op for op in fp32 on a
    2 x 2 ``post_rot`` and a 2-vector ``post_tran`` (both are modified, as there)."""
    post_rot *= resize
    post_tran -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        post_rot = A.matmul(post_rot)
        post_tran = A.matmul(post_tran) + b
    h = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    post_rot = A.matmul(post_rot)
    post_tran = A.matmul(post_tran) + b
    return post_rot, post_tran


def post_transform(resize, crop, flip, rotate):
    """``img_transform`` (:1119-1138) without the image, from the identity, widened as
    ``get_inputs`` does (:1249-1253) -> (post_rot (3, 3), post_tran (3,)), fp32."""
    post_rot, post_tran = post_homography(torch.eye(2), torch.zeros(2), resize, crop, flip,
                                          rotate)
    rot3, tran3 = torch.eye(3), torch.zeros(3)
    rot3[:2, :2] = post_rot
    tran3[:2] = post_tran
    return rot3, tran3


def quaternion_rotation_matrix(w, x, y, z):
    """pyquaternion's ``Quaternion(w, x, y, z).rotation_matrix`` restated in float64 (the
    package is absent where this was written: unpinned): normalise unless the quaternion is
    a unit one to 1e-14, then the lower-right 3 x 3 of Q(q) Qbar(q)^T."""
    q = np.array([w, x, y, z], np.float64)
    if abs(1.0 - np.dot(q, q)) >= 1e-14:
        n = math.sqrt(np.dot(q, q))
        if n > 0:
            q = q / n
    w, x, y, z = q
    Q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Qbar = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(Q, Qbar.conj().transpose())[1:, 1:]


# ------------------------------------------------------------------ the pipeline step
class PrepareImageInputs(object):
    """The reference's pipeline step by its constructor and methods, fed decoded frames:
    ``results['curr']['cams'][name]['frame']`` (uint8 (H, W, 3) array or tensor) when
    present, else ``data_path`` decoded with Pillow.  ``device``: where the frames are
    prepared (None: where they are)."""

    def __init__(self, data_config, is_train=False, sequential=False, img_norm_method='mmlab',
                 use_depth_input=False, depth_img_norm_method='midas', use_depth_pred=False,
                 depth_pred_home=None, device=None):
        self.is_train = is_train
        self.data_config = data_config
        if img_norm_method not in NORMS:
            raise ValueError('img_norm_method must be one of %s, got %r'
                             % (sorted(NORMS), img_norm_method))
        self.img_norm_method = img_norm_method
        self.sequential = sequential
        self.use_depth_input = use_depth_input
        self.use_depth_pred = use_depth_pred
        self.depth_img_norm_method = None
        self.depth_pred_home = depth_pred_home
        if not use_depth_pred and use_depth_input:
            if depth_img_norm_method not in ('midas', 'depthanythingv2'):
                raise ValueError('depth_img_norm_method must be midas or depthanythingv2, got '
                                 '%r' % (depth_img_norm_method,))
            self.depth_img_norm_method = depth_img_norm_method
        self.device = None if device is None else torch.device(device)

    def get_rot(self, h):
        return torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])

    def choose_cams(self):
        if self.is_train and self.data_config['Ncams'] < len(self.data_config['cams']):
            return np.random.choice(self.data_config['cams'], self.data_config['Ncams'],
                                    replace=False)
        return self.data_config['cams']

    def sample_augmentation(self, H, W, flip=None, scale=None):
        return sample_augmentation(self.data_config, H, W, self.is_train, flip, scale)

    def img_transform_core(self, img, resize_dims, crop, flip, rotate):
        """img: uint8 (H, W, 3) tensor -> the transformed (fH, fW, 3) tensor."""
        return transform_core_torch(img, resize_dims, crop, flip, rotate)

    def img_transform(self, img, post_rot, post_tran, resize, resize_dims, crop, flip, rotate):
        img = self.img_transform_core(img, resize_dims, crop, flip, rotate)
        post_rot, post_tran = post_homography(post_rot, post_tran, resize, crop, flip, rotate)
        return img, post_rot, post_tran

    def get_sensor_transforms(self, cam_info, cam_name):
        mats = []
        for prefix in ('sensor2ego', 'ego2global'):
            rot = torch.Tensor(quaternion_rotation_matrix(
                *cam_info['cams'][cam_name][prefix + '_rotation']))
            m = rot.new_zeros((4, 4))
            m[3, 3] = 1
            m[:3, :3] = rot
            m[:3, -1] = torch.Tensor(cam_info['cams'][cam_name][prefix + '_translation'])
            mats.append(m)
        return mats[0], mats[1]

    def _frame(self, cam_data):
        frame = cam_data.get('frame')
        if frame is None:
            try:
                from PIL import Image
            except ImportError:
                raise RuntimeError("no decoded 'frame' for %s and Pillow is not installed to "
                                   "decode it" % cam_data.get('data_path'))
            frame = np.array(Image.open(cam_data['data_path']).convert('RGB'))
        frame = torch.as_tensor(frame)
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError('a frame must be uint8 (H, W, 3), got %s %s'
                             % (frame.dtype, tuple(frame.shape)))
        return frame

    def get_inputs(self, results, flip=None, scale=None):
        cam_names = self.choose_cams()
        results['cam_names'] = cam_names
        if self.sequential:
            assert 'adjacent' in results
        infos = [results['curr']] + (list(results['adjacent']) if self.sequential else [])
        frames, augs, unique_tokens = [], [], []          # one entry per image, reference order
        sensor2egos, ego2globals, intrins, post_rots, post_trans = [], [], [], [], []
        for cam_name in cam_names:
            cam_data = results['curr']['cams'][cam_name]
            frame = self._frame(cam_data)
            resize, resize_dims, crop, flip, rotate = self.sample_augmentation(
                H=frame.shape[0], W=frame.shape[1], flip=flip, scale=scale)
            post_rot, post_tran = post_transform(resize, crop, flip, rotate)
            for info in infos:                             # adjacent: the current augmentation
                frames.append(frame if info is results['curr']
                              else self._frame(info['cams'][cam_name]))
                augs.append((tuple(frames[-1].shape[:2]), tuple(resize_dims), tuple(crop),
                             bool(flip), rotate))
                unique_tokens.append(info['token'] + '-' + cam_name)
            sensor2ego, ego2global = self.get_sensor_transforms(results['curr'], cam_name)
            intrins.append(torch.Tensor(cam_data['cam_intrinsic']))
            sensor2egos.append(sensor2ego)
            ego2globals.append(ego2global)
            post_rots.append(post_rot)
            post_trans.append(post_tran)
        for info in infos[1:]:
            post_trans.extend(post_trans[:len(cam_names)])
            post_rots.extend(post_rots[:len(cam_names)])
            intrins.extend(intrins[:len(cam_names)])
            for cam_name in cam_names:
                sensor2ego, ego2global = self.get_sensor_transforms(info, cam_name)
                sensor2egos.append(sensor2ego)
                ego2globals.append(ego2global)

        prepared = self._prepare(frames, augs)
        results['canvas'] = [c.cpu().numpy() for c in prepared['canvas']]
        results['unique_tokens'] = unique_tokens
        if self.use_depth_pred:
            results['depth_preds'] = depth_cache.load(self.depth_pred_home, unique_tokens)
        elif self.use_depth_input:
            results['depth_img_inputs'] = torch.stack(prepared['depth_img_inputs'])
        return (torch.stack(prepared['imgs']), torch.stack(sensor2egos),
                torch.stack(ego2globals), torch.stack(intrins), torch.stack(post_rots),
                torch.stack(post_trans))

    def _prepare(self, frames, augs):
        """One ``prepare_images`` call per group of images that share the frame size and
        ``resize_dims`` (at most 32 images each) -> per-image lists in the given order."""
        depth_size = self.data_config.get('depth_input_size') if self.depth_img_norm_method \
            else None
        groups = {}
        for i, (shape, resize_dims, crop, flip, rotate) in enumerate(augs):
            key = (shape, resize_dims, crop[2] - crop[0], crop[3] - crop[1], rotate)
            chunks = groups.setdefault(key, [[]])
            if len(chunks[-1]) == MAX_WINDOWS:
                chunks.append([])
            chunks[-1].append(i)
        res = {k: [None] * len(frames) for k in ('imgs', 'canvas', 'depth_img_inputs')}
        for (shape, resize_dims, _, _, rotate), chunks in groups.items():
            for idx in chunks:
                batch = torch.stack([frames[i] for i in idx])[None]
                if self.device is not None:
                    batch = batch.to(self.device)
                got = prepare_images(batch.contiguous(), resize_dims, [augs[i][2] for i in idx],
                                     [augs[i][3] for i in idx], norm=self.img_norm_method,
                                     depth_size=depth_size, depth_norm=self.depth_img_norm_method,
                                     return_canvas=True, rotate=rotate)
                for k in res:
                    if k in got:
                        for j, i in enumerate(idx):
                            res[k][i] = got[k][0, j]
        return res

    def __call__(self, results):
        results['img_inputs'] = self.get_inputs(results)
        return results
