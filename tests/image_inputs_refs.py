"""Shared inputs and independent restatements for the camera-input tests
(tests/test_image_inputs.py, tests/test_image_inputs_gpu.py) and the fixture's generator
(tools/gen_golden_image_inputs.py).

The uint8 images of tests/golden/image_inputs_tiny.npz are recordings of the reference's own
``PrepareImageInputs.img_transform_core`` on Pillow.  The normalised outputs are NOT
recorded, because mmcv and cv2 are absent where the fixture is made: ``normalize_ref``,
``midas_ref`` and ``cubic_norm_ref`` below restate them in numpy from the sources
(mmcv's ``imnormalize``; OpenCV's INTER_CUBIC as far as it can be stated without the
package).  They are restatements, not recordings: unpinned against mmcv / cv2."""
import math

import numpy as np

# (H, W), resize_dims (W', H'), two cameras of (crop, flip): the issue's table; the second
# camera has the opposite flip and, where the window is smaller than the resized image,
# another origin (a window that fills the resized image has only one origin)
TABLE = {
    1: dict(size=(45, 80), resize_dims=(70, 39),
            cams=[((3, 7, 67, 39), True), ((6, 0, 70, 32), False)]),
    2: dict(size=(30, 40), resize_dims=(53, 41),
            cams=[((0, 0, 53, 41), False), ((0, 0, 53, 41), True)]),
    3: dict(size=(45, 80), resize_dims=(31, 45),
            cams=[((0, 0, 31, 45), False), ((0, 0, 31, 45), True)]),
    4: dict(size=(30, 40), resize_dims=(40, 17),
            cams=[((2, 1, 34, 17), True), ((8, 0, 40, 16), False)]),
    5: dict(size=(24, 32), resize_dims=(32, 24),
            cams=[((5, 3, 29, 19), False), ((0, 8, 24, 24), True)]),
    6: dict(size=(64, 128), resize_dims=(16, 8),
            cams=[((0, 0, 16, 8), False), ((0, 0, 16, 8), True)]),
    7: dict(size=(37, 53), resize_dims=(80, 61),
            cams=[((9, 20, 73, 52), True), ((16, 29, 80, 61), False)]),
}
BATCH2_ROW = 1                      # the row that also runs as B = 2
RATIOS = [(1600, 1408), (900, 792), (1408, 704), (512, 256)]   # production, image and depth

# the 900 x 1600 -> 512 x 1408 window, recorded as a strip only
STRIP = dict(size=(900, 1600), resize_dims=(1408, 792), crop=(0, 280, 1408, 792), flip=False,
             rows=list(range(0, 8)) + list(range(504, 512)),
             cols=list(range(0, 16)) + list(range(1392, 1408)), seed=900)

VEON_DATA_CONFIG = {
    'cams': ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_LEFT', 'CAM_BACK',
             'CAM_BACK_RIGHT'],
    'Ncams': 6, 'input_size': (512, 1408), 'depth_input_size': (256, 704),
    'src_size': (900, 1600), 'resize': (-0.00, 0.00), 'rot': (-0.0, 0.0), 'flip': False,
    'crop_h': (0.0, 0.0), 'resize_test': 0.00,
}
# the augmentation ranges the VEON configs carry as comments: every draw is live
AUG_DATA_CONFIG = dict(VEON_DATA_CONFIG, resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                       crop_h=(0.0, 0.1))
AUG_SEED, AUG_DRAWS = 22, 4

NORMS = {'mmlab': ([123.675, 116.28, 103.53], [58.395, 57.12, 57.375]),
         'clipsan': ([122.7709, 116.7460, 104.0937], [68.5005, 66.6322, 70.3232])}
DA_MEAN, DA_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def depth_dims(crop):
    """The 2:1 depth size (w, h) of a window."""
    return (crop[2] - crop[0]) // 2, (crop[3] - crop[1]) // 2


def make_frame(seed, h, w):
    """Seeded random bytes with hard 0 / 255 stripes, so that both clamps of the resampling
    occur -> (h, w, 3) uint8."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    a[:, 0::7] = 0
    a[:, 3::11] = 255
    a[2::9] = 255
    a[5::13, :, 1] = 0
    return a


def make_bright_frame(seed, h, w):
    """Seeded random bytes in [128, 255] with 255 stripes: the input of the cubic tail's
    tests.  With every pixel p >= 128 / 255 > 0.5 > max(mean), the magnitude sum
    S = sum |w_y| |w_x| |p| of an output is at least 0.5 (the weights sum to 1), it bounds
    |x| and |x - mean|, and the four roundings after the sums (mean and std to fp32, the
    subtraction, the division) err by at most u (mean + 3 |x - mean|) <= 4 u S: the bound of
    ``cubic_norm_ref`` holds to first order.  On a black image S = 0 and the bound could not
    hold for a kernel that takes mean and std in fp32."""
    rng = np.random.RandomState(seed)
    a = rng.randint(128, 256, (h, w, 3)).astype(np.uint8)
    a[:, 3::11] = 255
    a[2::9] = 255
    return a


def table_frames(row, batch=1):
    """-> (batch, 2, H, W, 3) uint8: the two cameras of a table row."""
    h, w = TABLE[row]['size']
    return np.stack([np.stack([make_frame(1000 * row + 10 * b + n, h, w) for n in range(2)])
                     for b in range(batch)])


# ------------------------------------------------------------------ Pillow's tables, scalar
def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs_ref(n_in, n_out):
    """The issue's per-axis setup in scalar Python floats, one output index at a time ->
    (bounds (out, 2), kk (out, ksize)) int32 arrays."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass_ref(img, bounds, kk, axis):
    img = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.int64)
    for i, (first, n) in enumerate(bounds):
        k = kk[i, :n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        out[i] = (1 << 21) + (img[first:first + n] * k).sum(0)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), 0, axis)


def pil_resize_ref(img, size):
    """``Image.resize(size)`` on an (H, W, 3) uint8 array, from ``coeffs_ref``."""
    h, w = img.shape[:2]
    if size[0] != w:
        img = _pass_ref(img, *coeffs_ref(w, size[0]), axis=1)
    if size[1] != h:
        img = _pass_ref(img, *coeffs_ref(h, size[1]), axis=0)
    return img


def transform_ref(img, resize_dims, crop, flip):
    out = pil_resize_ref(img, resize_dims)[crop[1]:crop[3], crop[0]:crop[2]]
    return out[:, ::-1] if flip else out


# ------------------------------------------------------------------ normalisations
def normalize_ref(img, norm):
    """mmcv's ``imnormalize(np.array(img), mean, std, to_rgb=True)`` then the reference's
    permute: (h, w, 3) uint8 -> (3, h, w) fp32.  The image is RGB already, so the swap makes
    output channel c the input channel 2 - c; then one fp32 subtraction by f32(mean) and
    one fp32 multiplication by f32(1 / f64(std)).  A restatement (mmcv is absent)."""
    mean, std = (np.array(v, np.float32) for v in (NORMS[norm] if isinstance(norm, str)
                                                   else norm))
    x = img.astype(np.float32)[..., ::-1]
    stdinv = (1 / np.float64(std.reshape(1, -1))).astype(np.float32)
    x = (x - mean.reshape(1, -1)) * stdinv
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def midas_ref(img):
    """``midasNormalize`` (loading.py:1037-1045): / 255. in double, fp32, swap, (x - 0.5f) *
    f32(1 / 0.5).  A restatement."""
    x = (img / 255.).astype(np.float32)[..., ::-1]
    x = (x - np.float32(0.5)) * np.float32(1 / np.float64(np.float32(0.5)))
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def cubic_axis_ref(n_in, n_out):
    """Taps (out, 4) clamped and the four fp32 weights (out, 4) of the cubic definition."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    s = np.floor(f)
    t = (f - s).astype(np.float32)
    A, one = np.float32(-0.75), np.float32(1)
    t1 = t + one
    w0 = ((A * t1 - np.float32(5) * A) * t1 + np.float32(8) * A) * t1 - np.float32(4) * A
    w1 = ((A + np.float32(2)) * t - (A + np.float32(3))) * t * t + one
    u = one - t
    w2 = ((A + np.float32(2)) * u - (A + np.float32(3))) * u * u + one
    w3 = one - w0 - w1 - w2
    w = np.stack([w0, w1, w2, w3], 1)
    assert w.dtype == np.float32
    taps = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3), 0, n_in - 1)
    return taps, w


# roundings between a byte and an output of the fp32 chain: / 255, product and three sums
# along the row, product and three sums down the column, the subtraction, the division, and
# the fp32 roundings of mean and std themselves
CUBIC_CHAIN = 1 + 4 + 4 + 2 + 2


def cubic_norm_ref(img, oh, ow):
    """``depthanythingNormalize`` (:1048-1069) in float64 on an (h, w, 3) uint8 array, with
    the fp32 weights of the definition -> (out (3, oh, ow) float64, bound (3, oh, ow)): the
    bound is sum |w_y| |w_x| |p| of each output times the fp32 unit roundoff 2^-24 times
    ``CUBIC_CHAIN``, divided by the channel's std.  A restatement of OpenCV's INTER_CUBIC,
    unpinned against cv2 (absent)."""
    h, w = img.shape[:2]
    x = img[..., ::-1].astype(np.float64).transpose(2, 0, 1) / 255.0
    tx, wx = cubic_axis_ref(w, ow)
    ty, wy = cubic_axis_ref(h, oh)
    wx, wy = wx.astype(np.float64), wy.astype(np.float64)
    rows = sum(x[:, :, tx[:, k]] * wx[:, k] for k in range(4))
    rows_abs = sum(np.abs(x[:, :, tx[:, k]]) * np.abs(wx[:, k]) for k in range(4))
    val = sum(rows[:, ty[:, k], :] * wy[:, k, None] for k in range(4))
    mag = sum(rows_abs[:, ty[:, k], :] * np.abs(wy[:, k, None]) for k in range(4))
    mean = np.array(DA_MEAN, np.float64)[:, None, None]
    std = np.array(DA_STD, np.float64)[:, None, None]
    return (val - mean) / std, mag * 2.0 ** -24 * CUBIC_CHAIN / std
