"""The LiDAR depth labels of VEON's depth pre-training stage: the pipeline step
``PointToMultiViewDepth`` (mmdet3d/datasets/pipelines/loading.py:729-833), which every VEON
config runs with ``downsample=1``: project the sweep into every camera (:807-820), round to
a pixel, filter by image bounds and depth range, keep the nearest point of each pixel
(``points2depthmap``, :735-759).

On a ROCm device ``multiview_depth`` is native (csrc/lidar_depth.hip: fill, one scatter
with an integer atomic minimum on the output's own storage, sentinel to zero; nothing read
back) and can render the block-minimum by ``block`` directly: ``block = 16`` is what
``depth_pretrain_loss`` reads, 1/256 of the full maps.  ``multiview_depth_torch`` is the
same computation in torch at any dtype and device: the CPU path and the tests' yardstick.

The one departure from the reference, in both forms: the value of a pixel several kept
points share is their exact minimum.  The reference sorts by the fp32 key
``rank + depth / 100`` and keeps the first point of each rank; at ranks of 2^19 and above
(row 372 of a 1408-wide map and below) that key's unit in the last place is 0.0625, so
depths within 6.25 m of each other can round to one key and the unstable ``argsort`` picks
among them.  The intended result, the nearest return, is well defined and what is computed
here; away from such ties the two agree bit for bit (tests/test_lidar_depth.py)."""
import math

import torch

from . import _lib

BLOCKS = (1, 2, 4, 8, 16)


# ------------------------------------------------------------------ matrices
def compose_lidar2img(lidar2lidarego, lidarego2global, cam2camego, camego2global, intrins,
                      dtype=torch.float32):
    """loading.py:807-813 op for op, batched over any leading dimensions:
    ``cam2img @ (inverse(camego2global @ cam2camego) @ (lidarego2global @ lidar2lidarego))``
    with ``cam2img`` = identity(4) holding ``intrins`` -> (..., 3, 4) fp32, the rows the
    projection reads.  ``dtype=torch.float64`` composes in double and rounds once.  4x4
    algebra on whatever device the matrices are on (the loader's are on the CPU); it
    belongs outside a captured region."""
    l2le, le2g, c2ce, ce2g = (t.to(dtype) for t in (lidar2lidarego, lidarego2global,
                                                    cam2camego, camego2global))
    cam2img = torch.eye(4, dtype=dtype, device=intrins.device).expand(
        *intrins.shape[:-2], 4, 4).clone()
    cam2img[..., :3, :3] = intrins.to(dtype)
    lidar2cam = torch.inverse(ce2g.matmul(c2ce)).matmul(le2g.matmul(l2le))
    return cam2img.matmul(lidar2cam)[..., :3, :].to(torch.float32).contiguous()


# ------------------------------------------------------------------ torch mirror
def project_points_torch(points, lidar2img, post_rots, post_trans):
    """loading.py:814-820 for every camera: points (B, P, >=3), lidar2img (B, N, 3, 4),
    post_rots (B, N, 3, 3), post_trans (B, N, 3) -> image points (B, N, P, 3) = (u, v, d),
    in the dtype of ``points``."""
    dt = points.dtype
    p = points[:, None, :, :3]
    m = lidar2img.to(dt)
    q = p.matmul(m[..., :3, :3].transpose(-1, -2)) + m[..., None, :3, 3]
    q = torch.cat([q[..., :2] / q[..., 2:3], q[..., 2:3]], -1)
    return q.matmul(post_rots.to(dt).transpose(-1, -2)) + post_trans.to(dt)[..., None, :]


def points2depthmap_torch(points_img, height, width, depth_range, downsample=1, block=1):
    """``points2depthmap`` (:735-759) with the exact minimum: points_img (..., P, 3) image
    points (u, v, d); ``height``, ``width``: the image, as the reference's arguments ->
    (..., height // downsample // block, width // downsample // block), the smallest kept
    depth of each block x block pixels, 0 where nothing landed.

    Departs from the reference in one place: among the kept points of a pixel it takes the
    minimum depth (``scatter_reduce_ amin``) where the reference takes the first of an
    unstable argsort by the fp32 key ``rank + depth / 100``.  The two differ only where
    that key ties between different depths (the module docstring), and there the
    reference's choice has no definition to mirror."""
    lo, hi = depth_range
    height, width = height // downsample, width // downsample
    hb, wb = height // block, width // block
    lead = points_img.shape[:-2]
    pts = points_img.reshape(math.prod(lead), points_img.shape[-2], 3)
    coor = torch.round(pts[..., :2] / downsample)
    depth = pts[..., 2]
    kept = (coor[..., 0] >= 0) & (coor[..., 0] < width) & (coor[..., 1] >= 0) & \
        (coor[..., 1] < height) & (depth < hi) & (depth >= lo)
    coor = torch.where(kept[..., None], coor, torch.zeros_like(coor)).to(torch.long)
    cell = torch.div(coor[..., 1], block, rounding_mode='floor') * wb + \
        torch.div(coor[..., 0], block, rounding_mode='floor')
    inf = torch.full_like(depth, float('inf'))
    out = inf.new_full((pts.shape[0], hb * wb), float('inf'))
    out.scatter_reduce_(1, cell, torch.where(kept, depth, inf), 'amin', include_self=True)
    out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    return out.reshape(*lead, hb, wb)


def multiview_depth_torch(points, lidar2img, post_rots, post_trans, height, width,
                          depth_range, downsample=1, block=1):
    """The mirror of ``multiview_depth`` on a (B, P, S) tensor -> (B, N, H, W) maps in the
    dtype of ``points``.  ``lidar2img`` None: the rows are image points, N = 1."""
    if lidar2img is None:
        img = points[:, None, :, :3]
    else:
        img = project_points_torch(points, lidar2img, post_rots, post_trans)
    return points2depthmap_torch(img, height, width, depth_range, downsample, block)


# ------------------------------------------------------------------ public call
def pad_points(points):
    """A list of (P_b, S) tensors -> (B, max P_b, S), short samples filled with NaN rows:
    a NaN fails every comparison of the filter, so a padded row is no point."""
    if isinstance(points, torch.Tensor):
        return points
    P = max([int(p.shape[0]) for p in points] + [0])
    out = points[0].new_full((len(points), P, points[0].shape[1]), float('nan'))
    for b, p in enumerate(points):
        out[b, :p.shape[0]] = p
    return out


def _check_args(height, width, depth_range, downsample, block):
    lo, hi = (float(v) for v in depth_range[:2])
    if not lo > 0 or not hi > lo:
        raise ValueError('the depth range must satisfy 0 < lo < hi, got [%s, %s)' % (lo, hi))
    if block not in BLOCKS:
        raise ValueError('block must be in %s, got %s' % (BLOCKS, block))
    if downsample < 1 or height <= 0 or width <= 0 or height % (downsample * block) or \
            width % (downsample * block):
        raise ValueError('the image %dx%d is not a multiple of downsample * block = %d * %d'
                         % (height, width, downsample, block))
    return lo, hi


def _check_native(*tensors):
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.VeonHipError('the native depth render takes contiguous fp32 tensors, '
                                    'got %s with strides %s' % (t.dtype, t.stride()))


def multiview_depth(points, lidar2img, post_rots, post_trans, height, width, depth_range,
                    downsample=1, block=1, out=None):
    """The LiDAR depth maps of every camera.

    points (B, P, S >= 3): the sweeps, xyz first (nuScenes' 5-float rows are read in
    place), or a list of (P_b, S) tensors (padded with NaN rows; a NaN row is no point).
    lidar2img (B, N, 3, 4) (``compose_lidar2img``), post_rots (B, N, 3, 3), post_trans
    (B, N, 3); ``lidar2img`` None: the rows are image points (u, v, d), N = 1 and the post
    transform is not applied (``points2depthmap`` alone).  height, width: the image;
    depth_range: (lo, hi, ...) with 0 < lo < hi.  -> (B, N, height // downsample // block,
    width // downsample // block): the smallest depth in [lo, hi) among the points that
    round into each block x block pixels, 0 where there is none.  For hi <= 1e5 the result
    equals ``downsample_depth(block=1 result, block)`` with its 1e5 for an empty block read
    as 0, to the bit.

    ROCm tensors: native (contiguous fp32 only, anything else raises VeonHipError), every
    element of ``out`` written, no host synchronisation, graph-capturable, bit-reproducible
    in any point order.  CPU tensors: ``multiview_depth_torch``."""
    height, width, downsample, block = int(height), int(width), int(downsample), int(block)
    lo, hi = _check_args(height, width, depth_range, downsample, block)
    points = pad_points(points)
    if points.dim() != 3 or points.shape[2] < 3:
        raise ValueError('points must be (B, P, S >= 3), got %s' % (tuple(points.shape),))
    B, P, S = points.shape
    if lidar2img is None:
        N = 1
    else:
        N = lidar2img.shape[1]
        if tuple(lidar2img.shape) != (B, N, 3, 4) or tuple(post_rots.shape) != (B, N, 3, 3) \
                or tuple(post_trans.shape) != (B, N, 3):
            raise ValueError('lidar2img, post_rots, post_trans must be (B, N, 3, 4), (B, N, 3, '
                             '3), (B, N, 3) with B = %d; got %s, %s, %s'
                             % (B, tuple(lidar2img.shape), tuple(post_rots.shape),
                                tuple(post_trans.shape)))
    H, W = height // downsample, width // downsample
    shape = (B, N, H // block, W // block)
    if not points.is_cuda:
        res = multiview_depth_torch(points, lidar2img, post_rots, post_trans, height, width,
                                    (lo, hi), downsample, block)
        if out is None:
            return res
        out.copy_(res)
        return out
    mats = (None, None, None) if lidar2img is None else (lidar2img, post_rots, post_trans)
    dev = _lib.require_device(points, out, *mats)
    _check_native(points, out, *mats)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape:
        raise _lib.VeonHipError('out is %s, not %s' % (tuple(out.shape), shape))
    _lib.launch('veon_lidar_depth_render', dev, points, B, P, S, mats[0], mats[1], mats[2], N,
                H, W, downsample, block, lo, hi, out)
    return out


class PointToMultiViewDepth(object):
    """The reference's pipeline step (:729-833) by its constructor, attributes and
    ``points2depthmap`` signature; ``render`` is its ``__call__`` on the training step's
    tensors instead of the loader's ``results`` dict (no quaternions, no point class)."""

    def __init__(self, grid_config, downsample=1):
        self.downsample = downsample
        self.grid_config = grid_config

    def points2depthmap(self, points, height, width):
        """points (P, 3) image points (u, v, d) -> (height // downsample,
        width // downsample), on the device of ``points``."""
        return multiview_depth(points[None, :, :3].contiguous(), None, None, None, height,
                               width, self.grid_config['depth'], self.downsample)[0, 0]

    def render(self, points, img_inputs, block=1, mirror=False):
        """points: (B, P, S) lidar-frame sweeps or a list of (P_b, S); img_inputs: the
        eleven entries of a training step (images, rots, trans, intrins, post_rots,
        post_trans, bda, lidar2lidarego, lidarego2global, cam2camego, camego2global).
        -> gt_depth (B, N, H // block, W // block) on the device of ``points``, H x W the
        image (``img_inputs[0].shape[-2:]``) over ``downsample``.  ``mirror``: the torch
        sequence on whatever device the points are on."""
        points = pad_points(points)
        height, width = (int(v) for v in img_inputs[0].shape[-2:])
        lidar2img = compose_lidar2img(*img_inputs[7:11], img_inputs[3])
        mats = [t.to(device=points.device, dtype=points.dtype).contiguous()
                for t in (lidar2img, img_inputs[4], img_inputs[5])]
        fn = multiview_depth_torch if mirror else multiview_depth
        if mirror:
            _check_args(height, width, self.grid_config['depth'], self.downsample, block)
        return fn(points, mats[0], mats[1], mats[2], height, width,
                  self.grid_config['depth'][:2], self.downsample, block)
