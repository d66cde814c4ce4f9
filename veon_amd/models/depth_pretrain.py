"""``VeonDepthPretrain`` -- mirror of mmdet3d/models/detectors/veon_depth_pretrain.py, the
first of the reference's two training stages: DepthAnythingV2 (LoRA on the DINOv2
encoder, DPT head) against LiDAR depth.

    forward_train(img_inputs, depth_img_inputs, gt_depth) -> {'loss_depth_zoe',
                                                              'loss_depth_ce'}
    forward_train(img_inputs, depth_img_inputs, points=...)   the same, the LiDAR depth
                                                              rendered here

``estimate_depth`` (:157-166) runs the estimator and resizes its metric depth to half the
image (bilinear, align_corners=True; torch).  ``forward_train`` (:128-154) downsamples
that by ``pred_depth_scale`` and the LiDAR depth by ``gt_depth_scale``, updates the
running mean absolute error and returns ``get_depth_loss_own(zoe=True, ce=True)``.

Differences from the reference, all on the host side: ``avg_depth_error`` is a device
tensor updated in place (the reference reads the error back with ``.item()`` every step
and prints it now and then); the mmdet3d base class, the unused constructor arguments
and the ``NotImplementedError`` test stubs are not mirrored (call ``forward_train``).

``hip_train`` (default False): opt-in native training path.  It switches on the DINOv2
blocks' ``hip_train`` (depth_anything/dinov2.py) and computes the loss with
csrc/depth_loss.hip (no host synchronisation); off, the loss is the reference's torch
sequence.

``points`` (the reference's signature has the keyword and ignores it): when ``gt_depth``
is None the LiDAR depth is rendered from the sweeps and the eleven-entry ``img_inputs``
(veon_amd/lidar_depth.py, the pipeline step ``PointToMultiViewDepth`` at downsample 1).
With ``hip_train`` on a ROCm device it is rendered natively at the block size
``gt_depth_scale``, the 1/256 of the full maps that the loss reads, and the loss takes it
at scale 1: the same loss bits as the full maps at ``gt_depth_scale``.  Otherwise the full
maps come from the torch mirror.  With ``gt_depth`` given nothing changes."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .builder import build_neck
from .depth_anything.dinov2 import Block
from .. import depth_loss
from ..lidar_depth import PointToMultiViewDepth, pad_points


def _build(cfg):
    return build_neck(cfg) if isinstance(cfg, dict) else cfg


class VeonDepthPretrain(nn.Module):
    r"""Args as the reference (:23-40) where they matter here: ``depth_estimator`` and
    ``img_view_transformer`` (NECKS configs or built modules); the scales the reference
    hard-codes (:66-67) as ``pred_depth_scale`` = 8 and ``gt_depth_scale`` = 16; the
    veon_amd extension ``hip_train``.  Other reference arguments are accepted and
    ignored."""

    def __init__(self, depth_estimator=None, img_view_transformer=None, pred_depth_scale=8,
                 gt_depth_scale=16, hip_train=False, **kwargs):
        super().__init__()
        self.depth_estimator = _build(depth_estimator)
        self.img_view_transformer = _build(img_view_transformer)
        self.pred_depth_scale = pred_depth_scale
        self.gt_depth_scale = gt_depth_scale
        self.nonce = 0
        self.register_buffer('avg_depth_error', torch.zeros(()), persistent=False)
        self.hip_train = hip_train
        self._freeze_stages()

    @property
    def hip_train(self):
        return self._hip_train

    @hip_train.setter
    def hip_train(self, on):
        self._hip_train = bool(on)
        for m in self.depth_estimator.modules():
            if isinstance(m, Block):
                m.hip_train = self._hip_train

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self

    def _freeze_stages(self):
        """The reference's rule (:83-89): frozen iff the name contains 'pretrain' and
        not 'lora' (the DINOv2 encoder lives in ``depth_estimator.pretrained``)."""
        for name, param in self.depth_estimator.named_parameters():
            param.requires_grad = not ('pretrain' in name and 'lora' not in name)

    def estimate_depth(self, depth_input, depth_size):
        B, N, C, H, W = depth_input.shape
        dout = self.depth_estimator(depth_input.view(-1, C, H, W))
        abs_depth = dout['metric_depth']
        if tuple(abs_depth.shape[-2:]) != tuple(depth_size):
            abs_depth = F.interpolate(abs_depth[:, None], tuple(depth_size), mode='bilinear',
                                      align_corners=True)
        else:
            abs_depth = abs_depth[:, None]
        dout['metric_depth'] = abs_depth.view(B, N, *abs_depth.shape[-2:])
        return dout

    def forward_train(self, img_inputs=None, depth_img_inputs=None, gt_depth=None,
                      points=None, **kwargs):
        h, w = img_inputs[0].shape[-2:]
        depth = self.estimate_depth(depth_img_inputs, (h // 2, w // 2))['metric_depth']
        vt = self.img_view_transformer
        native = self.hip_train and depth.is_cuda
        gt_scale = self.gt_depth_scale
        if gt_depth is None:
            if points is None:
                raise ValueError('forward_train needs gt_depth or points')
            to_depth = PointToMultiViewDepth(vt.grid_config, downsample=1)
            points = pad_points(points).to(device=depth.device, dtype=torch.float32)
            if native:
                gt_depth = to_depth.render(points.contiguous(), img_inputs, block=gt_scale)
                gt_scale = 1
            else:
                gt_depth = to_depth.render(points, img_inputs, mirror=True)
        depth, gt_depth = depth.float(), gt_depth.float()          # @force_fp32 (:496)
        if native:
            losses = vt.depth_pretrain_loss(depth.contiguous(), gt_depth.contiguous(),
                                            self.pred_depth_scale, gt_scale)
        else:
            lo, _, step = vt.grid_config['depth']
            losses = depth_loss.depth_pretrain_loss_torch(
                depth, gt_depth, vt.D, lo, step, self.pred_depth_scale, gt_scale)
        depth_error = losses.pop('depth_error')
        # running mean over the steps (:146-147), kept on the device
        self.avg_depth_error.mul_(self.nonce).add_(depth_error.to(self.avg_depth_error.dtype)) \
            .div_(self.nonce + 1)
        self.nonce += 1
        return losses
