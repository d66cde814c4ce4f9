"""VEON's training loss on the occupancy path (``OccLossFB``, models/semantic_net/loss/
occ_loss.py:23-164): a two-class cross entropy on ``bin_occ`` (``BCE_BinOcc_Loss``) and
the 2D->3D feature-alignment loss (``Proj2Dto3DLoss``, loss/occ_loss_utils/
occ3d_nuscenes.py:228-523).

The modules take the LOW-resolution ``feat_occ`` / ``bin_occ`` (B, C, z, y, x) plus
``occ_size``.  The alignment loss is split in two:

* ``Proj2Dto3DLoss.select`` (no grad): everything discrete.  Voxel centres are projected
  into all cameras at once, the 2-D class logits are sampled at the projections, classes
  are arg-maxed (plain, merged by ``class_reflection``, restricted to the labelled
  group), the entries are split into the "det" and the "soft" term, the stage-2 rule
  drops confidently contradicted soft entries, and the class-balanced instance weights
  are folded together with the per-camera and per-sample normalisers into one weight
  per entry.  Result: flat lists ``(voxel, label, weight)`` per sample.
* the loss: ``sum_i w_i (1 - cos_i)`` with ``cos_i`` from ``align_loss.voxel_cosine``,
  the one differentiable primitive, which never forms the upsampled volume on a device.

The stage-2 rule needs, per entry, the class that maximises ``<f_i, table_k>`` over the
K-1 non-free rows and the cosine to it: ``retrieve_points`` with the K-1 rows as prompts
returns ``<f_i, t_k> / (|f_i| |t_k|)``; multiplied by ``|t_k|`` it ranks the classes as
the raw dot product does (the remaining factor is positive and common to the entry), and
the winner's score is the cosine the threshold applies to."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...align_loss import voxel_cosine
from ...align_select import select_entries
from ...occ_bin_loss import bin_occ_loss
from ...retrieval import retrieve_points
from ...vocabulary import group_ids


def _merged_argmax(values, gid, n_groups):
    """arg-max over the merged classes of the per-group maximum of ``values`` (K2, N)."""
    merged = values.new_full((n_groups, values.shape[1]), float('-inf'))
    merged.scatter_reduce_(0, gid[:, None].expand_as(values), values, 'amax')
    return merged.argmax(0)


def _balanced_weights(cam, cls, n_cam, n_cls, priority, scaled):
    """Weight of every entry of one term: 1 / (entries of its class in its camera)
    [times the class priority if ``scaled``], over the sum of the priorities of the
    classes present in the camera, times (entries of the camera) / (entries of all
    cameras) -- the reference's per-camera class-balanced mean and its mix over cameras
    in one factor.  -> (weights (n,), entries per camera (n_cam,))."""
    pair = cam * n_cls + cls
    count = torch.bincount(pair, minlength=n_cam * n_cls).reshape(n_cam, n_cls)
    per_cam = count.sum(1)
    norm = ((count > 0).to(priority.dtype) * priority[None]).sum(1)       # (n_cam,)
    total = per_cam.sum().clamp_min(1).to(priority.dtype)
    w = 1.0 / count.reshape(-1)[pair].to(priority.dtype)
    if scaled:
        w = w * priority[cls]
    w = w / norm[cam] * (per_cam[cam].to(priority.dtype) / total)
    return w, per_cam


class Proj2Dto3DLoss(nn.Module):
    """The 2D->3D feature-alignment loss from the low-resolution feature volume.
    ``epoch`` is set by the training loop; the stage-2 rule applies from
    ``stage2_start`` on.  ``priority``: one value per merged class.

    ``hip_select`` (class attribute, default False): opt-in native selection.  When set,
    ``select`` takes every sample's entries from ``align_select.select_entries``
    (csrc/occ_align_select.hip on a ROCm device with fp32 inputs: two small read-backs per
    sample in place of the torch sequence's 26 synchronising calls; the torch sequence
    below for anything else)."""
    hip_select = False

    def __init__(self, grid_config=None, loss_det_weight=1.0, loss_soft_weight=1.0,
                 ov_class_number=0, high_conf_thr=0.99, stage2_start=2, priority=None):
        super().__init__()
        if priority is None:
            raise ValueError('Proj2Dto3DLoss needs the class priorities')
        self.register_buffer('priority', torch.as_tensor(priority, dtype=torch.float32),
                             persistent=False)
        self.grid_config = grid_config
        self.ov_class_number = int(ov_class_number)
        self.high_conf_thr, self.stage2_start, self.epoch = high_conf_thr, stage2_start, 0
        self.loss_det_weight, self.loss_soft_weight = loss_det_weight, loss_soft_weight
        self.eps = 1e-6          # the clamp of the reference's nn.CosineSimilarity

    def _project(self, img_inputs, occ_size, dtype, device):
        """Voxel centres of the grid in every camera's augmented image:
        (B, n_cam, X*Y*Z, 3) = (u, v, depth), voxels in (x, y, z) row-major order."""
        Zo, Yo, Xo = occ_size
        gc = self.grid_config
        axes = [torch.arange(n, device=device).to(dtype) * gc[k][2] + (gc[k][0] + gc[k][2] / 2)
                for n, k in ((Xo, 'x'), (Yo, 'y'), (Zo, 'z'))]
        centres = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)
        intrins = img_inputs[3].to(dtype)
        post_rots, post_trans = img_inputs[4].to(dtype), img_inputs[5].to(dtype)
        lidarego2global, cam2camego, camego2global = (t.to(dtype) for t in img_inputs[8:11])
        B, n_cam = intrins.shape[:2]
        cam2img = torch.eye(4, dtype=dtype, device=device).repeat(B, n_cam, 1, 1)
        cam2img[..., :3, :3] = intrins
        ego2img = cam2img @ (torch.inverse(camego2global @ cam2camego) @ lidarego2global)
        p = centres @ ego2img[..., :3, :3].transpose(-1, -2) + ego2img[..., None, :3, 3]
        p = torch.cat([p[..., :2] / p[..., 2:3], p[..., 2:3]], -1)
        return p @ post_rots.transpose(-1, -2) + post_trans[..., None, :]

    @torch.no_grad()
    def select(self, feat_low, sem_seg_2d, img_inputs, voxel_semantics, class_reflection,
               ov_classifier_weight, occ_size, class_num=18):
        """The entry lists of ``_select_torch``; with ``hip_select``, sample by sample from
        ``select_entries``."""
        if not self.hip_select:
            return self._select_torch(feat_low, sem_seg_2d, img_inputs, voxel_semantics,
                                      class_reflection, ov_classifier_weight, occ_size,
                                      class_num)
        stage2 = {}
        if self.epoch >= self.stage2_start:
            stage2 = dict(feat_low=feat_low.detach(), table=ov_classifier_weight.detach(),
                          high_conf_thr=self.high_conf_thr)
        B = sem_seg_2d.shape[0]
        return [select_entries(sem_seg_2d[b].to(feat_low.dtype), img_inputs,
                               voxel_semantics[b], class_reflection, self.priority,
                               self.grid_config, occ_size, self.ov_class_number, batch=b,
                               is_last_sample=b == B - 1, class_num=class_num, **stage2)
                for b in range(B)]

    @torch.no_grad()
    def _select_torch(self, feat_low, sem_seg_2d, img_inputs, voxel_semantics,
                      class_reflection, ov_classifier_weight, occ_size, class_num=18,
                      only=None):
        """``only``: evaluate that sample alone (a one-element list).
        -> one dict per sample: ``voxels`` (n, 3) int32 (x, y, z), ``labels`` (n,)
        int32 rows of the table, ``weights`` (n,), ``n_det`` (the first n_det entries
        are the det term, the rest the soft term), and the per-camera counts ``det``,
        ``soft`` and ``ignored`` (soft entries dropped by the stage-2 rule).  The
        stage-2 cosine comes from ``retrieve_points``, whose norm clamp is 1e-8 where the
        reference's is 1e-6: the two differ only for features with |f| < 1e-6."""
        assert class_num == 18
        class_num -= 1                           # without the free class
        device, dtype = feat_low.device, feat_low.dtype
        Zo, Yo, Xo = occ_size
        table = ov_classifier_weight.detach().to(dtype)
        priority = self.priority.to(device=device, dtype=dtype)
        gid, n_groups = group_ids(class_reflection)
        gid = torch.tensor(gid, dtype=torch.long, device=device)
        assert gid.shape[0] == sem_seg_2d.shape[2] and n_groups == class_num
        height, width = img_inputs[0].shape[-2:]
        pts = self._project(img_inputs, occ_size, dtype, device)
        B, n_cam = pts.shape[:2]
        u, v, depth = pts.unbind(-1)
        in_view = (u >= 0) & (u <= width - 1) & (v >= 0) & (v <= height - 1) & \
            (depth < self.grid_config['depth'][1]) & (depth >= self.grid_config['depth'][0])
        det_scale = 0.0 if class_num == self.ov_class_number else 1.0
        out = []
        for b in (range(B) if only is None else [only]):
            gt_all = voxel_semantics[b].reshape(-1).long()
            kept = in_view[b] & ((gt_all < class_num) & (gt_all >= 0))[None]
            cam, vox = kept.nonzero(as_tuple=True)          # camera-major, voxel order
            gt = gt_all[vox]
            xy = torch.stack([u[b][kept] / ((width - 1) / 2) - 1,
                              v[b][kept] / ((height - 1) / 2) - 1], -1)
            bounds = torch.searchsorted(cam, torch.arange(n_cam + 1, device=device)).tolist()
            logits = torch.cat([
                F.grid_sample(sem_seg_2d[b, c][None].detach().to(dtype),
                              xy[None, None, bounds[c]:bounds[c + 1]], mode='bilinear',
                              align_corners=False)[0, :, 0]
                for c in range(n_cam)], 1)                                  # (K2, n)
            plain = logits.argmax(0)
            merged = _merged_argmax(logits, gid, n_groups)
            in_group = gid[:, None] == gt[None]
            restricted = torch.where(in_group, logits,
                                     logits.new_full((), float('-inf'))).argmax(0)

            soft = (merged == gt) | (gt >= class_num - self.ov_class_number)
            # the reference forces entry 0 of the last camera of the last sample into
            # both terms
            forced = bounds[n_cam - 1] if b == B - 1 and bounds[n_cam] > bounds[n_cam - 1] \
                else None
            if forced is not None:
                soft[forced] = True
            det = ~soft
            if forced is not None:
                det[forced] = True

            voxels = torch.stack([vox // (Yo * Zo), (vox // Zo) % Yo, vox % Zo], 1).to(torch.int32)
            ignored = torch.zeros(n_cam, dtype=torch.long, device=device)
            if self.epoch >= self.stage2_start and voxels.shape[0]:
                rows = table[:-1]
                score, _ = retrieve_points(feat_low.detach(), None, voxels, rows, occ_size, b)
                dots = score.to(dtype) * rows.norm(dim=1)[:, None]          # ranks as <f, t_k>
                confident = score.gather(0, dots.argmax(0)[None])[0] >= self.high_conf_thr
                pred_merged = _merged_argmax(dots, gid, n_groups)
                drop = confident & (priority[pred_merged] > priority[merged])
                ignored = torch.bincount(cam[soft & drop], minlength=n_cam)
                soft = soft & ~drop

            w_det, n_det = _balanced_weights(cam[det], gt[det], n_cam, class_num, priority, False)
            w_soft, n_soft = _balanced_weights(cam[soft], merged[soft], n_cam, class_num,
                                               priority, True)
            out.append(dict(
                voxels=torch.cat([voxels[det], voxels[soft]]),
                labels=torch.cat([restricted[det], plain[soft]]).to(torch.int32),
                weights=torch.cat([w_det * det_scale, w_soft]) / B,
                n_det=int(det.sum()), det=n_det, soft=n_soft, ignored=ignored))
        return out

    def forward(self, pred_feat_occ, sem_seg_2d, sem_embed_2d=None, img_inputs=None,
                prev_img_inputs=None, voxel_semantics=None, sem_seg_2d_prev=None,
                sem_embed_2d_prev=None, class_reflection=None, ov_classifier_weight=None,
                class_num=18, occ_size=None):
        """pred_feat_occ: the LOW-resolution (B, C, z, y, x) volume; ``occ_size`` =
        (Z, Y, X) of the labelled grid; voxel_semantics (B, X, Y, Z).  The 2-D
        embeddings and the previous frame's inputs are accepted and unused, as in the
        reference.  -> (loss_det, loss_soft), each already divided by B.  One
        ``voxel_cosine`` call per sample; each call's backward returns a gradient for the
        whole batch (zero outside its sample), so a step writes B^2 sample volumes:
        nothing at B = 1, the reference's training batch per GPU."""
        del sem_embed_2d, prev_img_inputs, sem_seg_2d_prev, sem_embed_2d_prev
        occ_size = tuple(int(v) for v in occ_size)
        table = ov_classifier_weight.detach()
        entries = self.select(pred_feat_occ, sem_seg_2d, img_inputs, voxel_semantics,
                              class_reflection, table, occ_size, class_num)
        loss_det = pred_feat_occ.new_zeros(())
        loss_soft = pred_feat_occ.new_zeros(())
        for b, e in enumerate(entries):
            if not e['voxels'].shape[0]:
                continue
            cos = voxel_cosine(pred_feat_occ, e['voxels'], e['labels'],
                               table.to(pred_feat_occ.dtype), occ_size, self.eps, b)
            term = e['weights'].to(cos.dtype) * (1 - cos)
            loss_det = loss_det + term[:e['n_det']].sum()
            loss_soft = loss_soft + term[e['n_det']:].sum()
        return loss_det, loss_soft


def BCE_BinOcc_Loss(pred, target, class_weights, ignore_index=255, free_index=17):
    """Weighted two-class cross entropy of the occupancy logits ``pred`` (B, 2, X, Y, Z)
    against the semantic labels (B, X, Y, Z): occupied (any class below ``free_index``)
    is class 0, free is class 1, ``ignore_index`` does not count."""
    labels = target.long()
    occupancy = torch.where(labels == ignore_index, labels, (labels >= free_index).long())
    return F.cross_entropy(pred, occupancy, weight=class_weights, ignore_index=ignore_index)


# name of every weight OccLossFB reads from ``loss_weight_cfg`` -> the value its default
# configuration gives it (a configuration that leaves one out gets 1.0)
_DEFAULT_WEIGHTS = {'loss_2d_pixel_align_weight': 1.0, 'loss_voxel_ce_weight': 1.5,
                    'loss_voxel_sem_scal_weight': 0.25, 'loss_voxel_geo_scal_weight': 0.25,
                    'loss_featalign_det_weight': 35.0, 'loss_featalign_soft_weight': 25.0}

# the terms loss_voxel reports: (key stem, its weight, present(open classes, classes))
_TERMS = (('loss_binocc', 'loss_voxel_ce_weight', lambda n_open, n_all: True),
          ('loss_featalign_det', 'loss_featalign_det_weight', lambda n_open, n_all: n_open != n_all),
          ('loss_featalign_soft', 'loss_featalign_soft_weight', lambda n_open, n_all: n_open != 0))


class OccLossFB(nn.Module):
    """``loss_occ=dict(type='OccLossFB', ...)`` of a reference config, on low-resolution
    inputs.  Every ``*_weight`` of ``loss_weight_cfg`` is also an attribute.
    ``class_weights`` (for the semantic CE term, which ``loss_voxel`` never calls) is
    1 / log(frequency + 0.001) when ``class_frequencies`` is given -- the dataset
    statistic is not part of this package -- and uniform otherwise.

    ``hip_train`` (keyword and attribute, default False): opt-in native occupancy term.
    When set and ``bin_occ`` is an fp32 tensor on a ROCm device, ``loss_voxel`` takes it
    from ``occ_bin_loss.bin_occ_loss`` (csrc/occ_bin_loss.hip: upsampling and cross entropy
    fused in both directions, nothing read back); anything else runs the torch sequence.

    ``hip_select`` (keyword and attribute, default False): opt-in native entry selection of
    the alignment loss, passed down to ``Proj2Dto3DLoss.hip_select``."""

    def __init__(self, out_channel=18, loss_weight_cfg=None, empty_idx=17, ignore_idx=255,
                 balance_cls_weight=True, grid_config=None, mode='nuscenes',
                 high_conf_thr=0.985, stage2_start=2, priority=None, ov_class_number=17,
                 class_frequencies=None, hip_train=False, hip_select=False):
        super().__init__()
        self.hip_train = bool(hip_train)
        if mode not in ('semkitti', 'nuscenes'):
            raise ValueError('unknown mode %r' % (mode,))
        self.loss_weight_cfg = dict(_DEFAULT_WEIGHTS) if loss_weight_cfg is None else loss_weight_cfg
        vars(self).update({name: self.loss_weight_cfg.get(name, 1.0) for name in _DEFAULT_WEIGHTS})
        self.out_channel, self.empty_idx, self.ignore_idx = out_channel, empty_idx, ignore_idx
        self.ov_class_number = ov_class_number
        self.high_conf_thr, self.stage2_start, self.priority = high_conf_thr, stage2_start, priority
        self.proj2dto3dloss = Proj2Dto3DLoss(
            grid_config=grid_config, ov_class_number=ov_class_number, priority=priority,
            high_conf_thr=high_conf_thr, stage2_start=stage2_start)
        if hip_select:          # otherwise the class attribute of Proj2Dto3DLoss decides
            self.hip_select = True
        self.bin_occ_loss = BCE_BinOcc_Loss
        self.bin_class_weights = torch.tensor([1.0, 0.5])       # occupied, free
        if balance_cls_weight and class_frequencies is not None:
            freq = torch.as_tensor(class_frequencies, dtype=torch.float64)[:out_channel]
            self.class_weights = 1.0 / torch.log(freq + 0.001)
        else:
            self.class_weights = torch.full((out_channel,), 1.0 / out_channel)

    @property
    def epoch(self):
        return self.proj2dto3dloss.epoch

    @epoch.setter
    def epoch(self, value):
        self.proj2dto3dloss.epoch = value

    @property
    def hip_select(self):
        return self.proj2dto3dloss.hip_select

    @hip_select.setter
    def hip_select(self, value):
        self.proj2dto3dloss.hip_select = bool(value)

    def _bin_weights_on(self, device):
        """``bin_class_weights`` as fp32 on ``device``, copied once per device and per value
        of the attribute (keyed on the tensor's storage and version counter, so no element
        is read: nothing synchronises, and a captured step stays capturable; the torch
        sequence copies the weights every step)."""
        w = self.bin_class_weights
        key = (str(device), w.data_ptr(), w._version, str(w.device))
        cache = self.__dict__.setdefault('_bin_weights_dev', {})
        if key not in cache:
            cache.clear()
            cache[key] = w.detach().to(device=device, dtype=torch.float32).contiguous()
        return cache[key]

    def masked_labels(self, voxel_semantics, mask_camera):
        """The labels with ``ignore_idx`` where no camera sees the voxel, in a copy (the
        reference overwrites the caller's tensor)."""
        return voxel_semantics.masked_fill(mask_camera == 0, self.ignore_idx)

    def loss_voxel(self, semantic_results, target_voxels, meta_info, tag):
        """semantic_results: ``feat_occ`` and ``bin_occ`` at LOW resolution (B, *, z, y, x)
        and ``occ_size``; target_voxels (B, X, Y, Z).  -> the weighted terms of ``_TERMS``
        that the open-vocabulary split leaves in, keyed ``<stem>_<tag>``."""
        occ_size = tuple(int(v) for v in semantic_results['occ_size'])
        value = {}
        value['loss_featalign_det'], value['loss_featalign_soft'] = self.proj2dto3dloss(
            semantic_results['feat_occ'], meta_info['sem_seg_ds'],
            img_inputs=meta_info['img_inputs'], voxel_semantics=target_voxels,
            class_reflection=meta_info['class_reflection'],
            ov_classifier_weight=meta_info['ov_classifier_weight'],
            class_num=self.out_channel, occ_size=occ_size)
        bin_low = semantic_results['bin_occ']
        if self.hip_train and bin_low.is_cuda and bin_low.dtype == torch.float32:
            value['loss_binocc'] = bin_occ_loss(
                bin_low, target_voxels, self._bin_weights_on(bin_low.device), occ_size,
                ignore_index=self.ignore_idx)
        else:
            # 2 channels, 5 MB at the VEON grid: upsampled in torch, (B, 2, X, Y, Z) as the
            # labels
            bin_up = F.interpolate(bin_low.float(), size=occ_size, mode='trilinear',
                                   align_corners=False).permute(0, 1, 4, 3, 2)
            value['loss_binocc'] = self.bin_occ_loss(bin_up, target_voxels,
                                                     self.bin_class_weights.to(bin_up),
                                                     ignore_index=self.ignore_idx)
        n_open, n_all = self.ov_class_number, self.out_channel - 1
        return {'%s_%s' % (stem, tag): getattr(self, weight) * value[stem]
                for stem, weight, present in _TERMS if present(n_open, n_all)}

    def loss(self, voxel_semantics, mask_camera, semantic_results, meta_info, **kwargs):
        """``semantic_results``: a list of result dicts, one per prediction head (tag
        ``c_<index>``)."""
        labels = self.masked_labels(voxel_semantics, mask_camera)
        losses = {}
        for index, result in enumerate(semantic_results):
            losses.update(self.loss_voxel(result, labels, meta_info, 'c_%d' % index))
        return losses

    def forward(self, voxel_semantics, mask_camera, semantic_results, img_inputs,
                prev_img_inputs=None, **kwargs):
        """semantic_results: dict with ``feat_occ``, ``bin_occ`` (low resolution),
        ``occ_size``, and the 2-D branch's ``sem_seg_ds``, ``class_reflection``,
        ``ov_classifier_weight``.  ``prev_img_inputs`` is accepted and unused."""
        side = ('sem_seg_ds', 'class_reflection', 'ov_classifier_weight')
        meta_info = {k: semantic_results[k] for k in side}
        meta_info['img_inputs'] = img_inputs
        heads = {k: v for k, v in semantic_results.items() if k not in side}
        return self.loss(voxel_semantics, mask_camera, [heads], meta_info, **kwargs)
