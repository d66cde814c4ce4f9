"""Open-vocabulary point retrieval on the occupancy path (POP-3D, the
``retrieval=True`` branch of ``VEONTemporal.simple_test``,
detectors/veon_temporal.py:232-241, 331-356).

The reference upsamples the head's feature volume ``feat_occ`` (B, C, z, y, x) to
the evaluation grid in fp32 (san_in_veon_temporal.py:195-200, 212), gathers it at the
voxel of every LiDAR point (``points_indices``, datasets/pipelines/loading.py:
990-1012), scores each point by ``F.cosine_similarity`` against a prompt embedding
(san_in_veon_temporal.py:268-273) and reports sklearn's ``average_precision_score``
over all points and over the visible ones (``compute_single_retrieval``).

On a ROCm device ``retrieve_points`` is one native call (csrc/occ_retrieval.hip):
every point interpolates from the 8 low-resolution rows it needs, so the upsampled
volume (1.31 GB at C = 512) is never formed.  On CPU it runs the reference sequence
in torch (the fallback, and the CPU tests' oracle).  Prompt embeddings are inputs; the
text side (``models/semantic_net/clip_text.py``: ``OvClassifier.retrieval_embedding``)
makes them from prompts, and ``VeonOccupancyPath.retrieve(..., prompts=[...])`` does both."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import half as _half


def _feat_view(feat):
    """(B, C, z, y, x) view of a PaddedVolume's interior (strided, no copy) or the
    tensor itself."""
    from .conv3d_ops import PaddedVolume
    if isinstance(feat, PaddedVolume):
        return feat.interior().permute(0, 4, 1, 2, 3)
    if not isinstance(feat, torch.Tensor) or feat.dim() != 5:
        raise ValueError('feat must be a PaddedVolume or a (B, C, z, y, x) tensor')
    return feat


def _reference(feat, bin_low, points, embeddings, occ_size, batch):
    """The reference sequence in torch: upsample, gather, cosine (and the occupancy
    softmax).  Points outside the grid give NaN."""
    dt = torch.float64 if feat.dtype == torch.float64 else torch.float32
    C = embeddings.shape[1]
    size = tuple(int(v) for v in occ_size)
    Zo, Yo, Xo = size
    pts = points.long()
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    inside = (x >= 0) & (x < Xo) & (y >= 0) & (y < Yo) & (z >= 0) & (z < Zo)
    xs, ys, zs = x.clamp(0, Xo - 1), y.clamp(0, Yo - 1), z.clamp(0, Zo - 1)
    f_up = F.interpolate(feat[batch:batch + 1, :C].to(dt), size, mode='trilinear',
                         align_corners=False)[0]
    f = f_up[:, zs, ys, xs]                                        # (C, P)
    e = embeddings.to(dt)
    score = F.cosine_similarity(f[None], e[:, :, None], dim=1)     # (Q, P)
    score = torch.where(inside[None], score, torch.full_like(score, float('nan')))
    prob = None
    if bin_low is not None:
        b_up = F.interpolate(bin_low[batch:batch + 1].to(dt), size, mode='trilinear',
                             align_corners=False)[0]
        prob = torch.softmax(b_up[:, zs, ys, xs], dim=0)[0]
        prob = torch.where(inside, prob, torch.full_like(prob, float('nan')))
    return score, prob


def retrieve_points(feat, bin_low, points, embeddings, occ_size, batch=0):
    """Cosine score of every point against every prompt, read from the
    LOW-resolution feature volume.

    feat: PaddedVolume (the sem head's rows, the build's half type; channels beyond
    C are ignored) or a (B, C, z, y, x) tensor (fp32, any strides, on the device).
    bin_low: (B, 2, z, y, x) occupancy logits or None.  points: (P, 3) int32 voxel
    indices (x, y, z) in ``occ_size`` = (Z, Y, X), all of sample ``batch``.
    embeddings: (Q, C) prompt embeddings of any scale.
    -> (score (Q, P) fp32, bin_prob (P,) fp32 or None); NaN for points outside the
    grid.  Device calls launch on the current stream and never synchronise
    (hipGraph-capturable)."""
    from .conv3d_ops import PaddedVolume
    view = _feat_view(feat)
    B, Cv, zi, yi, xi = view.shape
    if embeddings.dim() != 2:
        raise ValueError('embeddings must be (Q, C)')
    Q, C = embeddings.shape
    if C > Cv or (not isinstance(feat, PaddedVolume) and C != Cv):
        raise ValueError('embeddings have %d channels, the feature volume %d' % (C, Cv))
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError('points must be (P, 3) (x, y, z)')
    if not 0 <= batch < B:
        raise ValueError('batch %d outside [0, %d)' % (batch, B))
    if bin_low is not None and tuple(bin_low.shape) != (B, 2, zi, yi, xi):
        raise ValueError('bin_low must be (B, 2, z, y, x) = %s' % ((B, 2, zi, yi, xi),))
    if not view.is_cuda:
        return _reference(view, bin_low, points, embeddings, occ_size, batch)

    dev = _lib.require_device(view, bin_low, points, embeddings)
    if view.dtype == torch.float32:
        is_half = 0
    else:
        _lib.require_half(view)
        is_half = 1
    if bin_low is not None and bin_low.dtype != torch.float32:
        bin_low = bin_low.float()
    pts = points.to(torch.int32).contiguous()
    emb = embeddings.to(torch.float32).contiguous()
    P = pts.shape[0]
    Zo, Yo, Xo = (int(v) for v in occ_size)
    score = torch.empty((Q, P), dtype=torch.float32, device=dev)
    prob = (torch.empty((P,), dtype=torch.float32, device=dev)
            if bin_low is not None else None)
    norms = torch.empty((Q,), dtype=torch.float32, device=dev)
    bs = _lib.strides(bin_low) if bin_low is not None else _lib.host_array((0,) * 5)
    _lib.launch('veon_occ_retrieve', dev, view, is_half, _lib.strides(view), C, bin_low, bs,
                B, zi, yi, xi, Zo, Yo, Xo, pts, P, batch, emb, Q, norms, score, prob)
    return score, prob


def points_to_voxel_indices(points_lidar, lidar2lidarego, grid_config, occ_size):
    """``RetrievalForPointsIndices`` (datasets/pipelines/loading.py:990-1012): LiDAR
    points (P, >=3) into the ego frame (4x4 ``lidar2lidarego``), then the voxel index
    floor((p - lower) / interval) of the grid, clamped to [0, size - 1], in (x, y, z)
    order, int32.  ``grid_config``: dict with 'x', 'y', 'z' = [lower, upper, interval]
    of the evaluation grid; ``occ_size`` = (Z, Y, X)."""
    pts = torch.as_tensor(points_lidar)[:, :3].float()
    m = torch.as_tensor(lidar2lidarego, dtype=torch.float32, device=pts.device)
    pts = pts @ m[:3, :3].T + m[:3, 3]
    lower = torch.tensor([grid_config[k][0] for k in 'xyz'], device=pts.device)
    step = torch.tensor([grid_config[k][2] for k in 'xyz'], device=pts.device)
    Zo, Yo, Xo = (int(v) for v in occ_size)
    idx = torch.floor((pts - lower) / step).long()
    hi = torch.tensor([Xo - 1, Yo - 1, Zo - 1], device=pts.device)
    idx = torch.minimum(idx.clamp_min(0), hi)
    return idx.to(torch.int32)


def average_precision(labels, scores):
    """``sklearn.metrics.average_precision_score(labels, scores)`` in torch:
    sum over the distinct score thresholds (descending; tied scores form one step)
    of (R_n - R_{n-1}) * P_n.  0.0 when there is no positive (sklearn >= 1.7).
    Returns a Python float."""
    y = torch.as_tensor(labels).reshape(-1).to(torch.float64)
    s = torch.as_tensor(scores).reshape(-1).to(torch.float64)
    if y.numel() != s.numel():
        raise ValueError('labels and scores differ in length')
    y = (y > 0).to(torch.float64)
    npos = y.sum()
    if y.numel() == 0 or npos.item() == 0:
        return 0.0
    order = torch.argsort(s, descending=True, stable=True)
    s, y = s[order], y[order]
    tps = torch.cumsum(y, 0)
    # last index of every run of equal scores: one threshold each
    last = torch.ones_like(s, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]
    tp = tps[last]
    n = torch.nonzero(last).reshape(-1).to(torch.float64) + 1.0
    precision = tp / n
    recall = tp / npos
    prev = torch.cat([recall.new_zeros(1), recall[:-1]])
    return float(((recall - prev) * precision).sum().item())


def pop3d_retrieval(score_row, bin_prob, labels, visible_idx):
    """``compute_single_retrieval``: AP of one prompt's point scores over all points
    and over the visible subset -> {'map', 'map_visible'}.  ``bin_prob`` is accepted
    for the reference's signature (its occupancy probabilities travel with the
    scores) and does not enter the AP."""
    del bin_prob
    s = torch.as_tensor(score_row).reshape(-1)
    y = torch.as_tensor(labels).reshape(-1).to(s.device)
    vis = torch.as_tensor(np.asarray(visible_idx) if not isinstance(visible_idx, torch.Tensor)
                          else visible_idx).reshape(-1).long().to(s.device)
    return {'map': average_precision(y, s),
            'map_visible': average_precision(y[vis], s[vis])}
