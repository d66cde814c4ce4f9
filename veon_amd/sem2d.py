"""The semantic tail of SAN's 2-D branch in one pass (csrc/sem2d.hip): class
probabilities and mask embeddings spread over the sigmoid mask proposals
(san_in_veon_temporal.py:176-186, 240-255).

    semantic_maps_ds   sem_seg_ds (B,K,h,w) and sem_embed_ds (B,C,h,w) at the proposals'
                       own resolution
    semantic_map       sem_seg (B,K,H,W) at the image resolution; the bilinearly
                       upsampled proposals (B,Q,H,W) and their sigmoid are never formed
    semantic_labels    the arg-max of semantic_map as uint8 (B,H,W), optionally with runs
                       of rows merged by their maximum (a detailed vocabulary, as
                       ``occ_eval.occ_labels_grouped`` does in 3-D); the map is never
                       formed either

Each has a torch mirror (``*_torch``): the reference's own lines, which is the CPU path,
the path of a caller who needs gradients, and the yardstick of the tests.  Native on a
ROCm device: fp32, sums over the proposals in index order, bit-reproducible, no
synchronisation, capturable in a graph.  Q <= 256 proposals and K + 1 <= 256 logit
columns, beyond that ``ValueError`` (on either device; never a fallback).  +-inf in
``mask_preds`` is undefined; NaN propagates to every pixel whose four taps touch it.
"""
import torch
import torch.nn.functional as F

from . import _lib
from .occ_eval import _group_arg
from .vocabulary import group_table, lowest_argmax, merge_runs as merge_runs_torch

MAX_Q = 256
MAX_COLUMNS = 256     # K + 1


# ------------------------------------------------------------------ torch mirrors
def semantic_maps_ds_torch(mask_logits, mask_embs, mask_preds):
    """``semantic_inference_2d_w_embed`` (san_in_veon_temporal.py:248-255)."""
    cls = F.softmax(mask_logits, dim=-1)[..., :-1]
    sig = mask_preds.sigmoid()
    seg = torch.einsum('bqc,bqhw->bchw', cls, sig)
    emb = None if mask_embs is None else torch.einsum('bqc,bqhw->bchw', mask_embs, sig)
    return seg, emb


def semantic_map_torch(mask_logits, mask_preds, size):
    """san_in_veon_temporal.py:179-185 + ``semantic_inference_2d`` (:240-246)."""
    up = F.interpolate(mask_preds, size=tuple(int(v) for v in size), mode='bilinear',
                       align_corners=False)
    return torch.einsum('bqc,bqhw->bchw', F.softmax(mask_logits, dim=-1)[..., :-1],
                        up.sigmoid())


def labels_of_map(sem, group=None, n_merged=None, ignore_label=255):
    """uint8 (B,H,W) of a semantic map (B,K,H,W): runs of rows merged by their maximum,
    the lowest (merged) channel that attains the maximum, ``ignore_label`` where any row
    is NaN."""
    cls, _ = lowest_argmax(sem if group is None else merge_runs_torch(sem, group,
                                                                       n_merged))
    bad = torch.isnan(sem).any(dim=1)
    return torch.where(bad, torch.full_like(cls, ignore_label), cls).to(torch.uint8)


def semantic_labels_torch(mask_logits, mask_preds, size, group=None, n_merged=None,
                          ignore_label=255):
    return labels_of_map(semantic_map_torch(mask_logits, mask_preds, size), group, n_merged,
                         ignore_label)


# ------------------------------------------------------------------ checks
def _shapes(mask_logits, mask_embs, mask_preds):
    if mask_logits.dim() != 3 or mask_preds.dim() != 4:
        raise ValueError('mask_logits must be (B,Q,K+1) and mask_preds (B,Q,h,w), got %s and %s'
                         % (tuple(mask_logits.shape), tuple(mask_preds.shape)))
    B, Q, K1 = mask_logits.shape
    if tuple(mask_preds.shape[:2]) != (B, Q):
        raise ValueError('mask_logits is for %d x %d proposals, mask_preds for %d x %d'
                         % (B, Q, mask_preds.shape[0], mask_preds.shape[1]))
    if mask_embs is not None and (mask_embs.dim() != 3 or tuple(mask_embs.shape[:2]) != (B, Q)
                                  or mask_embs.shape[2] < 1):
        raise ValueError('mask_embs must be (%d,%d,C), got %s' % (B, Q, tuple(mask_embs.shape)))
    if not 1 <= Q <= MAX_Q:
        raise ValueError('the semantic tail takes 1 to %d proposals, got %d' % (MAX_Q, Q))
    if not 2 <= K1 <= MAX_COLUMNS:
        raise ValueError('the semantic tail takes 2 to %d logit columns (the void column '
                         'last), got %d' % (MAX_COLUMNS, K1))
    h, w = mask_preds.shape[2:]
    if B < 1 or h < 1 or w < 1:
        raise ValueError('empty input: mask_preds is %s' % (tuple(mask_preds.shape),))
    return B, Q, K1 - 1, h, w


def _size(size):
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise ValueError('the output size must be positive, got %s' % ((H, W),))
    return H, W


def _group(group, n_merged, ignore_label, K):
    ignore_label = int(ignore_label)
    if not 0 <= ignore_label <= 255:
        raise ValueError('ignore_label must be in [0, 255], got %d' % ignore_label)
    if group is None:
        if n_merged is not None:
            raise ValueError('n_merged is given without a group table')
        return None, None, ignore_label
    if n_merged is None:
        raise ValueError('a group table needs n_merged')
    return group_table(group, n_merged, ignore_label, K), int(n_merged), ignore_label


def _native(*tensors):
    """The kernels run without autograd: a caller who needs gradients keeps the mirror."""
    first = tensors[0]
    if not first.is_cuda:
        return False
    return not (torch.is_grad_enabled()
                and any(t is not None and t.requires_grad for t in tensors))


def _f32(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------ public calls
def semantic_maps_ds(mask_logits, mask_embs, mask_preds):
    """-> (sem_seg_ds (B,K,h,w), sem_embed_ds (B,C,h,w) or None).  ``mask_logits``
    (B,Q,K+1), ``mask_embs`` (B,Q,C) or None, ``mask_preds`` (B,Q,h,w)."""
    B, Q, K, h, w = _shapes(mask_logits, mask_embs, mask_preds)
    if not _native(mask_logits, mask_embs, mask_preds):
        return semantic_maps_ds_torch(mask_logits, mask_embs, mask_preds)
    logits, embs, preds = _f32(mask_logits), _f32(mask_embs), _f32(mask_preds)
    dev = _lib.require_device(logits, embs, preds)
    C = 0 if embs is None else embs.shape[2]
    probs = torch.empty((B, Q, K), dtype=torch.float32, device=dev)
    seg = torch.empty((B, K, h, w), dtype=torch.float32, device=dev)
    emb = None if embs is None else torch.empty((B, C, h, w), dtype=torch.float32, device=dev)
    _lib.launch('veon_sem2d_ds', dev, logits, embs, preds, B, Q, K, C, h, w, probs, seg, emb)
    return seg, emb


def semantic_map(mask_logits, mask_preds, size):
    """-> sem_seg (B,K,H,W) at ``size`` = (H, W): ``F.interpolate(mask_preds, size,
    'bilinear', align_corners=False)``, sigmoid and the contraction with the class
    probabilities, fused per output pixel."""
    B, Q, K, h, w = _shapes(mask_logits, None, mask_preds)
    H, W = _size(size)
    if not _native(mask_logits, mask_preds):
        return semantic_map_torch(mask_logits, mask_preds, (H, W))
    logits, preds = _f32(mask_logits), _f32(mask_preds)
    dev = _lib.require_device(logits, preds)
    probs = torch.empty((B, Q, K), dtype=torch.float32, device=dev)
    seg = torch.empty((B, K, H, W), dtype=torch.float32, device=dev)
    _lib.launch('veon_sem2d_full', dev, logits, preds, B, Q, K, h, w, H, W, probs, seg)
    return seg


def semantic_labels(mask_logits, mask_preds, size, group=None, n_merged=None,
                    ignore_label=255):
    """-> uint8 labels (B,H,W): the arg-max over the rows of ``semantic_map`` (the same
    values bit for bit, never written).  ``group`` (K ints, ``vocabulary.group_table``; with
    ``n_merged``): the merged channel of every row -- each run of rows is merged by its
    maximum and the label is the merged channel.  The lowest channel that attains the
    maximum wins; a pixel with a NaN in any row gets ``ignore_label``."""
    B, Q, K, h, w = _shapes(mask_logits, None, mask_preds)
    H, W = _size(size)
    group, n_merged, ignore_label = _group(group, n_merged, ignore_label, K)
    if not _native(mask_logits, mask_preds):
        with torch.no_grad():
            return semantic_labels_torch(mask_logits, mask_preds, (H, W), group, n_merged,
                                         ignore_label)
    logits, preds = _f32(mask_logits), _f32(mask_preds)
    dev = _lib.require_device(logits, preds)
    probs = torch.empty((B, Q, K), dtype=torch.float32, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    _lib.launch('veon_sem2d_labels', dev, logits, preds, B, Q, K, h, w, H, W,
                None if group is None else _group_arg(group), n_merged or 0, ignore_label,
                probs, labels)
    return labels
