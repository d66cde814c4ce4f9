"""References and tolerances of the fused 2-D semantic tail (veon_amd/sem2d.py), shared by
tests/test_sem2d.py and tests/test_sem2d_gpu.py.

Tolerance.  Against the fp64 restatement ``ref64`` an output element with weights
``W[b, :, c]`` (class probabilities, or mask embeddings) may differ by at most

    bound[b, c] = 2 * eps32 * (Q + 8 + max|mask_preds|) * sum_q |W[b, q, c]|

``Q * eps`` for the fp32 dot product over the proposals, ``8 * eps`` for the rounding of
softmax, interpolation and sigmoid in each term, ``max|m| * eps`` for the rounding of the
sigmoid's argument (slope at most 1/4), and a factor of 2 for safety.  Against values
that were themselves computed in fp32 (the recorded fixture, the torch tail) the allowance
is ``2 * bound``: both sides carry the error.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)
SEED = 11     # of the random cases; tests/test_sem2d.py re-checks the label statistics for it

# (B, Q, K, C, h, w, H, W): the smallest shapes at which tiles, tails and clamps can go wrong
SHAPES = {
    'fixture': (2, 5, 4, 24, 4, 6, 64, 96),
    'production_q_odd_source': (2, 100, 17, 40, 3, 5, 48, 80),
    'one_class_fractional_scale': (1, 7, 1, 3, 5, 7, 33, 50),
    'wide_classes': (2, 100, 67, 520, 4, 6, 64, 96),
    'q_past_128_prime_output': (1, 129, 17, 8, 2, 3, 37, 41),
    # the kernel's other paths: the general class instantiation (K > 72); two passes over
    # the classes (K > 128) with the proposals in two LDS chunks (Q > 64 at 128 columns);
    # a downscale whose tiles need more source pixels than LDS holds (sampled from memory;
    # the smallest such grid: the fp32 source index, which is ATen's arithmetic and not
    # part of the bound, rounds by half an ulp of the index, so its share grows with h, w)
    'general_classes': (1, 9, 75, 3, 3, 4, 10, 70),
    'two_class_passes': (1, 70, 131, 3, 2, 3, 9, 66),
    'downscale_unstaged': (1, 12, 2, 2, 66, 64, 5, 7),
}


def random_inputs(shape, seed):
    """mask_logits ~ 4 N(0,1), mask_embs ~ N(0,1), mask_preds ~ 6 N(0,1); every batch
    element differs."""
    B, Q, K, C, h, w, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = 4.0 * torch.randn(B, Q, K + 1, generator=g)
    embs = torch.randn(B, Q, C, generator=g)
    preds = 6.0 * torch.randn(B, Q, h, w, generator=g)
    return logits, embs, preds


# Shapes whose fp64 reference takes the source index and the two weights of every output
# index as ATen's fp32 arithmetic gives them (and blends in fp64).  The index rounds by half
# an ulp OF THE INDEX, which the bound does not hold: on a source grid of 64 and more pixels
# torch's own fp32 tail is 0.5 of the bound away from an fp64 index and more.
ATEN_INDEX = ('downscale_unstaged',)


def _axis(dst_size, src_size):
    scale = torch.tensor(src_size, dtype=torch.float32) / torch.tensor(dst_size,
                                                                       dtype=torch.float32)
    src = (scale * (torch.arange(dst_size, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0)
    i0 = src.to(torch.int64)
    l1 = src - i0.to(torch.float32)
    return i0, i0 + (i0 < src_size - 1).to(torch.int64), (1.0 - l1).double(), l1.double()


def interpolate_aten_index(preds64, size):
    y0, y1, ly0, ly1 = _axis(size[0], preds64.shape[2])
    x0, x1, lx0, lx1 = _axis(size[1], preds64.shape[3])
    top, bot = preds64[:, :, y0], preds64[:, :, y1]
    return ly0[:, None] * (lx0 * top[..., x0] + lx1 * top[..., x1]) + \
        ly1[:, None] * (lx0 * bot[..., x0] + lx1 * bot[..., x1])


def ref64(logits, embs, preds, size, aten_index=False):
    """fp64: (sem_seg_ds, sem_embed_ds, sem_seg) of the reference's lines."""
    logits, preds = logits.double(), preds.double()
    cls = F.softmax(logits, dim=-1)[..., :-1]
    sig = preds.sigmoid()
    seg_ds = torch.einsum('bqc,bqhw->bchw', cls, sig)
    emb_ds = None if embs is None else torch.einsum('bqc,bqhw->bchw', embs.double(), sig)
    if aten_index:
        up = interpolate_aten_index(preds, tuple(size))
    else:
        up = F.interpolate(preds, size=tuple(size), mode='bilinear', align_corners=False)
    seg = torch.einsum('bqc,bqhw->bchw', cls, up.sigmoid())
    return seg_ds, emb_ds, seg


def bound(weights, preds, max_pred=None):
    """(B, C) tolerance of a map with weights (B, Q, C) (see the module docstring);
    ``max_pred`` replaces max|mask_preds| (0 where the sigmoid is saturated and the
    rounding of its argument cannot matter)."""
    Q = weights.shape[1]
    m = float(preds.abs().max()) if max_pred is None else float(max_pred)
    return 2.0 * EPS32 * (Q + 8.0 + m) * weights.double().abs().sum(dim=1)


def class_bound(logits, preds, max_pred=None):
    return bound(F.softmax(logits.double(), dim=-1)[..., :-1], preds, max_pred)


def excess(got, ref, tol, factor=1.0):
    """max over elements of |got - ref| / (factor * tol[b, c]); <= 1 passes."""
    err = (got.detach().double().cpu() - ref.double().cpu()).abs()
    return float((err / (factor * tol.cpu()[:, :, None, None])).max())


def taps(dst_size, src_size):
    """(i0, i1) int64 (dst_size,): the two source indices of every output index, by
    ATen's align_corners=False arithmetic in fp32."""
    return _axis(dst_size, src_size)[:2]


def touched(size, src_hw, y, x):
    """bool (H, W): the output pixels of which one of the four taps is source pixel (y, x)."""
    y0, y1 = taps(size[0], src_hw[0])
    x0, x1 = taps(size[1], src_hw[1])
    return ((y0 == y) | (y1 == y))[:, None] & ((x0 == x) | (x1 == x))[None, :]


def loop_labels(sem, group, n_merged, ignore_label=255):
    """Hand-written: per pixel, the maximum of every run of rows, then the lowest merged
    channel that attains the overall maximum; ``ignore_label`` where any row is NaN."""
    sem = sem.cpu().numpy()
    B, K, H, W = sem.shape
    group = list(range(K)) if group is None else list(group)
    n_merged = K if n_merged is None else n_merged
    out = np.zeros((B, H, W), dtype=np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                v = sem[b, :, y, x]
                if np.isnan(v).any():
                    out[b, y, x] = ignore_label
                    continue
                merged = [max(v[c] for c in range(K) if group[c] == ch)
                          for ch in range(n_merged)]
                out[b, y, x] = min(ch for ch in range(n_merged) if merged[ch] == max(merged))
    return torch.from_numpy(out)


def top_two_margin(sem64, group=None, n_merged=None):
    """fp64 (B, H, W): best minus second-best merged channel (inf with one channel)."""
    from veon_amd.sem2d import merge_runs_torch
    merged = sem64 if group is None else merge_runs_torch(sem64, list(group), n_merged)
    if merged.shape[1] == 1:
        return torch.full_like(merged[:, 0], float('inf'))
    top = merged.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


GROUP_67_17 = [c * 17 // 67 for c in range(67)]      # 67 rows in 17 runs of 3 or 4
