"""Shared by the depth pre-training loss tests (test_depth_loss.py, test_depth_loss_gpu.py):
the seeded input builder with its planted hostile cases, and the closed form of the loss
and of its gradient evaluated in fp64 torch.

The closed form (a row is one output pixel; d / t the block-min of its prediction / label
block with zeros read as 1e5; the gradient of d goes to the first minimal pixel in
(dy, dx) row-major order and is zero when that pixel was a zero):

  zoe   valid rows t < 9225; g = log(d + 1e-7) - log(t + 1e-7); n, m = mean g,
        Dg = sum (g - m)^2/(n - 1) + 0.15 m^2; loss = min(sqrt Dg, 2);
        d loss/d d = [(g - m)/(n - 1) + 0.15 m/n] / sqrt Dg / (d + 1e-7), 0 when clipped
  ce    c_k = k*step + (lo + step/2) (fp32, k = 0..D); k* = argmax_k -|min(t, 500) - c_k|;
        foreground iff k* < D; p = softmax_k max(-gamma |d - c_k|, -16);
        row = -log p_k* - sum_{k<D, k != k*} log(1 - p_k); loss = 0.05 sum_fg row/max(1, n_fg)
        e_k = (p_k - y_k)/max(p_k (1 - p_k), 1e-12) (k < D), e_D = 0;
        d row/d d = sum_k p_k (e_k - sum_j p_j e_j) (-gamma sign(d - c_k))
  depth_error = mean |d - t| over the valid rows."""
import torch

from veon_amd import depth_loss

GRIDS = {64: (1.0, 32.5, 0.5), 65: (1.0, 33.0, 0.5), 89: (1.0, 45.0, 0.5), 60: (1.0, 60.0, 1.0)}


def grid_bins(grid):
    """(D, lo, step) of a [lo, hi, step] depth grid, D as LSSCore counts it."""
    lo, hi, step = grid
    return int(torch.arange(lo, hi, step).shape[0]), lo, step


def blocks(x, s):
    """(B,N,H,W) -> (rows, s*s) blocks in (dy, dx) row-major order."""
    B, N, H, W = x.shape
    return x.view(B * N, H // s, s, W // s, s).permute(0, 1, 3, 2, 4).reshape(-1, s * s)


def unblocks(rows, shape, s):
    B, N, H, W = shape
    return rows.view(B * N, H // s, W // s, s, s).permute(0, 1, 3, 2, 4).reshape(B, N, H, W)


def make_inputs(seed, B, N, Hg, Wg, grid, sp=8, sg=16, clipped=False, plant=True):
    """-> (depth (B,N,Hp,Wp), gt_depth (B,N,Hg,Wg)) fp32 on the CPU.

    Per-row target depths uniform in [2, 42]; labels = target + U(0, 2) on about 10 % of
    the pixels, zero elsewhere; predictions = target (1 + 0.15 N(0,1)) + U(0, 3), or
    U(0.5, 50.5), times 100 on every other row, for the clipped regime.  ``plant`` writes the hostile cases into rows
    0.. (as many as the map has rows for)."""
    D, lo, step = grid_bins(grid)
    h, w = Hg // sg, Wg // sg
    Hp, Wp = h * sp, w * sp
    g = torch.Generator().manual_seed(seed)
    rows = B * N * h * w
    target = 2.0 + 40.0 * torch.rand(rows, generator=g)
    lab = target[:, None] + 2.0 * torch.rand(rows, sg * sg, generator=g)
    lab = lab * (torch.rand(rows, sg * sg, generator=g) < 0.1)
    if clipped:
        pred = 0.5 + 50.0 * torch.rand(rows, sp * sp, generator=g)
        pred[1::2] *= 100.0       # keeps sqrt(Dg) > 2 however many rows there are
    else:
        pred = target[:, None] * (1 + 0.15 * torch.randn(rows, sp * sp, generator=g)) \
            + 3.0 * torch.rand(rows, sp * sp, generator=g)
    pred = pred.clamp_min(0.05)
    centers = depth_loss.bin_centers(D, lo, step)
    if plant:
        last = float(centers[-1])

        def only_label(r, i, v):
            lab[r].zero_()
            lab[r, i] = v

        def all_zero_far(r):      # d = 1e5 against a far label: valid, not foreground
            pred[r].zero_()
            only_label(r, 2, 9224.9)

        def on_centre(r):
            pred[r].clamp_min_(float(centers[7]) + 1.0)
            pred[r, sp * sp // 2] = float(centers[7])

        def tie(r):               # two equal minima at (0,0) and (1,1)
            pred[r].clamp_min_(6.0)
            pred[r, 0] = pred[r, sp + 1 if sp > 1 else 0] = 5.4

        plants = [
            ('pred_zeros', lambda r: pred[r].__setitem__(slice(0, sp * sp, 3), 0.0)),
            ('pred_all_zero_label_9224_9', all_zero_far),
            ('label_all_zero', lambda r: lab[r].zero_()),
            ('label_beyond', lambda r: only_label(r, 1, last + 7.3)),
            ('label_over_500', lambda r: only_label(r, 0, 731.0)),
            ('label_9225', lambda r: only_label(r, 3, 9225.0)),
            ('pred_on_centre', on_centre),
            ('pred_tie', tie),
            # d = 1e5 on a foreground row (every gap clamped, uniform p): its log
            # difference alone clips the zoe term of a small map, so only from 64 rows on
            ('pred_all_zero', lambda r: pred[r].zero_() if rows >= 64 else None),
        ]
        for r, (_, fn) in enumerate(plants[:rows]):
            fn(r)
    depth = unblocks(pred, (B, N, Hp, Wp), sp).contiguous()
    gt = unblocks(lab, (B, N, Hg, Wg), sg).contiguous()
    # a condition on the inputs, not a tolerance: no label within 1e-4 of a midpoint
    # between two centres, so the fp32 and fp64 label bins coincide
    t = torch.where(lab == 0, torch.full_like(lab, 1e5), lab).min(1).values.clamp_max(500)
    mid = (centers[1:] + centers[:-1]) / 2
    assert float((t[:, None].double() - mid[None, :].double()).abs().min()) > 1e-4
    return depth, gt


PLANTED = ('pred_zeros', 'pred_all_zero_label_9224_9', 'label_all_zero', 'label_beyond',
           'label_over_500', 'label_9225', 'pred_on_centre', 'pred_tie', 'pred_all_zero')


def closed_form(depth, gt_depth, grid, sp=8, sg=16, gamma=4.0, w_zoe=1.0, w_ce=1.0):
    """fp64 evaluation of the module docstring's formulas -> dict(loss_depth_zoe,
    loss_depth_ce, depth_error, grad (of w_zoe*zoe + w_ce*ce, shaped as depth), zoe_grad,
    ce_grad (each loss's own gradient map), d, t, winner, label_bin, valid, fg, n, n_fg,
    clipped)."""
    D, lo, step = grid_bins(grid)
    dd = torch.float64
    pb, lb = blocks(depth.to(dd), sp), blocks(gt_depth.to(dd), sg)
    pm = torch.where(pb == 0, torch.full_like(pb, 1e5), pb)
    d = pm.min(1).values
    winner = (pm == d[:, None]).to(torch.int8).argmax(1)        # first minimal pixel
    win_zero = pb.gather(1, winner[:, None])[:, 0] == 0
    t = torch.where(lb == 0, torch.full_like(lb, 1e5), lb).min(1).values
    valid = t < 9225
    n = valid.sum().to(dd)
    g = torch.log(d + 1e-7) - torch.log(t + 1e-7)
    m = (g * valid).sum() / n
    Dg = (((g - m) ** 2) * valid).sum() / (n - 1) + 0.15 * m * m
    sq = torch.sqrt(Dg)
    clipped = bool(sq > 2.0)
    zoe = torch.clamp(sq, max=2.0)
    zrow = ((g - m) / (n - 1) + 0.15 * m / n) / sq / (d + 1e-7) * valid
    if clipped:
        zrow = torch.zeros_like(zrow)
    c = depth_loss.bin_centers(D, lo, step).to(dd)
    kstar = (-(t.clamp_max(500)[:, None] - c[None, :]).abs()).argmax(1)
    fg = kstar < D
    n_fg = fg.sum().to(dd)
    gap = (-gamma * (d[:, None] - c[None, :]).abs()).clamp_min(-16.0)
    p = torch.softmax(gap, 1)
    y = torch.zeros_like(p).scatter_(1, kstar[:, None], 1.0)
    keep = torch.ones_like(p)
    keep[:, D] = 0
    row = -(y * torch.log(p).clamp_min(-100) + (1 - y) * torch.log(1 - p).clamp_min(-100))
    row = (row * keep).sum(1)
    w = 0.05 / torch.clamp(n_fg, min=1.0)
    ce = (row * fg).sum() * w
    e = (p - y) / (p * (1 - p)).clamp_min(1e-12) * keep
    S = (p * e).sum(1, keepdim=True)
    crow = (p * (e - S) * (-gamma * torch.sign(d[:, None] - c[None, :]))).sum(1) * fg * w
    live = ~win_zero

    def scatter(rowgrad):
        out = torch.zeros_like(pb)
        out.scatter_(1, winner[:, None], (rowgrad * live)[:, None])
        return unblocks(out, depth.shape, sp)
    zg, cg = scatter(zrow), scatter(crow)
    err = ((d - t).abs() * valid).sum() / n
    return dict(loss_depth_zoe=zoe, loss_depth_ce=ce, depth_error=err,
                grad=w_zoe * zg + w_ce * cg, zoe_grad=zg, ce_grad=cg, d=d, t=t,
                winner=winner, winner_zero=win_zero, label_bin=kstar, valid=valid, fg=fg,
                n=int(n), n_fg=int(n_fg), clipped=clipped, sqrt_Dg=float(sq))


def mirror_with_grad(depth, gt_depth, grid, sp=8, sg=16, dtype=None, device=None,
                     w_zoe=1.0, w_ce=1.0):
    """``depth_pretrain_loss_torch`` and autograd's gradient of w_zoe*zoe + w_ce*ce."""
    D, lo, step = grid_bins(grid)
    leaf = depth.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    out = depth_loss.depth_pretrain_loss_torch(leaf, gt_depth.to(device=device, dtype=dtype),
                                               D, lo, step, sp, sg)
    (w_zoe * out['loss_depth_zoe'] + w_ce * out['loss_depth_ce']).backward()
    return {k: v.detach() for k, v in out.items()}, leaf.grad
