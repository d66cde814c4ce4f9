"""Yardsticks of tests/test_optim_step*.py, independent of veon_amd/optim.py: clip + AdamW +
EMA restated in fp64 from their definitions, the reference's two EMA lines, and the
parameter sets the tests share."""
import math

import torch


# ------------------------------------------------------------------ the reference's EMA
def reference_ema_lines(v, d, msd_k):
    """mmdet3d/core/hook/ema.py:58-59 on one state_dict entry, in place."""
    v *= d
    v += (1.0 - d) * msd_k.detach()


def reference_decay(decay, updates):
    """ema.py:44."""
    return decay * (1 - math.exp(-updates / 2000))


# ------------------------------------------------------------------ fp64 restatement
class Fp64Step:
    """clip_grad_norm_(max_norm, 2) + AdamW (decoupled weight decay, bias-corrected
    moments) + EMA on fp64 copies of a list of tensors, every scalar in double."""

    def __init__(self, params, emas=None):
        self.p = [t.detach().double().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.e = None if emas is None else [t.detach().double().clone() for t in emas]
        self.t = 0
        self.norm = None

    def step(self, grads, lr, betas, eps, weight_decay, max_norm=None, d=None):
        """``lr`` and ``weight_decay``: one number, or one per tensor."""
        g = [t.detach().double() for t in grads]
        self.t += 1
        if max_norm is not None:
            self.norm = math.sqrt(sum(float((t * t).sum()) for t in g))
            coef = min(max_norm / (self.norm + 1e-6), 1.0)
            if math.isnan(self.norm):
                coef = float('nan')
            g = [t * coef for t in g]
        b1, b2 = betas
        per = lambda x, i: x[i] if isinstance(x, (list, tuple)) else x  # noqa: E731
        for i, gi in enumerate(g):
            self.p[i] *= 1.0 - per(lr, i) * per(weight_decay, i)
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * gi
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * gi * gi
            m_hat = self.m[i] / (1.0 - b1 ** self.t)
            v_hat = self.v[i] / (1.0 - b2 ** self.t)
            self.p[i] -= per(lr, i) * m_hat / (v_hat.sqrt() + eps)
            if self.e is not None:
                self.e[i] = d * self.e[i] + (1.0 - d) * self.p[i]


def scaled_error(got, want64):
    """max |got - want| / max |want| (0 for an empty tensor)."""
    if want64.numel() == 0:
        return 0.0
    return float((got.double() - want64).abs().max() / want64.abs().max().clamp_min(1e-300))


def wide_grads(shape, generator):
    """Gaussian times 10^k, k uniform in -4 .. 1 per element."""
    k = torch.randint(-4, 2, shape, generator=generator).float()
    return torch.randn(shape, generator=generator) * 10.0 ** k
