"""fp64 closed forms and operand builders for the native training of the CLIP tail
(csrc/attention_train.hip with a dense additive bias, the QuickGELU pair of
csrc/linear_train.hip), shared by tests/test_clip_tail_train.py (CPU) and
tests/test_clip_tail_train_gpu.py.  A plain module: no fixtures, nothing device-specific
(every function computes where its operands live) and nothing of the code under test.

Layouts: qkv [B, T, 3 H 64] and dout [B, T, H 64] as the kernels take them; per-head
tensors are [B, H, T, .].  A bias is (B, H, Tb, Tb), (1 | B, 1 | H, Tb, Tb), (B H, Tb, Tb)
or (Tb, Tb) with Tb = T - border; ``full_bias`` makes the (B, H, T, T) matrix the formula
adds, the border by zero padding.
"""
import torch

HD = 64
SCALE = 0.125
LOG2E = 1.4426950408889634
NEG = float('-inf')


def full_bias(bias, B, H, T, border):
    Tb = T - border
    if bias.dim() == 3:
        bias = bias.reshape(B, H, Tb, Tb)
    elif bias.dim() == 2:
        bias = bias.reshape(1, 1, Tb, Tb)
    if border:
        z = bias.new_zeros(bias.shape[:2] + (T, T))
        z[:, :, 1:, 1:] = bias
        bias = z
    return bias.expand(B, H, T, T)


def reduce_dbias(dense, like):
    """The dense (B, H, Tb, Tb) gradient summed to the shape of the bias ``like``."""
    if like.dim() == 2:
        return dense.sum((0, 1))
    if like.dim() == 3:
        return dense.reshape(like.shape)
    axes = [a for a in (0, 1) if like.shape[a] == 1 and dense.shape[a] > 1]
    return dense.sum(axes, keepdim=True) if axes else dense


def _split(qkv, H):
    B, T = qkv.shape[:2]
    return qkv.reshape(B, T, 3, H, HD).permute(2, 0, 3, 1, 4)


def scores(qkv, bias, H, border, scale=SCALE):
    """scale q k^T + bias, (B, H, T, T), in qkv's dtype (pass fp64)."""
    B, T = qkv.shape[:2]
    q, k, _ = _split(qkv, H)
    return (q * scale) @ k.transpose(-2, -1) + full_bias(bias.to(qkv.dtype), B, H, T, border)


def dead_rows(s):
    """(B, H, T, 1) bool: queries whose keys are all masked."""
    return (s == NEG).all(-1, keepdim=True)


def probabilities(s):
    """softmax over the keys; a fully masked query has P = 0 BY DEFINITION (torch: NaN)."""
    dead = dead_rows(s)
    return torch.where(dead, torch.zeros_like(s), s.masked_fill(dead, 0.0).softmax(-1))


def forward(qkv, bias, H, border, scale=SCALE):
    """-> (out [B, T, H 64], lse (B, H, T) in log2 units, +inf for a fully masked query)."""
    B, T = qkv.shape[:2]
    s = scores(qkv, bias, H, border, scale)
    v = _split(qkv, H)[2]
    out = (probabilities(s) @ v).transpose(1, 2).reshape(B, T, H * HD)
    lse = torch.logsumexp(s, -1) * LOG2E
    return out, torch.where(dead_rows(s).squeeze(-1), torch.full_like(lse, float('inf')), lse)


def backward(qkv, bias, dout, H, border, scale=SCALE):
    """The closed form -> (dqkv [B, T, 3 H 64], dbias dense (B, H, Tb, Tb)):
    dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dO o O)), dQ = scale dS K,
    dK = scale dS^T Q, dbias = dS inside the border.  With P = 0 for a fully masked query,
    its dq and dbias rows are zero and it adds nothing to dk, dv."""
    B, T = qkv.shape[:2]
    q, k, v = _split(qkv, H)
    do = dout.reshape(B, T, H, HD).permute(0, 2, 1, 3)
    P = probabilities(scores(qkv, bias, H, border, scale))
    O = P @ v
    dS = P * (do @ v.transpose(-2, -1) - (do * O).sum(-1, keepdim=True))
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-2, -1) @ q), P.transpose(-2, -1) @ do
    dqkv = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * HD)
    return dqkv, dS[:, :, border:, border:]


def quickgelu(y):
    return y * torch.sigmoid(1.702 * y)


def quickgelu_bwd(dh, y):
    s = torch.sigmoid(1.702 * y)
    return dh * (s + 1.702 * y * s * (1 - s))


# ------------------------------------------------------------------------------ operands
BIAS_KINDS = ('full', 'heads', 'matrix')     # (B, H, ..), (B, 1, ..), (Tb, Tb)


def gram_bias(B, T, H, border, kind, gen, dtype=torch.float32):
    """E E^T with E ~ N(0, 0.5) of width 32: a large positive diagonal, as the model's
    Gram-shaped biases have."""
    Tb = T - border
    lead = {'full': (B, H), 'heads': (B, 1), 'matrix': ()}[kind]
    E = torch.randn(*lead, Tb, 32, generator=gen) * 0.5 ** 0.5
    return (E @ E.transpose(-2, -1)).to(dtype)


def mask_some_(bias, border):
    """-inf at [r][(r + 1) % Tb] of every even row r (Tb >= 2): no query loses every key.
    Tb == 1 with a border: the one element (the class token stays a live key)."""
    Tb = bias.shape[-1]
    if Tb >= 2:
        r = torch.arange(0, Tb, 2)
        bias[..., r, (r + 1) % Tb] = NEG
    elif Tb == 1 and border:
        bias[..., 0, 0] = NEG
    return bias


def operands(B, T, H, gen, dtype=torch.float64):
    """(qkv, dout): N(0, 1), as the raw output of a qkv Linear and an upstream gradient."""
    return (torch.randn(B, T, 3 * H * HD, generator=gen).to(dtype),
            torch.randn(B, T, H * HD, generator=gen).to(dtype))
