"""Inputs and fp64 references shared by tests/test_temporal_train.py (CPU) and
tests/test_temporal_train_gpu.py.  A plain module: nothing device-specific, no fixtures.

Operands are what the kernels see: volumes rounded to the flavour's half dtype; everything
after that is float64 on the CPU.
"""
import torch

from tests import edge_refs as er
from veon_amd.models.semantic_net import temporal_fusion as tfm

S = 8
EDGE = 2.0 ** -10          # voxels: the width of the band around a node that is left out


def inputs(B, hd, heads, zyx, seed, offsets='randn', qscale=1.0, surplus=0):
    """(kv, q, off, dout) fp32 CPU tensors holding half-representable values; ``off`` RAW
    offsets: 'randn' (N(0, 1.5^2)), 'zero', 'saturated' (+-8); ``surplus`` NaN channels."""
    from tests.helpers import to_half
    g = torch.Generator().manual_seed(seed)
    Z, Y, X = zyx
    C = hd * heads
    kv = to_half(torch.randn(B, 2 * C, Z, Y, X, generator=g))
    q = to_half(torch.randn(B, C, Z, Y, X, generator=g) * qscale)
    dout = to_half(torch.randn(B, C, Z, Y, X, generator=g))
    noff = heads * S * 3
    if offsets == 'zero':
        off = torch.zeros(B, noff, Z, Y, X)
    elif offsets == 'saturated':
        off = 8.0 * (torch.randint(0, 2, (B, noff, Z, Y, X), generator=g) * 2 - 1).float()
    else:
        off = torch.randn(B, noff, Z, Y, X, generator=g) * 1.5
    off = to_half(off)
    if surplus:
        off = torch.cat([off, torch.full((B, surplus, Z, Y, X), float('nan'))], dim=1)
    return kv, q, off, dout


def attend_autograd(kv, q, off, dout, heads, dtype=torch.float64, device='cpu',
                    tanh_dtype=None):
    """Autograd of ``TemporalDeformable.attend`` (the definition) at ``dtype`` on
    ``device`` on the given operands; tanh is taken in ``dtype`` on the raw offsets ->
    (out, dkv, dq, doff); doff has the channels of ``off`` (zero in the surplus)."""
    C = q.shape[1]
    mod = tfm.TemporalDeformable(C, num_heads=heads)
    noff = heads * S * 3
    kv_, q_, dout_ = (t.detach().to(device=device, dtype=dtype) for t in (kv, q, dout))
    raw = off[:, :noff].detach().to(device=device, dtype=dtype)
    for t in (kv_, q_, raw):
        t.requires_grad_(True)
    out = mod.attend(kv_, q_, torch.tanh(raw))
    dkv, dq, draw = torch.autograd.grad(out, (kv_, q_, raw), dout_)
    doff = torch.zeros(off.shape, dtype=dtype, device=device)
    doff[:, :noff] = draw
    return out.detach(), dkv, dq, doff


def coordinates(off, heads, zyx):
    """fp64 UNCLAMPED un-normalised coordinates of every sample: three tensors
    (B, heads, S, Z, Y, X) along X, Y, Z (with the axis quirk), from raw offsets."""
    Z, Y, X = zyx
    B = off.shape[0]
    o = torch.tanh(er.half_round(off[:, :heads * S * 3])).reshape(B, heads, S, 3, Z, Y, X)
    lin = [torch.linspace(-1, 1, n, dtype=torch.float64) for n in (Z, Y, X)]
    base = [lin[0].view(Z, 1, 1), lin[1].view(1, Y, 1), lin[2].view(1, 1, X)]
    n_src, n_dst = (Z, Y, X), (X, Y, Z)
    return [((base[a] + o[:, :, :, a] / n_src[a]) + 1) * 0.5 * (n_dst[a] - 1) for a in range(3)]


def doff_keep_mask(off, heads, zyx):
    """bool (B, heads*24, Z, Y, X): False for the entries (voxel, head, sample; all three
    components) the GPU test leaves out of the doff comparison: on some axis of length
    > 1 the fp64 unclamped coordinate is within 2^-10 voxel of an integer AND lies inside
    [-2^-10, n - 1 + 2^-10] -- there fp32 and fp64 may floor differently.  Computed from
    the reference alone."""
    Z, Y, X = zyx
    B = off.shape[0]
    drop = torch.zeros(B, heads, S, Z, Y, X, dtype=torch.bool)
    for f, n in zip(coordinates(off, heads, zyx), (X, Y, Z)):
        if n > 1:
            near = (f - f.round()).abs() <= EDGE
            inside = (f >= -EDGE) & (f <= n - 1 + EDGE)
            drop |= near & inside
    keep = ~drop
    return keep.unsqueeze(3).expand(-1, -1, -1, 3, -1, -1, -1).reshape(B, heads * S * 3, Z, Y, X)


def rel_l2(got, want, mask=None):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if mask is not None:
        got, want = got[mask], want[mask]
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


# the op-level cases of the GPU file: (name, B, hd, heads, zyx, seed, kwargs)
LAYOUTS = [(32, 1), (32, 2), (32, 4), (32, 8), (64, 1), (64, 2), (64, 4)]
GPU_CASES = []
for _hd, _heads in LAYOUTS:
    for _B, _zyx in [(1, (3, 5, 7)), (2, (2, 4, 4))]:
        GPU_CASES.append(('layout', _B, _hd, _heads, _zyx, _hd + _heads, {}))
for _zyx in [(2, 4, 9), (2, 3, 33), (33, 3, 2)]:
    for _hd, _heads in [(32, 4), (64, 2)]:
        GPU_CASES.append(('box', 1, _hd, _heads, _zyx, 7 + _hd, {}))
for _zyx in [(1, 5, 7), (3, 1, 7), (3, 5, 1)]:
    for _hd, _heads in [(32, 4), (64, 1)]:
        GPU_CASES.append(('len1', 2, _hd, _heads, _zyx, 31 + _hd, {}))
for _qs in [1.0, 16.0, 64.0]:
    for _hd, _heads in [(32, 4), (64, 1)]:
        GPU_CASES.append(('qscale', 2, _hd, _heads, (3, 5, 7), 21 + _hd, {'qscale': _qs}))
for _hd, _heads in [(32, 4), (64, 1), (32, 1)]:
    GPU_CASES.append(('surplus', 2, _hd, _heads, (3, 5, 7), 41, {'surplus': 8}))
for _hd, _heads in [(32, 4), (64, 2)]:
    GPU_CASES.append(('zero', 1, _hd, _heads, (5, 5, 5), 3 + _hd, {'offsets': 'zero'}))
    GPU_CASES.append(('saturated', 1, _hd, _heads, (3, 5, 7), 5 + _hd, {'offsets': 'saturated'}))
    GPU_CASES.append(('randn', 1, _hd, _heads, (3, 5, 7), 5 + _hd, {}))


def case_id(case):
    name, B, hd, heads, zyx, seed, kw = case
    return '%s-B%d-hd%d-h%d-%s' % (name, B, hd, heads, 'x'.join(map(str, zyx)))
