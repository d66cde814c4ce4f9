"""Torch-level wrappers of the fusion-layer training kernels (csrc/fusion_train.hip):
the bilinear resize into channels-last rows and its adjoint, the dual LayerNorm forward
and backward, and the join / split around the ReLU.  Everything launches on the current
stream and nothing is read back; there is no CPU path (``axis_table`` alone is host code).
"""
import numpy as np
import torch

from . import _lib
from . import half as _half
from .conv3d_ops import _workspace

MAX_C = 2048      # widest concatenated row of the dual LayerNorm


def axis_table(n_in, n_out):
    """The bilinear filter (align_corners=False, no antialias) of one axis, in fp32 with
    torch's arithmetic: {'i0', 'i1' int32 [n_out], 'l1' float32 [n_out]} for the forward
    (destination d = (1 - l1) src[i0] + l1 src[i1]) and {'first', 'last' int32 [n_in]} for
    the adjoint (source s is read by the destinations first[s] <= d < last[s] and by no
    other; first == last where nothing reads it).

    src = max((d + 0.5f) * (float(in) / out) - 0.5f, 0) with the multiply-subtract as ONE
    fused operation, which is what torch's compiled kernels evaluate (their compilers
    contract it); here: exact in fp64 (a 24-bit by 24-bit product less one half), rounded to
    fp32 once.  The unfused form moves l1 by an ulp or two of src at non-integer ratios."""
    scale = np.float32(n_in) / np.float32(n_out)
    fused = (np.arange(n_out, dtype=np.float64) + 0.5) * np.float64(scale) - 0.5
    src = np.maximum(fused.astype(np.float32), np.float32(0))
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1).astype(np.int32)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    first = np.zeros(n_in, dtype=np.int32)
    last = np.zeros(n_in, dtype=np.int32)
    for s in range(n_in):
        hit = np.nonzero((i0 == s) | (i1 == s))[0]
        if hit.size:
            first[s], last[s] = hit[0], hit[-1] + 1
            assert hit.size == last[s] - first[s]       # one range: i0 is monotone
    return dict(i0=i0, i1=i1, l1=l1, first=first, last=last)


_TABLES = {}


def device_table(n_in, n_out, device):
    """``axis_table`` packed for the kernels (i0 | i1 | l1 | first | last as 32-bit words),
    uploaded once per (n_in, n_out, device)."""
    key = (int(n_in), int(n_out), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        t = axis_table(n_in, n_out)
        words = np.concatenate([t['i0'], t['i1'], t['l1'].view(np.int32), t['first'],
                                t['last']])
        assert words.size == 3 * n_out + 2 * n_in
        tab = _TABLES[key] = torch.from_numpy(words).to(device)
    return tab


def _tables(x_shape, size, device):
    (Hin, Win), (H, W) = x_shape[-2:], size
    if (Hin, Win) == (H, W):
        return None, None
    return device_table(Hin, H, device), device_table(Win, W, device)


def _check_map(x):
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4


def resize_cat(x1, x2, size):
    """x1 (N, C1, H1, W1), x2 (N, C2, H2, W2) fp32 NCHW -> fp32 rows [N*H*W, C1 + C2]:
    both maps resized to ``size`` = (H, W) as ``F.interpolate(mode='bilinear',
    align_corners=False)`` does, channels last, x1's channels first."""
    dev = _lib.require_device(x1, x2)
    _check_map(x1)
    _check_map(x2)
    H, W = (int(v) for v in size)
    N, C1 = x1.shape[:2]
    C2 = x2.shape[1]
    assert x2.shape[0] == N
    C = C1 + C2
    rc = torch.empty((N * H * W, C), dtype=torch.float32, device=dev)
    for x, coff in ((x1, 0), (x2, C1)):
        ty, tx = _tables(x.shape, (H, W), dev)
        _lib.launch('veon_fusion_resize_cat', dev, x, rc, ty, tx, N, x.shape[1], x.shape[2],
                    x.shape[3], H, W, C, coff)
    return rc


def resize_adjoint(drc, x_shape, size, coff, out=None):
    """The adjoint of one map's resize: drc fp32 [N*H*W, C], of which the map owns columns
    ``coff .. coff + Cin`` -> its gradient, fp32 NCHW of ``x_shape``.  Every element of the
    result is written (zero where no token reads the pixel)."""
    dev = _lib.require_device(drc)
    N, Cin, Hin, Win = (int(v) for v in x_shape)
    H, W = (int(v) for v in size)
    assert drc.dtype == torch.float32 and drc.is_contiguous() and drc.dim() == 2
    assert drc.shape[0] == N * H * W
    if out is None:
        out = torch.empty((N, Cin, Hin, Win), dtype=torch.float32, device=dev)
    _check_map(out)
    assert tuple(out.shape) == (N, Cin, Hin, Win)
    ty, tx = _tables(x_shape, (H, W), dev)
    _lib.launch('veon_fusion_resize_adjoint', dev, drc, out, ty, tx, N, Cin, Hin, Win, H, W,
                drc.shape[1], int(coff))
    return out


def _vec(t, n):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n


def dual_layernorm(rc, C1, gamma1, beta1, eps1, gamma2, beta2, eps2):
    """rc fp32 [M, C] -> (half [M, C] = LN1(rc), half [M, C - C1] = LN2(rc[:, C1:])) from one
    read of every row.  C1 and C - C1 multiples of 64, C <= 2048."""
    dev = _lib.require_device(rc, gamma1, beta1, gamma2, beta2)
    assert rc.dtype == torch.float32 and rc.is_contiguous() and rc.dim() == 2
    M, C = rc.shape
    C2 = C - C1
    for t, n in ((gamma1, C), (beta1, C), (gamma2, C2), (beta2, C2)):
        _vec(t, n)
    xn1 = torch.empty((M, C), dtype=_half.dtype(), device=dev)
    xn2 = torch.empty((M, C2), dtype=_half.dtype(), device=dev)
    _lib.launch('veon_fusion_dual_ln', dev, rc, gamma1, beta1, gamma2, beta2, xn1, xn2, M,
                int(C1), C2, float(eps1), float(eps2))
    return xn1, xn2


def dual_layernorm_bwd(dxn1, dxn2, rc, C1, gamma1, eps1, gamma2, eps2, out=None):
    """Backward of ``dual_layernorm`` at its stored input: half dxn1 [M, C], dxn2 [M, C2]
    -> (drc fp32 [M, C], dgamma1, dbeta1 [C], dgamma2, dbeta2 [C2]); the x2 columns of drc
    are the sum of both branches.  Deterministic: two stages in a fixed order."""
    dev = _lib.require_device(dxn1, dxn2, rc, gamma1, gamma2)
    _lib.require_half(dxn1, dxn2)
    assert rc.dtype == torch.float32 and rc.is_contiguous() and rc.dim() == 2
    M, C = rc.shape
    C2 = C - C1
    assert dxn1.is_contiguous() and dxn1.shape == (M, C)
    assert dxn2.is_contiguous() and dxn2.shape == (M, C2)
    _vec(gamma1, C)
    _vec(gamma2, C2)
    nbytes = int(_lib.lib().veon_fusion_dual_ln_bwd_workspace_bytes(int(C1), C2))
    if nbytes < 0:
        raise _lib.VeonHipError('dual_layernorm_bwd: unsupported widths %d + %d' % (C1, C2))
    ws = _workspace('fusion_dual_ln_bwd', nbytes, dev, int(C1), C2)
    drc = torch.empty_like(rc) if out is None else out
    assert drc.dtype == torch.float32 and drc.is_contiguous() and drc.shape == rc.shape
    sums = torch.empty(2 * C + 2 * C2, dtype=torch.float32, device=dev)
    _lib.launch('veon_fusion_dual_ln_bwd', dev, dxn1, dxn2, rc, gamma1, gamma2, drc, sums, ws,
                nbytes, M, int(C1), C2, float(eps1), float(eps2))
    return (drc, sums[:C], sums[C:2 * C], sums[2 * C:2 * C + C2], sums[2 * C + C2:])


def _half_rows(t, M):
    _lib.require_half(t)
    assert t.is_contiguous() and t.dim() == 2 and t.shape[0] == M


def join(y1, y2, p1, p2):
    """half y1 [M, ld1], y2 [M, ld2] -> fp32 [M, p1 + p2] = cat(y1[:, :p1], y2[:, :p2])."""
    dev = _lib.require_device(y1, y2)
    M = y1.shape[0]
    _half_rows(y1, M)
    _half_rows(y2, M)
    out = torch.empty((M, p1 + p2), dtype=torch.float32, device=dev)
    _lib.launch('veon_fusion_join', dev, y1, y2, out, M, int(p1), int(p2), y1.shape[1],
                y2.shape[1])
    return out


def relu_split(dout, y1, y2, p1, p2):
    """fp32 dout [M, p1 + p2] and the stored half ReLU outputs y1 [M, ld1], y2 [M, ld2] ->
    half (dy1 [M, ld1], dy2 [M, ld2]): dout where the output is positive, zero elsewhere and
    in the padding columns."""
    dev = _lib.require_device(dout, y1, y2)
    M = y1.shape[0]
    _half_rows(y1, M)
    _half_rows(y2, M)
    assert dout.dtype == torch.float32 and dout.is_contiguous()
    assert dout.shape == (M, p1 + p2)
    dy1, dy2 = torch.empty_like(y1), torch.empty_like(y2)
    _lib.launch('veon_fusion_relu_split', dev, dout, y1, y2, dy1, dy2, M, int(p1), int(p2),
                y1.shape[1], y2.shape[1])
    return dy1, dy2
