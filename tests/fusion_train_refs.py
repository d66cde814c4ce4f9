"""fp64 references of the fusion-layer training kernels (csrc/fusion_train.hip), on the
CPU: a restatement of ``CatFusionLift`` from its formulas, sharing no code with the
library.

 * per-axis tables of the bilinear filter (align_corners=False, no antialias) in numpy
   float32, torch's arithmetic:  src = max((d + 0.5f) * (float(in) / out) - 0.5f, 0),
   i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1 (l0 in fp32 too);
   the multiply-subtract of src is rounded ONCE (a fused multiply-add, as torch's compiled
   kernels contract it; tests/test_fusion_train.py checks that against F.interpolate);
 * the blend, both LayerNorms, their backward and the resize adjoint in fp64 from those
   fp32 weights: the same operands the kernels see.
"""
import numpy as np
import torch

# map cases of the tests: (H1, W1), (H2, W2) -> (H, W)
MAP_CASES = [((8, 22), (2, 6), (4, 11)),      # exact 2x down, non-integer up (VEON in small)
             ((4, 11), (4, 11), (4, 11)),     # both inputs identity
             ((13, 35), (3, 5), (4, 11)),     # ratio above 2: untouched source pixels
             ((1, 1), (1, 7), (4, 11))]       # an axis of size 1, i1 == i0
# widths (C1, C2, out) and the batch they run with
WIDTHS = [(64, 64, 64, 2), (64, 128, 256, 2), (384, 768, 256, 1), (384, 1024, 256, 1)]


def axis(n_in, n_out):
    """-> (i0, i1 int64 [n_out], l0, l1 float32 [n_out]) of one axis."""
    scale = np.float32(n_in) / np.float32(n_out)
    # fma(d + 0.5, scale, -0.5): the fp64 value is exact, so this is one rounding to fp32
    exact = (np.arange(n_out).astype(np.float64) + 0.5) * scale.astype(np.float64) - 0.5
    src = exact.astype(np.float32)
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i0 = np.floor(src).astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    assert src.dtype == l1.dtype == l0.dtype == np.float32
    return i0, i1, l0, l1


def axis_matrix(n_in, n_out):
    """The axis filter as a dense fp64 matrix [n_out, n_in] of the fp32 weights (the two
    taps of an edge position fall on one column and add)."""
    i0, i1, l0, l1 = axis(n_in, n_out)
    A = np.zeros((n_out, n_in))
    np.add.at(A, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(A, (np.arange(n_out), i1), l1.astype(np.float64))
    return torch.from_numpy(A)


def _identity(x, size):
    return tuple(x.shape[-2:]) == tuple(size)


def resize(x, size, absolute=False):
    """x (N, C, Hin, Win) -> fp64 (N, C, H, W); ``absolute``: sum_taps w |x| instead (the
    scale of the elementwise bounds).  A map already at ``size`` is returned as it is."""
    x = x.double().abs() if absolute else x.double()
    if _identity(x, size):
        return x
    Ay = axis_matrix(x.shape[2], size[0])
    Ax = axis_matrix(x.shape[3], size[1])
    return torch.einsum('yh,nchw,xw->ncyx', Ay, x, Ax)


def resize_adjoint(d, in_shape):
    """d fp64 (N, C, H, W), the gradient of ``resize``'s result -> (N, C, Hin, Win)."""
    if _identity(d, in_shape[-2:]):
        return d.double()
    Ay = axis_matrix(in_shape[2], d.shape[2])
    Ax = axis_matrix(in_shape[3], d.shape[3])
    return torch.einsum('yh,ncyx,xw->nchw', Ay, d.double(), Ax)


def untouched(in_shape, size):
    """bool (Hin, Win): source pixels no destination reads."""
    if tuple(in_shape[-2:]) == tuple(size):
        return torch.zeros(in_shape[-2:], dtype=torch.bool)
    uy = axis_matrix(in_shape[2], size[0]).abs().sum(0) == 0
    ux = axis_matrix(in_shape[3], size[1]).abs().sum(0) == 0
    return uy[:, None] | ux[None, :]


def rows(x):
    """(N, C, H, W) -> [N*H*W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def maps(r, N, H, W):
    """[N*H*W, C] -> (N, C, H, W)"""
    return r.view(N, H, W, -1).permute(0, 3, 1, 2)


def resize_cat(x1, x2, size, absolute=False):
    """-> fp64 rows [N*H*W, C1 + C2]"""
    return torch.cat([rows(resize(x1, size, absolute)), rows(resize(x2, size, absolute))], 1)


def layernorm(x, gamma, beta, eps):
    """Over the last axis, fp64: -> (out, xhat, rstd)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = (x - mean) * rstd
    return xhat * gamma.double() + beta.double(), xhat, rstd


def layernorm_bwd(dout, x, gamma, eps):
    """Closed form, fp64: -> (dx, dgamma, dbeta)."""
    dout = dout.double()
    _, xhat, rstd = layernorm(x, gamma, torch.zeros_like(gamma), eps)
    a = dout * gamma.double()
    dx = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    return dx, (dout * xhat).sum(0), dout.sum(0)


def dual_layernorm(rc, C1, g1, b1, eps1, g2, b2, eps2):
    return layernorm(rc, g1, b1, eps1)[0], layernorm(rc[:, C1:], g2, b2, eps2)[0]


def dual_layernorm_bwd(dxn1, dxn2, rc, C1, g1, eps1, g2, eps2):
    """-> (drc, dgamma1, dbeta1, dgamma2, dbeta2), fp64."""
    d1, dg1, db1 = layernorm_bwd(dxn1, rc, g1, eps1)
    d2, dg2, db2 = layernorm_bwd(dxn2, rc[:, C1:], g2, eps2)
    drc = d1.clone()
    drc[:, C1:] += d2
    return drc, dg1, db1, dg2, db2


def mirror_backward(x1, x2, size, dxn1, dxn2, g1, eps1, g2, eps2, dtype, device):
    """The same chain (resize, cat, both LayerNorms written as the module writes them) under
    torch autograd in ``dtype`` on ``device``, the beta gradients included: the yardstick of
    the kernels' backward (``dtype`` fp32 on the GPU) and a cross-check of the closed forms
    above (fp64 on the CPU).  -> dict of drc, dg1, db1, dg2, db2, dx1, dx2."""
    import torch.nn.functional as F
    t = dict(dtype=dtype, device=device)
    x1, x2 = x1.to(**t).requires_grad_(True), x2.to(**t).requires_grad_(True)
    g1, g2 = g1.to(**t).requires_grad_(True), g2.to(**t).requires_grad_(True)
    b1, b2 = torch.zeros_like(g1, requires_grad=True), torch.zeros_like(g2, requires_grad=True)

    def rs(x):
        if _identity(x, size):
            return x
        return F.interpolate(x, size=size, mode='bilinear', align_corners=False)

    def ln(x, g, b, eps):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return g[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]
    C1 = x1.shape[1]
    xc = torch.cat([rs(x1), rs(x2)], 1)      # LN2 reads the x2 columns of the same rows
    xc.retain_grad()
    N, _, H, W = xc.shape
    out1, out2 = ln(xc, g1, b1, eps1), ln(xc[:, C1:], g2, b2, eps2)
    ((out1 * maps(dxn1.to(**t), N, H, W)).sum()
     + (out2 * maps(dxn2.to(**t), N, H, W)).sum()).backward()
    return dict(drc=rows(xc.grad), dg1=g1.grad, db1=b1.grad, dg2=g2.grad, db2=b2.grad,
                dx1=x1.grad, dx2=x2.grad)
