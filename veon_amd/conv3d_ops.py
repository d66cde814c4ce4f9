"""Torch-level wrappers of the Conv3d body kernels (csrc/conv3d.hip).

``PaddedVolume`` owns the zero-padded channels-last bf16 grid
[B][Z+2][Y+2][X+2][C] (plus the guard rows the kernel may read) that the
implicit-GEMM conv consumes and produces.  Everything launches on the current
stream; there is no CPU path.
"""
import ctypes
import math

import torch

from . import _lib
from . import half as _half
from .vocabulary import group_table


class _PaddedGrid:
    """Zero-haloed channels-last half grid [B][S1+2]..[Sn+2][C] of a (B, C, S1..Sn)
    tensor; the number of spatial axes is ``len(shape) - 2`` (fixed by the subclass).
    ``rows`` is the [M, C] view of the padded grid (M = B * prod(Si + 2)); the storage
    has ``veon_conv3d_guard_rows`` zero rows before and after it."""

    _rank = None

    def __init__(self, shape, device, storage=None):
        self.shape = tuple(int(v) for v in shape)
        assert len(self.shape) == 2 + self._rank
        B, C = self.shape[:2]
        self.guard = int(_lib.lib().veon_conv3d_guard_rows(*self.shape[-2:]))
        self.M = B * math.prod(v + 2 for v in self.shape[2:])
        if storage is None:
            storage = torch.zeros((self.M + 2 * self.guard, C),
                                  dtype=_half.dtype(), device=device)
        else:
            assert tuple(storage.shape) == (self.M + 2 * self.guard, C)
            assert storage.is_contiguous() and storage.dtype == _half.dtype()
        self.storage = storage
        self.rows = storage[self.guard:self.guard + self.M]

    @property
    def device(self):
        return self.storage.device

    def like(self, C=None):
        B, C0, *spatial = self.shape
        return type(self)(B, C0 if C is None else C, *spatial, self.device)

    @classmethod
    def from_storage(cls, storage, shape):
        """The grid of ``shape`` on an existing storage tensor (guard rows included),
        e.g. one that autograd saved or handed over."""
        self = cls.__new__(cls)
        _PaddedGrid.__init__(self, shape, None, storage)
        return self

    def interior(self):
        """(B, S1..Sn, C) half view of the un-padded voxels / pixels."""
        B, C, *spatial = self.shape
        inner = (slice(None),) + (slice(1, -1),) * len(spatial)
        return self.rows.view(B, *(v + 2 for v in spatial), C)[inner]


class PaddedVolume(_PaddedGrid):
    """Channels-last bf16 volume with a zero halo.  ``rows`` is the
    [M, C] view of the padded grid (M = B*(Z+2)*(Y+2)*(X+2)); the storage has
    ``veon_conv3d_guard_rows`` zero rows before and after it."""

    _rank = 3

    def __init__(self, B, C, Z, Y, X, device):
        super().__init__((B, C, Z, Y, X), device)

    @staticmethod
    def rows_of(shape):
        """M of the padded grid of a (B, C, Z, Y, X) volume (guard rows not counted)."""
        return int(shape[0]) * math.prod(int(v) + 2 for v in shape[2:])


class PaddedImage(_PaddedGrid):
    """(B,C,Y,X) images as a zero-haloed channels-last bf16 grid
    [B][Y+2][X+2][C] (+ guard rows), the 2-D twin of ``PaddedVolume``."""

    _rank = 2

    def __init__(self, B, C, Y, X, device):
        super().__init__((B, C, Y, X), device)


def pack(x, out=None):
    """(B,C,Z,Y,X) fp32 -> PaddedVolume (bf16, round to nearest even)."""
    dev = _lib.require_device(x)
    x = x.contiguous().float()
    B, C, Z, Y, X = x.shape
    if out is None:
        out = PaddedVolume(B, C, Z, Y, X, dev)
    assert out.shape == tuple(x.shape)
    _lib.launch('veon_volume_pack_bf16', dev, x, out.rows, B, C, Z, Y, X)
    return out


def unpack(vol, out=None):
    """PaddedVolume -> (B,C,Z,Y,X) fp32."""
    dev = _lib.require_device(vol.storage)
    B, C, Z, Y, X = vol.shape
    if out is None:
        out = torch.empty(vol.shape, dtype=torch.float32, device=dev)
    _lib.launch('veon_volume_unpack_f32', dev, vol.rows, out, B, C, Z, Y, X)
    return out


def unpack_cl(vol, channels=None):
    """PaddedVolume -> contiguous fp32 (B, Z, Y, X, C) of its first ``channels`` channels
    (all by default): channels-last, no transpose.  Permuted to (B, C, Z, Y, X) its channel
    stride is 1, which is what ``align_loss.voxel_cosine`` reads without a copy."""
    dev = _lib.require_device(vol.storage)
    _lib.require_half(vol.rows)
    B, Cp, Z, Y, X = vol.shape
    C = Cp if channels is None else int(channels)
    out = torch.empty((B, Z, Y, X, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_volume_unpack_cl_f32', dev, vol.rows, out, B, Cp, C, Z, Y, X)
    return out


def sigm_bwd_pack_cl(grad, f, out=None):
    """Backward of ``f = sigmoid(pre) - 0.5`` fused with the pack: ``grad`` fp32
    (B, C, Z, Y, X) with channel stride 1 (any outer strides), ``f`` the stored half output
    (PaddedVolume) -> d pre = grad * (0.25 - f^2) as a PaddedVolume whose every row is
    stored, halo and guard rows as zeros (``out``: an existing volume to overwrite)."""
    dev = _lib.require_device(grad, f.storage)
    _lib.require_half(f.storage)
    B, C, Z, Y, X = f.shape
    if tuple(grad.shape) != f.shape or grad.dtype != torch.float32 or grad.stride(1) != 1:
        raise _lib.VeonHipError('sigm_bwd_pack_cl takes a channels-last fp32 gradient of %s, '
                                'got %s %s with strides %s' % (f.shape, grad.dtype,
                                                               tuple(grad.shape), grad.stride()))
    if out is None:
        out = PaddedVolume.from_storage(torch.empty_like(f.storage), f.shape)
    assert out.shape == f.shape and out is not f
    st = _lib.host_array([grad.stride(0), grad.stride(2), grad.stride(3), grad.stride(4)])
    _lib.launch('veon_volume_sigm_bwd_pack_cl', dev, grad, st, f.storage, out.storage,
                f.guard, B, C, Z, Y, X)
    return out


def pack_weight(w):
    """nn.Conv3d weight (Cout,Cin,3,3,3) -> bf16 [Cout][3][3][3][Cin]."""
    assert w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3)
    return w.detach().permute(0, 2, 3, 4, 1).contiguous().to(_half.dtype())


def conv3d_k3(vol, w_packed, scale=None, shift=None, resid=None, relu=False,
              out=None, act=None):
    """3x3x3 stride-1 pad-1 convolution on a PaddedVolume with the fused
    epilogue ``act(conv*scale + shift + resid?)`` -> PaddedVolume; ``act`` in
    none / relu / gelu (``relu=True`` is shorthand for act='relu')."""
    dev = _lib.require_device(vol.storage, w_packed)
    B, Cin, Z, Y, X = vol.shape
    Cout = w_packed.shape[0]
    _lib.require_half(w_packed, vol.rows)
    assert w_packed.is_contiguous()
    assert w_packed.numel() == Cout * 27 * Cin
    if out is None:
        out = vol.like(Cout)
    assert out.shape == (B, Cout, Z, Y, X) and out is not vol
    if resid is not None:
        assert resid.shape == out.shape
    _lib.launch('veon_conv3d_k3_bf16', dev, vol.rows, w_packed, scale, shift,
                None if resid is None else resid.rows, out.rows, B, Z, Y, X, Cin, Cout,
                1 if relu else _ACT[act])
    return out


# ------------------------------------------------- training of the Conv3d body
def _pack_weight_dgrad(w):
    """Flip every spatial axis, Cin first, Cout last."""
    spatial = tuple(range(2, w.dim()))
    return w.detach().flip(*spatial).permute(1, *spatial, 0).contiguous()


def pack_weight_dgrad(w):
    """nn.Conv3d weight (Cout,Cin,3,3,3) -> the packed weight [Cin][2-kz][2-ky][2-kx][Cout]
    with which ``conv3d_k3`` of the output gradient is the INPUT gradient of the
    stride-1 pad-1 convolution (taps flipped, channel roles swapped).  Plain torch, any
    device; the dtype follows ``w`` (the caller rounds to the half type)."""
    assert w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3)
    return _pack_weight_dgrad(w)


def _bshape(v, t):
    return v.view(1, -1, *([1] * (t.dim() - 2)))


def bn_train_forward_ref(y, gamma, beta, eps, ident=None, relu=True):
    """Train-mode BatchNorm (+ identity, + ReLU) of ``y`` (B,C,...) in plain torch, the
    mathematics the native passes implement: -> (a, mean, biased var, rstd)."""
    dims = [0] + list(range(2, y.dim()))
    mean = y.mean(dims)
    var = y.var(dims, unbiased=False)
    rstd = (var + eps).rsqrt()
    z = (y - _bshape(mean, y)) * _bshape(rstd * gamma, y) + _bshape(beta, y)
    if ident is not None:
        z = z + ident
    return (z.relu() if relu else z), mean, var, rstd


def bn_train_backward_ref(da, a, y, mean, rstd, gamma, relu=True):
    """The closed-form backward of ``bn_train_forward_ref``: -> (dy, dgamma, dbeta, dz);
    dz is also the gradient of the identity branch."""
    dims = [0] + list(range(2, y.dim()))
    n = y.numel() // y.shape[1]
    dz = da * (a > 0).to(da.dtype) if relu else da
    xhat = (y - _bshape(mean, y)) * _bshape(rstd, y)
    dbeta = dz.sum(dims)
    dgamma = (dz * xhat).sum(dims)
    dy = _bshape(gamma * rstd, y) * (dz - _bshape(dbeta, y) / n - xhat * _bshape(dgamma, y) / n)
    return dy, dgamma, dbeta, dz


def bn_update_running(bn, mean, var, n):
    """What nn.BatchNorm3d does to its buffers in a training step, given the batch
    mean and BIASED variance over ``n`` values per channel."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    with torch.no_grad():
        bn.num_batches_tracked += 1
        f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        # n == 1 never gets here on the native path (nn.BatchNorm3d raises for one
        # value per channel; the body's volumes have thousands)
        unbiased = var * (float(n) / max(n - 1, 1))
        bn.running_mean.mul_(1 - f).add_(mean.to(bn.running_mean.dtype), alpha=f)
        bn.running_var.mul_(1 - f).add_(unbiased.to(bn.running_var.dtype), alpha=f)


def bn_batch_stats(sums, n, eps):
    """fp32 (2, C) sums of ``bn_sums`` -> (mean, biased var, rstd), the C-sized algebra in
    fp64.  The variance is E[y^2] - mean^2 of fp32 SUMS: fp64 here adds no error of its
    own but cannot recover what the sums lost, so var carries about 2^-24 (1 + mean^2 /
    var) relative error times the sums' growth factor: fine for conv outputs (|mean| of the
    order of std), not for a channel with |mean| >> std."""
    s = sums.double()
    mean = s[0] / n
    var = (s[1] / n - mean * mean).clamp_min_(0)
    return mean, var, (var + eps).rsqrt()


def bn_bwd_coefficients(sums, n, gamma, mean, rstd):
    """(dbeta, dgamma) sums + the forward's statistics -> the fp32 vectors (ca, cb, cc)
    of ``bn_bwd_apply``: dy = ca dz + cb y + cc is the closed form
    gamma rstd (dz - dbeta / n - xhat dgamma / n) with xhat = (y - mean) rstd."""
    s = sums.double()
    g, mu, r = gamma.double(), mean.double(), rstd.double()
    ca = g * r
    cb = -g * r * r * s[1] / n
    cc = -g * r * s[0] / n - cb * mu
    return ca.float().contiguous(), cb.float().contiguous(), cc.float().contiguous()


# (kind, key..., device) -> tensor; reused: consumed inside one call.  As with the other
# native caches, one buffer per shape and device serves every stream: two streams that
# train the same shape concurrently must be ordered by the caller.
_WORKSPACES = {}


def _workspace(kind, nbytes, device, *key):
    k = (kind,) + key + (str(device),)
    ws = _WORKSPACES.get(k)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((int(nbytes) + 3) // 4, dtype=torch.float32, device=device)
        _WORKSPACES[k] = ws
    return ws


def wgrad_workspace_bytes(B, Z, Y, X, Cin, Cout):
    """Bytes of split-K slabs ``conv3d_k3_wgrad`` needs (host-only); -1: unsupported."""
    return int(_lib.lib().veon_conv3d_k3_wgrad_workspace_bytes(B, Z, Y, X, Cin, Cout))


def wgrad_supported(Cin, Cout):
    return Cin % 64 == 0 and Cout % 64 == 0


def _conv_k3_wgrad(dy, x, out):
    """The body of ``conv3d_k3_wgrad`` and ``conv2d_k3_wgrad``: the entry point, the tap
    count and the workspace's cache key follow from the rank of the grids."""
    dev = _lib.require_device(dy.storage, x.storage)
    B, Cin, *spatial = x.shape
    Cout = dy.shape[1]
    rank = len(spatial)
    name = 'conv%dd_k3_wgrad' % rank
    kind, workspace_bytes = {3: ('wgrad', wgrad_workspace_bytes),
                             2: ('wgrad2d', wgrad2d_workspace_bytes)}[rank]
    assert dy.shape == (B, Cout, *spatial)
    _lib.require_half(dy.rows, x.rows)
    nbytes = workspace_bytes(B, *spatial, Cin, Cout)
    if nbytes < 0:
        raise _lib.VeonHipError('%s: unsupported shape %s -> %d channels'
                                % (name, x.shape, Cout))
    ws = _workspace(kind, nbytes, dev, B, *spatial, Cin, Cout)
    if out is None:
        out = torch.empty((Cout,) + (3,) * rank + (Cin,), dtype=torch.float32, device=dev)
    assert (out.is_contiguous() and out.dtype == torch.float32
            and out.numel() == Cout * 3 ** rank * Cin)
    _lib.launch('veon_%s_bf16' % name, dev, dy.rows, x.rows, out, ws, nbytes,
                B, *spatial, Cin, Cout)
    return out


def conv3d_k3_wgrad(dy, x, out=None):
    """Weight gradient of the 3x3x3 stride-1 pad-1 convolution on PaddedVolumes:
    ``dy`` (Cout channels, halo zero), ``x`` (Cin) -> fp32 [Cout][3][3][3][Cin] (the
    layout of ``pack_weight``).  Deterministic: split-K slabs added in a fixed order."""
    assert isinstance(dy, PaddedVolume) and isinstance(x, PaddedVolume)
    return _conv_k3_wgrad(dy, x, out)


def wgrad_to_param(dw, w):
    """fp32 [Cout][taps..][Cin] of ``conv3d_k3_wgrad`` / ``conv2d_k3_wgrad`` (or None) ->
    the layout and dtype of the conv parameter ``w`` (Cout, Cin, taps..)."""
    return None if dw is None else dw.movedim(-1, 1).to(w.dtype)


def _bn_workspace(C, dev):
    nbytes = int(_lib.lib().veon_bn3d_sums_workspace_bytes(C))
    if nbytes < 0:
        raise _lib.VeonHipError('train-mode BN: unsupported channel count %d' % C)
    return _workspace('bn', nbytes, dev, C)


def bn_sums(y):
    """Per-channel (sum y, sum y^2) over the rows of a PaddedVolume (halo zero, so the
    interior's sums) -> fp32 (2, C); two-stage, fixed order."""
    dev = _lib.require_device(y.storage)
    B, C, Z, Y, X = y.shape
    sums = torch.empty((2, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_bn3d_sums_bf16', dev, y.rows, sums, _bn_workspace(C, dev),
                B, C, Z, Y, X)
    return sums


def bn_apply(y, scale, shift, ident=None, relu=False, out=None):
    """act(y * scale + shift (+ ident)) -> PaddedVolume, halo rows zero."""
    dev = _lib.require_device(y.storage, scale, shift)
    B, C, Z, Y, X = y.shape
    assert scale.dtype == shift.dtype == torch.float32 and scale.numel() == shift.numel() == C
    if out is None:
        out = y.like()
    assert out.shape == y.shape and out is not y and out is not ident
    assert ident is None or ident.shape == y.shape
    _lib.launch('veon_bn3d_apply_bf16', dev, y.rows, scale.contiguous(), shift.contiguous(),
                None if ident is None else ident.rows, out.rows, 1 if relu else 0,
                B, C, Z, Y, X)
    return out


def bn_bwd_sums(da, a, y, mean, rstd):
    """Per-channel (sum dz, sum dz * xhat), dz = da * [a > 0], xhat = (y - mean) * rstd
    -> fp32 (2, C): (dbeta, dgamma) of train-mode BN followed by ReLU."""
    dev = _lib.require_device(da.storage, a.storage, y.storage, mean, rstd)
    B, C, Z, Y, X = y.shape
    assert da.shape == a.shape == y.shape
    assert mean.dtype == rstd.dtype == torch.float32 and mean.numel() == rstd.numel() == C
    sums = torch.empty((2, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_bn3d_bwd_sums_bf16', dev, da.rows, a.rows, y.rows, mean.contiguous(),
                rstd.contiguous(), sums, _bn_workspace(C, dev), B, C, Z, Y, X)
    return sums


def bn_bwd_apply(da, a, y, ca, cb, cc, want_dz=False):
    """dz = da * [a > 0]; dy = ca * dz + cb * y + cc on interior rows, zero halo ->
    dy, or (dy, dz) with ``want_dz`` (the identity branch's gradient)."""
    dev = _lib.require_device(da.storage, a.storage, y.storage, ca, cb, cc)
    B, C, Z, Y, X = y.shape
    assert da.shape == a.shape == y.shape
    for v in (ca, cb, cc):
        assert v.dtype == torch.float32 and v.numel() == C and v.is_contiguous()
    dy = y.like()
    dz = y.like() if want_dz else None
    _lib.launch('veon_bn3d_bwd_apply_bf16', dev, da.rows, a.rows, y.rows, ca, cb, cc,
                dy.rows, None if dz is None else dz.rows, B, C, Z, Y, X)
    return (dy, dz) if want_dz else dy


def deform_attention(kv, q, off, heads, samples=8, out=None):
    """Sampling + attention core of TemporalDeformable on PaddedVolumes: ``kv``
    (2C channels, per head [key | value]), ``q`` (C), ``off`` (>= heads*samples*3
    raw offsets; tanh is applied here) -> PaddedVolume (C), halo zero."""
    dev = _lib.require_device(kv.storage, q.storage, off.storage)
    B, C, Z, Y, X = q.shape
    assert kv.shape == (B, 2 * C, Z, Y, X) and off.shape[0] == B
    assert tuple(off.shape[2:]) == (Z, Y, X)
    if out is None:
        out = q.like()
    assert out.shape == q.shape and out is not q
    _lib.launch('veon_deform_attention_bf16', dev, kv.rows, q.rows, off.rows, out.rows,
                B, Z, Y, X, C, heads, samples, off.shape[1])
    return out


# ------------------------------------ training of the deformable attention (temporal)
DEFORM_SAMPLES = 8
DEFORM_RANGE_SLOP = 1e-3     # voxels; far above the fp32 error of a position (< 1e-4)


def deform_attention_bwd_ref(kv, q, off, dout, heads):
    """The dense closed form of the backward of ``TemporalDeformable.attend`` in plain
    torch, on any device and in the dtype of its inputs -- the mathematics
    ``deform_attention_bwd`` implements (csrc/temporal_train.hip).  ``kv`` (B,2C,Z,Y,X)
    per head [key | value], ``q`` and ``dout`` (B,C,Z,Y,X), ``off`` (B, >= heads*24,
    Z,Y,X) RAW offsets -> (dkv, dq, doff) of those shapes; doff is the gradient of the
    raw offsets (through tanh), zero in the surplus channels.

    Per voxel, head and sample s (K_s, V_s the trilinear samples, scale = hd^-0.5):
    a = softmax_s(scale q.K_s); da_s = dout.V_s; dl_s = a_s (da_s - sum_t a_t da_t);
    dq = scale sum_s dl_s K_s; g_s = [scale dl_s q | a_s dout] is scattered to the 8
    corner rows with their weights; the position gradient along an axis is
    sum_c (+-1) (product of the other two axes' weights) (row_c . g_s), times
    0.5 (n_dst - 1) / n_src (1 - tanh^2).  ATen's conventions: the position gradient is
    zero on an axis where the coordinate f <= 0 or f >= n - 1 (the clamp, the border
    mode, axes of length one), and at a node ``floor`` gives the right-hand derivative.
    The axis quirk of the forward is kept: offset component 0 and the z index place the
    sample along X (divided by Z), component 2 and the x index along Z (divided by X)."""
    B, C, Z, Y, X = q.shape
    S, hd, N = DEFORM_SAMPLES, C // heads, Z * Y * X
    dt, dev = q.dtype, q.device
    scale = hd ** -0.5
    o = torch.tanh(off[:, :heads * S * 3].reshape(B, heads, S, 3, Z, Y, X))
    base = [torch.linspace(-1, 1, n, dtype=dt, device=dev).view(shape)
            for n, shape in ((Z, (Z, 1, 1)), (Y, (1, Y, 1)), (X, (1, 1, X)))]
    n_src, n_dst = (Z, Y, X), (X, Y, Z)
    i0, i1, t, jac = [], [], [], []
    for a in range(3):
        g = (base[a] + o[:, :, :, a] / n_src[a]).clamp(-1, 1)
        n = n_dst[a]
        f = (g + 1) * 0.5 * (n - 1)
        lo = f.floor().clamp(max=n - 1)
        i0.append(lo.long())
        i1.append((lo.long() + 1).clamp(max=n - 1))
        t.append(f - lo)
        inside = ((f > 0) & (f < n - 1)).to(dt)
        jac.append(inside * (0.5 * (n - 1) / n_src[a]) * (1 - o[:, :, :, a] ** 2))
    kvh = kv.reshape(B, heads, 2 * hd, N)
    qh = q.reshape(B, heads, hd, 1, N)
    do = dout.reshape(B, heads, hd, 1, N)

    def flat(v):                         # (B,heads,S,Z,Y,X) -> (B,heads,1,S,N)
        return v.reshape(B, heads, 1, S, N)
    corners = []
    samp = 0
    for c in range(8):
        xs, wx = (i1[0], t[0]) if c & 1 else (i0[0], 1 - t[0])
        ys, wy = (i1[1], t[1]) if c & 2 else (i0[1], 1 - t[1])
        zs, wz = (i1[2], t[2]) if c & 4 else (i0[2], 1 - t[2])
        idx = ((zs * Y + ys) * X + xs).reshape(B, heads, 1, S * N).expand(-1, -1, 2 * hd, -1)
        rows = kvh.gather(3, idx).reshape(B, heads, 2 * hd, S, N)
        corners.append((idx, rows, flat(wx), flat(wy), flat(wz)))
        samp = samp + flat(wz * wy * wx) * rows
    K, V = samp[:, :, :hd], samp[:, :, hd:]
    a_ = (scale * (qh * K).sum(2)).softmax(dim=2)                  # (B,heads,S,N)
    da = (do * V).sum(2)
    dl = a_ * (da - (a_ * da).sum(2, keepdim=True))
    dq = scale * (dl.unsqueeze(2) * K).sum(3)
    g = torch.cat([scale * dl.unsqueeze(2) * qh, a_.unsqueeze(2) * do], dim=2)
    dkv = torch.zeros_like(kvh)
    dpos = [0, 0, 0]
    for c, (idx, rows, wx, wy, wz) in enumerate(corners):
        dkv.scatter_add_(3, idx, ((wz * wy * wx) * g).reshape(B, heads, 2 * hd, S * N))
        d = (rows * g).sum(2, keepdim=True)
        dpos[0] = dpos[0] + (1 if c & 1 else -1) * wz * wy * d
        dpos[1] = dpos[1] + (1 if c & 2 else -1) * wz * wx * d
        dpos[2] = dpos[2] + (1 if c & 4 else -1) * wy * wx * d
    doff = torch.zeros_like(off)
    doff[:, :heads * S * 3] = torch.stack(
        [dpos[a].reshape(B, heads, S, Z, Y, X) * jac[a] for a in range(3)],
        dim=3).reshape(B, heads * S * 3, Z, Y, X)
    return dkv.reshape(kv.shape), dq.reshape(q.shape), doff


def deform_range_bound(n_src, n_dst):
    """Largest number of source indices ``deform_candidate_ranges`` can list for one
    target index: centres (n_dst-1)/(n_src-1) voxels apart, each reaching
    (n_dst-1)/(2 n_src) to either side, against a window of 1 + slop to either side."""
    if n_src == 1 or n_dst == 1:
        return n_src
    step = (n_dst - 1) / (n_src - 1)
    reach = 1 + DEFORM_RANGE_SLOP + (n_dst - 1) / (2 * n_src)
    return min(n_src, int(math.floor(2 * reach / step)) + 1)


def _deform_axis_ranges(n_src, n_dst):
    i = torch.arange(n_src, dtype=torch.float64)
    c = -1 + 2 * i / (n_src - 1) if n_src > 1 else torch.full((1,), -1.0, dtype=torch.float64)
    flo = ((c - 1.0 / n_src).clamp(-1, 1) + 1) * 0.5 * (n_dst - 1)
    fhi = ((c + 1.0 / n_src).clamp(-1, 1) + 1) * 0.5 * (n_dst - 1)
    tgt = torch.arange(n_dst, dtype=torch.float64).view(-1, 1)
    # a sample at f gives weight to node t iff t - 1 < f < t + 1
    hit = (fhi.view(1, -1) >= tgt - 1 - DEFORM_RANGE_SLOP) & \
        (flo.view(1, -1) <= tgt + 1 + DEFORM_RANGE_SLOP)
    lo = hit.int().argmax(1)
    hi = n_src - 1 - hit.flip(1).int().argmax(1)
    none = ~hit.any(1)
    lo[none], hi[none] = 0, -1
    return torch.stack([lo, hi], dim=1).to(torch.int32)


def deform_candidate_ranges(Z, Y, X):
    """The three (n, 2) int32 tables of inclusive (lo, hi) source indices whose samples
    can touch a target coordinate of the deformable attention (hi < lo: none):
    [0] per target x the source z (the X position is driven by the z index), [1] per
    target y the source y, [2] per target z the source x.  Along an axis source index i
    has centre c_i = -1 + 2i/(n_src-1) and reaches +-1/n_src (|tanh| <= 1), clamped to
    [-1, 1]; its coordinate range [flo_i, fhi_i] is monotone in i, so the indices that
    reach (t-1, t+1) are one contiguous run.  fp64 on the host, widened by
    ``DEFORM_RANGE_SLOP`` voxels; over-inclusion is harmless (the weight comes out 0)."""
    return (_deform_axis_ranges(Z, X), _deform_axis_ranges(Y, Y), _deform_axis_ranges(X, Z))


_DEFORM_TABLES = {}


def _deform_tables(Z, Y, X, dev):
    key = (Z, Y, X, str(dev))
    t = _DEFORM_TABLES.get(key)
    if t is None:
        t = torch.cat([r.reshape(-1) for r in deform_candidate_ranges(Z, Y, X)]).to(dev)
        _DEFORM_TABLES[key] = t
    return t


def deform_attention_bwd(kv, q, off, dout, heads, need_dkv=True, out=None):
    """Backward of ``deform_attention`` on PaddedVolumes -> (dkv, dq, doff), half volumes
    with zero halos; ``doff`` has the channels of ``off`` (gradient of the RAW offsets,
    surplus channels zero).  ``need_dkv`` False: the dKV kernel is not launched and dkv
    is None.  ``out``: (dkv, dq, doff) volumes to write into.  Nothing is accumulated
    with atomics: repeated calls give the same bits."""
    dev = _lib.require_device(kv.storage, q.storage, off.storage, dout.storage)
    B, C, Z, Y, X = q.shape
    assert kv.shape == (B, 2 * C, Z, Y, X) and dout.shape == q.shape
    assert off.shape[0] == B and tuple(off.shape[2:]) == (Z, Y, X)
    _lib.require_half(kv.rows, q.rows, off.rows, dout.rows)
    dkv, dq, doff = out if out is not None else (None, None, None)
    if dq is None:
        dq = q.like()
    if doff is None:
        doff = off.like()
    assert dq.shape == q.shape and doff.shape == off.shape
    assert dq is not q and dq is not dout and doff is not off
    nbytes = int(_lib.lib().veon_deform_attention_bwd_workspace_bytes(B, Z, Y, X, heads))
    if nbytes < 0:
        raise _lib.VeonHipError('deform_attention_bwd: unsupported shape %s' % (q.shape,))
    ws = _workspace('deform', nbytes, dev, B, Z, Y, X, heads)
    _lib.launch('veon_deform_attention_bwd_bf16', dev, kv.rows, q.rows, off.rows, dout.rows,
                dq.rows, doff.rows, ws, nbytes, B, Z, Y, X, C, heads, DEFORM_SAMPLES,
                off.shape[1])
    if not need_dkv:
        return None, dq, doff
    if dkv is None:
        dkv = kv.like()
    assert dkv.shape == kv.shape and dkv is not kv
    _lib.launch('veon_deform_attention_bwd_dkv_bf16', dev, q.rows, off.rows, dout.rows, ws,
                nbytes, _deform_tables(Z, Y, X, dev), dkv.rows, B, Z, Y, X, C, heads,
                DEFORM_SAMPLES, off.shape[1])
    return dkv, dq, doff


class _DeformAttentionFn(torch.autograd.Function):
    """``deform_attention`` under autograd on the STORAGE tensors of PaddedVolumes (as
    ``_ResBlockTrainFn``): saves its three inputs and nothing else."""

    @staticmethod
    def forward(ctx, kvs, qs, offs, heads, shape):
        B, C, Z, Y, X = shape
        vol = PaddedVolume.from_storage
        kv = vol(kvs, (B, 2 * C, Z, Y, X))
        q = vol(qs, shape)
        off = vol(offs, (B, offs.shape[1], Z, Y, X))
        ctx.heads, ctx.shape = heads, tuple(shape)
        ctx.save_for_backward(kvs, qs, offs)
        return deform_attention(kv, q, off, heads).storage

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, douts):
        kvs, qs, offs = ctx.saved_tensors
        B, C, Z, Y, X = ctx.shape
        vol = PaddedVolume.from_storage
        need_kv, need_q, need_off = ctx.needs_input_grad[:3]
        dkv, dq, doff = deform_attention_bwd(
            vol(kvs, (B, 2 * C, Z, Y, X)), vol(qs, ctx.shape),
            vol(offs, (B, offs.shape[1], Z, Y, X)), vol(douts.contiguous(), ctx.shape),
            ctx.heads, need_dkv=need_kv)
        return (dkv.storage if need_kv else None, dq.storage if need_q else None,
                doff.storage if need_off else None, None, None)


def deform_attention_train(kv, q, off, heads, shape):
    """``deform_attention`` under autograd.  ``kv``, ``q``, ``off``: the storage tensors
    of PaddedVolumes (guard rows included) of 2C, C and >= heads*24 channels on the grid
    ``shape`` = (B, C, Z, Y, X) of ``q``; ``off`` holds the RAW offsets.  -> the storage of
    the fused volume (C channels).  The forward is the inference kernel and saves only
    its inputs; the backward (csrc/temporal_train.hip) recomputes the sample positions
    and launches no dKV kernel when ``kv`` needs no gradient."""
    return _DeformAttentionFn.apply(kv, q, off, heads, tuple(int(v) for v in shape))


def warp_volume(vol, affine, out=None):
    """Trilinear resampling of a PaddedVolume at ``affine`` (B,3,4 fp32, voxel
    index units) applied to each output voxel index; zeros outside."""
    dev = _lib.require_device(vol.storage)
    B, C, Z, Y, X = vol.shape
    affine = affine.to(device=dev, dtype=torch.float32).contiguous()
    assert tuple(affine.shape) == (B, 3, 4)
    if out is None:
        out = vol.like()
    assert out.shape == vol.shape and out is not vol
    _lib.launch('veon_volume_warp_bf16', dev, vol.rows, out.rows, affine, B, C, Z, Y, X)
    return out


def warp_affine(cur2glob, prev2glob, first_xyz, step_xyz):
    """(B,1,4,4) or (B,4,4) ROCm fp32 ego->global transforms of the current and a
    past frame -> (B,3,4) voxel-index map for ``warp_volume`` (no host sync)."""
    dev = _lib.require_device(cur2glob, prev2glob)
    mats = []
    for m in (cur2glob, prev2glob):
        m = m.float()
        if m.dim() == 4:
            m = m[:, 0]
        mats.append(m.contiguous())
    B = mats[0].shape[0]
    assert tuple(mats[0].shape) == tuple(mats[1].shape) == (B, 4, 4)
    out = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    first = _lib.host_array([float(v) for v in first_xyz], ctypes.c_double)
    step = _lib.host_array([float(v) for v in step_xyz], ctypes.c_double)
    _lib.launch('veon_warp_affine', dev, mats[0], mats[1], 16, first, step, out, B)
    return out


def zero_halo(vol):
    """Reset the halo rows of a PaddedVolume to zero, in place."""
    dev = _lib.require_device(vol.storage)
    B, C, Z, Y, X = vol.shape
    _lib.launch('veon_volume_zero_halo_bf16', dev, vol.rows, B, C, Z, Y, X)
    return vol


# ----------------------------------------------------------------- 2-D images
def pack_image(x, out=None):
    """(B,C,H,W) fp32 or bf16 -> PaddedImage."""
    dev = _lib.require_device(x)
    if x.dtype not in (torch.float32, _half.dtype()):
        x = x.float()
    B, C, Y, X = x.shape
    if out is None:
        out = PaddedImage(B, C, Y, X, dev)
    assert out.shape == tuple(x.shape)
    if not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last):
        # already channels-last (e.g. a MIOpen NHWC result): one strided copy
        # into the interior, no transpose
        out.rows.view(B, Y + 2, X + 2, C)[:, 1:-1, 1:-1].copy_(x.permute(0, 2, 3, 1))
        return out
    x = x.contiguous()
    _lib.launch('veon_image_pack_bf16', dev, x, 1 if x.dtype == _half.dtype() else 0,
                out.rows, B, C, Y, X)
    return out


def unpack_image(img, dtype=torch.float32, channels=None):
    """PaddedImage -> (B,C,H,W) fp32 or bf16 (first ``channels`` channels)."""
    dev = _lib.require_device(img.storage)
    B, C, Y, X = img.shape
    out = torch.empty(img.shape, dtype=dtype, device=dev)
    _lib.launch('veon_image_unpack', dev, img.rows, out,
                1 if dtype == _half.dtype() else 0, B, C, Y, X)
    return out if channels is None else out[:, :channels]


def pack_weight2d(w, pad_out_to=8):
    """nn.Conv2d weight (Cout,Cin,3,3) -> bf16 [Cout'][3][3][Cin], Cout padded
    with zero filters to a multiple of ``pad_out_to``."""
    assert w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
    cout = w.shape[0]
    npad = (cout + pad_out_to - 1) // pad_out_to * pad_out_to
    wp = torch.zeros((npad,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
    wp[:cout] = w.detach().float()
    return wp.permute(0, 2, 3, 1).contiguous().to(_half.dtype())


_ACT = {None: 0, 'none': 0, 'relu': 1, 'gelu': 2}


def conv2d_k3(img, w_packed, scale=None, shift=None, resid=None, relu=False,
              out=None, act=None, resid2=None, out_relu=None):
    """3x3 stride-1 pad-1 convolution on a PaddedImage with the fused epilogue
    ``act(conv*scale + shift + resid? + resid2?)`` -> PaddedImage; ``act`` in none /
    relu / gelu (``relu=True`` is shorthand for act='relu').  ``out_relu``: a second
    PaddedImage that receives relu(result)."""
    dev = _lib.require_device(img.storage, w_packed)
    B, Cin, Y, X = img.shape
    Cout = w_packed.shape[0]
    _lib.require_half(w_packed)
    assert w_packed.is_contiguous()
    assert w_packed.numel() == Cout * 9 * Cin
    if out is None:
        out = PaddedImage(B, Cout, Y, X, dev)
    assert out.shape == (B, Cout, Y, X) and out is not img
    for extra in (resid, resid2, out_relu):
        assert extra is None or extra.shape == out.shape
    assert out_relu is None or (out_relu is not out and out_relu is not img)

    def rows(p):
        return None if p is None else p.rows
    if resid2 is None and out_relu is None:
        _lib.launch('veon_conv2d_k3_bf16', dev, img.rows, w_packed, scale, shift,
                    rows(resid), out.rows, B, Y, X, Cin, Cout, 1 if relu else _ACT[act])
    else:
        # CALLS counts both forms under 'veon_conv2d_k3_bf16' (what callers and tests read)
        _lib.CALLS['veon_conv2d_k3_bf16'] = _lib.CALLS.get('veon_conv2d_k3_bf16', 0) + 1
        _lib.launch('veon_conv2d_k3_bf16_ex', dev, img.rows, w_packed, scale, shift,
                    rows(resid), rows(resid2), out.rows, rows(out_relu), B, Y, X, Cin, Cout,
                    1 if relu else _ACT[act])
    return out


def conv2d_k3s2(img, w_packed, scale=None, shift=None, out=None, act=None):
    """3x3 stride-2 pad-1 convolution on a PaddedImage -> PaddedImage
    (B, Cout, ceil(Y/2), ceil(X/2)), epilogue as ``conv2d_k3``."""
    dev = _lib.require_device(img.storage, w_packed)
    B, Cin, Y, X = img.shape
    Cout = w_packed.shape[0]
    _lib.require_half(w_packed)
    assert w_packed.is_contiguous()
    assert w_packed.numel() == Cout * 9 * Cin
    Yo, Xo = (Y + 1) // 2, (X + 1) // 2
    if out is None:
        out = PaddedImage(B, Cout, Yo, Xo, dev)
    assert out.shape == (B, Cout, Yo, Xo) and out is not img
    _lib.launch('veon_conv2d_k3s2_bf16', dev, img.rows, w_packed, scale, shift, None,
                out.rows, B, Y, X, Cin, Cout, _ACT[act])
    return out


def image_layernorm(img, gamma, beta, eps, out=None, tokens=False, residual=None):
    """LayerNorm over the channels of every pixel of a PaddedImage.  ``tokens``
    False: -> PaddedImage (zero halo); True: -> fp32 tokens (B, Y*X, C), plus
    ``residual`` (fp32 tokens of that shape) when given."""
    dev = _lib.require_device(img.storage, gamma, beta)
    B, C, Y, X = img.shape
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == C
    if tokens:
        if out is None:
            out = torch.empty((B, Y * X, C), dtype=torch.float32, device=dev)
        assert out.is_contiguous() and tuple(out.shape) == (B, Y * X, C)
        if residual is not None:
            assert (residual.dtype == torch.float32 and residual.is_contiguous()
                    and tuple(residual.shape) == (B, Y * X, C))
        dst = out
    else:
        if out is None:
            out = PaddedImage(B, C, Y, X, dev)
        assert out.shape == img.shape and out is not img and residual is None
        dst = out.rows
    _lib.launch('veon_image_layernorm_bf16', dev, img.rows, gamma, beta, dst,
                1 if tokens else 0, B, C, Y, X, float(eps), residual)
    return out


# --------------------------------------------- training of the HSA ConvBlock (2-D)
def pack_weight2d_dgrad(w):
    """nn.Conv2d weight (Cout,Cin,3,3) -> the packed weight [Cin][2-ky][2-kx][Cout] with
    which ``conv2d_k3`` of the output gradient is the INPUT gradient of the stride-1
    pad-1 convolution (taps flipped, channel roles swapped).  Plain torch, any device;
    the dtype follows ``w`` (the caller rounds to the half type)."""
    assert w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
    return _pack_weight_dgrad(w)


def _cshape(v, t):
    return v.view(*([1] * (t.dim() - 1)), -1)


def ln_forward_ref(x, gamma, beta, eps, gelu=False):
    """LayerNorm over the LAST axis of ``x`` (of GELU(x), erf form, with ``gelu``) in
    plain torch, the mathematics the native passes implement: -> (out, xhat, rstd)."""
    u = torch.nn.functional.gelu(x) if gelu else x
    mean = u.mean(-1, keepdim=True)
    rstd = ((u - mean).square().mean(-1, keepdim=True) + eps).rsqrt()
    xhat = (u - mean) * rstd
    return xhat * _cshape(gamma, x) + _cshape(beta, x), xhat, rstd


def ln_gelu_backward_ref(dout, x, gamma, eps, gelu=False):
    """The closed-form backward of ``ln_forward_ref``: -> (dx, dgamma, dbeta), the sums
    taken over every axis but the last.  With ``gelu``, dx = du * GELU'(x),
    GELU'(x) = Phi(x) + x phi(x)."""
    _, xhat, rstd = ln_forward_ref(x, gamma, torch.zeros_like(gamma), eps, gelu)
    a = dout * _cshape(gamma, x)
    du = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    if gelu:
        cdf = 0.5 * (1 + torch.erf(x * 2.0 ** -0.5))
        pdf = torch.exp(-0.5 * x * x) * (2 * torch.pi) ** -0.5
        du = du * (cdf + x * pdf)
    red = list(range(x.dim() - 1))
    return du, (dout * xhat).sum(red), dout.sum(red)


def wgrad2d_workspace_bytes(B, Y, X, Cin, Cout):
    """Bytes of split-K slabs ``conv2d_k3_wgrad`` needs (host-only); -1: unsupported."""
    return int(_lib.lib().veon_conv2d_k3_wgrad_workspace_bytes(B, Y, X, Cin, Cout))


def conv2d_k3_wgrad(dy, x, out=None):
    """Weight gradient of the 3x3 stride-1 pad-1 convolution on PaddedImages: ``dy``
    (Cout channels, halo zero), ``x`` (Cin) -> fp32 [Cout][3][3][Cin] (the layout of
    ``pack_weight2d``).  Deterministic: split-K slabs added in a fixed order."""
    assert isinstance(dy, PaddedImage) and isinstance(x, PaddedImage)
    return _conv_k3_wgrad(dy, x, out)


def image_gelu_layernorm(img, gamma, beta, eps, out=None):
    """LayerNorm(GELU(img)) over the channels of every pixel -> PaddedImage, zero halo."""
    dev = _lib.require_device(img.storage, gamma, beta)
    B, C, Y, X = img.shape
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == C
    assert gamma.is_contiguous() and beta.is_contiguous()
    if out is None:
        out = PaddedImage(B, C, Y, X, dev)
    assert out.shape == img.shape and out is not img
    _lib.launch('veon_image_gelu_layernorm_bf16', dev, img.rows, gamma, beta, out.rows,
                B, C, Y, X, float(eps))
    return out


def image_layernorm_bwd(dout, x, gamma, eps, gelu_in=False):
    """Backward of ``image_layernorm`` (``gelu_in``: of ``image_gelu_layernorm``) at its
    stored input ``x`` (PaddedImage).  ``dout``: a PaddedImage or fp32 tokens
    (B, Y*X, C).  -> (dx PaddedImage with a zero halo, sums fp32 (3, C)): sums[0] =
    dgamma, sums[1] = dbeta, sums[2] = sum of dx over the pixels (the gradient of the
    bias of the conv that produced ``x``)."""
    B, C, Y, X = x.shape
    tokens = torch.is_tensor(dout)
    if tokens:
        dev = _lib.require_device(dout, x.storage, gamma)
        assert (dout.dtype == torch.float32 and dout.is_contiguous()
                and tuple(dout.shape) == (B, Y * X, C))
        src = dout
    else:
        dev = _lib.require_device(dout.storage, x.storage, gamma)
        assert dout.shape == x.shape and dout is not x
        _lib.require_half(dout.rows)
        src = dout.rows
    _lib.require_half(x.rows)
    assert gamma.dtype == torch.float32 and gamma.numel() == C and gamma.is_contiguous()
    nbytes = int(_lib.lib().veon_image_layernorm_bwd_workspace_bytes(C))
    if nbytes < 0:
        raise _lib.VeonHipError('image_layernorm_bwd: unsupported channel count %d' % C)
    ws = _workspace('lnbwd', nbytes, dev, C)
    dx = PaddedImage(B, C, Y, X, dev)
    sums = torch.empty((3, C), dtype=torch.float32, device=dev)
    _lib.launch('veon_image_layernorm_bwd_bf16', dev, src, 1 if tokens else 0, x.rows,
                1 if gelu_in else 0, gamma, dx.rows, sums, ws, nbytes, B, C, Y, X,
                float(eps))
    return dx, sums


def layernorm_tokens_to_image(x, gamma, beta, eps, out):
    """nn.LayerNorm of fp32 tokens (B, Y*X, C) written as bf16 into the interior of
    the PaddedImage ``out`` (its halo is left as it is: zero)."""
    dev = _lib.require_device(x, gamma, beta, out.storage)
    B, C, Y, X = out.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * Y * X * C
    _lib.launch('veon_layernorm_f32_to_padded', dev, x, gamma, beta, out.rows, B, Y, X, C,
                float(eps))
    return out


def resize_bilinear(img, size, out=None):
    """F.interpolate(mode='bilinear', align_corners=True) on a PaddedImage."""
    dev = _lib.require_device(img.storage)
    B, C, Yi, Xi = img.shape
    Yo, Xo = int(size[0]), int(size[1])
    if out is None:
        out = PaddedImage(B, C, Yo, Xo, dev)
    assert out.shape == (B, C, Yo, Xo)
    _lib.launch('veon_image_resize_bilinear', dev, img.rows, out.rows, B, C, Yi, Xi, Yo, Xo)
    return out


def tokens_to_image(rows, tokens_per_image, skip, h, w, s, C, out):
    """bf16 token rows [B*tokens_per_image, >= s*s*C] (the GEMM output of a
    ConvTranspose2d(k = s, stride = s) applied to the tokens; s = 1: plain tokens)
    -> interior of the PaddedImage ``out`` (B, C, s*h, s*w); the first ``skip`` rows
    of every image (class token) are passed over."""
    dev = _lib.require_device(rows, out.storage)
    B = out.shape[0]
    _lib.require_half(rows)
    assert rows.is_contiguous() and rows.dim() == 2
    assert out.shape == (B, C, s * h, s * w) and rows.shape[0] == B * tokens_per_image
    _lib.launch('veon_tokens_to_image', dev, rows, rows.shape[1], tokens_per_image, skip,
                h, w, s, C, out.rows, B)
    return out


def image_subsample(img, step, out=None):
    """out(y,x) = img(step*y, step*x) -> PaddedImage (B, C, ceil(Y/step), ceil(X/step))."""
    dev = _lib.require_device(img.storage)
    B, C, Y, X = img.shape
    Yo, Xo = (Y + step - 1) // step, (X + step - 1) // step
    if out is None:
        out = PaddedImage(B, C, Yo, Xo, dev)
    assert out.shape == (B, C, Yo, Xo)
    _lib.launch('veon_image_subsample', dev, img.rows, out.rows, B, C, Y, X, step)
    return out


def image_dot(img, w, bias, act='none'):
    """1x1 conv C -> 1 (+activation) of a PaddedImage -> (B,1,H,W) fp32.
    w fp32 [C], act in none / relu / sigmoid."""
    dev = _lib.require_device(img.storage, w)
    B, C, Y, X = img.shape
    assert w.dtype == torch.float32 and w.numel() >= C and w.is_contiguous()
    out = torch.empty((B, 1, Y, X), dtype=torch.float32, device=dev)
    _lib.launch('veon_image_dot', dev, img.rows, w, float(bias), out, B, C, Y, X,
                {'none': 0, 'relu': 1, 'sigmoid': 2}[act])
    return out


def _launch_classify(entry, sem_low, bin_low, occ_size, n_out, table):
    """(n_out channels (B,n_out,Z,Y,X), bin_occ (B,2,Z,Y,X), labels (B,X,Y,Z) int64) from
    ``entry``; ``table``: the arguments between the row count and ``bin_low`` (none, or
    the group table's three)."""
    dev = _lib.require_device(sem_low, bin_low)
    assert sem_low.dtype == bin_low.dtype == torch.float32
    B, K, zi, yi, xi = sem_low.shape
    Zo, Yo, Xo = (int(v) for v in occ_size)
    sem = torch.empty((B, n_out, Zo, Yo, Xo), dtype=torch.float32, device=dev)
    binv = torch.empty((B, 2, Zo, Yo, Xo), dtype=torch.float32, device=dev)
    cls = torch.empty((B, Xo, Yo, Zo), dtype=torch.int64, device=dev)
    _lib.launch(entry, dev, sem_low, _lib.strides(sem_low), K, *table, bin_low,
                _lib.strides(bin_low), B, zi, yi, xi, Zo, Yo, Xo, sem, binv, cls)
    return sem, binv, cls


def occ_classify(sem_low, bin_low, occ_size):
    """Trilinear upsampling (align_corners=False) of the class logits ``sem_low``
    (B,Q,z,y,x) and occupancy logits ``bin_low`` (B,2,z,y,x) -- fp32, ANY strides --
    to ``occ_size``, plus the label volume of VEONTemporal.simple_test, in one kernel.
    -> (sem_occ (B,Q,Z,Y,X), bin_occ (B,2,Z,Y,X), occ_pred_cls (B,X,Y,Z) int64)."""
    B, Q, zi, yi, xi = sem_low.shape
    assert tuple(bin_low.shape) == (B, 2, zi, yi, xi)
    return _launch_classify('veon_occ_classify', sem_low, bin_low, occ_size, Q, ())


def occ_classify_grouped(sem_low, bin_low, occ_size, group, n_merged, free_label):
    """``occ_classify`` against a detailed vocabulary (``occ_eval.occ_labels_grouped``
    states the rule): K logit rows ``sem_low`` (B,K,z,y,x), ``group`` the merged channel of
    each row.  -> (merged logits (B,n_merged,Z,Y,X), bin_occ (B,2,Z,Y,X), occ_pred_cls
    (B,X,Y,Z) int64); the K upsampled rows are never written.  Native on a ROCm device,
    ``occ_eval.occ_grouped_reference`` on the CPU."""
    from . import occ_eval
    B, K, zi, yi, xi = sem_low.shape
    group = group_table(group, n_merged, free_label, K)
    assert tuple(bin_low.shape) == (B, 2, zi, yi, xi)
    if not sem_low.is_cuda:
        return occ_eval.occ_grouped_reference(sem_low, bin_low, occ_size, group, n_merged,
                                              free_label)
    return _launch_classify('veon_occ_classify_grouped', sem_low, bin_low, occ_size,
                            int(n_merged),
                            (occ_eval._group_arg(group), int(n_merged), int(free_label)))
