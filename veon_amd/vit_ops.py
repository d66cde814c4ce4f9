"""Torch-level wrappers of the ViT block kernels (csrc/vit_block.hip).

bf16 tensors are ordinary ``torch.bfloat16`` tensors; the residual stream and
all vectors (bias, LayerNorm / LayerScale parameters) are fp32.  Everything
launches on the current stream; there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from . import half as _half
from .conv3d_ops import _workspace

EPI_BF16, EPI_GELU, EPI_QUICKGELU, EPI_RESID = 0, 1, 2, 3
EPI_AFFINE, EPI_AFFINE_RELU = 4, 5
EPI_AFFINE_SIGM = 6     # sigmoid(gamma * x + bias) - 0.5


def _dev(*ts):
    return _lib.require_device(*ts)


def to_bf16(x):
    """fp32 -> bf16 (round to nearest even) on the device."""
    dev = _dev(x)
    x = x.contiguous().float()
    out = torch.empty(x.shape, dtype=_half.dtype(), device=dev)
    _lib.launch('veon_vit_cast_bf16', dev, x, out, x.numel())
    return out


def patchify(img, patch, skip=0, kpad=None):
    """img fp32 (B,C,H,W) -> bf16 [B*(skip + h*w), kpad]: the conv-weight-ordered
    p x p patches as GEMM rows, ``skip`` zero rows in front of every image."""
    dev = _dev(img)
    img = img.contiguous().float()
    B, C, H, W = img.shape
    k = C * patch * patch
    kpad = kpad or (k + 63) // 64 * 64
    out = torch.empty((B * (skip + (H // patch) * (W // patch)), kpad), dtype=_half.dtype(),
                      device=dev)
    _lib.launch('veon_vit_patchify', dev, img, out, B, C, H, W, patch, skip, kpad)
    return out


def layernorm(x, weight, bias, eps=1e-6, out=None):
    """x fp32 [..., d] -> bf16 [..., d] (nn.LayerNorm over the last dim)."""
    dev = _dev(x, weight, bias)
    d = x.shape[-1]
    T = x.numel() // d
    assert x.dtype == torch.float32 and x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=_half.dtype(), device=dev)
    _lib.launch('veon_vit_layernorm', dev, x, weight, bias, out, T, d, float(eps))
    return out


def layernorm_padded(x, weight, bias, d, eps=1e-6):
    """x fp32 [T, ld] whose first ``d`` columns are the token -> bf16 [T, ld]:
    nn.LayerNorm over those d columns, zeros in the padding."""
    dev = _dev(x, weight, bias)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    T, ld = x.shape
    assert weight.numel() >= d and bias.numel() >= d and d <= ld
    out = torch.empty((T, ld), dtype=_half.dtype(), device=dev)
    _lib.launch('veon_vit_layernorm_padded', dev, x, weight, bias, out, T, int(d), ld,
                float(eps))
    return out


def layernorm_f32(x, weight, bias, eps=1e-5):
    """x fp32 [..., d] -> fp32 [..., d] (nn.LayerNorm over the last dim);
    d % 128 == 0 or d == 64, d <= 1024."""
    dev = _dev(x, weight, bias)
    d = x.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x)
    _lib.launch('veon_layernorm_f32', dev, x, weight, bias, out, x.numel() // d, d,
                float(eps))
    return out


def layernorm_f32_add_nearest(x, add, map_shape, add_shape, weight, bias, eps=1e-5):
    """LayerNorm(x + offset): x fp32 [B, L, d]; ``add`` fp32 [B, h*w, d] is resized
    (nearest, F.interpolate's default) from ``add_shape`` = (h, w) to ``map_shape`` =
    (Y, X) and added to the last Y*X tokens of every sample."""
    dev = _dev(x, add, weight, bias)
    B, L, d = x.shape
    (Y, X), (h, w) = map_shape, add_shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert add.dtype == torch.float32 and add.is_contiguous() and add.shape == (B, h * w, d)
    out = torch.empty_like(x)
    _lib.launch('veon_layernorm_f32_add_nearest', dev, x, add, weight, bias, out,
                B, L, d, Y, X, h, w, float(eps))
    return out


def linear(a, w, bias=None, epilogue=EPI_BF16, out=None, gamma=None):
    """a bf16 [M,K], w bf16 [N,K] (nn.Linear layout) -> bf16 [M,N].  ``gamma``
    (fp32 [N]) is the per-feature scale of the EPI_AFFINE* epilogues."""
    dev = _dev(a, w)
    _lib.require_half(a, w)
    assert a.is_contiguous() and w.is_contiguous()
    K = a.shape[-1]
    M = a.numel() // K
    N = w.shape[0]
    assert w.shape[1] == K
    if out is None:
        out = torch.empty(a.shape[:-1] + (N,), dtype=_half.dtype(), device=dev)
    _lib.launch('veon_vit_gemm', dev, a, w, bias, gamma, None, out, M, N, K, epilogue)
    return out


def linear_residual_(resid, a, w, bias=None, gamma=None):
    """resid fp32 [M,N] += gamma * (a @ w^T + bias), in place."""
    dev = _dev(resid, a, w)
    assert resid.dtype == torch.float32 and resid.is_contiguous()
    K = a.shape[-1]
    M = a.numel() // K
    N = w.shape[0]
    assert resid.numel() == M * N
    _lib.launch('veon_vit_gemm', dev, a, w, bias, gamma, resid, None, M, N, K, EPI_RESID)
    return resid


# ------------------------------------------------- training passes (csrc/linear_train.hip)
def _rows(t):
    """(M, width) of a contiguous half tensor read as rows of its last axis."""
    _lib.require_half(t)
    assert t.is_contiguous()
    return t.numel() // t.shape[-1], t.shape[-1]


def linear_wgrad_workspace_bytes(M, K, N):
    """Bytes of split-K slabs ``linear_wgrad`` needs (host-only); -1: unsupported."""
    return int(_lib.lib().veon_linear_wgrad_workspace_bytes(M, K, N))


def linear_wgrad(dy, x, out=None):
    """Weight gradient of ``y = x W^T``: dy half [M, N], x half [M, K] -> fp32 [N, K] (the
    nn.Linear layout) = dy^T x, the contraction over the M rows in fp32.  K and N
    multiples of 64.  Deterministic: split-K slabs added in a fixed order.  In the fp16
    flavour the operands are fp16 gradients as they are: loss scaling is the caller's."""
    dev = _dev(dy, x)
    (M, N), (Mx, K) = _rows(dy), _rows(x)
    assert M == Mx
    nbytes = linear_wgrad_workspace_bytes(M, K, N)
    if nbytes < 0:
        raise _lib.VeonHipError('linear_wgrad: unsupported shape %d rows, %d -> %d' % (M, K, N))
    ws = _workspace('linear_wgrad', nbytes, dev, M, K, N)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=dev)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == (N, K)
    _lib.launch('veon_linear_wgrad_bf16', dev, dy, x, out, ws, nbytes, M, K, N)
    return out


def linear_wgrad_ref(dy, x):
    """``linear_wgrad`` in torch, in the operands' own dtype (pass fp64 for a reference)."""
    return dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])


def colsum(dy):
    """dy half [M, N] -> fp32 [N], the sum over the rows (a bias gradient).  Two stages
    in a fixed order: deterministic."""
    dev = _dev(dy)
    M, N = _rows(dy)
    nbytes = int(_lib.lib().veon_rows_colsum_workspace_bytes(N))
    if nbytes < 0:
        raise _lib.VeonHipError('colsum: unsupported width %d' % N)
    ws = _workspace('colsum', nbytes, dev, N)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.launch('veon_rows_colsum_bf16', dev, dy, out, ws, nbytes, M, N)
    return out


def gelu(y):
    """GELU (erf form) of a half tensor, in fp32 from the stored half value -> half."""
    dev = _dev(y)
    _rows(y)
    out = torch.empty_like(y)
    _lib.launch('veon_gelu_bf16', dev, y, out, y.numel())
    return out


def gelu_bwd(dh, y):
    """dh * GELU'(y), GELU'(y) = Phi(y) + y phi(y), on half tensors -> half."""
    dev = _dev(dh, y)
    _rows(y)
    _rows(dh)
    assert dh.shape == y.shape
    out = torch.empty_like(y)
    _lib.launch('veon_gelu_bwd_bf16', dev, dh, y, out, y.numel())
    return out


def quickgelu(y):
    """CLIP's QuickGELU y * sigmoid(1.702 y) of a half tensor, in fp32 from the stored half
    value -> half."""
    dev = _dev(y)
    _rows(y)
    out = torch.empty_like(y)
    _lib.launch('veon_quickgelu_bf16', dev, y, out, y.numel())
    return out


def quickgelu_bwd(dh, y):
    """dh * (s + 1.702 y s (1 - s)), s = sigmoid(1.702 y), on half tensors -> half."""
    dev = _dev(dh, y)
    _rows(y)
    _rows(dh)
    assert dh.shape == y.shape
    out = torch.empty_like(y)
    _lib.launch('veon_quickgelu_bwd_bf16', dev, dh, y, out, y.numel())
    return out


def quickgelu_bwd_ref(dh, y):
    """``quickgelu_bwd`` in torch, in the operands' own dtype (pass fp64 for a reference)."""
    s = torch.sigmoid(1.702 * y)
    return dh * (s + 1.702 * y * s * (1 - s))


def layernorm_f32_bwd(dout, x, gamma, eps):
    """Backward of nn.LayerNorm over the last axis at its stored fp32 input ``x``
    [..., d]; ``dout`` fp32 or half, same shape.  -> (dx fp32, dgamma, dbeta fp32 [d]).
    d % 64 == 0, d <= 1024."""
    dev = _dev(dout, x, gamma)
    d = x.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert dout.shape == x.shape and dout.is_contiguous()
    if dout.dtype != torch.float32:
        _lib.require_half(dout)
    assert gamma.dtype == torch.float32 and gamma.numel() == d and gamma.is_contiguous()
    nbytes = int(_lib.lib().veon_layernorm_f32_bwd_workspace_bytes(d))
    if nbytes < 0:
        raise _lib.VeonHipError('layernorm_f32_bwd: unsupported width %d' % d)
    ws = _workspace('lnf32bwd', nbytes, dev, d)
    dx = torch.empty_like(x)
    sums = torch.empty((2, d), dtype=torch.float32, device=dev)
    _lib.launch('veon_layernorm_f32_bwd', dev, dout, 0 if dout.dtype == torch.float32 else 1,
                x, gamma, dx, sums, ws, nbytes, x.numel() // d, d, float(eps))
    return dx, sums[0], sums[1]


LOG2E = 1.4426950408889634   # folded into q by the packers that set ``q_log2``


def attention(qkv, num_heads, bias=None, out=None, q_log2=False):
    """qkv bf16 [B,T,3*H*64] (q pre-scaled by head_dim^-0.5; ``q_log2``: also by
    ``LOG2E``, the exp2-domain form of the kernel) -> bf16 [B,T,H*64].
    bias: optional fp32 additive logits, broadcastable [B|1, H|1, T, T]."""
    dev = _dev(qkv)
    B, T, three_d = qkv.shape
    H = num_heads
    hd = three_d // (3 * H)
    _lib.require_half(qkv)
    assert qkv.is_contiguous()
    if out is None:
        out = torch.empty((B, T, H * hd), dtype=_half.dtype(), device=dev)
    sb = sh = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.dim() == 4
        assert bias.shape[-2:] == (T, T) and bias.stride(-1) == 1 \
            and bias.stride(-2) == T
        sb = bias.stride(0) if bias.shape[0] > 1 else 0
        sh = bias.stride(1) if bias.shape[1] > 1 else 0
    if q_log2:
        # CALLS counts both forms under 'veon_vit_attention' (what callers and tests read)
        _lib.CALLS['veon_vit_attention'] = _lib.CALLS.get('veon_vit_attention', 0) + 1
    _lib.launch('veon_vit_attention_log2' if q_log2 else 'veon_vit_attention', dev,
                qkv, bias, sb, sh, out, B, T, H, hd)
    return out


# ------------------- query cross-attention with a self key (csrc/query_attention.hip)
def _query_dims(q_qkv, mem_kv, num_heads):
    """(B, Q, T, hd) of the operands of ``query_attention``: q_qkv [B, Q, 3*H*hd] or
    [B, Q, 3, H, hd]; mem_kv [B, T, 2*H*hd] or [B, T, 2, H, hd]."""
    H = num_heads
    B, Q = q_qkv.shape[:2]
    hd = q_qkv[0, 0].numel() // (3 * H)
    T = mem_kv.shape[1]
    assert q_qkv.dim() in (3, 5) and q_qkv[0, 0].numel() == 3 * H * hd
    assert mem_kv.dim() in (3, 5) and mem_kv.shape[0] == B
    assert mem_kv[0, 0].numel() == 2 * H * hd
    return B, Q, T, hd


def query_attention(q_qkv, mem_kv, num_heads, bias=None, key0=0, q_log2=False, out=None):
    """The attention core of ``cross_attn_with_self_bias`` (models/semantic_net/
    clip_blocks.py) as one launch of ``veon_query_attention``
    (include/ext/veon_hip_query.h): q_qkv half [B, Q, 3, H, 64], the packed projection of
    the query tokens (q pre-scaled by 64^-0.5; ``q_log2``: also by ``LOG2E``); mem_kv half
    [B, T, 2, H, 64], the k / v projection of the memory tokens -- it may be a VIEW with any
    token stride (the K/V part ``qkv.view(B, T, 3, H, 64)[:, :, 1:]`` of a packed buffer);
    the keys are tokens ``key0 .. T-1``.  bias: optional fp32 additive logits
    (B | 1, H | 1, Q, T - key0), natural-log units, -inf removes a key.  Every query also
    attends to itself through its own k / v rows.  -> half [B, Q, H*64]."""
    dev = _dev(q_qkv, mem_kv, bias, out)
    _lib.require_half(q_qkv, mem_kv, out)
    H = num_heads
    B, Q, T, hd = _query_dims(q_qkv, mem_kv, H)
    if hd != 64:
        raise _lib.VeonHipError('query_attention: head_dim %d, the kernel takes 64' % hd)
    assert q_qkv.is_contiguous()
    tok = mem_kv.stride(1) if T > 1 else 2 * H * hd
    inner = (H * hd, hd, 1) if mem_kv.dim() == 5 else (1,)
    assert tuple(mem_kv.stride()[2:]) == inner, 'mem_kv: the rows of a token must be dense'
    assert B == 1 or mem_kv.stride(0) == T * tok, 'mem_kv: images must follow each other'
    Lk = T - key0
    sb = sh = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.dim() == 4
        assert bias.shape[0] in (1, B) and bias.shape[1] in (1, H)
        assert bias.shape[-2:] == (Q, Lk)
        if Lk and (bias.stride(-1) != 1 or (Q > 1 and bias.stride(-2) != Lk)):
            bias = bias.contiguous()
        sb = bias.stride(0) if bias.shape[0] > 1 else 0
        sh = bias.stride(1) if bias.shape[1] > 1 else 0
    if out is None:
        out = torch.empty((B, Q, H * hd), dtype=_half.dtype(), device=dev)
    assert out.is_contiguous() and out.shape == (B, Q, H * hd)
    _lib.launch('veon_query_attention', dev, q_qkv, mem_kv, int(tok), bias, int(sb), int(sh),
                out, B, Q, T, int(key0), H, int(bool(q_log2)))
    return out


def query_attention_ref(q_qkv, mem_kv, num_heads, bias=None, key0=0, q_log2=False,
                        dtype=torch.float64):
    """``query_attention`` in torch on the operands as given, q k v in ``dtype`` (fp64 for
    a reference; any head_dim): logits s_j = q.k_j + bias_j over the memory keys
    ``key0 .. T-1`` and s_self = q.k_q, one softmax over the Lk + 1 of them,
    out = sum_j p_j v_j + p_self v_q.  The scores are promoted to the bias's precision
    before it is added; ``q_log2``: q carries log2(e), which is taken out of the scores."""
    H = num_heads
    B, Q, T, hd = _query_dims(q_qkv, mem_kv, H)
    x = q_qkv.reshape(B, Q, 3, H, hd).to(dtype)
    mem = mem_kv.reshape(B, T, 2, H, hd)[:, key0:].to(dtype)
    q, kq, vq = x.permute(2, 0, 3, 1, 4)               # (B, H, Q, hd)
    k, v = mem.permute(2, 0, 3, 1, 4)                  # (B, H, Lk, hd)
    s = torch.cat([q @ k.transpose(-2, -1), (q * kq).sum(-1, keepdim=True)], dim=-1)
    if q_log2:
        s = s / LOG2E
    if bias is not None:
        s = s.to(torch.promote_types(s.dtype, bias.dtype))
        s = torch.cat([s[..., :-1] + bias, s[..., -1:]], dim=-1)
    p = s.softmax(dim=-1).to(dtype)
    o = p[..., :-1] @ v + p[..., -1:] * vq
    return o.transpose(1, 2).reshape(B, Q, H * hd)


# ------------------------------------------- attention for training (csrc/attention_train.hip)
def attention_stats_len(T):
    """Floats per (b, h) row of ``lse`` and of the backward's workspace: T rounded up to 64."""
    return int(_lib.lib().veon_vit_attention_stats_len(int(T)))


def _qkv_dims(qkv, num_heads):
    _lib.require_half(qkv)
    assert qkv.dim() == 3 and qkv.is_contiguous()
    B, T, three_d = qkv.shape
    hd = three_d // (3 * num_heads)
    assert three_d == 3 * num_heads * hd
    return B, T, hd


def attention_fwd_lse(qkv, num_heads, scale, out=None, lse=None):
    """qkv half [B,T,3*H*64], the RAW output of the qkv Linear (q not pre-scaled) ->
    (out half [B,T,H*64] = softmax(scale q k^T) v, lse fp32 [B,H,Tp]): the log-sum-exp of
    the scaled scores in log2 units, rows padded to ``attention_stats_len(T)``; columns
    T.. of lse are not written."""
    dev = _dev(qkv)
    B, T, hd = _qkv_dims(qkv, num_heads)
    if out is None:
        out = torch.empty((B, T, num_heads * hd), dtype=_half.dtype(), device=dev)
    if lse is None:
        lse = torch.empty((B, num_heads, attention_stats_len(T)), dtype=torch.float32,
                          device=dev)
    assert lse.is_contiguous() and lse.dtype == torch.float32
    _lib.launch('veon_vit_attention_fwd_lse', dev, qkv, out, lse, B, T, num_heads, hd,
                float(scale))
    return out, lse


def attention_bwd(qkv, out, dout, lse, num_heads, scale, dqkv=None, workspace=None):
    """Backward of ``attention_fwd_lse``: dout half [B,T,H*64] and the saved qkv, out, lse
    -> dqkv half [B,T,3*H*64], every element written.  ``workspace``: fp32 [B,H,Tp] for
    delta = rowsum(dout * out) (allocated when None).  No atomics: deterministic.  In the
    fp16 flavour the gradients are fp16 as they are: loss scaling is the caller's."""
    dev = _dev(qkv, out, dout, lse)
    B, T, hd = _qkv_dims(qkv, num_heads)
    _lib.require_half(out, dout)
    assert out.is_contiguous() and dout.is_contiguous() and out.shape == dout.shape
    assert out.shape == (B, T, num_heads * hd)
    Tp = attention_stats_len(T)
    assert lse.is_contiguous() and lse.dtype == torch.float32
    assert lse.shape == (B, num_heads, Tp)
    nbytes = int(_lib.lib().veon_vit_attention_bwd_workspace_bytes(B, T, num_heads))
    if nbytes < 0:
        raise _lib.VeonHipError('attention_bwd: unsupported shape')
    if workspace is None:
        workspace = torch.empty((B, num_heads, Tp), dtype=torch.float32, device=dev)
    assert workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= nbytes
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    assert dqkv.is_contiguous() and dqkv.shape == qkv.shape and dqkv.dtype == qkv.dtype
    _lib.launch('veon_vit_attention_bwd', dev, qkv, out, dout, lse, dqkv, workspace,
                workspace.numel() * workspace.element_size(), B, T, num_heads, hd,
                float(scale))
    return dqkv


def attention_ref(qkv, num_heads, scale):
    """softmax(scale q k^T) v in torch, in the operand's own dtype: qkv [B,T,3*H*hd] ->
    [B,T,H*hd] (the arithmetic of the DINOv2 ``Attention`` module)."""
    B, T, three_d = qkv.shape
    q, k, v = qkv.reshape(B, T, 3, num_heads, -1).permute(2, 0, 3, 1, 4)
    attn = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, T, three_d // 3)


def attention_bwd_ref(qkv, dout, num_heads, scale):
    """``attention_bwd`` in torch, in the operands' own dtype (pass fp64 for a reference):
    the closed form dV = P^T dO, dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q
    with the T x T matrices formed explicitly."""
    B, T, three_d = qkv.shape
    q, k, v = qkv.reshape(B, T, 3, num_heads, -1).permute(2, 0, 3, 1, 4)
    do = dout.reshape(B, T, num_heads, -1).permute(0, 2, 1, 3)
    p = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    o = p @ v
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-2, -1) @ q) * scale
    return torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(B, T, three_d)


class _AttentionTrainFn(torch.autograd.Function):
    """Saves qkv, out and lse (B*H*Tp floats): never a T x T tensor."""

    @staticmethod
    def forward(ctx, qkv, num_heads, scale):
        out, lse = attention_fwd_lse(qkv.contiguous(), num_heads, scale)
        ctx.num_heads, ctx.scale = num_heads, scale
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return attention_bwd(qkv.contiguous(), out, dout.contiguous(), lse, ctx.num_heads,
                             ctx.scale), None, None


def attention_train(qkv, num_heads, scale):
    """``attention_fwd_lse``'s out under autograd, backward on ``attention_bwd``."""
    return _AttentionTrainFn.apply(qkv, num_heads, scale)


# --------------------------- attention with a dense additive bias, for training (the CLIP tail)
def _bias_view(bias, B, H, Tb):
    """A bias (B, H, Tb, Tb) with unit-size batch / head axes allowed, (B*H, Tb, Tb) or
    (Tb, Tb) as a 4-D VIEW whose last two axes are dense rows of Tb floats -> (view,
    bias_sb, bias_sh), a zero stride for a broadcast axis.  No copy unless the rows are
    not dense."""
    assert bias.dtype == torch.float32 and bias.shape[-2:] == (Tb, Tb)
    if bias.dim() == 2:
        v = bias.view(1, 1, Tb, Tb)
    elif bias.dim() == 3:
        assert bias.shape[0] == B * H
        if Tb and (bias.stride(-1) != 1 or bias.stride(-2) != Tb):
            bias = bias.contiguous()
        v = bias.reshape(B, H, Tb, Tb)
    else:
        assert bias.dim() == 4 and bias.shape[0] in (1, B) and bias.shape[1] in (1, H)
        v = bias
    if Tb and (v.stride(-1) != 1 or v.stride(-2) != Tb):
        v = v.contiguous()
    sb = v.stride(0) if v.shape[0] > 1 else 0
    sh = v.stride(1) if v.shape[1] > 1 else 0
    return v, sb, sh


def attention_bias_fwd_lse(qkv, bias, num_heads, scale, border=0, out=None, lse=None):
    """``attention_fwd_lse`` with an fp32 additive bias (natural-log units, added to
    scale q.k): (B, H, Tb, Tb) with unit-size axes broadcast, (B*H, Tb, Tb) or (Tb, Tb),
    Tb = T - border.  ``border`` = 1: the bias is patch-to-patch and token 0 has bias 0 as a
    query and as a key, by index.  A query whose keys are all masked (-inf) gets an out row
    of zeros and lse = +inf."""
    dev = _dev(qkv, bias)
    B, T, hd = _qkv_dims(qkv, num_heads)
    assert border in (0, 1)
    bv, sb, sh = _bias_view(bias, B, num_heads, T - border)
    if out is None:
        out = torch.empty((B, T, num_heads * hd), dtype=_half.dtype(), device=dev)
    if lse is None:
        lse = torch.empty((B, num_heads, attention_stats_len(T)), dtype=torch.float32,
                          device=dev)
    assert lse.is_contiguous() and lse.dtype == torch.float32
    _lib.launch('veon_vit_attention_bias_fwd_lse', dev, qkv, bv, sb, sh, int(border), out, lse,
                B, T, num_heads, hd, float(scale))
    return out, lse


def attention_bias_bwd(qkv, bias, out, dout, lse, num_heads, scale, border=0, dqkv=True,
                       dbias=True, workspace=None):
    """Backward of ``attention_bias_fwd_lse`` -> (dqkv half like qkv, dbias fp32
    (B, H, Tb, Tb)): dbias is ALWAYS dense (the caller sums over broadcast axes) and is the
    gradient with respect to the bias, dS.  ``dqkv`` / ``dbias``: True allocates, a tensor
    is written into, None skips that gradient (its result is None); without dqkv only the
    delta pass (here sum_k p dp, a sweep over the keys; ``out`` is not read) and the dS pass
    run, counted under ``'veon_vit_attention_bias_bwd:ds_only'``
    in ``_lib.CALLS``.  Every element of both is written; no atomics: deterministic."""
    dev = _dev(qkv, bias, out, dout, lse)
    B, T, hd = _qkv_dims(qkv, num_heads)
    H, Tb = num_heads, T - border
    assert border in (0, 1) and (dqkv is not None or dbias is not None)
    _lib.require_half(out, dout)
    assert out.is_contiguous() and dout.is_contiguous() and out.shape == dout.shape
    assert out.shape == (B, T, H * hd)
    Tp = attention_stats_len(T)
    assert lse.is_contiguous() and lse.dtype == torch.float32 and lse.shape == (B, H, Tp)
    bv, sb, sh = _bias_view(bias, B, H, Tb)
    nbytes = int(_lib.lib().veon_vit_attention_bwd_workspace_bytes(B, T, H))
    if nbytes < 0:
        raise _lib.VeonHipError('attention_bias_bwd: unsupported shape')
    if workspace is None:
        workspace = torch.empty((B, H, Tp), dtype=torch.float32, device=dev)
    assert workspace.is_contiguous() and workspace.numel() * workspace.element_size() >= nbytes
    if dqkv is True:
        dqkv = torch.empty_like(qkv)
    if dbias is True:
        dbias = torch.empty((B, H, Tb, Tb), dtype=torch.float32, device=dev)
    if dqkv is not None:
        assert dqkv.is_contiguous() and dqkv.shape == qkv.shape and dqkv.dtype == qkv.dtype
    if dbias is not None:
        assert dbias.is_contiguous() and dbias.shape == (B, H, Tb, Tb)
        assert dbias.dtype == torch.float32
    if dqkv is None:
        if Tb == 0:          # an empty matrix: nothing to compute
            return None, dbias
        _lib.CALLS['veon_vit_attention_bias_bwd:ds_only'] = \
            _lib.CALLS.get('veon_vit_attention_bias_bwd:ds_only', 0) + 1
    _lib.launch('veon_vit_attention_bias_bwd', dev, qkv, bv, sb, sh, int(border), out, dout,
                lse, dqkv, dbias if Tb else None, workspace,
                workspace.numel() * workspace.element_size(), B, T, H, hd, float(scale))
    return dqkv, dbias


def _full_bias(bias, B, H, T, border):
    """The bias of any accepted shape as (B, H, T, T); the border by zero padding."""
    Tb = T - border
    if bias.dim() == 3:
        bias = bias.reshape(B, H, Tb, Tb)
    elif bias.dim() == 2:
        bias = bias.reshape(1, 1, Tb, Tb)
    if border:
        bias = torch.nn.functional.pad(bias, (1, 0, 1, 0))
    return bias.expand(B, H, T, T)


def _masked_softmax(s):
    """softmax over the last axis; a row of -inf alone gives zeros (torch gives NaN)."""
    dead = (s == float('-inf')).all(-1, keepdim=True)
    return torch.where(dead, torch.zeros_like(s), s.masked_fill(dead, 0).softmax(dim=-1))


def attention_bias_ref(qkv, bias, num_heads, scale, border=0, dtype=None):
    """softmax(scale q k^T + bias) v in torch, q k v in ``dtype`` (default: qkv's own; pass
    fp64 for a reference): the scores are converted to the bias's precision (fp32, or fp64
    with a double bias) before the bias is added, which is what the kernel does.  A row
    whose keys are all masked is zero, as in the kernel."""
    B, T, three_d = qkv.shape
    x = qkv if dtype is None else qkv.to(dtype)
    q, k, v = x.reshape(B, T, 3, num_heads, -1).permute(2, 0, 3, 1, 4)
    full = _full_bias(bias, B, num_heads, T, border)
    s = ((q * scale) @ k.transpose(-2, -1)).to(full.dtype) + full
    attn = _masked_softmax(s).to(x.dtype)
    return (attn @ v).transpose(1, 2).reshape(B, T, three_d // 3)


def attention_bias_bwd_ref(qkv, bias, dout, num_heads, scale, border=0, dtype=None):
    """``attention_bias_bwd`` in torch -> (dqkv [B,T,3*H*hd], dbias dense (B, H, Tb, Tb)):
    the closed form of ``attention_bwd_ref`` with P = softmax(scale q k^T + bias) and
    dbias = dS.  A query whose keys are all masked has P = 0 by definition: its rows of
    dq, dbias are zero and it adds nothing to dk, dv."""
    B, T, three_d = qkv.shape
    x = qkv if dtype is None else qkv.to(dtype)
    q, k, v = x.reshape(B, T, 3, num_heads, -1).permute(2, 0, 3, 1, 4)
    do = dout.to(x.dtype).reshape(B, T, num_heads, -1).permute(0, 2, 1, 3)
    full = _full_bias(bias, B, num_heads, T, border)
    s = ((q * scale) @ k.transpose(-2, -1)).to(full.dtype) + full
    p = _masked_softmax(s).to(x.dtype)
    o = p @ v
    dv = p.transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-2, -1) @ q) * scale
    dqkv = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(B, T, three_d)
    return dqkv, ds[:, :, border:, border:]


class _AttentionBiasTrainFn(torch.autograd.Function):
    """Saves qkv, out, lse and the bias it was handed: no other T x T tensor."""

    @staticmethod
    def forward(ctx, qkv, bias, num_heads, scale, border):
        qkv = qkv.contiguous()
        out, lse = attention_bias_fwd_lse(qkv, bias.detach(), num_heads, scale, border)
        ctx.num_heads, ctx.scale, ctx.border = num_heads, scale, border
        ctx.save_for_backward(qkv, bias, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qkv, bias, out, lse = ctx.saved_tensors
        need_qkv, need_bias = ctx.needs_input_grad[:2]
        if not (need_qkv or need_bias):
            return None, None, None, None, None
        dqkv, dbias = attention_bias_bwd(
            qkv, bias.detach(), out, dout.contiguous(), lse, ctx.num_heads, ctx.scale,
            ctx.border, dqkv=True if need_qkv else None, dbias=True if need_bias else None)
        if dbias is not None:
            B, H = dbias.shape[:2]
            if bias.dim() == 2:
                dbias = dbias.sum((0, 1))
            elif bias.dim() == 3:
                dbias = dbias.view(bias.shape)
            else:
                axes = [a for a in (0, 1) if bias.shape[a] == 1 and dbias.shape[a] > 1]
                if axes:
                    dbias = dbias.sum(axes, keepdim=True)
        return dqkv, dbias, None, None, None


def attention_bias_train(qkv, bias, num_heads, scale, border=0):
    """``attention_bias_fwd_lse``'s out under autograd, backward on ``attention_bias_bwd``:
    a gradient for ``qkv`` and / or ``bias`` as ``needs_input_grad`` asks, the bias's in the
    shape it was given (summed over broadcast axes).  When qkv needs none, the dq / dk / dv
    work is not launched."""
    return _AttentionBiasTrainFn.apply(qkv, bias, num_heads, scale, border)


class BlockWeights:
    """Device weights of one transformer block packed for ``veon_vit_block``
    (include/veon_hip.h): keeps the tensors alive and the C struct ready."""

    def __init__(self, heads, n1, w_qkv, b_qkv, w_proj, b_proj, g1, n2, w_fc1,
                 b_fc1, w_fc2, b_fc2, g2, act, q_log2=False):
        self.heads = heads
        self.q_log2 = bool(q_log2)
        self.keep = (n1[0], n1[1], w_qkv, b_qkv, w_proj, b_proj, g1, n2[0], n2[1],
                     w_fc1, b_fc1, w_fc2, b_fc2, g2)
        for t in self.keep:
            assert t is None or (t.is_cuda and t.is_contiguous())
        self.d = w_qkv.shape[1]
        self.mlp_dim = w_fc1.shape[0]
        p = _lib.ptr
        self.c = _lib.VitBlockWeights(
            p(n1[0]).value, p(n1[1]).value, p(w_qkv).value, p(b_qkv).value,
            p(w_proj).value, p(b_proj).value, p(g1).value, p(n2[0]).value,
            p(n2[1]).value, p(w_fc1).value, p(b_fc1).value, p(w_fc2).value,
            p(b_fc2).value, p(g2).value, float(n1[2]), float(n2[2]),
            int(self.mlp_dim), int(act), int(self.q_log2))


def block_workspace(B, T, d, mlp_dim, device):
    """Workspace of ``veon_vit_block``.  It ends in the sync words of the split-K fc2
    (4 KiB), which every call expects zero and leaves zero: only those are cleared."""
    n = _lib.lib().veon_vit_block_workspace_bytes(B, T, d, mlp_dim)
    ws = torch.empty(n, dtype=torch.uint8, device=device)
    ws[n - 4096:].zero_()
    return ws


def linear_residual_splitk_(resid, a, w, bias=None, gamma=None, workspace=None):
    """``linear_residual_`` by the split-K kernel (fc2 shapes); raises when the shape is
    not one ``veon_vit_gemm_splitk_plan`` splits.  ``workspace``: (slab uint8 tensor,
    zeroed int32 sync tensor) to reuse; allocated when None."""
    dev = _dev(resid, a, w)
    K = a.shape[-1]
    M = a.numel() // K
    N = w.shape[0]
    need = _lib.lib().veon_vit_gemm_splitk_plan(M, N, K, None)
    if need == 0:
        raise _lib.VeonHipError('no split-K plan for %d x %d x %d' % (M, N, K))
    if workspace is None:
        workspace = (torch.empty(need, dtype=torch.uint8, device=dev),
                     torch.zeros(1024, dtype=torch.int32, device=dev))
    slab, sync = workspace
    _lib.launch('veon_vit_gemm_splitk', dev, a, w, bias, gamma, resid, M, N, K,
                slab, slab.numel(), sync, sync.numel())
    return resid


def block_forward_(x, w, B, T, ws, bias=None):
    """One pre-norm block on the fp32 residual stream x [B*T, d], in place, as a
    single native call (seven launches)."""
    dev = _dev(x, ws)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B * T, w.d)
    sb = sh = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.dim() == 4
        assert bias.shape[-2:] == (T, T) and bias.stride(-1) == 1 \
            and bias.stride(-2) == T
        sb = bias.stride(0) if bias.shape[0] > 1 else 0
        sh = bias.stride(1) if bias.shape[1] > 1 else 0
    _lib.launch('veon_vit_block', dev, x, ctypes.byref(w.c), bias, sb, sh, ws, ws.numel(),
                B, T, w.d, w.heads)
    return x
