"""CLIP ViT residual-attention blocks of SAN-CLIP on the MFMA kernels.

In the reference the CLIP transformer arithmetic is NOT in the tree: it lives in
third-party ``open_clip`` (``open_clip.transformer.ResidualAttentionBlock`` /
``VisionTransformer``; version unpinned anywhere in the reference -- SURVEY 8c),
and VEON only wraps it: ``FeatureExtractor`` runs ``conv1`` / class + position
embeddings / ``ln_pre`` / the first K ``resblocks``
(mmdet3d/models/semantic_net/clip_utils/visual.py:57-91) and
``update_remaining_clip_feats`` runs the tail blocks again over all tokens with
a dense additive ``attn_mask`` of shape (B*heads, L+1, L+1) (:258-285).
This module restates the published block
    x = x + attn(ln_1(x), attn_mask);  x = x + mlp(ln_2(x))
with ``nn.MultiheadAttention``'s packed ``in_proj_weight`` / ``in_proj_bias`` /
``out_proj`` and ``mlp.c_fc`` / ``mlp.c_proj`` parameter names (what an
``open_clip`` checkpoint holds), QuickGELU for OpenAI weights.
**Block parity unpinned**: ``open_clip`` is not installed and the reference holds
no vectors for it; tests compare against ``torch.nn.MultiheadAttention``
semantics.  What the reference itself owns around the block IS pinned by vectors
generated from its unmodified files (oracle/tools/gen_golden_clip_*.py): the
query-token cross attention with the extra "self" logit (attn_helper.py:34-300,
PyTorch here; natively with ``ClipRecHead.hip_query``), the trunk wiring
(``FeatureExtractor``) and the recognition head (``RecWithAttnbiasHead``).
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import vit_ops
from .._native_cache import NativeCacheMixin
from .._train_fns import _GeluFn, _LinearTrainFn, _LNHalfFn, _QuickGeluFn
from .resize import interpolate


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


def _ln_train_ok(ln, d):
    return (type(ln) is nn.LayerNorm and tuple(ln.normalized_shape) == (d,)
            and ln.weight is not None and ln.bias is not None
            and ln.weight.dtype == torch.float32 and ln.bias.dtype == torch.float32)


def _mask_train_ok(m, N, H, L):
    """None, or a floating additive mask (N, H, Lb, Lb) with unit-size batch / head axes
    allowed, (N*H, Lb, Lb) or (Lb, Lb), Lb = L (with the class token) or L - 1 (without)."""
    if m is None:
        return True
    if not (torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float32
            and m.dim() in (2, 3, 4) and m.shape[-1] == m.shape[-2]
            and m.shape[-1] in (L, L - 1)):
        return False
    if m.dim() == 3:
        return m.shape[0] == N * H
    return m.dim() == 2 or (m.shape[0] in (1, N) and m.shape[1] in (1, H))


class ResidualAttentionBlock(nn.Module):
    """``hip_train`` (class attribute, default False): opt-in native TRAINING path.  When
    set, a block under autograd on ROCm fp32 tokens whose shapes the kernels take
    (``_hip_train_ok``) runs its LayerNorms, the four Linears, the attention with its dense
    additive mask (csrc/attention_train.hip: the only T x T tensor saved is the mask it was
    handed, and the mask receives its gradient) and the activation, forward and backward, in
    HIP on half rows; the residual adds stay in torch on the fp32 stream.  The block has no
    dropout and no batch statistics, so unlike the other ``hip_train`` switches this one
    does NOT depend on ``.training``.  Anything else takes ``forward``'s lines unchanged."""

    hip_train = False

    def __init__(self, d_model, n_head, mlp_ratio=4.0, quick_gelu=True):
        super().__init__()
        self.ln_1 = nn.LayerNorm(d_model)
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ls_1 = nn.Identity()
        self.ln_2 = nn.LayerNorm(d_model)
        width = int(d_model * mlp_ratio)
        self.mlp = nn.Sequential(OrderedDict([
            ('c_fc', nn.Linear(d_model, width)),
            ('gelu', QuickGELU() if quick_gelu else nn.GELU()),
            ('c_proj', nn.Linear(width, d_model))]))
        self.ls_2 = nn.Identity()
        self.n_head = n_head
        self.quick_gelu = quick_gelu

    def _hip_train_ok(self, x, attn_mask=None):
        """The native training path's own test: the switch, autograd, ROCm fp32 tokens
        (L, N, D), D % 64 == 0, head dim 64, D <= 1024 (the LayerNorm backward), MLP width
        % 64 == 0, affine fp32 LayerNorms, QuickGELU or exact
        GELU, identity ``ls_1`` / ``ls_2``, fp32 parameters, an nn.MultiheadAttention with
        its packed in_proj and an out_proj with bias and no dropout, and a mask that is None
        or a floating additive one of the three shapes.  Not ``.training``: see the class."""
        if not (self.hip_train and torch.is_grad_enabled() and torch.is_tensor(x)
                and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and type(self.attn) is nn.MultiheadAttention
                and type(self.mlp) is nn.Sequential and len(self.mlp) == 3):
            return False
        a, d = self.attn, x.shape[-1]
        L, N = x.shape[:2]
        fc, act, pr = self.mlp[0], self.mlp[1], self.mlp[2]
        return (d % 64 == 0 and d <= 1024 and a.embed_dim == d and d == a.num_heads * 64
                and a.num_heads == self.n_head
                and a.in_proj_weight is not None and a.in_proj_bias is not None
                and a._qkv_same_embed_dim and a.dropout == 0.0 and not a.batch_first
                and a.bias_k is None and a.bias_v is None and not a.add_zero_attn
                and isinstance(a.out_proj, nn.Linear) and a.out_proj.bias is not None
                and type(fc) is nn.Linear and type(pr) is nn.Linear
                and fc.bias is not None and pr.bias is not None
                and fc.in_features == d and fc.out_features % 64 == 0
                and pr.in_features == fc.out_features and pr.out_features == d
                and _ln_train_ok(self.ln_1, d) and _ln_train_ok(self.ln_2, d)
                and (type(act) is QuickGELU
                     or (type(act) is nn.GELU and getattr(act, 'approximate', 'none') == 'none'))
                and type(self.ls_1) is nn.Identity and type(self.ls_2) is nn.Identity
                and all(p.dtype == torch.float32 and p.is_cuda for p in self.parameters())
                and _mask_train_ok(attn_mask, N, a.num_heads, L))

    def _hip_train_forward(self, x, attn_mask=None):
        """The native step on BATCH-MAJOR fp32 tokens x (N, L, D) -> (N, L, D)."""
        N, L, d = x.shape
        a, n1, n2 = self.attn, self.ln_1, self.ln_2
        fc, act, pr = self.mlp[0], self.mlp[1], self.mlp[2]
        scale = (d // a.num_heads) ** -0.5
        xn = _LNHalfFn.apply(x, n1.weight, n1.bias, n1.eps)              # half [N*L, d]
        qkv = _LinearTrainFn.apply(xn, a.in_proj_weight, a.in_proj_bias).view(N, L, 3 * d)
        if attn_mask is None:
            o = vit_ops.attention_train(qkv, a.num_heads, scale)         # raw q: no scale
        else:
            o = vit_ops.attention_bias_train(qkv, attn_mask, a.num_heads, scale,
                                             border=L - attn_mask.shape[-1])
        y = _LinearTrainFn.apply(o.view(N * L, d), a.out_proj.weight, a.out_proj.bias)
        x = x + y.view(N, L, d).float()
        xn = _LNHalfFn.apply(x, n2.weight, n2.bias, n2.eps)
        h = _LinearTrainFn.apply(xn, fc.weight, fc.bias)
        h = (_QuickGeluFn if type(act) is QuickGELU else _GeluFn).apply(h)
        y = _LinearTrainFn.apply(h, pr.weight, pr.bias)
        return x + y.view(N, L, d).float()

    def forward(self, x, attn_mask=None):
        """x (L, N, D) sequence-first, attn_mask additive (N*heads, L, L) or
        (L, L), as open_clip passes it."""
        if self._hip_train_ok(x, attn_mask):
            return self._hip_train_forward(x.permute(1, 0, 2), attn_mask).permute(1, 0, 2)
        h = self.ln_1(x)
        a = self.attn(h, h, h, need_weights=False, attn_mask=attn_mask)[0]
        x = x + self.ls_1(a)
        return x + self.ls_2(self.mlp(self.ln_2(x)))


def cross_attn_with_self_bias(attn, query, key, value, attn_mask=None):
    """The SOS/query-token attention of SAN's ``RecWithAttnbiasHead``
    (mmdet3d/models/semantic_net/attn_helper.py:34-300, called from
    ``cross_attn_layer`` :303-314): queries (K, N, D) attend over the memory
    tokens (L, N, D) with an additive per-head bias (N*heads, K, L) and, in
    addition, over THEMSELVES through one extra logit q.k_self whose value is
    the query's own v projection -- a softmax over L + 1 logits per query.
    ``attn`` is an nn.MultiheadAttention holding the packed projections.
    PyTorch implementation; ``ClipRecHead.hip_query`` runs the same arithmetic on the
    library (``vit_ops.query_attention``)."""
    K, N, D = query.shape
    L = key.shape[0]
    H = attn.num_heads
    hd = D // H
    w, b = attn.in_proj_weight, attn.in_proj_bias
    q = F.linear(query, w[:D], b[:D]) * hd ** -0.5
    k = F.linear(key, w[D:2 * D], b[D:2 * D])
    v = F.linear(value, w[2 * D:], b[2 * D:])
    q_k = F.linear(query, w[D:2 * D], b[D:2 * D])   # the query as its own key
    q_v = F.linear(query, w[2 * D:], b[2 * D:])     # ... and value

    def heads(t):  # (T, N, D) -> (N*H, T, hd)
        return t.contiguous().view(t.shape[0], N * H, hd).transpose(0, 1)
    q, k, v, q_k, q_v = heads(q), heads(k), heads(v), heads(q_k), heads(q_v)
    logits = torch.bmm(q, k.transpose(1, 2))                   # (N*H, K, L)
    if attn_mask is not None:
        if attn_mask.dtype == torch.bool:
            logits = logits.masked_fill(attn_mask, float('-inf'))
        else:
            logits = logits + attn_mask
    self_logit = (q * q_k).sum(dim=-1, keepdim=True)           # (N*H, K, 1)
    p = F.softmax(torch.cat([logits, self_logit], dim=-1), dim=-1)
    out = torch.bmm(p[:, :, :-1], v) + p[:, :, -1:] * q_v      # (N*H, K, hd)
    out = out.transpose(0, 1).contiguous().view(K, N, D)
    return F.linear(out, attn.out_proj.weight, attn.out_proj.bias)


def cross_attn_layer(block, x, mem, attn_bias):
    """attn_helper.py:303-314: x (K,N,D) queries, mem (L,N,D), attn_bias
    (N*heads, K, L)."""
    q_x = block.ln_1(x)
    k_x = block.ln_1(mem)
    x = x + block.ls_1(cross_attn_with_self_bias(block.attn, q_x, k_x, k_x,
                                                 attn_mask=attn_bias))
    return x + block.ls_2(block.mlp(block.ln_2(x)))


class _HipClipWeights:
    def __init__(self, blk):
        a = blk.attn
        d = a.embed_dim
        scale = (d // a.num_heads) ** -0.5
        w = a.in_proj_weight.detach().float().clone()
        b = a.in_proj_bias.detach().float().clone()
        # F.multi_head_attention_forward scales q; log2(e) rides along (exp2-domain
        # attention kernel, BlockWeights(q_log2=True))
        w[:d] *= scale * vit_ops.LOG2E
        b[:d] *= scale * vit_ops.LOG2E
        self.heads = a.num_heads
        self.w_qkv, self.b_qkv = vit_ops.to_bf16(w), b.contiguous()
        self.w_proj = vit_ops.to_bf16(a.out_proj.weight.detach().float())
        self.b_proj = a.out_proj.bias.detach().float().contiguous()
        self.w_fc1 = vit_ops.to_bf16(blk.mlp.c_fc.weight.detach().float())
        self.b_fc1 = blk.mlp.c_fc.bias.detach().float().contiguous()
        self.w_fc2 = vit_ops.to_bf16(blk.mlp.c_proj.weight.detach().float())
        self.b_fc2 = blk.mlp.c_proj.bias.detach().float().contiguous()
        self.n1 = (blk.ln_1.weight.detach().float().contiguous(),
                   blk.ln_1.bias.detach().float().contiguous(), blk.ln_1.eps)
        self.n2 = (blk.ln_2.weight.detach().float().contiguous(),
                   blk.ln_2.bias.detach().float().contiguous(), blk.ln_2.eps)
        self.act = vit_ops.EPI_QUICKGELU if blk.quick_gelu else vit_ops.EPI_GELU
        self.packed = vit_ops.BlockWeights(
            self.heads, self.n1, self.w_qkv, self.b_qkv, self.w_proj, self.b_proj,
            None, self.n2, self.w_fc1, self.b_fc1, self.w_fc2, self.b_fc2, None,
            self.act, q_log2=True)


def hip_blocks_ok(blocks, x, D):
    """The condition of run_blocks' MFMA path."""
    return (x.is_cuda and not torch.is_grad_enabled()
            and not any(b.training for b in blocks)
            and D % 64 == 0 and all(D // b.n_head == 64 for b in blocks))


def hip_train_blocks_ok(blocks, x_lnd, attn_masks=None):
    """The condition of run_blocks' native training path: the inference path does not
    apply and every block passes its ``_hip_train_ok`` with its mask.  The switch is read
    first, so that with it off (the default) a call costs one attribute read per block."""
    if not blocks or not all(getattr(b, 'hip_train', False) for b in blocks) \
            or hip_blocks_ok(blocks, x_lnd, x_lnd.shape[-1]):
        return False
    return all(b._hip_train_ok(x_lnd, None if attn_masks is None else attn_masks[i])
               for i, b in enumerate(blocks))


def run_blocks(blocks, x_lnd, attn_masks=None, cache=None, keep=None, stream=None,
               train_native=None):
    """Run ``blocks`` over x (L, N, D).  On a ROCm device in no-grad eval mode
    the MFMA kernels are used (one transpose in, one out); under autograd with
    ``ResidualAttentionBlock.hip_train`` set and every block passing ``_hip_train_ok``, the
    native training path (batch-major, one transpose in, every output handed back as an
    (L, N, D) view whatever ``keep`` says; a mask whose last axis is L - 1 is the
    patch-to-patch bias and goes to the kernel with ``border`` = 1); otherwise the torch
    blocks.  attn_masks: None or one additive mask per block, each
    (N*heads, L, L) / (N, heads, L, L) / (L, L).  Returns the list of per-block
    outputs (L, N, D).  ``keep``: indices of the blocks whose output the caller reads
    (the last one always is); the native path leaves the others as None instead of
    copying the stream out after every block.  ``train_native``: a caller that has already
    evaluated ``hip_train_blocks_ok`` for these arguments hands its answer over; None
    evaluates it here."""
    L, N, D = x_lnd.shape
    if train_native is None:
        train_native = hip_train_blocks_ok(blocks, x_lnd, attn_masks)
    hip = not train_native and hip_blocks_ok(blocks, x_lnd, D)
    outs = []
    if train_native:
        x = x_lnd.permute(1, 0, 2).contiguous()
        for i, blk in enumerate(blocks):
            x = blk._hip_train_forward(x, None if attn_masks is None else attn_masks[i])
            outs.append(x.permute(1, 0, 2))
        return outs
    if not hip:
        x = x_lnd
        for i, blk in enumerate(blocks):
            m = None if attn_masks is None else attn_masks[i]
            if m is not None and m.dim() == 4:
                m = m.reshape(-1, L, L)
            x = blk(x, attn_mask=m)
            outs.append(x)
        return outs
    if cache is None:
        cache = {}
    # private batch-major fp32 copy of the stream (the kernels update it in place);
    # ``stream``: the caller already holds one ((N, L, D) fp32, its to overwrite) of
    # which x_lnd is the (L, N, D) view
    if stream is not None:
        assert stream.shape == (N, L, D) and stream.dtype == torch.float32 \
            and stream.is_contiguous()
        s = stream
    else:
        s = torch.empty((N, L, D), dtype=torch.float32, device=x_lnd.device)
        s.copy_(x_lnd.permute(1, 0, 2))
    s = s.view(N * L, D)
    ws = None
    for i, blk in enumerate(blocks):
        w = cache.get(id(blk))
        if w is None:
            w = cache[id(blk)] = _HipClipWeights(blk)
        m = None if attn_masks is None else attn_masks[i]
        if m is not None:
            m = m.float()
            if m.dim() == 2:
                m = m.view(1, 1, L, L)
            elif m.dim() == 3:
                m = m.view(N, -1, L, L)
            m = m.contiguous()
        if ws is None:
            ws = vit_ops.block_workspace(N, L, D, w.packed.mlp_dim, s.device)
        vit_ops.block_forward_(s, w.packed, N, L, ws, m)
        if keep is None or i in keep or i == len(blocks) - 1:
            # (L, N, D)-shaped VIEW of a batch-major snapshot (the stream itself after
            # the last block): ClipRecHead._save's permute / reshape to an (N, C, h, w)
            # map is then a view too (channels-last strides) -- one copy per tapped
            # layer instead of two, none for the last
            snap = s.view(N, L, D) if i == len(blocks) - 1 else s.view(N, L, D).clone()
            outs.append(snap.permute(1, 0, 2))
        else:
            outs.append(None)
    return outs


class ClipVisualTrunk(NativeCacheMixin, nn.Module):
    """conv1 patchify + class / position embeddings + ln_pre + resblocks: what
    ``FeatureExtractor.forward`` runs (clip_utils/visual.py:57-91), with
    open_clip's VisionTransformer parameter names."""

    # rebound, not cleared: ``run_blocks`` holds the dict object it was handed
    _native_cache = {'_hip_cache': dict, '_pos_cache': dict}

    def __init__(self, image_size=224, patch_size=16, width=768, layers=12,
                 heads=12, mlp_ratio=4.0, quick_gelu=True):
        super().__init__()
        self.grid_size = (image_size // patch_size, image_size // patch_size)
        self.patch_size = patch_size
        self.conv1 = nn.Conv2d(3, width, patch_size, patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(
            scale * torch.randn(self.grid_size[0] * self.grid_size[1] + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.resblocks = nn.ModuleList(
            [ResidualAttentionBlock(width, heads, mlp_ratio, quick_gelu)
             for _ in range(layers)])
        self._hip_cache = {}
        self._pos_cache = {}

    def _pos_embed(self, h, w):
        pe = self.positional_embedding
        if (h, w) == self.grid_size:
            return pe
        inference = not (self.training or torch.is_grad_enabled())
        key = (h, w, pe.device, pe.dtype)
        if inference and key in self._pos_cache:
            return self._pos_cache[key]
        cls, grid = pe[:1], pe[1:]
        grid = grid.reshape(1, self.grid_size[0], self.grid_size[1], -1).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, size=(h, w), mode='bicubic', align_corners=False)
        out = torch.cat([cls, grid.permute(0, 2, 3, 1).reshape(h * w, -1)], 0)
        if inference:  # the resize costs more than a block at these sizes
            self._pos_cache[key] = out
        return out

    def _patchify(self, x):
        """conv1 (kernel = stride = patch): at inference the non-overlapping
        patches are gathered and multiplied as one GEMM -- the same sums without
        a convolution library call."""
        p = self.patch_size
        N, C, H, W = x.shape
        if self.training or torch.is_grad_enabled():
            x = self.conv1(x)
            _, _, h, w = x.shape
            return x.flatten(2).permute(0, 2, 1), (h, w)
        h, w = H // p, W // p
        if H % p or W % p:   # a stride-p conv without padding never reads the remainder
            x = x[:, :, :h * p, :w * p].contiguous()     # (ViT-L/14 on 128 x 352: 9 x 25)
        cols = x.view(N, C, h, p, w, p).permute(0, 2, 4, 1, 3, 5).reshape(N * h * w, C * p * p)
        out = cols @ self.conv1.weight.view(self.conv1.out_channels, -1).t()
        return out.view(N, h * w, -1), (h, w)

    def tokens(self, x):
        x, (h, w) = self._patchify(x)
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self._pos_embed(h, w).to(x.dtype)
        return self.ln_pre(x).permute(1, 0, 2), (h, w)     # LND

    def _native_stream(self, x):
        """``tokens`` at inference as four launches: the position rows (+ the class
        embedding in row 0) repeated into a fresh fp32 stream, the patches gathered as
        bf16 GEMM rows (class-token slots zero), one MFMA GEMM accumulating conv-weight x
        patch onto the stream, ln_pre fp32 -> fp32.  -> ((N, L, D) fp32, (h, w)).
        (The patch product runs on bf16 operands here; everything after it does anyway.)"""
        N, C, H, W = x.shape
        p, D = self.patch_size, self.conv1.out_channels
        h, w = H // p, W // p
        key = ('tok', h, w, x.device)
        if key not in self._pos_cache:
            k = C * p * p
            kpad = (k + 63) // 64 * 64
            wp = torch.zeros(D, kpad, device=x.device)
            wp[:, :k] = self.conv1.weight.detach().float().view(D, k)
            base = self._pos_embed(h, w).detach().float().clone()
            base[0] += self.class_embedding.detach().float()
            self._pos_cache[key] = (vit_ops.to_bf16(wp), base.contiguous(), kpad)
        wp, base, kpad = self._pos_cache[key]
        s = base.repeat(N, 1)           # always a fresh buffer: the blocks run in place on it
        assert s.data_ptr() != base.data_ptr()
        vit_ops.linear_residual_(s, vit_ops.patchify(x, p, 1, kpad), wp, None)
        s = vit_ops.layernorm_f32(s, self.ln_pre.weight.detach(), self.ln_pre.bias.detach(),
                                  self.ln_pre.eps)
        return s.view(N, 1 + h * w, D), (h, w)

    def forward(self, x, last_layer_idx=-1, attn_masks=None, taps=None):
        """-> (list of per-block token tensors (L,N,D), (h, w)); entry 0 = the tokens
        after ``ln_pre``, entry i = the output of block i.  ``taps``: the entries the
        caller reads (None = all); untapped entries may come back as None."""
        blocks = list(self.resblocks if last_layer_idx == -1
                      else self.resblocks[:last_layer_idx])
        keep = None if taps is None else {i - 1 for i in taps if i >= 1}
        D = self.conv1.out_channels
        if (hip_blocks_ok(blocks, x, D) and not self.training and D % 128 == 0
                and D <= 1024 and x.dtype == torch.float32 and blocks):
            s, hw = self._native_stream(x)
            t = (s.clone() if taps is None or 0 in taps else s).permute(1, 0, 2)
            return [t] + run_blocks(blocks, t, attn_masks, self._hip_cache, keep,
                                    stream=s), hw
        t, hw = self.tokens(x)
        return [t] + run_blocks(blocks, t, attn_masks, self._hip_cache, keep), hw


class ClipRecHead(NativeCacheMixin, nn.Module):
    """Mirror of ``RecWithAttnbiasHead`` (clip_utils/visual.py:112-292) for the
    configuration VEON uses (``cross_attn=True``): the tail blocks
    ``resblocks[first_layer_idx:]`` of the CLIP visual transformer, ``ln_post``
    and ``proj``.

    * ``forward(features, attn_bias)``: the SOS/query tokens attend over the
      patch tokens of layer ``first_layer_idx`` through ``cross_attn_layer``
      (per-head additive bias + self logit) while the patch tokens run through
      the plain blocks; returns the projected query tokens (:164-216).
    * ``update_remaining_clip_feats(clip_outputs, offsets, attns)``: the tail
      blocks once more over all tokens, with feature offsets added before the
      first and the middle block and a dense additive (B*heads, L+1, L+1) mask
      per block; fills the per-layer outputs and ``clip_feat_proj`` (:258-285).
      On a ROCm device at inference the blocks run on the MFMA kernels
      (``run_blocks``).

    ``features`` / ``clip_outputs``: dict with ``[i]`` = (N,C,h,w) patch map and
    ``['%d_cls_token' % i]`` = (1,N,C), as ``ClipOutput`` in the reference.

    ``hip_query`` (class attribute, default False; ``forward(hip_query=...)`` overrides it
    for one call): opt-in native query path.  When set, and ``_hip_query_ok`` holds (a ROCm
    device, no autograd, every block in eval mode, fp32 tokens, D % 64 == 0, head_dim 64),
    ``forward`` runs the SOS/query tokens batch-major on the library, nine launches per
    tail block (``_native_queries``) and no fp32 projection; ``ln_post``, ``proj`` and
    ``normalize`` stay in torch.  Anything else takes ``cross_attn_layer`` unchanged.
    """

    _native_cache = {'_hip_cache': dict}
    hip_query = False

    def __init__(self, resblocks, ln_post, proj, first_layer_idx=0,
                 sos_token_format='cls_token', sos_token_num=1,
                 downsample_method='bilinear'):
        super().__init__()
        if first_layer_idx < 0:
            raise NotImplementedError('first_layer_idx < 0 is not implemented yet.')
        self.first_layer_idx = first_layer_idx
        self.resblocks = nn.ModuleList(list(resblocks)[first_layer_idx:])
        self.ln_post = ln_post
        self.proj = proj                       # (width, output_dim) parameter
        self.sos_token_format = sos_token_format
        self.sos_token_num = sos_token_num
        self.downsample_method = downsample_method
        if sos_token_format in ('learnable_token', 'pos_embedding'):
            self.sos_token = nn.Parameter(
                torch.randn(sos_token_num, 1, proj.shape[0]) * 0.02)
        self._hip_cache = {}

    @staticmethod
    def _save(outputs, idx, tokens, hw):
        l, n, c = tokens.shape
        outputs[idx] = tokens[1:].permute(1, 2, 0).reshape(n, c, *hw)
        outputs['%d_cls_token' % idx] = tokens[0:1]

    def _build_attn_biases(self, attn_biases, target_shape):
        """[N, heads|1, num_sos, H, W] per entry -> (N*heads, num_sos, h*w)
        (:218-256, the cross_attn branch)."""
        out = []
        true_heads = self.resblocks[0].attn.num_heads
        for ab in attn_biases:
            n, num_head, num_sos, h, w = ab.shape
            ab = ab.reshape(n, num_head * num_sos, h, w)
            if (h, w) == tuple(target_shape):
                pass        # already at the target grid (MLPMaskDecoder.attn_bias_at)
            elif self.downsample_method in ('bicubic', 'bilinear', 'nearest'):
                ab = interpolate(ab, size=target_shape, mode=self.downsample_method,
                                 align_corners=False)
            elif self.downsample_method == 'avg':
                ab = F.adaptive_avg_pool2d(ab, output_size=target_shape)
            else:
                ab = F.adaptive_max_pool2d(ab, output_size=target_shape)
            ab = ab.reshape(n, num_head, num_sos, *target_shape)
            assert num_head in (1, true_heads), 'num_head=%d is not supported.' % num_head
            if num_head == 1:
                ab = ab.repeat(1, true_heads, 1, 1, 1)
            out.append(ab.reshape(n * true_heads, num_sos, -1))
        if len(out) == 1:
            out = [out[0] for _ in self.resblocks]
        return out

    def _hip_query_ok(self, x):
        """The native query path's own test (the switch is read by ``forward``): the
        condition of ``run_blocks``' MFMA path over ALL tail blocks, on fp32 tokens."""
        blocks = list(self.resblocks)
        return (bool(blocks) and x.dtype == torch.float32
                and hip_blocks_ok(blocks, x, x.shape[-1]))

    def _native_queries(self, blocks, sos, xs, biases):
        """``cross_attn_layer`` over the tail blocks on the library: sos (K, N, D) fp32 query
        tokens, xs[i] (L, N, D) the memory of block i, biases[i] (N*heads, K, L - 1) float
        or bool -> (K, N, D), a view of a batch-major stream.  Per block: LayerNorm and the
        K/V half of the packed projection over the memory rows (the q rows of the weight
        are skipped: a contiguous row slice), LayerNorm and the whole projection over the
        query rows, ``veon_query_attention`` (key0 = 1: the patch tokens only, exp2
        domain), out_proj onto the stream, LayerNorm, fc1 + activation, fc2 onto the
        stream."""
        K, N, D = sos.shape
        s = torch.empty((N, K, D), dtype=torch.float32, device=sos.device)
        s.copy_(sos.permute(1, 0, 2))         # a private stream: updated in place
        s = s.view(N * K, D)
        for i, blk in enumerate(blocks):
            w = self._hip_cache.get(id(blk))
            if w is None:
                w = self._hip_cache[id(blk)] = _HipClipWeights(blk)
            H = w.heads
            # run_blocks' native snapshots are batch-major already: no copy then
            mem = xs[i].permute(1, 0, 2).contiguous()
            L = mem.shape[1]
            hm = vit_ops.layernorm(mem.view(N * L, D), *w.n1)
            mem_kv = vit_ops.linear(hm, w.w_qkv[D:], w.b_qkv[D:]).view(N, L, 2, H, 64)
            hq = vit_ops.layernorm(s, *w.n1)
            q_qkv = vit_ops.linear(hq, w.w_qkv, w.b_qkv).view(N, K, 3, H, 64)
            b = biases[i]
            if b is not None:
                if b.dtype == torch.bool:
                    b = torch.zeros(b.shape, dtype=torch.float32, device=b.device) \
                        .masked_fill_(b, float('-inf'))
                b = b.float().reshape(N, H, K, L - 1)
            o = vit_ops.query_attention(q_qkv, mem_kv, H, b, key0=1, q_log2=True)
            vit_ops.linear_residual_(s, o.view(N * K, D), w.w_proj, w.b_proj)
            h2 = vit_ops.layernorm(s, *w.n2)
            u = vit_ops.linear(h2, w.w_fc1, w.b_fc1, epilogue=w.act)
            vit_ops.linear_residual_(s, u, w.w_fc2, w.b_fc2)
        return s.view(N, K, D).permute(1, 0, 2)

    def forward(self, features, attn_bias, normalize=False, clip_outputs=None,
                hip_query=None):
        k0 = self.first_layer_idx
        cls_token = features['%d_cls_token' % k0]        # 1,n,c
        pix = features[k0]                               # n,c,h,w
        n, c, h, w = pix.shape
        x = torch.cat([cls_token, pix.reshape(n, c, -1).permute(2, 0, 1)])
        if self.sos_token_format == 'cls_token':
            sos = cls_token.repeat(self.sos_token_num, 1, 1)
        elif self.sos_token_format == 'learnable_token':
            sos = self.sos_token.expand(-1, n, -1)
        else:
            sos = self.sos_token.expand(-1, n, -1) + cls_token
        biases = self._build_attn_biases(attn_bias, (h, w))
        blocks = list(self.resblocks)
        # the patch tokens run through the plain blocks (the last one only when its
        # output is saved): all at once, on the MFMA kernels where run_blocks can
        run = blocks if clip_outputs is not None else blocks[:-1]
        xs = [x] + (run_blocks(run, x, None, self._hip_cache) if run else [])
        native = (self.hip_query if hip_query is None else hip_query) \
            and self._hip_query_ok(x)
        if native:
            sos = self._native_queries(blocks, sos, xs, biases)
        for i, blk in enumerate(blocks):
            if not native:
                sos = cross_attn_layer(blk, sos, xs[i][1:], biases[i])
            if clip_outputs is not None:
                self._save(clip_outputs, i + k0 + 1, xs[i + 1], (h, w))
        sos = self.ln_post(sos.permute(1, 0, 2))
        if self.proj is not None:
            sos = sos @ self.proj
        if normalize:
            sos = F.normalize(sos, dim=-1)
        if clip_outputs is not None:
            clip_outputs['clip_feat_proj'] = torch.einsum(
                'bchw,cd->bdhw', clip_outputs[len(self.resblocks) + k0], self.proj)
            return sos, clip_outputs
        return sos

    @staticmethod
    def build_attn_bias(attn):
        """(B, heads, L, L) patch-to-patch bias -> (B*heads, L+1, L+1) with a
        zero row / column for the class token (:287-292)."""
        B, H, L, _ = attn.shape
        new = torch.zeros((B, H, L + 1, L + 1), device=attn.device, dtype=attn.dtype)
        new[:, :, 1:, 1:] = attn
        return new.reshape(B * H, L + 1, L + 1)

    def update_remaining_clip_feats(self, clip_outputs, offsets=None, attns=None,
                                    keep_layers=None):
        """``keep_layers`` (veon_amd extension): the CLIP layers the caller reads
        afterwards (None = every tail layer, as the reference saves them)."""
        k0 = self.first_layer_idx
        cls_token = clip_outputs['%d_cls_token' % k0]
        x = clip_outputs[k0]
        hw = tuple(x.shape[2:])
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(2, 0, 1)
        x = torch.cat([cls_token, x], dim=0)
        nblk = len(self.resblocks)
        # the offsets (added before block 0 and before block nblk // 2) split the
        # tail into runs of blocks that go to the MFMA path back to back
        cuts = [0, nblk] if offsets is None else sorted({0, nblk // 2, nblk})
        for a, b in zip(cuts[:-1], cuts[1:]):
            if offsets is not None:
                if a == 0:
                    x = torch.cat([x[:1], x[1:] + offsets[0].permute(1, 0, 2)], dim=0)
                if a == nblk // 2:
                    x = torch.cat([x[:1], x[1:] + offsets[1].permute(1, 0, 2)], dim=0)
                    if a > 0:
                        # reference behaviour kept: ClipOutput.save stores a VIEW
                        # of the block output, and the in-place offset add of the
                        # next iteration (:268-271) writes through it, so the
                        # saved map of the block before the middle carries the
                        # second offset too
                        self._save(clip_outputs, a + k0, x, hw)
            # (biases that already carry the class token's zero row / column --
            # AttnManipulateBlock.pad_class_token -- pass through)
            L1 = x.shape[0]
            blocks = list(self.resblocks)[a:b]
            native = attns is not None and hip_train_blocks_ok(blocks, x, attns[a:b])
            if native:
                # the native training path takes the patch-to-patch matrix as it is: the
                # class token's zero row / column is the kernel's ``border``
                masks = list(attns[a:b])
            else:
                masks = None if attns is None else \
                    [attns[t].reshape(-1, L1, L1) if attns[t].shape[-1] == L1
                     else self.build_attn_bias(attns[t]) for t in range(a, b)]
            keep = None if keep_layers is None else \
                {t - a for t in range(a, b) if t + k0 + 1 in keep_layers}
            outs = run_blocks(blocks, x, masks, self._hip_cache, keep,
                              train_native=None if attns is None else native)
            for t, o in zip(range(a, b), outs):
                if o is not None and (keep_layers is None or t + k0 + 1 in keep_layers
                                      or t + 1 == nblk):
                    self._save(clip_outputs, t + k0 + 1, o, hw)
            x = outs[-1]
        clip_outputs['clip_feat_proj'] = torch.einsum(
            'bchw,cd->bdhw', clip_outputs[nblk + k0], self.proj)
        return clip_outputs
