"""Hostile operands, fp64 references, an emulation of the kernel's arithmetic and an
elementwise error bound for the attention of training (csrc/attention_train.hip, DESIGN
section 4n), shared by tests/test_attention_train_refs.py (CPU) and
tests/test_vit_train_hostile_gpu.py.  A plain module: no fixtures, nothing device-specific
(every function computes where its operands live), and nothing of the code under test but
``vit_ops.attention_ref`` (the definition) and ``vit_ops.LOG2E``.

Layouts: qkv [B, T, 3 H 64] and dout [B, T, H 64] as the kernels take them; everything
"per head" here is [B, H, T, .] (``heads``) and a gradient is split by ``thirds``.
"""
import torch

from veon_amd import vit_ops

HD = 64
B = 2
SCALE = 0.125
# |lse - fp64| in log2 units.  Stated for a row sum of half-rounded weights (relative error
# 2^-9 / 2^-12 each, log2(1 + e) <= 1.45 e, plus fp32 slack) and kept at that; the kernel
# sums the weights in fp32 before their rounding and stays orders below it
LSE_BOUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# unit roundoff of a half result
U = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}

# (case, T): T from the kernel's seams -- 65: one live row in the last streamed 64-row tile;
# 129: one row past the 128-row workgroup; 200: several tiles
CASES = [('big4', 65), ('big4', 129),
         ('outlier8', 65), ('outlier8', 129), ('outlier8', 200),
         ('voffset8', 65), ('voffset8', 129),
         ('doffset16', 129),
         ('onehot', 65), ('onehot', 129),
         ('samekeys', 129),
         ('mixed', 129)]
GAUSS = ('gauss', 129)     # the unmodified construction, for comparison (CPU file only)
THIRDS = ('dq', 'dk', 'dv')


def heads_of(name):
    return 3 if name == 'mixed' else 2


def _big4(x, h):
    x[:, :, :2, h] *= 4


def _onehot(x, h):
    x[:, :, 1, h] = x[:, :, 0, h]
    x[:, :, :2, h] *= 3


def operands(name, T, dtype):
    """(qkv, dout) of one case on the CPU in ``dtype``: N(0, 1) draws of a seeded
    generator, the case's modification, the cast, and then q values below 2^-10 in
    magnitude set to zero (so that q / 8 is exact in fp16 too: the premise of the bit
    equality of the two forward forms).

      big4       q and k x 4: logit s.d. about 16, the median largest weight about 0.98
      outlier8   key 0 and value 0 of every (b, h) x 8: one massive-activation token
      voffset8   v + 8: dP and delta share a large term that must cancel
      doffset16  dout + 16: the same on the gradient's side
      onehot     k = q, then q and k x 3: every row saturated on its own key
      samekeys   every key of a (b, h) equals key 0: uniform softmax, dq = 0 exactly
      mixed      H = 3: head 0 big4, head 1 unmodified, head 2 onehot
      gauss      unmodified"""
    H = heads_of(name)
    g = torch.Generator().manual_seed(1000 * B + 10 * T + H)
    x = torch.randn(B, T, 3, H, HD, generator=g)
    dout = torch.randn(B, T, H * HD, generator=g)
    if name == 'big4':
        for h in range(H):
            _big4(x, h)
    elif name == 'outlier8':
        x[:, 0, 1:] *= 8
    elif name == 'voffset8':
        x[:, :, 2] += 8
    elif name == 'doffset16':
        dout += 16
    elif name == 'onehot':
        for h in range(H):
            _onehot(x, h)
    elif name == 'samekeys':
        x[:, :, 1] = x[:, :1, 1]
    elif name == 'mixed':
        _big4(x, 0)
        _onehot(x, 2)
    else:
        assert name == 'gauss', name
    x = x.to(dtype)
    q = x[:, :, 0]
    q[q.abs().float() < 2.0 ** -10] = 0
    return x.view(B, T, 3 * H * HD), dout.to(dtype)


def checks(name):
    """[(head or None for all, third, 'rel' | 'abs')]: where the project's relative rule
    e <= 2 e(torch) applies and where only the elementwise bound does (the true gradient is
    zero or many orders below the operands)."""
    if name == 'onehot':
        return [(None, i, 'abs') for i in range(3)]
    if name == 'samekeys':
        return [(None, 0, 'abs'), (None, 1, 'rel'), (None, 2, 'rel')]
    if name == 'mixed':
        return [(h, i, 'abs' if h == 2 else 'rel') for h in range(3) for i in range(3)]
    return [(None, i, 'rel') for i in range(3)]


# ------------------------------------------------------------------------------ layouts
def heads(t, H):
    """[B, T, H 64] -> [B, H, T, 64]"""
    return t.reshape(t.shape[0], t.shape[1], H, HD).permute(0, 2, 1, 3)


def thirds(t, H):
    """qkv or dqkv [B, T, 3 H 64] -> (q, k, v), each [B, H, T, 64]"""
    return t.reshape(t.shape[0], t.shape[1], 3, H, HD).permute(2, 0, 3, 1, 4)


def pick(t, head):
    """Head ``head`` (None: all) of a [B, H, ...] tensor."""
    return t if head is None else t[:, head]


def rel_l2(got, want):
    want = want.double()
    return ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()


# --------------------------------------------------------------------------- references
def fp64_parts(qkv, dout, H, scale=SCALE):
    """The fp64 quantities of the closed form on the given (half) operands, each
    [B, H, T, .]: P, O, dP, delta [B, H, T, 1], dS, dq, dk, dv, and lse in log2 units."""
    q, k, v = thirds(qkv.double(), H)
    do = heads(dout.double(), H)
    s = (q * scale) @ k.transpose(-2, -1)
    P = s.softmax(-1)
    O = P @ v
    dP = do @ v.transpose(-2, -1)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    return {'q': q, 'k': k, 'v': v, 'dO': do, 'P': P, 'O': O, 'dP': dP, 'delta': delta,
            'dS': dS, 'dq': scale * (dS @ k), 'dk': scale * (dS.transpose(-2, -1) @ q),
            'dv': P.transpose(-2, -1) @ do,
            'lse': torch.logsumexp(s, -1) * vit_ops.LOG2E}


def autograd(qkv, dout, H, dtype, scale=SCALE):
    """(out, dqkv) of ``vit_ops.attention_ref`` by torch's autograd in ``dtype``."""
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = vit_ops.attention_ref(x, H, scale)
    dqkv, = torch.autograd.grad(out, x, dout.to(dtype))
    return out.detach(), dqkv


def emulate(qkv, dout, H, scale=SCALE):
    """The kernel's arithmetic in torch, stating where it rounds -> (out, lse, dqkv), out
    and dqkv in the operands' half dtype.  Matrix products are fp32 sums of exact products
    of half values; only the ORDER of those sums is not the kernel's, and the kernel's
    reference maximum may stand up to 8 log2 units below the true one (its weights are
    then rounded at up to 2^8 instead of at 1: the same relative rounding)."""
    dt = qkv.dtype

    def rh(t):                         # round to half, carried on in fp32
        return t.to(dt).float()
    q, k, v = thirds(qkv.float(), H)
    do = heads(dout.float(), H)
    c = torch.tensor(scale * vit_ops.LOG2E, dtype=torch.float32).item()
    s = q @ k.transpose(-2, -1)                       # raw scores, fp32
    sc = s * c
    m = sc.max(-1, keepdim=True).values
    P = torch.exp2(sc - m)
    Ph = rh(P)
    O = rh((Ph @ v) / Ph.sum(-1, keepdim=True))       # normalised by the rounded weights' sum
    lse = m + torch.log2(P.sum(-1, keepdim=True))     # from the weights before rounding
    delta = (do * O).sum(-1, keepdim=True)            # from the half-rounded O, fp32
    p = torch.exp2(sc - lse)                          # never clamped
    ds = rh(p * (do @ v.transpose(-2, -1) - delta))
    dq = rh(scale * (ds @ k))
    dk = rh(scale * (ds.transpose(-2, -1) @ q))
    dv = rh(rh(p).transpose(-2, -1) @ do)
    Bn, T = qkv.shape[:2]
    dqkv = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(Bn, T, 3 * H * HD)
    out = O.permute(0, 2, 1, 3).reshape(Bn, T, H * HD)
    return out.to(dt), lse.squeeze(-1), dqkv.to(dt)


def elementwise_bound(parts, dtype, scale=SCALE, subnormal_ds=True):
    """(dq, dk, dv) bounds [B, H, T, 64] on |kernel - fp64|, in fp64 from the inputs alone.

    The kernel forms ds = p (dp - delta') with
      p      = exp2(s c - lse'): lse' within LSE_BOUND log2 units of the true one, so p is
               within eps_l = LSE_BOUND ln 2 of P, relatively (to first order; the fp32
               evaluation of s c - lse' and of exp2 goes into the slack below);
      delta' = the fp32 sum of dO O' over 64 values, O' the half-rounded O:
               |delta' - delta| <= E_delta = (u + 64 2^-24) sum_d |dO O|;
      dp     = an fp32 sum of 64 exact products, within 64 2^-24 sum_d |dO v| of dP: no
               term of its own; it is left to the slack (2u where u would do, 1.01 where 1
               would), which the CPU test shows to hold for the emulation on every case;
    and rounds ds to half (u, relative; in fp16 additionally half the spacing of a
    subnormal, 2^-25, absolutely: on saturated rows ds is about 1e-6).  Hence
      dS_err = P ((eps_l + 2u) |dP - delta| + 1.01 E_delta)   (+ 2^-25 in fp16)
    which goes through the two products linearly; the products themselves add T 2^-24 of
    the sum of the absolute terms (fp32 accumulation) and the result's half rounding u.
    dv sums the half-rounded p against dO: (eps_l + u) P^T |dO|, within the (eps_l + 2u)
    used, and the result's rounding; in fp16 the stored p is subnormal below 2^-14, which
    adds 2^-25 sum_i |dO[i]| (on 'big4' a value that no query attends to has a dv of 1e-8
    and would otherwise be held to 1e-3 of that).  ``subnormal_ds=False`` leaves the fp16
    terms out (the CPU test shows that the emulation then exceeds the bound on 'onehot')."""
    u = U[dtype]
    eps_l = LSE_BOUND[dtype] * 0.6931471805599453
    T = parts['P'].shape[-1]
    P, dS = parts['P'], parts['dS']
    E_delta = (u + 64 * 2.0 ** -24) * (parts['dO'] * parts['O']).abs().sum(-1, keepdim=True)
    dS_err = P * ((eps_l + 2 * u) * (parts['dP'] - parts['delta']).abs() + 1.01 * E_delta)
    if dtype == torch.float16 and subnormal_ds:
        dS_err = dS_err + 2.0 ** -25
    acc = T * 2.0 ** -24 * scale
    ak, aq = parts['k'].abs(), parts['q'].abs()
    dq = scale * (dS_err @ ak) + u * parts['dq'].abs() + acc * (dS.abs() @ ak)
    dk = scale * (dS_err.transpose(-2, -1) @ aq) + u * parts['dk'].abs() + \
        acc * (dS.abs().transpose(-2, -1) @ aq)
    dv = (eps_l + 2 * u) * (P.transpose(-2, -1) @ parts['dO'].abs()) + u * parts['dv'].abs()
    if dtype == torch.float16 and subnormal_ds:
        # the stored p is subnormal in fp16 wherever P < 2^-14 (most of a saturated row):
        # 2^-25 absolutely per weight, for the same reason as on ds
        dv = dv + 2.0 ** -25 * parts['dO'].abs().sum(-2, keepdim=True)
    return dq, dk, dv


def largest_share(got, want, bound, head=None):
    """max |got - want| / bound over head ``head`` (None: all); inf where the bound is 0
    and the error is not."""
    err = pick((got.double() - want).abs(), head)
    bnd = pick(bound, head)
    share = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return float(share.max())
