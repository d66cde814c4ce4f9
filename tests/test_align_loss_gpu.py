"""GPU checks of the native feature-alignment primitive (csrc/occ_align_loss.hip via
veon_amd.align_loss.voxel_cosine) and of the loss mirrors on the device.

Forward: against the reference sequence (trilinear upsample, gather, cosine) in fp64 on
the same operands, at the bound this project holds a cosine to (test_retrieval_gpu.ATOL).

Backward: against the fp64 gradient of the same sequence.  The yardstick is the torch
fp32 formulation (upsample, gather, cosine_similarity, autograd) on the same device and
inputs: with e_ref = max |grad_ref32 - grad64| and e_nat = max |grad_native - grad64|,
e_nat <= 2 e_ref + floor.  Both are fp32 sums of the same terms in different orders and
either may be the luckier, hence the 2.  ``floor`` guards e_ref ~ 0 and comes from an
error model: an element of the gradient is a sum of n terms w * g_i * (u_c / n_i -
<f_i, u_i> f_c / (n_i^2 |f_i|)), one per (stencil candidate, entry) pair: n <= 64 x the
largest number of entries on one voxel; each term carries the rounding of a C-term dot product (relative
to |f_i| |u_i|, not to the dot product), of the 8-term blend and of its own products.  So
|error| <= (n + C + 8) * 2^-24 * sum |terms|, with sum |terms| = sum w |g_i| (|u_c| +
|f_c| / n_i) / n_i evaluated in fp64 through the same interpolation adjoint.  The floor is
taken element by element (an element that few or small terms reach gets a small one):
max over the elements of (|grad_native - grad64| - floor) <= 2 e_ref."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden
from veon_amd import _lib, align_loss
from veon_amd.align_loss import voxel_cosine
from veon_amd.models.semantic_net import occ_loss as occ_loss_mod

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ATOL = 2e-5          # tests/test_retrieval_gpu.py: fp32 accumulation of C <= 768 products
U = 2.0 ** -24
EPS = 1e-6


def sequence(feat, vox, lab, table, occ, batch=0, dtype=torch.float64):
    """The reference sequence on the device in ``dtype``; feat may be a leaf."""
    v = vox.long()
    f_up = F.interpolate(feat[batch:batch + 1].to(dtype), tuple(occ), mode='trilinear',
                         align_corners=False)[0]
    f = f_up[:, v[:, 2], v[:, 1], v[:, 0]].T
    return F.cosine_similarity(f, table.to(dtype)[lab.long()], dim=1, eps=EPS)


def grad_of(fn, feat, g):
    leaf = feat.detach().clone().requires_grad_(True)
    out = fn(leaf)
    grad, = torch.autograd.grad(out, leaf, g.to(out.dtype))
    return out.detach(), grad


def floor_of(feat, vox, lab, table, occ, g, batch=0):
    """(n + C + 8) * 2^-24 * sum |terms| of every element of the gradient (module
    docstring), fp64, shaped as ``feat``."""
    d = torch.float64
    v = vox.long()
    C = feat.shape[1]
    leaf = feat.detach().to(d).clone().requires_grad_(True)
    f_up = F.interpolate(leaf[batch:batch + 1], tuple(occ), mode='trilinear', align_corners=False)[0]
    f = f_up[:, v[:, 2], v[:, 1], v[:, 0]].T
    with torch.no_grad():
        t = table.to(d)[lab.long()]
        u = t / t.norm(dim=1, keepdim=True).clamp_min(EPS)
        n = f.norm(dim=1, keepdim=True).clamp_min(EPS)
        terms = g.to(d).abs()[:, None] * (u.abs() + f.abs() / n) / n
    sum_abs, = torch.autograd.grad((f * terms).sum(), leaf)
    Zo, Yo, Xo = occ
    keys = (v[:, 2] * Yo + v[:, 1]) * Xo + v[:, 0]
    dup = int(torch.unique(keys, return_counts=True)[1].max()) if keys.numel() else 1
    return (64 * dup + C + 8) * U * sum_abs


def uniform_entries(occ, n, K, seed, dup=0):
    """all 8 grid corners, every face, uniform random voxels; ``dup`` extra copies of a
    block of them (a voxel seen by several cameras), labels independent"""
    Z, Y, X = occ
    g = torch.Generator().manual_seed(seed)
    pts = [(x, y, z) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
    face = torch.stack([torch.randint(0, s, (48,), generator=g) for s in (X, Y, Z)], 1)
    for axis, size in enumerate((X, Y, Z)):
        for val in (0, size - 1):
            f = face.clone()
            f[:, axis] = val
            pts += [tuple(r) for r in f.tolist()]
    rnd = torch.stack([torch.randint(0, s, (n,), generator=g) for s in (X, Y, Z)], 1)
    vox = torch.cat([torch.tensor(pts), rnd])
    for k in range(dup):
        vox = torch.cat([vox, vox[k * 7:k * 7 + max(1, n // 4)]])
    vox = vox[torch.randperm(vox.shape[0], generator=g)]
    lab = torch.randint(0, K, (vox.shape[0],), generator=g)
    return vox.to(torch.int32).to(DEV), lab.to(torch.int32).to(DEV)


def slab_entries(occ, n, K, seed):
    """a thin slab (two z layers, a band of y): surface-like, heavy stencil overlap"""
    Z, Y, X = occ
    g = torch.Generator().manual_seed(seed)
    z0, y0 = Z // 2, Y // 3
    vox = torch.stack([torch.randint(0, X, (n,), generator=g),
                       y0 + torch.randint(0, max(1, min(12, Y - y0)), (n,), generator=g),
                       z0 + torch.randint(0, min(2, Z - z0), (n,), generator=g)], 1)
    lab = torch.randint(0, K, (n,), generator=g)
    return vox.to(torch.int32).to(DEV), lab.to(torch.int32).to(DEV)


def volume(B, C, low, seed, layout):
    """sem-head-like values with a region of zeros and one of tiny values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.sigmoid(2 * torch.randn((B, C) + tuple(low), generator=g)) - 0.5
    x[:, :, 0, :2, :3] = 0.0
    x[:, :, -1, -2:, :3] *= 1e-8
    x = x.to(DEV)
    if layout == 'channels_last':
        x = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    return x


def make_table(K, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, C, generator=g) * torch.logspace(-2, 1, K)[:, None]).to(DEV)


def mixed_g(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 10 ** torch.randint(-3, 2, (n,), generator=g)).to(DEV)


def check_both(feat, vox, lab, table, occ, g, batch=0, what=''):
    """forward and backward of the native op by the module docstring's rules; the
    measured triple (forward error, e_nat, e_ref)."""
    n0 = dict(_lib.CALLS)
    cos, grad = grad_of(lambda f: voxel_cosine(f, vox, lab, table, occ, EPS, batch), feat, g)
    exact = tuple(int(o) == 2 * int(i) for o, i in zip(occ, feat.shape[2:]))
    assert _lib.CALLS.get('veon_occ_align_fwd', 0) == n0.get('veon_occ_align_fwd', 0) + 1
    assert _lib.CALLS.get('veon_occ_align_bwd', 0) == n0.get('veon_occ_align_bwd', 0) + all(exact)
    cos64, grad64 = grad_of(lambda f: sequence(f, vox, lab, table, occ, batch), feat.double(), g)
    _, grad32 = grad_of(lambda f: sequence(f, vox, lab, table, occ, batch, torch.float32), feat, g)
    err = float((cos.double() - cos64).abs().max())
    assert grad.shape == feat.shape and grad.dtype == torch.float32
    assert torch.isfinite(grad).all() and torch.isfinite(cos).all()
    e_nat = float((grad.double() - grad64).abs().max())
    e_ref = float((grad32.double() - grad64).abs().max())
    floor = floor_of(feat, vox, lab, table, occ, g, batch)
    over = float(((grad.double() - grad64).abs() - floor).max())
    print('%s: N %d  max|cos - fp64| %.2e;  grad e_nat %.3e  e_ref %.3e  max floor %.3e  '
          'max|grad| %.3e' % (what, vox.shape[0], err, e_nat, e_ref, float(floor.max()),
                              float(grad64.abs().max())))
    assert err <= ATOL, err
    assert over <= 2 * e_ref, (over, e_nat, e_ref)
    if feat.shape[0] > 1:       # nothing reaches the other samples
        other = [b for b in range(feat.shape[0]) if b != batch]
        assert not grad[other].any()
    return err, e_nat, e_ref


@pytest.mark.parametrize('layout', ['ncdhw', 'channels_last'])
@pytest.mark.parametrize('C', [512, 768])
def test_veon_shapes_forward_and_backward(C, layout):
    low, occ, K = (8, 100, 100), (16, 200, 200), 18
    feat = volume(1, C, low, C, layout)
    table = make_table(K, C, 1)
    vox, lab = uniform_entries(occ, 40000, K, 2, dup=6)
    check_both(feat, vox, lab, table, occ, mixed_g(vox.shape[0], 3),
               what='VEON C=%d %s uniform' % (C, layout))
    vox, lab = slab_entries(occ, 40000, K, 4)
    check_both(feat, vox, lab, table, occ, mixed_g(vox.shape[0], 5),
               what='VEON C=%d %s slab' % (C, layout))


@pytest.mark.parametrize('low,occ', [((3, 7, 5), (6, 14, 10)), ((2, 5, 9), (4, 10, 18)),
                                     ((2, 5, 9), (5, 11, 20))])
@pytest.mark.parametrize('C', [512, 768, 24, 20, 1000, 130])
def test_odd_shapes(low, occ, C):
    """vector path (C % 4 == 0: channels-last as it is, other layouts through the
    per-sample copy), the scalar tail (C < 64 or C % 4 != 0; C = 130 takes its 32-chunk
    instantiation), B = 2 / batch = 1, and a non-2x grid (native forward, torch backward)"""
    K = 7
    table = make_table(K, C, 6)
    vox, lab = uniform_entries(occ, 300, K, 7, dup=3)
    g = mixed_g(vox.shape[0], 8)
    for layout in ('ncdhw', 'channels_last'):
        feat = volume(2, C, low, C + 1, layout)
        check_both(feat, vox, lab, table, occ, g, batch=1, what='odd C=%d %s' % (C, layout))
    # strided channels (neither layout) and a cropped view
    big = volume(2, 2 * C if C <= 512 else C, (low[0] + 2, low[1] + 2, low[2] + 2), 9, 'ncdhw')
    view = big[:, ::2 if C <= 512 else 1, 1:-1, 1:-1, 1:-1]
    check_both(view, vox, lab, table, occ, g, batch=0, what='odd C=%d strided view' % C)


def test_gradient_in_the_clamped_regime():
    """zeros and tiny features: the native gradient is autograd's (through the norm), not
    the derivative of the clamped expression; entries only there"""
    low, occ, C, K = (4, 6, 6), (8, 12, 12), 64, 5
    g0 = torch.Generator().manual_seed(11)
    feat = torch.randn((1, C) + low, generator=g0)
    feat[:, :, :2] = 0.0
    feat[:, :, 2] *= 1e-9
    feat = feat.to(DEV)
    table = make_table(K, C, 12)
    vox, lab = uniform_entries(occ, 500, K, 13, dup=2)
    g = mixed_g(vox.shape[0], 14)
    cos, grad = grad_of(lambda f: voxel_cosine(f, vox, lab, table, occ), feat, g)
    cos64, grad64 = grad_of(lambda f: sequence(f, vox, lab, table, occ), feat.double(), g)
    assert torch.isfinite(grad).all()
    # relative to the largest entry: the gradients reach |g| / eps here
    scale = float(grad64.abs().max())
    e_nat = float((grad.double() - grad64).abs().max())
    _, grad32 = grad_of(lambda f: sequence(f, vox, lab, table, occ, 0, torch.float32), feat, g)
    e_ref = float((grad32.double() - grad64).abs().max())
    floor = floor_of(feat, vox, lab, table, occ, g)
    print('clamped regime: max|grad| %.3e e_nat %.3e e_ref %.3e max floor %.3e'
          % (scale, e_nat, e_ref, float(floor.max())))
    assert scale > 1e3
    assert float(((grad.double() - grad64).abs() - floor).max()) <= 2 * e_ref
    assert float((cos.double() - cos64).abs().max()) <= ATOL


def test_bit_identical_over_launches_and_under_load():
    """No float atomics on the gradient: the same input gives the same bits in every
    launch, alone and beside another stream that keeps the chip busy."""
    low, occ, C, K = (8, 100, 100), (16, 200, 200), 512, 18
    feat = volume(1, C, low, 20, 'channels_last')
    table = make_table(K, C, 21)
    vox, lab = slab_entries(occ, 40000, K, 22)
    vox = torch.cat([vox, vox[:5000]])
    lab = torch.cat([lab, lab[5000:10000]])
    g = mixed_g(vox.shape[0], 23)
    cos0, grad0 = grad_of(lambda f: voxel_cosine(f, vox, lab, table, occ), feat, g)
    grad0 = grad0.clone()
    for _ in range(10):
        cos, grad = grad_of(lambda f: voxel_cosine(f, vox, lab, table, occ), feat, g)
        assert torch.equal(cos, cos0) and torch.equal(grad, grad0)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    for _ in range(5):
        with torch.cuda.stream(side):
            for _ in range(8):
                a = torch.tanh(a @ a * 1e-3)
        cos, grad = grad_of(lambda f: voxel_cosine(f, vox, lab, table, occ), feat, g)
        assert torch.equal(cos, cos0) and torch.equal(grad, grad0)
    torch.cuda.synchronize()
    # an entry list in another order: same voxels grouped differently, same sums per
    # voxel only up to the entry order -> not compared; the order is part of the input


def test_step_never_holds_the_upsampled_volume():
    """VEON-B, N = 40 000: forward + backward stay below the byte size of the upsampled
    volume (C * 16 * 200 * 200 * 4 = 1.31 GB, derived), which the reference formulation
    (upsample, then gather) on the same inputs exceeds."""
    low, occ, C, K = (8, 100, 100), (16, 200, 200), 512, 18
    volume_bytes = C * occ[0] * occ[1] * occ[2] * 4
    feat = volume(1, C, low, 30, 'ncdhw')
    table = make_table(K, C, 31)
    vox, lab = uniform_entries(occ, 40000, K, 32)
    vox, lab = vox[:40000].contiguous(), lab[:40000].contiguous()
    g = mixed_g(40000, 33)

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        leaf = feat.detach().clone().requires_grad_(True)
        fn(leaf).backward(g)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    native = peak_of(lambda f: voxel_cosine(f, vox, lab, table, occ))
    ref = peak_of(lambda f: sequence(f, vox, lab, table, occ, 0, torch.float32))
    print('align step peak allocation: native %.1f MB, upsample-then-gather %.1f MB '
          '(upsampled volume %.1f MB)' % (native / 1e6, ref / 1e6, volume_bytes / 1e6))
    assert native < volume_bytes
    assert ref > volume_bytes


def test_device_refusals_and_empty():
    low, occ, C = (2, 3, 4), (4, 6, 8), 16
    feat = volume(1, C, low, 40, 'ncdhw').requires_grad_(True)
    table = make_table(3, C, 41)
    ok_v = torch.tensor([[0, 0, 0]], dtype=torch.int32, device=DEV)
    ok_l = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        voxel_cosine(feat, torch.tensor([[8, 0, 0]], dtype=torch.int32, device=DEV), ok_l, table, occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v, ok_l + 3, table, occ)
    with pytest.raises(ValueError):
        voxel_cosine(feat, ok_v, ok_l, table.clone().requires_grad_(True), occ)
    with pytest.raises(ValueError):      # half features that require grad
        voxel_cosine(feat.detach().half().requires_grad_(True), ok_v, ok_l, table, occ)
    # the C ABI refuses a batch outside [0, B) and C > 1024 (status 1)
    import ctypes
    s5 = ctypes.c_int64 * 5
    st = ctypes.cast(s5(*feat.stride()), ctypes.c_void_p)
    buf = torch.empty(8, device=DEV)
    for Cbad, batch in ((C, 1), (2048, 0)):
        with pytest.raises(_lib.VeonHipError):
            _lib.launch('veon_occ_align_fwd', feat.device, feat.detach(), st, Cbad, 1, 2, 3, 4,
                        4, 6, 8, ok_v, ok_l, 1, batch, table, 3, EPS, buf, buf, buf)
    # an out-of-range entry that reaches the kernel reads nothing and gives zeros
    bad_v = torch.tensor([[5, 4, 2], [-1, 0, 0], [0, 6, 0]], dtype=torch.int32, device=DEV)
    bad_l = torch.tensor([0, 0, 0], dtype=torch.int32, device=DEV)
    cos = torch.full((3,), 7.0, device=DEV)
    stats = torch.full((3, 2), 7.0, device=DEV)
    _lib.launch('veon_occ_align_fwd', feat.device, feat.detach(), st, C, 1, 2, 3, 4, 4, 6, 8,
                bad_v, bad_l, 3, 0, table, 3, EPS, buf, cos, stats)
    assert cos[0] != 0 and not cos[1:].any() and not stats[1:].any()
    # N = 0: empty result, zero gradient
    cos = voxel_cosine(feat, ok_v[:0], ok_l[:0], table, occ)
    assert cos.shape == (0,)
    cos.sum().backward()
    assert feat.grad is not None and not feat.grad.any()


# ------------------------------------------------------------------ the mirrors

def _fixture(dtype, device):
    from tests.test_align_loss import fixture_inputs
    g = load_golden('align_loss_tiny')
    return g, fixture_inputs(g, dtype, device)


@pytest.mark.parametrize('case', ['open', 'mixed', 'stage2'])
def test_fixture_on_the_device(case):
    """The mirrors on the device with the native primitive underneath: the same entry
    counts, and losses and gradient by the rule of the module docstring with the CPU
    mirror in fp64 as the exact value (tests/test_align_loss.py pins it to the reference)
    and the RECORDED fp32 reference result as the yardstick.  Floors: a loss is a sum of
    N weighted (1 - cos_i), each cosine carrying (C + 8) roundings -> (N + C + 8) * 2^-24
    * sum w_i (1 + |cos_i|) <= ... * 2 sum w_i; the gradient's as for the primitive."""
    from tests.test_align_loss import run_case, selection
    g, inp64 = _fixture(torch.float64, 'cpu')
    out64, loss64, grad64, counts64 = run_case(g, inp64, case)
    sel64 = selection(loss64, inp64)
    _, inp = _fixture(torch.float32, DEV)
    n0 = dict(_lib.CALLS)
    out, loss, grad, counts = run_case(g, inp, case)
    assert _lib.CALLS.get('veon_occ_align_fwd', 0) > n0.get('veon_occ_align_fwd', 0)
    assert _lib.CALLS.get('veon_occ_align_bwd', 0) > n0.get('veon_occ_align_bwd', 0)
    assert np.array_equal(counts.numpy(), g[case + '_counts'])
    assert np.array_equal(counts64.numpy(), g[case + '_counts'])
    C = inp['feat_low'].shape[1]
    n_all = sum(int(s['voxels'].shape[0]) for s in sel64)
    w_all = sum(float(s['weights'].sum()) for s in sel64)
    floor_loss = (n_all + C + 8) * U * 2 * w_all
    for key, rec, weight in (('loss_featalign_det_c_0', case + '_loss_det', loss.loss_featalign_det_weight),
                             ('loss_featalign_soft_c_0', case + '_loss_soft', loss.loss_featalign_soft_weight)):
        assert (key in out) == (key in out64)
        if key not in out:
            continue
        exact = float(out64[key].detach()) / weight
        e_ref = abs(float(g[rec]) - exact)
        e_nat = abs(float(out[key].detach()) / weight - exact)
        print('%s %s: e_nat %.3e e_ref %.3e floor %.3e' % (case, key, e_nat, e_ref, floor_loss))
        assert e_nat <= 2 * e_ref + floor_loss, (key, e_nat, e_ref)
    e_ref = float(np.abs(g[case + '_grad'].astype(np.float64) - grad64.numpy()).max())
    e_nat = float((grad.double().cpu() - grad64).abs().max())
    floor = torch.zeros_like(grad64)
    for b, s in enumerate(sel64):
        if s['voxels'].shape[0]:
            floor += floor_of(inp64['feat_low'], s['voxels'], s['labels'], inp64['table'],
                              inp64['occ_size'], s['weights'], b)
    print('%s gradient: e_nat %.3e e_ref %.3e max floor %.3e max|grad| %.3e'
          % (case, e_nat, e_ref, float(floor.max()), float(grad64.abs().max())))
    assert float(((grad.double().cpu() - grad64).abs() - floor).max()) <= 2 * e_ref, (e_nat, e_ref)
    assert abs(float(out['loss_binocc_c_0'].detach()) - float(out64['loss_binocc_c_0'])) <= 1e-5


def test_path_occ_loss_backward_reaches_the_parameters(monkeypatch):
    """VeonOccupancyPath (the tiny configuration of tests/test_path_golden.py) with grad
    enabled, occ_loss of its output, backward: finite non-zero gradients on the sem
    head's and the body's first conv's parameters, equal by the module docstring's rule
    to those obtained with the torch sequence in place of the primitive.

    One forward, three alignment-loss tails on its feat_low: native, the torch fp32
    sequence, and the torch sequence in fp64 on the loss's own entries and weights (the
    exact value).  d loss / d feat_low: e_nat <= 2 e_ref + floor, floor element by element
    as for the primitive.  Parameters: the fp64 feature gradient is pushed through the
    SAME fp32 backward of the network to give the exact value p64, and e_nat <= 2 e_ref +
    floor again, e_ref that of the torch-sequence run.  The three parameter gradients are
    images of three feature gradients under one linear map, so what the floor has to
    cover is the map's own fp32 rounding when it is run three times: an entry of a weight
    gradient sums B z y x products, and the gradient it multiplies has come through
    27 C-term sums per conv on the way -> (B z y x + 27 C) * 2^-24 * max |p64|."""
    from tests.test_path_golden import _build, _inputs
    from tests.test_align_loss import selection
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=False)
    images, geom, metric = _inputs(g, DEV)
    gen = torch.Generator().manual_seed(50)
    C = net.ov_classifier_weight.shape[1]
    net.ov_classifier_weight = torch.nn.Parameter(torch.randn(25, C, generator=gen).to(DEV))
    _, inp = _fixture(torch.float32, DEV)
    B = images.shape[0]
    occ = tuple(net.occ_size)
    assert occ == inp['occ_size']
    inp = dict(inp, voxel_semantics=inp['voxel_semantics'][:B], mask_camera=inp['mask_camera'][:B],
               img_inputs=[t[:B] for t in inp['img_inputs']], sem_seg_ds=inp['sem_seg_ds'][:B],
               table=net.ov_classifier_weight.detach())
    loss = occ_loss_mod.OccLossFB(grid_config=inp['grid_config'], high_conf_thr=0.3, stage2_start=2,
                                  priority=inp['priority'], ov_class_number=8)
    loss.epoch = 3
    args = (inp['voxel_semantics'], inp['mask_camera'], inp['img_inputs'], inp['sem_seg_ds'],
            inp['class_reflection'], loss)
    params = dict(net.occ_decoder.feat_pred.named_parameters())
    params.update({'body0.' + k: v for k, v in net.occ_decoder.layers_3d_body[0].named_parameters()})
    names, plist = list(params), list(params.values())
    w_det, w_soft = loss.loss_featalign_det_weight, loss.loss_featalign_soft_weight

    with torch.enable_grad():
        out = net(images, geom, depth=metric, return_features=True)
        feat = out['feat_low']
        assert isinstance(feat, torch.Tensor) and feat.requires_grad and feat.dtype == torch.float32

        def tail():
            losses = net.occ_loss(out, *args)
            assert set(losses) == {'loss_binocc_c_0', 'loss_featalign_det_c_0',
                                   'loss_featalign_soft_c_0'}
            align = losses['loss_featalign_det_c_0'] + losses['loss_featalign_soft_c_0']
            grads = torch.autograd.grad(align, [feat] + plist, retain_graph=True)
            return losses, grads[0], grads[1:]

        n0 = dict(_lib.CALLS)
        losses, f_nat, p_nat = tail()
        assert _lib.CALLS.get('veon_occ_align_fwd', 0) > n0.get('veon_occ_align_fwd', 0)
        assert _lib.CALLS.get('veon_occ_align_bwd', 0) > n0.get('veon_occ_align_bwd', 0)
        n1 = dict(_lib.CALLS)
        monkeypatch.setattr(occ_loss_mod, 'voxel_cosine', align_loss._reference)
        _, f_ref, p_ref = tail()
        monkeypatch.undo()
        assert _lib.CALLS.get('veon_occ_align_fwd', 0) == n1.get('veon_occ_align_fwd', 0)

        # the exact tail: the loss's own entries and weights, the sequence in fp64
        sel = selection(loss, inp, feat.detach())
        assert sum(int(e['voxels'].shape[0]) for e in sel) > 0 and sel[0]['n_det'] > 0
        leaf = feat.detach().double().requires_grad_(True)
        total = leaf.new_zeros(())
        floor = torch.zeros_like(leaf)
        for b, e in enumerate(sel):
            wt = e['weights'].double().clone()
            wt[:e['n_det']] *= w_det
            wt[e['n_det']:] *= w_soft
            cos = sequence(leaf, e['voxels'], e['labels'], inp['table'], occ, b)
            total = total + (wt * (1 - cos)).sum()
            floor += floor_of(feat, e['voxels'], e['labels'], inp['table'], occ, wt, b)
        f64, = torch.autograd.grad(total, leaf)
        e_nat = float((f_nat.double() - f64).abs().max())
        e_ref = float((f_ref.double() - f64).abs().max())
        print('path d loss / d feat_low: e_nat %.3e e_ref %.3e max floor %.3e max|grad| %.3e'
              % (e_nat, e_ref, float(floor.max()), float(f64.abs().max())))
        assert float(((f_nat.double() - f64).abs() - floor).max()) <= 2 * e_ref, (e_nat, e_ref)

        p64 = torch.autograd.grad(feat, plist, grad_outputs=f64.float(), retain_graph=True)
        n_terms = feat.shape[0] * feat.shape[2] * feat.shape[3] * feat.shape[4] + 27 * feat.shape[1]
        for k, pn, pr, pe in zip(names, p_nat, p_ref, p64):
            assert torch.isfinite(pn).all() and pn.abs().max() > 0, k
            e_nat = float((pn - pe).abs().max())
            e_ref = float((pr - pe).abs().max())
            floor_p = n_terms * U * float(pe.abs().max())
            print('path %s: max|grad| %.3e e_nat %.3e e_ref %.3e floor %.3e'
                  % (k, float(pe.abs().max()), e_nat, e_ref, floor_p))
            assert e_nat <= 2 * e_ref + floor_p, (k, e_nat, e_ref, floor_p)

        # and the whole loss back-propagates into the parameters
        net.zero_grad(set_to_none=True)
        sum(losses.values()).backward()
    for k, prm in params.items():
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and prm.grad.abs().max() > 0, k


def test_path_feature_gradient_against_fp64():
    """d (alignment loss) / d feat_low at the path's own feat_low, native against the
    fp64 sequence, yardstick the fp32 sequence (module docstring)."""
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=False)
    images, geom, metric = _inputs(g, DEV)
    with torch.enable_grad():
        feat = net(images, geom, depth=metric, return_features=True)['feat_low'].detach()
    assert isinstance(feat, torch.Tensor) and feat.dtype == torch.float32
    occ = tuple(net.occ_size)
    K = 9
    table = make_table(K, feat.shape[1], 60)
    vox, lab = uniform_entries(occ, 600, K, 61, dup=3)
    check_both(feat, vox, lab, table, occ, mixed_g(vox.shape[0], 62), what='path_tiny feat_low')
