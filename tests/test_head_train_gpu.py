"""GPU checks of the prediction heads' native training path
(``_PredHead3D.hip_train``) and of its hand-over kernels (csrc/volume_handover.hip).

Heads and decoder tail: e = relative L2 error against the same step in fp64;
e(native) <= 2 e(autocast), the project's rule, with the yardstick the same modules with
the switches off under ``torch.autocast`` in the flavour's dtype.  Every numeric test
prints its figures (run with -s) and has an fp16 twin."""
import copy
import types

import pytest
import torch

from tests.helpers import flavour, fp16_twin, roundoff, to_half  # noqa: F401
from veon_amd import _lib, conv3d_ops, half
from veon_amd.align_loss import voxel_cosine
from veon_amd.models.semantic_net.align_net_body import (PredHead3DOcc, PredHead3DSem,
                                                          ResBlock3D, _PredHead3D)
from veon_amd.occ_bin_loss import bin_occ_loss

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = (2, 256, 2, 3, 5)          # 2 * 4 * 5 * 7 = 280 padded rows: not a tile multiple


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    _PredHead3D.hip_train = False
    ResBlock3D.hip_train = False


def _rel(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300)).item()


# --------------------------------------------------------------- hand-over kernels
def _random_volume(B, C, Z, Y, X, seed):
    g = torch.Generator().manual_seed(seed)
    vol = conv3d_ops.PaddedVolume(B, C, Z, Y, X, DEV)
    vol.interior().copy_(torch.randn(B, Z, Y, X, C, generator=g).to(DEV))
    return vol


@pytest.mark.parametrize('C,Cp', [(64, 64), (2, 8)])
def test_unpack_cl_is_the_interior(C, Cp, flavour):
    vol = _random_volume(2, Cp, 2, 3, 5, seed=C)
    got = conv3d_ops.unpack_cl(vol, C)
    assert got.is_contiguous() and got.dtype == torch.float32
    assert torch.equal(got, vol.interior().float()[..., :C])
    assert got.permute(0, 4, 1, 2, 3).stride(1) == 1


test_unpack_cl_is_the_interior_fp16 = fp16_twin(test_unpack_cl_is_the_interior)


@pytest.mark.parametrize('layout', ['contiguous', 'voxel_cosine'])
def test_sigm_bwd_pack_cl_against_fp64(layout, flavour):
    """d pre = g (0.25 - f^2) within one rounding of the flavour (2 roundoff |ref|, plus
    2^-22 |ref| for the fp32 arithmetic ahead of it); every row of a NaN-filled
    destination written, halo and guard rows exactly zero."""
    B, C, Z, Y, X = 2, 64, 2, 3, 5
    gen = torch.Generator().manual_seed(5)
    f = conv3d_ops.PaddedVolume(B, C, Z, Y, X, DEV)
    f.interior().copy_((torch.sigmoid(2 * torch.randn(B, Z, Y, X, C, generator=gen)) - 0.5).to(DEV))
    if layout == 'contiguous':
        g = torch.randn(B, Z, Y, X, C, generator=gen).to(DEV).permute(0, 4, 1, 2, 3)
    else:
        # what voxel_cosine's backward returns for sample 1 of 2: the batch's
        # channels-last buffer, zero outside the sample
        feat = (f.interior().float().permute(0, 4, 1, 2, 3)).requires_grad_(True)
        vox = torch.stack([torch.randint(0, n, (40,), generator=gen)
                           for n in (2 * X, 2 * Y, 2 * Z)], 1).int().to(DEV)
        lab = torch.randint(0, 5, (40,), generator=gen).int().to(DEV)
        table = torch.randn(5, C, generator=gen).to(DEV)
        cos = voxel_cosine(feat, vox, lab, table, (2 * Z, 2 * Y, 2 * X), batch=1)
        g, = torch.autograd.grad(cos.sum(), feat)
        assert g.stride(1) == 1 and float(g[0].abs().sum()) == 0 and float(g[1].abs().sum()) > 0
    out = conv3d_ops.PaddedVolume.from_storage(
        torch.full_like(f.storage, float('nan')), f.shape)
    got = conv3d_ops.sigm_bwd_pack_cl(g, f, out=out)
    assert got is out and bool(torch.isfinite(out.storage.float()).all())
    fi = f.interior().double()
    ref = g.permute(0, 2, 3, 4, 1).double() * (0.25 - fi * fi)
    diff = (out.interior().double() - ref).abs()
    bound = (2 * roundoff() + 2.0 ** -22) * ref.abs()
    # half the spacing of the format's subnormals: the rounding of a result below its
    # smallest normal number (2^-25 in fp16, nothing to speak of in bf16)
    tiny = torch.finfo(half.dtype()).tiny * torch.finfo(half.dtype()).eps / 2
    print('largest |diff| / |ref| %.3e (bound %.3e)'
          % (float((diff / ref.abs().clamp_min(2.0 ** -14)).max()), 2 * roundoff() + 2.0 ** -22))
    assert bool((diff <= bound + tiny).all())
    halo = out.rows.view(B, Z + 2, Y + 2, X + 2, C).clone()
    halo[:, 1:-1, 1:-1, 1:-1] = 0
    assert float(halo.float().abs().sum()) == 0.0
    assert float(out.storage[:out.guard].float().abs().sum()) == 0.0
    assert float(out.storage[out.guard + out.M:].float().abs().sum()) == 0.0


test_sigm_bwd_pack_cl_against_fp64_fp16 = fp16_twin(test_sigm_bwd_pack_cl_against_fp64)


# --------------------------------------------------------------------------- heads
def _init(mod, seed):
    torch.manual_seed(seed)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
        if isinstance(m, torch.nn.Conv3d):
            m.weight.data = to_half(m.weight.data)
            if m.bias is not None:
                m.bias.data.normal_(0, 0.5)
    return mod.train()


def _step(mod, x, G, how, fn=None):
    """One forward + backward of a copy of ``mod``: {name: tensor} of the output, the
    input gradient, every parameter gradient and every buffer afterwards."""
    mod = copy.deepcopy(mod)
    _PredHead3D.hip_train = ResBlock3D.hip_train = how == 'native'
    if how == 'fp64':
        mod, x, G = mod.double().cpu(), x.double().cpu(), G.double().cpu()
    else:
        mod = mod.to(DEV)
    x = x.clone().requires_grad_(True)
    call = fn or (lambda m, t: m(t))
    if how == 'autocast':
        with torch.autocast('cuda', dtype=half.dtype()):
            out = call(mod, x)
    else:
        out = call(mod, x)
    out.backward(G.to(out.dtype).to(out.device))
    _PredHead3D.hip_train = ResBlock3D.hip_train = False
    res = {'out': out.detach(), 'dx': x.grad}
    res.update({'grad:' + k: p.grad for k, p in mod.named_parameters()})
    res.update({'buf:' + k: b.detach() for k, b in mod.named_buffers()})
    return res


def _compare(exact, nat, auto):
    assert set(nat) == set(exact) == set(auto)
    worst = []
    for k in sorted(exact):
        want = exact[k].to(DEV)
        assert nat[k] is not None and nat[k].shape == want.shape, k
        if not want.is_floating_point():
            assert torch.equal(nat[k].to(DEV), want), k
            continue
        assert bool(torch.isfinite(nat[k]).all()), k
        e_n, e_a = _rel(nat[k].to(DEV), want), _rel(auto[k].to(DEV), want)
        print('%-40s e(native) %.3e  e(autocast) %.3e' % (k, e_n, e_a))
        worst.append((e_n / max(e_a, 1e-30), k))
        assert e_n <= 2 * e_a, (k, e_n, e_a)
    print('largest e(native) / e(autocast): %.2f at %s' % max(worst))


@pytest.mark.parametrize('which', ['occ', 'sem'])
def test_heads_match_the_module_definition(which, flavour):
    head = _init(PredHead3DOcc(256, 2) if which == 'occ' else PredHead3DSem(256, 64), 3)
    gen = torch.Generator().manual_seed(7)
    x = to_half(torch.randn(*GRID, generator=gen).relu()).to(DEV)
    G = torch.randn(GRID[0], 2 if which == 'occ' else 64, *GRID[2:], generator=gen).to(DEV)
    exact = _step(head, x, G, 'fp64')
    before = dict(_lib.CALLS)
    nat = _step(head, x, G, 'native')
    for name in ('veon_linear_wgrad_bf16', 'veon_bn3d_sums_bf16'):
        assert _lib.CALLS.get(name, 0) > before.get(name, 0), name
    auto = _step(head, x, G, 'autocast')
    _compare(exact, nat, auto)
    if which == 'sem':
        bias_grad = nat['grad:occ_conv1.conv.bias']
        assert torch.equal(bias_grad, torch.zeros_like(bias_grad))
        assert nat['out'].stride(1) == 1                      # voxel_cosine's vector path
        assert _lib.CALLS.get('veon_volume_sigm_bwd_pack_cl', 0) > \
            before.get('veon_volume_sigm_bwd_pack_cl', 0)


test_heads_match_the_module_definition_fp16 = fp16_twin(test_heads_match_the_module_definition)


def test_sem_head_stores_a_zero_halo(flavour):
    _PredHead3D.hip_train = True
    head = _init(PredHead3DSem(256, 64), 4).to(DEV)
    x = torch.randn(*GRID, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    out = head(x)
    assert type(out.grad_fn).__name__ == '_SigmTailFnBackward'
    _, fs, _ = out.grad_fn.saved_tensors
    B, _, Z, Y, X = GRID
    f = conv3d_ops.PaddedVolume.from_storage(fs, (B, 64, Z, Y, X))
    halo = f.rows.view(B, Z + 2, Y + 2, X + 2, 64).clone()
    assert torch.equal(halo[:, 1:-1, 1:-1, 1:-1].float(), out.detach().permute(0, 2, 3, 4, 1))
    halo[:, 1:-1, 1:-1, 1:-1] = 0
    assert float(halo.float().abs().sum()) == 0.0
    assert float(fs[:f.guard].float().abs().sum()) == 0.0
    assert float(fs[f.guard + f.M:].float().abs().sum()) == 0.0


test_sem_head_stores_a_zero_halo_fp16 = fp16_twin(test_sem_head_stores_a_zero_halo)


# -------------------------------------------------------------------- decoder tail
def _decoder():
    """``AlignNetOcc3D`` with two ResBlock3D(256) and both heads; its own ``forward`` runs,
    with the lift in front of the body replaced by the test's volume (``fuse`` of block 0)."""
    from veon_amd.models.semantic_net.align_net_occ3d import AlignNetOcc3D
    dec = AlignNetOcc3D(clip_dim=8, hsa_dim=8, embed_dim=256, clip_outdim=64,
                        layer_lifting_map=['0->0->0'], fusion_type='add_fusion',
                        layer_depth=2)
    dec.lss_view_transformer = types.SimpleNamespace(mode='lifted')
    dec.prepare_depth = lambda depth: depth
    return dec


def _decode(dec, x):
    dec.fuse = lambda idx, cur, *a, **k: x if idx == 0 else cur
    shape = x.new_zeros(1, 1, 2, 2)
    out = dec(shape, [shape, shape], [shape], None, [])
    return out['bin_occ'], out['feat_occ']


def _tail_loss(entries):
    vox, lab, table, labels, cw, occ = entries

    def fn(mod, x):
        bin_low, feat = _decode(mod, x)
        dev = feat.device
        bin_low, feat = bin_low.to(x.dtype), feat.to(x.dtype)     # autocast hands halves over
        total = bin_occ_loss(bin_low, labels.to(dev), cw.to(dev).to(x.dtype), occ)
        for b in range(feat.shape[0]):
            cos = voxel_cosine(feat, vox.to(dev), lab.to(dev), table.to(dev).to(x.dtype), occ,
                               batch=b)
            total = total + (1 - cos).mean().to(total.dtype)
        return total
    return fn


def test_decoder_tail_matches_the_module_definition(flavour, monkeypatch):
    tail = _init(_decoder(), 5)
    gen = torch.Generator().manual_seed(9)
    B, _, Z, Y, X = GRID
    occ = (2 * Z, 2 * Y, 2 * X)
    x = to_half(torch.randn(*GRID, generator=gen).relu()).to(DEV)
    vox = torch.stack([torch.randint(0, n, (50,), generator=gen) for n in occ[::-1]], 1).int()
    lab = torch.randint(0, 6, (50,), generator=gen).int()
    table = torch.randn(6, 64, generator=gen)
    labels = torch.tensor([0, 5, 16, 17, 17, 200, 255])[
        torch.randint(0, 7, (B, 2 * X, 2 * Y, 2 * Z), generator=gen)].to(torch.uint8)
    fn = _tail_loss((vox, lab, table, labels, torch.tensor([1.0, 0.5]), occ))
    G = torch.tensor(1.0)
    exact = _step(tail, x, G, 'fp64', fn)

    calls = []
    pack, unpack = conv3d_ops.pack, conv3d_ops.unpack
    monkeypatch.setattr(conv3d_ops, 'pack',
                        lambda t, *a, **k: (calls.append(('pack', t.shape[1])), pack(t, *a, **k))[1])
    monkeypatch.setattr(conv3d_ops, 'unpack',
                        lambda v, *a, **k: (calls.append(('unpack', v.shape[1])),
                                            unpack(v, *a, **k))[1])
    before = dict(_lib.CALLS)
    nat = _step(tail, x, G, 'native', fn)
    monkeypatch.undo()
    print('pack / unpack calls of the native step:', calls)
    # forward: the input is packed once; the only unpack is the 8-channel occupancy volume
    # (no unpack -> pack pair between the body and the heads).  backward: its pack, and the
    # unpack of the input gradient
    assert calls == [('pack', 256), ('unpack', 8), ('pack', 8), ('unpack', 256)]
    for name in ('veon_occ_bin_loss_fwd', 'veon_occ_bin_loss_bwd', 'veon_occ_align_bwd',
                 'veon_volume_sigm_bwd_pack_cl', 'veon_volume_unpack_cl_f32',
                 'veon_conv3d_k3_wgrad_bf16'):
        assert _lib.CALLS.get(name, 0) > before.get(name, 0), name
    auto = _step(tail, x, G, 'autocast', fn)
    keep = ('out', 'dx')
    _compare({k: exact[k] for k in keep}, {k: nat[k] for k in keep}, {k: auto[k] for k in keep})


test_decoder_tail_matches_the_module_definition_fp16 = fp16_twin(
    test_decoder_tail_matches_the_module_definition)


def test_forward_features_is_forward_without_the_inference_tail(monkeypatch):
    """``forward_features`` hands the decoder exactly what ``forward(...,
    return_features=True)`` hands it under grad, returns the decoder's own output tensors,
    and never enters ``_classify``.  The decoder's arguments are compared bit for bit; its
    outputs are not compared across the two calls, because under autograd the tiny path's
    lift adds its points with atomics, so two runs of ``forward`` itself need not agree in
    the last bits."""
    from tests.conftest import load_golden
    from tests.test_path_golden import _build, _inputs
    g = load_golden('path_tiny')
    net = _build(g, DEV, native=False)
    images, geom, metric = _inputs(g, DEV)
    dec = net.occ_decoder
    seen, classified = [], []
    inner, classify = dec.forward, net._classify

    def decoder(*args):
        out = inner(*args)
        seen.append((args, out))
        return out
    monkeypatch.setattr(dec, 'forward', decoder)
    monkeypatch.setattr(net, '_classify',
                        lambda *a, **k: (classified.append(1), classify(*a, **k))[1])
    with torch.enable_grad():
        full = net(images, geom, depth=metric, return_features=True)
        assert len(seen) == 1 and len(classified) == 1
        feats = net.forward_features(images, geom, depth=metric)
    assert len(seen) == 2 and len(classified) == 1            # no inference tail
    assert set(feats) == {'feat_low', 'bin_low'}
    (args_a, out_a), (args_b, out_b) = seen
    assert full['feat_low'] is out_a['feat_occ'] and full['bin_low'] is out_a['bin_occ']
    assert feats['feat_low'] is out_b['feat_occ'] and feats['bin_low'] is out_b['bin_occ']

    def same(a, b, where):
        if torch.is_tensor(a):
            assert torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b), where
        elif isinstance(a, dict):
            assert a.keys() == b.keys(), where
            for k in a:
                same(a[k], b[k], '%s[%r]' % (where, k))
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), where
            for i, (u, v) in enumerate(zip(a, b)):
                same(u, v, '%s[%d]' % (where, i))
        else:
            assert a == b, where
    same(args_a, args_b, 'decoder argument')
    for k in feats:
        assert isinstance(feats[k], torch.Tensor) and feats[k].requires_grad, k
        assert feats[k].shape == full[k].shape and feats[k].dtype == full[k].dtype, k
