"""CPU checks of the native occupancy term's Python side (veon_amd/occ_bin_loss.py): the
torch sequence against today's ``OccLossFB.loss_voxel`` and the reference's recorded value,
the gather formulation of the native backward against fp64 autograd, the host-only
argument checks of the entry points, the ``OccLossFB(hip_train=...)`` switch, the header."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import load_golden
from tests.test_align_loss import CASES, build_loss, fixture_inputs
from veon_amd import _lib
from veon_amd.models.semantic_net.occ_loss import BCE_BinOcc_Loss, OccLossFB
from veon_amd.occ_bin_loss import bin_occ_loss, bin_occ_loss_bwd_ref, bin_occ_loss_torch

ENTRY_POINTS = ('veon_occ_bin_loss_workspace_bytes', 'veon_occ_bin_loss_fwd',
                'veon_occ_bin_loss_bwd')


def make_case(B, low, seed, dtype=torch.float64, big=True):
    """Logits with a few +-80 entries and labels over the whole range of a uint8: the
    classes, free (17), 18..254 (free as well) and ignored (255)."""
    g = torch.Generator().manual_seed(seed)
    z, y, x = low
    logits = torch.randn((B, 2, z, y, x), generator=g, dtype=torch.float64) * 3
    if big:
        flat = logits.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 12)]
        flat[idx] = torch.tensor([80.0, -80.0])[torch.arange(idx.numel()) % 2].double()
    pool = torch.tensor([0, 3, 16, 17, 17, 18, 200, 254, 255, 255])
    labels = pool[torch.randint(0, pool.numel(), (B, 2 * x, 2 * y, 2 * z), generator=g)]
    return logits.to(dtype), labels.to(torch.uint8), torch.tensor([1.0, 0.5])


def autograd_fp64(logits, labels, cw, occ, **kw):
    leaf = logits.double().clone().requires_grad_(True)
    loss = bin_occ_loss_torch(leaf, labels, cw.double(), occ, **kw)
    grad, = torch.autograd.grad(loss, leaf)
    return loss.detach(), grad


def test_header_declares_and_libraries_export_the_entry_points():
    from veon_amd import build
    build.build()
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    ptr, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib._SIGNATURES['veon_occ_bin_loss_workspace_bytes'] == (i64, [i] * 4)
    assert _lib._SIGNATURES['veon_occ_bin_loss_fwd'] == (
        i, [ptr, ptr] + [i] * 7 + [ptr, ptr, i, i, ptr, ptr, i64, ptr, ptr])
    assert _lib._SIGNATURES['veon_occ_bin_loss_bwd'] == (i, [ptr] * 3 + [i] * 4 + [ptr, ptr])
    for flavour, path in _lib.LIB_PATHS.items():
        lib = ctypes.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), (flavour, name)
        lib.veon_abi_version.restype = ctypes.c_int
        assert lib.veon_abi_version() == 2      # the additions are additive


def test_workspace_and_bad_arguments_on_the_host():
    """The checks that run before any launch (no device needed)."""
    lib = _lib.lib()
    assert lib.veon_occ_bin_loss_workspace_bytes(1, 16, 200, 200) == 2500 * 16
    assert lib.veon_occ_bin_loss_workspace_bytes(2, 2, 4, 6) == 16
    assert lib.veon_occ_bin_loss_workspace_bytes(0, 2, 4, 6) == -1
    assert lib.veon_occ_bin_loss_workspace_bytes(1, 2048, 2048, 2048) == -1
    bad = 1                                      # VEON_ERR_BAD_ARG
    st = (ctypes.c_int64 * 5)(16, 8, 4, 2, 1)
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    sp = ctypes.cast(st, ctypes.c_void_p)
    fwd, bwd = lib.veon_occ_bin_loss_fwd, lib.veon_occ_bin_loss_bwd
    assert fwd(None, sp, 1, 1, 1, 1, 2, 2, 2, p, p, 255, 17, p, p, 16, p, None) == bad
    assert fwd(p, None, 1, 1, 1, 1, 2, 2, 2, p, p, 255, 17, p, p, 16, p, None) == bad
    assert fwd(p, sp, 1, 0, 1, 1, 2, 2, 2, p, p, 255, 17, p, p, 16, p, None) == bad
    assert fwd(p, sp, 1, 1, 1, 1, 2, 0, 2, p, p, 255, 17, p, p, 16, p, None) == bad
    neg = (ctypes.c_int64 * 5)(16, 8, -4, 2, 1)
    assert fwd(p, ctypes.cast(neg, ctypes.c_void_p), 1, 1, 1, 1, 2, 2, 2, p, p, 255, 17, p, p,
               16, p, None) == bad
    assert fwd(p, sp, 1, 1, 1, 1, 2, 2, 2, p, p, 255, 17, p, p, 8, p, None) == 3   # workspace
    assert bwd(None, p, p, 1, 1, 1, 1, p, None) == bad
    assert bwd(p, p, p, 1, 0, 1, 1, p, None) == bad
    assert bwd(p, p, p, 1, 1, 1, (1 << 20) + 1, p, None) == bad
    assert bwd(p, p, p, 64, 1024, 1024, 1024, p, None) == bad


def test_torch_sequence_is_todays_loss_voxel_term_and_the_references_value():
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, torch.float32)
    loss = build_loss(g, inp, 'mixed')
    labels = loss.masked_labels(inp['voxel_semantics'], inp['mask_camera'])
    # the lines of OccLossFB.loss_voxel, verbatim
    bin_up = F.interpolate(inp['bin_low'].float(), size=inp['occ_size'], mode='trilinear',
                           align_corners=False).permute(0, 1, 4, 3, 2)
    today = BCE_BinOcc_Loss(bin_up, labels, loss.bin_class_weights.to(bin_up),
                            ignore_index=loss.ignore_idx)
    got = bin_occ_loss_torch(inp['bin_low'], labels, loss.bin_class_weights, inp['occ_size'],
                             ignore_index=loss.ignore_idx)
    assert torch.equal(got, today)
    assert abs(float(got) - float(g['loss_binocc'])) <= 1e-5
    # the public entry takes the same path on CPU tensors
    assert torch.equal(bin_occ_loss(inp['bin_low'], labels, loss.bin_class_weights,
                                    inp['occ_size']), today)


@pytest.mark.parametrize('B,low', [(1, (1, 1, 1)), (2, (1, 2, 3)), (2, (3, 5, 4)),
                                   (2, (2, 2, 2))])
def test_gather_formulation_matches_fp64_autograd(B, low):
    logits, labels, cw = make_case(B, low, seed=sum(low) + B)
    occ = tuple(2 * v for v in low)
    want_loss, want = autograd_fp64(logits, labels, cw, occ)
    loss, grad = bin_occ_loss_bwd_ref(logits, labels, cw, occ)
    scale = float(want.abs().max())
    assert scale > 0
    print('loss diff %.3e  grad diff / max %.3e' % (abs(float(loss - want_loss)),
                                                    float((grad - want).abs().max()) / scale))
    assert abs(float(loss - want_loss)) <= 1e-12 * max(1.0, abs(float(want_loss)))
    assert float((grad - want).abs().max()) <= 1e-12 * scale
    assert torch.equal(grad[:, 1], -grad[:, 0])
    # an upstream gradient scales it
    _, g3 = bin_occ_loss_bwd_ref(logits, labels, cw, occ, grad_out=3.0)
    assert float((g3 - 3 * want).abs().max()) <= 3e-12 * scale


def test_all_labels_ignored_gives_nan_and_a_zero_gradient():
    logits, labels, cw = make_case(2, (2, 3, 2), seed=5)
    labels = torch.full_like(labels, 255)
    occ = (4, 6, 4)
    want_loss, want = autograd_fp64(logits, labels, cw, occ)
    loss, grad = bin_occ_loss_bwd_ref(logits, labels, cw, occ)
    assert torch.isnan(want_loss) and torch.isnan(loss)
    assert torch.equal(want, torch.zeros_like(want)) and torch.equal(grad, torch.zeros_like(grad))


def test_labels_18_to_254_count_as_free():
    logits, labels, cw = make_case(1, (2, 2, 3), seed=9, big=False)
    occ = (4, 4, 6)
    odd = torch.randint(18, 255, labels.shape, generator=torch.Generator().manual_seed(1))
    keep = labels == 255
    a = torch.where(keep, labels, odd.to(torch.uint8))
    b = torch.where(keep, labels, torch.full_like(labels, 17))
    for fn in (lambda l: bin_occ_loss_bwd_ref(logits, l, cw, occ),
               lambda l: autograd_fp64(logits, l, cw, occ)):
        (la, ga), (lb, gb) = fn(a), fn(b)
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    # another split point moves the classes with it
    l3, _ = bin_occ_loss_bwd_ref(logits, labels, cw, occ, free_index=3)
    w3, _ = autograd_fp64(logits, labels, cw, occ, free_index=3)
    assert abs(float(l3 - w3)) <= 1e-12


def test_int64_labels_and_refusals():
    logits, labels, cw = make_case(1, (1, 2, 2), seed=2)
    occ = (2, 4, 4)
    assert torch.equal(bin_occ_loss_torch(logits, labels.long(), cw, occ),
                       bin_occ_loss_torch(logits, labels, cw, occ))
    with pytest.raises(ValueError):
        bin_occ_loss_torch(logits, labels.float(), cw, occ)
    with pytest.raises(ValueError):
        bin_occ_loss_torch(logits, labels, cw, (2, 4, 5))
    with pytest.raises(ValueError):
        bin_occ_loss_torch(logits[:, :1], labels, cw, occ)
    with pytest.raises(ValueError):          # the gather formulation is the 2x stencil
        bin_occ_loss_bwd_ref(logits, labels[:, :3, :3, :1], cw, (1, 3, 3))


@pytest.mark.parametrize('case', CASES)
def test_switch_changes_nothing_on_the_cpu(case):
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, torch.float32)
    outs = []
    for on in (False, True):
        loss = build_loss(g, inp, case)
        assert loss.hip_train is False
        loss.hip_train = on
        results = dict(feat_occ=inp['feat_low'], bin_occ=inp['bin_low'],
                       occ_size=inp['occ_size'], sem_seg_ds=inp['sem_seg_ds'],
                       class_reflection=inp['class_reflection'],
                       ov_classifier_weight=inp['table'])
        outs.append(loss(inp['voxel_semantics'], inp['mask_camera'], results,
                         inp['img_inputs']))
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_switch_is_a_keyword_and_adds_no_state():
    kw = dict(grid_config=None, priority=[1.0] * 17)
    on, off = OccLossFB(hip_train=True, **kw), OccLossFB(**kw)
    assert on.hip_train is True and off.hip_train is False
    assert list(on.state_dict()) == list(off.state_dict())
    assert np.array_equal(on.bin_class_weights.numpy(), [1.0, 0.5])
