"""GPU checks of the native occupancy term (csrc/occ_bin_loss.hip) against the torch
sequence evaluated in fp64: every logit layout, several workgroups, +-80 logits, both
label dtypes, the NaN-filled gradient buffer, bit-reproducibility, the non-2x fallback of
the backward, the all-ignored case, the reference's recorded value, graph capture, and the
``OccLossFB(hip_train=True)`` switch on the alignment fixture.

Bounds: |loss diff| <= 1e-5 and largest gradient |diff| <= 1e-5 of the largest |gradient|,
both against fp64 (the fp32 torch sequence itself is within 1e-7 / 2e-7 at these shapes)."""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_align_loss import CASES, build_loss, fixture_inputs
from tests.test_occ_bin_loss import autograd_fp64, make_case
from veon_amd import _lib, occ_bin_loss
from veon_amd.occ_bin_loss import bin_occ_loss, bin_occ_loss_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, (1, 1, 1)), (2, (1, 2, 3)), (2, (3, 5, 4)), (1, (4, 33, 17))]
LAYOUTS = ('contiguous', 'channels_last', 'two_of_eight')


def lay_out(logits, layout):
    """The same values in the layout the heads hand over."""
    if layout == 'channels_last':
        v = logits.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        assert v.stride(1) == 1
        return v
    if layout == 'two_of_eight':
        B, _, z, y, x = logits.shape
        wide = torch.full((B, z, y, x, 8), float('nan'), dtype=logits.dtype,
                          device=logits.device)
        wide[..., :2] = logits.permute(0, 2, 3, 4, 1)
        return wide.permute(0, 4, 1, 2, 3)[:, :2]
    return logits.contiguous()


def native(logits, labels, cw, occ, **kw):
    leaf = logits.detach().requires_grad_(True)
    n0 = _lib.CALLS.get('veon_occ_bin_loss_fwd', 0)
    loss = bin_occ_loss(leaf, labels, cw, occ, **kw)
    assert _lib.CALLS.get('veon_occ_bin_loss_fwd', 0) == n0 + 1
    grad, = torch.autograd.grad(loss, leaf)
    return loss.detach(), grad


def check(loss, grad, want_loss, want, tag):
    scale = float(want.abs().max())
    dl = abs(float(loss) - float(want_loss))
    dg = float((grad.double() - want).abs().max())
    print('%s: loss diff %.3e  grad diff / max %.3e' % (tag, dl, dg / scale))
    assert dl <= 1e-5
    assert dg <= 1e-5 * scale
    assert torch.equal(grad[:, 1], -grad[:, 0])


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('B,low', SHAPES)
def test_matches_fp64_torch(B, low, layout):
    logits, labels, cw = make_case(B, low, seed=sum(low) + B)
    occ = tuple(2 * v for v in low)
    want_loss, want = autograd_fp64(logits.to(DEV), labels.to(DEV), cw.to(DEV), occ)
    x = lay_out(logits.float().to(DEV), layout)
    n0 = _lib.CALLS.get('veon_occ_bin_loss_bwd', 0)
    loss, grad = native(x, labels.to(DEV), cw.to(DEV), occ)
    assert _lib.CALLS.get('veon_occ_bin_loss_bwd', 0) == n0 + 1      # the native backward
    assert grad.shape == x.shape and grad.dtype == torch.float32
    check(loss, grad, want_loss, want, '%s %s %s' % (B, low, layout))
    # int64 labels: cast on the device, the same bits
    loss64, grad64 = native(x, labels.long().to(DEV), cw.to(DEV), occ)
    assert torch.equal(loss64, loss) and torch.equal(grad64, grad)
    # a second run gives the same bits
    again = native(x, labels.to(DEV), cw.to(DEV), occ)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grad)


def test_every_gradient_element_is_stored():
    B, low = 2, (3, 5, 4)
    logits, labels, cw = make_case(B, low, seed=3)
    occ = tuple(2 * v for v in low)
    x = logits.float().to(DEV)
    coef, out = occ_bin_loss.loss_forward(x, labels.to(DEV), cw.to(DEV), occ)
    buf = torch.full((B, 2) + low, float('nan'), device=DEV)
    g = torch.tensor(1.0, device=DEV)
    got = occ_bin_loss.loss_backward(coef, out, g, (B,) + low, grad=buf)
    assert got is buf and bool(torch.isfinite(buf).all())
    _, want = autograd_fp64(logits.to(DEV), labels.to(DEV), cw.to(DEV), occ)
    assert float((buf.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # the coefficients of ignored voxels are zero
    assert bool((coef[labels.to(DEV) == 255] == 0).all())


def test_other_scales_native_forward_torch_backward():
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(2, 2, 2, 3, 3, generator=g, dtype=torch.float64) * 3
    occ = (5, 7, 4)
    labels = torch.randint(0, 19, (2, 4, 7, 5), generator=g).to(torch.uint8)
    labels[0, 0, :3] = 255
    cw = torch.tensor([1.0, 0.5])
    want_loss, want = autograd_fp64(logits.to(DEV), labels.to(DEV), cw.to(DEV), occ)
    n0 = _lib.CALLS.get('veon_occ_bin_loss_bwd', 0)
    loss, grad = native(logits.float().to(DEV), labels.to(DEV), cw.to(DEV), occ)
    assert _lib.CALLS.get('veon_occ_bin_loss_bwd', 0) == n0           # torch took the backward
    scale = float(want.abs().max())
    assert abs(float(loss) - float(want_loss)) <= 1e-5
    assert float((grad.double() - want).abs().max()) <= 1e-5 * scale


def test_all_labels_ignored():
    logits, labels, cw = make_case(2, (2, 3, 2), seed=5)
    labels = torch.full_like(labels, 255)
    loss, grad = native(logits.float().to(DEV), labels.to(DEV), cw.to(DEV), (4, 6, 4))
    assert bool(torch.isnan(loss))
    assert torch.equal(grad, torch.zeros_like(grad))


def test_the_references_recorded_value():
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, torch.float32, DEV)
    loss = build_loss(g, inp, 'mixed')
    labels = loss.masked_labels(inp['voxel_semantics'], inp['mask_camera'])
    got = bin_occ_loss(inp['bin_low'], labels, loss.bin_class_weights, inp['occ_size'])
    assert abs(float(got) - float(g['loss_binocc'])) <= 1e-5


def test_graph_capture_forward_and_backward():
    """forward + backward captured in one graph on one side stream; the replay follows new
    logits and labels in place and equals eager bit for bit: nothing reads the device back"""
    B, low = 1, (4, 33, 17)
    occ = tuple(2 * v for v in low)
    first = make_case(B, low, seed=11)
    second = make_case(B, low, seed=12)
    logits = first[0].float().to(DEV).requires_grad_(True)
    labels = first[1].long().to(DEV)              # the cast to uint8 is captured too
    cw = first[2].to(DEV)
    gout = torch.tensor(1.5, device=DEV)

    def step_fn():
        loss = bin_occ_loss(logits, labels, cw, occ)
        grad, = torch.autograd.grad(loss, logits, gout)
        return loss, grad

    def eager():
        return [t.detach().clone() for t in step_fn()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step_fn()                                                  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    want = eager()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        held = step_fn()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, want))
    with torch.no_grad():
        logits.copy_(second[0])
        labels.copy_(second[1])
        gout.fill_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in held]
    new = eager()
    assert not torch.equal(new[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(got, new))


@pytest.mark.parametrize('case', CASES)
def test_occ_loss_fb_switch(case):
    g = load_golden('align_loss_tiny')
    inp = fixture_inputs(g, torch.float32, DEV)
    outs = []
    for on in (False, True):
        loss = build_loss(g, inp, case)
        loss.hip_train = on
        bin_low = inp['bin_low'].clone().requires_grad_(True)
        results = dict(feat_occ=inp['feat_low'], bin_occ=bin_low, occ_size=inp['occ_size'],
                       sem_seg_ds=inp['sem_seg_ds'], class_reflection=inp['class_reflection'],
                       ov_classifier_weight=inp['table'])
        n0 = _lib.CALLS.get('veon_occ_bin_loss_fwd', 0)
        out = loss(inp['voxel_semantics'], inp['mask_camera'], results, inp['img_inputs'])
        assert _lib.CALLS.get('veon_occ_bin_loss_fwd', 0) == n0 + (1 if on else 0)
        grad, = torch.autograd.grad(out['loss_binocc_c_0'], bin_low)
        outs.append((out, grad))
    (off, g_off), (on, g_on) = outs
    assert off.keys() == on.keys()
    for k in off:
        print(k, float(off[k]), float(on[k]))
        assert abs(float(off[k]) - float(on[k])) <= 1e-5, k
    scale = float(g_off.abs().max())
    assert float((g_on - g_off).abs().max()) <= 1e-5 * scale
