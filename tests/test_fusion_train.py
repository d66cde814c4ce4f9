"""CPU side of the native training of the lift's 2-D fusion (csrc/fusion_train.hip, DESIGN
section 4s): the fp64 references of tests/fusion_train_refs.py against torch's own bilinear
filter, the adjoint tables the kernels read, the switch's fallback, and the header."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fusion_train_refs as refs
from veon_amd import _lib, fusion_ops
from veon_amd.models.semantic_net.fusion_layers import CatFusionLift

NEW_SYMBOLS = ('veon_fusion_resize_cat', 'veon_fusion_resize_adjoint', 'veon_fusion_dual_ln',
               'veon_fusion_dual_ln_bwd', 'veon_fusion_dual_ln_bwd_workspace_bytes',
               'veon_fusion_join', 'veon_fusion_relu_split')
AXES = sorted({(i, o) for s1, s2, s in refs.MAP_CASES for src in (s1, s2)
               for i, o in zip(src, s)} | {(64, 32), (176, 88), (16, 32), (44, 88)})


@pytest.mark.parametrize('case', range(len(refs.MAP_CASES)))
def test_mirror_on_fp32_tables_matches_torch_interpolate(case):
    """The fp64 blend with the fp32 tables against F.interpolate(bilinear,
    align_corners=False) in fp32 on the CPU, elementwise within 8 * 2^-24 * sum_taps w |x|
    (four products and three additions in fp32, doubled for the order); an index off by one
    misses this by orders of magnitude.  Largest error seen: 1.97 x 2^-24 of that sum."""
    s1, s2, size = refs.MAP_CASES[case]
    g = torch.Generator().manual_seed(case)
    worst = 0.0
    for s in (s1, s2):
        x = torch.randn(2, 5, *s, generator=g) * 1.5 + 0.3
        want = x if s == size else F.interpolate(x, size=size, mode='bilinear',
                                                 align_corners=False)
        got = refs.resize(x, size)
        bound = 8 * 2.0 ** -24 * refs.resize(x, size, absolute=True)
        err = (got - want.double()).abs()
        worst = max(worst, float((err / refs.resize(x, size, absolute=True)).max()) * 2 ** 24)
        assert got.shape == want.shape
        assert bool((err <= bound).all()), float((err / bound).max())
    print('case %d: largest error %.2f x 2^-24 sum w|x|' % (case, worst))


@pytest.mark.parametrize('n_in,n_out', AXES)
def test_adjoint_tables_are_consistent(n_in, n_out):
    """Scattering with (i0, i1, l1) equals gathering over [first, last) exactly on
    integer-valued data (weights replaced by the integers 1 and 2, so every sum is exact),
    the library's forward tables equal the references' to the bit, and no destination
    outside a source's range reads it."""
    t = fusion_ops.axis_table(n_in, n_out)
    i0, i1, l0, l1 = refs.axis(n_in, n_out)
    assert np.array_equal(t['i0'], i0) and np.array_equal(t['i1'], i1)
    assert t['l1'].dtype == np.float32 and np.array_equal(t['l1'], l1)
    assert 0 <= t['i0'].min() and t['i1'].max() <= n_in - 1
    assert np.all(np.diff(t['i0']) >= 0)
    d = np.random.RandomState(n_in * 131 + n_out).randint(-9, 10, size=n_out).astype(np.int64)
    scatter = np.zeros(n_in, dtype=np.int64)
    np.add.at(scatter, t['i0'], 1 * d)
    np.add.at(scatter, t['i1'], 2 * d)
    gather = np.zeros(n_in, dtype=np.int64)
    for s in range(n_in):
        assert 0 <= t['first'][s] <= t['last'][s] <= n_out
        for dd in range(t['first'][s], t['last'][s]):
            gather[s] += (1 * d[dd] if t['i0'][dd] == s else 0) + \
                         (2 * d[dd] if t['i1'][dd] == s else 0)
    assert np.array_equal(scatter, gather)


def test_closed_form_backward_agrees_with_fp64_autograd_of_the_mirror():
    """The closed forms of the references (LayerNorm backward, adjoint matrices) against
    fp64 autograd of the mirror sequence with torch's own interpolate: relative L2 below
    1e-6 (the two differ only by torch computing the filter weights in fp64, 2^-24
    relative)."""
    s1, s2, size = refs.MAP_CASES[0]
    g = torch.Generator().manual_seed(3)
    C1, C2, N = 8, 12, 2
    x1 = torch.randn(N, C1, *s1, generator=g)
    x2 = torch.randn(N, C2, *s2, generator=g)
    M = N * size[0] * size[1]
    d1, d2 = torch.randn(M, C1 + C2, generator=g), torch.randn(M, C2, generator=g)
    g1, g2 = torch.rand(C1 + C2, generator=g) + 0.5, torch.rand(C2, generator=g) + 0.5
    rc = refs.resize_cat(x1, x2, size)
    drc, dg1, db1, dg2, db2 = refs.dual_layernorm_bwd(d1, d2, rc, C1, g1, 1e-6, g2, 1e-6)
    got = dict(drc=drc, dg1=dg1, db1=db1, dg2=dg2, db2=db2,
               dx1=refs.resize_adjoint(refs.maps(drc[:, :C1], N, *size), x1.shape),
               dx2=refs.resize_adjoint(refs.maps(drc[:, C1:], N, *size), x2.shape))
    want = refs.mirror_backward(x1, x2, size, d1, d2, g1, 1e-6, g2, 1e-6, torch.float64, 'cpu')
    for k in want:
        rel = float((got[k] - want[k]).norm() / want[k].norm())
        assert rel < 1e-6, (k, rel)


def test_switch_on_cpu_tensors_falls_back_bit_for_bit():
    torch.manual_seed(0)
    mod = CatFusionLift(64, 64, 64).train()
    x1 = torch.randn(2, 64, 8, 22)
    x2 = torch.randn(2, 64, 2, 6)
    G = torch.randn(2, 64, 4, 11)

    def step(on):
        m = copy.deepcopy(mod)
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        CatFusionLift.hip_train = on
        try:
            out = m(a, b, (4, 11))
            out.backward(G)
        finally:
            CatFusionLift.hip_train = False
        return [out.detach(), a.grad, b.grad] + [p.grad for p in m.parameters()]
    before = dict(_lib.CALLS)
    off, on = step(False), step(True)
    assert _lib.CALLS == before
    assert len(on) == 11
    for u, v in zip(off, on):
        assert v is not None and torch.equal(u, v)
    assert CatFusionLift.hip_train is False


def test_header_declares_the_new_symbols():
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
