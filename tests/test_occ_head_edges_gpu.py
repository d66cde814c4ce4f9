"""The fused tail of the occupancy path (csrc/occ_tail.hip) at its edges, against the
float64 reference ``tests/edge_refs.occ_tail_ref`` (pinned on the CPU by
tests/test_edge_refs.py).  The kernel is fp32 and independent of the half flavour.

Values.  The kernel evaluates a depth-3 nest of fp32 multiplies and adds on fp32
lambdas that the reference shares (the library is built with contraction off, so the
source index is the plain scale*(dst+0.5)-0.5), hence
    |got - ref| <= 8 * 2^-24 * blend(|logits|)        element-wise.
Labels.  A label may differ from the reference only where the fp64 top-2 margin of the
class logits, or |o0 - o1|, is at most twice that bound ("undecided"); the share of
such voxels stays below 1e-3 in every case.  Each test prints its largest err/bound
ratio and its undecided share (run with -s).
"""
import pytest
import torch

from tests import edge_refs as er
from veon_amd import conv3d_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _check_values(tag, got, ref, mag):
    ratio = ((got.cpu().double() - ref).abs() / (er.VALUE_BOUND * mag))
    ratio = torch.nan_to_num(ratio, nan=0.0)      # 0 / 0: both exactly zero
    print('%s: max err/bound %.3f' % (tag, ratio.max().item()))
    assert bool((got.cpu().double() - ref).abs().le(er.VALUE_BOUND * mag).all()), \
        (tag, ratio.max().item())


def _check_labels(tag, occ, r, Q):
    occ = occ.cpu()
    und = r.undecided()
    share = und.double().mean().item()
    differ = (occ != r.labels).permute(0, 3, 2, 1)
    print('%s: undecided share %.2e, labels differing %d (all undecided: %s)'
          % (tag, share, int(differ.sum()), not bool((differ & ~und).any())))
    assert share < er.UNDECIDED_CAP, (tag, share)
    assert not bool((differ & ~und).any()), (tag, int((differ & ~und).sum()))
    assert int(occ.min()) >= 0 and int(occ.max()) <= Q


def _channels_last(x, row=None, shift=0):
    """(B,Q,z,y,x) -> the same values as a channels-last slice of rows of ``row``
    floats (default 4*ceil(Q/4): 16-byte rows), starting ``shift`` floats into a
    16-byte-aligned buffer; the surplus floats are NaN."""
    B, Q, z, y, xx = x.shape
    row = row or (Q + 3) // 4 * 4
    buf = torch.full((B * z * y * xx * row + 4,), float('nan'), device=x.device)
    rows = buf[shift:shift + B * z * y * xx * row].view(B, z, y, xx, row)
    rows[..., :Q] = x.permute(0, 2, 3, 4, 1)
    return rows[..., :Q].permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize('name', sorted(er.OCC_CASES))
def test_tail_against_the_float64_reference(name):
    """Both instantiations and the scalar fall-back on the same data: bit-equal to each
    other, inside the value bound, labels equal outside the undecided set."""
    sem_low, bin_low, size = er.occ_inputs(name)
    Q = sem_low.shape[1]
    r = er.occ_tail_ref(sem_low, bin_low, size)
    sem_d, bin_d = sem_low.to(DEV), bin_low.to(DEV)
    vec = _channels_last(sem_d)
    assert vec.stride(1) == 1 and vec.data_ptr() % 16 == 0 and vec.stride(4) % 4 == 0
    odd_row = _channels_last(sem_d, row=(Q + 3) // 4 * 4 + 1)      # row stride % 4 != 0
    off_base = _channels_last(sem_d, shift=1)                      # base 4 bytes off
    assert odd_row.stride(4) % 4 == 1 and off_base.data_ptr() % 16 == 4
    outs = {'scalar': conv3d_ops.occ_classify(sem_d.contiguous(), bin_d, size),
            'vec4': conv3d_ops.occ_classify(vec, bin_d, size),
            'odd row': conv3d_ops.occ_classify(odd_row, bin_d, size),
            'shifted base': conv3d_ops.occ_classify(off_base, bin_d, size)}
    sem, binv, occ = outs['scalar']
    for key, (s, b, o) in outs.items():
        assert torch.equal(s, sem) and torch.equal(b, binv) and torch.equal(o, occ), key
    assert occ.shape == r.labels.shape and occ.dtype == torch.int64
    _check_values(name + ' sem', sem, r.sem, r.sem_abs)
    _check_values(name + ' bin', binv, r.bin, r.bin_abs)
    _check_labels(name, occ, r, Q)
    if tuple(size) == tuple(sem_low.shape[2:]):          # l1 = 0: a copy, bit for bit
        assert torch.equal(sem.cpu(), sem_low) and torch.equal(binv.cpu(), bin_low)


def test_strided_occupancy_logits():
    """The occupancy logits as a channel slice of a transposed volume (the form the path
    hands over), next to a contiguous copy: bit-equal."""
    sem_low, bin_low, size = er.occ_inputs('q17')
    B, _, z, y, x = bin_low.shape
    wide = torch.full((B, z, 8, y, x), float('nan'), device=DEV)
    wide[:, :, :2] = bin_low.to(DEV).transpose(1, 2)
    strided = wide.transpose(1, 2)[:, :2]
    assert not strided.is_contiguous()
    a = conv3d_ops.occ_classify(sem_low.to(DEV), strided, size)
    b = conv3d_ops.occ_classify(sem_low.to(DEV), bin_low.to(DEV), size)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('form', ['scalar', 'vec4'])
def test_integer_logits_are_exact(form):
    """Integer logits in [-4, 4] at a 2x ratio: every product and sum is exact in fp32,
    so values equal the float64 reference exactly and so does every label -- the first
    of tied maxima wins, o0 == o1 is free."""
    sem_low, bin_low, size = er.occ_integer_inputs()
    Q = sem_low.shape[1]
    r = er.occ_tail_ref(sem_low, bin_low, size)
    sem_d = sem_low.to(DEV)
    sem, binv, occ = conv3d_ops.occ_classify(
        _channels_last(sem_d) if form == 'vec4' else sem_d, bin_low.to(DEV), size)
    assert torch.equal(sem.cpu().double(), r.sem) and torch.equal(binv.cpu().double(), r.bin)
    tied = r.sem_margin == 0
    free = r.bin_margin == 0
    print('integer logits: %.2f %% tied maxima, %.2f %% o0 == o1'
          % (100 * tied.double().mean().item(), 100 * free.double().mean().item()))
    assert tied.double().mean().item() > 0.01 and bool(free.any())
    assert bool((tied & ~free & (r.bin[:, 0] > r.bin[:, 1])).any())   # tied AND labelled
    assert torch.equal(occ.cpu(), r.labels)
    assert bool((occ.cpu().permute(0, 3, 2, 1)[free] == Q).all())


@pytest.mark.parametrize('form', ['scalar', 'vec4'])
def test_special_values(form):
    """NaN, +inf and -inf hand-placed in the class and occupancy logits: at every output
    voxel whose corner set touches one, labels and the non-finite pattern of the volumes
    equal ATen's own op sequence (fp32, CPU); finite entries stay inside the bound."""
    sem_low, bin_low, size, mask = er.occ_special_inputs()
    Q = sem_low.shape[1]
    touch = er.corner_touch(mask, size)
    rs, rb, ro = er.aten_tail(sem_low, bin_low, size)
    r = er.occ_tail_ref(sem_low, bin_low, size)
    sem_d = sem_low.to(DEV)
    sem, binv, occ = conv3d_ops.occ_classify(
        _channels_last(sem_d) if form == 'vec4' else sem_d, bin_low.to(DEV), size)
    sem, binv, occ = sem.cpu(), binv.cpu(), occ.cpu()
    assert int(occ.min()) >= 0 and int(occ.max()) <= Q
    lab_touch = touch.permute(0, 3, 2, 1)
    assert torch.equal(occ[lab_touch], ro[lab_touch])
    for tag, got, want, ref, mag in (('sem', sem, rs, r.sem, r.sem_abs),
                                     ('bin', binv, rb, r.bin, r.bin_abs)):
        fin = torch.isfinite(want)
        assert bool((~fin).any())
        # NaN where ATen has NaN, the same infinity where it has one
        torch.testing.assert_close(got[~fin], want[~fin], rtol=0, atol=0, equal_nan=True)
        err = (got.double() - ref).abs()[fin]
        bound = (er.VALUE_BOUND * mag)[fin]
        print('special %s (%s): max err/bound %.3f on %d finite entries, %d non-finite'
              % (tag, form, torch.nan_to_num(err / bound).max().item(), int(fin.sum()),
                 int((~fin).sum())))
        assert bool((err <= bound).all())
    # away from the special values: the ordinary label rule
    und = r.undecided()
    differ = (occ != r.labels).permute(0, 3, 2, 1)
    assert not bool((differ & ~und & ~touch).any())
