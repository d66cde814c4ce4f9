"""Host side of the seam table of the shared weight-gradient body (tests/wgrad_seams.py):
the plan rule written out in Python against the three ``*_wgrad_workspace_bytes`` entry
points, and the premises that make each row of the table a seam.  No GPU.
"""
import pytest

from tests import wgrad_seams as ws
from veon_amd import conv3d_ops, vit_ops


def _library_bytes(kind, shape):
    if kind == 'linear':
        return vit_ops.linear_wgrad_workspace_bytes(*shape)
    B, Cin, Cout, *spatial = shape
    entry = conv3d_ops.wgrad2d_workspace_bytes if kind == 'conv2d' else \
        conv3d_ops.wgrad_workspace_bytes
    return entry(B, *spatial, Cin, Cout)


@pytest.mark.parametrize('kind,shape', ws.SHAPES, ids=ws.IDS)
def test_workspace_is_split_slabs_of_the_plan_rule(kind, shape):
    M, Cin, Cout = ws.dims(kind, shape)
    p = ws.plan_of(kind, shape)
    assert _library_bytes(kind, shape) == p['split'] * Cout * ws.TAPS[kind] * Cin * 4


@pytest.mark.parametrize('kind,shape,premises', ws.TABLE, ids=ws.IDS)
def test_premises_of_the_table(kind, shape, premises):
    M, Cin, Cout = ws.dims(kind, shape)
    facts = dict(ws.plan_of(kind, shape), M=M, tail=M % ws.WBK)
    for key, want in premises.items():
        assert facts[key] == want, (key, facts[key], want)
    assert sum(facts['slabs']) == facts['nsteps'] and min(facts['slabs']) >= 1
    assert facts['split'] == 1 or facts['tiles'] * facts['split'] <= ws.CUS
    # every product of integers in [-4, 4] summed over the rows stays an exact fp32 integer
    assert 16 * M < 2 ** 24


def test_the_table_reaches_every_seam():
    facts = [dict(ws.plan_of(k, s), kind=k, tail=ws.dims(k, s)[0] % ws.WBK) for k, s in ws.SHAPES]
    assert {f['tail'] for f in facts if f['kind'] == 'linear'} >= {0, 1, 63}
    assert max(f['split'] for f in facts) > 2
    assert any(len(set(f['slabs'])) > 1 for f in facts)              # an uneven last split
    assert any(f['split'] < f['first'] for f in facts)               # a recomputed split
    assert any(f['tiles'] > ws.CUS for f in facts)                   # more tiles than CUs
    for kind in ws.GROUPS:                  # a wide tile with nco != nci in each instantiation
        assert any(f['kind'] == kind and f['tile'] == 128 and f['nco'] != f['nci'] for f in facts)
    # the first M at which the split turns on, and the one before it
    assert ws.plan(960, 64, 64, 1)['split'] == 1 and ws.plan(961, 64, 64, 1)['split'] == 2


@pytest.mark.parametrize('kind,shape,M,workgroups', ws.WORKLOADS)
def test_the_workloads_fill_one_round_of_the_cus(kind, shape, M, workgroups):
    assert ws.dims(kind, shape)[0] == M
    p = ws.plan_of(kind, shape)
    assert p['tiles'] * p['split'] == workgroups <= ws.CUS
    Cin, Cout = shape[1:3]
    assert _library_bytes(kind, shape) == p['split'] * Cout * ws.TAPS[kind] * Cin * 4
