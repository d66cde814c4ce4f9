"""Host side of the seam table of the two-stage column sums (tests/reduce_seams.py): the
premises that make each row of the table a seam, asserted against the plans mirrored
there, and the block caps and refusals of the library's own ``*_workspace_bytes`` entry
points, which load without a GPU.  No GPU.
"""
import pytest

from tests import reduce_seams as rs
from veon_amd import _lib

ENTRY = {'bn': 'veon_bn3d_sums_workspace_bytes',
         'colsum': 'veon_rows_colsum_workspace_bytes',
         'ln_tokens': 'veon_layernorm_f32_bwd_workspace_bytes',
         'ln_image': 'veon_image_layernorm_bwd_workspace_bytes'}


def _library_bytes(kind, width):
    return int(getattr(_lib.lib(), ENTRY[kind])(width))


@pytest.mark.parametrize('kind,shape,premises', rs.TABLE, ids=rs.IDS)
def test_premises_of_the_table(kind, shape, premises):
    facts = rs.plan_of(kind, shape)
    if 'interior' in premises:
        facts['interior'] = rs.interior_rows(kind, shape)
    if 'live_blocks' in premises:
        facts['live_blocks'] = rs.live_blocks(kind, shape)
    assert premises, 'a row without a premise pins nothing'
    for key, want in premises.items():
        assert facts[key] == want, (key, facts[key], want)
    M, rows, nb = facts['M'], facts['rows'], facts['nblocks']
    assert (nb - 1) * rows < M <= nb * rows and 1 <= facts['last'] <= rows
    assert nb <= rs.CAP[kind] and rows >= facts['minimum']
    assert facts['capped'] == (rows > facts['minimum'])
    # integers in [-4, 4], and their products with |xhat| <= 12 in the BN backward sums,
    # summed over the rows stay exact fp32 integers
    assert 48 * M < 2 ** 24
    live = rs.live_rows(kind, shape)
    assert live and 0 <= live[0] and live[-1] < M
    assert len(live) <= 9


@pytest.mark.parametrize('kind,shape', rs.SHAPES, ids=rs.IDS)
def test_workspace_is_cap_partials(kind, shape):
    """cap * sums * C * 4 bytes with caps 512, 512, 1024, 1024 and 2, 1, 2, 3 sums per
    channel: the plans' ``nblocks`` never exceeds what the library allocates."""
    assert (rs.CAP, rs.SUMS) == ({'bn': 512, 'colsum': 512, 'ln_tokens': 1024, 'ln_image': 1024},
                                 {'bn': 2, 'colsum': 1, 'ln_tokens': 2, 'ln_image': 3})
    C = rs.channels(kind, shape)
    assert _library_bytes(kind, C) == rs.CAP[kind] * rs.SUMS[kind] * C * 4


ACCEPTED = {'bn': lambda C: C > 0 and C % 8 == 0 and C <= 2048,
            'colsum': lambda N: N > 0 and N % 8 == 0,
            'ln_tokens': lambda d: d > 0 and d % 64 == 0 and d <= 1024,
            'ln_image': lambda C: C > 0 and C % 8 == 0 and C <= 1024}
WIDTHS = [-8, 0, 1, 4, 7, 8, 9, 12, 24, 63, 64, 65, 72, 128, 136, 512, 520, 576, 1024, 1032,
          1088, 2040, 2048, 2056, 4096]


@pytest.mark.parametrize('kind', sorted(ENTRY))
def test_refusals(kind):
    """-1 outside the accepted widths, the full workspace inside:
      bn         C a multiple of 8, at most 2048 (``bn_shape_ok``); refused widths surface
                 as VeonHipError in ``conv3d_ops._bn_workspace`` (bn_sums, bn_bwd_sums);
      colsum     N a multiple of 8, no upper bound; ``vit_ops.colsum``;
      ln_tokens  d a multiple of 64, at most 1024 (``ln_width_ok``);
                 ``vit_ops.layernorm_f32_bwd``;
      ln_image   C a multiple of 8, at most 1024 (``ln_shape_ok``);
                 ``conv3d_ops.image_layernorm_bwd``."""
    for w in WIDTHS:
        got = _library_bytes(kind, w)
        if ACCEPTED[kind](w):
            assert got == rs.CAP[kind] * rs.SUMS[kind] * w * 4, (kind, w, got)
        else:
            assert got == -1, (kind, w, got)
    # every width of the table is an accepted one
    for shape in rs.shapes_of(kind):
        assert ACCEPTED[kind](rs.channels(kind, shape))


def test_the_table_reaches_every_seam():
    facts = {kind: [rs.plan_of(kind, s) for s in rs.shapes_of(kind)] for kind in rs.PLANS}
    for kind, fs in facts.items():
        if kind != 'ln_image':        # the smallest padded image has 9 rows: two blocks
            assert any(f['nblocks'] == 1 and f['last'] < f['rows'] for f in fs), kind
        assert any(f['nblocks'] == 2 for f in fs), kind
        assert any(f['nblocks'] > 64 for f in fs), kind       # stage two: a second round
        # off the minimum with a count of rows that the in-flight stride does not divide
        assert any(f['capped'] and f['rows'] % f['stride'] for f in fs), kind
        assert any(f['last'] % f['stride'] for f in fs), kind
        # exactly on the cap with the minimum rows: the last shape before the plan changes
        assert any(f['nblocks'] == rs.CAP[kind] and not f['capped'] for f in fs), kind
    assert {f['idle'] for f in facts['bn']} >= {0, 1, 4, 127}
    assert {f['rpb'] for f in facts['bn']} >= {1, 256}
    assert {f['chunks'] for f in facts['colsum']} >= {1, 64, 65}
    for kind in ('ln_tokens', 'ln_image'):
        assert {f['N'] for f in facts[kind]} == {1, 2}
        assert any(f['N'] == 1 and f['chunks'] == 64 for f in facts[kind])
        assert any(f['N'] == 2 and 0 < f['second'] < 64 for f in facts[kind])
        assert any(f['second'] == 64 for f in facts[kind])
    # the first M at which each plan leaves its minimum, and the one before it
    assert not rs.colsum_plan(8192, 64)['capped'] and rs.colsum_plan(8193, 64)['capped']
    assert not rs.ln_tokens_plan(8192, 64)['capped'] and rs.ln_tokens_plan(8193, 64)['capped']
    assert not rs.ln_image_plan(2, 64, 62, 62)['capped']
    assert not rs.bn_plan(1, 64, 2, 126, 126)['capped']
    for kind, shape in rs.STALE:
        assert (kind, shape) in rs.SHAPES
    for kind in rs.PLANS:
        assert {rs.plan_of(k, s)['capped'] for k, s in rs.STALE if k == kind} == {True, False}


def test_live_rows_cover_the_block_edges():
    """The rows of the one-live-row tests: both ends of block 0, the first row of block 1,
    the last row of the last block, and five rows of a middle block where the cap binds."""
    assert rs.live_rows('ln_tokens', (9, 64)) == [0, 7, 8]
    assert rs.live_rows('ln_tokens', (8193, 64)) == [0, 8, 9, 4095, 4096, 4097, 4098, 4103, 8192]
    assert rs.live_rows('ln_tokens', (7, 64)) == [0, 6]
    assert rs.live_rows('ln_image', (1, 8, 1, 1)) == [4]
    assert rs.live_rows('ln_image', (3, 8, 1, 1)) == [4, 22]
    assert rs.live_rows('bn', (1, 72, 2, 3, 4)) == [0, 111, 112, 119]
    # with a zero halo the second block of most 'bn' rows adds nothing: the GPU tests also
    # fill every padded row, and one row of the table has interior rows in both blocks
    assert rs.live_blocks('bn', (1, 8, 3, 13, 14)) == [0]
    assert rs.live_blocks('bn', (1, 72, 2, 3, 4)) == [0]
    for kind, shape in rs.SHAPES:
        if kind == 'ln_image':
            assert set(rs.live_rows(kind, shape)) <= set(rs.interior_rows(kind, shape))
