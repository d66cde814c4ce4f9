"""The seam table of the two-stage column sums of the BatchNorm and LayerNorm passes
(csrc/conv3d_train.hip, csrc/linear_train.hip, csrc/conv2d_train.hip, csrc/ln_common.h;
DESIGN sections 4k - 4m), shared by tests/test_reduce_seams.py (CPU: the table's premises
against the plans below and the library's workspace sizes) and
tests/test_reduce_seams_gpu.py.  A plain module: no fixtures, no GPU, nothing of the code
under test.

Stage one: a workgroup walks ``rows`` rows and writes a partial; stage two adds the
partials in a fixed order.  The host picks ``rows = max(ceil(M / cap), minimum)`` and
``nblocks = ceil(M / rows)``.  The caps (512, 512, 1024, 1024) are what the library's
``*_workspace_bytes`` entry points report, and the CPU test pins them there; the minimum
rounds (4 rpb, 16, 8, 8) are NOT exported by the library: they are copied from the host
code of ``bn_sums_impl``, ``veon_rows_colsum_bf16``, ``veon_layernorm_f32_bwd`` and
``veon_image_layernorm_bwd_bf16``.
"""
import bisect
import functools

CAP = {'bn': 512, 'colsum': 512, 'ln_tokens': 1024, 'ln_image': 1024}
SUMS = {'bn': 2, 'colsum': 1, 'ln_tokens': 2, 'ln_image': 3}     # sums per channel
WAVES = 4                       # the wave stride of the three wave-per-row walks


def _cdiv(a, b):
    return -(-a // b)


def _blocks(M, cap, minimum):
    rows = max(_cdiv(M, cap), minimum)
    nblocks = _cdiv(M, rows)
    return {'M': M, 'rows': rows, 'nblocks': nblocks, 'last': M - (nblocks - 1) * rows,
            'minimum': minimum, 'capped': rows > minimum}


def bn_plan(B, C, Z, Y, X):
    """``bn_sums_impl``: one lane = 8 channels of a row, rpb rows in flight, the threads
    past lpr rpb idle; at least four rounds of rows per workgroup."""
    lpr = C // 8
    rpb = 256 // lpr
    p = _blocks(B * (Z + 2) * (Y + 2) * (X + 2), CAP['bn'], 4 * rpb)
    p.update(lpr=lpr, rpb=rpb, idle=256 - lpr * rpb, stride=rpb, N=1)
    return p


def colsum_plan(M, N):
    """``veon_rows_colsum_bf16``: grid.x workgroups of 64 16-byte chunks each."""
    p = _blocks(M, CAP['colsum'], 16)
    chunks = N // 8
    p.update(chunks=chunks, xblocks=_cdiv(chunks, 64), idle=_cdiv(chunks, 64) * 64 - chunks,
             stride=WAVES, N=1)
    return p


def _ln(M, C, kind):
    p = _blocks(M, CAP[kind], 8)
    chunks = C // 8
    n = 1 if C <= 512 else 2
    p.update(chunks=chunks, N=n, idle=64 - min(chunks, 64), second=max(chunks - 64, 0),
             stride=WAVES)
    return p


def ln_tokens_plan(T, d):
    """``veon_layernorm_f32_bwd``: one wave per row; 'second': lanes with a second chunk."""
    return _ln(T, d, 'ln_tokens')


def ln_image_plan(B, C, Y, X):
    """``veon_image_layernorm_bwd_bf16``: the same walk over the PADDED rows."""
    return _ln(B * (Y + 2) * (X + 2), C, 'ln_image')


PLANS = {'bn': bn_plan, 'colsum': colsum_plan, 'ln_tokens': ln_tokens_plan,
         'ln_image': ln_image_plan}


def plan_of(kind, shape):
    return PLANS[kind](*shape)


def channels(kind, shape):
    return shape[1]


@functools.lru_cache(maxsize=None)
def interior_rows(kind, shape):
    """The padded-row indices of the interior voxels / pixels of a 'bn' or 'ln_image'
    shape, ascending."""
    B, C, *spatial = shape
    rows = range(B)
    for v in spatial:
        rows = [r * (v + 2) + i for r in rows for i in range(1, v + 1)]
    return rows


def live_blocks(kind, shape):
    """The blocks of the plan that hold at least one interior row of a padded grid."""
    rows = plan_of(kind, shape)['rows']
    return sorted({m // rows for m in interior_rows(kind, shape)})


def live_rows(kind, shape):
    """The rows of the plan at which the one-live-row tests put their row: the first and
    the last row of block 0, the first row of block 1, the last row of the last block,
    and for a capped shape the rows r0 + 0..3 and the last row of a middle block.  Images:
    the nearest interior padded row of each (the lower one of two equally near), since the
    image kernel skips halo rows.  The BatchNorm sums walk every padded row alike, so
    their live row may be a halo row and sits on the block edge itself.  Ascending,
    without repeats."""
    p = plan_of(kind, shape)
    M, rows, nb = p['M'], p['rows'], p['nblocks']
    want = [0, min(rows, M) - 1, M - 1]
    if nb > 1:
        want.append(rows)
    if p['capped']:
        r0 = (nb // 2) * rows
        want += [r0, r0 + 1, r0 + 2, r0 + 3, r0 + rows - 1]
    if kind == 'ln_image':
        inner = interior_rows(kind, shape)

        def nearest(r):
            i = bisect.bisect_left(inner, r)
            near = inner[max(i - 1, 0):i + 1]
            return min(near, key=lambda m: (abs(m - r), m))
        want = [nearest(r) for r in want]
    return sorted(set(want))


# (kind, shape, premises): bn (B, C, Z, Y, X); colsum (M, N); ln_tokens (T, d); ln_image
# (B, C, Y, X).  Premises are facts of the plan that make the row a seam; the CPU test
# asserts each, so a later change of a plan or of the table cannot silently turn a seam
# case into an ordinary one.  'last': rows of the last block; 'idle': threads (bn) or lanes
# without a chunk; 'second': lanes that hold a second chunk (N = 2).
TABLE = [
    # one lane per row: thread 0 alone adds 256 row-lanes, most of them idle (27 rows)
    ('bn', (1, 8, 1, 1, 1), {'M': 27, 'lpr': 1, 'rpb': 256, 'nblocks': 1, 'last': 27}),
    ('bn', (1, 8, 3, 13, 14), {'M': 1200, 'rows': 1024, 'nblocks': 2, 'last': 176,
                               'rpb': 256}),
    # the same with one more plane: block 1 holds interior rows (above, its 176 rows are
    # the last halo plane and add zeros)
    ('bn', (1, 8, 4, 13, 14), {'M': 1440, 'nblocks': 2, 'last': 416, 'live_blocks': [0, 1]}),
    ('bn', (1, 24, 1, 2, 3), {'lpr': 3, 'rpb': 85, 'idle': 1}),
    ('bn', (1, 72, 2, 3, 4), {'M': 120, 'lpr': 9, 'rpb': 28, 'idle': 4, 'rows': 112,
                              'nblocks': 2, 'last': 8}),
    ('bn', (1, 1032, 1, 2, 3), {'lpr': 129, 'rpb': 1, 'idle': 127, 'rows': 4,
                                'nblocks': 15}),
    ('bn', (1, 2048, 1, 1, 2), {'lpr': 256, 'rpb': 1, 'idle': 0, 'nblocks': 9}),
    # the cap binds
    ('bn', (1, 2048, 1, 11, 51), {'M': 2067, 'capped': True, 'rows': 5, 'nblocks': 414,
                                  'last': 2}),
    # stage two beyond 64 partials; the last block is no multiple of rpb
    ('bn', (1, 128, 1, 41, 41), {'M': 5547, 'rows': 64, 'nblocks': 87, 'last': 43,
                                 'rpb': 16}),
    # the last shape on the minimum, and the first off it (129 is no multiple of rpb 32)
    ('bn', (1, 64, 2, 126, 126), {'M': 65536, 'rows': 128, 'nblocks': 512, 'last': 128,
                                  'capped': False}),
    ('bn', (1, 64, 2, 126, 127), {'M': 66048, 'rows': 129, 'nblocks': 512, 'rpb': 32,
                                  'capped': True}),

    ('colsum', (1, 8), {'nblocks': 1, 'last': 1, 'chunks': 1}),
    ('colsum', (15, 8), {'rows': 16, 'nblocks': 1, 'last': 15}),
    ('colsum', (16, 64), {'nblocks': 1, 'last': 16}),
    ('colsum', (17, 64), {'nblocks': 2, 'last': 1}),
    # a second x-block with one live lane
    ('colsum', (33, 520), {'chunks': 65, 'xblocks': 2, 'idle': 63, 'nblocks': 3, 'last': 1}),
    ('colsum', (100, 512), {'chunks': 64, 'xblocks': 1, 'idle': 0}),
    ('colsum', (8192, 64), {'rows': 16, 'nblocks': 512, 'last': 16, 'capped': False}),
    ('colsum', (8193, 64), {'rows': 17, 'nblocks': 482, 'last': 16, 'capped': True}),
    ('colsum', (8209, 512), {'rows': 17, 'nblocks': 483, 'last': 15, 'capped': True}),

    ('ln_tokens', (1, 64), {'nblocks': 1, 'last': 1}),
    ('ln_tokens', (7, 64), {'rows': 8, 'nblocks': 1, 'last': 7}),
    ('ln_tokens', (8, 64), {'nblocks': 1, 'last': 8}),
    ('ln_tokens', (9, 64), {'nblocks': 2, 'last': 1}),
    ('ln_tokens', (9, 512), {'N': 1, 'chunks': 64, 'idle': 0}),
    ('ln_tokens', (13, 576), {'N': 2, 'chunks': 72, 'second': 8}),
    ('ln_tokens', (11, 1024), {'N': 2, 'chunks': 128, 'second': 64}),
    ('ln_tokens', (8192, 64), {'rows': 8, 'nblocks': 1024, 'last': 8, 'capped': False}),
    ('ln_tokens', (8193, 64), {'rows': 9, 'nblocks': 911, 'last': 3, 'capped': True}),
    ('ln_tokens', (9217, 64), {'rows': 10, 'last': 7, 'capped': True}),

    # one interior row (padded row 4)
    ('ln_image', (1, 8, 1, 1), {'M': 9, 'nblocks': 2, 'last': 1, 'interior': [4]}),
    # a batch index above 0 on the tokens path
    ('ln_image', (3, 8, 1, 1), {'M': 27, 'interior': [4, 13, 22]}),
    ('ln_image', (1, 72, 3, 5), {'chunks': 9, 'N': 1}),
    ('ln_image', (1, 512, 2, 3), {'chunks': 64, 'N': 1, 'idle': 0}),
    ('ln_image', (1, 520, 3, 4), {'chunks': 65, 'N': 2, 'second': 1}),
    ('ln_image', (1, 1024, 2, 3), {'N': 2, 'second': 64}),
    ('ln_image', (2, 64, 62, 62), {'M': 8192, 'rows': 8, 'nblocks': 1024, 'last': 8,
                                   'capped': False}),
    ('ln_image', (1, 64, 62, 127), {'M': 8256, 'rows': 9, 'nblocks': 918, 'last': 3,
                                    'capped': True}),
]
SHAPES = [(kind, shape) for kind, shape, _ in TABLE]


def ident(kind, shape):
    return '%s-%s' % (kind, 'x'.join(str(v) for v in shape))


IDS = [ident(kind, shape) for kind, shape in SHAPES]


def shapes_of(kind):
    return [shape for k, shape in SHAPES if k == kind]


def ids_of(kind):
    return ['x'.join(str(v) for v in shape) for shape in shapes_of(kind)]


# (c) nothing stale: one capped and one uncapped row per kind
STALE = [('bn', (1, 72, 2, 3, 4)), ('bn', (1, 2048, 1, 11, 51)),
         ('colsum', (33, 520)), ('colsum', (8193, 64)),
         ('ln_tokens', (13, 576)), ('ln_tokens', (8193, 64)),
         ('ln_image', (1, 520, 3, 4)), ('ln_image', (1, 64, 62, 127))]
