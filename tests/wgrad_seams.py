"""The seam table of the shared weight-gradient body (csrc/wgrad_kernel.h, DESIGN sections
4k - 4m), shared by tests/test_wgrad_seams.py (CPU: the table's premises against the plan
rule and the library's workspace sizes) and tests/test_wgrad_seams_gpu.py.  A plain module:
no fixtures, no GPU, nothing of the code under test.

The body contracts over the rows in slabs of 64 (WBK); the linear case zeroes the tail of a
partial last slab.  The host plan splits the slabs over K: at least 8 slabs per split, all
workgroups within one round of the 256 CUs, and no empty split.
"""
WBK = 64
CUS = 256
GROUPS = {'linear': 1, 'conv2d': 3, 'conv3d': 9}    # workgroups per (Cout, Cin) tile
TAPS = {'linear': 1, 'conv2d': 9, 'conv3d': 27}


def plan(M, Cin, Cout, groups):
    """The rule of ``wgrad_plan`` as DESIGN and its comment state it."""
    tile = 128 if Cin % 128 == 0 and Cout % 128 == 0 else 64
    tiles = groups * (Cout // tile) * (Cin // tile)
    nsteps = -(-M // WBK)
    first = max(1, min(CUS // tiles, nsteps // 8))
    sps = -(-nsteps // first)
    split = -(-nsteps // sps)                        # no empty split
    return {'tile': tile, 'nco': Cout // tile, 'nci': Cin // tile, 'tiles': tiles,
            'nsteps': nsteps, 'first': first, 'sps': sps, 'split': split,
            'slabs': [min(sps, nsteps - i * sps) for i in range(split)]}


def dims(kind, shape):
    """(rows M of the contraction, Cin, Cout) of a shape of the table."""
    if kind == 'linear':
        M, K, N = shape
        return M, K, N
    B, Cin, Cout, *spatial = shape
    M = B
    for v in spatial:
        M *= v + 2
    return M, Cin, Cout


def plan_of(kind, shape):
    M, Cin, Cout = dims(kind, shape)
    return plan(M, Cin, Cout, GROUPS[kind])


# (kind, shape, premises): linear (M, K, N); conv2d (B, Cin, Cout, Y, X); conv3d
# (B, Cin, Cout, Z, Y, X).  Premises are facts of ``plan`` (and of M) that make the row a
# seam; the CPU test asserts each, so a later change of the plan cannot silently turn a seam
# case into an ordinary one.  'tail': live rows of the last slab (0: full); 'slabs': slabs
# per split; 'first': the split count before "no empty split" lowers it.
TABLE = [
    # the slab and zero_tail: 1, 63, 0 and 1 live tail rows
    ('linear', (1, 64, 64), {'nsteps': 1, 'tail': 1, 'split': 1}),
    ('linear', (63, 64, 64), {'nsteps': 1, 'tail': 63, 'split': 1}),
    ('linear', (64, 64, 64), {'nsteps': 1, 'tail': 0, 'split': 1}),
    ('linear', (65, 64, 64), {'nsteps': 2, 'tail': 1, 'split': 1}),
    # 15 slabs: the last shape with no split
    ('linear', (960, 64, 64), {'nsteps': 15, 'tail': 0, 'split': 1}),
    # split 2 turns on, and the last slab has one row
    ('linear', (961, 64, 64), {'nsteps': 16, 'tail': 1, 'split': 2, 'slabs': [8, 8]}),
    ('linear', (1024, 64, 64), {'nsteps': 16, 'tail': 0, 'split': 2, 'slabs': [8, 8]}),
    # wide tile with nco != nci, an uneven last split
    ('linear', (1025, 128, 256), {'tile': 128, 'nco': 2, 'nci': 1, 'split': 2, 'slabs': [9, 8],
                                  'tail': 1}),
    ('linear', (1537, 64, 192), {'tile': 64, 'nco': 3, 'nci': 1, 'split': 3, 'slabs': [9, 9, 7],
                                 'tail': 1}),
    # the first guess of 11 splits is recomputed to 10
    ('linear', (5760, 64, 64), {'nsteps': 90, 'first': 11, 'split': 10, 'tail': 0}),
    # narrow tile although one side is a multiple of 128
    ('linear', (70, 384, 320), {'tile': 64, 'nco': 5, 'nci': 6, 'tiles': 30, 'split': 1,
                                'tail': 6}),
    ('conv2d', (2, 128, 256, 7, 5), {'tile': 128, 'nco': 2, 'nci': 1, 'split': 1}),
    # M = 1023: split 2, and the last slab runs into guard rows
    ('conv2d', (1, 64, 192, 29, 31), {'M': 1023, 'nco': 3, 'nci': 1, 'split': 2,
                                      'slabs': [8, 8], 'tail': 63}),
    ('conv2d', (1, 64, 64, 30, 30), {'M': 1024, 'split': 2, 'slabs': [8, 8], 'tail': 0}),
    ('conv2d', (1, 384, 320, 3, 5), {'tile': 64, 'tiles': 90, 'split': 1}),
    ('conv3d', (2, 128, 256, 3, 7, 5), {'tile': 128, 'nco': 2, 'nci': 1, 'split': 1}),
    # 81 tiles: the CU cap of 3 binds before nsteps / 8 = 4
    ('conv3d', (1, 192, 192, 2, 14, 30), {'tiles': 81, 'nsteps': 32, 'first': 3, 'split': 3,
                                          'slabs': [11, 11, 10]}),
    ('conv3d', (1, 64, 64, 2, 14, 30), {'tiles': 9, 'split': 4, 'slabs': [8, 8, 8, 8]}),
    # 270 tiles, more than the CUs: 256 // tiles = 0 and the split is clamped to 1
    ('conv3d', (1, 384, 320, 1, 3, 5), {'tiles': 270, 'split': 1}),
]
SHAPES = [(kind, shape) for kind, shape, _ in TABLE]
IDS = ['%s-%s' % (kind, 'x'.join(str(v) for v in shape)) for kind, shape in SHAPES]
# the two workloads the comment in wgrad_plan names, with their workgroup counts
WORKLOADS = [('conv3d', (1, 256, 256, 8, 100, 100), 104040, 252),
             ('conv2d', (6, 384, 384, 64, 176), 70488, 243)]
