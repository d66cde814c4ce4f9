"""``OccFScoreMetric.all_reduce`` over gloo groups of two and three ranks on the CPU: the
ranks add unequal numbers of samples of tests/golden/occ_fscore_tiny.npz, afterwards
every rank holds every sample's counts in rank order, the same ``cnt`` and the same means.

Against a single-process metric over all samples the means are compared within 1e-12:
the rank order changes the order of at most 7 additions of terms <= 1.00000001, so the
sums differ by less than 7^2 * 2^-53 (each partial sum is below 7.0000001, each addition
rounds by at most half an ulp of that)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from veon_amd.occ_eval import OccFScoreMetric

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'occ_fscore_tiny.npz')
# sample indices per rank: unequal shares, one rank with the all-void prediction (2)
SHARES = {2: {0: (0, 1, 3, 0, 1), 1: (2, 3)},
          3: {0: (3,), 1: (0, 1, 2, 1), 2: (1, 0)}}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _add(m, gold, indices):
    for i in indices:
        m.add_batch(gold['pred'][i], gold['gt'][i], gold['mask_lidar'][i],
                    gold['mask_camera'][i])
    return m


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        with np.load(GOLDEN) as z:
            gold = {k: z[k] for k in z.files}
        m = _add(OccFScoreMetric(device='cpu', use_image_mask=True), gold, SHARES[world][rank])
        own = m.sample_counts()
        m.all_reduce()
        q.put((rank, own, m.sample_counts(), m.count_fscore()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_all_reduce_gives_every_rank_every_sample(world):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    with np.load(GOLDEN) as z:
        gold = {k: z[k] for k in z.files}
    order = [i for r in range(world) for i in SHARES[world][r]]
    assert len(order) <= 7 and len({len(s) for s in SHARES[world].values()}) > 1
    single = _add(OccFScoreMetric(device='cpu', use_image_mask=True), gold, order)
    want = single.count_fscore()
    assert want[3] == len(order)
    for rank, own, gathered, got in res:
        assert np.array_equal(own, gold['default_image_counts'][list(SHARES[world][rank])])
        assert np.array_equal(gathered, single.sample_counts())       # in rank order
        assert got == res[0][3]                 # every rank: the same cnt, the same means
        assert got[3] == len(order)
        np.testing.assert_allclose(got[:3], want[:3], rtol=0, atol=1e-12)
    # ... and the same as one process that saw the samples in another order
    shuffled = _add(OccFScoreMetric(device='cpu', use_image_mask=True), gold, sorted(order))
    np.testing.assert_allclose(shuffled.count_fscore()[:3], want[:3], rtol=0, atol=1e-12)
