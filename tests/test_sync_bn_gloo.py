"""``sync_bn.batch_norm_train`` over gloo groups of 2 and 3 ranks on the CPU with UNEQUAL
per-rank batch sizes: each rank runs forward and backward on its slice of one fp64 tensor;
together they must be nn.BatchNorm3d on the whole batch (the semantics of
nn.SyncBatchNorm, which itself refuses CPU tensors)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from veon_amd import sync_bn

C = 6
SPATIAL = (2, 3, 4)
SPLITS = {2: (2, 1), 3: (1, 2, 1)}       # samples per rank
RTOL = 1e-10


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(world, momentum):
    """The whole batch, the output gradient and the module, from one seed: every process
    builds the same.  Sample b is shifted by 2 b and scaled by 1 + b, so the samples'
    means differ and a mean of per-rank means is not the batch mean on an unequal split."""
    g = torch.Generator().manual_seed(10 + world)
    B = sum(SPLITS[world])
    x = torch.randn(B, C, *SPATIAL, generator=g, dtype=torch.float64)
    b = torch.arange(B, dtype=torch.float64).view(B, 1, 1, 1, 1)
    x = x * (1 + b) + 2 * b
    ident = torch.randn(B, C, *SPATIAL, generator=g, dtype=torch.float64)
    da = torch.randn(B, C, *SPATIAL, generator=g, dtype=torch.float64)
    bn = nn.BatchNorm3d(C, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.normal_(0, 0.2, generator=g)
        bn.running_mean.normal_(0, 0.2, generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    return x, ident, da, bn


def _slice(world, rank):
    lo = sum(SPLITS[world][:rank])
    return slice(lo, lo + SPLITS[world][rank])


def _worker(rank, world, port, momentum, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        x, ident, da, bn = _problem(world, momentum)
        bn = nn.SyncBatchNorm.convert_sync_batchnorm(bn)
        assert sync_bn.is_sync(bn) and sync_bn.group_of(bn) is dist.group.WORLD
        sl = _slice(world, rank)
        xs = x[sl].clone().requires_grad_(True)
        ids = ident[sl].clone().requires_grad_(True)
        before = sync_bn.ALL_REDUCE_CALLS
        out = sync_bn.batch_norm_train(xs, bn, ids, relu=True)
        out.backward(da[sl])
        calls = sync_bn.ALL_REDUCE_CALLS - before
        q.put((rank, out.detach().numpy(), xs.grad.numpy(), ids.grad.numpy(),
               bn.weight.grad.numpy(), bn.bias.grad.numpy(), bn.running_mean.numpy(),
               bn.running_var.numpy(), int(bn.num_batches_tracked), calls))
    finally:
        dist.destroy_process_group()


def _close(got, want):
    return bool((got - want).norm() <= RTOL * want.norm())


@pytest.mark.parametrize('momentum', [0.1, None])
@pytest.mark.parametrize('world', sorted(SPLITS))
def test_ranks_together_are_the_full_batch(world, momentum):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, momentum, q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    x, ident, da, bn = _problem(world, momentum)
    x.requires_grad_(True)
    ident.requires_grad_(True)
    want = torch.relu(bn(x) + ident)
    want.backward(da)
    t = torch.from_numpy
    assert _close(torch.cat([t(r[1]) for r in res]), want.detach())
    assert _close(torch.cat([t(r[2]) for r in res]), x.grad)
    assert _close(torch.cat([t(r[3]) for r in res]), ident.grad)
    # the parameter gradients stay per rank: they SUM to the full batch's
    assert _close(sum(t(r[4]) for r in res), bn.weight.grad)
    assert _close(sum(t(r[5]) for r in res), bn.bias.grad)
    assert not _close(t(res[0][4]) * world, bn.weight.grad)
    for r in res:
        assert _close(t(r[6]), bn.running_mean) and _close(t(r[7]), bn.running_var)
        assert r[8] == int(bn.num_batches_tracked) == 1
        assert r[9] == 2            # one collective per direction
    # a mean of per-rank means (equal weights) is NOT the batch mean on this split: the
    # inputs must tell the two apart by far more than the tolerance
    xd = x.detach()
    dims = [0, 2, 3, 4]
    mean_of_means = torch.stack([xd[_slice(world, r)].mean(dims)
                                 for r in range(world)]).mean(0)
    full = xd.mean(dims)
    assert float((mean_of_means - full).norm() / full.norm()) > 1e-2
    wrong = torch.relu((xd - mean_of_means.view(1, -1, 1, 1, 1))
                       * (xd.var(dims, unbiased=False) + bn.eps).rsqrt().view(1, -1, 1, 1, 1)
                       * bn.weight.detach().view(1, -1, 1, 1, 1)
                       + bn.bias.detach().view(1, -1, 1, 1, 1) + ident.detach())
    assert float((wrong - want.detach()).norm() / want.detach().norm()) > 1e6 * RTOL
