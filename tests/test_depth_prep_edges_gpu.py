"""Depth preparation (csrc/depth_ops.hip) away from the golden fixtures: depth maps built
by hand, every block-min factor, ragged pixel counts, other (D, lo, step, gamma) and so
other slot counts K (inputs: tests/edge_refs.depth_map, whose construction
tests/test_edge_refs.py checks on the CPU) -- against the C oracle (``oracle.c_oracle.downsample_depth`` /
``two_hot_depth``) at the tolerance the project states for these kernels (rtol 1e-5,
atol 1e-8 for the weights: ``expf`` implementations; exact for the block minimum), with
the exactly-known cases on top, and the compact window form against the dense kernel bit
for bit.  Every output is carved out of an arena with poisoned guard bands
(tests/test_lift_bounds_gpu.py), checked untouched after the launches.

All steps used are binary fractions, so every bin centre k*step + (lo + step/2) and
every midpoint is exact in float32 whatever the contraction of the multiply-add.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import edge_refs as er
from tests.test_lift_bounds_gpu import Arena
from veon_amd import _lib, depth_ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = [0.0, 1e-4, 0.05]


class Run:
    """One raw-ABI pass of the three kernels into a guarded arena."""

    def __init__(self, depth, ds, params, eps_list):
        D, lo, step, gamma = params
        L, s = _lib.lib(), _lib.stream_ptr(DEV)
        _, bn, Hs, Ws = depth.shape
        h, w = Hs // ds, Ws // ds
        n = bn * h * w
        self.K = K = L.veon_two_hot_window_slots(D, step, gamma)
        assert K == depth_ops.two_hot_window_slots(D, step, gamma) and 2 <= K <= D + 1
        ar = Arena(8 << 20)
        src = torch.from_numpy(depth).to(DEV)
        down = ar.take(n, torch.float32)
        assert L.veon_downsample_depth(bn, Hs, Ws, ds, _lib.ptr(src), _lib.ptr(down), s) == 0
        dense = ar.take(n * D, torch.float32)
        assert L.veon_two_hot_depth(bn, h, w, ds, D, lo, step, gamma, _lib.ptr(src),
                                    _lib.ptr(dense), s) == 0
        two_step = ar.take(n * D, torch.float32)
        assert L.veon_two_hot_depth(bn, h, w, 0, D, lo, step, gamma, _lib.ptr(down),
                                    _lib.ptr(two_step), s) == 0
        self.windows = {}
        for eps in eps_list:
            for route, (inp, dsf) in (('fused', (src, ds)), ('two-step', (down, 0))):
                win = ar.take(n * 2, torch.int32)
                wts = ar.take(n * K, torch.float32)
                assert L.veon_two_hot_window(bn, h, w, dsf, D, lo, step, gamma, eps, K,
                                             _lib.ptr(inp), _lib.ptr(win), _lib.ptr(wts), s) == 0
                self.windows[eps, route] = (win.view(1, bn, h, w, 2), wts.view(1, bn, h, w, K))
        torch.cuda.synchronize()
        ar.check()
        self.down = down.view(1, bn, h, w)
        self.dense = dense.view(1, bn, D, h, w)
        self.two_step = two_step.view(1, bn, D, h, w)


def _check(depth, want_min, kind, ds, params):
    D, lo, step, gamma = params
    run = Run(depth, ds, params, EPS)
    # block minimum: exact, against the oracle and against the construction
    o_min = c_oracle.downsample_depth(depth, ds)
    assert np.array_equal(o_min, want_min)
    assert np.array_equal(run.down.cpu().numpy(), o_min)
    # dense weights: the oracle at the stated tolerance; fused == two-step to the bit
    o_w = c_oracle.two_hot_depth(o_min, D, lo, step, gamma)
    got = run.dense.cpu().numpy()
    np.testing.assert_allclose(got, o_w, rtol=1e-5, atol=1e-8)
    assert torch.equal(run.dense, run.two_step)
    # exactly-known pixels: every logit clamped -> 1/(D+1) on all D bins
    uniform = np.broadcast_to((kind != 2)[:, :, None], got.shape)
    assert uniform.any()
    assert np.array_equal(got[uniform], np.full(uniform.sum(), np.float32(1) / np.float32(D + 1),
                                                np.float32))
    # on a midpoint the two neighbours are bit-equal
    c = er.depth_centres(D, lo, step)
    mids = (c[:-1] + c[1:]) / np.float32(2)
    for k in range(D - 1):
        at = (o_min == mids[k])[:, :, None] & (np.arange(D) == k)[None, None, :, None, None]
        if at.any():
            nxt = np.roll(at, 1, axis=2)
            assert np.array_equal(got[at], got[nxt])
    cpu_depth = torch.from_numpy(o_min)
    for eps in EPS:
        win, wts = run.windows[eps, 'fused']
        w2, t2 = run.windows[eps, 'two-step']
        assert torch.equal(win, w2) and torch.equal(wts, t2)
        tw = depth_ops.TwoHotWindows(win, wts, D, eps)
        assert torch.equal(tw.dense(), run.dense)                  # bit for bit
        x, y = win[..., 0].cpu().long(), win[..., 1].cpu().long()
        k0, nk = x & 0xffff, x >> 16
        q0, nq, flag = y & 0xffff, (y >> 16) & 0x7fff, y < 0
        assert int(nk.max()) <= run.K - 1 and int(nk.min()) >= 0
        some = nk > 0
        assert bool((k0[some] >= 0).all()) and bool(((k0 + nk)[some] <= D).all())
        assert bool((k0[~some] == D).all())
        kept = nq > 0
        assert bool((nq <= nk).all())
        assert bool((q0[kept] >= k0[kept]).all())
        assert bool(((q0 + nq)[kept] <= (k0 + nk)[kept]).all())
        tail = wts[..., 0].cpu()
        assert torch.equal(flag, tail >= torch.tensor(eps, dtype=torch.float32))
        # the kept window is exactly the bins with weight >= eps
        dense_cpu = run.dense.cpu()
        assert torch.equal(tw.kept().cpu(), dense_cpu >= torch.tensor(eps, dtype=torch.float32))
        # the CPU mirror
        mirror = depth_ops.two_hot_windows(cpu_depth, D, lo, step, gamma, eps)
        assert mirror.K == run.K
        assert torch.equal(win.cpu(), mirror.win)
        np.testing.assert_allclose(wts.cpu().numpy(), mirror.wts.numpy(), rtol=1e-5, atol=1e-8)
    return run


@pytest.mark.parametrize('params', er.DEPTH_PARAMS, ids=lambda p: 'D%d_lo%g_st%g_g%g' % p)
@pytest.mark.parametrize('ds', [1, 2, 4, 8, 16])
def test_hand_built_maps(ds, params):
    h, w = {1: (16, 44), 2: (1, 257), 4: (16, 44), 8: (1, 257), 16: (16, 44)}[ds]
    assert er.DEPTH_BN * h * w >= len(er.depth_targets(*params)[0])   # every special depth occurs
    depth, want_min, kind = er.depth_map(h, w, ds, params)
    run = _check(depth, want_min, kind, ds, params)
    D, _, step, gamma = params
    print('ds %d  %dx%d  D %d step %g gamma %g: K %d, %d pixels (%d zero blocks, %d uniform)'
          % (ds, h, w, D, step, gamma, run.K, kind.size, (kind == 0).sum(), (kind == 1).sum()))


@pytest.mark.parametrize('size', er.DEPTH_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('ds', [1, 2, 8])
def test_ragged_pixel_counts(ds, size):
    for params in (er.DEPTH_PARAMS[0], er.DEPTH_PARAMS[3]):
        depth, want_min, kind = er.depth_map(size[0], size[1], ds, params)
        _check(depth, want_min, kind, ds, params)


def test_wrappers_agree_with_the_raw_calls():
    """``depth_ops`` on ROCm tensors (what the path calls) gives the arena run's bits."""
    from veon_amd import depth_ops_hip
    params = er.DEPTH_PARAMS[1]
    D, lo, step, gamma = params
    depth, want_min, kind = er.depth_map(3, 5, 4, params)
    run = Run(depth, 4, params, [1e-4])
    src = torch.from_numpy(depth).to(DEV)
    down = depth_ops.downsample_depth(src, 4)
    assert torch.equal(down, run.down)
    assert torch.equal(depth_ops.two_hot_depth_fused(src, 4, D, lo, step, gamma), run.dense)
    assert torch.equal(depth_ops.two_hot_depth(down, D, lo, step, gamma), run.dense)
    for inp, dsf in ((src, 4), (down, 0)):
        tw = depth_ops_hip.two_hot_windows(inp, D, lo, step, gamma, 1e-4, fused_downsample=dsf)
        assert torch.equal(tw.win, run.windows[1e-4, 'fused'][0])
        assert torch.equal(tw.wts, run.windows[1e-4, 'fused'][1])
