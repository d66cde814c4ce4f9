"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only
(everything else is behind --full), and --dump-outputs writes what the last timed
step computed as .npy files, identical from run to run with the same arguments.

CPU: the dump helper (budget, dtypes, fixed sample) on host tensors.
GPU: two plain S2 runs with --dump-outputs give the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_samples_a_large_output_within_budget(tmp_path):
    g = torch.Generator().manual_seed(1)
    vol = torch.randn(1, 80, 16, 100, 100, generator=g)       # 51.2 MB of fp32
    small = torch.randn(3, 5, generator=g)
    arrays = bench.named_tensors({'vol': vol, 'small': small, 'ids': torch.arange(7)})
    assert [n for n, _ in arrays] == ['out.ids', 'out.small', 'out.vol']
    a, b = tmp_path / 'a', tmp_path / 'b'
    info = bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    assert _dir_bytes(a) <= bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6
    for name in ('out.ids', 'out.small', 'out.vol'):
        x, y = np.load(a / (name + '.npy')), np.load(b / (name + '.npy'))
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)
    # small arrays whole, in their shape; integers widened exactly
    assert np.array_equal(np.load(a / 'out.small.npy'), small.numpy())
    ids = np.load(a / 'out.ids.npy')
    assert ids.dtype == np.float64 and np.array_equal(ids, np.arange(7))
    assert info['out.small']['sampled'] is None
    # the large one: a sample of its own elements, at the seeded indices
    s = np.load(a / 'out.vol.npy')
    assert info['out.vol']['sampled'] and s.ndim == 1 and s.size < vol.numel()
    idx = torch.randint(0, vol.numel(), (s.size,),
                        generator=torch.Generator().manual_seed(bench.DUMP_SEED)).sort().values
    assert np.array_equal(s, vol.reshape(-1)[idx].numpy())


def test_full_and_dump_options_are_accepted_by_a_dry_run(tmp_path):
    r = subprocess.run([sys.executable, BENCH, '--dry-run', '--full', '--steps', '2',
                        '--warmup', '0', '--dump-outputs', str(tmp_path / 'd')],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def _run(dump, timeout=600):
    r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '30', '--warmup', '3',
                        '--dump-outputs', dump], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dump_repeats(tmp_path):
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    la, lb = _run(a), _run(b)
    for line in (la, lb):
        assert line['metric'] == '6cam_lift_samples_per_sec' and line['value'] > 0
        assert line['unit'] == 'samples/s' and line['higher_is_better'] is True
        assert line['dtype'] == 'f32' and line['steps'] == 30 and line['ms_per_step'] > 0
        for extra in ('roofline', 'cpu_baseline', 'sv', 'veonb', 'veonl_fp16', 'backward',
                      'percall_prepare'):
            assert extra not in line, extra
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ['bev_volume.npy']
    assert _dir_bytes(a) <= 64 * 10 ** 6
    x, y = np.load(os.path.join(a, 'bev_volume.npy')), np.load(os.path.join(b, 'bev_volume.npy'))
    assert x.dtype == np.float32 and np.isfinite(x).all() and np.count_nonzero(x) > 0
    assert np.array_equal(x, y)
    assert la['outputs']['bev_volume']['shape'] == [1, 80, 16, 200, 200]
