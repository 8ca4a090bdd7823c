"""bench.py host logic that needs no GPU: the self-spawn of `--gpus N`."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_spawns_its_own_ranks_when_no_launcher_is_present():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '3', '--warmup', '1',
                          '--dry-run-spawn'], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    cmd = json.loads(out.stdout.strip().splitlines()[-1])['spawn']
    assert cmd[1:3] == ['-m', 'torch.distributed.run'] and '--nproc-per-node=4' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:i + 3] == ['--gpus', '4'] and '--steps' in cmd[i:]


def test_dump_outputs_keeps_float_types_and_samples_within_the_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4000)
    arrays = {'small': np.arange(10, dtype=np.float16).reshape(2, 5), 'big': np.arange(3000, dtype=np.float64)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    small = np.load(tmp_path / 'a' / 'small.npy')
    assert small.dtype == np.float32 and small.shape == (2, 5) and np.array_equal(small, arrays['small'])
    big = np.load(tmp_path / 'a' / 'big.npy')
    assert big.dtype == np.float64 and big.nbytes <= 2000 and big.size == 250
    assert np.all(np.diff(big) > 0) and np.all(np.isin(big, arrays['big']))        # a sample, in index order
    assert np.array_equal(big, np.load(tmp_path / 'b' / 'big.npy'))                # the same sample every run


def test_roofline_peak_is_the_executing_unit():
    sys.path.insert(0, ROOT)
    import bench
    m = dict(cfg=bench.WORKLOADS['airplane'], achieved=200.0, kern_ms=0.5, pts_per_launch=4 * 64 * 2048)
    r = bench.roofline_record('airplane', m)
    assert abs(r['peak'] - 2500.0 / 3) < 0.1 and r['frac'] < 1 and abs(r['frac'] - 200.0 / (2500.0 / 3)) < 1e-3
    assert r['ratio_vs_fp32_mfma'] > 1            # the secondary ratio may exceed 1: that unit is not the one executing
