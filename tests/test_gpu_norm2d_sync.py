"""The fused BatchNorm2d layer with batch statistics over several ranks (SyncBatchNorm: gwtf_norm2d_*_sums / _apply through
norm2d.NormAct2dFn's count argument), the image encoder and the whole single-view-reconstruction step on top of it.  Needs an MI355X.

One GPU: two ranks share cuda:0 over gloo (tests/test_gpu_encoder.py::test_two_rank_syncbn_encoder_matches_single_process), and the
collectives run over RCCL, eagerly and captured in a hipGraph, on a 1-rank group with GWTF_FORCE_SHARDED=1.  Nothing here has run on
more than one GPU.

Layer bar: the project's rule for an fp32 kernel against float64 (tests/test_gpu_norm2d.py): err <= max(2 err_torch_fp32, 1e-6 scale)
against the CPU float64 chain of the FULL batch, with that file's kink-margin assertion per case (a property of the full-batch inputs).
Nothing is excluded from a comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record_parity
from dist_norm2d_worker import LOCAL_ONE, SYNC_CASES
from go_with_the_flows_amd.dist import shard_bounds
from test_gpu_norm2d import CASES, KEYS, chain

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _torchrun(worker, tmp_path, offset):
    """Two ranks of `worker`, launched as test_two_rank_syncbn_encoder_matches_single_process launches its worker."""
    env = dict(os.environ, GWTF_TMP=str(tmp_path), MASTER_ADDR='127.0.0.1')
    port = 29700 + (os.getpid() + offset) % 1000
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(HERE, worker)]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope='module')
def two_rank_layers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('norm2d_sync')
    r = _torchrun('dist_norm2d_worker.py', tmp, 311)
    assert r.returncode == 0 and 'NORM2D2 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return [np.load(os.path.join(tmp, f'norm2d{rank}.npz')) for rank in range(2)]


@pytest.mark.parametrize('name', SYNC_CASES)
def test_two_rank_layer_matches_the_full_batch_chain(name, two_rank_layers):
    """Concatenated y / dx / d_residual rows, dgamma / dbeta SUMMED over the ranks (they stay rank-local, as torch's SyncBatchNorm
    leaves them) and each rank's mean, rstd and running statistics against the float64 chain of the full batch."""
    shape, variant, _, margin, _, _ = CASES[name]
    r64, r32 = chain(name, torch.float64), chain(name, torch.float32)
    if margin is not None:                                   # the property of the input the gradient comparison rests on
        assert float(r64['pre'].abs().min()) > margin, (name, float(r64['pre'].abs().min()))
    parts = two_rank_layers
    sizes = [b - a for a, b in (shard_bounds(shape[0], rank, 2) for rank in range(2))]
    if name == LOCAL_ONE:
        assert sizes == [1, 1] and shape[2] * shape[3] == 1                     # one value per channel on each rank
    get = lambda rank, key: torch.from_numpy(parts[rank][f'{name}.{key}'])
    for rank in range(2):
        assert get(rank, 'y').shape[0] == sizes[rank]
        assert list(parts[rank][f'{name}.collectives']) == [1, 1]               # one all-reduce forward, one backward
    for key in ('running_mean', 'running_var'):
        assert torch.equal(get(0, key), get(1, key)), (name, key)               # both ranks finalise from the same totals
    got = {}
    for key in KEYS:
        if key not in r64:
            continue
        if key in ('y', 'dx', 'd_residual'):
            got[key] = [torch.cat([get(0, key), get(1, key)])]
        elif key in ('dgamma', 'dbeta'):
            got[key] = [get(0, key).double() + get(1, key).double()]
        else:
            got[key] = [get(0, key), get(1, key)]
    for key, tensors in got.items():
        ref = r64[key]
        scale = float(ref.abs().max())
        err32 = float((r32[key].double() - ref).abs().max())
        for rank, t in enumerate(tensors):
            err = float((t.double() - ref).abs().max())
            record_parity(f'norm2d_sync_{name}_{key}' + (f'_rank{rank}' if len(tensors) > 1 else ''), err=err, err_torch_fp32=err32,
                          scale=scale)
            assert err <= max(2.0 * err32, 1e-6 * scale), (name, key, rank, err, err32, scale)


def test_single_rank_rccl_sync_path_gives_the_plain_path_bits():
    """residual_2x3x33x33 and pool_2x3x9x11 over RCCL on a 1-rank group: y, stats and running statistics bit-equal to the plain call,
    dx within the bar of the float64 chain, two collectives per layer."""
    r = subprocess.run([sys.executable, os.path.join(HERE, 'rccl_norm2d_worker.py'), 'layer'], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'LAYER1 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_two_rank_svr_training_step_matches_single_process(tmp_path):
    """The whole SVR model (small_cfg, 64 x 64 images, B = 4 as 2 + 2, train_norm = 'hip', convert_sync_batchnorm): loss terms,
    parameter gradients averaged over the ranks and every running statistic against the single-process full-batch forward_fused
    step on the same kernels, within the bounds tests/dist_model_worker.py uses for the autoencoding model (terms 1e-5, gradients
    2e-3 of the largest entry, running statistics 1e-4; measured on an MI355X: 2.4e-7, 6.2e-6, 1.5e-7); 20 + 20 BatchNorm2d
    collectives per step."""
    r = _torchrun('dist_svr_worker.py', tmp_path, 523)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'SVR2 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_graphed_data_parallel_svr_step_captures_and_replays():
    """GraphedTrainStep(svr, ..., images_example=..., data_parallel=True) on a 1-rank RCCL group with GWTF_FORCE_SHARDED=1: 40
    BatchNorm2d all-reduces per pass inside the capture, none issued by a replay.  Against the plain graphed step: after the first
    step the single-step bounds of tests/rccl_graph_worker.py (measured: terms 1.2e-7 of 1e-5, gradients 7.7e-4 of 2e-3, buffers
    5.8e-7 of 1e-4, parameters 1.99 of 2.2 lr); after the second, which starts from weights Adam left up to 2 lr apart, the
    trajectory bounds of tests/test_gpu_svr_fused.py (terms 1.9e-5 of 1e-4, state 3.1e-3 of 2e-2, parameters 3.25 of 4.4 lr).  The
    worker's docstring has the reasoning."""
    r = subprocess.run([sys.executable, os.path.join(HERE, 'rccl_norm2d_worker.py'), 'graph'], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'GRAPHSVR1 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
