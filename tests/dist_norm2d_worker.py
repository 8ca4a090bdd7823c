"""Worker for tests/test_gpu_norm2d_sync.py::test_two_rank_layer_matches_the_full_batch_chain.
Two ranks share cuda:0 (one-GPU box), gloo carries the (C, 2) float64 sums.  Every case of SYNC_CASES runs through
norm2d.NormAct2dFn with the global count, each rank on its shard_bounds share of the images; every tensor goes into
$GWTF_TMP/norm2d<rank>.npz for the test to compare with the float64 chain of the full batch."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_with_the_flows_amd import norm2d                      # noqa: E402
from go_with_the_flows_amd.dist import shard_bounds          # noqa: E402
from test_gpu_norm2d import CASES, EPS, MOMENTUM, inputs     # noqa: E402

# the cases of tests/test_gpu_norm2d.py that run split over the ranks, and one more: ONE value per channel on each rank
LOCAL_ONE = 'none_2x4x1x1'
CASES.setdefault(LOCAL_ONE, ((2, 4, 1, 1), 'none', 7, None, 0.0, 1.0))
SYNC_CASES = ('plain_3x5x7x7', 'residual_3x5x7x7', 'none_3x5x7x7', 'shifted_3x5x7x7', 'plain_2x3x56x56', 'residual_2x64x14x14',
              'pool_2x3x9x11', 'pool_2x4x49x66', LOCAL_ONE)
DEV = 'cuda:0'


def run_case(name, rank, world):
    shape, variant = CASES[name][:2]
    b0, b1 = shard_bounds(shape[0], rank, world)
    x, gamma, beta, r, rm, rv, dy = inputs(name)
    x, dy = x[b0:b1].contiguous().to(DEV), dy[b0:b1].contiguous().to(DEV)
    r = None if r is None else r[b0:b1].contiguous().to(DEV)
    gamma, beta, rm, rv = (t.to(DEV) for t in (gamma, beta, rm, rv))
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    if r is not None:
        r.requires_grad_(True)
    count = norm2d.global_count(b1 - b0, shape[2], shape[3], x.device)
    assert count == shape[0] * shape[2] * shape[3], (name, count)
    n0 = norm2d.COLLECTIVES['n']
    y, stats, _ = norm2d.NormAct2dFn.apply(x, gamma, beta, r, rm, rv, EPS, MOMENTUM, variant != 'none', variant == 'pool', count)
    n1 = norm2d.COLLECTIVES['n']
    y.backward(dy)
    n2 = norm2d.COLLECTIVES['n']
    out = {'y': y.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad, 'mean': stats[0], 'rstd': stats[1],
           'running_mean': rm, 'running_var': rv}
    if r is not None:
        out['d_residual'] = r.grad
    out = {f'{name}.{k}': v.detach().cpu().numpy() for k, v in out.items()}
    out[f'{name}.collectives'] = np.array([n1 - n0, n2 - n1])
    return out


def main():
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    saved = {}
    for name in SYNC_CASES:
        saved.update(run_case(name, rank, world))
    torch.cuda.synchronize()
    np.savez(os.path.join(os.environ['GWTF_TMP'], f'norm2d{rank}.npz'), **saved)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print('NORM2D2 ok', flush=True)


if __name__ == '__main__':
    main()
