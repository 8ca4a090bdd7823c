"""Worker for tests/test_gpu_norm2d_sync.py::test_two_rank_svr_training_step_matches_single_process.
Two ranks share cuda:0 (one-GPU box), gloo carries the collectives.  The whole Flow_Mixture_SVR_Model (contract_svr.json's
small_cfg, img_encoder.train_norm = 'hip') is converted to SyncBatchNorm as the reference's train_svr.py does; each rank owns two
of the four shapes.  Loss terms, the parameter gradients averaged over the ranks and every running statistic must equal the
single-process full-batch forward_fused step on the same kernels (tests/dist_model_worker.py for the autoencoding model)."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_with_the_flows_amd import models, norm2d             # noqa: E402
from go_with_the_flows_amd.dist import shard_bounds, all_reduce_gradients   # noqa: E402
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images   # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
N_NORM2D = 20                   # BatchNorm2d layers of ResNet-18: the stem, 16 in the blocks, 3 downsample branches


def build(D):
    """tests/test_gpu_svr_fused.py build(), with the fused BatchNorm2d kernels."""
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    m.img_encoder.train_norm = 'hip'
    return m.cuda().train(), cfg


def step(m, cfg, g_in, p_in, images, noise):
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    crit = models.Flow_Mixture_Loss(**cfg)
    terms = crit.fused(*m.forward_fused(g_in, p_in, images=images))
    terms[0].backward()
    return torch.stack([t.detach().reshape(()) for t in terms])


def flat_state(m):
    return torch.cat([v.reshape(-1).float() for k, v in m.state_dict().items() if 'running' in k]).cpu().numpy()


def flat_state_2d(m):
    """The running statistics the fused BatchNorm2d kernels wrote (every norm of the image encoder but fc_bn)."""
    return torch.cat([v.reshape(-1).float() for k, v in m.img_encoder.state_dict().items() if 'running' in k and 'fc_bn' not in k]).cpu().numpy()


def flat_grads(m):
    return torch.cat([q.grad.reshape(-1) for q in m.parameters() if q.grad is not None]).cpu().numpy()


def main():
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    D = np.load(os.path.join(GOLDEN, 'g21_svr.npz'))
    g_all, p_all, noise = (torch.from_numpy(np.ascontiguousarray(D[k], np.float32)).cuda() for k in ('gcloud', 'pcloud', 'noise_g'))
    images = torch.from_numpy(synth_images(4, 64, 64, 2123)).cuda()
    B = g_all.shape[0]
    assert B == 4
    b0, b1 = shard_bounds(B, rank, world)
    m, cfg = build(D)
    m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert m.img_encoder._hip_ok and isinstance(m.img_encoder.bn1, torch.nn.SyncBatchNorm)
    n0 = norm2d.COLLECTIVES['n']
    m.reparameterize = lambda mu, logvar: noise[b0:b1] * torch.exp(0.5 * logvar) + mu
    crit = models.Flow_Mixture_Loss(**cfg)
    terms = crit.fused(*m.forward_fused(g_all[b0:b1], p_all[b0:b1], images=images[b0:b1].contiguous()))
    n_fwd = norm2d.COLLECTIVES['n'] - n0
    terms[0].backward()
    n_bwd = norm2d.COLLECTIVES['n'] - n0 - n_fwd
    assert (n_fwd, n_bwd) == (N_NORM2D, N_NORM2D), (n_fwd, n_bwd)
    all_reduce_gradients(m, average=True)
    lt = torch.stack([t.detach().reshape(()) for t in terms])
    dist.all_reduce(lt)                                        # each rank's terms: the mean over its own rows
    np.savez(os.path.join(os.environ['GWTF_TMP'], f'svr{rank}.npz'), grads=flat_grads(m), terms=(lt / world).cpu().numpy(),
             state=flat_state(m), state2d=flat_state_2d(m))
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        m1, cfg = build(D)
        t1 = step(m1, cfg, g_all, p_all, images, noise).cpu().numpy()
        g1 = flat_grads(m1)
        parts = [np.load(os.path.join(os.environ['GWTF_TMP'], f'svr{r}.npz')) for r in range(world)]
        assert np.array_equal(parts[0]['state2d'], parts[1]['state2d'])      # both ranks finalise from the same all-reduced sums
        part = parts[0]
        rel = lambda a, b: float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
        res = {'terms': float(np.max(np.abs(part['terms'] - t1) / np.maximum(1.0, np.abs(t1)))), 'grads': rel(part['grads'], g1),
               'running': rel(part['state'], flat_state(m1))}
        off, per = 0, {}                                       # per top-level module, for the failure message
        for name, q in m1.named_parameters():
            if q.grad is None:
                continue
            n = q.numel()
            key = name.split('.')[0]
            per[key] = max(per.get(key, 0.0), float(np.abs(part['grads'][off:off + n] - g1[off:off + n]).max() / (np.abs(g1).max() + 1e-12)))
            off += n
        print('SVR2', ' '.join(f'{k}={v:.2e}' for k, v in res.items()), '|', ' '.join(f'{k}={v:.1e}' for k, v in per.items()),
              f'collectives={n_fwd}+{n_bwd}', flush=True)
        # the bounds of tests/dist_model_worker.py (the autoencoding model's two-rank step)
        assert res['terms'] < 1e-5 and res['grads'] < 2e-3 and res['running'] < 1e-4, res
        print('SVR2 ok', flush=True)


if __name__ == '__main__':
    main()
