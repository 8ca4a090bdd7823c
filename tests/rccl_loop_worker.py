"""Run by tests/test_gpu_loop_dist.py in a subprocess: training.ResidentTrainLoop with data_parallel=True over RCCL (backend 'nccl')
on a 1-rank group with GWTF_FORCE_SHARDED=1 -- the only multi-rank configuration one GPU allows (RCCL refuses two ranks on one
device), so this has never run on more than one GPU.  The capture must succeed with the guard flag's MAX all-reduce inside (between
gwtf_loop_detect and gwtf_loop_commit); two replays give the plain resident loop's loss terms; a NaN loss value skips the update."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import go_with_the_flows_amd as gw                                              # noqa: E402
from go_with_the_flows_amd import models, optim                                # noqa: E402
from go_with_the_flows_amd.synth import load_synth_                            # noqa: E402
from go_with_the_flows_amd.training import ResidentTrainLoop                   # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
B, N = 4, 48
SCHEDULE = dict(cycle_length=2, min_lr=1.7e-5, max_lr=2.56e-4, beta1=0.9, min_beta2=0.9945, max_beta2=0.999)
noise = torch.from_numpy(np.load(os.path.join(GOLDEN, 'g13_full_model.npz'))['noise_g']).cuda()


class TriggerLoss(models.Flow_Mixture_Loss):
    """The loss VALUE is poisoned, not the data: gradients stay finite."""

    def fused(self, output_prior, dec):
        loss, pnll, gnll, gent = super().fused(output_prior, dec)
        return loss + self.trigger, pnll, gnll, gent


def store():
    D = np.load(os.path.join(GOLDEN, 'g22_clouds.npz'))
    v, f, copies = D['vertices_c'], D['faces_vc'], 4
    vb, fb = D['vertices_c_bounds'].astype(np.int64), D['faces_bounds'].astype(np.int64)
    vbs = np.concatenate([vb[:1]] + [vb[1:] + k * len(v) for k in range(copies)])
    fbs = np.concatenate([fb[:1]] + [fb[1:] + k * len(f) for k in range(copies)])
    return gw.MeshStore.from_arrays(np.tile(v, (copies, 1)), np.tile(f, (copies, 1)), vbs, fbs, device=dev)


def build(sync, data_parallel):
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], pc_enc_n_features=[128, 256, 512])
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    m = m.cuda().train()
    if sync:
        m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)                   # train_ae.py:152
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    crit = TriggerLoss(**cfg)
    crit.trigger = torch.zeros((), device=dev)
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    loader = gw.DeviceCloudLoader(MESHES, B, N, gw.CloudTransform(center=True), seed=21)
    loop = ResidentTrainLoop(m, crit, opt, loader, scheduler=optim.LRUpdater(3, **SCHEDULE), data_parallel=data_parallel)
    loop.set_epoch(0)
    return m, crit, opt, loop


def two_replays(loop):
    terms = []
    for _ in range(2):
        loop.run(1)
        terms.append([float(t) for t in loop.terms])
    return terms


MESHES = store()
# ---- the plain resident loop: one process, no process group ----
_, _, _, loop1 = build(False, None)
assert not loop1.data_parallel and loop1.reducer is None
terms1 = two_replays(loop1)

# ---- the same loop, sharded, over RCCL ----
os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
os.environ.setdefault('MASTER_PORT', str(29850 + os.getpid() % 200))
os.environ['GWTF_FORCE_SHARDED'] = '1'
dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
m2, crit2, opt2, loop2 = build(True, True)                  # the capture holds the flag's all-reduce
assert loop2.data_parallel and loop2.reducer is not None
terms2 = two_replays(loop2)
worst = max(abs(a - b) / max(1.0, abs(b)) for x, y in zip(terms2, terms1) for a, b in zip(x, y))
print('LOOP1 terms', terms1, terms2, f'worst={worst:.2e}', flush=True)
assert worst < 1e-5, worst
rec = loop2.meters()
assert rec['step'] == 2 and rec['iteration'] == 2 and not rec['poisoned'], rec
snap = [p.detach().clone() for p in m2.parameters()] + [opt2.state[p]['exp_avg'].clone() for p in loop2.parameters]
crit2.trigger.fill_(float('nan'))
loop2.run(1)
rec = loop2.meters()
assert rec['poisoned'] and rec['poisoned_at'] == 2 and rec['step'] == 2 and rec['iteration'] == 2, rec
now = [p.detach() for p in m2.parameters()] + [opt2.state[p]['exp_avg'] for p in loop2.parameters]
assert all(torch.equal(a, b) for a, b in zip(snap, now))
dist.barrier()
dist.destroy_process_group()
print('LOOP1 ok', flush=True)
