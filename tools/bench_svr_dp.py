#!/usr/bin/env python3
"""What data parallelism costs one training step of the single-view-reconstruction model on ONE MI355X (tools/bench_svr_train.py's
model and batches: tests/golden/contract_svr.json svr_cfg, 224 x 224 images, img_encoder.train_norm = 'hip'), two ways in ONE
process, alternated:

  plain   training.GraphedTrainStep(..., images_example=...)
  dp      the same model after nn.SyncBatchNorm.convert_sync_batchnorm, GraphedTrainStep(..., data_parallel=True) on a 1-rank RCCL
          group with GWTF_FORCE_SHARDED=1: every exchange of the multi-rank step is in the graph as an RCCL kernel -- the 20 + 20
          BatchNorm2d all-reduces of the image encoder with their 40 fold / finalise / float launches, the decoders' and the cloud
          encoder's statistic all-reduces, the row gathers, the gradient exchange -- each over one rank.

That is the launch and collective overhead a rank pays, NOT multi-GPU scaling: nothing here runs on more than one GPU, no byte
crosses a link.  Timing: stream events around --steps steps, after --warmup steps per variant, --repeats times per variant (the
spread).  Before the timing each variant takes ONE step from the same initial state with the same injected reparameterisation noise:
the four loss terms go into the record (the two must agree).

    python tools/bench_svr_dp.py [--batches 128,32] [--steps 50] [--warmup 10] [--repeats 3] [--out profiles/r24_svr_dp.jsonl]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from bench_svr_train import config, make_optimizer  # noqa: E402
from go_with_the_flows_amd import models, norm2d  # noqa: E402
from go_with_the_flows_amd.synth import calibrate_image_encoder, load_image_encoder_stats_, load_synth_, synth_images, synth_inputs  # noqa: E402
from go_with_the_flows_amd.training import GraphedTrainStep  # noqa: E402


class Variant:
    """The graphed step, plain or data parallel, on its own copy of the model (same initial state) with its own optimiser."""

    def __init__(self, dp, base_model, cfg, batch, noise=None):
        self.key, self.batch = 'dp' if dp else 'plain', batch
        os.environ['GWTF_FORCE_SHARDED'] = '1' if dp else '0'            # read while the step is built; a replay reads nothing
        self.model = copy.deepcopy(base_model)
        if dp:
            self.model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(self.model)
        self.model.img_encoder.train_norm = 'hip'
        if noise is not None:
            self.model.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
        self.opt = make_optimizer(self.model, cfg)
        n0 = norm2d.COLLECTIVES['n']
        self.graph = GraphedTrainStep(self.model, models.Flow_Mixture_Loss(**cfg), self.opt, batch[0], batch[1], images_example=batch[2],
                                      data_parallel=dp)
        self.norm2d_collectives_per_pass = (norm2d.COLLECTIVES['n'] - n0) // 3       # 2 warm-up passes + the captured one

    def step(self):
        return self.graph(*self.batch)

    def timed(self, steps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(steps):
            self.step()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,32')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r24_svr_dp.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_svr_dp needs a HIP device'
    dev, cfg = torch.device('cuda', 0), config()
    torch.cuda.set_device(dev)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(29900 + os.getpid() % 90))
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    n_points, (H, W) = cfg['cloud_size'], cfg['image_size']
    base = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(base, 2310, output_gain=0.3)
    with torch.no_grad():                       # the prior flow near the identity: tools/bench_svr_train.py has the reason
        for couple in base.g_prior.flows:
            for nvp in (couple.nvp1, couple.nvp2):
                for head in (nvp.T_mu_0, nvp.T_logvar_0):
                    head[3].weight.mul_(0.1)
                    head[3].bias.mul_(0.1)
    load_image_encoder_stats_(base.img_encoder, calibrate_image_encoder(base.img_encoder, 2311))
    base = base.to(dev).train()
    lines = []
    for B in (int(b) for b in args.batches.split(',')):
        g = torch.from_numpy(synth_inputs(B, n_points, 4, 2320)[0]).to(dev)
        p = torch.from_numpy(synth_inputs(B, n_points, 4, 2321)[0]).to(dev)
        imgs = torch.from_numpy(synth_images(B, H, W, 2322)).to(dev)
        batch = (g, p, imgs)
        noise = torch.randn(B, cfg['g_latent_space_size'], generator=torch.Generator().manual_seed(2323)).to(dev)
        terms = {}
        for dp in (False, True):                # one step each from the same state with the same noise: the same four numbers
            v = Variant(dp, base, cfg, batch, noise)
            terms[v.key] = [float(t) for t in v.step()]
            del v
        torch.cuda.empty_cache()
        vs = [Variant(dp, base, cfg, batch) for dp in (False, True)]
        for v in vs:
            for _ in range(args.warmup):
                v.step()
        ms = {v.key: [] for v in vs}
        for _ in range(args.repeats):           # alternated: a drift of the machine hits both alike
            for v in vs:
                ms[v.key].append(round(v.timed(args.steps), 3))
        rec = {'bench': 'svr_train_step_dp', 'B': B, 'n_points': n_points, 'image': [H, W], 'K': cfg['n_components'], 'ranks': 1,
               'gpus': 1, 'backend': 'nccl', 'timer': 'stream events', 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms,
               'norm2d_collectives_per_pass': vs[1].norm2d_collectives_per_pass,
               'dp_over_plain': (round(min(ms['dp']) / max(ms['plain']), 3), round(max(ms['dp']) / min(ms['plain']), 3)),
               'dp_slower_beyond_spread': min(ms['dp']) > max(ms['plain']),
               'dp_minus_plain_ms': round(sorted(ms['dp'])[len(ms['dp']) // 2] - sorted(ms['plain'])[len(ms['plain']) // 2], 3),
               'terms_loss_pnll_gnll_gent': terms}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del vs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
