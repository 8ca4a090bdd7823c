#!/usr/bin/env python3
"""One training step of the single-view-reconstruction model (tests/golden/contract_svr.json svr_cfg = configs/config_SVR.yaml:
K = 4 decoders, G = 512, 2500 points per cloud, 224 x 224 four-channel images, ResNet-18 image encoder on the library modules) on one
MI355X, three ways in ONE process, alternated:

  list     model(g, p, images) -> lists -> Flow_Mixture_Loss -> backward -> optimizer.step()      (the reference's loop,
           training.py:206-232; the only way to train this model before forward_fused took images)
  fused    forward_fused(g, p, images=...) -> Flow_Mixture_Loss.fused -> backward -> optimizer.step()
  graphed  training.GraphedTrainStep(..., images_example=...)

at B = 128 (the config's batch size) and B = 32.  Timing: host clock around --steps steps ending in a device synchronise, after
--warmup steps per variant, --repeats times per variant (the spread).  Before the timing each variant takes ONE step from the same
initial state with the same injected reparameterisation noise: its four loss terms go into the record (the three must agree).

    python tools/bench_svr_train.py [--batches 128,32] [--steps 50] [--warmup 10] [--repeats 3] [--variants list,fused,graphed]
                                    [--out profiles/r21_svr_train.jsonl]
    python tools/bench_svr_train.py --profile-steps 20 --batches 128        # graphed variant only, for rocprofv3 --kernel-trace
    python tools/bench_svr_train.py --profile-encoder 20 --batches 128      # the image encoder alone (library forward + backward)
    python tools/bench_svr_train.py --encoder-norm library,hip --variants graphed --out profiles/r23_svr_norm.jsonl
    python tools/bench_svr_train.py --profile-encoder 20 --batches 128 --encoder-norm hip
    python tools/bench_svr_train.py --encoder-norm hip --encoder-conv library,hip --variants graphed --out profiles/r27_svr_conv.jsonl

--encoder-norm: the values of ResNet.train_norm to measure ('library': BatchNorm2d / ReLU / add / max-pool on the library modules;
'hip': the fused kernels of csrc/gwtf_norm2d.hip).  With more than one value every variant is built once per value and all of them
are alternated in the one call; the profile programs take the first value.  norm2d_byte_model gives the bytes the fused kernels
must move per pass, from the shapes alone: kernel time from a trace divides into it.

--encoder-conv: the values of ResNet.train_conv to measure ('library': F.conv2d; 'hip': csrc/gwtf_conv2d.hip, which needs
--encoder-norm hip: a 'hip' convolution is paired with the 'hip' norm only).  Alternated in the one call like the norms; the record
key of a variant on the HIP convolutions ends in '+conv'.

The profile programs are the programs of two `rocprofv3 --kernel-trace --stats` runs; tools/svr_train_split.py turns their kernel_stats.csv
files into the split of a step's kernel time between the image encoder's library kernels and everything else.
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from go_with_the_flows_amd import models, optim  # noqa: E402
from go_with_the_flows_amd.synth import calibrate_image_encoder, load_image_encoder_stats_, load_synth_, synth_images, synth_inputs  # noqa: E402
from go_with_the_flows_amd.training import GraphedTrainStep  # noqa: E402

VARIANTS = ('list', 'fused', 'graphed')
NORMS = ('library', 'hip')
CONVS = ('library', 'hip')


def norm2d_byte_model(B, H, W):
    """Bytes the four kernel families of csrc/gwtf_norm2d.hip move in one forward + backward pass over the 20 BatchNorm2d layers of
    the ResNet-18 encoder on (B, 4, H, W) images, counted from shapes (float32 activations, uint8 pool offsets; per-channel vectors
    and partials left out).  Per layer of E elements (Ep pooled ones), reads + writes:
        statistics        x                                             4 E
        forward apply     x (+ residual) -> y                           8 E (12 E);  pool: x -> pooled y, offsets    4 E + 5 Ep
        backward sums     x, dy (, saved y with ReLU)                   8 E (12 E);  pool: x, pooled dy, offsets     4 E + 5 Ep
        backward apply    the same reads -> dx (+ d_residual)           +4 E (+8 E); pool                            8 E + 5 Ep
    Returns {'activations', 'stats', 'apply_fwd', 'sums_bwd', 'apply_bwd', 'total'}."""
    conv = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    h, w = conv(H, 7, 2, 3), conv(W, 7, 2, 3)
    out = {'activations': 0, 'stats': 0, 'apply_fwd': 0, 'sums_bwd': 0, 'apply_bwd': 0}

    def layer(E, relu=True, residual=False, Ep=0):
        out['activations'] += E
        out['stats'] += 4 * E
        if Ep:
            out['apply_fwd'] += 4 * E + 5 * Ep
            out['sums_bwd'] += 4 * E + 5 * Ep
            out['apply_bwd'] += 8 * E + 5 * Ep
            return
        reads = 8 * E + (4 * E if relu else 0)
        out['apply_fwd'] += (12 if residual else 8) * E
        out['sums_bwd'] += reads
        out['apply_bwd'] += reads + (8 if residual else 4) * E

    hp, wp = conv(h, 3, 2, 1), conv(w, 3, 2, 1)
    layer(B * 64 * h * w, Ep=B * 64 * hp * wp)                      # stem
    h, w = hp, wp
    for C, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        h, w = conv(h, 3, stride, 1), conv(w, 3, stride, 1)
        E = B * C * h * w
        for block in range(2):
            layer(E)                                                # bn1 -> relu
            layer(E, residual=True)                                 # bn2 -> add -> relu
        if stride != 1:
            layer(E, relu=False)                                    # the downsample branch
    out['total'] = out['stats'] + out['apply_fwd'] + out['sums_bwd'] + out['apply_bwd']
    return out


def config():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'contract_svr.json')))['svr_cfg']


def make_optimizer(model, cfg):
    return optim.Adam(model.parameters(), lr=cfg['max_lr'], betas=(cfg['beta1'], cfg['max_beta2']), weight_decay=cfg['wd'], amsgrad=True)


class Variant:
    """One way of taking a step, on its own copy of the model (same initial state) with its own optimiser."""

    def __init__(self, kind, base_model, cfg, batch, noise=None, norm='library', conv='library'):
        self.kind, self.batch, self.norm, self.conv = kind, batch, norm, conv
        self.key = (kind if norm == 'library' else f'{kind}/{norm}') + ('' if conv == 'library' else '+conv')
        self.model = copy.deepcopy(base_model)
        self.model.img_encoder.train_norm = norm
        self.model.img_encoder.train_conv = conv
        if noise is not None:
            self.model.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
        self.crit = models.Flow_Mixture_Loss(**cfg)
        self.opt = make_optimizer(self.model, cfg)
        self.graph = GraphedTrainStep(self.model, self.crit, self.opt, batch[0], batch[1], images_example=batch[2]) \
            if kind == 'graphed' else None

    def step(self):
        g, p, imgs = self.batch
        if self.kind == 'graphed':
            return self.graph(g, p, imgs)
        self.opt.zero_grad(set_to_none=True)
        if self.kind == 'list':
            enc, dec, logits = self.model(g, p, imgs)
            terms = self.crit(enc, dec, logits)
        else:
            enc, dec = self.model.forward_fused(g, p, images=imgs)
            terms = self.crit.fused(enc, dec)
        terms[0].backward()
        self.opt.step()
        return tuple(t.detach() for t in terms)

    def timed(self, steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,32')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--variants', default=','.join(VARIANTS), help='comma-separated subset of list,fused,graphed')
    ap.add_argument('--encoder-norm', default='library', help='comma-separated subset of library,hip (ResNet.train_norm)')
    ap.add_argument('--encoder-conv', default='library', help='comma-separated subset of library,hip (ResNet.train_conv); hip is '
                                                              'measured with --encoder-norm hip only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_svr_train.jsonl'))
    ap.add_argument('--profile-steps', type=int, default=0, metavar='N',
                    help='run N steps of the graphed variant at the first batch size and exit (the program of a kernel trace)')
    ap.add_argument('--profile-encoder', type=int, default=0, metavar='N',
                    help='run N train-mode forward + backward passes of the image encoder ALONE (library modules) at the first batch '
                         'size and exit: the kernels a trace of the whole step owes to the encoder')
    args = ap.parse_args()
    kinds = [k for k in args.variants.split(',') if k]
    assert all(k in VARIANTS for k in kinds), kinds
    norms = [n for n in args.encoder_norm.split(',') if n]
    assert norms and all(n in NORMS for n in norms), norms
    convs = [c for c in args.encoder_conv.split(',') if c]
    assert convs and all(c in CONVS for c in convs), convs
    paths = [(n, c) for n in norms for c in convs if c == 'library' or n == 'hip']
    assert paths, "--encoder-conv hip needs --encoder-norm hip"
    assert torch.cuda.is_available(), 'bench_svr_train needs a HIP device'
    dev, cfg = 'cuda:0', config()
    n_points, (H, W) = cfg['cloud_size'], cfg['image_size']
    base = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(base, 2310, output_gain=0.3)
    # synth_state draws the prior flow's output layers at O(1) log-variance per coupling; 14 couplings at G = 512 compound that to
    # |z| ~ 1e10 and a gnll of 1e22 in which the variants' rounding differences are all one sees.  Scaled after the draw (what
    # output_gain does for the decoders) the flow is near the identity, as at the reference's initialisation (weight_std 0.01), and the
    # four terms are comparable; the step's work does not depend on the values.
    with torch.no_grad():
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
        if args.profile_encoder:
            enc = base.img_encoder
            enc.train_norm, enc.train_conv = paths[0]
            for _ in range(args.profile_encoder):
                enc.zero_grad(set_to_none=True)
                enc(imgs).square().mean().backward()
            torch.cuda.synchronize()
            print(json.dumps({'bench': 'svr_encoder_profile', 'B': B, 'steps': args.profile_encoder, 'encoder_norm': paths[0][0],
                              'encoder_conv': paths[0][1],
                              'norm2d_bytes_per_pass': norm2d_byte_model(B, H, W)}), flush=True)
            return
        if args.profile_steps:
            v = Variant('graphed', base, cfg, batch, norm=paths[0][0], conv=paths[0][1])
            for _ in range(args.profile_steps):
                v.step()
            torch.cuda.synchronize()
            print(json.dumps({'bench': 'svr_train_profile', 'B': B, 'steps': args.profile_steps}), flush=True)
            return
        noise = torch.randn(B, cfg['g_latent_space_size'], generator=torch.Generator().manual_seed(2323)).to(dev)
        terms = {}
        for kind in kinds:                      # one step each from the same state with the same noise: the same four numbers
            for norm, conv in paths:
                v = Variant(kind, base, cfg, batch, noise, norm, conv)
                terms[v.key] = [float(t) for t in v.step()]
                del v
        torch.cuda.empty_cache()
        vs = [Variant(kind, base, cfg, batch, norm=norm, conv=conv) for kind in kinds for norm, conv in paths]
        for v in vs:
            for _ in range(args.warmup):
                v.step()
        ms = {v.key: [] for v in vs}
        for _ in range(args.repeats):           # alternated: a drift of the machine hits every variant alike
            for v in vs:
                ms[v.key].append(round(v.timed(args.steps), 3))
        rec = {'bench': 'svr_train_step', 'B': B, 'n_points': n_points, 'image': [H, W], 'K': cfg['n_components'],
               'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms, 'terms_loss_pnll_gnll_gent': terms}
        if 'graphed' in ms and 'graphed/hip' in ms:
            rec['encoder_norm'] = norms
            rec['graphed_library_over_hip'] = (round(min(ms['graphed']) / max(ms['graphed/hip']), 3),
                                               round(max(ms['graphed']) / min(ms['graphed/hip']), 3))
            rec['hip_faster_beyond_spread'] = max(ms['graphed/hip']) < min(ms['graphed'])
            rec['hip_slower_beyond_spread'] = min(ms['graphed/hip']) > max(ms['graphed'])
        if 'graphed/hip' in ms and 'graphed/hip+conv' in ms:       # both on the fused norm kernels; only the convolutions differ
            lib, hip = ms['graphed/hip'], ms['graphed/hip+conv']
            rec['encoder_conv'] = convs
            rec['graphed_conv_library_over_hip'] = round(min(lib) / max(hip), 3), round(max(lib) / min(hip), 3)
            rec['hip_conv_faster_beyond_spread'] = max(hip) < min(lib)
            rec['hip_conv_slower_beyond_spread'] = min(hip) > max(lib)
        if 'list' in ms and 'graphed' in ms:
            rec['list_over_graphed'] = round(min(ms['list']) / max(ms['graphed']), 3), round(max(ms['list']) / min(ms['graphed']), 3)
            rec['graphed_faster_beyond_spread'] = max(ms['graphed']) < min(ms['list'])
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del vs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
