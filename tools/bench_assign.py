#!/usr/bin/env python3
"""Per-point component posteriors of B observed clouds of n points, two ways.

* composed   what the API offered before assign_many: the batched density launch (MixtureStack.forward_all), then torch operators
             for lp (K, B, n), logsumexp, argmax, the label's responsibility and a bincount per shape.
* assign     one call of Flow_Mixture_Model.assign_many on explicit codes: the same density launch, then ONE launch of
             gwtf_mixture_assign (csrc/gwtf_assign.hip).

The density launch is the same in both and dominates both; what assign_many removes is the torch operator chain behind it.  Before
anything is timed the two paths are compared and the figures recorded (largest log-density difference, share of equal labels): both
are float32 evaluations of the same formula, the parity tests are tests/test_gpu_assign.py.

Both run eager and as a replayed graph.  The variants ALTERNATE inside each of `--windows` windows; a window times `--calls`
consecutive calls of one variant with stream events and reports ms per call; the figure of a variant is the median over the windows,
with the smallest and the largest window beside it.  The assignment launch ALONE (on z / logdet held fixed) is timed the same way and
set against its byte model, (24 K + 12) B per point -- z and logdet read once, log-density, label and confidence written.  Airplane
decoder shape (K = 4 x 33 couplings, f = 37) and the K = 16 configuration (18 couplings, f = 19), both G = 128.  GPU box only.

    python tools/bench_assign.py [--out profiles/r32_assign.jsonl]     -> one JSON line per workload
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from go_with_the_flows_amd import _lib, models  # noqa: E402
from go_with_the_flows_amd.synth import load_synth_  # noqa: E402

DEV = 'cuda:0'
CFG = dict(train_mode='p_rnvp_mc_g_rnvp_vae', util_mode='generating', deterministic=False, pc_enc_init_n_channels=3,
           pc_enc_init_n_features=64, pc_enc_n_features=[128, 256, 512], g_latent_space_size=128, g_prior_n_flows=7,
           g_prior_n_features=128, g_posterior_n_layers=1, p_latent_space_size=3, p_prior_n_layers=1, p_decoder_n_flows=21,
           p_decoder_n_features=64, p_decoder_base_type='free', p_decoder_base_var=-3.9551, params_reduce_mode='depth_and_feature',
           weights_type='learned_weights')                    # config_generative_modeling_airplane.yaml; n_components per workload
WORKLOADS = {'airplane': 4, 'k16': 16}
STREAM_TB_PER_S = (5.0, 6.0)                                  # the streaming rate the byte model is set against


def window(fn, calls):
    """ms per call of `calls` consecutive calls, stream events around them."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def captured(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def base_rows(m, codes, K):
    B, P = codes.shape[0], m.p_latent_space_size
    mu, lv = m._base_gaussian(codes)
    return tuple(t.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P).contiguous().float() for t in (mu, lv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, default=64)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    B, n, G = a.shapes, a.points, CFG['g_latent_space_size']
    lines = []
    for name, K in WORKLOADS.items():
        m = models.Flow_Mixture_Model(**dict(CFG, n_components=K))
        load_synth_(m, 2000 + K)
        m = m.to(DEV).eval()
        dec = m.pc_decoder[0]
        gen = torch.Generator().manual_seed(K)
        clouds = (0.3 * torch.randn(B, 3, n, generator=gen)).to(DEV)
        codes = torch.randn(B, G, generator=gen).to(DEV)
        half_log2pi3 = 1.5 * math.log(2.0 * math.pi)
        held = {}

        @torch.no_grad()
        def composed():
            logits = m.get_weights(codes).contiguous().float()
            mu0, lv0 = base_rows(m, codes, K)
            z, logdet = m.mixture_stack().forward_all(clouds, codes, mode='inverse')
            logw = torch.log(torch.exp(logits)) - torch.logsumexp(logits, dim=-1, keepdim=True)                  # losses.py:101-104
            q = ((lv0[..., None] + logdet) + (z - mu0[..., None]) ** 2 / torch.exp(lv0[..., None])).sum(2)
            lp = -0.5 * q - half_log2pi3 + logw.t()[:, :, None]                                                  # (K, B, n)
            dens = torch.logsumexp(lp, dim=0)
            best, labels = lp.max(0)
            conf = torch.exp(best - dens)
            counts = torch.zeros(B, K, device=DEV, dtype=torch.int64).scatter_add_(1, labels, torch.ones_like(labels))    # bincount per shape
            held['composed'] = (dens, labels, conf, counts)

        def assign():
            held['assign'] = m.assign_many(clouds, codes=codes, out=held.get('assign'))

        # ---- the same answers
        composed()
        assign()
        torch.cuda.synchronize()
        dens_c, labels_c, _, counts_c = held['composed']
        res = held['assign']
        with torch.no_grad():
            z, logdet = m.mixture_stack().forward_all(clouds, codes, mode='inverse')
            mu0, lv0 = base_rows(m, codes, K)
            logits = m.get_weights(codes).contiguous().float()
        finite = torch.isfinite(dens_c) & torch.isfinite(res['log_density'])
        diff = float((dens_c - res['log_density'])[finite].abs().max())
        scale = float(dens_c[finite].abs().max())
        agree = float((labels_c.int() == res['labels'])[finite].float().mean())
        counts_same = bool(torch.equal(counts_c.int(), res['counts'])) if agree == 1.0 else None

        out_alone = _lib.mixture_assign(z, logdet, mu0, lv0, logits)

        def launch_alone():
            _lib.mixture_assign(z, logdet, mu0, lv0, logits, out=out_alone)

        variants = {'composed_eager': composed, 'assign_eager': assign, 'launch_alone_eager': launch_alone}
        for fn in variants.values():
            fn()                                                                                              # every variant has run eagerly
        torch.cuda.synchronize()
        graphs = {k.replace('eager', 'graph'): captured(fn) for k, fn in list(variants.items())}
        variants.update({k: g.replay for k, g in graphs.items()})
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.windows):
            for k, fn in variants.items():                                                                    # alternating
                ms[k].append(window(fn, a.calls))
        bytes_moved = (24 * K + 12) * B * n
        line = {'what': 'assign', 'workload': name, 'K': K, 'couplings': 3 * dec.n_flows, 'f': dec.f_n_features, 'B': B, 'n': n,
                'log_density_max_abs_diff': diff, 'log_density_max_abs': scale, 'labels_agree': agree, 'counts_equal': counts_same,
                'non_finite_points': int((~finite).sum())}
        for k, v in ms.items():
            line[k + '_ms'] = round(float(np.median(v)), 4)
            line[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        alone = line['launch_alone_graph_ms']
        line['launch_bytes'] = bytes_moved
        line['launch_byte_model_us'] = [round(bytes_moved / (r * 1e12) * 1e6, 2) for r in reversed(STREAM_TB_PER_S)]
        line['launch_alone_graph_TB_per_s'] = round(bytes_moved / (alone * 1e-3) / 1e12, 3)
        line['timed_by'] = (f'median of {a.windows} windows of {a.calls} calls per variant, variants alternating, stream events around '
                            f'each window, after {a.warmup} calls each; launch_alone = the memset of counts / invalid and the assignment '
                            f'kernel on fixed z / logdet')
        line['device'] = torch.cuda.get_device_name(0)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del graphs, variants, m, held, z, logdet
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
