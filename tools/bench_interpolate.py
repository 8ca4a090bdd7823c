#!/usr/bin/env python3
"""A latent sweep of S pairs of codes, T steps, n points per cloud, two ways.

* baseline   T calls of generate_many, one per step, on the step's codes with the SAME explicit draws (label words and normals): what
             the API offered before interpolate_many.  T routing launches, T FiLM launches, T head passes, T routed stack launches.
* sweep      one call of interpolate_many: one head pass on the S * T codes, one routing launch (gwtf_mixture_route_sweep), one
             FiLM launch, one routed stack launch over S * T rows -- with the same explicit draws, and with its own Philox draws.

The routed stack launch does the same arithmetic in both, so no speed-up of the device work is expected; what the sweep removes is
T - 1 routing, FiLM and head launches.  Before anything is timed the two paths are compared on the same draws.

Every variant runs eager and as a replayed graph.  The variants ALTERNATE inside each of `--windows` windows; a window times
`--calls` consecutive calls of one variant with stream events and reports ms per call; the figure of a variant is the median over
the windows, with the smallest and the largest window beside it.  Airplane decoder shape (K = 4 x 33 couplings, f = 37) and the
K = 16 configuration (18 couplings, f = 19), both G = 128.

    python tools/bench_interpolate.py [--out profiles/r31_interpolate.jsonl]     -> one JSON line per workload
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import go_with_the_flows_amd as gw  # noqa: E402
from go_with_the_flows_amd import models  # noqa: E402
from go_with_the_flows_amd.synth import load_synth_  # noqa: E402

DEV = 'cuda:0'
CFG = dict(train_mode='p_rnvp_mc_g_rnvp_vae', util_mode='generating', deterministic=False, pc_enc_init_n_channels=3,
           pc_enc_init_n_features=64, pc_enc_n_features=[128, 256, 512], g_latent_space_size=128, g_prior_n_flows=7,
           g_prior_n_features=128, g_posterior_n_layers=1, p_latent_space_size=3, p_prior_n_layers=1, p_decoder_n_flows=21,
           p_decoder_n_features=64, p_decoder_base_type='free', p_decoder_base_var=-3.9551, params_reduce_mode='depth_and_feature',
           weights_type='learned_weights')                    # config_generative_modeling_airplane.yaml; n_components per workload
WORKLOADS = {'airplane': 4, 'k16': 16}
TOL_COORD = 2e-5                                              # tests/conftest.py: absolute, coordinates, 12 couplings, |x| <= 6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, default=64)
    ap.add_argument('--steps', type=int, default=9)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    S, T, n, G = a.shapes, a.steps, a.points, CFG['g_latent_space_size']
    weights = [float(w) for w in np.float32(np.arange(1, T + 1) / (T + 1))]
    lines = []
    for name, K in WORKLOADS.items():
        m = models.Flow_Mixture_Model(**dict(CFG, n_components=K))
        load_synth_(m, 2000 + K)
        m = m.to(DEV).eval()
        dec = m.pc_decoder[0]
        gen = torch.Generator().manual_seed(K)
        ca, cb = torch.randn(S, G, generator=gen).to(DEV), torch.randn(S, G, generator=gen).to(DEV)
        rng = np.random.RandomState(K)
        ex = {'words': torch.from_numpy(rng.randint(0, 2**32, (S, n), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(DEV),
              'normals': torch.randn(S, 3, n, generator=gen).to(DEV)}
        w = torch.tensor(weights, device=DEV).view(1, T, 1)
        codes = ((1. - w) * ca.unsqueeze(1) + w * cb.unsqueeze(1)).transpose(0, 1).contiguous()          # (T, S, G)
        state = gw.make_state(K, DEV)
        out_b, out_s = torch.empty(T, S, 3, n, device=DEV), torch.empty(S, T, 3, n, device=DEV)

        def baseline():
            for t in range(T):
                m.generate_many(codes[t], n, state=state, explicit=ex, out=out_b[t])

        def sweep():
            m.interpolate_many(ca, cb, n, weights=weights, state=state, explicit=ex, out=out_s)

        def sweep_philox():
            m.interpolate_many(ca, cb, n, weights=weights, state=state, out=out_s)

        # ---- the same clouds on the same draws
        baseline()
        sweep()
        torch.cuda.synchronize()
        x_b, x_s = out_b.transpose(0, 1), out_s
        nan_b, nan_s = torch.isnan(x_b), torch.isnan(x_s)
        assert bool((nan_b == nan_s).all()), 'the two paths flag different points out of range'
        xmax = float(x_b[~nan_b].abs().max())
        tol = TOL_COORD * max(1.0, 3 * dec.n_flows / 12.0) * max(1.0, xmax / 6.0)                            # tests/conftest.py tol_at_depth
        diff = float((x_b - x_s)[~nan_b].abs().max())
        assert diff <= tol, f'{name}: baseline and sweep differ by {diff} (bound {tol})'
        same_bits = bool(torch.equal(x_b[~nan_b], x_s[~nan_b]))                                               # (before the buffers are reused)

        variants = {'baseline_eager': baseline, 'sweep_eager': sweep, 'sweep_philox_eager': sweep_philox}
        sweep_philox()                                                                                        # every variant has run eagerly once
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
        line = {'what': 'interpolate', 'workload': name, 'K': K, 'couplings': 3 * dec.n_flows, 'f': dec.f_n_features, 'S': S, 'T': T,
                'n': n, 'same_draws_max_abs_diff': diff, 'same_draws_bit_equal': same_bits,
                'same_draws_bound': tol, 'nan_points': int(nan_b.sum())}
        for k, v in ms.items():
            line[k + '_ms'] = round(float(np.median(v)), 4)
            line[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        line['timed_by'] = (f'median of {a.windows} windows of {a.calls} calls per variant, variants alternating, stream events around '
                            f'each window, after {a.warmup} calls each; one call = the whole sweep of S x T clouds')
        line['device'] = torch.cuda.get_device_name(0)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del graphs, variants, m
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
