#!/usr/bin/env python3
"""Producing the generated clouds of the generation evaluation: S latent codes -> S clouds of n points, per call, three ways.

* sample_many            components drawn with np.random.choice shape by shape (one device-to-host copy of the logits per shape), the
                         padded layout built on the host, scatter + partitioned stack launch + gather
* generate_many          components and base samples drawn on the device, routing launch + routed stack launch, no host round trip
* generate_many (graph)  the same call captured once with torch.cuda.graph and replayed

Two clocks per call: the host clock around call + synchronize (what a loop that needs the clouds pays) and stream events around the
call (what the device is busy).  Every figure is the median of `--calls` calls after `--warmup` calls, on the airplane decoder shape
(K = 4 x 33 couplings, f = 37) and the K = 16 configuration (18 couplings, f = 19), both G = 128, for S in {1, 32, 64}, n = 2048.

    python tools/bench_generate.py [--calls 30] [--warmup 5] [--out profiles/r20_generate.jsonl]     -> one JSON line per point
"""
import argparse
import json
import os
import sys
import time

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


def timed(fn, calls, warmup):
    """-> (median host ms of call + synchronize, median stream-event ms of the call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    host, device = [], []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - w0) * 1e3)
        device.append(t0.elapsed_time(t1))
    return float(np.median(host)), float(np.median(device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shapes', type=int, nargs='*', default=[1, 32, 64])
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    assert a.calls >= 20, 'medians of fewer than 20 calls are not reported'
    n, lines = a.points, []
    for name, K in WORKLOADS.items():
        m = models.Flow_Mixture_Model(**dict(CFG, n_components=K))
        load_synth_(m, 2000 + K)
        m = m.to(DEV).eval()
        dec = m.pc_decoder[0]
        for S in a.shapes:
            g = torch.randn(S, CFG['g_latent_space_size'], generator=torch.Generator().manual_seed(S)).to(DEV)
            np.random.seed(S)
            state = gw.make_state(S, DEV)
            out = torch.empty(S, 3, n, device=DEV)
            t_many = timed(lambda: m.sample_many(g, n), a.calls, a.warmup)
            t_eager = timed(lambda: m.generate_many(g, n, state=state, out=out), a.calls, a.warmup)
            assert bool(torch.isfinite(out).all())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                m.generate_many(g, n, state=state, out=out)
            t_graph = timed(graph.replay, a.calls, a.warmup)
            assert bool(torch.isfinite(out).all())
            del graph
            lines.append({'what': 'generate', 'workload': name, 'K': K, 'couplings': 3 * dec.n_flows, 'f': dec.f_n_features, 'S': S,
                          'n': n, 'sample_many_host_ms': round(t_many[0], 4), 'sample_many_event_ms': round(t_many[1], 4),
                          'generate_many_host_ms': round(t_eager[0], 4), 'generate_many_event_ms': round(t_eager[1], 4),
                          'generate_many_graph_host_ms': round(t_graph[0], 4), 'generate_many_graph_event_ms': round(t_graph[1], 4),
                          'host_ratio_sample_many_over_generate_many': round(t_many[0] / t_eager[0], 2),
                          'host_ratio_sample_many_over_graph': round(t_many[0] / t_graph[0], 2),
                          'timed_by': f'median of {a.calls} calls after {a.warmup}; host = perf_counter around call + synchronize, '
                                      'event = stream events around the call', 'device': torch.cuda.get_device_name(0)})
            print(json.dumps(lines[-1]), flush=True)
        del m
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
