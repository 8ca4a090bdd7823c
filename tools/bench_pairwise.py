#!/usr/bin/env python3
"""Time the all-pairs generation metrics (evaluation.generation_metrics) against the per-row host loop
(evaluation.compute_all_metrics, batch_size=60, accelerated_cd=True -- called once per threshold, as evaluating.py:212-216 does),
and the directed Chamfer kernel against nn_distance, in one process.  Minimum of 5 after a warm-up.  GPU box only.

    python tools/bench_pairwise.py [--clouds 128] [--points 2048] [--out profiles/r18_pairwise.jsonl] [--skip-emd]

Appends one JSON line per measurement to --out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from go_with_the_flows_amd import evaluation as ev  # noqa: E402
from go_with_the_flows_amd import metrics  # noqa: E402


def best_of(fn, reps=5):
    fn(); torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=128)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--out', default=os.path.join('profiles', 'r18_pairwise.jsonl'))
    ap.add_argument('--skip-emd', action='store_true')
    a = ap.parse_args()
    S, n = a.clouds, a.points
    g = torch.Generator(device='cuda').manual_seed(0)
    smp = torch.randn(S, n, 3, device='cuda', generator=g) * 0.25
    ref = torch.randn(S, n, 3, device='cuda', generator=g) * 0.25
    lines = []

    def record(**kw):
        kw.update(clouds=S, points=n, device=torch.cuda.get_device_name(0))
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    thresholds = (0.005, 0.01)
    configs = [('cd+f1, 2 thresholds', thresholds, dict(cd_option=True, f1_option=True)),
               ('cd+f1, 1 threshold', thresholds[:1], dict(cd_option=True, f1_option=True))]
    if not a.skip_emd:
        configs.append(('cd+emd', thresholds[:1], dict(cd_option=True, emd_option=True)))
    for name, thr, opts in configs:
        new = best_of(lambda: ev.generation_metrics(smp, ref, thr, **opts))
        old = best_of(lambda: [ev.compute_all_metrics(smp, ref, 60, accelerated_cd=True, f1_threshold=t, **opts) for t in thr])
        record(case='generation_metrics vs compute_all_metrics', config=name, generation_metrics_ms=round(new, 3),
               compute_all_metrics_ms=round(old, 3), ratio=round(old / new, 3))

    # kernel against kernel: evaluations (one squared distance + running minimum) per second
    b = 64
    x, y = smp[:b].contiguous(), ref[:b].contiguous()
    ms = best_of(lambda: metrics.nn_distance_raw(x, y), 20)
    record(case='nn_distance_raw', b=b, ms=round(ms, 4), gevals_per_s=round(2 * b * n * n / ms / 1e6, 1))
    for nq in (b, S):
        q, t = smp[:nq].contiguous(), ref[:nq].contiguous()
        ms = best_of(lambda: metrics.chamfer_directed(q, t, thresholds), 20)
        record(case='chamfer_directed', nq=nq, nt=nq, ms=round(ms, 4), gevals_per_s=round(nq * nq * n * n / ms / 1e6, 1))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        for kw in lines:
            fh.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
