#!/usr/bin/env python3
"""Time the per-batch metric loop of the reconstruction / autoencoding evaluation on device-resident clouds of the config_SVR size
(2500 points): the reference-shaped loop on the library's existing functions (tests/recon_ref.py hand_loop: a transposed copy of both
clouds, distChamferCUDA, emd_approx, f_score once per threshold, an .item() read per metric and batch) against the one-call path
(metrics.clouds_to_eval_frame + metrics.paired_metrics into a device meter, ONE read after the last batch).  The model's own work is
the same on both sides and is left out.  The two paths alternate inside one process, repetition by repetition, after a warm-up of
each; every repetition runs --batches batches and is timed twice over, by the host clock around a synchronised call and by stream
events; figures are minimum / median / maximum over the repetitions, per batch.  The paired Chamfer launch alone is timed next to
nn_distance at 64 x 2048 points (stream events around --kernel-launches launches, divided).  GPU box only.

    python tools/bench_recon_eval.py [--batch-sizes 1,32,128] [--thresholds 1,3] [--points 2500] [--reps 7] [--out profiles/r26_recon_eval.jsonl]

Appends one JSON line per case to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import recon_ref  # noqa: E402
from go_with_the_flows_amd import _lib, metrics  # noqa: E402

THRESHOLDS = (0.0001, 0.001, 0.01)


def timed(fn):
    """(host ms around a synchronised call, stream-event ms) of one call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, start.elapsed_time(stop)


def spread(xs, per):
    xs = [x / per for x in xs]
    return {'min': round(min(xs), 4), 'median': round(statistics.median(xs), 4), 'max': round(max(xs), 4), 'n': len(xs)}


def kernel_lines(launches, reps):
    """The paired Chamfer launch and nn_distance on the same 64 pairs of 2048 points, per launch."""
    g = torch.Generator(device='cuda').manual_seed(1)
    a = torch.rand(64, 2048, 3, device='cuda', generator=g) - 0.5
    b = torch.rand(64, 2048, 3, device='cuda', generator=g) - 0.5
    L = _lib.lib()
    partials = torch.empty(2 * 64 * L.gwtf_chamfer_paired_partials(2048, 2048) * metrics.PAIRED_WORDS, device='cuda')
    thr, _ = metrics._thr_array((0.001,))

    def paired():
        for _ in range(launches):
            metrics._chamfer_paired_launch(L, a, b, partials, thr, 64, 2048, 2048)

    def nnd():
        for _ in range(launches):
            metrics.nn_distance_raw(a, b)

    paired(), nnd()
    p_ms, n_ms = [], []
    for _ in range(reps):
        p_ms.append(timed(paired)[1])
        n_ms.append(timed(nnd)[1])
    return {'case': 'paired Chamfer launch vs nn_distance, 64 x 2048 points, stream events over %d launches' % launches,
            'device': torch.cuda.get_device_name(0), 'chamfer_paired_ms': spread(p_ms, launches), 'nn_distance_ms': spread(n_ms, launches)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch-sizes', default='1,32,128')
    ap.add_argument('--thresholds', default='1,3', help='numbers of F1 thresholds')
    ap.add_argument('--points', type=int, default=2500)
    ap.add_argument('--batches', type=int, default=0, help='batches per repetition (0: 64 at B = 1 down to 4 at B >= 128)')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--kernel-launches', type=int, default=50)
    ap.add_argument('--out', default=os.path.join('profiles', 'r26_recon_eval.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_recon_eval: no HIP device; this measurement has no CPU form')
    lines = [kernel_lines(a.kernel_launches, a.reps)]
    print(json.dumps(lines[0]), flush=True)
    n = a.points
    for B in (int(v) for v in a.batch_sizes.split(',')):
        nb = a.batches or max(4, min(64, 256 // B))
        g = torch.Generator(device='cuda').manual_seed(B)
        batches = [(torch.rand(B, 3, n, device='cuda', generator=g) - 0.5, torch.rand(B, 3, n, device='cuda', generator=g) - 0.5)
                   for _ in range(nb)]
        for T in (int(v) for v in a.thresholds.split(',')):
            thresholds = THRESHOLDS[:T]
            for emd in (True, False):
                def baseline():
                    return recon_ref.hand_loop(batches, thresholds, cd=True, emd=emd, f1=True)

                def one_call():
                    meter = metrics.new_meter(T, 'cuda')
                    for gen, ref in batches:
                        x, y = metrics.clouds_to_eval_frame(gen, ref)
                        metrics.paired_metrics(x, y, thresholds, cd=True, emd=emd, meter=meter)
                    return meter.tolist()                                            # the one read

                want, got = baseline(), one_call()                                   # warm-up of both, and the two answers
                diff = {'cd_rel': abs(got[1] / got[0] - want['cd']) / want['cd']}
                if emd:
                    diff['emd_rel'] = abs(got[2] / got[0] - want['emd']) / want['emd']
                base_host, base_ev, new_host, new_ev = [], [], [], []
                for _ in range(a.reps):                                              # alternating: drift hits both alike
                    h, e = timed(baseline)
                    base_host.append(h), base_ev.append(e)
                    h, e = timed(one_call)
                    new_host.append(h), new_ev.append(e)
                line = {'case': 'paired evaluation loop, per batch', 'B': B, 'points': n, 'thresholds': T, 'emd': emd,
                        'batches_per_rep': nb, 'device': torch.cuda.get_device_name(0),
                        'baseline_host_ms': spread(base_host, nb), 'baseline_event_ms': spread(base_ev, nb),
                        'one_call_host_ms': spread(new_host, nb), 'one_call_event_ms': spread(new_ev, nb),
                        'host_ratio_of_medians': round(statistics.median(base_host) / statistics.median(new_host), 2),
                        'agreement': {k: float('%.3g' % v) for k, v in diff.items()}}
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        for line in lines:
            fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
