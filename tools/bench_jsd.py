#!/usr/bin/env python3
"""Time evaluation.JSD on two cloud sets held on the device: the device path (metrics.voxel_occupancy + metrics.jsd_from_counts,
device time by stream events) against the host path on the same inputs (numpy searchsorted / add.at and scipy's entropy, INCLUDING
the device-to-host copy of both sets, which is what a caller with device-resident clouds pays; wall clock around a synchronised
call).  The two paths alternate inside one process, repetition by repetition, after a warm-up of each; every figure is reported as
minimum / median / maximum over the repetitions.  The occupancy kernel alone is timed too and turned into bytes read per second
(12 B per point).  GPU box only.

    python tools/bench_jsd.py [--sizes 1000x2048,10000x2048] [--reps 7] [--host-reps 3] [--out profiles/r25_jsd.jsonl]

Appends one JSON line per size to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from go_with_the_flows_amd import evaluation as ev  # noqa: E402
from go_with_the_flows_amd import metrics  # noqa: E402


def event_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(xs):
    return {'min': round(min(xs), 4), 'median': round(statistics.median(xs), 4), 'max': round(max(xs), 4), 'n': len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000x2048,10000x2048')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=3, help='host repetitions (each alternates with a device one)')
    ap.add_argument('--out', default=os.path.join('profiles', 'r25_jsd.jsonl'))
    a = ap.parse_args()
    lines = []
    for size in a.sizes.split(','):
        S, n = (int(v) for v in size.split('x'))
        g = torch.Generator(device='cuda').manual_seed(0)
        gen = (torch.randn(S, n, 3, device='cuda', generator=g) * 0.2).contiguous()
        ref = (torch.randn(S, n, 3, device='cuda', generator=g) * 0.2).contiguous()

        def device_path():
            return ev.JSD(gen, ref, warning=False)

        def host_path():
            return ev.JSD(gen.cpu().numpy(), ref.cpu().numpy(), warning=False)

        out = torch.zeros(28, 28, 28, dtype=torch.int64, device='cuda')

        def kernel_alone():
            metrics.voxel_occupancy(gen, out=out)

        d, h = float(device_path()), float(host_path())                 # warm-up of both, and the two answers
        kernel_alone()
        dev_ms, host_ms, kern_ms = [], [], []
        for rep in range(a.reps):                                        # alternating: drift hits both alike
            dev_ms.append(event_ms(device_path))
            if rep < a.host_reps:
                host_ms.append(wall_ms(host_path))
            kern_ms.append(event_ms(kernel_alone))
        line = {'case': 'JSD, device path vs host path', 'clouds': S, 'points': n, 'device': torch.cuda.get_device_name(0),
                'device_ms': spread(dev_ms), 'host_ms_with_copy': spread(host_ms), 'occupancy_kernel_ms': spread(kern_ms),
                'occupancy_GB_per_s_at_min': round(12.0 * S * n / min(kern_ms) / 1e6, 1),
                'ratio_of_minima': round(min(host_ms) / min(dev_ms), 1), 'abs_diff': abs(d - h), 'jsd': d}
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        for line in lines:
            fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
