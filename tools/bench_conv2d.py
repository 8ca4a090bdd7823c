#!/usr/bin/env python3
"""The convolutions of the ResNet-18 image encoder in train mode, layer by layer, on one MI355X: csrc/gwtf_conv2d.hip
(conv2d.Conv2dFn) against the library (F.conv2d and torch.autograd.grad on contiguous NCHW float32, which is how the encoder calls
them), forward, backward_input and backward_weight timed SEPARATELY.

The 20 convolutions of resnet18 on 224 x 224 four-channel images have 11 distinct geometries (the stem; per stage the 3 x 3 / stride 1
body, and from layer2 on the 3 x 3 / stride 2 entry and the 1 x 1 / stride 2 downsample); each is measured at B = 128 and B = 32.
The stem has no backward_input: its input is the image.

Timing: stream events around --iters back-to-back calls of ONE pass on ONE side, after --warmup calls; --repeats such measurements
per side, the two sides ALTERNATED so a drift of the machine hits both alike.  Launch gaps between the calls are inside the number
(they are inside a training step's too, unless it is graphed).  Per layer and pass the record has every measurement, the median, the
spread (min, max), TFLOP/s of the median by the nominal count 2 * N * Ho * Wo * Cout * Cin * k * k, the HIP side's fraction of the
157 TFLOP/s peak of v_mfma_f32_16x16x4_f32, and which side won ('tie' when the ranges overlap).  A closing line per batch size sums
the medians over the 20 convolutions (count x median).

    python tools/bench_conv2d.py [--batches 128,32] [--iters 5] [--warmup 3] [--repeats 5] [--out profiles/r27_conv2d.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from go_with_the_flows_amd import conv2d as c2d  # noqa: E402

PEAK_TFLOPS = 157.0
PASSES = ('forward', 'backward_input', 'backward_weight')
# name, Cin, H = W of the input, Cout, k, stride, how many of the 20 convolutions have this geometry
GEOMETRIES = (
    ('stem_4x224_64_k7s2', 4, 224, 64, 7, 2, 1),
    ('layer1_64x56_64_k3s1', 64, 56, 64, 3, 1, 4),
    ('layer2_64x56_128_k3s2', 64, 56, 128, 3, 2, 1),
    ('layer2_64x56_128_k1s2', 64, 56, 128, 1, 2, 1),
    ('layer2_128x28_128_k3s1', 128, 28, 128, 3, 1, 3),
    ('layer3_128x28_256_k3s2', 128, 28, 256, 3, 2, 1),
    ('layer3_128x28_256_k1s2', 128, 28, 256, 1, 2, 1),
    ('layer3_256x14_256_k3s1', 256, 14, 256, 3, 1, 3),
    ('layer4_256x14_512_k3s2', 256, 14, 512, 3, 2, 1),
    ('layer4_256x14_512_k1s2', 256, 14, 512, 1, 2, 1),
    ('layer4_512x7_512_k3s1', 512, 7, 512, 3, 1, 3),
)


def make_calls(side, x, w, dy, stride, pad):
    """{pass: callable} on one side; the backward callables differentiate a forward result that is kept alive.  Each backward pass
    has a forward result of its own in which ONLY its operand requires a gradient: a custom Function decides what to launch from
    that (needs_input_grad), not from the targets of autograd.grad, and a result with both would run both passes in either call."""
    conv = (lambda a, b: c2d.Conv2dFn.apply(a, b, stride, pad)) if side == 'hip' else (lambda a, b: F.conv2d(a, b, None, stride, pad))
    y_w = conv(x.detach(), w)
    calls = {'forward': lambda: conv(x, w), 'backward_weight': lambda: torch.autograd.grad(y_w, w, dy, retain_graph=True)}
    if x.requires_grad:
        y_x = conv(x, w.detach())
        calls['backward_input'] = lambda: torch.autograd.grad(y_x, x, dy, retain_graph=True)
    return calls


def timed(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='128,32')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r27_conv2d.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_conv2d needs a HIP device'
    dev = 'cuda:0'
    lines = []
    for B in (int(b) for b in args.batches.split(',')):
        total = {p: {'hip': 0.0, 'library': 0.0} for p in PASSES}
        for name, cin, size, cout, k, stride, count in GEOMETRIES:
            g = torch.Generator().manual_seed(2700)
            pad = k // 2
            out = c2d.out_size(size, k, stride, pad)
            x = torch.randn(B, cin, size, size, generator=g).to(dev).requires_grad_(cin != 4)      # the stem's input is the image
            w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev).requires_grad_(True)
            dy = torch.randn(B, cout, out, out, generator=g).to(dev)
            calls = {side: make_calls(side, x, w, dy, stride, pad) for side in ('hip', 'library')}
            flop = 2.0 * B * out * out * cout * cin * k * k
            rec = {'bench': 'conv2d', 'B': B, 'name': name, 'count': count, 'x': [B, cin, size, size], 'w': [cout, cin, k, k],
                   'stride': stride, 'iters': args.iters, 'warmup': args.warmup, 'gflop': round(flop / 1e9, 3), 'passes': {}}
            for p in PASSES:
                if p not in calls['hip']:
                    rec['passes'][p] = None
                    continue
                for side in calls:
                    for _ in range(args.warmup):
                        calls[side][p]()
                ms = {'hip': [], 'library': []}
                for _ in range(args.repeats):       # alternated: a drift of the machine hits both sides alike
                    for side in ms:
                        ms[side].append(round(timed(calls[side][p], args.iters), 4))
                med = {side: statistics.median(v) for side, v in ms.items()}
                winner = 'hip' if max(ms['hip']) < min(ms['library']) else 'library' if max(ms['library']) < min(ms['hip']) else 'tie'
                rec['passes'][p] = {'ms': ms, 'median_ms': med, 'spread_ms': {s: [min(v), max(v)] for s, v in ms.items()},
                                    'tflops': {s: round(flop / (m * 1e-3) / 1e12, 2) for s, m in med.items()},
                                    'hip_fraction_of_peak': round(flop / (med['hip'] * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
                                    'library_over_hip': round(med['library'] / med['hip'], 3), 'winner': winner}
                for side in med:
                    total[p][side] += count * med[side]
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del calls, x, w, dy
            torch.cuda.empty_cache()
        summ = {'bench': 'conv2d_sum_over_resnet18', 'B': B,
                'sum_of_medians_ms': {p: {s: round(v, 3) for s, v in t.items()} for p, t in total.items()},
                'all_passes_ms': {s: round(sum(total[p][s] for p in PASSES), 3) for s in ('hip', 'library')}}
        line = json.dumps(summ)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
