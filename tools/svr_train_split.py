#!/usr/bin/env python3
"""Kernel time of one graphed SVR training step split between the image encoder's library kernels and everything else, from two
`rocprofv3 --kernel-trace --stats --output-format csv` runs:

    rocprofv3 ... -- python tools/bench_svr_train.py --profile-steps N --batches B       -> STEP_kernel_stats.csv
    rocprofv3 ... -- python tools/bench_svr_train.py --profile-encoder M --batches B     -> ENC_kernel_stats.csv

    python tools/svr_train_split.py STEP_kernel_stats.csv STEP_CALLS ENC_kernel_stats.csv M [--batch B]  -> one JSON line

STEP_CALLS = N + the warm-up and capture passes of GraphedTrainStep's constructor that launched kernels (2 warm-ups; the capture
launches none) = N + 2.  The encoder's kernels cannot be told from the rest by name alone (its ReLUs and residual adds are the same
elementwise kernels the rest of the step uses), so its share is the per-pass kernel time of the encoder-alone trace; the trace of the
step also gives a by-name lower bound (convolution / BatchNorm / pooling / GEMM kernels of the libraries, which only the encoder calls).
"""
import argparse
import csv
import json


def rows(path):
    return [r for r in csv.DictReader(open(path)) if 'copyBuffer' not in r['Name'] and 'fillBuffer' not in r['Name']]


def bucket(name):
    if 'at::' in name:
        return 'torch_operators'
    if '(anonymous namespace)' in name or name.startswith('gwtf'):
        return 'project_kernels'
    return 'library_kernels'          # MIOpen convolutions / BatchNorm / pooling, rocBLAS / Tensile GEMMs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('step_csv')
    ap.add_argument('step_calls', type=int)
    ap.add_argument('encoder_csv')
    ap.add_argument('encoder_calls', type=int)
    ap.add_argument('--batch', type=int, default=None)
    a = ap.parse_args()
    step, enc = rows(a.step_csv), rows(a.encoder_csv)
    by = {}
    for r in step:
        by[bucket(r['Name'])] = by.get(bucket(r['Name']), 0.0) + float(r['TotalDurationNs'])
    step_ms = sum(by.values()) / a.step_calls / 1e6
    enc_ms = sum(float(r['TotalDurationNs']) for r in enc) / a.encoder_calls / 1e6
    out = {'bench': 'svr_train_kernel_split', 'B': a.batch, 'step_kernel_ms': round(step_ms, 3),
           'image_encoder_kernel_ms': round(enc_ms, 3), 'everything_else_kernel_ms': round(step_ms - enc_ms, 3),
           'image_encoder_share': round(enc_ms / step_ms, 3),
           'step_by_name_ms': {k: round(v / a.step_calls / 1e6, 3) for k, v in sorted(by.items())},
           'step_top_kernels': [[r['Name'][:90], round(float(r['TotalDurationNs']) / a.step_calls / 1e6, 3)] for r in
                                sorted(step, key=lambda r: -float(r['TotalDurationNs']))[:12]]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
