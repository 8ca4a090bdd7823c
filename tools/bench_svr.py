#!/usr/bin/env python3
"""Single-view reconstruction timings (separate from bench.py, which measures the flagship decoder workload).

* image-encoder eval forward on 224 x 224 images at B = 1, 8, 64: the HIP kernels (csrc/gwtf_resnet.hip) and the same module's
  torch graph (library convolutions), each captured in a hipGraph and replayed; achieved TFLOP/s against the 157 TFLOP/s fp32
  matrix peak of the MI355X;
* reconstructions per second through Flow_Mixture_SVR_Model.reconstruct_many at S = 1 and S = 32 (configs/config_SVR.yaml
  model, 2500 points per cloud), wall clock including the host-side component draws.

    python tools/bench_svr.py [--reps 50] [--out FILE]      -> one JSON line per measurement (and all of them in FILE)
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

from go_with_the_flows_amd import models, resnet  # noqa: E402
from go_with_the_flows_amd.synth import calibrate_image_encoder, load_image_encoder_stats_, load_synth_, synth_images  # noqa: E402

PEAK_FP32_MATRIX_TFLOPS = 157.3
SVR_CFG = dict(train_mode='p_rnvp_mc_g_rnvp_vae_ic', util_mode='reconstruction', deterministic=False, pc_enc_init_n_channels=3,
               pc_enc_init_n_features=64, pc_enc_n_features=[128, 256, 512], g_latent_space_size=512, g_prior_n_flows=7,
               g_prior_n_features=128, g_posterior_n_layers=1, g_prior_n_layers=1, p_latent_space_size=3, p_prior_n_layers=1,
               p_decoder_n_flows=21, p_decoder_n_features=64, p_decoder_base_type='freevar', p_decoder_base_var=0.0,
               n_components=4, params_reduce_mode='depth_and_feature', weights_type='global_weights')   # config_SVR.yaml


def encoder_flops(H, W, nc=512):
    """2 x multiply-adds of one image (convolutions and fc; pooling / BatchNorm / ReLU not counted)."""
    o = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    h, w = o(H, 7, 2, 3), o(W, 7, 2, 3)
    macs = h * w * 64 * 49 * 4
    h, w = o(h, 3, 2, 1), o(w, 3, 2, 1)
    cin = 64
    for li in range(4):
        planes = 64 << li
        for j in range(2):
            s = 2 if li > 0 and j == 0 else 1
            h2, w2 = o(h, 3, s, 1), o(w, 3, s, 1)
            macs += h2 * w2 * planes * 9 * cin + h2 * w2 * planes * 9 * planes
            if s == 2:
                macs += h2 * w2 * planes * cin
            h, w, cin = h2, w2, planes
    return 2.0 * (macs + 512 * nc)


def graph_time(fn, reps):
    """Median-free mean of `reps` replays of fn captured in a hipGraph (ms per call)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_svr needs a HIP device'
    dev = 'cuda:0'
    lines = []

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        lines.append(line)

    enc = resnet.resnet18(num_classes=512)
    load_synth_(enc, 2300)
    load_image_encoder_stats_(enc, calibrate_image_encoder(enc, 2301))
    enc = enc.to(dev).eval()
    for B in (1, 8, 64):
        x = torch.from_numpy(synth_images(B, 224, 224, 2302)).to(dev)
        flops = encoder_flops(224, 224) * B
        with torch.no_grad():
            enc.packed()
            ms_hip = graph_time(lambda: enc.forward_hip(x), args.reps)
            ms_lib = graph_time(lambda: enc.forward_torch(x), args.reps)
        emit(bench='image_encoder_eval', B=B, H=224, W=224, hip_ms=round(ms_hip, 4), library_ms=round(ms_lib, 4),
             hip_tflops=round(flops / ms_hip / 1e9, 2), library_tflops=round(flops / ms_lib / 1e9, 2),
             hip_pct_of_fp32_matrix_peak=round(100 * flops / ms_hip / 1e9 / PEAK_FP32_MATRIX_TFLOPS, 1),
             speedup_hip_vs_library=round(ms_lib / ms_hip, 3))

    m = models.Flow_Mixture_SVR_Model(**SVR_CFG)
    load_synth_(m, 2310, output_gain=0.3)
    load_image_encoder_stats_(m.img_encoder, calibrate_image_encoder(m.img_encoder, 2311))
    m = m.to(dev).eval()
    for S in (1, 32):
        imgs = torch.from_numpy(synth_images(S, 224, 224, 2312)).to(dev)
        for _ in range(2):
            m.reconstruct_many(imgs, 2500)
        torch.cuda.synchronize()
        reps = max(3, args.reps // 5)
        t = time.perf_counter()
        for _ in range(reps):
            m.reconstruct_many(imgs, 2500)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / reps
        emit(bench='reconstruct_many', S=S, n_points=2500, ms_per_call=round(ms, 3), reconstructions_per_s=round(S * 1e3 / ms, 1))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
