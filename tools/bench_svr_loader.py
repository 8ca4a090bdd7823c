#!/usr/bin/env python3
"""What feeds the SVR training step: one batch of transformed images (and a whole loader batch) produced on the device, against the
same pipeline composed from torch operators on the device and against the reference's per-item host path.

Source 137 x 137 x 3 uint8 renderings, output 4 x 224 x 224 float32, the image flags of configs/config_SVR.yaml; B = 32 and 128.

* fused: transform_images (csrc/gwtf_images.hip), one launch per batch.
* torch: index_select -> float -> / 255 -> channels 0, 1 times channel 2 -> interpolate(bilinear) -> grayscale + cat -> normalise,
  the same stages from torch operators on the same device (not bit-equal: interpolate forms its coordinates in float32).
* loader: a whole DeviceSVRLoader batch (sample_clouds of N = 2048 with an eval cloud + transform_images).
* host: ToNumpy, a numpy bilinear resize, grayscale, normalisation per item on ONE core, the image already in memory (no HDF5
  read, no collation, no H2D copy): a lower bound for one worker of the reference loader.

Device times are stream events around consecutive calls, as many as fill about `--window-s` seconds; fused and torch windows
ALTERNATE in one process after a warm-up of both, `windows` windows each.  Reported per variant: median, best, the spread
(max - min) of its windows, and the host's time to enqueue one call (an event time close to it is bounded by the host, not the device).  The bar: the torch
median exceeds the fused median by more than the larger of the two spreads.  share_of_step relates the time to the graphed SVR
training step quoted in the README (14.0 ms at B = 32, 40.8 ms at B = 128).

    python tools/bench_svr_loader.py [--window-s 0.2] [--windows 7] [--out profiles/r22_svr_loader.jsonl]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import go_with_the_flows_amd as gw  # noqa: E402

CFG = dict(image_add_grayscale=True, image_means=[0.03492457, 0.03379815, 0.03475684, 0.03874264], image_noise=False,
           image_noise_scale=0.02, image_normalize=True, image_pad=False, image_pad_size=[0, 0], image_remove_alpha=True,
           image_resize=True, image_size=[224, 224], image_stds=[0.10963749, 0.10795733, 0.11031612, 0.12266339])
STEP_MS = {32: 14.0, 128: 40.8}
SRC, VIEWS, N_SHAPES, CLOUD = 137, 24, 32, 2048
DEV = 'cuda:0'


def torch_pipeline(images, rows, mean, std, gray):
    x = images.index_select(0, rows).float() / 255.0
    x = torch.cat([x[:, 2:3] * x[:, :2], x[:, 2:3]], 1)
    x = torch.nn.functional.interpolate(x, size=(CFG['image_size'][1], CFG['image_size'][0]), mode='bilinear', align_corners=False)
    x = torch.cat([(x * gray).sum(1, keepdim=True), x], 1)
    return (x - mean) / std


def host_item(image, tables, mean, std):
    img = np.float32(image / 255.)
    img[:2] = img[2][None] * img[:2]
    (xs, x1, a0, a1), (ys, y1, b0, b1) = tables
    rows = img[:, :, xs] * a0 + img[:, :, x1] * a1
    img = rows[:, ys, :] * b0 + rows[:, y1, :] * b1
    img = np.concatenate([(np.float32(0.299) * img[0] + np.float32(0.587) * img[1] + np.float32(0.114) * img[2])[None], img])
    return ((img - mean) / std)[:4]


def host_tables():
    out = []
    for axis, n_dst in ((2, CFG['image_size'][0]), (1, CFG['image_size'][1])):
        s, f = gw.images.resize_table(SRC, n_dst)
        shape = [1, 1, 1]
        shape[axis] = -1
        out.append((s, np.minimum(s + 1, SRC - 1), (np.float32(1) - f).reshape(shape), f.reshape(shape)))
    return out


ENQUEUE_US = []          # host time per call of every window, in order: where it equals the event time, the host is the bound


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    wall = time.perf_counter()
    for i in range(reps):
        fn(i)
    ENQUEUE_US.append((time.perf_counter() - wall) / reps * 1e6)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


def stats(times):
    return {'median_us': round(float(np.median(times)), 2), 'best_us': round(min(times), 2), 'spread_us': round(max(times) - min(times), 2)}


def synthetic_mesh(n_faces, seed):
    rng = np.random.RandomState(seed)
    nv = max(4, n_faces // 2)
    v = rng.normal(size=(nv, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.5).astype(np.float32)
    first = rng.randint(0, nv, n_faces)
    f = np.stack([first, (first + rng.randint(1, 16, n_faces)) % nv, (first + rng.randint(16, 32, n_faces)) % nv], axis=1)
    return v, f.astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50, help='calls of the calibrating window (and the least per window)')
    ap.add_argument('--window-s', type=float, default=0.2, help='device seconds a timed window aims at')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--host-items', type=int, default=16)
    ap.add_argument('--batches', type=int, nargs='*', default=[32, 128])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_svr_loader.jsonl'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    rng = np.random.RandomState(22)
    raw = rng.randint(0, 256, (N_SHAPES * VIEWS, 3, SRC, SRC)).astype(np.uint8)
    store = gw.ImageStore.from_arrays(raw, views_per_shape=VIEWS, device=DEV)
    t = gw.ImageTransform.from_config(channels=3, **CFG)
    mean = torch.tensor(CFG['image_means'], device=DEV).view(1, 4, 1, 1)
    std = torch.tensor(CFG['image_stds'], device=DEV).view(1, 4, 1, 1)
    gray = torch.tensor([0.299, 0.587, 0.114], device=DEV).view(1, 3, 1, 1)
    meshes = [synthetic_mesh(20000, 7 + i) for i in range(N_SHAPES)]
    mesh_store = gw.MeshStore.from_arrays(np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes]),
                                          np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes]),
                                          device=DEV)
    cloud_t = gw.CloudTransform.from_config(cloud_scale=True, cloud_scale_scale=2.0)
    name = torch.cuda.get_device_name(0)
    lines = []
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        rows = [torch.randperm(len(store), generator=g)[:B].to(torch.int32).to(DEV) for _ in range(8)]
        rows64 = [r.long() for r in rows]
        out = torch.empty(B, 4, CFG['image_size'][1], CFG['image_size'][0], device=DEV)
        fused = lambda i: gw.transform_images(store, rows[i % 8], t, out=out)
        composed = lambda i: torch_pipeline(store.images, rows64[i % 8], mean, std, gray)
        for i in range(8):
            fused(i)
            composed(i)
        diff = float((composed(0) - fused(0)).abs().max())
        torch.cuda.synchronize()
        # calls per window: enough for about a.window_s seconds of device work each, from a first short window
        rf, rc = (max(a.reps, min(20000, int(a.window_s * 1e6 / window(fn, a.reps)) + 1)) for fn in (fused, composed))
        tf, tc = [], []
        del ENQUEUE_US[:]
        for _ in range(a.windows):
            tf.append(window(fused, rf))
            tc.append(window(composed, rc))
        sf, sc = stats(tf), stats(tc)
        sf['host_enqueue_us'] = round(float(np.median(ENQUEUE_US[0::2])), 2)
        sc['host_enqueue_us'] = round(float(np.median(ENQUEUE_US[1::2])), 2)
        gap, spread = sc['median_us'] - sf['median_us'], max(sf['spread_us'], sc['spread_us'])
        out_bytes, in_bytes = out.numel() * 4, B * 3 * SRC * SRC
        lines.append({'what': 'svr_images_batch', 'B': B, 'source': [3, SRC, SRC], 'output': list(out.shape[1:]), 'flags': 'config_SVR',
                      'fused': sf, 'torch_composition': sc, 'gap_us': round(gap, 2), 'larger_spread_us': spread,
                      'fused_faster_beyond_spread': bool(gap > spread), 'max_abs_diff_fused_vs_torch': diff,
                      'bytes_read': in_bytes, 'bytes_written': out_bytes,
                      'fused_write_GBps': round(out_bytes / (sf['median_us'] * 1e-6) / 1e9, 1),
                      'share_of_step': round(sf['median_us'] / (STEP_MS[B] * 1e3), 5) if B in STEP_MS else None,
                      'step_ms': STEP_MS.get(B),
                      'timed_by': f'stream events, {a.windows} alternating windows of {rf} fused / {rc} torch calls', 'device': name})
        print(json.dumps(lines[-1]), flush=True)

        loader = gw.DeviceSVRLoader(mesh_store, store, B, CLOUD, cloud_t, t, seed=1)
        n_batches, epochs = len(loader), 10
        for _ in loader:                                                    # warm-up epoch: scratch and tables exist from here on
            pass
        torch.cuda.synchronize()
        tl = []
        for _ in range(a.windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            wall = time.perf_counter()
            t0.record()
            for _ in range(epochs):
                for _ in loader:
                    pass
            t1.record()
            torch.cuda.synchronize()
            tl.append((t0.elapsed_time(t1) / (n_batches * epochs) * 1e3, (time.perf_counter() - wall) / (n_batches * epochs) * 1e6))
        sl = stats([x[0] for x in tl])
        lines.append({'what': 'svr_loader_batch', 'B': B, 'cloud_size': CLOUD, 'eval_cloud': True, 'faces_per_shape': 20000,
                      'batches_per_window': n_batches, 'device': sl, 'host_wall_us_per_batch_median': round(float(np.median([x[1] for x in tl])), 1),
                      'share_of_step': round(sl['median_us'] / (STEP_MS[B] * 1e3), 5) if B in STEP_MS else None, 'step_ms': STEP_MS.get(B),
                      'timed_by': f'stream events around {epochs} epochs of {n_batches} batches, {a.windows} windows', 'device_name': name})
        print(json.dumps(lines[-1]), flush=True)

    tables = host_tables()
    m, s = np.asarray(CFG['image_means'], np.float32).reshape(-1, 1, 1), np.asarray(CFG['image_stds'], np.float32).reshape(-1, 1, 1)
    host_item(raw[0], tables, m, s)
    t0 = time.perf_counter()
    for i in range(a.host_items):
        host_item(raw[i], tables, m, s)
    host_ms = (time.perf_counter() - t0) / a.host_items * 1e3
    lines.append({'what': 'svr_images_host_item', 'host_ms_per_item_one_core': round(host_ms, 3),
                  'host_ms_per_batch_8_workers': {str(B): round(host_ms * B / 8, 2) for B in a.batches},
                  'host_path': 'numpy ToNumpy + bilinear resize + grayscale + normalise, image in memory (no HDF5, collation or H2D copy): '
                               'a lower bound'})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
