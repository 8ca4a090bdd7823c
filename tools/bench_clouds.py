#!/usr/bin/env python3
"""What feeds a training step: one batch of (cloud, eval_cloud) pairs drawn on the device against the reference's per-item host path.

* device: sample_clouds (csrc/gwtf_clouds.hip) for B = 64 shapes x N = 2048 points with the training transformations of the
  shipped configs (ScaleCloud 2.0; --all-transforms times every fused transformation instead), on synthetic stores of F = 1e3, 2e4
  and 2e5 faces per shape; stream events around `reps` consecutive calls after a warm-up, best and median of `windows` windows.
* host: what ShapeNetCoreDataset.__getitem__ does per item (lib/datasets/datasets.py:69-106) restated here in numpy -- the two array
  copies, sample_cloud, the transformation -- on ONE core, reading the mesh from memory instead of HDF5: a lower bound for the
  reference loader.  A batch needs 64 of them; the reference spreads them over num_workers = 8 processes.

    python tools/bench_clouds.py [--reps 200] [--out FILE]      -> one JSON line per measurement (and all of them in FILE)
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

B, N, WORKERS = 64, 2048, 8


def synthetic_mesh(n_faces, seed):
    """A closed-surface-like soup: n_faces small triangles with log-normal areas scattered over the unit sphere."""
    rng = np.random.RandomState(seed)
    nv = max(4, n_faces // 2)
    v = rng.normal(size=(nv, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.5).astype(np.float32)
    first = rng.randint(0, nv, n_faces)
    f = np.stack([first, (first + rng.randint(1, 16, n_faces)) % nv, (first + rng.randint(16, 32, n_faces)) % nv], axis=1)
    return v, f.astype(np.uint32)


def host_item(vertices_all, faces_all, vb, fb, i, size, scale):
    """One __getitem__ of the reference, restated: slice copies, sample_cloud (cloud_sampling.py:4-32) with an eval cloud, ScaleCloud."""
    vertices_c = np.array(vertices_all[vb[i]:vb[i + 1]], dtype=np.float32)
    faces_vc = np.array(faces_all[fb[i]:fb[i + 1]], dtype=np.uint32)
    polygons = vertices_c[faces_vc]
    cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
    areas = np.sqrt((cross**2).sum(1)) / 2.0
    probs = areas / areas.sum()
    p_sample = np.random.choice(np.arange(polygons.shape[0]), size=2 * size, p=probs)
    sp = polygons[p_sample]
    s1 = np.random.random((2 * size, 1)).astype(np.float32)
    s2 = np.random.random((2 * size, 1)).astype(np.float32)
    cond = (s1 + s2) > 1.
    s1[cond] = 1. - s1[cond]
    s2[cond] = 1. - s2[cond]
    cloud = (sp[:, 0] + s1 * (sp[:, 1] - sp[:, 0]) + s2 * (sp[:, 2] - sp[:, 0])).astype(np.float32)
    sample = {'eval_cloud': cloud[1::2].copy().T, 'cloud': cloud[::2].T}
    sample['cloud'] /= scale
    sample['eval_cloud'] /= scale
    return sample


def time_host(packed, items):
    host_item(*packed, 0, N, np.float32(2.0))
    t0 = time.perf_counter()
    for i in range(items):
        host_item(*packed, i % (len(packed[2]) - 1), N, np.float32(2.0))
    return (time.perf_counter() - t0) / items * 1e3


def time_device(store, transform, reps, windows):
    dev = store.device
    state = gw.make_state(1, dev)
    out = {k: torch.empty(B, 3, N, device=dev) for k in ('cloud', 'eval_cloud')}
    g = torch.Generator().manual_seed(0)
    rows = [torch.randperm(len(store), generator=g)[:B].to(torch.int32).to(dev) for _ in range(8)]
    for r in rows:
        gw.sample_clouds(store, r, N, True, transform, state, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(reps):
            gw.sample_clouds(store, rows[i % len(rows)], N, True, transform, state, out=out)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / reps * 1e3)
    assert bool(torch.isfinite(out['cloud']).all())
    return min(times), float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--host-items', type=int, default=16)
    ap.add_argument('--faces', type=int, nargs='*', default=[1000, 20000, 200000])
    ap.add_argument('--all-transforms', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    if a.all_transforms:
        transform = gw.CloudTransform(rescale2orig=True, recenter2orig=True, translate=True, translate_shift=(0.1, 0.2, 0.3), scale=True,
                                      scale_scale=2.0, noise=True, noise_scale=0.002, center=True)
    else:
        transform = gw.CloudTransform.from_config(cloud_scale=True, cloud_scale_scale=2.0)      # configs/config_generative_modeling_*.yaml
    lines = []
    for F in a.faces:
        n_shapes = 256 if F <= 20000 else 64
        meshes = [synthetic_mesh(F, 7 + i) for i in range(n_shapes)]
        packed = (np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes]),
                  np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes]))
        t0 = time.perf_counter()
        store = gw.MeshStore.from_arrays(*packed, orig_c=np.zeros((n_shapes, 3), np.float32), orig_s=np.ones(n_shapes, np.float32),
                                         device='cuda:0')
        build_s = time.perf_counter() - t0
        best, med = time_device(store, transform, a.reps, a.windows)
        host_ms = time_host(packed, a.host_items)
        lines.append({'what': 'clouds_batch', 'B': B, 'N': N, 'faces_per_shape': F, 'shapes_in_store': n_shapes,
                      'transforms': 'all' if a.all_transforms else 'scale', 'device_us_per_batch_best': round(best, 2),
                      'device_us_per_batch_median': round(med, 2), 'timed_by': f'stream events, {a.windows} windows x {a.reps} calls',
                      'host_ms_per_item_one_core': round(host_ms, 3), 'host_ms_per_batch_8_workers': round(host_ms * B / WORKERS, 2),
                      'host_path': 'numpy restatement of __getitem__, mesh in memory (no HDF5): a lower bound',
                      'store_build_s': round(build_s, 2), 'device': torch.cuda.get_device_name(0)})
        print(json.dumps(lines[-1]), flush=True)
        del store
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
