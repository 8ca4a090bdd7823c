#!/usr/bin/env python3
"""One training batch of B = 64 x N = 2048 (cloud, eval_cloud) pairs drawn from STORED clouds, against the two ways a user had before.

Three ways to the same batch, alternated window by window in one process, each timed by stream events around `reps` consecutive
batches after a warm-up -- once as replays of a captured graph of eight batches (device time), once as eager calls -- for stores of
P = 4096 and P = 15000 points per shape:

* stored:  sample_stored_clouds on a CloudStore (csrc/gwtf_clouds.hip cloud_gather_kernel + the finishing launch);
* mesh:    sample_clouds on a MeshStore of as many shapes at 2e4 faces each (what a user without this store would resample from);
* torch:   the same batch composed from torch operators on the device: torch.rand(B, P).argsort(1)[:, :M] as the draw without
           replacement, a gather, the transpose to channel-major, the split into the two clouds, the transformation.

All three apply ScaleCloud 2.0, the transformation of the shipped configs.  Medians, best and the spread (max - min) / median over
the windows are recorded.

    python tools/bench_cloud_store.py [--reps 200] [--windows 7] [--out profiles/r30_cloud_store.jsonl]
"""
import argparse
import json
import os
import sys

os.environ.setdefault('OMP_NUM_THREADS', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import go_with_the_flows_amd as gw  # noqa: E402
from tools.bench_clouds import synthetic_mesh  # noqa: E402

B, N, SHAPES, FACES, SCALE = 64, 2048, 256, 20000, 2.0
M = 2 * N


def stats(times):
    t = np.asarray(times)
    return {'median_us': round(float(np.median(t)), 2), 'best_us': round(float(t.min()), 2),
            'spread': round(float((t.max() - t.min()) / np.median(t)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--points', type=int, nargs='*', default=[4096, 15000])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r30_cloud_store.jsonl'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    transform = gw.CloudTransform.from_config(cloud_scale=True, cloud_scale_scale=SCALE)
    meshes = [synthetic_mesh(FACES, 7 + i) for i in range(SHAPES)]
    mesh_store = gw.MeshStore.from_arrays(np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes]),
                                          np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes]),
                                          device=dev)
    g = torch.Generator().manual_seed(0)
    rows = [torch.randperm(SHAPES, generator=g)[:B].to(torch.int32).to(dev) for _ in range(8)]
    out = {k: torch.empty(B, 3, N, device=dev) for k in ('cloud', 'eval_cloud')}
    lines = []
    for P in a.points:
        store = gw.CloudStore.from_mesh_store(mesh_store, P, seed=1)
        cube = store.points.view(SHAPES, P, 3)
        state, mesh_state = gw.make_state(1, dev), gw.make_state(2, dev)

        def stored(r):
            gw.sample_stored_clouds(store, r, N, True, transform, state, out=out)

        def mesh(r):
            gw.sample_clouds(mesh_store, r, N, True, transform, mesh_state, out=out)

        def composed(r):
            idx = torch.rand(B, P, device=dev).argsort(1)[:, :M]
            pts = cube[r.long()].gather(1, idx[:, :, None].expand(B, M, 3)).transpose(1, 2) / SCALE
            return pts[:, :, 0::2].contiguous(), pts[:, :, 1::2].contiguous()

        ways = (('stored', stored), ('mesh', mesh), ('torch', composed))
        for _, fn in ways:                                    # every shape the windows use, once
            for r in rows:
                fn(r)
        torch.cuda.synchronize()
        # the composed batch is a draw without replacement from the right clouds, like the stored one
        c, e = composed(rows[0])
        both = torch.cat([c, e], dim=2)[0].T.contiguous()
        assert len({bytes(p) for p in both.cpu().numpy()}) == M
        # device time: the eight calls (one per row set) of each way captured in one graph, replayed reps / 8 times per window -- no
        # host enqueue between the launches; eager calls are timed beside it
        graphs = {}
        for name, fn in ways:
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for r in rows:
                    fn(r)
            graphs[name].replay()
        torch.cuda.synchronize()
        times = {f'{name}_{mode}': [] for name, _ in ways for mode in ('graph', 'eager')}
        replays = max(1, a.reps // len(rows))
        for _ in range(a.windows):
            for mode in ('graph', 'eager'):
                for name, fn in ways:                         # alternated: one window of each, then the next round
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    if mode == 'graph':
                        for _ in range(replays):
                            graphs[name].replay()
                    else:
                        for i in range(replays * len(rows)):
                            fn(rows[i % len(rows)])
                    t1.record()
                    torch.cuda.synchronize()
                    times[f'{name}_{mode}'].append(t0.elapsed_time(t1) / (replays * len(rows)) * 1e3)
        assert bool(torch.isfinite(out['cloud']).all())
        line = {'what': 'cloud_store_batch', 'B': B, 'N': N, 'points_per_shape': P, 'shapes_in_store': SHAPES,
                'mesh_faces_per_shape': FACES, 'transforms': 'scale', 'gathered_bytes_per_batch': B * M * 12,
                'timed_by': f'stream events per batch, {a.windows} alternated windows x {replays * len(rows)} batches; graph: replays of '
                            'a captured graph of 8 batches (device time), eager: host calls (enqueue included where it is longer)',
                'device': torch.cuda.get_device_name(0)}
        for name in times:
            line.update({f'{name}_{k}': v for k, v in stats(times[name]).items()})
        lines.append(line)
        print(json.dumps(line), flush=True)
        del store, cube
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
