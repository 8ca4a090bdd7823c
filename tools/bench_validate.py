#!/usr/bin/env python3
"""One validation pass of the airplane configuration (25 batches of B = 64 x 2048): training.ResidentEvalLoop.validate (one replay of
the refresh graph, 25 replays of the batch graph, one read of the 160-byte record) against the reference-shaped host loop on the
pieces the project had before it:

    model.eval(); invalidate_packed_weights()             # what a training script does between train() and eval()
    with torch.no_grad():
        for batch in loader:                              # DeviceCloudLoader
            enc, dec = model.forward_fused(batch['cloud'], batch['eval_cloud'])
            loss, pnll, gnll, gent = criterion.fused(enc, dec)
            if torch.isnan(loss) or torch.isinf(loss): stop        # eval()'s guards (training.py:130-135)   -> two synchronisations
            meters: pnll.item(), gnll.item(), gent.item(), (pnll + gnll - gent).item()                     -> four more

Each on its own copy of the model (the resident loop pins its model's eval packings), ALTERNATING in one process; one warm-up round,
then `--rounds` timed rounds.  Wall clock from the first enqueue to a final synchronise.  Reported per loop: the median milliseconds
per pass, the best, and the spread (max - min) over the rounds.  Also, by stream events: the refresh graph alone and one batch replay
alone (medians over `--event-reps` replays).  No threshold: the numbers and the spread are the result.

    python tools/bench_validate.py [--batches 25] [--rounds 5] [--out profiles/r29_validate.jsonl]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_train_loop import AIRPLANE, synthetic_mesh      # noqa: E402  (the same configuration and synthetic meshes)

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=25, help='batches of one validation pass (the synthetic store is sized for it)')
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--event-reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_validate.jsonl'))
    a = ap.parse_args()

    import numpy as np
    import torch
    import go_with_the_flows_amd as gw
    from go_with_the_flows_amd import models
    from go_with_the_flows_amd.training import ResidentEvalLoop

    torch.cuda.set_device(0)
    B, N = a.batch_size, a.points
    meshes = [synthetic_mesh(2000, 7 + i) for i in range(a.batches * B)]
    store = gw.MeshStore.from_arrays(np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes]),
                                     np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes]), device=DEV)
    make_loader = lambda: gw.DeviceCloudLoader(store, B, N, gw.CloudTransform(center=True), shuffle=False, seed=3)
    crit = models.Flow_Mixture_Loss(**AIRPLANE)

    def make_model():
        torch.manual_seed(0)
        return models.Flow_Mixture_Model(**AIRPLANE).to(DEV).train()

    # the reference-shaped host loop
    m0, loader0 = make_model().eval(), make_loader()

    def host_pass():
        for mod in m0.modules():
            if hasattr(mod, 'invalidate_packed_weights'):
                mod.invalidate_packed_weights()
        total, count = [0.0] * 4, 0
        with torch.no_grad():
            for batch in loader0:
                enc, dec = m0.forward_fused(batch['cloud'], batch['eval_cloud'])
                loss, pnll, gnll, gent = crit.fused(enc, dec)
                if bool(torch.isnan(loss)) or bool(torch.isinf(loss)):
                    raise RuntimeError('Stopping without updating the net')
                vals = (pnll + gnll - gent).item(), pnll.item(), gnll.item(), gent.item()
                total = [t + v * B for t, v in zip(total, vals)]
                count += B
        return [t / count for t in total]

    # the resident pass
    m1 = make_model()
    val = ResidentEvalLoop(m1, crit, make_loader())
    epoch = [0]

    def resident_pass():
        rec = val.validate(epoch[0])
        epoch[0] += 1
        return rec

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    timed(host_pass), timed(resident_pass)                  # warm-up round
    th, tr = [], []
    for _ in range(a.rounds):
        ms, avg = timed(host_pass)
        th.append(ms)
        ms, rec = timed(resident_pass)
        tr.append(ms)
        assert rec['LB'][3] == a.batches * B and not rec['poisoned'], rec
    stats = lambda x: {'median_ms_per_pass': round(float(np.median(x)), 3), 'best_ms_per_pass': round(min(x), 3),
                       'spread_ms_per_pass': round(max(x) - min(x), 3), 'median_ms_per_batch': round(float(np.median(x)) / a.batches, 3),
                       'rounds_ms': [round(v, 3) for v in x]}
    sh, sr = stats(th), stats(tr)

    def by_events(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return round(float(np.median(out)), 4)

    refresh_ms = by_events(val.refresh_graph.replay, a.event_reps)
    val.begin(epoch[0])
    batch_ms = by_events(lambda: val.run(1), min(a.event_reps, a.batches))
    torch.cuda.synchronize()
    gap, spread = sh['median_ms_per_pass'] - sr['median_ms_per_pass'], max(sh['spread_ms_per_pass'], sr['spread_ms_per_pass'])
    line = {'bench': 'validate', 'config': 'airplane', 'B': B, 'n_points': N, 'batches': a.batches, 'rounds': a.rounds,
            'host_loop': sh, 'resident_pass': sr, 'gap_ms_per_pass': round(gap, 3), 'larger_spread_ms_per_pass': spread,
            'resident_faster_beyond_spread': bool(gap > spread),
            'speedup': round(sh['median_ms_per_pass'] / sr['median_ms_per_pass'], 4),
            'refresh_graph_ms': refresh_ms, 'batch_replay_ms': batch_ms,
            'last_meter_avg_host': avg, 'last_meter_avg_resident': [rec[k][1] for k in ('LB', 'PNLL', 'GNLL', 'GENT')],
            'timed_by': 'wall clock around whole passes, final synchronise; the two alternate in one process after a warm-up round; '
                        'refresh / batch: stream events around one replay, median',
            'device': torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
