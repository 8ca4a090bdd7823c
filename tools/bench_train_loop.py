#!/usr/bin/env python3
"""Steps per second of a training epoch: training.ResidentTrainLoop (one graph replay per iteration, the host only replays) against
the reference-shaped loop on the pieces the project had before it:

    for i, batch in enumerate(loader):                    # DeviceCloudLoader / DeviceSVRLoader
        scheduler(optimizer, epoch, i)                    # optim.LRUpdater edits param_groups
        loss, pnll, gnll, gent = step(...)                # GraphedTrainStep: replay + Adam.step()
        if torch.isnan(loss): stop                        # the reference's guard (training.py:48)   -> a synchronisation
        meters: loss.item(), pnll.item(), gnll.item(), gent.item()                                   -> four more

Both run `--steps` iterations (whole epochs of `--epoch-iters` iterations) per round on their own copy of the model, ALTERNATING in
one process; one warm-up round, then `--rounds` timed rounds.  Wall-clock from the first enqueue to a final synchronise.  Reported
per loop: the median steps per second, the best, and the spread (max - min) over the rounds; for the resident loop also the host
time `run` takes per iteration (the graph launch: where it comes close to the step, the launch itself is the bound).  The baseline's
host is inside the step for all of it (it waits in `.item()`).  No threshold: both numbers and the spread are the result.

Configurations (one fresh process each, started by --config all):
    airplane   config_generative_modeling_airplane.yaml, B = 64 x 2048
    shard      config_autoencoding.yaml, the 16-shape shard of a data-parallel rank: B = 16 x 2048, SyncBatchNorm, a 1-rank RCCL
               group with GWTF_FORCE_SHARDED=1 (every collective of the multi-rank step inside the graph, the guard flag's included)
    svr        config_SVR.yaml (tests/golden/contract_svr.json svr_cfg), B = 32 x 2048, 137 x 137 synthetic renderings -> 224 x 224,
               train_norm = 'hip'

    python tools/bench_train_loop.py [--config all] [--steps 200] [--rounds 5] [--out profiles/r28_train_loop.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AIRPLANE = dict(train_mode='p_rnvp_mc_g_rnvp_vae', util_mode='training', deterministic=False,
                pc_enc_init_n_channels=3, pc_enc_init_n_features=64, pc_enc_n_features=[128, 256, 512],
                g_latent_space_size=128, g_prior_n_flows=7, g_prior_n_features=128, g_posterior_n_layers=1,
                p_latent_space_size=3, p_prior_n_layers=1, p_decoder_n_flows=21, p_decoder_n_features=64,
                p_decoder_base_type='free', p_decoder_base_var=-3.9551, n_components=4,
                params_reduce_mode='depth_and_feature', weights_type='learned_weights',
                pnll_weight=1.0, gnll_weight=1.0, gent_weight=1.0)
SCHEDULE = dict(cycle_length=2, min_lr=1.7e-5, max_lr=2.56e-4, beta1=0.9, min_beta2=0.9945, max_beta2=0.999)
IMAGES = dict(image_add_grayscale=True, image_means=[0.03492457, 0.03379815, 0.03475684, 0.03874264], image_noise=False,
              image_noise_scale=0.02, image_normalize=True, image_pad=False, image_pad_size=[0, 0], image_remove_alpha=True,
              image_resize=True, image_size=[224, 224], image_stds=[0.10963749, 0.10795733, 0.11031612, 0.12266339])
DEV = 'cuda:0'


def synthetic_mesh(n_faces, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    nv = max(4, n_faces // 2)
    v = rng.normal(size=(nv, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.5).astype(np.float32)
    first = rng.randint(0, nv, n_faces)
    f = np.stack([first, (first + rng.randint(1, 16, n_faces)) % nv, (first + rng.randint(16, 32, n_faces)) % nv], axis=1)
    return v, f.astype(np.uint32)


def run_config(a):
    import numpy as np
    import torch
    import go_with_the_flows_amd as gw
    from go_with_the_flows_amd import models, optim
    from go_with_the_flows_amd.training import GraphedTrainStep, ResidentTrainLoop

    torch.cuda.set_device(0)
    sharded = a.config == 'shard'
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(29930 + os.getpid() % 60))
        os.environ['GWTF_FORCE_SHARDED'] = '1'
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device(DEV))
    svr = a.config == 'svr'
    B, N, wd = {'airplane': (64, 2048, 1e-5), 'shard': (16, 2048, 1e-6), 'svr': (32, 2048, 1e-5)}[a.config]
    if svr:
        cfg = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'contract_svr.json')))['svr_cfg']
        N = cfg['cloud_size']
    else:
        cfg = dict(AIRPLANE)
        if sharded:
            cfg.update(g_latent_space_size=512, p_decoder_base_type='freevar', p_decoder_base_var=-3.596)
    views = 2 if svr else 1
    n_shapes = a.epoch_iters * B // views
    meshes = [synthetic_mesh(2000, 7 + i) for i in range(n_shapes)]
    store = gw.MeshStore.from_arrays(np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes]),
                                     np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes]), device=DEV)
    cloud_t = gw.CloudTransform(center=True)
    if svr:
        raw = np.random.RandomState(28).randint(0, 256, (n_shapes * views, 3, 137, 137)).astype(np.uint8)
        images = gw.ImageStore.from_arrays(raw, views_per_shape=views, device=DEV)
        image_t = gw.ImageTransform.from_config(channels=3, **IMAGES)
        make_loader = lambda: gw.DeviceSVRLoader(store, images, B, N, cloud_t, image_t, seed=3)
    else:
        make_loader = lambda: gw.DeviceCloudLoader(store, B, N, cloud_t, seed=3)

    def make_model():
        torch.manual_seed(0)
        m = (models.Flow_Mixture_SVR_Model if svr else models.Flow_Mixture_Model)(**cfg).to(DEV).train()
        if svr:
            m.img_encoder.train_norm = 'hip'
        if sharded:
            m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
        return m, optim.Adam(m.parameters(), lr=2.56e-4, betas=(0.9, 0.999), weight_decay=wd, amsgrad=True)

    crit = models.Flow_Mixture_Loss(**cfg)
    up = optim.LRUpdater(a.epoch_iters, **SCHEDULE)
    epochs = a.steps // a.epoch_iters
    assert epochs >= 1 and epochs * a.epoch_iters == a.steps, '--steps must be a multiple of --epoch-iters'
    # the reference-shaped loop on the existing pieces
    m0, opt0 = make_model()
    loader0 = make_loader()
    first = next(iter(make_loader()))
    step = GraphedTrainStep(m0, crit, opt0, first['cloud'], first['eval_cloud'], images_example=first.get('image'))
    epoch0 = [0]

    def baseline():
        last = None
        for _ in range(epochs):
            loader0.set_epoch(epoch0[0])
            for i, batch in enumerate(loader0):
                up(opt0, epoch0[0], i)
                terms = step(batch['cloud'], batch['eval_cloud'], batch['image']) if svr else step(batch['cloud'], batch['eval_cloud'])
                if bool(torch.isnan(terms[0])):
                    raise RuntimeError('Stopping without updating the net')
                last = [t.item() for t in terms]
            epoch0[0] += 1
        return last

    # the resident loop
    m1, opt1 = make_model()
    loop = ResidentTrainLoop(m1, crit, opt1, make_loader(), scheduler=up)
    epoch1, enqueue = [0], []

    def resident():
        spent = 0.0
        for _ in range(epochs):
            loop.set_epoch(epoch1[0])
            t0 = time.perf_counter()
            loop.run(a.epoch_iters)
            spent += time.perf_counter() - t0
            epoch1[0] += 1
        enqueue.append(spent / a.steps * 1e3)               # host time to enqueue one iteration (the replay call)
        return loop.meters(reset=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return a.steps / (time.perf_counter() - t0), out

    timed(baseline), timed(resident)                        # warm-up round
    rb, rr = [], []
    for _ in range(a.rounds):
        sps, last = timed(baseline)
        rb.append(sps)
        sps, rec = timed(resident)
        rr.append(sps)
        assert rec['LB'][3] == a.steps * B and not rec['poisoned'], rec
    stats = lambda x: {'median_steps_per_s': round(float(np.median(x)), 2), 'best_steps_per_s': round(max(x), 2),
                       'spread_steps_per_s': round(max(x) - min(x), 2), 'median_ms_per_step': round(1e3 / float(np.median(x)), 3)}
    sb, sr = stats(rb), stats(rr)
    sr['host_enqueue_ms_per_step'] = round(float(np.median(enqueue[1:])), 3)
    gap, spread = sr['median_steps_per_s'] - sb['median_steps_per_s'], max(sb['spread_steps_per_s'], sr['spread_steps_per_s'])
    line = {'bench': 'train_loop', 'config': a.config, 'B': B, 'n_points': N, 'steps_per_round': a.steps, 'epoch_iters': a.epoch_iters,
            'rounds': a.rounds, 'graphed_step_loop': sb, 'resident_loop': sr, 'gap_steps_per_s': round(gap, 2),
            'larger_spread_steps_per_s': spread, 'resident_faster_beyond_spread': bool(gap > spread),
            'speedup': round(sr['median_steps_per_s'] / sb['median_steps_per_s'], 4),
            'last_terms_baseline': last, 'last_meter_avg_resident': [rec[k][1] for k in ('LB', 'PNLL', 'GNLL', 'GENT')],
            'timed_by': 'wall clock around whole rounds, final synchronise; the two loops alternate in one process after a warm-up round',
            'device': torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write(json.dumps(line) + '\n')
    if sharded:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='all', choices=['all', 'airplane', 'shard', 'svr'])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--epoch-iters', type=int, default=25, help='iterations per epoch (the synthetic stores are sized for it)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r28_train_loop.jsonl'))
    a = ap.parse_args()
    if a.config != 'all':
        return run_config(a)
    for config in ('airplane', 'shard', 'svr'):                  # a fresh process each: the shard needs its own process group
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--config', config, '--steps', str(a.steps), '--epoch-iters',
                            str(a.epoch_iters), '--rounds', str(a.rounds), '--out', a.out])
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == '__main__':
    main()
