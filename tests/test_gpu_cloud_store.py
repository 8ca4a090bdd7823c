"""The stored-cloud sampler on the GPU (csrc/gwtf_clouds.hip cloud_gather_kernel, clouds.CloudStore): explicit indices, the Philox
rule against its numpy restatement (cloud_store_ref.py) bit for bit, the stored order, the transformations, determinism and graph
capture, uniformity, CloudStore.from_mesh_store, and the loaders and resident loops on a CloudStore.  Needs an MI355X.

Most stores here name every point by its coordinates -- x = index within the cloud, y = shape, z = 0 -- so the index the device
used is read back exactly."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
import cloud_store_ref as sr
from test_cloud_store_cpu import uniformity_counts
from test_gpu_loop import SCHEDULE, AverageMeter, close_state, moments
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models, optim
from go_with_the_flows_amd.synth import load_synth_
from go_with_the_flows_amd.training import GraphedTrainStep, ResidentEvalLoop, ResidentTrainLoop

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def naming_arrays(sizes):
    """(points (T,3), bounds (S+1,)): x = index within the cloud, y = shape, z = 0."""
    bounds = np.cumsum([0] + list(sizes)).astype(np.int64)
    points = np.zeros((bounds[-1], 3), np.float32)
    for s, P in enumerate(sizes):
        points[bounds[s]:bounds[s + 1], 0] = np.arange(P)
        points[bounds[s]:bounds[s + 1], 1] = s
    return points, bounds


def naming_store(sizes):
    points, bounds = naming_arrays(sizes)
    return gw.CloudStore.from_arrays(points, bounds, device=DEV), points, bounds


def assert_draws(got, want, eval_cloud):
    """got: the batch as numpy; want (B,3,M): the points in draw order (NaN compares as bits: 0x7fc00000 on both sides)."""
    wb = np.where(np.isnan(want), np.uint32(0x7fc00000), _bits(want))
    if eval_cloud:
        assert np.array_equal(_bits(got['cloud']), wb[:, :, 0::2]) and np.array_equal(_bits(got['eval_cloud']), wb[:, :, 1::2])
    else:
        assert 'eval_cloud' not in got and np.array_equal(_bits(got['cloud']), wb)


# ---- G1. explicit indices -----------------------------------------------------------------------------------------------------------
G1_SIZES = (1, 2, 3, 5, 16, 17, 257)


@pytest.fixture(scope='module')
def g1_store():
    return naming_store(G1_SIZES)


@pytest.mark.parametrize('eval_cloud', [False, True])
@pytest.mark.parametrize('N', [1, 33, 300, 600])
def test_explicit_indices_gather_exactly(g1_store, N, eval_cloud):
    store, points, bounds = g1_store
    rows = np.array([6, 1, 3, 6, 9, 5, 0], np.int32)        # shape 6 twice, row 4 outside the store
    M = 2 * N if eval_cloud else N
    rng = np.random.RandomState(N + eval_cloud)
    sizes = np.array([G1_SIZES[s] if s < len(G1_SIZES) else 4 for s in rows])
    index = (rng.randint(0, 2**31 - 1, (7, M)) % sizes[:, None]).astype(np.int32)
    index[1, 0], index[2, M - 1], index[5, M // 2] = -1, G1_SIZES[3], G1_SIZES[5] + 1000       # outside their clouds
    state = gw.make_state(3, DEV, 8)
    got = _np(gw.sample_stored_clouds(store, _dev(rows), N, eval_cloud, None, state, {'index': _dev(index)}))
    want = sr.gather(points, bounds, rows, index.astype(np.int64))
    assert np.isnan(want[4]).all() and np.isnan(want[1, :, 0]).all() and np.isnan(want[2, :, M - 1]).all() and np.isnan(want[5, :, M // 2]).all()
    assert np.isnan(want).sum() == 3 * (M + 3)
    assert_draws(got, want, eval_cloud)
    assert state.cpu().tolist() == [3, 9]


# ---- G2. the Philox rule ------------------------------------------------------------------------------------------------------------
G2_SIZES = (1, 5, 16, 17, 257, 300, 1000, 100003)


@pytest.fixture(scope='module')
def g2_store():
    return naming_store(G2_SIZES)


# every row meets every case; by cloud: M < P everywhere for the largest; M = P at (16, N 8 pairs), (17, 17), (300, 150 pairs);
# M = P + 1 at (17, 18), (257, 129 pairs); M = 3P + 2 at (5, 17), (257, 773), (300, 451 pairs), (1000, 3002): round changes inside a
# tile, across tiles and across the 1024-point chunk; P = 1 with an eval cloud wraps at every draw
@pytest.mark.parametrize('N,eval_cloud,call', [(1, True, 0), (8, True, 2**32 + 5), (17, False, 0), (18, False, 2**32 + 5),
                                               (129, True, 0), (150, True, 2**32 + 5), (773, False, 2**32 + 5), (451, True, 0),
                                               (3002, False, 0), (2048, True, 2**32 + 5)])
def test_philox_mode_equals_the_restatement(g2_store, N, eval_cloud, call):
    store, points, bounds = g2_store
    rows = np.array([7, 0, 1, 2, 3, 4, 5, 6, 4, 8], np.int32)                  # shape 4 twice, the last row outside the store
    M = 2 * N if eval_cloud else N
    seed = 0x1234567890abcdef + N
    state = gw.make_state(seed, DEV, call)
    got = _np(gw.sample_clouds(store, _dev(rows), N, eval_cloud, None, state))       # through the dispatch
    index = sr.stored_indices(seed, call, [G2_SIZES[s] if s < 8 else 1 for s in rows], M)
    assert index.max() < 2**31                                                        # no walk met the cap
    want = sr.gather(points, bounds, rows, index)
    assert np.isnan(want[9]).all() and not np.isnan(want[:9]).any()
    assert_draws(got, want, eval_cloud)
    if M <= 100003:                                                                   # without replacement: no point twice
        assert len(set(index[0].tolist())) == M
    assert not np.array_equal(index[5, :min(M, 257)], index[8, :min(M, 257)]) or M < 3     # one shape twice: different draws
    assert state.cpu().tolist() == [seed, call + 1]


# ---- G3. the stored order -----------------------------------------------------------------------------------------------------------
def test_permute_false_and_clouds_give_the_stored_order():
    store, points, bounds = naming_store((40, 7, 300))
    rows = np.array([2, 0, 1, 2], np.int32)
    for N, eval_cloud in ((7, False), (3, True), (20, True)):                  # M = 40 wraps the cloud of 7
        M = 2 * N if eval_cloud else N
        got = _np(gw.sample_stored_clouds(store, _dev(rows), N, eval_cloud, None, gw.make_state(1, DEV), permute=False))
        want = sr.gather(points, bounds, rows, sr.stored_indices(1, 0, [300, 40, 7, 300], M, permute=False))
        assert_draws(got, want, eval_cloud)
    fixed = store.clouds().cpu().numpy()
    assert fixed.shape == (3, 3, 7)
    for s in range(3):
        assert np.array_equal(fixed[s], points[bounds[s]:bounds[s] + 7].T)
    some = store.clouds(rows=[2, 0], n_points=40).cpu().numpy()
    assert some.shape == (2, 3, 40) and np.array_equal(some[0], points[bounds[2]:bounds[2] + 40].T) and np.array_equal(some[1], points[:40].T)
    with pytest.raises(gw.GwtfError, match='n_points'):
        store.clouds(rows=[2, 0], n_points=41)
    assert store._state is None                                                 # clouds() moved no sampler state
    loader = gw.DeviceCloudLoader(store, 2, 3, shuffle=False, drop_last=False, seed=4, permute=False)
    epochs = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        epochs.append([{k: v.clone() for k, v in b.items()} for b in loader])
    assert len(epochs[0]) == 2 and int(loader._state[1]) == 4
    for a, b in zip(*epochs):
        assert torch.equal(a['cloud'], b['cloud']) and torch.equal(a['eval_cloud'], b['eval_cloud'])
    assert np.array_equal(epochs[0][0]['cloud'].cpu().numpy()[1], points[bounds[1]:bounds[1] + 6:2].T)
    assert np.array_equal(epochs[0][0]['eval_cloud'].cpu().numpy()[1], points[bounds[1] + 1:bounds[1] + 6:2].T)
    shuffled = gw.DeviceCloudLoader(store, 2, 3, shuffle=False, drop_last=False, seed=4)          # permute=True: fresh draws
    first, second = [[b['cloud'].clone() for b in shuffled] for _ in range(2)]
    assert not torch.equal(first[0], second[0])


# ---- G4. the transformations --------------------------------------------------------------------------------------------------------
G4_SIZES = (9, 300, 41, 700)
SHIFT, SCALE, NOISE = (0.1, -0.2, 0.05), 1.7, 0.01


@pytest.fixture(scope='module')
def g4():
    rng = np.random.RandomState(12)
    bounds = np.cumsum((0,) + G4_SIZES).astype(np.int64)
    points = rng.uniform(-0.5, 0.5, (bounds[-1], 3)).astype(np.float32)
    orig_c, orig_s = rng.uniform(-1, 1, (4, 3)).astype(np.float32), (rng.rand(4) + 0.5).astype(np.float32)
    store = gw.CloudStore.from_arrays(points, bounds, orig_c, orig_s, device=DEV)
    rows, N = np.array([1, 3, 0, 2, 3], np.int32), 300                          # M = 600: three tiles
    index = (rng.randint(0, 2**31 - 1, (5, 2 * N)) % np.array(G4_SIZES)[rows][:, None]).astype(np.int32)
    normals = rng.standard_normal((5, 3, 2 * N)).astype(np.float32)
    pre = sr.gather(points, bounds, rows, index.astype(np.int64))
    return dict(store=store, rows=rows, N=N, index=index, normals=normals, pre=pre, orig_c=orig_c[rows], orig_s=orig_s[rows])


@pytest.mark.parametrize('name', ['orig', 'translate', 'scale', 'noise', 'center', 'all'])
def test_transformations_against_numpy(g4, name):
    """The bars of test_gpu_clouds.py for the same statements: orig and translate bitwise; scale 1 ulp; noise 2 ulp of
    max(|x|, |noise|); center 2e-6 max|x| against the float64 mean of the points before centring; all together 3 ulp of
    X = max(|x|, |noise|) before centring plus 2e-6 X."""
    flags = {'orig': dict(rescale2orig=True, recenter2orig=True), 'translate': dict(translate=True, translate_shift=SHIFT),
             'scale': dict(scale=True, scale_scale=SCALE), 'noise': dict(noise=True, noise_scale=NOISE), 'center': dict(center=True)}
    flags['all'] = {k: v for d in flags.values() for k, v in d.items()}
    t = gw.CloudTransform(**flags[name])
    got = _np(gw.sample_stored_clouds(g4['store'], _dev(g4['rows']), g4['N'], True, t, gw.make_state(0, DEV),
                                      {'index': _dev(g4['index']), 'normals': _dev(g4['normals'])}))
    assert np.array_equal(got['orig_c'], g4['orig_c']) and np.array_equal(got['orig_s'], g4['orig_s'])
    f32 = np.float32
    x = g4['pre'].copy()
    noise = f32(NOISE) * g4['normals']
    if name in ('orig', 'all'):
        x = g4['orig_s'][:, None, None] * x
        x = x + g4['orig_c'][:, :, None]
    if name in ('translate', 'all'):
        x = x - np.array(SHIFT, f32)[None, :, None]
    if name in ('scale', 'all'):
        x = x / f32(SCALE)
    before_noise = x
    if name in ('noise', 'all'):
        x = x + noise
    assert x.dtype == np.float32
    for key, sl in (('cloud', slice(0, None, 2)), ('eval_cloud', slice(1, None, 2))):
        mine, ref = got[key], x[:, :, sl]
        if name in ('orig', 'translate'):
            assert np.array_equal(_bits(mine), _bits(ref)), (name, key)
            continue
        if name == 'scale':
            err, bound = np.abs(mine.astype(np.float64) - ref), np.spacing(np.maximum(np.abs(mine), np.abs(ref)))
        elif name == 'noise':
            err, bound = np.abs(mine.astype(np.float64) - ref), 2 * np.spacing(np.maximum(np.abs(before_noise[:, :, sl]), np.abs(noise[:, :, sl])))
        else:
            pre = ref.astype(np.float64)
            err = np.abs(mine.astype(np.float64) - (pre - pre.mean(axis=2, keepdims=True)))
            X = np.abs(pre).max(axis=(1, 2), keepdims=True) if name == 'center' else \
                np.maximum(np.abs(pre).max(axis=(1, 2), keepdims=True), np.abs(noise[:, :, sl]).max())
            bound = 2e-6 * X + (0 if name == 'center' else 3 * 2.0**-23 * X)
        print(f'CLOUDSTORE {name} {key}: max err {err.max():.3e}, min slack (bound - err) {(bound - err).min():.3e}')
        assert np.all(err <= bound), (name, key, float(err.max()))


def test_philox_noise_is_the_restated_stream(g4):
    """Noise without explicit draws comes from stream 1 with counter (j, r, ...), the mesh sampler's: float32 log / sqrt / cos / sin
    here and in numpy differ by a few ulp of |z| < 6, about 1e-5 with the rounding of the two additions (test_gpu_clouds.py's bar
    1e-4; a wrong word or stream would differ by order 1)."""
    rows, N = _dev(g4['rows']), 200
    plain = _np(gw.sample_stored_clouds(g4['store'], rows, N, True, None, gw.make_state(77, DEV, 6)))
    noisy = _np(gw.sample_stored_clouds(g4['store'], rows, N, True, gw.CloudTransform(noise=True, noise_scale=1.0), gw.make_state(77, DEV, 6)))
    z = sr.noise_draws(77, 6, 5, 2 * N)
    assert np.abs((noisy['cloud'] - plain['cloud']) - z[:, :, 0::2]).max() < 1e-4
    assert np.abs((noisy['eval_cloud'] - plain['eval_cloud']) - z[:, :, 1::2]).max() < 1e-4


# ---- G5. determinism and capture ----------------------------------------------------------------------------------------------------
def test_determinism_tuning_independence_and_the_call_word(g4):
    t = gw.CloudTransform(rescale2orig=True, recenter2orig=True, translate=True, translate_shift=SHIFT, scale=True, scale_scale=SCALE,
                          noise=True, noise_scale=NOISE, center=True)
    rows, N = _dev(np.array([1, 3, 0, 3, 2], np.int32)), 1024 + 77

    def run(word=0, call=3):
        state = gw.make_state(99, DEV, call)
        with _lib.tuning(word=word):
            out = _np(gw.sample_stored_clouds(g4['store'], rows, N, True, t, state))
        assert state.cpu().tolist() == [99, call + 1]
        return out
    base = run()
    assert np.isfinite(base['cloud']).all() and np.abs(base['cloud'].mean(axis=2)).max() < 1e-5
    again = run()
    assert np.array_equal(_bits(again['cloud']), _bits(base['cloud'])) and np.array_equal(_bits(again['eval_cloud']), _bits(base['eval_cloud']))
    for word in (256, 2048):
        other = run(word)
        assert np.array_equal(_bits(other['cloud']), _bits(base['cloud'])), word
        assert np.array_equal(_bits(other['eval_cloud']), _bits(base['eval_cloud'])), word
    assert not np.array_equal(run(call=4)['cloud'], base['cloud'])


def test_a_captured_call_draws_fresh_points_on_every_replay(g2_store):
    store, points, bounds = g2_store
    rows_h, N = np.array([6, 4, 5, 4], np.int32), 300                           # M = 600: within, twice and once around the clouds
    rows = _dev(rows_h)
    state = gw.make_state(7, DEV, 40)
    out = {k: torch.empty(4, 3, N, device=DEV) for k in ('cloud', 'eval_cloud')}
    gw.sample_clouds(store, rows, N, True, None, state, out=out)
    state.copy_(gw.make_state(7, DEV, 40))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw.sample_clouds(store, rows, N, True, None, state, out=out)
    replays = []
    for _ in range(3):
        graph.replay()
        replays.append({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [7, 43]
    assert not torch.equal(replays[0]['cloud'], replays[1]['cloud']) and not torch.equal(replays[1]['cloud'], replays[2]['cloud'])
    for i, rep in enumerate(replays):
        index = sr.stored_indices(7, 40 + i, [G2_SIZES[s] for s in rows_h], 2 * N)
        assert_draws(_np(rep), sr.gather(points, bounds, rows_h, index), True)


# ---- G6. uniformity -----------------------------------------------------------------------------------------------------------------
def test_draws_are_uniform_over_the_cloud():
    """One cloud of 37 points, 64 rows x 8 draws without an eval cloud, 64 consecutive calls from seed 1234: n = 4096 draws of 8.
    Derived bounds, 5 binomial standard deviations: inclusion |count - 885.6| <= 131, first drawn |count - 110.7| <= 51 (the
    restatement is held to the same in test_cloud_store_cpu.py)."""
    store, _, _ = naming_store((37,))
    rows, state = torch.zeros(64, dtype=torch.int32, device=DEV), gw.make_state(1234, DEV)
    calls = torch.stack([gw.sample_stored_clouds(store, rows, 8, False, None, state)['cloud'][:, 0] for _ in range(64)]).cpu().numpy()
    assert np.array_equal(calls, np.round(calls)) and calls.min() >= 0 and calls.max() <= 36
    inclusion, first = uniformity_counts(lambda call: calls[call].astype(np.int64))
    print(f'CLOUDSTORE device: inclusion worst {np.abs(inclusion - 4096 * 8 / 37).max():.1f} (bar 131), '
          f'first worst {np.abs(first - 4096 / 37).max():.1f} (bar 51)')
    assert np.abs(inclusion - 4096 * 8 / 37).max() <= 131 and np.abs(first - 4096 / 37).max() <= 51
    assert all(len(set(row.tolist())) == 8 for row in calls[0])                  # without replacement


# ---- G7. from_mesh_store ------------------------------------------------------------------------------------------------------------
def test_from_mesh_store_freezes_what_sample_clouds_draws():
    D = golden('g22_clouds')
    meshes = gw.MeshStore.from_arrays(D['vertices_c'], D['faces_vc'], D['vertices_c_bounds'], D['faces_bounds'], D['orig_c'], D['orig_s'],
                                      device=DEV)
    store = gw.CloudStore.from_mesh_store(meshes, 50, seed=3, chunk=2)
    assert len(store) == 3 and store.points.shape == (150, 3) and store.bounds.tolist() == [0, 50, 100, 150]
    assert torch.equal(store.orig_c, meshes.orig_c) and torch.equal(store.orig_s, meshes.orig_s)
    state = gw.make_state(3, DEV)
    by_hand = [gw.sample_clouds(meshes, _dev(np.array(r, np.int32)), 50, False, None, state)['cloud'] for r in ([0, 1], [2])]
    assert torch.equal(store.clouds(), torch.cat(by_hand))
    assert torch.equal(store.points.view(3, 50, 3), torch.cat(by_hand).transpose(1, 2))
    one_call = gw.CloudStore.from_mesh_store(meshes, 50, seed=3)
    assert torch.equal(one_call.points[:100], store.points[:100]) and not torch.equal(one_call.points[100:], store.points[100:])


# ---- G8. the loaders and the loops on a CloudStore ----------------------------------------------------------------------------------
LB, LN = 2, 48


def loop_store(n_clouds=6):
    rng = np.random.RandomState(21)
    return gw.CloudStore.from_arrays(rng.uniform(-0.5, 0.5, (n_clouds, 200, 3)).astype(np.float32), device=DEV)


def cloud_model(B=LB):
    """test_gpu_loop.cloud_model for a batch of B <= 4 shapes."""
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg']
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    m = m.to(DEV).train()
    noise = torch.from_numpy(golden('g13_full_model')['noise_g'][:B]).to(DEV)
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    return m, cfg


@pytest.mark.parametrize('B', [2, 4])
def test_resident_train_loop_on_a_cloud_store_equals_the_host_loop(B):
    """test_gpu_loop.test_resident_loop_equals_the_graphed_step_loop's comparison, at its bars, with a CloudStore of 3 B clouds of 200
    points behind the loader: three iterations, the four terms of every iteration and the meters they leave at 1e-4 relative, the
    parameters and Adam moments by that test's close_state.

    At B = 4, the batch that test uses, all of it holds.  At B = 2 only what precedes the first update is compared between the two
    loops -- the terms of iteration 1, which both compute from the same weights and the same batch -- because behind it the HOST loop
    does not agree with itself at these bars: every train-mode BatchNorm over a batch of two normalises two values to +-1 and the
    gradients behind it divide by their difference, so the float atomics of the batch statistics decide the low bits of an update.
    Measured on the device: two runs of the same graphed-step loop leave FiLM-weight moments 0.40 of their largest entry apart (the
    resident loop against it: 0.64; at B = 4 the two loops agree to 2.2e-4), and the resident loop's third-iteration GNLL lay
    5e-6 from the graphed loop's in one run and 1.5e-4 in the next.  The loop's own record (its meters against its terms, the
    counts, the sampler state both loaders end in) is checked at both sizes."""
    store, transform, up = loop_store(3 * B), gw.CloudTransform(center=True), optim.LRUpdater(3, **SCHEDULE)
    m0, cfg = cloud_model(B)
    crit = models.Flow_Mixture_Loss(**cfg)
    opt0 = optim.Adam(m0.parameters(), lr=1e-4, amsgrad=True)
    loader0 = gw.DeviceCloudLoader(store, B, LN, transform, seed=11)
    step = GraphedTrainStep(m0, crit, opt0, torch.rand(B, 3, LN, device=DEV), torch.rand(B, 3, LN, device=DEV))
    base = []
    for i, batch in enumerate(loader0):
        up(opt0, 0, i)
        base.append([float(t) for t in step(batch['cloud'], batch['eval_cloud'])])
    assert len(base) == 3
    m1, _ = cloud_model(B)
    opt1 = optim.Adam(m1.parameters(), lr=1e-4, amsgrad=True)
    loader1 = gw.DeviceCloudLoader(store, B, LN, transform, seed=11)
    loop = ResidentTrainLoop(m1, crit, opt1, loader1, scheduler=up)
    assert torch.equal(loader1._state, gw.make_state(11, DEV))
    loop.set_epoch(0)
    got = []
    for i in range(3):
        loop.run(1)
        got.append([float(t) for t in loop.terms])
    print('graphed', base, 'resident', got)
    compared = 3 if B == 4 else 1
    for a, b in zip(base[:compared], got[:compared]):
        for x, y in zip(a, b):
            assert abs(x - y) <= 1e-4 * abs(x), (a, b)
    assert np.isfinite(got).all()
    rec = loop.meters()
    assert rec['step'] == 3 and rec['iteration'] == 3 and not rec['poisoned'] and rec['LB'][3] == 3 * B
    assert abs(rec['PNLL'][0] - got[-1][1]) <= 1e-6 * abs(got[-1][1])
    assert abs(rec['GNLL'][1] - np.mean([g[2] for g in got])) <= 1e-5 * abs(rec['GNLL'][1])
    assert torch.equal(loader1._state, loader0._state) and int(loader1._state[1]) == 3
    if B == 4:
        host = np.array(base)                                                    # the meters of the host loop: last value, average
        for name, col in (('PNLL', host[:, 1]), ('GNLL', host[:, 2]), ('GENT', host[:, 3]), ('LB', host[:, 1] + host[:, 2] - host[:, 3])):
            assert abs(rec[name][0] - col[-1]) <= 1e-4 * abs(col[-1]) and abs(rec[name][1] - col.mean()) <= 1e-4 * abs(col.mean()), name
        close_state(m0.state_dict(), m1.state_dict())
        close_state({i: t for i, t in enumerate(moments(opt0))}, {i: t for i, t in enumerate(moments(opt1))})


def test_resident_eval_loop_on_a_cloud_store_equals_the_host_loop():
    """test_gpu_validate's comparison (meters of ResidentEvalLoop.validate against a host loop over an equally seeded loader, 1e-4
    relative), on a frozen set: permute=False, so both passes and a second validate see the same clouds."""
    store = loop_store()
    m, cfg = cloud_model()
    crit = models.Flow_Mixture_Loss(**cfg)

    def val_loader():
        loader = gw.DeviceCloudLoader(store, LB, LN, gw.CloudTransform(center=True), shuffle=False, seed=5, permute=False)
        loader._state = gw.make_state(5, DEV)
        return loader
    ref = copy.deepcopy(m).eval()
    for mod in ref.modules():
        if hasattr(mod, 'invalidate_packed_weights'):
            mod.invalidate_packed_weights()
    meters = [AverageMeter() for _ in range(4)]
    with torch.no_grad():
        for batch in val_loader():
            t = crit.fused(*ref.forward_fused(batch['cloud'], batch['eval_cloud']))
            for meter, v in zip(meters, ((t[1] + t[2] - t[3]).item(), t[1].item(), t[2].item(), t[3].item())):
                meter.update(v, LB)
    loader = val_loader()
    val = ResidentEvalLoop(m, crit, loader)
    first = val.validate(0)
    assert first['iteration'] == 3 and not first['poisoned'] and first['LB'][3] == 3 * LB and int(loader._state[1]) == 3
    for name, meter in zip(('LB', 'PNLL', 'GNLL', 'GENT'), meters):
        assert abs(first[name][1] - meter.avg) <= 1e-4 * abs(meter.avg), (name, first[name], meter.avg)
        assert abs(first[name][0] - meter.val) <= 1e-4 * abs(meter.val), (name, first[name], meter.val)
    second = val.validate(0)                                                     # the frozen set again: the same clouds, the same figures
    for name in ('LB', 'PNLL', 'GNLL', 'GENT'):                                  # test_gpu_validate's bar for a pass repeated
        assert abs(second[name][1] - first[name][1]) <= 1e-5 * abs(first[name][1]), name


def test_svr_loader_takes_a_cloud_store():
    store = loop_store()
    src = np.random.RandomState(6).randint(0, 256, (12, 3, 9, 7)).astype(np.uint8)
    imgs = gw.ImageStore.from_arrays(src, views_per_shape=2, device=DEV)
    loader = gw.DeviceSVRLoader(store, imgs, 4, LN, gw.CloudTransform(center=True), gw.ImageTransform(channels=3), seed=5)
    batch = next(iter(loader))
    assert set(batch) == {'cloud', 'eval_cloud', 'image'}
    assert batch['cloud'].shape == (4, 3, LN) and batch['eval_cloud'].shape == (4, 3, LN) and batch['image'].shape[0] == 4
    assert torch.isfinite(batch['cloud']).all() and torch.isfinite(batch['eval_cloud']).all()
    both = torch.cat([batch['cloud'], batch['eval_cloud']], dim=2)[0].T.cpu().numpy()      # 96 of 200 points: no point twice
    assert len({p.tobytes() for p in both}) == 2 * LN
