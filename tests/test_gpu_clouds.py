"""The device cloud sampler (csrc/gwtf_clouds.hip, go_with_the_flows_amd/clouds.py) on the GPU: against the genuine reference's
sample_cloud and cloud transformations (fixture g22_clouds, explicit draws), against the numpy restatement of its Philox draws
(clouds_ref.py), and its determinism, graph capture, distribution and loader."""
import numpy as np
import pytest
import torch

from conftest import golden
import clouds_ref as cr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, clouds

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def fx():
    return golden('g22_clouds')


@pytest.fixture(scope='module')
def fx_store(fx):
    return gw.MeshStore.from_arrays(fx['vertices_c'], fx['faces_vc'], fx['vertices_c_bounds'], fx['faces_bounds'], fx['orig_c'],
                                    fx['orig_s'], device=DEV)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _explicit(words, s1, s2, normals=None):
    ex = {'words': _dev(words.astype(np.uint32)), 's1': _dev(s1.astype(np.float32)), 's2': _dev(s2.astype(np.float32))}
    if normals is not None:
        ex['normals'] = _dev(normals.astype(np.float32))
    return ex


def _np(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _fixture_run(fx, store, transform):
    out = gw.sample_clouds(store, _dev(fx['rows']), int(fx['cloud_size']), True, transform, gw.make_state(0, DEV),
                           _explicit(fx['words'], fx['s1'], fx['s2'], fx['normals']))
    return _np(out)


def _transform(fx, **flags):
    return gw.CloudTransform.from_config(cloud_translate_shift=fx['translate_shift'].tolist(), cloud_scale_scale=float(fx['scale_scale']),
                                         cloud_noise_scale=float(fx['noise_scale']), **flags)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. explicit draws, no transformation: the reference's bits ---------------------------------------------------------------
def test_explicit_draws_reproduce_the_reference_bit_for_bit(fx, fx_store):
    got = _fixture_run(fx, fx_store, None)
    assert got['cloud'].shape == (6, 3, 24) and got['eval_cloud'].shape == (6, 3, 24)
    assert np.array_equal(_bits(got['cloud']), _bits(fx['cloud_none']))
    assert np.array_equal(_bits(got['eval_cloud']), _bits(fx['eval_cloud_none']))
    assert np.array_equal(got['orig_c'], fx['orig_c'][fx['rows']]) and np.array_equal(got['orig_s'], fx['orig_s'][fx['rows']])
    # without an eval cloud all M points go to `cloud`, in draw order
    one = gw.sample_clouds(fx_store, _dev(fx['rows']), 48, False, None, gw.make_state(0, DEV), _explicit(fx['words'], fx['s1'], fx['s2']))
    assert 'eval_cloud' not in one
    one = one['cloud'].cpu().numpy()
    assert np.array_equal(_bits(one[:, :, 0::2]), _bits(fx['cloud_none'])) and np.array_equal(_bits(one[:, :, 1::2]), _bits(fx['eval_cloud_none']))


# ---- 2. every transformation alone, and all together --------------------------------------------------------------------------
def _noise(fx):
    """(cloud, eval) noise terms scale * z in float32, as the kernel forms them."""
    n = fx['noise_scale'] * fx['normals']
    return n[:, :, 0::2], n[:, :, 1::2]


@pytest.mark.parametrize('name', ['orig', 'translate', 'scale', 'noise', 'center', 'all'])
def test_transformations_against_the_reference(fx, fx_store, name):
    """Bars (set by the issue): orig, translate bitwise; scale 1 ulp; noise 2 ulp of max(|x|, |noise|) (the float64 normal is rounded
    before the multiply here, after it in the reference); center 2e-6 max|x| against the float64 mean of the reference's pre-centring
    points (two float32 tree sums of <= 4096 terms, each within log2(4096) 2^-24, plus the subtraction).  All together: the
    reference's own uncentred output carries what scale (1 ulp) and noise (2 ulp) may differ by, 3 ulp of X = max(|x|, |noise|)
    before centring, and centring adds its 2e-6 X: the sum of the bars of its parts."""
    flags = {'orig': dict(cloud_rescale2orig=True, cloud_recenter2orig=True), 'translate': dict(cloud_translate=True),
             'scale': dict(cloud_scale=True), 'noise': dict(cloud_noise=True), 'center': dict(cloud_center=True)}
    flags['all'] = {k: v for d in flags.values() for k, v in d.items()}
    got = _fixture_run(fx, fx_store, _transform(fx, **flags[name]))
    for key, noise in zip(('cloud', 'eval_cloud'), _noise(fx)):
        mine, ref = got[key], fx[f'{key}_{name}']
        if name in ('orig', 'translate'):
            assert np.array_equal(_bits(mine), _bits(ref)), (name, key)
            continue
        err = np.abs(mine.astype(np.float64) - ref)
        if name == 'scale':
            bound = np.spacing(np.maximum(np.abs(mine), np.abs(ref)))
        elif name == 'noise':
            bound = 2 * np.spacing(np.maximum(np.abs(fx[f'{key}_none']), np.abs(noise)))
        else:
            pre = fx[f'{key}_none' if name == 'center' else f'{key}_all_nocenter'].astype(np.float64)
            ref = pre - pre.mean(axis=2, keepdims=True)
            err = np.abs(mine.astype(np.float64) - ref)
            x = np.abs(pre).max(axis=(1, 2), keepdims=True) if name == 'center' else \
                np.maximum(np.abs(pre).max(axis=(1, 2), keepdims=True), np.abs(noise).max())
            bound = 2e-6 * x + (0 if name == 'center' else 3 * 2.0**-23 * x)
        print(f'CLOUDS {name} {key}: max err {err.max():.3e}, min slack (bound - err) {(bound - err).min():.3e}')
        assert np.all(err <= bound), (name, key, float(err.max()))


# ---- 3. Philox mode against the numpy restatement ------------------------------------------------------------------------------
def _signatures(v, f):
    """Per face (F, 9): v0 and the two edge midpoints as the kernel forms them -- what explicit (s1, s2) = (0,0), (.5,0), (0,.5) return."""
    p = v[f.astype(np.int64)]
    half = np.float32(0.5)
    return np.concatenate([p[:, 0], p[:, 0] + half * (p[:, 1] - p[:, 0]), p[:, 0] + half * (p[:, 2] - p[:, 0])], axis=1)


def _device_faces(store, packed, rows, words, eval_cloud):
    """Face index of every (row, point) as the DEVICE found it for these words: three explicit runs return v0 and two edge
    midpoints of the chosen face, looked up among the shape's faces."""
    B, M = words.shape
    N = M // 2 if eval_cloud else M
    runs = []
    for a, b in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5)):
        out = _np(gw.sample_clouds(store, _dev(rows), N, eval_cloud, None, gw.make_state(0, DEV),
                                   _explicit(words, np.full((B, M), a), np.full((B, M), b))))
        pts = np.zeros((B, 3, M), np.float32)
        if eval_cloud:
            pts[:, :, 0::2], pts[:, :, 1::2] = out['cloud'], out['eval_cloud']
        else:
            pts = out['cloud']
        runs.append(pts)
    sig = np.concatenate(runs, axis=1).transpose(0, 2, 1)              # (B, M, 9)
    faces = np.zeros((B, M), np.int64)
    for r, shape in enumerate(rows):
        table = {}
        for k, s in enumerate(_signatures(*cr.shape_arrays(packed, int(shape)))):
            table.setdefault(s.tobytes(), k)
        faces[r] = [table[np.ascontiguousarray(s).tobytes()] for s in sig[r]]
    return faces


CHUNK = 1024          # the default chunk of csrc/gwtf_clouds.hip


@pytest.mark.parametrize('B,N,F,eval_cloud,lead', [(1, 1, 1, False, False), (1, 1, 1, True, False), (5, 33, 77, True, False),
                                                   (3, CHUNK + 1, 1025, True, False), (2, 64, 2, True, True),
                                                   (2, 2 * CHUNK + 1, 5000, False, False)])
def test_philox_mode_equals_the_restatement(B, N, F, eval_cloud, lead):
    meshes = [cr.random_mesh(F, max(3, min(F, 300)), 100 + i, leading_zero_area=lead) for i in range(3)]
    packed = cr.pack(meshes)
    store = gw.MeshStore.from_arrays(*packed, device=DEV)
    rows = np.array({1: [1], 2: [1, 1], 3: [2, 0, 2], 5: [2, 0, 1, 0, 2]}[B], np.int32)     # B > 1: a shape appears twice
    seed, call = 0x1234567890abcdef + F, (5 << 32) + 17 + N
    M = 2 * N if eval_cloud else N
    state = gw.make_state(seed, DEV, call)
    got = _np(gw.sample_clouds(store, _dev(rows), N, eval_cloud, None, state))
    words, s1, s2 = cr.sampling_draws(seed, call, B, M)
    faces, points = cr.restate(packed, rows, words, s1, s2)
    if eval_cloud:
        assert np.array_equal(_bits(got['cloud']), _bits(points[:, :, 0::2]))
        assert np.array_equal(_bits(got['eval_cloud']), _bits(points[:, :, 1::2]))
    else:
        assert np.array_equal(_bits(got['cloud']), _bits(points))
    sig_faces = _device_faces(store, packed, rows, words, eval_cloud)
    for r, shape in enumerate(rows):                                          # same face, or a twin with the same three vertices
        sig = _signatures(*cr.shape_arrays(packed, int(shape)))
        assert np.array_equal(sig[sig_faces[r]], sig[faces[r]])
    if lead:
        assert faces.min() >= 1 and sig_faces.min() >= 1                      # the leading zero-area face is never chosen
    if B > 1:                                                                 # one shape twice: different points, each as restated
        same = [(i, j) for i in range(B) for j in range(i + 1, B) if rows[i] == rows[j]]
        assert same and all(not np.array_equal(got['cloud'][i], got['cloud'][j]) for i, j in same)
    assert state.cpu().tolist() == [seed, call + 1]


# ---- 4. determinism and independence -------------------------------------------------------------------------------------------
def test_determinism_tuning_independence_and_the_call_word(fx, fx_store):
    t = _transform(fx, cloud_rescale2orig=True, cloud_recenter2orig=True, cloud_translate=True, cloud_scale=True, cloud_noise=True,
                   cloud_center=True)
    rows = _dev(np.array([0, 1, 2, 0, 0], np.int32))
    N = 2 * CHUNK + 77

    def run(word=0, call=3, transform=t):
        state = gw.make_state(99, DEV, call)
        with _lib.tuning(word=word):
            out = _np(gw.sample_clouds(fx_store, rows, N, True, transform, state))
        assert state.cpu().tolist() == [99, call + 1]
        return out
    base = run()
    assert np.isfinite(base['cloud']).all() and np.abs(base['cloud'].mean(axis=2)).max() < 1e-5      # centred (coordinates of order 1)
    for _ in range(3):                                      # repeated runs, centring on: no float atomics
        again = run()
        assert np.array_equal(_bits(again['cloud']), _bits(base['cloud'])) and np.array_equal(_bits(again['eval_cloud']), _bits(base['eval_cloud']))
    for word in (256, 512, 300, 2048, 8192, 0xffff):        # every chunk size the tuning word can ask for
        other = run(word)
        assert np.array_equal(_bits(other['cloud']), _bits(base['cloud'])), word
        assert np.array_equal(_bits(other['eval_cloud']), _bits(base['eval_cloud'])), word
    assert not np.array_equal(run(call=4)['cloud'], base['cloud'])
    plain, other = run(transform=None), run(2048, transform=None)
    assert np.array_equal(_bits(plain['cloud']), _bits(other['cloud'])) and not np.array_equal(plain['cloud'], plain['eval_cloud'])


def test_a_row_outside_the_store_gives_nan_and_reads_nothing(fx_store):
    out = _np(gw.sample_clouds(fx_store, _dev(np.array([0, 3, -1], np.int32)), 16, True, None, gw.make_state(1, DEV)))
    assert np.isfinite(out['cloud'][0]).all() and np.isnan(out['cloud'][1:]).all() and np.isnan(out['eval_cloud'][1:]).all()


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def test_a_captured_call_draws_fresh_points_on_every_replay(fx, fx_store):
    t = _transform(fx, cloud_scale=True, cloud_noise=True, cloud_center=True)
    rows, N = _dev(np.array([0, 1, 2, 0], np.int32)), 300
    state = gw.make_state(7, DEV, 40)
    out = {k: torch.empty(4, 3, N, device=DEV) for k in ('cloud', 'eval_cloud')}
    gw.sample_clouds(fx_store, rows, N, True, t, state, out=out)              # warm-up: the scratch of this (B, M) exists from here on
    state.copy_(gw.make_state(7, DEV, 40))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw.sample_clouds(fx_store, rows, N, True, t, state, out=out)
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [7, 42]
    assert not torch.equal(replays[0]['cloud'], replays[1]['cloud'])
    eager_state = gw.make_state(7, DEV, 40)
    for rep in replays:
        eager = gw.sample_clouds(fx_store, rows, N, True, t, eager_state)
        assert torch.equal(eager['cloud'], rep['cloud']) and torch.equal(eager['eval_cloud'], rep['eval_cloud'])


# ---- 6. distribution ------------------------------------------------------------------------------------------------------------
DIST_SEED = 2024


def test_face_counts_and_noise_moments(fx, fx_store):
    B, N = 8, 2048
    M = 2 * N
    rows = np.zeros(B, np.int32)                                              # the 77-face mesh
    packed = (fx['vertices_c'], fx['faces_vc'], fx['vertices_c_bounds'], fx['faces_bounds'])
    plain = _np(gw.sample_clouds(fx_store, _dev(rows), N, True, None, gw.make_state(DIST_SEED, DEV)))
    words, s1, s2 = cr.sampling_draws(DIST_SEED, 0, B, M)
    faces, points = cr.restate(packed, rows, words, s1, s2)
    assert np.array_equal(_bits(plain['cloud']), _bits(points[:, :, 0::2])) and np.array_equal(_bits(plain['eval_cloud']), _bits(points[:, :, 1::2]))
    assert np.array_equal(_device_faces(fx_store, packed, rows, words, True), faces)      # the faces the device chose
    _, probs, _ = cr.reference_cdf(*cr.shape_arrays(packed, 0))
    counts = np.bincount(faces.ravel(), minlength=len(probs))
    expected = probs.astype(np.float64) * faces.size
    chi2, df = float(((counts - expected)**2 / expected).sum()), len(probs) - 1
    print(f'CLOUDS chi2 {chi2:.1f} df {df} bar {df + 5 * np.sqrt(2 * df):.1f}')
    assert chi2 <= df + 5 * np.sqrt(2 * df)
    noisy = _np(gw.sample_clouds(fx_store, _dev(rows), N, True, gw.CloudTransform(noise=True, noise_scale=1.0), gw.make_state(DIST_SEED, DEV)))
    z = np.concatenate([noisy['cloud'] - plain['cloud'], noisy['eval_cloud'] - plain['eval_cloud']]).astype(np.float64).ravel()
    n = z.size
    assert n == 8 * 3 * 4096
    print(f'CLOUDS noise mean {z.mean():.4e} (bar {5 / np.sqrt(n):.4e}) var-1 {z.var() - 1:.4e} (bar {5 * np.sqrt(2 / n):.4e})')
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    # and they are the restated Box-Muller values: float32 log / sqrt / cos / sin here and in numpy differ by a few ulp of |z| < 6,
    # about 1e-5 with the rounding of the two additions; a wrong word or stream would differ by order 1
    restated = cr.noise_draws(DIST_SEED, 0, B, M).reshape(B, 3, N, 2).transpose(3, 0, 1, 2).ravel()
    assert np.abs(z - restated).max() < 1e-4


# ---- 7. the loader --------------------------------------------------------------------------------------------------------------
def test_loader_on_the_device():
    meshes = [cr.random_mesh(20, 12, 300 + i) for i in range(7)]
    rng = np.random.RandomState(1)
    store = gw.MeshStore.from_arrays(*cr.pack(meshes), orig_c=rng.rand(7, 3), orig_s=rng.rand(7) + 0.5, device=DEV)
    loader = gw.DeviceCloudLoader(store, batch_size=3, cloud_size=50, transform=gw.CloudTransform(center=True), seed=5)
    epochs = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        batches = [{k: v.clone() for k, v in b.items()} for b in loader]
        assert len(batches) == len(loader) == 2
        plan = loader.index_plan()
        for i, b in enumerate(batches):
            assert set(b) == {'cloud', 'eval_cloud', 'orig_c', 'orig_s'}
            assert b['cloud'].shape == (3, 3, 50) and b['eval_cloud'].shape == (3, 3, 50) and b['cloud'].is_cuda
            assert b['orig_c'].shape == (3, 3) and b['orig_s'].shape == (3,)
            assert b['cloud'].cuda(non_blocking=True) is b['cloud']                       # the reference loop's line works unchanged
            assert np.array_equal(b['orig_s'].cpu().numpy(), store.orig_s.cpu().numpy()[plan[3 * i:3 * i + 3]])
            assert torch.isfinite(b['cloud']).all()
        epochs.append(batches)
    all_points = [b['cloud'] for e in epochs for b in e]
    assert all(not torch.equal(a, b) for i, a in enumerate(all_points) for b in all_points[i + 1:])
