#!/usr/bin/env python3
"""Generate g22_clouds.npz by running the GENUINE reference's sample_cloud and cloud transformations on CPU.

Build-container only, like make_golden_svr.py (make_golden*.py and their fixtures are left untouched): the reference is imported,
never copied; only data is written.  The two reference modules are loaded by file path, because their package pulls in h5py;
torchvision is absent too, so torchvision.transforms.Compose gets a stand-in in sys.modules.

For every row (a mesh and a numpy seed) the script first REPLAYS the draws in the order the reference consumes them --
random_sample(M) (RandomState.choice), random((M,1)) twice, normal(size=(3,N)) twice -- and records them, then reseeds and runs
the reference.  The recorded draws, restated, must reproduce the reference's clouds bit for bit, or the script stops.

    python tests/golden/make_golden_clouds.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('reference checkout not present: fixtures can only be regenerated in the build container')

import numpy as np


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


sys.modules['torchvision'] = types.ModuleType('torchvision')
sys.modules['torchvision.transforms'] = types.ModuleType('torchvision.transforms')
sys.modules['torchvision.transforms'].Compose = _Compose


def _load(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(REF, 'lib', 'datasets', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sample_cloud = _load('cloud_sampling').sample_cloud
ComposeCloudTransformation = _load('cloud_transformations').ComposeCloudTransformation

N = 24
M = 2 * N
VALUES = dict(cloud_translate_shift=[0.1, -0.2, 0.05], cloud_scale_scale=1.7, cloud_noise_scale=0.01)
CONFIGS = {
    'none': {},
    'orig': dict(cloud_rescale2orig=True, cloud_recenter2orig=True),
    'translate': dict(cloud_translate=True),
    'scale': dict(cloud_scale=True),
    'noise': dict(cloud_noise=True),
    'center': dict(cloud_center=True),
    'all_nocenter': dict(cloud_rescale2orig=True, cloud_recenter2orig=True, cloud_translate=True, cloud_scale=True, cloud_noise=True),
    'all': dict(cloud_rescale2orig=True, cloud_recenter2orig=True, cloud_translate=True, cloud_scale=True, cloud_noise=True,
                cloud_center=True),
}
ROWS = [0, 1, 2, 0, 1, 2]
SEEDS = [2201, 2202, 2203, 2204, 2205, 2206]


def meshes():
    rng = np.random.RandomState(22)
    out = []
    # 0: 77 faces on 40 vertices
    v = rng.uniform(-0.5, 0.5, (40, 3)).astype(np.float32)
    f = np.stack([rng.choice(40, 3, replace=False) for _ in range(77)]).astype(np.uint32)
    out.append((v, f))
    # 1: 12 faces on 12 vertices; face 0 (leading) and face 5 (interior) have zero area: they name one vertex twice
    v = rng.uniform(-0.5, 0.5, (12, 3)).astype(np.float32)
    f = np.stack([rng.choice(12, 3, replace=False) for _ in range(12)]).astype(np.uint32)
    f[0, 1] = f[0, 0]
    f[5, 2] = f[5, 1]
    out.append((v, f))
    # 2: a single face
    v = rng.uniform(-0.5, 0.5, (3, 3)).astype(np.float32)
    out.append((v, np.array([[0, 1, 2]], np.uint32)))
    return out


def main():
    ms = meshes()
    vertices_c = np.concatenate([v for v, _ in ms]).astype(np.float32)
    faces_vc = np.concatenate([f for _, f in ms]).astype(np.uint32)
    vb = np.cumsum([0] + [len(v) for v, _ in ms]).astype(np.uint64)
    fb = np.cumsum([0] + [len(f) for _, f in ms]).astype(np.uint64)
    rng = np.random.RandomState(23)
    orig_c = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    orig_s = rng.uniform(0.5, 2.0, 3).astype(np.float32)

    B = len(ROWS)
    u = np.zeros((B, M))
    words = np.zeros((B, M), np.uint32)
    s1 = np.zeros((B, M), np.float32)
    s2 = np.zeros((B, M), np.float32)
    normals = np.zeros((B, 3, M), np.float32)          # [.., 2i] the cloud's draw i, [.., 2i+1] the eval cloud's
    normals64 = np.zeros((B, 3, M))
    ref_faces = np.zeros((B, M), np.int64)
    outs = {k: (np.zeros((B, 3, N), np.float32), np.zeros((B, 3, N), np.float32)) for k in CONFIGS}
    for r, (shape, seed) in enumerate(zip(ROWS, SEEDS)):
        v, f = ms[shape]
        # ---- replay of the draws
        np.random.seed(seed)
        u[r] = np.random.random_sample(M)
        s1[r] = np.random.random((M, 1)).astype(np.float32)[:, 0]
        s2[r] = np.random.random((M, 1)).astype(np.float32)[:, 0]
        normals64[r, :, 0::2] = np.random.normal(size=(3, N))
        normals64[r, :, 1::2] = np.random.normal(size=(3, N))
        normals[r] = normals64[r].astype(np.float32)
        words[r] = np.floor(u[r] * 2.0**32).astype(np.uint32)
        # ---- what RandomState.choice does with them (restated only to CHECK the recorded draws against the reference's output)
        polygons = v[f]
        cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
        areas = np.sqrt((cross**2).sum(1)) / 2.0
        probs = areas / areas.sum()
        cdf = np.cumsum(probs.astype(np.float64))
        cdf /= cdf[-1]
        ref_faces[r] = cdf.searchsorted(u[r], side='right')
        word_faces = np.searchsorted(np.ceil(cdf * 2.0**32), words[r].astype(np.float64), side='right')
        assert np.array_equal(word_faces, ref_faces[r]), 'word-driven face differs: choose another seed'
        assert np.all(areas[ref_faces[r]] > 0), 'a zero-area face was drawn'
        a1, a2 = s1[r][:, None].copy(), s2[r][:, None].copy()
        cond = (a1 + a2) > 1.
        a1[cond] = 1. - a1[cond]
        a2[cond] = 1. - a2[cond]
        sp = polygons[ref_faces[r]]
        restated = (sp[:, 0] + a1 * (sp[:, 1] - sp[:, 0]) + a2 * (sp[:, 2] - sp[:, 0])).astype(np.float32)
        # ---- the reference
        for name, flags in CONFIGS.items():
            np.random.seed(seed)
            sample = sample_cloud(v, f, size=N, return_eval_cloud=True)
            if name == 'none':
                assert np.array_equal(sample['cloud'], restated[0::2].T) and np.array_equal(sample['eval_cloud'], restated[1::2].T), \
                    'the recorded draws do not reproduce the reference'
            sample['orig_c'], sample['orig_s'] = orig_c[shape], orig_s[shape]
            compose, _ = ComposeCloudTransformation(**dict(VALUES, **flags))
            if compose is not None:
                sample = compose(sample)
            assert sample['cloud'].dtype == np.float32 and sample['eval_cloud'].dtype == np.float32
            outs[name][0][r], outs[name][1][r] = sample['cloud'], sample['eval_cloud']
        # the noise the reference added is the recorded normal (float64) times the scale, rounded to float32
        sc = np.float32(VALUES['cloud_noise_scale'])
        assert np.array_equal(outs['noise'][0][r], outs['none'][0][r] + (sc * normals64[r, :, 0::2]).astype(np.float32))
        assert np.array_equal(outs['noise'][1][r], outs['none'][1][r] + (sc * normals64[r, :, 1::2]).astype(np.float32))

    data = dict(vertices_c=vertices_c, faces_vc=faces_vc, vertices_c_bounds=vb, faces_bounds=fb, orig_c=orig_c, orig_s=orig_s,
                rows=np.asarray(ROWS, np.int32), seeds=np.asarray(SEEDS, np.int64), cloud_size=np.int64(N), u=u, words=words, s1=s1,
                s2=s2, normals=normals, faces=ref_faces,
                translate_shift=np.asarray(VALUES['cloud_translate_shift'], np.float32),
                scale_scale=np.float32(VALUES['cloud_scale_scale']), noise_scale=np.float32(VALUES['cloud_noise_scale']))
    for name, (c, e) in outs.items():
        data['cloud_' + name], data['eval_cloud_' + name] = c, e
    path = os.path.join(HERE, 'g22_clouds.npz')
    np.savez_compressed(path, **data)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
