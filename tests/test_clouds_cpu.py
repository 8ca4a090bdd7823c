"""Host side of the device cloud sampler (go_with_the_flows_amd/clouds.py, csrc/gwtf_clouds.hip): threshold encoding, the Philox
restatement the GPU tests compare against, the loader's index plan, the ABI additions and the argument checks.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import clouds_ref as cr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, clouds


@pytest.fixture(scope='module')
def fx():
    return golden('g22_clouds')


@pytest.fixture(scope='module')
def store(fx):
    return gw.MeshStore.from_arrays(fx['vertices_c'], fx['faces_vc'], fx['vertices_c_bounds'], fx['faces_bounds'], fx['orig_c'],
                                    fx['orig_s'], device='cpu')


def _packed(fx):
    return fx['vertices_c'], fx['faces_vc'], fx['vertices_c_bounds'], fx['faces_bounds']


def test_thresholds_are_the_ceiling_of_the_reference_cdf(fx, store):
    fb = fx['faces_bounds'].astype(np.int64)
    assert store.n_shapes == 3 and fx['vertices_c_bounds'][1] != 0
    for shape in range(3):
        v, f = cr.shape_arrays(_packed(fx), shape)
        t = np.ceil(cr.reference_cdf(v, f)[2] * 2.0**32)
        assert t[-1] == 2.0**32
        n = int(store.search_len_host[shape])
        mine = store.thresholds_host[fb[shape]:fb[shape + 1]]
        assert n == np.count_nonzero(t < 2.0**32) and n < len(f)
        assert np.array_equal(mine[:n].astype(np.float64), t[:n])
        assert np.all(mine[n:] == 0xffffffff) and np.all(t[n:] == 2.0**32)     # 2^32 itself does not fit: above every word
        assert np.array_equal(store.thresholds.numpy().view(np.uint32)[fb[shape]:fb[shape + 1]], mine)
    assert store.thresholds_host[fb[1]] == 0                                    # the leading zero-area face of mesh 1
    assert store.search_len_host[2] == 0                                        # a single face: nothing to search


def test_integer_search_equals_the_float64_search_and_skips_zero_area_faces(fx, store):
    fb = fx['faces_bounds'].astype(np.int64)
    rng = np.random.RandomState(5)
    for shape in range(3):
        v, f = cr.shape_arrays(_packed(fx), shape)
        areas, _, cdf = cr.reference_cdf(v, f)
        words = rng.randint(0, 2**32, 100000, dtype=np.uint64).astype(np.uint32)
        words[:4] = [0, 1, 0xfffffffe, 0xffffffff]
        t = store.thresholds_host[fb[shape]:fb[shape + 1]]
        words[4:4 + len(t)] = t                                                 # every boundary word itself
        words[4 + len(t):4 + 2 * len(t)] = t - np.uint32(1)                     # and the word below it
        got = clouds.search_faces(t, int(store.search_len_host[shape]), words)
        assert np.array_equal(got, np.searchsorted(cdf, words.astype(np.float64) * 2.0**-32, side='right'))
        assert got.max() < len(f) and np.all(areas[got] > 0)
    assert np.count_nonzero(cr.reference_cdf(*cr.shape_arrays(_packed(fx), 1))[0] == 0) == 2


def test_philox_restatement_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, key, want in kat:
        out = cr.philox4x32_10([np.array([c], np.uint32) for c in ctr], key)
        assert ' '.join('%08x' % int(o[0]) for o in out) == want
    # the draws of a call: counter (j, r, call lo, call hi | stream << 28), key (seed lo, seed hi)
    seed, call = 0x299f31d0a4093822, (0x3707344 << 32) | 0x13198a2e
    w = cr.draws(seed, call, 3, 5, stream=1)
    one = cr.philox4x32_10([np.array([x], np.uint32) for x in (4, 2, 0x13198a2e, 0x3707344 | (1 << 28))], (0xa4093822, 0x299f31d0))
    assert [int(x[2, 4]) for x in w] == [int(x[0]) for x in one]
    _, s1, s2 = cr.sampling_draws(7, 0, 2, 1000)
    assert s1.dtype == np.float32 and 0 <= s1.min() and s1.max() < 1 and 0 <= s2.min() and s2.max() < 1


def _loader(n, **kw):
    v, f = cr.random_mesh(4, 6, 1)
    st = gw.MeshStore.from_arrays(*cr.pack([(v, f)] * n), device='cpu')
    return gw.DeviceCloudLoader(st, cloud_size=8, **kw)


def test_loader_index_plan():
    ld = _loader(7, batch_size=3)
    assert len(ld) == 2 and len(_loader(7, batch_size=3, drop_last=False)) == 3                     # drop_last is the default
    e0, e1 = ld.index_plan(0), ld.index_plan(1)
    assert sorted(e0.tolist()) == list(range(7)) and sorted(e1.tolist()) == list(range(7))          # every shape once per epoch
    assert e0.tolist() != e1.tolist()
    ld.set_epoch(1)
    assert ld.index_plan().tolist() == e1.tolist()
    assert _loader(7, batch_size=3, seed=1).index_plan(0).tolist() != e0.tolist()
    assert _loader(7, batch_size=3, shuffle=False).index_plan(4).tolist() == list(range(7))
    from torch.utils.data import DistributedSampler
    for world in (2, 3):
        seen = []
        for rank in range(world):
            ld = _loader(7, batch_size=2, seed=11, rank=rank, world_size=world)
            ds = DistributedSampler(range(7), num_replicas=world, rank=rank, shuffle=True, seed=11)
            for epoch in (0, 3):
                ds.set_epoch(epoch)
                ld.set_epoch(epoch)
                assert ld.index_plan().tolist() == list(iter(ds))
            assert len(ld) == len(ds) // 2
            seen += ld.index_plan().tolist()
        assert sorted(set(seen)) == list(range(7)) and len(seen) == world * -(-7 // world)          # padded, nothing dropped


def test_abi_additions_are_declared_bound_and_check_their_arguments():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    for name in ('gwtf_sample_clouds', 'gwtf_cloud_partials'):
        assert name in declared and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header
    # the ctypes mirror follows the record field for field
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct GwtfCloudArgs \{(.*?)\} GwtfCloudArgs;', header, re.S).group(1), flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        names += [re.search(r'(\w+)\s*(?:\[\d+\])?$', piece.strip()).group(1) for piece in decl.split(',')]
    assert names == [n for n, _ in _lib.CloudArgs._fields_]
    L = _lib.lib()
    assert L.gwtf_abi_version() == 12
    assert L.gwtf_cloud_partials(4096) == 16 and L.gwtf_cloud_partials(257) == 2 and L.gwtf_cloud_partials(0) == 0
    assert L.gwtf_sample_clouds(None) == 10001
    fake = 0x1000                                     # never dereferenced: every check below fails before anything is launched
    ok = dict(rows=fake, vertices=fake, faces=fake, thresholds=fake, vertices_bounds=fake, faces_bounds=fake, search_len=fake,
              cloud=fake, eval_cloud=fake, state=fake, B=2, M=8, n_shapes=1)

    def call(**kw):
        record = _lib.CloudArgs(**dict(ok, **kw))     # named: it must outlive the call
        return L.gwtf_sample_clouds(ctypes.addressof(record))
    for name in ('rows', 'vertices', 'faces', 'thresholds', 'vertices_bounds', 'faces_bounds', 'search_len', 'cloud', 'state'):
        assert call(**{name: None}) == 10001, name
    assert call(M=7) == 10001                         # odd M with an eval cloud
    assert call(B=0) == 10001 and call(M=0) == 10001
    assert call(scale=1, scale_div=0.0) == 10001 and call(scale=1, scale_div=-2.0) == 10001
    assert call(noise=1, noise_scale=0.0) == 10001 and call(noise=1, noise_scale=-0.01) == 10001
    assert call(center=1) == 10001                    # no scratch
    assert call(rescale=1) == 10001 and call(recenter=1) == 10001          # no orig_s / orig_c
    assert call(words=fake) == 10001 and call(s1=fake) == 10001            # explicit draws given in part


def test_transform_config():
    t = gw.CloudTransform.from_config(cloud_rescale2orig=True, cloud_recenter2orig=False, cloud_translate=True,
                                      cloud_translate_shift=[0.1, -0.2, 0.05], cloud_scale=True, cloud_scale_scale=1.7, cloud_noise=True,
                                      cloud_noise_scale=0.01, cloud_center=True, cloud_random_rotate=False, batch_size=64)
    assert (t.rescale2orig, t.recenter2orig, t.translate, t.scale, t.noise, t.center) == (True, False, True, True, True, True)
    assert t.translate_shift == tuple(float(np.float32(x)) for x in (0.1, -0.2, 0.05)) and t.scale_scale == float(np.float32(1.7))
    none = gw.CloudTransform.from_config()
    assert not (none.rescale2orig or none.recenter2orig or none.translate or none.scale or none.noise or none.center)
    with pytest.raises(NotImplementedError, match='Rotation'):
        gw.CloudTransform.from_config(cloud_random_rotate=True)
    with pytest.raises(ValueError):
        gw.CloudTransform.from_config(cloud_noise=True, cloud_noise_scale=-1.0)


def test_empty_and_zero_area_shapes_raise(fx):
    v, f = cr.random_mesh(4, 6, 2)
    with pytest.raises(gw.GwtfError, match='shape 1 has no faces'):
        gw.MeshStore.from_arrays(np.concatenate([v, v]), f, [0, 6, 12], [0, 4, 4], device='cpu')
    flat = f.copy()
    flat[:, 2] = flat[:, 1]                                                  # every face names a vertex twice
    with pytest.raises(gw.GwtfError, match='shape 1 has zero total face area'):
        gw.MeshStore.from_arrays(np.concatenate([v, v]), np.concatenate([f, flat]), [0, 6, 12], [0, 4, 8], device='cpu')
    with pytest.raises(gw.GwtfError, match='outside the shape'):
        gw.MeshStore.from_arrays(v, f + 3, [0, 6], [0, 4], device='cpu')
    st = gw.MeshStore.from_arrays(v, f, [0, 6], [0, 4], device='cpu')
    with pytest.raises(gw.GwtfError, match='no CPU path'):
        gw.sample_clouds(st, torch.zeros(1, dtype=torch.int32), 8)


def test_h5_wrapper_says_so_when_h5py_is_absent():
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(gw.GwtfError, match='h5py'):
            gw.MeshStore.from_h5('/nonexistent/meshes.h5', 'train', device='cpu')
