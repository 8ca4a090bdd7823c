"""The stored-cloud sampler without a device: its ABI additions, the C++ index rule (gwtf_perm_index) against the numpy restatement
(cloud_store_ref.py), the restatement's own properties, and the host-side refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import clouds_ref as cr
import cloud_store_ref as sr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib

KEY_SETS = [(0, 0, 0, 0, 0, 0), (1, 2, 3, 4, 5, 6), (0xffffffff, 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x12345678, 0xdeadbeef)]
SMALL_P = (1, 2, 3, 4, 5, 16, 17, 64, 65, 257)


# ---- C1 ---------------------------------------------------------------------------------------------------------------------------
def test_abi_additions_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('gwtf_sample_stored_clouds', 'gwtf_perm_index'):
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGNATURES and hasattr(handle, name), name
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header and _lib.lib().gwtf_abi_version() == 12
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct GwtfStoredCloudArgs \{(.*?)\} GwtfStoredCloudArgs;', header, re.S).group(1),
                  flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        names += [re.search(r'(\w+)\s*(?:\[\d+\])?$', piece.strip()).group(1) for piece in decl.split(',')]
    assert names == [n for n, _ in _lib.StoredCloudArgs._fields_]
    assert names == ['rows', 'points', 'bounds', 'orig_c', 'orig_s', 'cloud', 'eval_cloud', 'partials', 'state', 'index', 'normals',
                     'B', 'M', 'n_shapes', 'rescale', 'recenter', 'translate', 'scale', 'noise', 'center', 'permute', 'tune',
                     'shift', 'scale_div', 'noise_scale', 'stream']
    # 11 pointers, 11 ints, 5 floats (152 bytes: no padding), the stream pointer
    assert ctypes.sizeof(_lib.StoredCloudArgs) == 11 * 8 + 11 * 4 + 5 * 4 + 8
    assert len(_lib.CloudArgs._fields_) == 31                      # the mesh sampler's record did not move


# ---- C2 ---------------------------------------------------------------------------------------------------------------------------
def _c_perm(keys, ts, P):
    L = _lib.lib()
    k = (ctypes.c_uint * 6)(*keys)
    return np.array([L.gwtf_perm_index(k, int(t), int(P)) for t in ts], np.uint32)


@pytest.mark.parametrize('keys', KEY_SETS)
def test_the_cpp_rule_equals_the_restatement_and_is_a_bijection(keys):
    for P in SMALL_P:
        t = np.arange(P)
        got = _c_perm(keys, t, P)
        assert np.array_equal(got, sr.perm_index(keys, t, P)), P
        assert sorted(got.tolist()) == list(range(P)), P
    rng = np.random.RandomState(5)
    for P in (100003, 2**31 - 1):
        t = rng.randint(0, P, 4096)
        got = _c_perm(keys, t, P)
        assert got.max() < P and np.array_equal(got, sr.perm_index(keys, t, P)), P


def test_the_cpp_rule_refuses_what_lies_outside():
    L = _lib.lib()
    k = (ctypes.c_uint * 6)(*KEY_SETS[1])
    assert L.gwtf_perm_index(k, 5, 5) == 0xffffffff and L.gwtf_perm_index(k, 0, 0) == 0xffffffff
    assert L.gwtf_perm_index(k, 0, 2**31) == 0xffffffff and L.gwtf_perm_index(None, 0, 4) == 0xffffffff
    assert L.gwtf_perm_index(k, 0, 1) == 0


# ---- C3 ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_properties():
    assert [sr.half_bits(P) for P in (1, 2, 3, 4, 5, 16, 17, 257, 100003, 2**31 - 1)] == [1, 1, 1, 1, 2, 2, 3, 5, 9, 16]
    for P in (1, 2, 5, 17, 64, 257, 1000):
        idx = sr.stored_indices(77, 3, [P, P], P)
        assert sorted(idx[0].tolist()) == list(range(P)) and sorted(idx[1].tolist()) == list(range(P))     # M = P: a permutation
        if P >= 17:
            assert not np.array_equal(idx[0], idx[1])                                                      # rows differ
            assert not np.array_equal(idx[0], sr.stored_indices(77, 4, [P], P)[0])                         # calls differ
            assert not np.array_equal(idx[0], sr.stored_indices(78, 3, [P], P)[0])                         # seeds differ
        wrapped = sr.stored_indices(77, 3, [P], 3 * P + 2)[0]
        counts = np.bincount(wrapped, minlength=P)
        if P == 1:
            assert counts.tolist() == [5]
        elif P == 2:
            assert counts.tolist() == [4, 4]
        else:
            assert counts.min() == 3 and counts.max() == 4 and int((counts == 4).sum()) == 2, P
        for q in range(3):                                                                                 # every round is a permutation
            assert sorted(wrapped[q * P:(q + 1) * P].tolist()) == list(range(P))
    assert np.array_equal(sr.stored_indices(1, 0, [5, 3], 7, permute=False), [[0, 1, 2, 3, 4, 0, 1], [0, 1, 2, 0, 1, 2, 0]])


def uniformity_counts(index_of_call):
    """(inclusion counts, first-draw counts) over 64 calls of 64 rows x 8 draws from one cloud of 37 points."""
    inclusion, first = np.zeros(37, np.int64), np.zeros(37, np.int64)
    for call in range(64):
        idx = index_of_call(call)
        assert idx.shape == (64, 8)
        inclusion += np.bincount(idx.ravel(), minlength=37)
        first += np.bincount(idx[:, 0], minlength=37)
    return inclusion, first


def test_restatement_uniformity():
    """The bounds of the device test: 5 binomial standard deviations around n 8/37 = 885.6 (sd 26.3) and n/37 = 110.7 (sd 10.4),
    n = 4096."""
    inclusion, first = uniformity_counts(lambda call: sr.stored_indices(1234, call, [37] * 64, 8))
    assert inclusion.sum() == 4096 * 8 and first.sum() == 4096
    print(f'CLOUDSTORE restatement: inclusion worst {np.abs(inclusion - 4096 * 8 / 37).max():.1f} (bar 131), '
          f'first worst {np.abs(first - 4096 / 37).max():.1f} (bar 51)')
    assert np.abs(inclusion - 4096 * 8 / 37).max() <= 131 and np.abs(first - 4096 / 37).max() <= 51


# ---- C4 ---------------------------------------------------------------------------------------------------------------------------
def test_refused_records_return_badarg_without_a_device():
    L = _lib.lib()
    assert L.gwtf_sample_stored_clouds(None) == 10001
    fake = 0x1000                                     # never dereferenced: every check below fails before anything is launched
    ok = dict(rows=fake, points=fake, bounds=fake, cloud=fake, eval_cloud=fake, state=fake, B=2, M=8, n_shapes=1, permute=1)

    def call(**kw):
        record = _lib.StoredCloudArgs(**dict(ok, **kw))
        return L.gwtf_sample_stored_clouds(ctypes.addressof(record))
    for name in ('rows', 'points', 'bounds', 'cloud', 'state'):
        assert call(**{name: None}) == 10001, name
    assert call(M=7) == 10001                         # odd M with an eval cloud
    assert call(B=0) == 10001 and call(B=65536) == 10001 and call(M=0) == 10001 and call(n_shapes=0) == 10001
    assert call(scale=1, scale_div=0.0) == 10001 and call(scale=1, scale_div=-2.0) == 10001
    assert call(noise=1, noise_scale=0.0) == 10001 and call(noise=1, noise_scale=-0.01) == 10001
    assert call(center=1) == 10001                    # no scratch
    assert call(rescale=1) == 10001 and call(recenter=1) == 10001          # no orig_s / orig_c
    assert call(normals=fake) == 10001 and call(noise=1, noise_scale=1.0, normals=fake) == 10001      # normals without index
    assert call(noise=1, noise_scale=1.0, index=fake) == 10001             # explicit indices, noise on, no normals


def test_store_construction_checks():
    pts = np.arange(30, dtype=np.float32).reshape(10, 3)
    st = gw.CloudStore.from_arrays(pts, [0, 4, 10], orig_c=np.zeros((2, 3)), orig_s=[1.0, 2.0], device='cpu')
    assert len(st) == 2 and st.device == torch.device('cpu') and st.bounds.tolist() == [0, 4, 10] and st.points.shape == (10, 3)
    assert st.orig_c.shape == (2, 3) and st.orig_s.tolist() == [1.0, 2.0] and st._work == {} and st._state is None
    cube = gw.CloudStore.from_arrays(np.zeros((3, 5, 3)), device='cpu')
    assert len(cube) == 3 and cube.bounds.tolist() == [0, 5, 10, 15] and cube.orig_c is None and cube.orig_s is None
    with pytest.raises(gw.GwtfError, match='cloud 1 has no points'):
        gw.CloudStore.from_arrays(pts, [0, 4, 4, 10], device='cpu')
    with pytest.raises(gw.GwtfError, match='ascending'):
        gw.CloudStore.from_arrays(pts, [0, 6, 4, 10], device='cpu')
    with pytest.raises(gw.GwtfError, match='ascending'):
        gw.CloudStore.from_arrays(pts, [0, 4, 11], device='cpu')
    with pytest.raises(gw.GwtfError, match=r'\(T, 3\)'):
        gw.CloudStore.from_arrays(np.zeros((10, 2)), [0, 10], device='cpu')
    with pytest.raises(gw.GwtfError, match=r'\(S, P, 3\)'):
        gw.CloudStore.from_arrays(np.zeros((10, 3)), device='cpu')
    with pytest.raises(gw.GwtfError, match='n_shapes'):
        gw.CloudStore.from_arrays(pts, [0], device='cpu')
    with pytest.raises(TypeError):
        gw.CloudStore()
    with pytest.raises(gw.GwtfError, match='no CPU path'):
        gw.sample_clouds(st, torch.zeros(1, dtype=torch.int32), 2)
    with pytest.raises(gw.GwtfError, match='n_points'):
        st.clouds(n_points=5)                         # the smallest cloud holds 4
    with pytest.raises(gw.GwtfError, match='rows'):
        st.clouds(rows=[2])


def test_permute_false_is_for_stored_clouds_only():
    v, f = cr.random_mesh(4, 6, 2)
    meshes = gw.MeshStore.from_arrays(*cr.pack([(v, f)] * 3), device='cpu')
    with pytest.raises(ValueError, match='stored order'):
        gw.DeviceCloudLoader(meshes, 2, 8, permute=False)
    with pytest.raises(ValueError, match='stored order'):
        gw.sample_clouds(meshes, torch.zeros(1, dtype=torch.int32), 8, permute=False)
    stored = gw.CloudStore.from_arrays(np.zeros((3, 5, 3)), device='cpu')
    loader = gw.DeviceCloudLoader(stored, 2, 2, permute=False, shuffle=False)
    assert loader.permute is False and len(loader) == 1 and gw.DeviceCloudLoader(stored, 2, 2).permute is True
