"""Latent sweeps without a GPU: the ABI additions (gwtf_mixture_route_sweep, gwtf_film_forward_k), every record the sweep routing
entry refuses, the numpy restatement (sweep_ref.py) the GPU tests compare the kernel against, and the guards of
Flow_Mixture_Model.interpolate_many that need no device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN
import generate_ref as gr
import sweep_ref as sr
from test_generate_cpu import _record_fields
from go_with_the_flows_amd import _lib, models, GwtfError

BAD = 10001


def test_sweep_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    handle = _lib.lib()
    for name in ('gwtf_mixture_route_sweep', 'gwtf_film_forward_k'):
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGNATURES and hasattr(handle, name), name
    assert declared == set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header and handle.gwtf_abi_version() == 12
    assert _record_fields(header, 'GwtfRouteSweepArgs') == [n for n, _ in _lib.RouteSweepArgs._fields_]
    # the sweep record is the routing record with three fields in front of the stream; the routing record itself has not moved
    old = [n for n, _ in _lib.RouteArgs._fields_]
    assert _record_fields(header, 'GwtfRouteArgs') == old
    assert [n for n, _ in _lib.RouteSweepArgs._fields_] == old[:-1] + ['group', 'mu0_stride_k', 'lv0_stride_k', 'stream']
    assert _lib._SIGNATURES['gwtf_mixture_route_sweep'] == (ctypes.c_int, [ctypes.c_void_p])
    assert len(_lib._SIGNATURES['gwtf_film_forward_k'][1]) == 11


FAKE = 0x1000                                         # never dereferenced: every check fails before anything is launched
OK = dict(logits=FAKE, mu0=FAKE, lv0=FAKE, state=FAKE, thresholds=FAKE, tile_comp=FAKE, perm=FAKE, zp=FAKE, labels=FAKE,
          S=6, n=8, K=3, P=64, mu0_stride=3, lv0_stride=3, group=3, mu0_stride_k=18, lv0_stride_k=18)


def sweep(**kw):
    record = _lib.RouteSweepArgs(**dict(OK, **kw))    # named: it must outlive the call
    return _lib.lib().gwtf_mixture_route_sweep(ctypes.addressof(record))


def test_the_sweep_routing_entry_refuses_a_null_record_and_bad_groups_and_strides():
    assert _lib.lib().gwtf_mixture_route_sweep(None) == BAD
    for kw in (dict(group=0), dict(group=-1), dict(group=4), dict(S=7), dict(group=12), dict(mu0_stride_k=-18), dict(lv0_stride_k=-1)):
        assert sweep(**kw) == BAD, kw


def test_the_sweep_routing_entry_refuses_what_the_routing_entry_refuses():
    for name in ('logits', 'mu0', 'lv0', 'state', 'tile_comp', 'perm', 'zp', 'labels'):
        assert sweep(**{name: None}) == BAD, name
    assert sweep(state=None, words=FAKE) == BAD       # the normals still need the state
    assert sweep(state=None, z0_in=FAKE) == BAD       # and so do the label words
    for kw in (dict(S=0), dict(n=0), dict(K=0), dict(K=65), dict(P=0), dict(P=100), dict(P=512), dict(mu0_stride=-3),
               dict(lv0_stride=-3), dict(n=(1 << 30) + 1), dict(S=3 << 20, n=1 << 20)):
        assert sweep(**kw) == BAD, kw


def test_the_per_component_film_entry_refuses_bad_arguments():
    L = _lib.lib()
    ok = dict(g=FAKE, pf=FAKE, out=FAKE, B=4, G=16, K=3, Cper=3, f=8, eps=1e-6, stride=64)

    def film(**kw):
        a = dict(ok, **kw)
        return L.gwtf_film_forward_k(a['g'], a['pf'], a['out'], a['B'], a['G'], a['K'], a['Cper'], a['f'], a['eps'], a['stride'], None)
    for kw in (dict(g=None), dict(pf=None), dict(out=None), dict(B=0), dict(G=0), dict(K=0), dict(Cper=0), dict(f=0), dict(f=129),
               dict(stride=-1)):
        assert film(**kw) == BAD, kw


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def inputs(S, T, n, K, seed):
    rng = np.random.RandomState(seed)
    R = S * T
    return dict(logits=rng.normal(0, 1.5, (R, K)).astype(np.float32),
                words=rng.randint(0, 2**32, (S, n), dtype=np.uint64).astype(np.uint32),
                normals=rng.normal(0, 1, (S, 3, n)).astype(np.float32),
                mu0=rng.normal(0, 0.3, (K, R, 3)).astype(np.float32), lv0=rng.normal(-1, 0.5, (K, R, 3)).astype(np.float32))


@pytest.mark.parametrize('S,n,K,P', [(1, 1, 1, 64), (5, 300, 3, 64), (2, 2500, 64, 128)])
def test_with_one_row_per_shape_and_one_base_the_restatement_is_generate_ref(S, n, K, P):
    d = inputs(S, 1, n, K, n + K)
    mu0, lv0 = d['mu0'][0], d['lv0'][0, :1]                                   # per row / shared, no component axis
    got = sr.route(d['logits'], 1, n, K, P, words=d['words'], normals=d['normals'], mu0=mu0, lv0=lv0)
    thr = gr.thresholds(d['logits'])
    labels = gr.labels_of(thr, d['words'])
    tile_comp, perm, _ = gr.layout(labels, K, P)
    z0 = gr.base_samples(d['normals'], mu0, lv0)
    assert np.array_equal(got['thresholds'], thr) and np.array_equal(got['labels'], labels)
    assert np.array_equal(got['tile_comp'], tile_comp) and np.array_equal(got['perm'], perm)
    assert np.array_equal(got['z0'], z0)
    # the same with the Philox draws of a (seed, call)
    got = sr.route(d['logits'], 1, n, K, P, mu0=mu0, lv0=lv0, seed=7, call=3)
    assert np.array_equal(got['labels'], gr.labels_of(thr, gr.label_words(7, 3, S, n)))
    assert np.array_equal(got['z0'], gr.base_samples(gr.normal_draws(7, 3, S, n), mu0, lv0))


def test_restated_rows_of_a_group_share_their_draws_and_take_the_base_of_their_own_component():
    S, T, n, K, P = 2, 3, 300, 3, 64
    d = inputs(S, T, n, K, 11)
    d['logits'] = np.repeat(d['logits'][::T], T, axis=0)                      # equal logits on the rows of a group
    got = sr.route(d['logits'], T, n, K, P, words=d['words'], normals=d['normals'], mu0=d['mu0'], lv0=d['lv0'])
    for s in range(S):
        for t in range(1, T):
            assert np.array_equal(got['labels'][s * T + t], got['labels'][s * T])
            assert np.array_equal(got['perm'][s * T + t], got['perm'][s * T])
    r, i = 4, 17
    k = got['labels'][r, i]
    want = d['normals'][r // T, :, i] * np.exp(np.float32(0.5) * d['lv0'][k, r]) + d['mu0'][k, r]
    assert np.array_equal(got['z0'][r, :, i], want.astype(np.float32))
    valid = got['perm'][r] >= 0
    assert (got['zp'][r][:, ~valid] == 0).all() and np.array_equal(got['zp'][r][:, valid], got['z0'][r][:, got['perm'][r][valid]])
    # explicit labels and base samples are taken from the row's shape as they are
    lab = gr.crafted_labels(n, K, P)[:S]
    got = sr.route(None, T, n, K, P, labels_in=lab, z0_in=d['normals'])
    assert np.array_equal(got['labels'], np.repeat(lab, T, axis=0)) and np.array_equal(got['z0'], np.repeat(d['normals'], T, axis=0))


# ---- interpolate_many: the guards that need no device --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cpu_model():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating')
    return models.Flow_Mixture_Model(**cfg).eval(), cfg


def test_interpolate_many_refuses_bad_arguments_before_it_looks_for_a_device(cpu_model):
    m, cfg = cpu_model
    G, K = cfg['g_latent_space_size'], cfg['n_components']
    a, b = torch.zeros(2, G), torch.ones(2, G)
    for bad in (dict(codes_b=torch.ones(3, G)), dict(codes_b=torch.ones(2, G + 1)), dict(codes_a=torch.zeros(2, G, 1)),
                dict(codes_a=a.numpy()), dict(weights=[]), dict(weights=torch.zeros(0)), dict(weights=torch.zeros(2, 2)),
                dict(flow_idx=[K]), dict(flow_idx=[-1]), dict(flow_idx=[0, K + 3])):
        kw = dict(dict(codes_a=a, codes_b=b, n_points=16), **bad)
        with pytest.raises(GwtfError):
            m.interpolate_many(**kw)
    with pytest.raises(GwtfError, match='no CPU path'):
        m.interpolate_many(a, b, 16)
    with pytest.raises(GwtfError, match='no CPU path'):
        m.interpolate_many(a, b, 16, weights=[0.5], flow_idx=[0])
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.interpolate_many(a, b, 16)
    finally:
        m.eval()
    assert hasattr(models.Flow_Mixture_SVR_Model, 'interpolate_many') and hasattr(models.Flow_Mixture_Model, 'upsample_many')
    assert np.array_equal(np.float32(models.Flow_Mixture_Model._SWEEP_WEIGHTS), np.float32(np.arange(1, 10) / 10))
