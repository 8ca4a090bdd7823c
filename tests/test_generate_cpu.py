"""Device-resident generation without a GPU: the ABI additions (gwtf_mixture_route, gwtf_stack_forward_routed, gwtf_route_tiles),
the tile bound, and the properties of the numpy restatement (generate_ref.py) the GPU tests compare the routing kernel against."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import generate_ref as gr
from go_with_the_flows_amd import _lib

SEED = gr.SEED
BAD = 10001


def _record_fields(header, name):
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1), flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        names += [re.search(r'(\w+)\s*(?:\[\d+\])?$', piece.strip()).group(1) for piece in decl.split(',')]
    return names


def test_abi_additions_are_declared_bound_and_check_their_arguments():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    for name in ('gwtf_mixture_route', 'gwtf_stack_forward_routed', 'gwtf_route_tiles'):
        assert name in declared and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header
    assert _record_fields(header, 'GwtfRouteArgs') == [n for n, _ in _lib.RouteArgs._fields_]
    assert _record_fields(header, 'GwtfRoutedStackArgs') == [n for n, _ in _lib.RoutedStackArgs._fields_]
    L = _lib.lib()
    assert L.gwtf_abi_version() == 12
    fake = 0x1000                                     # never dereferenced: every check below fails before anything is launched

    ok = dict(logits=fake, mu0=fake, lv0=fake, state=fake, thresholds=fake, tile_comp=fake, perm=fake, zp=fake, labels=fake,
              S=2, n=8, K=3, P=64, mu0_stride=3, lv0_stride=3)

    def route(**kw):
        record = _lib.RouteArgs(**dict(ok, **kw))     # named: it must outlive the call
        return L.gwtf_mixture_route(ctypes.addressof(record))
    assert L.gwtf_mixture_route(None) == BAD
    for name in ('logits', 'mu0', 'lv0', 'state', 'tile_comp', 'perm', 'zp', 'labels'):
        assert route(**{name: None}) == BAD, name
    assert route(state=None, words=fake) == BAD       # the normals still need the state
    assert route(state=None, z0_in=fake) == BAD       # and so do the label words
    for kw in (dict(S=0), dict(n=0), dict(K=0), dict(K=65), dict(P=0), dict(P=100), dict(P=512), dict(mu0_stride=-3)):
        assert route(**kw) == BAD, kw

    ok2 = dict(zp=fake, weights=fake, film=fake, tile_comp=fake, perm=fake, out=fake, K=3, S=2, n=8, P=64, C=3, f=8, pattern0=0,
               eps=1e-6)

    def routed(**kw):
        record = _lib.RoutedStackArgs(**dict(ok2, **kw))
        return L.gwtf_stack_forward_routed(ctypes.addressof(record))
    assert L.gwtf_stack_forward_routed(None) == BAD
    for name in ('zp', 'weights', 'film', 'tile_comp', 'perm', 'out'):
        assert routed(**{name: None}) == BAD, name
    for kw in (dict(S=0), dict(n=0), dict(K=0), dict(K=65), dict(P=96), dict(C=0), dict(f=0), dict(pattern0=6)):
        assert routed(**kw) == BAD, kw
    assert routed(f=129) == 10002 and routed(f=100, P=256) == 10002          # widths / tiles no instantiation covers


@pytest.mark.parametrize('P', [64, 128, 256])
def test_route_tiles_is_the_stated_bound_and_the_layout_fits_it(P):
    L = _lib.lib()
    rng = np.random.RandomState(5)
    for n in (1, 63, 64, 65, 300, 2048, 2500):
        for K in (1, 3, 16, 64):
            tiles = L.gwtf_route_tiles(n, K, P)
            assert tiles == (n + K * (P - 1)) // P == gr.route_tiles(n, K, P) == _lib.route_tiles(n, K, P)
            one = np.zeros(n, np.int32)                                   # all points in one component
            spread = (np.arange(n) % K).astype(np.int32)                  # one point per component (as far as n reaches)
            rand = rng.randint(0, K, n).astype(np.int32)
            _, _, used = gr.layout(np.stack([one, spread, rand]), K, P)
            assert used.max() <= tiles, (n, K, P, used)
            if n >= K:                                                    # the bound is attained: K - 1 components of one point ...
                tight = np.concatenate([np.arange(K - 1), np.full(n - (K - 1), K - 1)]).astype(np.int32)
                if (n - (K - 1)) % P == 1 or K == 1 and n % P == 0:
                    assert gr.layout(tight[None], K, P)[2][0] == tiles
    assert L.gwtf_route_tiles(0, 3, 64) == 0 and L.gwtf_route_tiles(8, 0, 64) == 0 and L.gwtf_route_tiles(8, 3, 100) == 0


@pytest.mark.parametrize('n,K,P', [(1, 1, 64), (300, 3, 64), (300, 3, 256), (2500, 64, 128), (777, 16, 128)])
def test_restated_layout_is_a_stable_bijection_in_component_order(n, K, P):
    rng = np.random.RandomState(n + K)
    labels = rng.randint(0, K, (4, n)).astype(np.int32)
    labels[1] = K - 1
    tile_comp, perm, used = gr.layout(labels, K, P)
    for s in range(4):
        valid = perm[s] >= 0
        assert sorted(perm[s][valid].tolist()) == list(range(n))                       # a bijection onto 0 .. n-1
        tc = tile_comp[s]
        assert (tc[:used[s]] >= 0).all() and (tc[used[s]:] == -1).all() and (np.diff(tc[:used[s]]) >= 0).all()
        slot_comp = np.repeat(tc, P)
        assert (labels[s][perm[s][valid]] == slot_comp[valid]).all()                   # every point sits in a tile of its component
        for k in range(K):                                                             # stable: original order inside a component
            own = perm[s][valid & (slot_comp == k)]
            assert (np.diff(own) > 0).all()
            assert len(own) == (labels[s] == k).sum()
            first = np.nonzero(slot_comp == k)[0]
            if len(first):                                                             # no holes: padding only at the end of the run
                assert valid[first[0]:first[0] + len(own)].all()


def test_crafted_label_rows_sit_on_the_edges():
    lab = gr.crafted_labels(300, 3, 64)
    counts = np.stack([np.bincount(r, minlength=3) for r in lab])
    assert counts[0].max() == 300 and counts[1][0] == 64 and counts[2][0] == 65 and counts[3][1] == 1 and counts[4][1] == 0
    assert (counts.sum(1) == 300).all()


def test_restated_philox_labels_follow_the_mixture_weights():
    n, logits = 20000, np.array([[0.0, 1.0, -1.0]], np.float32)
    thr = gr.thresholds(logits)
    assert thr[0, -1] == 0xffffffff and (np.diff(thr[0].astype(np.int64)) > 0).all()
    labels = gr.labels_of(thr, gr.label_words(SEED, 0, 1, n))
    p = np.exp(logits[0].astype(np.float64))
    p /= p.sum()
    counts = np.bincount(labels[0], minlength=3)
    sigma = np.sqrt(n * p * (1 - p))
    assert (np.abs(counts - n * p) < 5 * sigma).all(), (counts, n * p, sigma)
    # thresholds against the float64 search they stand for
    w = gr.label_words(SEED, 1, 1, 4096)
    cdf = np.cumsum(p) / np.cumsum(p)[-1]
    assert np.array_equal(gr.labels_of(thr, w)[0], np.minimum(np.searchsorted(cdf, w[0] * 2.0**-32, side='right'), 2))
