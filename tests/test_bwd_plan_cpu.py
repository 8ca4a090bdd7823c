"""The launch plan of the coupling backward (csrc/gwtf_bwd.hip bwd_plan, exported host-only as gwtf_bwd_plan): which kernel variant
runs, on which grid, with how many tiles per workgroup -- asked without launching anything, and compared to the rules restated here."""
import ctypes

import pytest

from go_with_the_flows_amd import _lib

E = 10001                                  # GWTF_E_BADARG
DIRECT, LIGHT, MERGED = 0, 2, 3            # include/gwtf.h GWTF_BWD_PASS_*
SMALL, SINGLE = _lib.TUNE_SMALL_LIGHT_TILE, _lib.TUNE_SINGLE_TILE
KEYS = ('MB', 'NB', 'MG', 'K2', 'FULL', 'tpw', 'grid_x', 'grid_y')


def plan(pas, f, B, N, K=1, pat=0, tune=0):
    out = (ctypes.c_int * 8)()
    rc = _lib.lib().gwtf_bwd_plan(pas, f, B, N, K, pat, tune, out)
    return rc if rc else dict(zip(KEYS, out))


def ceil_div(a, b):
    return -(-a // b)


def rules(pas, f, B, N, K=1, pat=0, tune=0):
    """The plan as the design states it: 64-point tiles below 64 Ki points and 128-point ones from there; at the abs-form widths
    (f = 33..40) the train pipeline's passes take the MG = 1 kernels, per warp-pattern class from 128 points up; the light pass takes
    256-point tiles where it fills the GPU (several per workgroup at the abs-form widths); the merged pass a full-tile kernel."""
    MB = ceil_div(f, 16)
    if not 1 <= MB <= 6:
        return E
    nb = 2 if B * N >= 65536 else 1
    p = dict(MB=MB, NB=nb, MG=-1, K2=-1, FULL=0, tpw=1, grid_x=B * ceil_div(N, 64 * nb), grid_y=K)
    large = pas == LIGHT and nb == 2 and B * N * K >= 262144 and not tune & SMALL
    if 33 <= f <= 40 and pas in (LIGHT, MERGED):
        if large:
            tps = ceil_div(N, 256)
            tpw = 1 if tune & SINGLE else max(1, min(tps, B * tps * K // 512))
            p.update(NB=4, MG=1, K2=1 if pat < 3 else 0, tpw=tpw, grid_x=B * ceil_div(tps, tpw))
        elif nb == 1:
            p.update(NB=1, MG=1)
        else:
            p.update(NB=2, MG=1, K2=1 if pat < 3 else 0, FULL=int(pas == MERGED and N % 128 == 0))
    elif large and MB <= 3:
        p.update(NB=4, grid_x=B * ceil_div(N, 256))
    return p if p['grid_x'] < 2 ** 31 else E


def tup(p):
    return tuple(p[k] for k in KEYS)


CELLS = [(DIRECT, 8, 2, 5, 1, 0, 0), (LIGHT, 37, 2, 130, 1, 0, 0), (MERGED, 37, 32, 2048, 1, 2, 0), (MERGED, 37, 32, 2048, 1, 4, 0),
         (MERGED, 37, 33, 2000, 1, 0, 0), (MERGED, 37, 64, 2048, 4, 0, 0), (LIGHT, 37, 33, 2000, 4, 1, 0),
         (LIGHT, 37, 33, 2000, 4, 4, 0), (LIGHT, 37, 33, 2000, 4, 1, SINGLE), (LIGHT, 37, 33, 2000, 4, 1, SMALL),
         (LIGHT, 19, 33, 2000, 4, 0, 0), (LIGHT, 64, 33, 2000, 4, 0, 0)]
CELLS += [(pas, f, 32, 2048, 1, 0, 0) for pas in (DIRECT, LIGHT, MERGED) for f in (32, 33, 37, 40, 41, 96, 97)]
CELLS += [(pas, 37, 1, 65535, 1, 3, 0) for pas in (DIRECT, LIGHT, MERGED)]


@pytest.mark.parametrize('cell', CELLS)
def test_plan_follows_the_stated_rules(cell):
    assert plan(*cell) == rules(*cell)


def test_plan_at_the_named_shapes():
    assert tup(plan(DIRECT, 8, 2, 5)) == (1, 1, -1, -1, 0, 1, 2, 1)
    for pas in (DIRECT, LIGHT, MERGED):                                   # the tile threshold: 64 Ki points
        assert plan(pas, 37, 32, 2048)['NB'] == 2 and plan(pas, 37, 1, 65535)['NB'] == 1
        assert plan(pas, 96, 32, 2048)['MB'] == 6 and plan(pas, 97, 32, 2048) == E
    assert [plan(MERGED, f, 32, 2048)['MG'] for f in (32, 33, 37, 40, 41)] == [-1, 1, 1, 1, -1]
    assert tup(plan(LIGHT, 37, 2, 130)) == (3, 1, 1, -1, 0, 1, 6, 1)
    assert tup(plan(MERGED, 37, 32, 2048, 1, 2)) == (3, 2, 1, 1, 1, 1, 512, 1)
    p = plan(MERGED, 37, 32, 2048, 1, 4)
    assert (p['K2'], p['FULL']) == (0, 1)
    assert plan(MERGED, 37, 33, 2000)['FULL'] == 0
    assert plan(MERGED, 37, 64, 2048, 4)['NB'] == 2                       # the merged pass never takes the large tile
    assert tup(plan(LIGHT, 37, 33, 2000, 4, 1)) == (3, 4, 1, 1, 0, 2, 132, 4)
    assert plan(LIGHT, 37, 33, 2000, 4, 4)['K2'] == 0
    p = plan(LIGHT, 37, 33, 2000, 4, 1, SINGLE)
    assert (p['tpw'], p['grid_x']) == (1, 264)
    p = plan(LIGHT, 37, 33, 2000, 4, 1, SMALL)
    assert (p['NB'], p['K2']) == (2, 1)
    assert tup(plan(LIGHT, 19, 33, 2000, 4)) == (2, 4, -1, -1, 0, 1, 264, 4)
    assert plan(LIGHT, 64, 33, 2000, 4)['NB'] == 2


def test_plan_rejects_bad_arguments():
    L = _lib.lib()
    assert L.gwtf_bwd_plan(MERGED, 37, 32, 2048, 1, 0, 0, None) == E      # a NULL out8
    for pas in (-1, 1, 4):
        assert plan(pas, 37, 32, 2048) == E
    for f in (0, -3, 97):
        assert plan(MERGED, f, 32, 2048) == E
    for B, N, K in ((0, 2048, 1), (-1, 2048, 1), (32, 0, 1), (32, -5, 1), (32, 2048, 0), (32, 2048, -2), (32, 2048, 65)):
        assert plan(MERGED, 37, B, N, K) == E
    assert plan(MERGED, 37, 32, 2048, 64)['grid_y'] == 64
    for pat in (-1, 6):
        assert plan(LIGHT, 37, 32, 2048, 1, pat) == E
    # 2^25 shapes of 2^13 points: 2^25 * 64 workgroups of 128 points = 2^31, one more than an int holds; half of them fit
    assert plan(DIRECT, 37, 1 << 25, 1 << 13) == E and rules(DIRECT, 37, 1 << 25, 1 << 13) == E
    assert plan(DIRECT, 37, 1 << 24, 1 << 13)['grid_x'] == 1 << 30
    # ... and the workspace is sized by the same rule: no partial count, no floats, no reduction for the refused shape
    assert L.gwtf_dw1_partials(1 << 25, 1 << 13) == 0 and L.gwtf_dw1_workspace_floats(37, 1 << 25, 1 << 13) == 0
    assert L.gwtf_dw1_reduce(0x1000, 1, 0x1000, 37 * 37, 37, 1 << 25, 1 << 13, None) == E
    assert L.gwtf_dw1_partials(1 << 24, 1 << 13) == 1 << 30


def test_dw1_workspace_is_sized_by_the_planned_grid():
    """The merged and the direct pass write one dW1 partial per workgroup; the workspace holds gwtf_dw1_partials(B, N) of them."""
    L = _lib.lib()
    for N in (1, 63, 64, 100, 127, 128, 130, 1000, 2000, 2047, 2048, 2049):
        for B in (1, 2, 31, 32, 33, 64, 65536 // N, 65536 // N + 1, 65535 // N + 1):
            for pas in (DIRECT, MERGED):
                for f in (8, 37, 64):
                    assert plan(pas, f, B, N, 3, 4)['grid_x'] == L.gwtf_dw1_partials(B, N), (pas, f, B, N)
