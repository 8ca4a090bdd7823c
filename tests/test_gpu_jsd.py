"""Occupancy histogram and Jensen-Shannon divergence on the GPU (csrc/gwtf_occupancy.hip) against the project's own host path
(evaluation.get_voxel_occ_dist / JSD on numpy copies, which test_evaluation_cpu.py pins to the reference through golden g14);
replace_nan_clouds and evaluate_generation.  Needs an MI355X."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import metrics, models
from go_with_the_flows_amd import evaluation as ev
from go_with_the_flows_amd.synth import load_synth_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_JSD = 1e-12            # absolute; the summation-order effect on 28^3 bins is 4e-15
PPW = metrics.OCC_POINTS_PER_WORKGROUP


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def inside(c, res):
    """Points of c with a bin on every axis, by the rule's two outer edges."""
    e = metrics.occupancy_edges(res)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    return int(np.all((c >= e[0]) & (c < e[-1]), axis=1).sum())


def check_against_host(c, res=28, clouds=None):
    """Device counts of `c` (numpy float32 (..., 3)) equal the host path's histogram exactly: the same normalised array, and the total
    the rule's outer edges give (a kernel that counted every point twice would pass the first alone)."""
    counts = host(metrics.voxel_occupancy(dev(c) if clouds is None else clouds, res=res))
    assert counts.shape == (res, res, res) and counts.dtype == np.int64
    assert counts.min() >= 0 and counts.sum() == inside(c, res)
    if counts.sum() > 0:
        want = ev.get_voxel_occ_dist(np.asarray(c), res=res, warning=False)
        assert np.array_equal(counts.astype(np.float64) / counts.sum(), np.asarray(want).reshape(counts.shape))
    return counts


def uniform(m, seed, lo=-0.6, hi=0.6):
    return np.random.RandomState(seed).uniform(lo, hi, (m, 3)).astype(np.float32)


# ---- golden ------------------------------------------------------------------------------------------------------------------------
def test_golden_occupancy_and_jsd():
    D = golden('g14_evaluation')
    for c, occ in ((D['c1'], D['occ1']), (D['c2'], D['occ2'])):
        counts = host(metrics.voxel_occupancy(dev(c)))
        assert np.array_equal(np.float64(counts) / counts.sum(), occ)
        got = ev.get_voxel_occ_dist(dev(c), warning=False)
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(host(got), occ)
    jsd = ev.JSD(dev(D['c1']), dev(D['c2']), warning=False)
    assert jsd.is_cuda and jsd.dtype == torch.float64 and jsd.dim() == 0
    err = abs(float(jsd) - float(D['jsd']))
    print('device JSD against g14: |diff| =', err)
    assert err < TOL_JSD
    assert abs(float(jsd) - float(ev.JSD(D['c1'], D['c2'], warning=False))) < TOL_JSD


# ---- the float32 neighbours of every edge -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [28, 8, 32])
def test_edge_neighbours_fall_where_the_table_says(res):
    vals = []
    for e in metrics.occupancy_edges(res):
        f = np.float32(e)
        vals += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    vals = np.asarray(vals, np.float32)
    pts = np.full((3, len(vals), 3), 0.1, np.float32)
    for axis in range(3):
        pts[axis, :, axis] = vals
    check_against_host(pts, res)
    for axis in range(3):                                             # and axis by axis: no axis hides behind another
        check_against_host(pts[axis], res)


# ---- values without a bin, and the two statistics ---------------------------------------------------------------------------------
def test_dropped_points_and_stats():
    nan, inf, tiny = np.nan, np.inf, 1e-45
    c = np.array([[nan, .1, .1], [.1, inf, .1], [.1, .1, -inf], [-0.0, 0.0, .1], [0.5, .1, .1], [-0.5, .1, .1], [.1, -0.5, 0.5],
                  [0.7, .1, .1], [tiny, -tiny, .1], [-tiny, tiny, -tiny], [.1, .1, 0.7], [.1, -0.7, .1], [nan, nan, 0.7],
                  [0.49999997, -0.49999997, .2], [inf, nan, -inf], [.2, .2, .2]], np.float32)
    assert np.float32(tiny) != 0 and abs(np.float32(tiny)) < np.finfo(np.float32).tiny           # a subnormal
    for res in (28, 8):
        check_against_host(c, res)
    for bound in (0.5, 0.25):
        stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        metrics.voxel_occupancy(dev(c), bound=bound, stats=stats)
        with np.errstate(invalid='ignore'):
            assert stats.tolist() == [int((np.fabs(c) > bound).sum()), int(np.isnan(c).sum())]
        metrics.voxel_occupancy(dev(c), bound=bound, stats=stats)                                 # added to, not overwritten
        with np.errstate(invalid='ignore'):
            assert stats.tolist() == [2 * int((np.fabs(c) > bound).sum()), 2 * int(np.isnan(c).sum())]


def test_warnings_come_from_the_stats(capsys):
    c = uniform(50, 3)
    c[7, 1] = np.nan
    ev.get_voxel_occ_dist(dev(c), clouds_flag='gen', warning=True)
    out = capsys.readouterr().out
    assert 'gen clouds out of cube bounds: [-0.5; 0.5]' in out and '1 NaN values in point cloud tensors.' in out
    ev.JSD(dev(c), dev(uniform(50, 4, -0.4, 0.4)), warning=True)
    out = capsys.readouterr().out
    assert 'gen clouds out of cube bounds' in out and 'ref clouds out of cube bounds' not in out and '1 NaN values' in out
    ev.JSD(dev(c), dev(c), warning=False)
    assert capsys.readouterr().out == ''


# ---- sizes at which the loop can go wrong --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 63, 64, 65, 4095, 4096, 4097, PPW - 1, PPW + 1, 20000])
def test_point_counts_around_the_tile_and_the_workgroup_share(m):
    check_against_host(uniform(m, m))


def test_three_clouds_of_67_points():
    check_against_host(uniform(201, 5).reshape(3, 67, 3))


def test_identical_points_in_one_bin():
    c = np.tile(np.array([[0.21, -0.33, 0.05]], np.float32), (5000, 1))
    counts = check_against_host(c)
    assert counts.max() == 5000 and (counts > 0).sum() == 1


def test_res_1_and_other_grids():
    c = uniform(3000, 9)
    assert check_against_host(c, 1).reshape(-1).tolist() == [inside(c, 1)]
    for res in (2, 7, 32):
        check_against_host(c, res)


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_a_tensor_that_starts_off_a_16_byte_boundary(shift):
    m = 9000                                                          # three tiles: points straddle the 16-byte pieces of each
    c = uniform(m, 20 + shift)
    flat = torch.zeros(3 * m + 8, device=DEV)
    off = (shift - flat.data_ptr() // 4) % 4 + 4                      # floats to skip so that the view starts `shift` floats off
    view = flat[off:off + 3 * m].view(m, 3)
    assert view.is_contiguous() and (view.data_ptr() % 16) // 4 == shift
    view.copy_(dev(c))
    flat[:off] = float('nan')                                         # what lies around the view must not be counted
    flat[off + 3 * m:] = float('nan')
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    counts = metrics.voxel_occupancy(view, stats=stats)
    assert np.array_equal(host(counts), check_against_host(c))
    assert stats.tolist() == [int((np.fabs(c) > 0.5).sum()), 0]


# ---- accumulation and determinism --------------------------------------------------------------------------------------------------
def test_accumulation_and_identical_bits():
    a, b = uniform(3000, 31), uniform(PPW + 700, 32)
    whole = metrics.voxel_occupancy(dev(np.concatenate([a, b])))
    out = metrics.voxel_occupancy(dev(a))
    assert metrics.voxel_occupancy(dev(b), out=out) is out
    assert torch.equal(out, whole)
    assert torch.equal(metrics.voxel_occupancy(dev(b)), metrics.voxel_occupancy(dev(b)))
    seven = torch.full((28, 28, 28), 7, dtype=torch.int64, device=DEV)
    metrics.voxel_occupancy(dev(a), out=seven)
    assert torch.equal(seven, metrics.voxel_occupancy(dev(a)) + 7)
    j = [ev.JSD(dev(a), dev(b), warning=False) for _ in range(2)]
    assert torch.equal(j[0], j[1])


def test_the_device_path_is_capturable():
    """JSD(warning=False) and replace_nan_clouds synchronise nothing and read nothing back: a stream capture of them succeeds (a
    host synchronisation inside it would fail the capture), and the replay gives the eager call's bits."""
    a, b = dev(uniform(3000, 33)), dev(uniform(5000, 34, -0.5, 0.4))
    clouds = dev(uniform(6 * 50, 35).reshape(6, 50, 3))
    clouds[2, 7, 0] = float('nan')
    want = ev.JSD(a, b, warning=False)                                # warm-up: the kernel's LDS limit is raised from here on
    ev.replace_nan_clouds(clouds)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ev.JSD(a, b, warning=False)
        fixed = ev.replace_nan_clouds(clouds)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert not torch.isnan(fixed).any() and torch.equal(fixed[:2], clouds[:2]) and torch.equal(fixed[3:], clouds[3:])


# ---- the divergence -----------------------------------------------------------------------------------------------------------------
def test_device_jsd_of_identical_disjoint_and_empty_histograms():
    a = dev(uniform(4000, 41, -0.5, 0.5))
    assert abs(float(ev.JSD(a, a.clone(), warning=False))) < TOL_JSD
    left, right = uniform(900, 42, -0.45, -0.05), uniform(1100, 43, 0.05, 0.45)
    assert abs(float(ev.JSD(dev(left), dev(right), warning=False)) - 1.0) < TOL_JSD
    c1 = torch.zeros(8, 8, 8, dtype=torch.int64, device=DEV)
    c2 = torch.zeros(8, 8, 8, dtype=torch.int64, device=DEV)
    c1[0, 0, 0], c2[7, 3, 1] = 5, 9
    assert abs(float(metrics.jsd_from_counts(c1, c2)) - 1.0) < TOL_JSD
    assert abs(float(metrics.jsd_from_counts(c1, c1))) < TOL_JSD
    empty = torch.zeros_like(c1)
    assert math.isnan(float(metrics.jsd_from_counts(empty, c2))) and math.isnan(float(metrics.jsd_from_counts(c1, empty)))
    outside = dev(uniform(100, 44, 0.6, 0.9))
    assert math.isnan(float(ev.JSD(outside, a, warning=False)))
    x, y = uniform(5000, 45), uniform(7000, 46, -0.5, 0.3)
    assert abs(float(ev.JSD(dev(x), dev(y), warning=False)) - float(ev.JSD(x, y, warning=False))) < TOL_JSD


# ---- guards --------------------------------------------------------------------------------------------------------------------------
def test_guards():
    good = dev(uniform(40, 51))
    vo = metrics.voxel_occupancy
    i64 = dict(dtype=torch.int64, device=DEV)
    for bad in (good.cpu(), good.double(), good.t().contiguous().t(), good[:, :2].contiguous(), torch.empty(0, 3, device=DEV),
                host(good)):
        with pytest.raises(gw.GwtfError):
            vo(bad)
    for res in (0, 33, -1, 2.5):
        with pytest.raises(gw.GwtfError):
            vo(good, res=res)
    for out in (torch.zeros(28, 28, 27, **i64), torch.zeros(28, 28, 28, dtype=torch.int32, device=DEV),
                torch.zeros(28, 28, 28, dtype=torch.int64), torch.zeros(8, 8, 8, **i64)):
        with pytest.raises(gw.GwtfError):
            vo(good, out=out)
    for stats in (torch.zeros(3, **i64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, device=DEV)):
        with pytest.raises(gw.GwtfError):
            vo(good, stats=stats)
    c = vo(good)
    for a, b in ((c, c.cpu()), (c, c.int()), (c, torch.zeros(8, 8, 8, **i64)), (c.float(), c.float())):
        with pytest.raises(gw.GwtfError):
            metrics.jsd_from_counts(a, b)
    with pytest.raises(gw.GwtfError):
        ev.JSD(good, host(good))
    for bad in (good, good.cpu().view(1, 40, 3), good.view(1, 40, 3).double()):
        with pytest.raises(gw.GwtfError):
            ev.replace_nan_clouds(bad)


# ---- replace_nan_clouds --------------------------------------------------------------------------------------------------------------
def test_replace_nan_clouds():
    S, n = 9, 16
    c = uniform(S * n, 61).reshape(S, n, 3)
    c[0, 3, 1] = np.nan
    c[5, 15, 2] = np.nan
    c[5, 0, 0] = np.nan
    clouds = dev(c)
    before = clouds.clone()
    out = ev.replace_nan_clouds(clouds, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(clouds.view(torch.int32), before.view(torch.int32))                       # the input is left alone
    assert out.shape == (S, n, 3) and out.is_contiguous() and out.data_ptr() != clouds.data_ptr()
    got = host(out)
    assert not np.isnan(got).any()
    keep = [i for i in range(S) if i not in (0, 5)]
    for i in keep:
        assert np.array_equal(got[i].view(np.uint32), c[i].view(np.uint32))
    for i in (0, 5):
        assert any(np.array_equal(got[i].view(np.uint32), c[k].view(np.uint32)) for k in keep), i
    again = ev.replace_nan_clouds(clouds, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(out, again)
    # over many draws every good cloud is drawn, and none but good ones
    many = np.tile(c[:1], (400, 1, 1))
    many[:7] = c[keep]
    drawn = host(ev.replace_nan_clouds(dev(many), generator=torch.Generator(device=DEV).manual_seed(6)))
    assert not np.isnan(drawn).any()
    firsts = {float(v) for v in drawn[7:, 0, 0]}
    assert firsts == {float(c[k, 0, 0]) for k in keep}
    fine = dev(c[keep])
    assert torch.equal(ev.replace_nan_clouds(fine), fine)
    all_bad = dev(c).clone()
    all_bad[:, 0, 0] = float('nan')
    same = ev.replace_nan_clouds(all_bad)
    assert torch.equal(same.view(torch.int32), all_bad.view(torch.int32))


# ---- evaluate_generation -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating')
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    return m.to(DEV).eval()


def same_value(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def test_evaluate_generation_is_the_hand_composition(model):
    thresholds = (0.001, 0.01)
    ref = dev(uniform(6 * 64, 71, -0.4, 0.4).reshape(6, 64, 3))

    def by_hand():
        torch.manual_seed(11)
        gen = ev.generate_clouds(model, 6, 64, batch_size=64, state=gw.make_state(3, DEV))
        gen = ev.replace_nan_clouds(gen)
        want = {'jsd': float(ev.JSD(gen, ref, warning=False) * 1e2)}
        per = ev.generation_metrics(gen, ref, thresholds, cd_option=True, emd_option=True, f1_option=True)
        for thr in thresholds:
            m = per[thr]
            want.update(cd_mmds=float(m['lgan_mmd-CD'] * 1e4), cd_covs=float(m['lgan_cov-CD'] * 1e2),
                        cd_1nns=float(m['1-NN-CD-acc'] * 1e2), emd_mmds=float(m['lgan_mmd-EMD'] * 1e2),
                        emd_covs=float(m['lgan_cov-EMD'] * 1e2), emd_1nns=float(m['1-NN-EMD-acc'] * 1e2))
            want['f1_%.4f_mmds' % thr] = float(m['lgan_mmd-F1'])
            want['f1_%.4f_covs' % thr] = float(m['lgan_cov-F1'] * 1e2)
            want['f1_%.4f_1nns' % thr] = float(m['1-NN-F1-acc'] * 1e2)
        return want

    want = by_hand()
    torch.manual_seed(11)
    got = ev.evaluate_generation(model, ref, f1_threshold_lst=thresholds, state=gw.make_state(3, DEV))
    keys = {'jsd', 'cd_mmds', 'cd_covs', 'cd_1nns', 'emd_mmds', 'emd_covs', 'emd_1nns'} | \
        {'f1_%s_%s' % (t, k) for t in ('0.0010', '0.0100') for k in ('mmds', 'covs', '1nns')}
    assert set(got) == keys == set(want)
    print('evaluate_generation:', got)
    for k in keys:
        assert isinstance(got[k], float) and same_value(got[k], want[k]), (k, got[k], want[k])
    torch.manual_seed(11)
    part = ev.evaluate_generation(model, ref, f1_threshold_lst=thresholds, jsd=False, emd=False, state=gw.make_state(3, DEV))
    assert set(part) == {k for k in keys if k != 'jsd' and not k.startswith('emd')}
    for k in part:
        assert same_value(part[k], want[k]), k
    with pytest.raises(gw.GwtfError):
        ev.evaluate_generation(model, ref.cpu())
