"""All-pairs generation metrics on the device (gwtf_chamfer_directed / gwtf_emd_cost_pairs through metrics.py and evaluation.py)
against oracle/metrics_oracle.py and against the per-row host loop they stand in for.  Needs an MI355X.

Bars: the per-point minimum is nn_distance's, bit for bit, so the COUNTS are exact; the per-pair SUM is a float32 reduction of
those minima in another order than the oracle's: rtol 1e-5 against their float64 sum (the bar test_gpu_metrics.py holds CDL / CDR
to); F1 matrices rtol 1e-6 (integer counts, then the same float32 expression up to one ulp in the mean); the fused EMD cost rtol
1e-4 (the project's bar for it: its tile partials meet in a float atomic).
"""
import numpy as np
import pytest
import torch

from go_with_the_flows_amd import _lib, metrics
from go_with_the_flows_amd import evaluation as ev
from oracle import metrics_oracle as mo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GROUP, CHUNK, TILE = 8, 2048, 1024      # kCdGroup, kCdChunk, kTile of csrc/gwtf_metrics.hip


def cloud_sets(seed, na, nb, n, m):
    r = np.random.default_rng(seed)
    return (r.standard_normal((na, n, 3)) * 0.25).astype(np.float32), (r.standard_normal((nb, m, 3)) * 0.25).astype(np.float32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def all_pairs(a, b):
    """Row-major expansion of the pair grid: pair (i, j) -> index i * nb + j."""
    return np.repeat(a, len(b), 0), np.tile(b, (len(a), 1, 1))


def oracle_minima(q, t):
    """(nq, nt, n) float32: for every ordered pair the oracle's dist1."""
    qe, te = all_pairs(q, t)
    return mo.nn_distance(qe, te)[0].reshape(len(q), len(t), q.shape[1])


@pytest.mark.parametrize('nq,nt,n,m', [(1, 1, 1, 1), (5, 7, 96, 96), (3, 4, 100, 37), (2, 3, CHUNK + 1, TILE + 1),
                                       (2, GROUP + 1, 33, 20)])
def test_directed_sums_and_counts_against_the_oracle(nq, nt, n, m):
    q, t = cloud_sets(100 * nq + n, nq, nt, n, m)
    mins = oracle_minima(q, t)
    thr = np.array([0.0, np.inf, np.quantile(mins, 0.25), np.quantile(mins, 0.75), mins.reshape(-1)[mins.size // 2]], np.float32)
    assert (mins == thr[4]).any()                      # one threshold EQUAL to a minimum: the compare is a strict '<'
    s, c = metrics.chamfer_directed(dev(q), dev(t), thr)
    assert s.shape == (nq, nt) and s.dtype == torch.float32 and c.shape == (5, nq, nt) and c.dtype == torch.int32
    want = np.stack([(mins < h).sum(2) for h in thr])
    assert (want[0] == 0).all() and (want[1] == n).all()
    err = np.abs(host(s) - mins.astype(np.float64).sum(2)) / mins.astype(np.float64).sum(2)
    print('directed', (nq, nt, n, m), 'max rel err of sum %.2e' % err.max(), 'count mismatches', int((host(c) != want).sum()))
    assert np.array_equal(host(c), want)
    np.testing.assert_allclose(host(s), mins.astype(np.float64).sum(2), rtol=1e-5)
    # no thresholds: the sums alone, the same bits
    s0, c0 = metrics.chamfer_directed(dev(q), dev(t))
    assert torch.equal(s0, s) and c0.shape == (0, nq, nt)


def test_directed_more_than_eight_thresholds_loops_on_the_host():
    q, t = cloud_sets(5, 3, 4, 50, 60)
    mins = oracle_minima(q, t)
    thr = np.quantile(mins, np.linspace(0.05, 0.95, 11)).astype(np.float32)
    s, c = metrics.chamfer_directed(dev(q), dev(t), thr)
    assert np.array_equal(host(c), np.stack([(mins < h).sum(2) for h in thr]))
    np.testing.assert_allclose(host(s), mins.astype(np.float64).sum(2), rtol=1e-5)


def test_directed_is_deterministic_and_a_cloud_is_at_distance_zero_of_itself():
    q, t = cloud_sets(7, 5, GROUP + 3, CHUNK + 77, 300)
    qd, td = dev(q), dev(t)
    thr = (0.002, 0.01)
    s1, c1 = metrics.chamfer_directed(qd, td, thr)
    s2, c2 = metrics.chamfer_directed(qd, td, thr)
    assert torch.equal(s1, s2) and torch.equal(c1, c2)
    s, c = metrics.chamfer_directed(qd, qd, thr)
    assert float(s.diagonal().abs().max()) == 0.0
    assert bool((c.diagonal(dim1=1, dim2=2) == q.shape[1]).all())
    assert float(s.min()) >= 0.0 and float((s + torch.eye(5, device=DEV)).min()) > 0.0


# ---- the evaluation layer against the per-row host loop (the parent path) -------------------------------------------------------
S, R, N, THRESHOLDS = 6, 7, 96, (0.005, 0.01)
SEED = 41           # issue-stated inputs of the matrix comparison
SEED_VOTES = 2277     # inputs of the generation_metrics comparison: a seed whose parent-path matrices meet the gap precondition


def parent_matrices(s, r):
    """{'cd','emd','left','right'} and {'f1': {thr: M}} from _pairwise_EMD_CD_F1_SCORE (accelerated_cd=True, batch_size=3)."""
    out = {'f1': {}}
    for k, thr in enumerate(THRESHOLDS):
        cd, emd, f1, left, right = ev._pairwise_EMD_CD_F1_SCORE(s, r, 3, thr, accelerated_cd=True, cd_option=k == 0,
                                                                one_part_of_cd=k == 0, emd_option=k == 0, f1_option=True)
        out['f1'][thr] = f1
        if k == 0:
            out.update(cd=cd, emd=emd, left=left, right=right)
    return out


@pytest.fixture(scope='module')
def seed41():
    s_np, r_np = cloud_sets(SEED, S, R, N, N)
    s, r = dev(s_np), dev(r_np)
    return s, r, parent_matrices(s, r)


def test_pairwise_matrices_against_the_parent_path(seed41):
    s, r, want = seed41
    got = ev.pairwise_matrices(s, r, THRESHOLDS, cd_option=True, one_part_of_cd=True, emd_option=True)
    assert set(got) == {'cd', 'left', 'right', 'emd', 'f1'} and set(got['f1']) == set(THRESHOLDS)
    for k in ('cd', 'left', 'right'):
        assert got[k].shape == (S, R)
        print(k, 'max rel err %.2e' % float(((got[k] - want[k]).abs() / want[k].abs()).max()))
        np.testing.assert_allclose(host(got[k]), host(want[k]), rtol=1e-5)
    for thr in THRESHOLDS:
        np.testing.assert_allclose(host(got['f1'][thr]), host(want['f1'][thr]), rtol=1e-6)
    print('emd max rel err %.2e' % float(((got['emd'] - want['emd']).abs() / want['emd'].abs()).max()))
    np.testing.assert_allclose(host(got['emd']), host(want['emd']), rtol=1e-4)
    # options that are off come back as [] / {}
    off = ev.pairwise_matrices(s, r, cd_option=True)
    assert off['left'] == [] and off['right'] == [] and off['emd'] == [] and off['f1'] == {} and torch.equal(off['cd'], got['cd'])


def test_pairwise_matrices_of_a_set_against_itself_are_symmetric_bitwise(seed41):
    s, _, _ = seed41
    got = ev.pairwise_matrices(s, s, THRESHOLDS, cd_option=True, one_part_of_cd=True)
    assert torch.equal(got['right'], got['left'].t()) and torch.equal(got['cd'], got['cd'].t())
    # ... and they are what two directed passes over a COPY give (left == right.T is a fact of the arithmetic, not of the shortcut)
    two = ev.pairwise_matrices(s, s.clone(), THRESHOLDS, cd_option=True, one_part_of_cd=True)
    for k in ('cd', 'left', 'right'):
        assert torch.equal(got[k], two[k]), k
    for thr in THRESHOLDS:
        assert torch.equal(got['f1'][thr], two['f1'][thr])


def test_pairwise_cd_is_left_plus_right(seed41):
    s, r, want = seed41
    cd = ev.pairwise_CD(s, r)
    assert cd.shape == (S, R)
    np.testing.assert_allclose(host(cd), host(want['left'] + want['right']), rtol=1e-5)
    assert torch.equal(ev.pairwise_CD(s, r, bs=2), cd)             # bs is accepted and ignored


def rel_gap(M, dim):
    """Smallest relative distance between the best (smallest) and second-best entry along ``dim``."""
    v = M.double().sort(dim=dim)[0].movedim(dim, 0)
    return float(((v[1] - v[0]) / v[1].abs()).min())


def test_generation_metrics_against_compute_all_metrics():
    s_np, r_np = cloud_sets(SEED_VOTES, S, R, N, N)
    s, r = dev(s_np), dev(r_np)
    tol = {'CD': 1e-5, 'EMD': 1e-4, 'F1': 1e-6}
    # precondition of the exact comparisons, on the PARENT path's matrices: along every row and column of every matrix a vote
    # reads (sample x ref for MMD / COV, the joint matrix of knn), best and second best are more than 100 tolerances apart
    rs, rr, ss = parent_matrices(s, r), parent_matrices(r, r), parent_matrices(s, s)
    for name, key in (('CD', 'cd'), ('EMD', 'emd')):
        joint = torch.cat((torch.cat((ss[key], rs[key]), 1), torch.cat((rs[key].t(), rr[key]), 1)), 0)
        joint = joint + torch.diag(torch.full((S + R,), float('inf'), device=DEV))
        gaps = [rel_gap(rs[key], 0), rel_gap(rs[key], 1), rel_gap(joint, 0), rel_gap(joint, 1)]
        print(name, 'parent-path gaps (rs cols, rs rows, joint cols, joint rows):', ['%.2e' % g for g in gaps])
        assert min(gaps) > 100 * tol[name], (name, gaps)
    got = ev.generation_metrics(s, r, THRESHOLDS, cd_option=True, emd_option=True, f1_option=True)
    assert set(got) == set(THRESHOLDS)
    for thr in THRESHOLDS:
        want = ev.compute_all_metrics(s, r, 3, accelerated_cd=True, f1_threshold=thr, cd_option=True, emd_option=True,
                                      f1_option=True)
        assert set(got[thr]) == set(want)
        for key, w in want.items():
            g = got[thr][key]
            name = next(nm for nm in ('CD', 'EMD', 'F1') if key.endswith('-' + nm) or ('-%s-' % nm) in key)
            if key.startswith(('lgan_mmd', 'mmd_contrib')):
                np.testing.assert_allclose(host(g), host(w), rtol=tol[name], err_msg=key)
            elif name != 'F1':       # lgan_cov-*, idx_mmd-*, 1-NN-*-acc*: indices and votes, exactly (F1: ties, not compared)
                assert key.startswith(('lgan_cov', 'idx_mmd', '1-NN')), key
                assert torch.equal(g, w), key


def test_generation_metrics_needs_no_thresholds_for_cd_alone_and_reports_nothing_without_them():
    s_np, r_np = cloud_sets(3, 4, 5, 40, 40)
    s, r = dev(s_np), dev(r_np)
    got = ev.generation_metrics(s, r, cd_option=True)
    want = ev.compute_all_metrics(s, r, 60, accelerated_cd=True, cd_option=True)
    assert list(got) == [0.001] and set(got[0.001]) == set(want)
    assert ev.generation_metrics(s, r, (), cd_option=True) == {}


@pytest.mark.parametrize('na,nb,n,m', [(2, 3, 200, 200), (1, 2, 96, 32), (2, 2, 1030, 1030)])
def test_emd_cost_pairs_against_the_oracle(na, nb, n, m):
    a, b = cloud_sets(11 + n, na, nb, n, m)
    ae, be = all_pairs(a, b)
    want = mo.match_cost(ae, be, mo.approx_match(ae, be)).reshape(na, nb)
    got = metrics.emd_cost_pairs(dev(a), dev(b))
    assert got.shape == (na, nb) and got.dtype == torch.float32
    print('emd pairs', (na, nb, n, m), 'max rel err %.2e' % (np.abs(host(got) - want) / want).max())
    np.testing.assert_allclose(host(got), want, rtol=1e-4)
    one_row = metrics.emd_cost_pairs(dev(a), dev(b), max_temp_bytes=1)      # one row of the result per block
    np.testing.assert_allclose(host(one_row), want, rtol=1e-4)


def test_input_checks():
    a, b = cloud_sets(0, 2, 3, 8, 8)
    for fn in (metrics.chamfer_directed, metrics.emd_cost_pairs, ev.pairwise_CD,
               lambda x, y: ev.pairwise_matrices(x, y, (0.01,), cd_option=True)):
        with pytest.raises(_lib.GwtfError):
            fn(torch.from_numpy(a), torch.from_numpy(b))                  # host tensors
        with pytest.raises(_lib.GwtfError):
            fn(dev(a)[:, ::2], dev(b))                                    # not contiguous
        with pytest.raises(_lib.GwtfError):
            fn(dev(a), dev(b).transpose(1, 2))                            # last dimension is not 3
    with pytest.raises(_lib.GwtfError):
        ev.pairwise_matrices(dev(a), dev(b)[:, :5].contiguous(), emd_option=True)      # EMD needs n == m
    # the library itself rejects what the wrappers never send
    L = _lib.lib()
    x = dev(a)
    assert L.gwtf_chamfer_directed(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 9, 2, 2, 8, 8, None) == 10001
    assert L.gwtf_chamfer_directed(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, 1, 2, 2, 8, 8, None) == 10001
    assert L.gwtf_emd_cost_pairs(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 2, 2, 8, 8, 1, 2, None) == 10001
