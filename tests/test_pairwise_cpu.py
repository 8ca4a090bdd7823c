"""Host-side pieces of the all-pairs generation metrics: the mirrors of lib/networks/utils.py:120-144 on hand-made matrices with
known answers, and the two new C ABI entries in the header and the binding table (test_contract.py then checks the export)."""
import os
import re

import torch

from conftest import ROOT
from go_with_the_flows_amd import _lib
from go_with_the_flows_amd import evaluation as ev


def test_cov_counts_distinct_nearest_clouds_along_either_axis():
    # rows = 3 samples, columns = 4 references
    d = torch.tensor([[0.1, 0.9, 0.8, 0.7],
                      [0.2, 0.9, 0.8, 0.7],
                      [0.9, 0.8, 0.7, 0.1]])
    # axis=1: every row's nearest column -> {0, 0, 3}: 2 of the 4 columns are covered
    assert ev.COV(d, axis=1) == 2.0 / 4.0
    # axis=0: every column's nearest row -> {0, 2, 2, 2}: 2 of the 3 rows are covered
    assert ev.COV(d, axis=0) == 2.0 / 3.0
    assert ev.COV(d) == ev.COV(d, axis=1)
    assert ev.COV(torch.eye(5).neg(), axis=1) == 1.0 and ev.COV(torch.eye(5).neg(), axis=0) == 1.0


def test_mmd_averages_the_minimum_over_the_other_axis():
    d = torch.tensor([[0.1, 0.9, 0.8, 0.7],
                      [0.2, 0.9, 0.8, 0.7],
                      [0.9, 0.8, 0.7, 0.1]])
    # axis=1: for every column its smallest entry (over rows): 0.1, 0.8, 0.7, 0.1
    assert abs(ev.MMD(d, axis=1) - (0.1 + 0.8 + 0.7 + 0.1) / 4) < 1e-7
    # axis=0: for every row its smallest entry: 0.1, 0.2, 0.1
    assert abs(ev.MMD(d, axis=0) - (0.1 + 0.2 + 0.1) / 3) < 1e-7
    assert isinstance(ev.MMD(d), float) and ev.MMD(d) == ev.MMD(d, axis=1)


def _line_matrices(x, y):
    x, y = torch.tensor(x, dtype=torch.float32), torch.tensor(y, dtype=torch.float32)
    return (x[:, None] - x[None, :]).abs(), (x[:, None] - y[None, :]).abs(), (y[:, None] - y[None, :]).abs()


def test_knn_separated_and_interleaved_sets():
    # two far-apart clusters on a line: every point's nearest other point is of its own set
    acc = ev.KNN(*_line_matrices([0.0, 0.1, 0.25], [10.0, 10.1, 10.25]), 1)
    assert isinstance(acc, float) and acc == 1.0
    assert float(ev.knn(*_line_matrices([0.0, 0.1, 0.25], [10.0, 10.1, 10.25]), 1)['acc']) == 1.0
    # interleaved: every point's nearest other point is of the OTHER set
    assert ev.KNN(*_line_matrices([0.0, 2.0, 4.0], [0.9, 2.9, 4.9]), 1) == 0.0
    # sqrt is monotone: same neighbours
    assert ev.KNN(*_line_matrices([0.0, 2.0, 4.0], [0.9, 2.9, 4.9]), 1, sqrt=True) == 0.0


def test_knn_even_k_tie_goes_to_the_second_set_unlike_knn():
    """x = {0, 1}, y = {0.4, 1.4} on a line, k = 2.  Two nearest others: 0 -> (0.4 y, 1 x); 1 -> (0.4 y, 1.4 y); 0.4 -> (0 x, 1 x);
    1.4 -> (1 x, 0.4 y).  KNN's +-1 labels: votes 0, +2, -2, 0 -> a vote of 0 predicts the second set (+1): predictions y, y, x, y
    against x, x, y, y: 1 of 4 right.  knn's 1/0 labels with count >= k/2: counts 1, 0, 2, 1 -> predictions x, y, x, x: 1 of 4 right
    too, but on DIFFERENT points (x=0 right there, y=1.4 right here)."""
    mats = _line_matrices([0.0, 1.0], [0.4, 1.4])
    assert ev.KNN(*mats, 2) == 0.25
    s = ev.knn(*mats, 2)
    assert float(s['acc']) == 0.25 and float(s['tp']) == 1.0 and float(s['tn']) == 0.0     # knn: its one hit is of the first set
    # one more point in y moves only the tie: x = {0}, y = {1, 2}: the neighbours of 0 are (y, y), of 1 (x, y), of 2 (y, x)
    mats = _line_matrices([0.0], [1.0, 2.0])
    assert abs(ev.KNN(*mats, 2) - 2.0 / 3.0) < 1e-7        # votes +2, 0, 0 -> y, y, y: the two y's are right
    assert float(ev.knn(*mats, 2)['acc']) == 0.0           # counts 0, 1, 1 -> y, x, x: nobody is right


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    for name in ('gwtf_chamfer_directed', 'gwtf_emd_cost_pairs'):
        assert name in declared and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header
    # malformed arguments never reach a launch (host-side checks of the library, no GPU needed)
    L = _lib.lib()
    assert L.gwtf_chamfer_directed(None, None, None, None, None, 0, 1, 1, 1, 1, None) == 10001
    assert L.gwtf_emd_cost_pairs(None, None, None, None, 1, 1, 1, 1, 0, 1, None) == 10001
