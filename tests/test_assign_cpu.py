"""CPU-side checks of the per-point assignment boundary: header, export and record mirror, the unchanged ABI number, the float64
restatement (assign_ref.py) pinned to the genuine reference's values, part_agreement on hand-made tables, records refused without a
device, loud failure of the entry points on host tensors."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, TOL_NLL_REL, golden
import assign_ref as ar
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models
from go_with_the_flows_amd import evaluation as ev
from oracle import flow_oracle as fo


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def _record_fields(header, name):
    """[(field, kind)] of `typedef struct <name> { ... } <name>;` in declaration order, kind 'pointer' or the C scalar type: the parser
    idea of test_contract.py applied to the one new record (every `*` declarator is a pointer, `int K, B, N` declares three)."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ctype, names = re.fullmatch(r'((?:const\s+)?(?:long\s+long|\w+)(?:\s*\*)?)\s*(\w+(?:\s*,\s*\w+)*)', decl).groups()
        kind = 'pointer' if '*' in ctype else ctype
        assert kind in ('pointer', 'int'), decl
        fields += [(n.strip(), kind) for n in names.split(',')]
    return fields


def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = _header()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert 'gwtf_mixture_assign' in declared and 'typedef struct GwtfAssignArgs {' in header
    assert 'gwtf_mixture_assign' in _lib.EXPORTS and declared == set(_lib.EXPORTS)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'gwtf_mixture_assign')
    assert 'gwtf_assign.hip' in open(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'Makefile')).read()


def test_record_follows_the_header_field_for_field():
    declared = _record_fields(_header(), 'GwtfAssignArgs')
    assert len(declared) == 19
    kinds = {ctypes.c_void_p: 'pointer', ctypes.c_int: 'int'}
    assert [(n, kinds[t]) for n, t in _lib.AssignArgs._fields_] == declared
    assert [n for n, k in declared if k == 'int'] == ['K', 'B', 'N', 'P'] and declared[-1] == ('stream', 'pointer')


def test_abi_version_is_still_12():
    assert re.search(r'#define GWTF_ABI_VERSION (\d+)', _header()).group(1) == '12'
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12


def test_restatement_is_the_reference_density_on_the_golden_inputs():
    d = golden('g5_losses')
    arrs64 = [d[k].astype(np.float64) for k in ('z', 'logdet', 'mu0', 'lv0', 'logits')]
    lp = ar.lp(*arrs64)
    K, B, _, N = d['z'].shape
    assert lp.shape == (K, B, N)
    dens = ar.log_density(lp)
    mean, per_shape = fo.mixture_nll_fused(*arrs64)
    assert np.abs(-dens.sum(1) - per_shape).max() <= 1e-12 * np.abs(per_shape).max()
    assert abs(-dens.sum(1).mean() - float(d['mixture_nll'])) <= TOL_NLL_REL * abs(float(d['mixture_nll']))
    # what follows from lp: responsibilities sum to one, the label carries the largest, the counts are those of the labels
    r, lab = ar.resp(lp), ar.labels(lp)
    assert np.abs(r.sum(1) - 1).max() < 1e-12 and lab.min() >= 0 and lab.max() < K
    assert np.array_equal(lab, r.argmax(1)) and np.allclose(ar.confidence(lp), r.max(1), rtol=0, atol=1e-15)
    c, inv = ar.counts(lab, K)
    assert c.sum() == B * N and not inv.any()
    assert ar.margin(lp).min() > 7e-3                             # no point of this input sits near a tie


def test_restatement_edge_rules():
    rng = np.random.default_rng(3)
    K, B, N = 3, 2, 5
    z, ld = rng.normal(size=(K, B, 3, N)), rng.normal(size=(K, B, 3, N))
    mu0, lv0, logits = rng.normal(size=(K, B, 3)), rng.normal(size=(K, B, 3)), rng.normal(size=(B, K))
    logits[0, 1] = -200.0                                         # float32 exp underflows: the log weight is -inf
    logits[1] = -200.0
    z[2, 0, 1, 3] = np.nan
    lp = ar.lp(z, ld, mu0, lv0, logits)
    assert np.isneginf(lp[1, 0]).all() and np.isneginf(lp[:, 1]).all()
    dens, lab = ar.log_density(lp), ar.labels(lp)
    assert np.isnan(dens[0, 3]) and np.isfinite(np.delete(dens[0], 3)).all() and np.isneginf(dens[1]).all()
    assert lab[0, 3] == -1 and (np.delete(lab[0], 3) != 1).all() and (np.delete(lab[0], 3) >= 0).all() and (lab[1] == -1).all()
    r = ar.resp(lp)
    assert np.isnan(r[0, :, 3]).all() and np.isnan(r[1]).all() and (np.delete(r[0, 1], 3) == 0).all()
    assert ar.confidence(lp)[0, 3] == 0 and (ar.confidence(lp)[1] == 0).all()
    c, inv = ar.counts(lab, K)
    assert inv.tolist() == [1, N] and c[0].sum() == N - 1 and c[1].sum() == 0
    # an exact tie goes to the lower component
    same = ar.lp(np.repeat(z[:1], 2, 0), np.repeat(ld[:1], 2, 0), np.repeat(mu0[:1], 2, 0), np.repeat(lv0[:1], 2, 0), np.zeros((B, 2)))
    assert (ar.labels(same)[:, :3] == 0).all() and (ar.margin(same)[:, :3] == 0).all()
    table, skipped = ar.contingency(np.array([[0, 1, -1, 1]]), np.array([[2, 0, 1, 5]]), 2, 3)
    assert table.tolist() == [[0, 0, 1], [1, 0, 0]] and skipped == 2


@pytest.mark.parametrize('fn', [ev.part_agreement, ar.part_agreement], ids=['evaluation', 'restatement'])
def test_part_agreement_on_hand_made_tables(fn):
    res = fn(np.diag([3, 4, 5]))
    assert res['purity'] == 1.0 and res['miou'] == 1.0 and abs(res['nmi'] - 1.0) < 1e-15 and list(res['mapping']) == [0, 1, 2]
    res = fn(np.array([[3, 4, 5]]))                               # one component: no information about the parts
    assert res['nmi'] == 0.0 and list(res['mapping']) == [2] and res['purity'] == 5 / 12
    assert abs(res['miou'] - (0 + 0 + 5 / 12) / 3) < 1e-15
    res = fn(np.array([[2, 2, 1], [0, 1, 1]]))                    # ties in both rows: the lowest part
    assert list(res['mapping']) == [0, 1] and res['purity'] == 3 / 7
    # part 0: TP 2, GT 2, predicted 5; part 1: TP 1, GT 3, predicted 2; part 2: TP 0, GT 2
    assert abs(res['miou'] - (2 / 5 + 1 / 4 + 0) / 3) < 1e-15
    pk, pp, joint = np.array([5, 2]) / 7, np.array([2, 3, 2]) / 7, np.array([[2, 2, 1], [0, 1, 1]]) / 7
    info = sum(joint[k, p] * math.log(joint[k, p] / (pk[k] * pp[p])) for k in range(2) for p in range(3) if joint[k, p] > 0)
    h = lambda q: -sum(v * math.log(v) for v in q)
    assert abs(res['nmi'] - info / math.sqrt(h(pk) * h(pp))) < 1e-15
    res = fn(np.array([[4, 0], [0, 0], [1, 3]]))                  # an empty component maps to part 0 and predicts nothing
    assert list(res['mapping']) == [0, 0, 1] and res['purity'] == 7 / 8 and abs(res['miou'] - (4 / 5 + 3 / 4) / 2) < 1e-15
    res = fn(np.zeros((2, 3), np.int64))
    assert all(math.isnan(res[k]) for k in ('purity', 'nmi', 'miou'))


def test_part_agreement_takes_a_tensor():
    t = torch.tensor([[7, 1], [2, 6]])
    a, b = ev.part_agreement(t), ar.part_agreement(t.numpy())
    assert all(abs(a[k] - b[k]) < 1e-15 for k in ('purity', 'nmi', 'miou')) and list(a['mapping']) == b['mapping']
    assert gw.part_agreement is ev.part_agreement and gw.segment_clouds is ev.segment_clouds


def test_bad_records_are_refused_before_anything_is_launched():
    L, E, p = _lib.lib(), 10001, 0x1000

    def record(**over):
        a = _lib.AssignArgs(z=p, logdet=p, mu0=p, lv0=p, logits=p, parts=p, log_density=p, labels=p, confidence=p, resp=p, counts=p,
                            invalid=p, table=p, skipped=p, K=4, B=2, N=33, P=5)
        for k, v in over.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert L.gwtf_mixture_assign(None) == E
    for bad in (dict(z=None), dict(logdet=None), dict(mu0=None), dict(lv0=None), dict(logits=None), dict(log_density=None),
                dict(labels=None), dict(K=0), dict(K=65), dict(K=-1), dict(B=0), dict(B=-3), dict(N=0), dict(N=-1), dict(P=0), dict(P=65),
                dict(table=None), dict(table=None, skipped=None)):
        assert L.gwtf_mixture_assign(record(**bad)) == E, bad


def test_entry_points_refuse_host_tensors_and_train_mode():
    K, B, N = 2, 2, 8
    z = torch.zeros(K, B, 3, N)
    with pytest.raises(gw.GwtfError):
        _lib.mixture_assign(z, z, torch.zeros(K, B, 3), torch.zeros(K, B, 3), torch.zeros(B, K))
    with pytest.raises(gw.GwtfError):
        _lib.mixture_assign(z[0], z, torch.zeros(K, B, 3), torch.zeros(K, B, 3), torch.zeros(B, K))          # and the wrong layout
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating')
    m = models.Flow_Mixture_Model(**cfg).eval()
    with pytest.raises(gw.GwtfError):
        m.assign_many(torch.zeros(B, 3, N))
    m.train()
    with pytest.raises(NotImplementedError):
        m.assign_many(torch.zeros(B, 3, N))
    batch = {'cloud': torch.zeros(B, 3, N), 'eval_cloud': torch.zeros(B, 3, N)}
    with pytest.raises(gw.GwtfError):
        ev.segment_clouds(m.eval(), [batch])
    with pytest.raises(gw.GwtfError):
        ev.segment_clouds(m, [])
    assert hasattr(models.Flow_Mixture_SVR_Model, 'assign_many')
