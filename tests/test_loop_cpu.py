"""Host side of the resident training loop (training.ResidentTrainLoop): the hyper-parameter planner gwtf_adam_hyper, the schedule
table LRUpdater.table, the GwtfLoopState / GwtfLoopArgs records and the new exports.  Runs without a GPU."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from test_contract import _c_struct_fields, _mirror_fields
from go_with_the_flows_amd import _lib, optim

NEW_SYMBOLS = ('gwtf_adam_hyper', 'gwtf_adam_step_table_dev', 'gwtf_loop_begin', 'gwtf_loop_detect', 'gwtf_loop_commit')


def hyper(lr, b1, b2, t):
    out = (ctypes.c_float * 8)()
    assert _lib.lib().gwtf_adam_hyper(lr, b1, b2, t, out) == 0
    return np.asarray(list(out), np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


STEPS = list(range(1, 201)) + list(range(200, 20001, 617)) + [20000]


@pytest.mark.parametrize('b1', [0.9, 0.8, 0.95])
@pytest.mark.parametrize('b2', [0.999, 0.99, 0.9945])
def test_adam_hyper_is_the_python_expression_bit_for_bit(b1, b2):
    lr = 1e-3 + 1e-11                                        # off the float32 grid: the record holds its one rounding
    assert float(np.float32(lr)) != lr
    for t in STEPS:
        want = np.asarray([np.float32(lr), np.float32(b1), np.float32(b2), np.float32(1.0 - b1), np.float32(1.0 - b2),
                           np.float32(1.0 - b1 ** t), np.float32(math.sqrt(1.0 - b2 ** t)), 0.0], np.float32)
        assert np.array_equal(bits(hyper(lr, b1, b2, t)), bits(want)), (b1, b2, t)


def test_adam_hyper_refuses_bad_arguments():
    L = _lib.lib()
    out = (ctypes.c_float * 8)()
    assert L.gwtf_adam_hyper(1e-3, 0.9, 0.999, 0, out) == 10001
    assert L.gwtf_adam_hyper(1e-3, 0.9, 0.999, 1, None) == 10001


def test_schedule_table_rows_are_the_records_of_what_the_updater_sets():
    """Row i of LRUpdater.table == gwtf_adam_hyper of the lr / betas LRUpdater.__call__ writes at (epoch, first_iteration + i), with
    step count first_step + i -- across a cycle boundary (cycle_length = 2: epoch 1 ends the cycle, epoch 2 starts the next)."""
    up = optim.LRUpdater(7, cycle_length=2, min_lr=1.7e-5, max_lr=2.56e-4 + 1e-12, beta1=0.9, min_beta2=0.9945, max_beta2=0.999)
    opt = types.SimpleNamespace(param_groups=[{'lr': None, 'betas': None}, {'lr': None, 'betas': None}])
    step = 11
    seen = []
    for epoch, first in ((1, 3), (2, 0)):
        n = 7 - first
        table = up.table(epoch, first, n, step)
        assert table.shape == (n, 8) and table.dtype == np.float32
        for i in range(n):
            up(opt, epoch, first + i)
            g = opt.param_groups[1]
            assert g == opt.param_groups[0]
            want = hyper(g['lr'], g['betas'][0], g['betas'][1], step + i)
            assert np.array_equal(bits(table[i]), bits(want)), (epoch, i)
            seen.append(g['lr'])
        step += n
    assert seen[3] < seen[0] and abs(seen[4] - up.max_lr) < 1e-12           # the cycle restarts at its maximum
    assert up.table(0, 0, 0, 1).shape == (0, 8)
    with pytest.raises(ValueError):
        up.table(0, 0, 1, 0)


def test_loop_records_follow_the_header_field_for_field():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    for c_name, mirror, count in (('GwtfLoopArgs', _lib.LoopArgs, 13), ('GwtfLoopState', _lib.LoopState, 10)):
        declared = _c_struct_fields(header, c_name)
        assert len(declared) == count, c_name
        assert _mirror_fields(mirror) == declared, c_name
    # the offsets training.ResidentTrainLoop hands the optimiser launch, and the size meters() copies
    S = _lib.LoopState
    assert ctypes.sizeof(S) == 160 and S.meters.offset == 0 and S.hyper.offset == 96 and S.cursor.offset == 128
    assert S.skip.offset == 148 and S.flag.offset == 152


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(handle, name) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12


def test_loop_launches_validate_before_anything_is_launched():
    L = _lib.lib()
    E = 10001

    def record(**over):
        a = _lib.LoopArgs(state=0x1000, plan=0x1000, rows=0x1000, table=0x1000, B=4, views=1, plan_len=8, table_rows=2)
        a.terms[:] = [0x1000] * 4
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return ctypes.byref(a)

    for call in (L.gwtf_loop_begin, L.gwtf_loop_detect, L.gwtf_loop_commit):
        assert call(None) == E
        for bad in (dict(state=None), dict(B=0), dict(views=0), dict(plan_len=-1), dict(table_rows=-1)):
            assert call(record(**bad)) == E, bad
    assert L.gwtf_loop_begin(record(plan=None)) == E and L.gwtf_loop_begin(record(rows=None)) == E
    assert L.gwtf_loop_detect(record(terms=(0, None))) == E
    assert L.gwtf_loop_commit(record(table=None)) == E and L.gwtf_loop_commit(record(terms=(3, None))) == E
    assert L.gwtf_adam_step_table_dev(None, 0x1000, 0x1000, 1, 0x1000, 0x1000, 1e-8, 0.0, 0, None) == E
    assert L.gwtf_adam_step_table_dev(0x1000, 0x1000, 0x1000, 1, None, 0x1000, 1e-8, 0.0, 0, None) == E
    assert L.gwtf_adam_step_table_dev(0x1000, 0x1000, 0x1000, 1, 0x1000, None, 1e-8, 0.0, 0, None) == E
    assert L.gwtf_adam_step_table_dev(0x1000, 0x1000, 0x1000, 0, 0x1000, 0x1000, 1e-8, 0.0, 0, None) == 0      # nothing to do


def test_resident_loop_refuses_before_it_touches_a_device():
    """Every argument check of training.ResidentTrainLoop stands in front of the first device call."""
    import json
    import torch
    import go_with_the_flows_amd as gw
    from conftest import GOLDEN, golden
    from go_with_the_flows_amd import models
    from go_with_the_flows_amd.training import ResidentTrainLoop
    D = golden('g22_clouds')
    store = gw.MeshStore.from_arrays(D['vertices_c'], D['faces_vc'], D['vertices_c_bounds'], D['faces_bounds'], device='cpu')
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg']
    m = models.Flow_Mixture_Model(**cfg)
    crit = models.Flow_Mixture_Loss(**cfg)
    loader = gw.DeviceCloudLoader(store, 2, 48)
    opt = optim.Adam(m.parameters(), lr=1e-4)
    with pytest.raises(gw.GwtfError, match='HIP device'):                   # parameters on the host
        ResidentTrainLoop(m, crit, opt, loader)
    with pytest.raises(gw.GwtfError, match='float32'):
        ResidentTrainLoop(m.double(), crit, optim.Adam(m.parameters(), lr=1e-4), loader)
    m = m.float()
    with pytest.raises(ValueError, match='eval_cloud'):
        ResidentTrainLoop(m, crit, opt, gw.DeviceCloudLoader(store, 2, 48, return_eval_cloud=False))
    with pytest.raises(ValueError, match='no full batch'):
        ResidentTrainLoop(m, crit, opt, gw.DeviceCloudLoader(store, 4, 48))
    ps = list(m.parameters())
    two = optim.Adam([{'params': ps[:3]}, {'params': ps[3:], 'lr': 3e-4}], lr=1e-4)
    with pytest.raises(ValueError, match='one schedule table'):
        ResidentTrainLoop(m, crit, two, loader)
    svr_cfg = json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']
    svr = models.Flow_Mixture_SVR_Model(**svr_cfg)
    with pytest.raises(ValueError, match='do not go together'):
        ResidentTrainLoop(svr, crit, optim.Adam(svr.parameters(), lr=1e-4), loader)
    images = gw.ImageStore.from_arrays(np.zeros((6, 3, 8, 8), np.uint8), views_per_shape=2, device='cpu')
    with pytest.raises(gw.GwtfError, match='host-resident ImageStore'):
        ResidentTrainLoop(svr, crit, optim.Adam(svr.parameters(), lr=1e-4), gw.DeviceSVRLoader(store, images, 2, 48))
