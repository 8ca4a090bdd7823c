"""Host side of the resident validation pass (training.ResidentEvalLoop): the gwtf_loop_eval_commit export and its argument checks,
the unchanged GwtfLoopState record, the loop's refusals, the best-model rule and the checkpoint dictionary.  Runs without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models, optim, training

E_BADARG = 10001


def test_the_abi_is_still_12_and_the_new_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    name = 'gwtf_loop_eval_commit'
    assert name in declared and hasattr(handle, name) and name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert declared == set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12
    assert int(re.search(r'#define\s+GWTF_ABI_VERSION\s+(\d+)', header).group(1)) == 12


def test_the_loop_state_record_is_unchanged():
    S = _lib.LoopState
    assert ctypes.sizeof(S) == 160
    offsets = {n: getattr(S, n).offset for n, _ in S._fields_}
    assert offsets == {'meters': 0, 'hyper': 96, 'cursor': 128, 'n_iters': 132, 'adam_step': 136, 'status': 140, 'poisoned_at': 144,
                       'skip': 148, 'flag': 152, 'reserved': 156}
    assert ctypes.sizeof(_lib.LoopArgs) == 5 * 8 + 4 * 8 + 6 * 4 + 8        # GwtfLoopArgs: 13 fields, as before


def test_eval_commit_validates_before_anything_is_launched():
    """No device is needed to see it: a call that got past the checks would try to launch."""
    L = _lib.lib()

    def record(**over):
        a = _lib.LoopArgs(state=0x1000, plan=0x1000, rows=0x1000, table=None, B=4, views=1, plan_len=8, table_rows=2)
        a.terms[:] = [0x1000] * 4
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return ctypes.byref(a)

    assert L.gwtf_loop_eval_commit(None) == E_BADARG
    assert L.gwtf_loop_eval_commit(record(state=None)) == E_BADARG
    for k in range(4):
        assert L.gwtf_loop_eval_commit(record(terms=(k, None))) == E_BADARG, k
    assert L.gwtf_loop_eval_commit(record(B=0)) == E_BADARG and L.gwtf_loop_eval_commit(record(B=-3)) == E_BADARG


def result(avg, poisoned=False):
    return {'LB': (avg, avg, 4 * avg, 4.0), 'poisoned': poisoned, 'poisoned_at': 0 if poisoned else -1}


def test_track_best_is_the_reference_rule():
    assert training.START_MIN_LOSS == 10000
    assert training.track_best(result(12.5)) == (True, 12.5)                   # first epoch: below the start value
    assert training.track_best(result(12.5), 12.5) == (False, 12.5)            # strictly below only (LB.avg < min_loss)
    assert training.track_best(result(12.25), 12.5) == (True, 12.25)
    assert training.track_best(result(20000.0)) == (False, 10000)
    assert training.track_best(result(-3.0), -2.0) == (True, -3.0)
    assert training.track_best(result(0.0, poisoned=True), 5.0) == (False, 5.0)  # a poisoned pass (empty meters) is never the best


def small_model():
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg']
    return models.Flow_Mixture_Model(**cfg), cfg


def test_checkpoint_is_the_reference_dictionary(tmp_path):
    m, _ = small_model()
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    ck = training.checkpoint(m, opt, 3, 7)
    assert list(ck) == ['epoch', 'iter', 'model_state', 'optimizer_state'] and (ck['epoch'], ck['iter']) == (3, 7)
    assert list(ck['model_state']) == list(m.state_dict()) and set(ck['optimizer_state']) == {'state', 'param_groups'}

    class Loop:                                            # the step count is read from the loop BEFORE the state is taken
        def meters(self):
            p = opt.param_groups[0]['params'][0]
            opt.state[p] = {'step': 5, 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p),
                            'max_exp_avg_sq': torch.zeros_like(p)}

    path = str(tmp_path / 'model.pth')
    training.save_checkpoint(path, m, opt, 4, 0, loop=Loop())
    back = torch.load(path, map_location='cpu')
    assert (back['epoch'], back['iter']) == (4, 0) and back['optimizer_state']['state'][0]['step'] == 5
    # the reference's resume sequence (train_ae.py:142-147)
    m2, _ = small_model()
    opt2 = optim.Adam(m2.parameters(), lr=1e-4, amsgrad=True)
    m2.load_state_dict(back['model_state'])
    opt2.load_state_dict(back['optimizer_state'])
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_resident_eval_loop_refuses_before_it_touches_a_device():
    D = golden('g22_clouds')
    store = gw.MeshStore.from_arrays(D['vertices_c'], D['faces_vc'], D['vertices_c_bounds'], D['faces_bounds'], device='cpu')
    m, cfg = small_model()
    crit = models.Flow_Mixture_Loss(**cfg)
    loader = gw.DeviceCloudLoader(store, 2, 48)
    with pytest.raises(ValueError, match='posterior'):
        training.ResidentEvalLoop(m, crit, loader, posterior='median')
    svr = models.Flow_Mixture_SVR_Model(**json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'])
    with pytest.raises(NotImplementedError, match='single-view reconstruction'):
        training.ResidentEvalLoop(svr, crit, loader)
    images = gw.ImageStore.from_arrays(np.zeros((6, 3, 8, 8), np.uint8), views_per_shape=2, device='cpu')
    with pytest.raises(NotImplementedError, match='single-view reconstruction'):
        training.ResidentEvalLoop(m, crit, gw.DeviceSVRLoader(store, images, 2, 48))
    with pytest.raises(NotImplementedError, match='one rank'):
        training.ResidentEvalLoop(m, crit, gw.DeviceCloudLoader(store, 1, 48, rank=1, world_size=2))
    with pytest.raises(ValueError, match='eval_cloud'):
        training.ResidentEvalLoop(m, crit, gw.DeviceCloudLoader(store, 2, 48, return_eval_cloud=False))
    with pytest.raises(ValueError, match='no full batch'):
        training.ResidentEvalLoop(m, crit, gw.DeviceCloudLoader(store, 4, 48))
    with pytest.raises(gw.GwtfError, match='HIP device'):                   # model and store on the host
        training.ResidentEvalLoop(m, crit, loader)
    with pytest.raises(NotImplementedError, match='image-conditioned'):
        svr.pin_eval_weights()
    assert m.eval_weights is None and m.training                            # nothing was pinned, no flag moved
