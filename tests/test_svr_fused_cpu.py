"""Host side of the fused single-view-reconstruction training path: the latent-loss exports (csrc/gwtf_latent.hip: one record, the
per-row base Gaussian its `rows` field) are declared, bound and exported, and every argument check of Flow_Mixture_SVR_Model.forward_fused / GraphedTrainStep(images_example=)
fires before any device work.  No GPU: a check that came after a device call would fail here with another exception."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT
from go_with_the_flows_amd import _lib, models
from go_with_the_flows_amd.training import GraphedTrainStep

NEW = ('gwtf_latent_loss_forward', 'gwtf_latent_loss_backward')


def small_cfg(**over):
    return dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], **over)


@pytest.fixture(scope='module')
def svr():
    return models.Flow_Mixture_SVR_Model(**small_cfg())


@pytest.fixture(scope='module')
def plain():
    return models.Flow_Mixture_Model(**small_cfg())


def inputs(B=2, N=8, side=32):
    return torch.zeros(B, 3, N), torch.zeros(B, 3, N), torch.zeros(B, 4, side, side)


def test_exports_are_declared_bound_and_exported_without_an_abi_bump():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES and name in _lib.EXPORTS
        assert _lib._SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p])     # both families: one record, its `rows` field
    assert 'rows' in dict(_lib.LatentLossArgs._fields_)
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header
    L = _lib.lib()
    assert L.gwtf_abi_version() == 12
    for name in NEW:
        assert hasattr(L, name)
    # argument checks of the launchers: nothing is launched on a refused call
    fake = 0x1000
    pointers = [n for n, t in _lib.LatentLossArgs._fields_ if t is ctypes.c_void_p and n != 'stream']
    for rows in (0, 1):
        null = _lib.LatentLossArgs(B=2, G=2, n2=2, rows=rows, pw=1.0, gw=1.0, ew=1.0)
        assert L.gwtf_latent_loss_forward(ctypes.byref(null)) == 10001
        assert L.gwtf_latent_loss_backward(ctypes.byref(null)) == 10001
        for B, G, n2 in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (1 << 20, 1 << 12, 1)):     # the last: B * G does not fit the element index
            a = _lib.LatentLossArgs(B=B, G=G, n2=n2, rows=rows, pw=1.0, gw=1.0, ew=1.0, **{n: fake for n in pointers})
            assert L.gwtf_latent_loss_forward(ctypes.byref(a)) == 10001
            assert L.gwtf_latent_loss_backward(ctypes.byref(a)) == 10001


def test_rows_function_names_all_shapes_in_its_error():
    from go_with_the_flows_amd.prior import LatentLossRowsFn
    B, G, n2 = 3, 5, 2
    good = [torch.zeros(B), torch.zeros(B, G), torch.zeros(B, G), torch.zeros(B, G), torch.zeros(n2, B, G), torch.zeros(B, G)]
    for i, bad in ((0, torch.zeros(B + 1)), (2, torch.zeros(G)), (3, torch.zeros(1, G)), (4, torch.zeros(n2, B, G + 1)),
                   (5, torch.zeros(G, B)), (1, torch.zeros(B * G))):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.GwtfError) as err:
            LatentLossRowsFn.apply(*args, 1.0, 1.0, 1.0)
        for t in args:
            assert str(tuple(t.shape)) in str(err.value)


def test_forward_fused_checks_its_arguments_before_any_device_work(svr):
    g, p, imgs = inputs()
    with pytest.raises(ValueError, match='images'):
        svr.forward_fused(g, p)
    svr.mode = 'reconstruction'
    try:
        with pytest.raises(ValueError, match='training'):
            svr.forward_fused(g, p, images=imgs)
    finally:
        svr.mode = 'training'


def test_graphed_step_checks_its_arguments_before_any_device_work(svr, plain):
    g, p, imgs = inputs()
    crit = models.Flow_Mixture_Loss(**small_cfg())
    with pytest.raises(ValueError, match='images_example'):
        GraphedTrainStep(svr, crit, None, g, p)
    with pytest.raises(ValueError, match='img_encoder'):
        GraphedTrainStep(plain, crit, None, g, p, images_example=imgs)
    with pytest.raises(NotImplementedError, match='multi-rank SVR training is not built'):
        GraphedTrainStep(svr, crit, None, g, p, data_parallel=True, images_example=imgs)


def test_graphed_step_refuses_inconsistent_images_at_call_time():
    g, p, imgs = inputs()
    step = GraphedTrainStep.__new__(GraphedTrainStep)          # (construction needs a device: only the call-time check is under test)
    step.g_static, step.p_static, step.i_static = g.clone(), p.clone(), imgs.clone()
    with pytest.raises(ValueError, match='images'):
        step(g, p)
    step.i_static = None
    with pytest.raises(ValueError, match='images'):
        step(g, p, imgs)


def test_encode_keeps_the_rows_entry_off_the_default_dict(svr, monkeypatch):
    """encode(fused_base=...) on the CPU through the module graph: '_g0_rows' appears only on request and holds the list's tensors."""
    imgs = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(3))
    monkeypatch.setattr(svr.img_encoder, 'forward', svr.img_encoder.forward_torch)
    svr.eval()
    svr.mode = 'reconstruction'                  # (the 'training' branch needs the cloud encoder's kernels; the base is built before it)
    try:
        with torch.no_grad():
            plain_out = svr.encode(None, imgs)
            fused_out = svr.encode(None, imgs, fused_base=True)
    finally:
        svr.mode = 'training'
        svr.train()
    assert '_g0_rows' not in plain_out and '_g0_params' not in plain_out and '_g0_params' not in fused_out
    mus, logvars = fused_out['_g0_rows']
    assert mus is fused_out['g_prior_mus'][0] and logvars is fused_out['g_prior_logvars'][0] and mus.shape == (2, 16)
