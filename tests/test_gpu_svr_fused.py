"""Flow_Mixture_SVR_Model on the fused training path (forward_fused + Flow_Mixture_Loss.fused + GraphedTrainStep with an image
buffer) against the genuine reference (golden g21), against the list path, and graphed against eager.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
from go_with_the_flows_amd import models, optim
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images
from go_with_the_flows_amd.training import GraphedTrainStep

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def build(**over):
    """tests/test_gpu_svr.py build()."""
    D = golden('g21_svr')
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], **over)
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    return m.to(DEV), cfg, D


def with_noise(m, D):
    noise = dev(D['noise_g'])
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    return m


@pytest.fixture(scope='module')
def images():
    return dev(synth_images(4, 64, 64, 2123))


@pytest.mark.parametrize('training', [False, True])
def test_fused_terms_match_reference(training, images):
    m, cfg, D = build()
    with_noise(m, D).train(training)
    loss_fn = models.Flow_Mixture_Loss(**cfg)
    with torch.no_grad():
        enc, dec = m.forward_fused(dev(D['gcloud']), dev(D['pcloud']), images=images)
        terms = [float(v) for v in loss_fn.fused(enc, dec)]
    assert '_g0_rows' in enc and '_g0_params' not in enc
    assert dec['z'].shape == (cfg['n_components'], 4, 3, D['pcloud'].shape[2])
    t = 'train' if training else 'eval'
    print('fused terms', t, terms, list(D[f'fwd_{t}_terms']))
    for got, want in zip(terms, D[f'fwd_{t}_terms']):
        assert abs(got - want) < (1e-3 if training else 2e-5) * max(1.0, abs(want))


def test_fused_step_matches_list_api_and_list_dict_is_unchanged(images):
    m, cfg, D = build()
    with_noise(m, D).train()
    loss_fn = models.Flow_Mixture_Loss(**cfg)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    g, p = dev(D['gcloud']), dev(D['pcloud'])
    enc, dec, logits = m(g, p, images)
    assert '_g0_params' not in enc and '_g0_rows' not in enc
    l1 = loss_fn(enc, dec, logits)[0]
    l1.backward()
    g1 = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
    m.load_state_dict(state)                       # undo the running-statistic updates
    m.zero_grad(set_to_none=True)
    enc, fused = m.forward_fused(g, p, images=images)
    l2 = loss_fn.fused(enc, fused)[0]
    l2.backward()
    assert abs(float(l1) - float(l2)) < 1e-4 * abs(float(l1))
    names = {n for n, q in m.named_parameters() if q.grad is not None}
    assert names == set(g1)
    for key in ('img_encoder.conv1.weight', 'g0_prior.mus.mu_mlp0.weight'):
        assert key in names and float(g1[key].abs().sum()) > 0 and float(dict(m.named_parameters())[key].grad.abs().sum()) > 0
    # the bound of tests/test_gpu_models.py:97-102: two evaluations whose batch statistics are summed with float atomics in different
    # orders move single entries of a FiLM weight gradient by up to ~2e-3 of the tensor's largest entry
    worst, wn = max((float((q.grad - g1[n]).abs().max() / (g1[n].abs().max() + 1e-3)), n) for n, q in m.named_parameters() if n in g1)
    print('fused vs list: worst', worst, wn)
    assert worst < 5e-3, (wn, worst, float(g1[wn].abs().max()))


def test_graphed_step_construction_leaves_no_trace_in_the_model(images):
    m, cfg, D = build()
    m.train()
    crit = models.Flow_Mixture_Loss(**cfg)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    g, p = dev(D['gcloud']), dev(D['pcloud'])
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert 'img_encoder.bn1.running_mean' in before and 'img_encoder.fc_bn.num_batches_tracked' in before
    rng_before = torch.cuda.get_rng_state(torch.device(DEV)).clone()
    step = GraphedTrainStep(m, crit, opt, g, p, images_example=images)
    torch.cuda.synchronize()
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert torch.equal(rng_before, torch.cuda.get_rng_state(torch.device(DEV)))
    terms = step(g, p, images)
    assert np.isfinite(float(terms[0]))
    assert int(after['img_encoder.bn1.num_batches_tracked']) == 1


def test_graphed_step_equals_eager_fused_steps_and_copies_the_images(images):
    """Three optimiser steps through GraphedTrainStep == three eager fused steps (same noise, same batches); then the image buffer:
    equal clouds with other images give another gnll."""
    D = golden('g21_svr')
    batches = [(dev(D['gcloud']) * s, dev(D['pcloud']) * s, dev(synth_images(4, 64, 64, seed))) for s, seed in
               ((1.0, 2123), (0.9, 2124), (1.1, 2125))]
    runs = []
    for graphed in (False, True):
        m, cfg, _ = build()
        with_noise(m, D).train()
        crit = models.Flow_Mixture_Loss(**cfg)
        opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
        losses = []
        if graphed:
            step = GraphedTrainStep(m, crit, opt, *batches[0][:2], images_example=batches[0][2])
            for g_in, p_in, i_in in batches:
                losses.append(float(step(g_in, p_in, i_in)[0]))
        else:
            for g_in, p_in, i_in in batches:
                opt.zero_grad(set_to_none=True)
                enc, dec = m.forward_fused(g_in, p_in, images=i_in)
                loss = crit.fused(enc, dec)[0]
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
                del loss, enc, dec
        runs.append((losses, {k: v.clone() for k, v in m.state_dict().items()}))
    (l0, s0), (l1, s1) = runs
    print('eager', l0, 'graphed', l1)
    for a, b in zip(l0, l1):
        assert abs(a - b) < 1e-4 * abs(a)
    # the step-size rule of tests/test_gpu_models.py:213-220: Adam normalises every gradient entry to ~lr, so entries whose gradient is
    # rounding noise move by +-lr either way -- compare against the step size, not against the gradient noise
    rel = [float((s0[k].float() - s1[k].float()).abs().max() / (s0[k].float().abs().max() + 1e-3)) for k in s0]
    print('max rel', max(rel), 'mean rel', sum(rel) / len(rel))
    assert max(rel) < 2e-2 and sum(rel) / len(rel) < 2e-4
    g_in, p_in = batches[0][:2]
    state = {k: v.clone() for k, v in m.state_dict().items()}
    gnll = []
    for i_in in (batches[0][2], batches[1][2]):
        m.load_state_dict(state)                  # the same model both times
        gnll.append(float(step(g_in, p_in, i_in)[2]))
    print('gnll', gnll)
    # independent images change every entry of the base Gaussian; a stale buffer would leave the two replays equal up to the fp32
    # rounding of the batch statistics' summation order (~1e-7 relative), two orders below this bound
    assert abs(gnll[0] - gnll[1]) > 1e-5 * abs(gnll[0]), gnll
