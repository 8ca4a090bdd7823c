"""Flow_Mixture_SVR_Model end to end on the GPU against the genuine reference (golden g21: weights seeded, image-encoder running
statistics calibrated and stored, noise injected).  Needs an MI355X."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN, TOL_COORD
from helpers import maxabs
from go_with_the_flows_amd import models, optim
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def build(**over):
    D = golden('g21_svr')
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], **over)
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    return m.to(DEV), cfg, D


def test_labelled_reconstruction_matches_reference():
    m, cfg, D = build(util_mode='reconstruction')
    m.eval()
    noise_p = dev(D['rec_noise_p'])
    m.reparameterize = lambda mu, logvar: noise_p[:, :, :mu.shape[2]] * torch.exp(0.5 * logvar) + mu
    Ns = D['rec_samples'].shape[2]
    imgs = synth_images(4, 64, 64, 2123)
    np.random.seed(2130)
    with torch.no_grad():
        enc, samples, labels, logits = m(dev(D['gcloud'][:1, :, :Ns]), dev(D['pcloud'][:1, :, :Ns]), dev(imgs[:1]), Ns, True, False)
    assert maxabs(host(enc['g_prior_samples'][-1]), D['rec_g']) < 2e-5
    assert maxabs(host(logits), D['rec_logits']) < 2e-5
    assert np.array_equal(host(labels), D['rec_labels'])
    assert maxabs(host(samples), D['rec_samples']) < TOL_COORD


@pytest.mark.parametrize('training', [False, True])
def test_encode_both_modes_match_reference(training):
    m, cfg, D = build()
    m.train(training)
    noise = dev(D['noise_g'])
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    imgs = dev(synth_images(4, 64, 64, 2123))
    t = 'train' if training else 'eval'
    tol = 5e-4 if training else 2e-5
    for mode in ('training', 'reconstruction'):
        m.mode = mode
        with torch.no_grad():
            enc = m.encode(dev(D['gcloud']), imgs)
        k = f'enc_{mode}_{t}'
        assert [len(enc['g_prior_samples']), len(enc['g_prior_mus'])] == list(D[k + '_n_lists'])
        assert maxabs(host(enc['g_prior_mus'][0]), D[k + '_prior_mu0']) < tol
        assert maxabs(host(enc['g_prior_logvars'][0]), D[k + '_prior_lv0']) < tol
        assert maxabs(host(enc['g_prior_samples'][0]), D[k + '_prior_first']) < 10 * tol
        assert maxabs(host(enc['g_prior_samples'][-1]), D[k + '_prior_last']) < 10 * tol
    m.mode = 'generating'
    with pytest.raises(ValueError):
        m.encode(dev(D['gcloud']), imgs)


@pytest.mark.parametrize('training', [False, True])
def test_training_mode_forward_and_loss_match_reference(training):
    m, cfg, D = build()
    m.train(training)
    noise = dev(D['noise_g'])
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    t = 'train' if training else 'eval'
    tol = 5e-4 if training else 2e-5
    loss_fn = models.Flow_Mixture_Loss(**cfg)
    with torch.no_grad():
        enc, dec, logits = m(dev(D['gcloud']), dev(D['pcloud']), dev(synth_images(4, 64, 64, 2123)))
        terms = [float(v) for v in loss_fn(enc, dec, logits)]
    assert '_g0_params' not in enc
    assert [len(enc['g_prior_samples']), len(enc['g_prior_mus']), len(dec[0]['p_prior_samples'])] == list(D[f'fwd_{t}_n_lists'])
    assert maxabs(host(logits), D[f'fwd_{t}_logits']) < tol
    assert maxabs(host(enc['g_posterior_samples']), D[f'fwd_{t}_g_sample']) < tol
    assert maxabs(host(enc['g_prior_samples'][0]), D[f'fwd_{t}_g_base']) < 10 * tol
    assert maxabs(np.stack([host(o['p_prior_samples'][0]) for o in dec]), D[f'fwd_{t}_z']) < 10 * tol
    for got, want in zip(terms, D[f'fwd_{t}_terms']):
        assert abs(got - want) < (1e-3 if training else 2e-5) * max(1.0, abs(want))


def test_reconstruct_many_equals_separate_calls():
    m, cfg, D = build(util_mode='reconstruction')
    m.eval()
    S, n, K = 4, 300, cfg['n_components']
    imgs = dev(synth_images(S, 64, 64, 2250))
    rng = np.random.default_rng(5)
    draws = [rng.integers(0, K, n) for _ in range(S)]
    base = torch.randn(S, 3, n, device=DEV)
    it = iter(draws)
    m._draw_components = lambda row, k: next(it)
    m.reparameterize = lambda mu, logvar: base * torch.exp(0.5 * logvar) + mu
    x, labels = m.reconstruct_many(imgs, n, return_labels=True)
    assert x.shape == (S, 3, n) and np.array_equal(host(labels), np.stack(draws) + 1)
    for s in range(S):
        m._draw_components = lambda row, k, s=s: draws[s]
        m.reparameterize = lambda mu, logvar, s=s: base[s:s + 1, :, :mu.shape[2]] * torch.exp(0.5 * logvar) + mu
        with torch.no_grad():
            enc = m.encode(None, imgs[s:s + 1])
            want = m.sample_many(enc['g_prior_samples'][-1], n)
        assert maxabs(host(x[s:s + 1]), host(want)) < TOL_COORD, s


def test_one_training_step_gradients_match_float64_autograd():
    """Forward, Flow_Mixture_Loss, backward and the fused AMSGrad step on a small SVR config (64 x 64 images); the parameter
    gradients against a float64 CPU autograd of the module graph (the image encoder's library path, oracle-free)."""
    m, cfg, D = build()
    m.train()
    noise = dev(D['noise_g'])
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    imgs = dev(synth_images(4, 64, 64, 2123))
    loss_fn = models.Flow_Mixture_Loss(**cfg)
    enc, dec, logits = m(dev(D['gcloud']), dev(D['pcloud']), imgs)
    loss = loss_fn(enc, dec, logits)[0]
    assert torch.isfinite(loss)
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    opt.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert grads['img_encoder.conv1.weight'].abs().sum() > 0 and grads['g0_prior.mus.mu_mlp0.weight'].abs().sum() > 0
    # float64 autograd of the image-conditioned base: the only new path in the gradient (the rest is pinned by test_gpu_models)
    enc64 = copy.deepcopy(m.img_encoder).cpu().double().train()
    enc64.load_state_dict({k[len('img_encoder.'):]: v.cpu().double() for k, v in state.items() if k.startswith('img_encoder.')})
    head64 = copy.deepcopy(m.g0_prior).cpu().double().train()
    head64.load_state_dict({k[len('g0_prior.'):]: v.cpu().double() for k, v in state.items() if k.startswith('g0_prior.')})
    mu64, lv64 = head64(enc64.forward_torch(imgs.cpu().double()))
    z0 = enc['g_prior_samples'][0].detach().cpu().double()
    gnll_base = 0.5 * ((lv64 + (z0 - mu64) ** 2 / torch.exp(lv64)).sum() / z0.shape[0]) * cfg['gnll_weight']
    gnll_base.backward()
    pairs = [('img_encoder.' + n, q) for n, q in enc64.named_parameters()] + [('g0_prior.' + n, q) for n, q in head64.named_parameters()]
    top = max(float(q.grad.abs().max()) for _, q in pairs)
    for key, p in pairs:
        # (a Linear bias in front of a train-mode BatchNorm has a zero gradient: fp32 leaves ~1e-6 of the largest gradient there)
        got, want = grads[key].cpu().double(), p.grad
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()) + 1e-5 * top, key
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.step()
    moved = [n for n, p in m.named_parameters() if n in grads and not torch.equal(p, before[n])]
    assert 'img_encoder.conv1.weight' in moved and all(torch.isfinite(p).all() for p in m.parameters())


def test_base_class_still_refuses_images():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'])
    m = models.Flow_Mixture_Model(**cfg).to(DEV)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 3, 8, device=DEV), torch.zeros(2, 3, 8, device=DEV), torch.zeros(2, 4, 64, 64, device=DEV))
