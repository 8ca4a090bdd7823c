"""Fused latent-loss launch with one base Gaussian per row (csrc/gwtf_latent.hip, prior.LatentLossRowsFn: the single-view
reconstruction model's base) against the reference formulas in float64 torch (losses.py:24-41, :159-170), against the shared-base
launch on a repeated row, and run to run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOG2PI = float(np.log(2.0 * np.pi))
W = (1.0, 0.75, 0.3)
UP = [1.3, -0.2, 0.5, 0.9]
NAMES = ['nll', 'z', 'mu0', 'lv0', 'flow_lv', 'post_lv']


def ref_terms(nll, z, mu0, lv0, flow_lv, post_lv, pw, gw, ew):
    """tests/test_gpu_latent.py ref_terms with (B, G) base tensors."""
    B, G = z.shape
    lv_sum = lv0 + flow_lv.sum(0)
    gnll = 0.5 * (torch.sum(lv_sum + (z - mu0) ** 2 / torch.exp(lv0)) / B + LOG2PI * G)
    gent = 0.5 * (G * (1.0 + LOG2PI) + post_lv.sum(1).mean())
    pnll = nll.mean()
    return torch.stack([pw * pnll + gw * gnll - ew * gent, pnll, gnll, gent])


def host_inputs(B, G, n2, rows=True):
    gen = torch.Generator().manual_seed(B * 1000 + G)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale)
    base = (B, G) if rows else (G,)
    return [mk(B) * 100 + 3000, mk(B, G), mk(*base, scale=0.1), mk(*base, scale=0.5), mk(n2, B, G, scale=0.3), mk(B, G, scale=0.7)]


# (1,1,1) smallest; (5,7,2) one partial block with a tail; (2,129,3) two blocks, a 2-element tail, odd n2 = the tail of the 2-unrolled
# flow_lv loop; (130,33,4) many blocks; (300,3,1) B > 256: the strided nll loop of the finish kernel, g_nll beyond the first block;
# (64,128,28) a training shape
@pytest.mark.parametrize('B,G,n2', [(1, 1, 1), (5, 7, 2), (2, 129, 3), (130, 33, 4), (300, 3, 1), (64, 128, 28)])
def test_values_and_gradients_match_float64(B, G, n2):
    from go_with_the_flows_amd.prior import LatentLossRowsFn
    host = host_inputs(B, G, n2)
    dev = [t.cuda().requires_grad_(True) for t in host]
    f64 = [t.double().requires_grad_(True) for t in host]
    got, want = LatentLossRowsFn.apply(*dev, *W), ref_terms(*f64, *W)
    assert torch.allclose(got.double().cpu(), want, rtol=2e-6, atol=1e-5), (got, want)
    up = torch.tensor(UP)
    got.backward(up.cuda())
    want.backward(up.double())
    for a, b, name in zip(dev, f64, NAMES):
        assert a.grad.shape == b.grad.shape, name
        scale = max(1e-30, float(b.grad.abs().max()))
        assert float((a.grad.double().cpu() - b.grad).abs().max()) <= 5e-6 * scale, name


@pytest.mark.parametrize('B,G,n2', [(5, 7, 2), (64, 128, 28)])
def test_repeated_row_equals_the_shared_base_launch(B, G, n2):
    from go_with_the_flows_amd.prior import LatentLossFn, LatentLossRowsFn
    host = host_inputs(B, G, n2, rows=False)
    shared = [t.cuda().requires_grad_(True) for t in host]
    rows = [t.cuda() for t in host]
    rows[2], rows[3] = rows[2].expand(B, G).contiguous(), rows[3].expand(B, G).contiguous()
    rows = [t.requires_grad_(True) for t in rows]
    a, b = LatentLossRowsFn.apply(*rows, *W), LatentLossFn.apply(*shared, *W)
    for x, y in zip(a.tolist(), b.tolist()):
        assert abs(x - y) <= 2e-6 * max(1.0, abs(y))
    up = torch.tensor(UP).cuda()
    a.backward(up)
    b.backward(up)
    for i in (2, 3):                               # relative to the tensor's largest entry, as every gradient check of this kernel
        want = shared[i].grad.double()
        assert float((rows[i].grad.double().sum(0) - want).abs().max()) <= 5e-6 * float(want.abs().max()), NAMES[i]


def test_two_calls_give_identical_bits():
    from go_with_the_flows_amd.prior import LatentLossRowsFn
    host = host_inputs(130, 33, 4)
    outs = []
    for _ in range(2):
        dev = [t.cuda().requires_grad_(True) for t in host]
        got = LatentLossRowsFn.apply(*dev, *W)
        got.backward(torch.tensor(UP).cuda())
        outs.append([got.detach().clone()] + [t.grad.clone() for t in dev])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_loss_module_uses_the_rows_launch_and_matches_the_torch_combination(monkeypatch):
    from go_with_the_flows_amd.models import Flow_Mixture_Loss
    crit = Flow_Mixture_Loss(pnll_weight=1.0, gnll_weight=1.0, gent_weight=0.5, n_components=4)
    B, G, n2 = 6, 16, 4
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    mu0, lv0 = r(B, G).requires_grad_(True), r(B, G).requires_grad_(True)
    stacked = r(n2, B, G).requires_grad_(True)
    z, post = r(B, G).requires_grad_(True), r(B, G).requires_grad_(True)
    nll = (r(B) + 50).requires_grad_(True)
    leaves = [mu0, lv0, stacked, z, post, nll]

    def prior():
        return {'g_prior_samples': [z, z], 'g_prior_mus': [mu0] + list(stacked.unbind(0)),
                'g_prior_logvars': [lv0] + list(stacked.unbind(0)), 'g_posterior_logvars': post,
                '_g_prior_logvars_stacked': stacked, '_g0_rows': (mu0, lv0)}

    from go_with_the_flows_amd import prior as prior_mod
    calls, shared_calls = [], []
    orig, orig_shared = prior_mod.LatentLossRowsFn.apply, prior_mod.LatentLossFn.apply
    monkeypatch.setattr(prior_mod.LatentLossRowsFn, 'apply', staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    monkeypatch.setattr(prior_mod.LatentLossFn, 'apply', staticmethod(lambda *a: (shared_calls.append(1), orig_shared(*a))[1]))
    a = crit._combine(nll, prior())
    a[0].backward()
    ga = [t.grad.clone() for t in leaves]
    assert calls == [1] and shared_calls == []
    for t in leaves:
        t.grad = None
    monkeypatch.setenv('GWTF_NO_FUSED_LATENT_LOSS', '1')
    b = crit._combine(nll, prior())
    b[0].backward()
    assert calls == [1] and shared_calls == []
    for x, y in zip(a, b):
        assert abs(float(x) - float(y)) <= 2e-6 * max(1.0, abs(float(y)))
    for x, t in zip(ga, leaves):
        assert float((x - t.grad).abs().max()) <= 2e-6 * max(1e-30, float(t.grad.abs().max()))
