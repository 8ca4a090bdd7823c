"""The mixture NLL kernels (csrc/gwtf_nll.hip: nll_kernel / nll_bwd_kernel) against the reference formula in float64 torch, at
the shapes that select each branch of the launch: one 1024-thread workgroup per shape (N <= 4096 and B >= 16) or 512-point
blocks with float atomics, a partial last block, K up to kMaxK.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from conftest import TOL_NLL_REL
from helpers import mixture_nll_torch
from go_with_the_flows_amd import _lib
from go_with_the_flows_amd.mixture import _MixtureNLLFn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24                      # fp32 unit roundoff
FLT_MIN = float(np.finfo(np.float32).tiny)

SHAPES = [
    (4, 64, 2048),     # airplane: single-workgroup path
    (4, 16, 4096),     # last single-workgroup size
    (4, 16, 4097),     # first multi-block size
    (4, 15, 2048),     # multi-block because B < 16
    (4, 4, 2500),      # the 11x33x512 config: last block partial
    (2, 2, 513),       # two blocks, one point in the second
    (1, 1, 1),         # minimal shape
    (16, 1, 2048),     # the sampling K
    (64, 3, 700),      # kMaxK
]
LOGITS = ['random', 'dominant', 'c0_m200', 'c2_m200', 'all_m200']


def _inputs(K, B, N, magnitude, logit_case, seed):
    """Synthetic z, logdet (K,B,3,N), mu0, lv0 (K,B,3), logits (B,K), float32 numpy.  The components' lv0 form a ladder from ~-6 to
    ~+4 (jitter a fifth of a rung, so every component is wider than the one below it in every dimension): far out in the tail one
    component dominates by a wide margin, and the points where two components share the responsibility are those of moderate |z|,
    where fp32 resolves the log-densities to a few ulp.  'bench' is the heavy tail of synth_state(output_gain=1) on the airplane grid
    (Cauchy-like, reaching |z| = 5e3)."""
    rng = np.random.default_rng(seed)
    if K > 1:
        rung = 10.0 / (K - 1)
        base = np.linspace(-6.0, 4.0, K)[rng.permutation(K)]
        lv0 = base[:, None, None] + 0.2 * rung * rng.uniform(-1, 1, size=(K, B, 3))
    else:
        lv0 = rng.uniform(-1, 1, size=(K, B, 3))
    mu0 = 2.0 * rng.normal(size=(K, B, 3))
    if magnitude == 'conditioned':
        z = 1.5 * rng.normal(size=(K, B, 3, N))
        logdet = 2.0 * rng.normal(size=(K, B, 3, N))
    else:
        z = np.clip(3.0 * rng.standard_cauchy(size=(K, B, 3, N)), -5e3, 5e3)
        z.flat[rng.integers(z.size)] = -5e3
        logdet = 5.0 * rng.normal(size=(K, B, 3, N))
    logits = 2.0 * rng.normal(size=(B, K))
    if logit_case == 'dominant':
        logits[np.arange(B), rng.integers(K, size=B)] = 30.0
    elif logit_case == 'c0_m200':
        logits[:, 0] = -200.0
    elif logit_case == 'c2_m200':
        logits[:, 2] = -200.0
    elif logit_case == 'all_m200':
        logits[:] = -200.0
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (z, logdet, mu0, lv0, logits))


def _cases():
    for K, B, N in SHAPES:
        for mag in ('conditioned', 'bench'):
            for lc in LOGITS:
                if (lc == 'c0_m200' and K < 2) or (lc == 'c2_m200' and K < 3):
                    continue
                yield pytest.param(K, B, N, mag, lc, id=f'K{K}-B{B}-N{N}-{mag}-{lc}')


def _t(arrs, dtype, device='cpu', grad=False):
    return [torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(grad) for a in arrs]


@pytest.mark.parametrize('K,B,N,mag,lc', list(_cases()))
def test_mixture_nll_vs_fp64(K, B, N, mag, lc):
    arrs = _inputs(K, B, N, mag, lc, seed=K * 1000003 + B * 1009 + N + LOGITS.index(lc) + (7 if mag == 'bench' else 0))
    z, logdet, mu0, lv0, logits = _t(arrs, torch.float32, DEV)
    nll, plse = _lib.mixture_nll(z, logdet, mu0, lv0, logits, want_point_lse=True)
    nll, plse = nll.cpu().double(), plse.cpu().double()
    nll32 = mixture_nll_torch(*_t(arrs, torch.float32), quirk=True)[0].double()          # fp32 torch of the reference
    if lc == 'all_m200':
        # every log weight underflows in fp32 (log(exp(-200)) = -inf): the reference's fp32 loss is +inf, and so is the kernel's
        assert torch.isinf(nll32).all() and (nll32 > 0).all()
        assert torch.equal(nll, nll32), (nll, nll32)
        return
    leaves = _t(arrs, torch.float64, grad=True)
    nll64, lse64, lp64, logw64 = mixture_nll_torch(*leaves, quirk=True)
    assert torch.isfinite(nll).all() and torch.isfinite(plse).all(), (nll, int((~torch.isfinite(plse)).sum()))

    # per-point lse: a few ulp of the magnitude of the terms the components that carry the point sum
    z64, ld64, mu64, lv64, lg64 = (t.detach() for t in leaves)
    diff = z64 - mu64[..., None]
    iv = torch.exp(-lv64)[..., None]
    terms = 0.5 * (lv64[..., None].abs() + ld64.abs() + diff * diff * iv).sum(2) + logw64.detach().t()[:, :, None].abs() + 3.0
    a = lp64.detach() + logw64.detach().t()[:, :, None]                                   # (K,B,N)
    terms = torch.where(torch.isfinite(a), terms, torch.zeros_like(terms))              # an underflowed component carries nothing
    carry = a >= a.max(0, keepdim=True).values - 30.0                                    # the dominant component (and any near tie)
    scale = torch.where(carry, terms, torch.zeros_like(terms)).max(0).values
    err_pt = (plse - lse64.detach()).abs()
    assert (err_pt <= 8 * U * scale).all(), float((err_pt / scale).max() / U)

    # per-shape NLL: sum-condition bound, and no worse than fp32 torch's own distance to fp64
    cond = lse64.detach().abs().sum(-1)
    err = (nll - nll64.detach()).abs()
    assert (err <= TOL_NLL_REL * cond).all(), float((err / cond).max())
    err32 = (nll32 - nll64.detach()).abs()
    assert (err <= 3 * err32 + 1e-6 * cond).all(), (err, err32, cond)

    # backward with a non-uniform upstream gradient
    g = torch.from_numpy(np.random.default_rng(N + K).normal(size=B))
    (nll64 * g).sum().backward()
    hl = _t(arrs, torch.float32, DEV, grad=True)
    nll_h, _ = _MixtureNLLFn.apply(*hl)
    grads = torch.autograd.grad((nll_h * g.float().to(DEV)).sum(), hl)
    grads = [t.cpu().double() for t in grads]
    # Every gradient carries the responsibility r_k(n) = exp(lp_k - lse_n).  fp32 resolves lp_k - lse_n only to a few ulp of the terms
    # that enter it (the bound on lse above), so r is known to the relative precision rho = 8u (terms_k + scale_n) and no better: at a
    # bench-like point with terms ~1e3, rho ~ 5e-4 (fp32 torch of the reference misses the plain 1e-5 bounds there by 3x).  That part
    # of the error sits on each contribution on top of the 1e-5.
    rho = 8 * U * (terms + scale[None])                                                  # (K,B,N)
    for name, gh, leaf in zip(('z', 'logdet'), grads[:2], leaves[:2]):
        ref = leaf.grad
        assert torch.isfinite(gh).all(), name
        bad = (gh - ref).abs() > 1e-5 * ref.abs().max() + rho[:, :, None] * ref.abs()
        assert not bad.any(), (name, float((gh - ref).abs().max()), float(ref.abs().max()))
    # mu0 / lv0 / logits: sums over the N points -- bounded by the sum of the magnitudes of what the points contribute
    r = torch.exp(a - lse64.detach()[None])                                              # (K,B,N) responsibilities
    ga = g.abs()[None, :, None]
    w = 1e-5 + rho
    s_mu = (w[:, :, None] * r[:, :, None] * (diff * iv).abs()).sum(-1) * ga              # (K,B,3)
    s_lv = (w[:, :, None] * r[:, :, None] * (0.5 + 0.5 * diff * diff * iv)).sum(-1) * ga
    sm = torch.softmax(lg64, -1)                                                         # (B,K)
    s_lg = ((w * r).sum(-1).t() + 1e-5 * N * sm) * g.abs()[:, None]
    for name, gh, leaf, s in zip(('mu0', 'lv0', 'logits'), grads[2:], leaves[2:], (s_mu, s_lv, s_lg)):
        ref = leaf.grad
        assert torch.isfinite(gh).all(), name            # a -200 logit: the finite limit, where fp32 autograd of log(exp(.)) is NaN
        bad = (gh - ref).abs() > s + FLT_MIN
        assert not bad.any(), (name, float(((gh - ref).abs() / (s + FLT_MIN)).max()))


@pytest.mark.parametrize('nan_k,lc', [(0, 'random'), (2, 'random'), (2, 'c0_m200')])
def test_nan_point_poisons_only_its_shape(nan_k, lc):
    """A NaN in one point of shape b makes nll[b] NaN (also after a component skipped for its -inf log weight); every other shape is
    finite and bit-equal to the NaN-free run (single-workgroup path: no atomics, so the sums are reproducible)."""
    K, B, N = 4, 16, 1024
    arrs = _inputs(K, B, N, 'conditioned', lc, seed=77)
    clean = _lib.mixture_nll(*_t(arrs, torch.float32, DEV), want_point_lse=True)
    z = arrs[0].copy()
    z[nan_k, 5, 1, 100] = np.nan
    dirty = _lib.mixture_nll(*_t((z,) + arrs[1:], torch.float32, DEV), want_point_lse=True)
    (n0, p0), (n1, p1) = [(a.cpu(), b.cpu()) for a, b in (clean, dirty)]
    assert torch.isfinite(n0).all()
    assert torch.isnan(n1[5]) and torch.isnan(p1[5, 100])
    others = torch.arange(B) != 5
    assert torch.isfinite(n1[others]).all() and torch.equal(n1[others], n0[others])
    keep = torch.ones(B, N, dtype=torch.bool)
    keep[5, 100] = False
    assert torch.equal(p1[keep], p0[keep])


def test_more_components_than_kmaxk_is_refused():
    K, B, N = 65, 1, 4
    z, logdet, mu0, lv0, logits = _t(_inputs(K, B, N, 'conditioned', 'random', 1), torch.float32, DEV)
    with pytest.raises(_lib.GwtfError):
        _lib.mixture_nll(z, logdet, mu0, lv0, logits, want_point_lse=True)
