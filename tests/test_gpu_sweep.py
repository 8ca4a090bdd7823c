"""Latent sweeps on the GPU: the sweep routing launch (gwtf_mixture_route_sweep) against its numpy restatement (sweep_ref.py) and
against gwtf_mixture_route, the per-component FiLM launch (gwtf_film_forward_k) against gwtf_film_forward, and
Flow_Mixture_Model.interpolate_many / upsample_many and evaluation.interpolate_clouds / upsample_clouds on top.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_COORD
from helpers import decoder_and_state, maxabs
import generate_ref as gr
import sweep_ref as sr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models
from go_with_the_flows_amd.synth import load_synth_
from oracle import torch_port as tp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_NORMAL = 1e-4          # restated exp / Box-Muller values against the device's (tests/test_gpu_generate.py, the same arithmetic)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(words):
    return dev(np.asarray(words, np.uint32).view(np.int32))


def make_model(**over):
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating', **over)
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    return m.to(DEV).eval(), cfg


_MODELS = {}


def model_of(weights_type='learned_weights', n_components=3):
    key = (weights_type, n_components)
    if key not in _MODELS:
        _MODELS[key] = make_model(weights_type=weights_type, n_components=n_components)
    return _MODELS[key]


def sweep_inputs(S, T, n, K, seed, lv_scale=0.0):
    rng = np.random.RandomState(seed)
    R = S * T
    words = rng.randint(0, 2**32, (S, n), dtype=np.uint64).astype(np.uint32)
    words[0, :1] = 0
    words[-1, -1:] = 0xffffffff
    return dict(logits=rng.normal(0, 1.5, (R, K)).astype(np.float32), words=words,
                normals=rng.normal(0, 1, (S, 3, n)).astype(np.float32), mu0=rng.normal(0, 0.3, (K, R, 3)).astype(np.float32),
                lv0=(lv_scale * rng.normal(-1, 0.5, (K, R, 3))).astype(np.float32))


def check_rows(work, want, tol=0.0):
    """labels / tile_comp / perm of a sweep routing call equal the restatement exactly, zp within tol with exact zeros in the padding."""
    for k in ('labels', 'tile_comp', 'perm'):
        assert np.array_equal(host(work[k]), want[k]), k
    zp, valid = host(work['zp']), want['perm'] >= 0
    for r in range(len(valid)):
        assert (zp[r][:, ~valid[r]] == 0).all()
        if valid[r].any():
            err = np.abs(zp[r][:, valid[r]] - want['zp'][r][:, valid[r]]).max()
            assert err <= tol, (r, err)


def z0_of(work):
    """The base samples of a routing call in the points' own order, (R, 3, n), from zp and perm."""
    R, n = work['labels'].shape
    z0 = torch.full((R, 3, n), float('nan'), device=DEV)
    perm = work['perm'].long()
    for r in range(R):
        valid = perm[r] >= 0
        z0[r][:, perm[r][valid]] = work['zp'][r][:, valid]
    assert torch.isfinite(z0).all()
    return z0


# ---- 1. the sweep routing launch against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize('S,T,n,K,P', [(1, 1, 1, 1, 64), (3, 4, 300, 3, 64), (2, 9, 300, 3, 256), (2, 3, 2500, 64, 128)])
def test_sweep_routing_with_explicit_draws_equals_the_restatement(S, T, n, K, P):
    d = sweep_inputs(S, T, n, K, 100 + n + K + P)                         # lv0 = 0: sd = expf(0) = 1, the base samples are exact
    work = _lib.route_scratch(S * T, n, K, P, torch.device(DEV))
    _lib.mixture_route_sweep(work, group=T, logits=dev(d['logits']), mu0=dev(d['mu0']), lv0=dev(d['lv0']), words=bits(d['words']),
                             normals=dev(d['normals']))
    thr = host(work['thresholds']).view(np.uint32)
    # one ulp of float64 times 2^32 is far below 1: the ceiling moves by at most one
    assert np.abs(thr.astype(np.int64) - gr.thresholds(d['logits']).astype(np.int64)).max() <= 1
    want = sr.route(d['logits'], T, n, K, P, words=d['words'], normals=d['normals'], mu0=d['mu0'], lv0=d['lv0'], thr=thr)
    assert want['labels'].min() >= 0 and want['labels'].max() <= K - 1
    check_rows(work, want)


def test_sweep_routing_with_a_deviation_per_component():
    S, T, n, K, P = 3, 4, 300, 3, 64
    d = sweep_inputs(S, T, n, K, 21, lv_scale=1.0)
    work = _lib.route_scratch(S * T, n, K, P, torch.device(DEV))
    _lib.mixture_route_sweep(work, group=T, logits=dev(d['logits']), mu0=dev(d['mu0']), lv0=dev(d['lv0']), words=bits(d['words']),
                             normals=dev(d['normals']))
    want = sr.route(d['logits'], T, n, K, P, words=d['words'], normals=d['normals'], mu0=d['mu0'], lv0=d['lv0'],
                    thr=host(work['thresholds']).view(np.uint32))
    check_rows(work, want, tol=TOL_NORMAL)
    # the tables differ between components: points that took the next component's base miss by far more than the tolerance
    wrong = sr.base_samples(d['normals'], (want['labels'] + 1) % K, d['mu0'], d['lv0'], T, K)
    assert np.abs(wrong - want['z0']).max() > 1000 * TOL_NORMAL


@pytest.mark.parametrize('P', [64, 128])
def test_sweep_routing_of_crafted_labels_sits_on_the_tile_edges(P):
    n, K, T = 300, 3, 2
    labels = gr.crafted_labels(n, K, P)
    S = len(labels)
    d = sweep_inputs(S, T, n, K, 3)
    work = _lib.route_scratch(S * T, n, K, P, torch.device(DEV))
    _lib.mixture_route_sweep(work, group=T, mu0=dev(d['mu0']), lv0=dev(d['lv0']), labels_in=dev(labels), normals=dev(d['normals']))
    check_rows(work, sr.route(None, T, n, K, P, labels_in=labels, normals=d['normals'], mu0=d['mu0'], lv0=d['lv0']))
    # and with the base samples themselves
    _lib.mixture_route_sweep(work, group=T, labels_in=dev(labels), z0_in=dev(d['normals']))
    check_rows(work, sr.route(None, T, n, K, P, labels_in=labels, z0_in=d['normals']))


# ---- 2. / 3. Philox mode against gwtf_mixture_route --------------------------------------------------------------------------------
KEYS = ('thresholds', 'tile_comp', 'perm', 'zp', 'labels')


def test_one_row_per_shape_and_one_base_is_the_routing_launch_bit_for_bit():
    S, n, K, P, seed, call = 3, 1000, 3, 128, 77, 5
    rng = np.random.RandomState(6)
    logits = dev(rng.normal(0, 1, (S, K)).astype(np.float32))
    mu0, lv0 = dev(rng.normal(0, 0.3, (S, 3)).astype(np.float32)), dev(rng.normal(-1, 0.5, (1, 3)).astype(np.float32))
    a, b = (_lib.route_scratch(S, n, K, P, torch.device(DEV)) for _ in range(2))
    sa, sb = gw.make_state(seed, DEV, call), gw.make_state(seed, DEV, call)
    _lib.mixture_route(a, logits=logits, mu0=mu0, lv0=lv0, state=sa)
    _lib.mixture_route_sweep(b, group=1, logits=logits, mu0=mu0, lv0=lv0, state=sb)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert sa.cpu().tolist() == sb.cpu().tolist() == [seed, call + 1]


def test_the_rows_of_a_group_share_the_draws_of_their_shape():
    S, T, n, K, P, seed, call = 3, 4, 1000, 3, 128, 78, 9
    rng = np.random.RandomState(7)
    logits = rng.normal(0, 1, (S, K)).astype(np.float32)
    mu0, lv0 = rng.normal(0, 0.3, (S, 3)).astype(np.float32), rng.normal(-1, 0.5, (S, 3)).astype(np.float32)
    one = _lib.route_scratch(S, n, K, P, torch.device(DEV))
    _lib.mixture_route(one, logits=dev(logits), mu0=dev(mu0), lv0=dev(lv0), state=gw.make_state(seed, DEV, call))
    rows = _lib.route_scratch(S * T, n, K, P, torch.device(DEV))
    state = gw.make_state(seed, DEV, call)
    table = lambda t: dev(np.broadcast_to(np.repeat(t, T, axis=0), (K, S * T, 3)))      # every component: the shape's base
    _lib.mixture_route_sweep(rows, group=T, logits=dev(np.repeat(logits, T, axis=0)), mu0=table(mu0), lv0=table(lv0), state=state)
    assert state.cpu().tolist() == [seed, call + 1]                                       # one advance per call, whatever R
    for k in KEYS:
        got = rows[k].view(S, T, *rows[k].shape[1:])
        for t in range(T):
            assert torch.equal(got[:, t], one[k]), (k, t)


# ---- 4. the per-component FiLM launch ----------------------------------------------------------------------------------------------
_STACKS = {}


def film_stack(f, G, K=3):
    """K one-Triple decoders of width f (Cper = 3 couplings each): the concatenated FiLM packing and eps."""
    if (f, G) not in _STACKS:
        decs = [decoder_and_state(1, f, G, 900 + 10 * f + G + k)[0].to(DEV).eval() for k in range(K)]
        _STACKS[(f, G)] = gw.MixtureStack(decs)
    stack = _STACKS[(f, G)]
    return stack, stack.packed()[1], stack.engines[0].couplings[0]._eps_value


def check_film(f, G, B, K=3, Cper=3):
    stack, pf, eps = film_stack(f, G, K)
    assert stack.C == Cper
    gk = torch.randn(K, B, G, generator=torch.Generator().manual_seed(f + G + B)).to(DEV)
    # stride 0: gwtf_film_forward over the K * Cper couplings
    want = _lib.film_forward(gk[0], pf, K * Cper, f, eps)
    got = torch.empty_like(want)
    _lib.check(_lib.lib().gwtf_film_forward_k(gk[0].data_ptr(), pf.data_ptr(), got.data_ptr(), B, G, K, Cper, f, float(eps), 0,
                                              torch.cuda.current_stream().cuda_stream))
    assert torch.equal(got, want)
    # three tables: component k's slice is gwtf_film_forward on table k
    got = _lib.film_forward_k(gk, pf, Cper, f, eps)
    assert got.shape == want.shape
    for k in range(K):
        alone = _lib.film_forward(gk[k].contiguous(), pf, K * Cper, f, eps)
        assert torch.equal(got[:, k * Cper:(k + 1) * Cper], alone[:, k * Cper:(k + 1) * Cper]), k
    assert not torch.equal(got[:, Cper:], want[:, Cper:])                  # (the tables do differ)
    assert torch.equal(stack._film_k(gk)[1], got)


@pytest.mark.parametrize('G', [32, 128])
@pytest.mark.parametrize('f', [19, 33, 37, 64])
def test_film_per_component_equals_the_film_launch_bit_for_bit(f, G):
    for B in (15, 16, 17):                                                # below, at and above the kernel's 16-row tile
        check_film(f, G, B)


def test_film_per_component_on_a_grid_beyond_one_round():
    check_film(37, 32, 700)                                               # 9 x 2 x 44 workgroups > 768: the two-round instantiation


# ---- 5. interpolate_many -----------------------------------------------------------------------------------------------------------
def codes_and_draws(cfg, S, n, seed):
    gen = torch.Generator().manual_seed(seed)
    G = cfg['g_latent_space_size']
    a, b = torch.randn(S, G, generator=gen).to(DEV), torch.randn(S, G, generator=gen).to(DEV)
    rng = np.random.RandomState(seed)
    ex = {'words': bits(rng.randint(0, 2**32, (S, n), dtype=np.uint64).astype(np.uint32)),
          'normals': dev(rng.normal(0, 1, (S, 3, n)).astype(np.float32))}
    return a, b, ex


def step_codes(a, b, weights):
    w = torch.tensor(weights, dtype=torch.float32, device=DEV).view(1, -1, 1)
    return (1. - w) * a.unsqueeze(1) + w * b.unsqueeze(1)                 # (S, T, G)


@pytest.mark.parametrize('weights_type', ['learned_weights', 'global_weights'])
def test_interpolate_many_is_generate_many_at_the_ends_and_the_routed_stack_at_every_step(weights_type):
    m, cfg = model_of(weights_type)
    S, n, weights = 3, 300, (0.0, 0.3, 1.0)
    T = len(weights)
    a, b, ex = codes_and_draws(cfg, S, n, 41)
    state = gw.make_state(5, DEV, 2)
    x, labels = m.interpolate_many(a, b, n, weights=weights, return_labels=True, state=state, explicit=ex)
    assert x.shape == (S, T, 3, n) and labels.shape == (S, T, n) and labels.dtype == torch.float32
    assert state.cpu().tolist() == [5, 3]
    stack = m.mixture_stack()
    work = stack._routed_work(S * T, n, torch.device(DEV))
    lab, z0 = work['labels'].clone(), z0_of(work)
    assert torch.equal(labels.view(S * T, n), (lab + 1).float())
    assert torch.equal(m.interpolate_many(a, b, n, weights=weights, explicit=ex), x)
    # every step: the existing per-point path with the step's code, the sweep's base samples and labels
    codes = step_codes(a, b, weights)
    want, _ = stack.forward_routed(z0, codes.reshape(S * T, -1).contiguous(), lab)
    assert torch.equal(x.view(S * T, 3, n), want)
    # the ends: generate_many at codes_a and codes_b on the same draws
    for t, end in ((0, a), (2, b)):
        assert torch.equal(codes[:, t], end)
        g, gl = m.generate_many(end, n, return_labels=True, explicit=ex)
        assert torch.equal(labels[:, t], gl), t
        assert torch.equal(x[:, t], g), t
    if weights_type == 'global_weights':
        assert torch.equal(labels[:, 1], labels[:, 0])
    assert not torch.equal(x[:, 1], x[:, 0])


# ---- 6. one flow -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights_type', ['learned_weights', 'global_weights'])
@pytest.mark.parametrize('flow_idx', [(1,), (0, 2)])
def test_one_flow_sweeps_move_the_chosen_components_only(flow_idx, weights_type):
    m, cfg = model_of(weights_type, n_components=4)
    S, n, weights, K = 3, 300, (0.25, 0.5, 1.0), 4
    a, b, ex = codes_and_draws(cfg, S, n, 43)
    full, labels = m.interpolate_many(a, b, n, weights=weights, return_labels=True, explicit=ex)
    full, labels = full.clone(), labels.clone()
    one, labels_one = m.interpolate_many(a, b, n, weights=weights, flow_idx=set(flow_idx), return_labels=True, explicit=ex)
    assert torch.equal(labels_one, labels)                                # the logits come from the interpolated code in both
    if weights_type == 'global_weights':
        for t in range(1, len(weights)):
            assert torch.equal(labels[:, t], labels[:, 0])
    lab = labels.int() - 1
    assert all(int((lab == k).sum()) > 0 for k in range(K))
    moved = torch.zeros_like(lab, dtype=torch.bool)
    for k in flow_idx:
        moved |= lab == k
    sel = lambda x, mask: x.transpose(2, 3)[mask]                         # (S, T, 3, n) -> the (points, 3) of a mask over (S, T, n)
    assert torch.equal(sel(one, moved), sel(full, moved))
    assert not torch.equal(sel(one, ~moved), sel(full, ~moved))
    # the others: codes_a for the FiLM conditioning and for the base Gaussian, on the step's labels and the shared normals
    for t in range(len(weights)):
        stay = m.generate_many(a, n, explicit={'labels_in': lab[:, t].contiguous(), 'normals': ex['normals']})
        keep = ~moved[:, t]
        assert torch.equal(one[:, t].transpose(1, 2)[keep], stay.transpose(1, 2)[keep]), t


# ---- 7. float64 anchor: which code reaches which component ---------------------------------------------------------------------------
@pytest.mark.parametrize('flow_idx', [None, (1,)])
def test_a_sweep_against_the_float64_port_per_component_and_code(flow_idx):
    m, cfg = model_of('learned_weights')
    S, n, weights, K = 2, 128, (0.2, 0.5, 0.8), cfg['n_components']
    T = len(weights)
    a, b, ex = codes_and_draws(cfg, S, n, 47)
    x = m.interpolate_many(a, b, n, weights=weights, flow_idx=flow_idx, explicit=ex)
    work = m.mixture_stack()._routed_work(S * T, n, torch.device(DEV))
    lab, z0 = host(work['labels']).reshape(S, T, n), host(z0_of(work)).reshape(S, T, 3, n)
    codes, x = host(step_codes(a, b, weights)).astype(np.float64), host(x)
    states = [{k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in d.state_dict().items()}
              for d in m.pc_decoder]
    worst = 0.0
    for s in range(S):
        for t in range(T):
            for k in range(K):
                idx = np.nonzero(lab[s, t] == k)[0]
                if len(idx) == 0:
                    continue
                code = codes[s, t] if flow_idx is None or k in flow_idx else host(a)[s].astype(np.float64)
                want, _ = tp.decoder_fused(torch.from_numpy(z0[s, t][None][:, :, idx].astype(np.float64)), torch.from_numpy(code[None]),
                                           states[k], cfg['p_decoder_n_flows'], 'direct')
                worst = max(worst, maxabs(x[s, t][:, idx], want.numpy()[0]))
    print('sweep against the float64 port: max |x - x64| =', worst)
    assert worst < TOL_COORD, worst
    if flow_idx is not None:
        # the base Gaussian follows the same rule: p_prior of the row's code for the chosen components, of codes_a for the others
        rows = step_codes(a, b, weights).reshape(S * T, -1)
        eps = host(ex['normals'])
        for g, ks in ((rows, [k for k in range(K) if k in flow_idx]), (a.repeat_interleave(T, dim=0), [k for k in range(K) if k not in flow_idx])):
            mu0, lv0 = (host(v[:, :, 0]).reshape(S, T, 3) for v in m._base_gaussian(g.contiguous()))
            for k in ks:
                for s in range(S):
                    for t in range(T):
                        idx = np.nonzero(lab[s, t] == k)[0]
                        want = eps[s][:, idx] * np.exp(np.float32(0.5) * lv0[s, t])[:, None] + mu0[s, t][:, None]
                        if len(idx):
                            assert np.abs(z0[s, t][:, idx] - want).max() <= TOL_NORMAL, (k, s, t)


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flow_idx', [None, (0,)])
def test_a_captured_interpolate_many_draws_fresh_clouds_on_every_replay(flow_idx):
    m, cfg = model_of('learned_weights')
    S, n, seed, call, T = 2, 200, 9, 30, 9
    a, b, _ = codes_and_draws(cfg, S, n, 51)
    state = gw.make_state(seed, DEV, call)
    out = torch.empty(S, T, 3, n, device=DEV)
    m.interpolate_many(a, b, n, flow_idx=flow_idx, state=state, out=out)      # warm-up: scratch, constants and packed weights exist
    state.copy_(gw.make_state(seed, DEV, call))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a host synchronisation inside the call would fail the capture
        m.interpolate_many(a, b, n, flow_idx=flow_idx, state=state, out=out)
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append(out.clone())
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [seed, call + 2]
    assert not torch.equal(replays[0], replays[1])
    for i, rep in enumerate(replays):
        eager = m.interpolate_many(a, b, n, flow_idx=flow_idx, state=gw.make_state(seed, DEV, call + i))
        assert torch.equal(eager, rep), i
    # the draws are generate_many's for the same (seed, call): with one weight of 0 the sweep is generate_many(codes_a)
    x = m.interpolate_many(a, b, n, weights=[0.0], state=gw.make_state(seed, DEV, call))
    assert torch.equal(x[:, 0], m.generate_many(a, n, state=gw.make_state(seed, DEV, call)))


# ---- 9. upsample_many ----------------------------------------------------------------------------------------------------------------
def test_upsample_many_is_generate_many_on_the_posterior_means_in_every_mode():
    m, cfg = model_of('learned_weights')
    S, n_sparse, n = 3, 100, 256
    clouds = torch.randn(S, 3, n_sparse, generator=torch.Generator().manual_seed(3)).to(DEV)
    try:
        m.mode = 'autoencoding'
        with torch.no_grad():                                                 # (as the reference's evaluation runs: no autograd path)
            g = m.encode(clouds)['g_posterior_mus']
        want, want_labels = m.generate_many(g, n, return_labels=True, state=gw.make_state(11, DEV, 4))
        for mode in ('training', 'autoencoding', 'generating'):
            m.mode = mode
            state = gw.make_state(11, DEV, 4)
            x, labels = m.upsample_many(clouds, n, return_labels=True, state=state)
            assert x.shape == (S, 3, n) and torch.equal(x, want) and torch.equal(labels, want_labels), mode
            assert state.cpu().tolist() == [11, 5]
            assert labels.min() >= 1 and labels.max() <= cfg['n_components']
    finally:
        m.mode = 'generating'


# ---- 10. evaluation.interpolate_clouds / upsample_clouds ---------------------------------------------------------------------------
def two_batches(B=4, N=96):
    gen = torch.Generator().manual_seed(8)
    return [{'cloud': torch.randn(B, 3, N, generator=gen).to(DEV), 'eval_cloud': torch.randn(B, 3, N, generator=gen).to(DEV)}
            for _ in range(2)]


def test_interpolate_clouds_returns_the_layouts_of_the_reference_file():
    m, cfg = model_of('learned_weights')
    batches, n, B, N = two_batches(), 64, 4, 96
    gen = torch.Generator(device=DEV).manual_seed(5)
    res = gw.evaluation.interpolate_clouds(m, batches + batches, n, n_batches=2, state=gw.make_state(3, DEV), generator=gen)
    assert set(res) == {'clouds1', 'clouds2', 'interpolations', 'labels'}
    assert res['clouds1'].shape == res['clouds2'].shape == (2 * B, 3, N)
    assert res['interpolations'].shape == (2 * B, 3, n, 9) and res['interpolations'].dtype == torch.float32
    assert res['labels'].shape == (2 * B, n, 9) and res['labels'].dtype == torch.uint8
    assert all(v.is_contiguous() and v.device == torch.device(DEV) for v in res.values())
    assert res['labels'].min() >= 1 and res['labels'].max() <= cfg['n_components'] and torch.isfinite(res['interpolations']).all()
    gen = torch.Generator(device=DEV).manual_seed(5)
    for i, batch in enumerate(batches):
        assert torch.equal(res['clouds1'][i * B:(i + 1) * B], batch['cloud'])
        perm = torch.randperm(B, device=DEV, generator=gen)
        assert sorted(perm.tolist()) == list(range(B))
        assert torch.equal(res['clouds2'][i * B:(i + 1) * B], batch['eval_cloud'][perm])
    # step t of pair i is the model at the interpolated posterior means; layout (N, 3, n, T): the step is the LAST axis
    one = gw.evaluation.interpolate_clouds(m, batches, n, n_batches=1, weights=[0.5], flow_idx=[1], state=gw.make_state(3, DEV),
                                           generator=torch.Generator(device=DEV).manual_seed(5))
    assert one['interpolations'].shape == (B, 3, n, 1) and one['labels'].shape == (B, n, 1)
    with pytest.raises(gw.GwtfError):
        gw.evaluation.interpolate_clouds(m, [], n)
    with pytest.raises(gw.GwtfError):
        gw.evaluation.interpolate_clouds(m, [{'cloud': batches[0]['cloud'].cpu(), 'eval_cloud': batches[0]['eval_cloud']}], n)


def test_upsample_clouds_returns_the_layouts_of_the_reference_file():
    m, cfg = model_of('learned_weights')
    batches, sparse, n, B = two_batches(), 40, 128, 4
    res = gw.evaluation.upsample_clouds(m, batches, sparse, n, state=gw.make_state(4, DEV))
    assert set(res) == {'clouds_sparse', 'clouds_dense', 'labels'}
    assert res['clouds_sparse'].shape == (2 * B, 3, sparse) and res['clouds_dense'].shape == (2 * B, 3, n)
    assert res['labels'].shape == (2 * B, n) and res['labels'].dtype == torch.uint8 and res['clouds_dense'].dtype == torch.float32
    assert all(v.is_contiguous() and v.device == torch.device(DEV) for v in res.values())
    for i, batch in enumerate(batches):
        assert torch.equal(res['clouds_sparse'][i * B:(i + 1) * B], batch['cloud'][:, :, :sparse])
    want, labels = m.upsample_many(batches[0]['cloud'][:, :, :sparse].contiguous(), n, return_labels=True, state=gw.make_state(4, DEV))
    assert torch.equal(res['clouds_dense'][:B], want) and torch.equal(res['labels'][:B], labels.to(torch.uint8))
    assert gw.evaluation.upsample_clouds(m, batches, sparse, n, n_batches=1)['labels'].shape == (B, n)


# ---- 11. guards --------------------------------------------------------------------------------------------------------------------
def test_guards_refuse_before_anything_is_launched():
    m, cfg = model_of('learned_weights')
    S, n, K = 2, 100, cfg['n_components']
    a, b, ex = codes_and_draws(cfg, S, n, 8)
    state = gw.make_state(21, DEV, 6)
    ok = dict(codes_a=a, codes_b=b, n_points=n, state=state)
    for bad in (dict(codes_a=a.cpu()), dict(codes_b=b.cpu()), dict(codes_a=a.cpu(), codes_b=b.cpu()), dict(codes_b=b[:1]),
                dict(codes_b=b[:, :-1]), dict(weights=[]), dict(weights=torch.zeros(0, device=DEV)), dict(flow_idx=[K]),
                dict(flow_idx=[-1]), dict(explicit={'labels': ex['words']}), dict(out=torch.empty(S, 9, 3, n)),
                dict(out=torch.empty(S, 3, 9, n, device=DEV)), dict(out=torch.empty(S, 9, 3, n, device=DEV, dtype=torch.float64)),
                dict(explicit={'words': ex['words'][:1]}), dict(explicit={'normals': ex['normals'].double()}),
                dict(state=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(gw.GwtfError):
            m.interpolate_many(**dict(ok, **bad))
    with _lib.exact_fp32():
        with pytest.raises(gw.GwtfError):
            m.interpolate_many(**ok)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.interpolate_many(**ok)
    finally:
        m.eval()
    stack = m.mixture_stack()
    with pytest.raises(gw.GwtfError):
        stack._film_k(torch.zeros(K + 1, 4, cfg['g_latent_space_size'], device=DEV))
    work = _lib.route_scratch(6, n, K, 64, torch.device(DEV))
    for kw in (dict(group=0), dict(group=4), dict(group=3, mu0=torch.zeros(K + 1, 6, 3, device=DEV)),
               dict(group=3, words=ex['words'][:1])):
        args = dict(dict(logits=torch.zeros(6, K, device=DEV), mu0=torch.zeros(1, 3, device=DEV), lv0=torch.zeros(1, 3, device=DEV),
                         state=state), **kw)
        with pytest.raises(gw.GwtfError):
            _lib.mixture_route_sweep(work, **args)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [21, 6]                                # nothing was launched: the state has not advanced
    assert m.interpolate_many(**ok).shape == (S, 9, 3, n) and state.cpu().tolist() == [21, 7]
