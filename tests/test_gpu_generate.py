"""Device-resident generation on the GPU: the routing kernel (csrc/gwtf_route.hip) against its numpy restatement (generate_ref.py),
the routed stack launch against one decoder pass per point group, the genuine reference's recorded generation (golden g13), graph
capture, the guards, and evaluation.generate_clouds.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN, TOL_COORD
from helpers import decoder_and_state, maxabs
import generate_ref as gr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models
from go_with_the_flows_amd.synth import load_synth_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_NORMAL = 1e-4          # restated Box-Muller values against the device's (tests/test_gpu_clouds.py uses it for the same arithmetic)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(words):
    return dev(np.asarray(words, np.uint32).view(np.int32))


@pytest.fixture(scope='module')
def model():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating')
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    return m.to(DEV).eval(), cfg


_STACKS = {}


def small_stack(f, K=4, G=32):
    """K one-Triple decoders of width f (C = 3 couplings each) as a MixtureStack."""
    if f not in _STACKS:
        decs = [decoder_and_state(1, f, G, 700 + 10 * f + k)[0].to(DEV).eval() for k in range(K)]
        _STACKS[f] = (gw.MixtureStack(decs), decs, G)
    return _STACKS[f]


def check_layout(work, labels, K):
    """tile_comp / perm / labels of a routing call equal the restatement of `labels` exactly."""
    tile_comp, perm, _ = gr.layout(labels, K, work['P'])
    assert np.array_equal(host(work['labels']), labels)
    assert np.array_equal(host(work['tile_comp']), tile_comp)
    assert np.array_equal(host(work['perm']), perm)
    return perm


def check_zp(work, z0, perm, tol=0.0):
    """zp holds z0 in slot order (within tol) and exact zeros in the padding."""
    zp = host(work['zp'])
    for s in range(len(perm)):
        valid = perm[s] >= 0
        assert (zp[s][:, ~valid] == 0).all()
        err = np.abs(zp[s][:, valid] - z0[s][:, perm[s][valid]]).max()
        assert err <= tol, (s, err)


# ---- 5. the routing kernel alone, explicit draws -----------------------------------------------------------------------------------
@pytest.mark.parametrize('S,n,K,P', [(1, 1, 1, 64), (5, 300, 3, 64), (5, 300, 3, 256), (2, 2500, 64, 128)])
def test_routing_with_explicit_words_equals_the_restatement(S, n, K, P):
    rng = np.random.RandomState(100 + n + K + P)
    logits = rng.normal(0, 1.5, (S, K)).astype(np.float32)
    words = rng.randint(0, 2**32, (S, n), dtype=np.uint64).astype(np.uint32)
    words[0, :1] = 0
    words[-1, -1:] = 0xffffffff
    z0 = rng.normal(0, 1, (S, 3, n)).astype(np.float32)
    work = _lib.route_scratch(S, n, K, P, torch.device(DEV))
    _lib.mixture_route(work, logits=dev(logits), words=bits(words), z0_in=dev(z0))
    thr = host(work['thresholds']).view(np.uint32)
    want = gr.thresholds(logits)
    # one ulp of float64 times 2^32 is far below 1: the ceiling moves by at most one
    assert np.abs(thr.astype(np.int64) - want.astype(np.int64)).max() <= 1
    labels = gr.labels_of(thr, words)                                 # searchsorted on the DEVICE's thresholds
    assert labels.min() >= 0 and labels.max() <= K - 1
    perm = check_layout(work, labels, K)
    check_zp(work, z0, perm)


@pytest.mark.parametrize('P', [64, 128])
def test_routing_of_crafted_labels_sits_on_the_tile_edges(P):
    n, K = 300, 3
    labels = gr.crafted_labels(n, K, P)
    S = len(labels)
    z0 = np.random.RandomState(3).normal(0, 1, (S, 3, n)).astype(np.float32)
    work = _lib.route_scratch(S, n, K, P, torch.device(DEV))
    _lib.mixture_route(work, labels_in=dev(labels), z0_in=dev(z0))
    perm = check_layout(work, labels, K)
    check_zp(work, z0, perm)


# ---- 6. Philox mode ----------------------------------------------------------------------------------------------------------------
def test_philox_draws_equal_the_restatement_and_advance_the_state():
    S, n, K, P, seed, call = 3, 1000, 3, 128, 77, 5
    rng = np.random.RandomState(6)
    logits = rng.normal(0, 1, (S, K)).astype(np.float32)
    mu0, lv0 = rng.normal(0, 0.3, (S, 3)).astype(np.float32), rng.normal(-1, 0.5, (1, 3)).astype(np.float32)   # per shape / shared
    outs = []
    for _ in range(2):
        state = gw.make_state(seed, DEV, call)
        work = _lib.route_scratch(S, n, K, P, torch.device(DEV))
        _lib.mixture_route(work, logits=dev(logits), mu0=dev(mu0), lv0=dev(lv0), state=state)
        assert state.cpu().tolist() == [seed, call + 1]
        outs.append(work)
    for k in ('thresholds', 'tile_comp', 'perm', 'zp', 'labels'):
        assert torch.equal(outs[0][k], outs[1][k]), k                 # equal (seed, call): identical bits
    work = outs[0]
    labels = gr.labels_of(host(work['thresholds']).view(np.uint32), gr.label_words(seed, call, S, n))
    perm = check_layout(work, labels, K)
    z0 = gr.base_samples(gr.normal_draws(seed, call, S, n), mu0, lv0)
    check_zp(work, z0, perm, tol=TOL_NORMAL)


def test_philox_component_counts_follow_the_mixture_weights():
    n, logits = 20000, np.array([[0.0, 1.0, -1.0]], np.float32)
    work = _lib.route_scratch(1, n, 3, 256, torch.device(DEV))
    zero = torch.zeros(1, 3, device=DEV)
    _lib.mixture_route(work, logits=dev(logits), mu0=zero, lv0=zero, state=gw.make_state(gr.SEED, DEV))
    counts = np.bincount(host(work['labels'])[0], minlength=3)
    p = np.exp(logits[0].astype(np.float64))
    p /= p.sum()
    assert (np.abs(counts - n * p) < 5 * np.sqrt(n * p * (1 - p))).all(), counts
    z = host(work['zp'])[0][:, host(work['perm'])[0] >= 0]
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02               # standard normals (3 * 20000 values: sigma of the mean 0.004)


# ---- 7. forward_routed against one decoder pass per point group --------------------------------------------------------------------
def routed_inputs(S, n, K, G, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, K, (S, n)).astype(np.int32)
    labels[1] = 0                                                     # a shape whose points all fall into ONE component
    gen = torch.Generator().manual_seed(seed)
    return labels, torch.randn(S, 3, n, generator=gen).to(DEV), torch.randn(S, G, generator=gen).to(DEV)


def check_against_decoder_passes(stack, decoders, z0, g, labels, out, logdet):
    S, K = labels.shape[0], len(decoders)
    worst = 0.0
    with torch.no_grad():
        for s in range(S):
            for k in range(K):
                idx = np.nonzero(labels[s] == k)[0]
                if len(idx) == 0:
                    continue
                it = torch.from_numpy(idx).to(DEV)
                want = decoders[k](z0[s:s + 1][:, :, it].contiguous(), g[s:s + 1], mode='direct')[0][-1]
                worst = max(worst, maxabs(host(out[s:s + 1][:, :, it]), host(want)))
            order = np.argsort(labels[s], kind='stable')
            ot = torch.from_numpy(order).to(DEV)
            counts = [int((labels[s] == k).sum()) for k in range(K)]
            xp, ldp = stack.forward_partition(z0[s:s + 1][:, :, ot].contiguous(), g[s:s + 1], counts, mode='direct')
            worst_ld = maxabs(host(logdet[s:s + 1][:, :, ot]), host(ldp))
            assert worst_ld < TOL_COORD, (s, worst_ld)
            assert maxabs(host(out[s:s + 1][:, :, ot]), host(xp)) < TOL_COORD
    print('forward_routed: max |routed - decoder pass| =', worst)
    assert worst < TOL_COORD, worst


def test_forward_routed_equals_one_decoder_pass_per_point_group(model):
    m, cfg = model
    S, n, K = 5, 300, cfg['n_components']
    labels, z0, g = routed_inputs(S, n, K, cfg['g_latent_space_size'], 4)
    stack = m.mixture_stack()
    out, logdet = stack.forward_routed(z0, g, dev(labels))
    assert out.shape == (S, 3, n) and logdet.shape == (S, 3, n)
    check_against_decoder_passes(stack, list(m.pc_decoder), z0, g, labels, out, logdet)


@pytest.mark.parametrize('f', [19, 37, 64])
def test_forward_routed_at_every_body_width(f):
    stack, decs, G = small_stack(f)
    labels, z0, g = routed_inputs(5, 300, 4, G, f)
    out, logdet = stack.forward_routed(z0, g, dev(labels))
    check_against_decoder_passes(stack, decs, z0, g, labels, out, logdet)
    with _lib.tuning(generic_body=True):                              # the run-time-width body of the same width
        out_g, logdet_g = stack.forward_routed(z0, g, dev(labels))
    assert maxabs(host(out_g), host(out)) < TOL_COORD and maxabs(host(logdet_g), host(logdet)) < TOL_COORD


# ---- 8. tile independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', [19, 37, 64])
def test_forced_tiles_agree_and_every_point_is_written(f):
    stack, decs, G = small_stack(f)
    S, n = 5, 300
    labels, z0, g = routed_inputs(S, n, 4, G, 50 + f)
    res = {}
    for ppw in (16, 32, 64):
        with _lib.tuning(points_per_wave=ppw):
            work = stack._routed_work(S, n, torch.device(DEV))
            assert work['P'] == 4 * ppw
            _lib.mixture_route(work, labels_in=dev(labels), z0_in=z0)
            out = torch.full((S, 3, n), float('nan'), device=DEV)
            out, logdet = stack.launch_routed(work, g, out=out, want_logdet=True)
        assert torch.isfinite(out).all() and torch.isfinite(logdet).all()          # no entry of the (S, 3, n) result is left unwritten
        res[ppw] = (host(out), host(logdet))
    for ppw in (32, 64):
        assert maxabs(res[ppw][0], res[16][0]) < TOL_COORD and maxabs(res[ppw][1], res[16][1]) < TOL_COORD


# ---- 9. the genuine reference's recorded generation ----------------------------------------------------------------------------------
def test_generate_many_reproduces_the_recorded_reference_generation(model):
    D = golden('g13_full_model')
    m, cfg = model
    Ns = D['gen_samples'].shape[2]
    labels = (D['gen_labels'] - 1).astype(np.int32)                                   # (1, Ns) in [0, K)
    # the reference hands component k's j-th point gen_noise_p[:, :, j]: every component reads the FIRST c_k columns
    normals = D['gen_noise_p'][:, :, gr.ranks_within_component(labels[0])]
    x, got = m.generate_many(dev(D['gen_g']), Ns, return_labels=True,
                             explicit={'labels_in': dev(labels), 'normals': dev(normals.astype(np.float32))})
    assert np.array_equal(host(got), D['gen_labels'])
    err = maxabs(host(x), D['gen_samples'])
    print('generate_many against the reference: max |x - gen_samples| =', err)
    assert err < TOL_COORD


# ---- 10. graph capture ------------------------------------------------------------------------------------------------------------
def test_a_captured_generate_many_draws_fresh_clouds_on_every_replay(model):
    m, cfg = model
    S, n, seed, call = 4, 200, 9, 30
    g = torch.randn(S, cfg['g_latent_space_size'], generator=torch.Generator().manual_seed(1)).to(DEV)
    state = gw.make_state(seed, DEV, call)
    out = torch.empty(S, 3, n, device=DEV)
    m.generate_many(g, n, state=state, out=out)                      # warm-up: scratch and packed weights exist from here on
    state.copy_(gw.make_state(seed, DEV, call))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # a host synchronisation inside the call would fail the capture
        m.generate_many(g, n, state=state, out=out)
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append(out.clone())
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [seed, call + 2]
    assert not torch.equal(replays[0], replays[1])
    for i, rep in enumerate(replays):
        eager = m.generate_many(g, n, state=gw.make_state(seed, DEV, call + i))
        assert torch.equal(eager, rep), i


# ---- 11. guards --------------------------------------------------------------------------------------------------------------------
def test_guards(model):
    m, cfg = model
    S, n, K = 2, 100, cfg['n_components']
    labels, z0, g = routed_inputs(S, n, K, cfg['g_latent_space_size'], 8)
    stack = m.mixture_stack()
    lab = dev(labels)
    for bad in (lab.long(), lab.cpu(), lab[:, :-1].contiguous(), lab.float()):
        with pytest.raises(gw.GwtfError):
            stack.forward_routed(z0, g, bad)
    with _lib.exact_fp32():
        with pytest.raises(gw.GwtfError):
            stack.forward_routed(z0, g, lab)
        with pytest.raises(gw.GwtfError):
            m.generate_many(g, n)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            stack.forward_routed(z0, g, lab)
        with pytest.raises(NotImplementedError):
            m.generate_many(g, n)
    finally:
        m.eval()
    with pytest.raises(gw.GwtfError):
        m.generate_many(g, n, explicit={'labels': lab})
    # a base sample outside the f16-safe range comes back NaN, in that point only
    z_far = z0.clone()
    z_far[1, 0, 37] = 1e6
    x = host(m.generate_many(g, n, explicit={'labels_in': lab, 'z0_in': z_far}))
    nan = np.isnan(x)
    assert nan[1, :, 37].all() and nan.sum() == 3
    ok = host(m.generate_many(g, n, explicit={'labels_in': lab, 'z0_in': z0}))
    assert np.array_equal(x[~nan], ok[~nan])


# ---- 12. evaluation.generate_clouds ------------------------------------------------------------------------------------------------
def test_generate_clouds_fills_the_layout_the_metrics_take(model):
    m, cfg = model
    clouds = gw.evaluation.generate_clouds(m, 5, 64, batch_size=2, state=gw.make_state(3, DEV))
    assert clouds.shape == (5, 64, 3) and clouds.is_contiguous() and clouds.device == torch.device(DEV) and clouds.dtype == torch.float32
    assert torch.isfinite(clouds).all()
    assert not torch.equal(clouds[0], clouds[2])                                       # batches draw from an advancing state
    m.mode = 'training'
    try:
        with pytest.raises(gw.GwtfError):
            gw.evaluation.generate_clouds(m, 2, 16)
    finally:
        m.mode = 'generating'
