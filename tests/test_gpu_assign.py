"""Per-point component posteriors on the GPU: the assignment launch (csrc/gwtf_assign.hip) against its float64 restatement
(assign_ref.py), its edge values, determinism and accumulation rules, and Flow_Mixture_Model.assign_many /
Flow_Mixture_SVR_Model.assign_many / evaluation.segment_clouds on top.  Needs an MI355X.

Tolerances.  lp_k is about fifteen float32 operations on terms no larger than |lp|; per point delta = TOL_NLL_REL * max(1, max_k |lp_k|)
over the finite lp_k of the restatement.  log_density within delta, confidence and resp within 2 delta absolute, labels EQUAL wherever
the float64 margin between the best and the second-best lp is at least 2 delta; the points below that margin are exempt, and a case
may exempt at most 1 % of its points.  counts, invalid and the contingency table are exact against the kernel's own labels."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_NLL_REL, golden, record_parity
import assign_ref as ar
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models
from go_with_the_flows_amd.mixture import flow_mixture_nll
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('log_density', 'labels', 'confidence', 'resp', 'counts', 'invalid')
MAX_EXEMPT = 0.01


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def synthetic(K, B, N):
    """z ~ 1.5 N(0,1), logdet ~ 0.3 N, mu0 ~ 0.2 N, lv0 ~ 0.3 N, logits ~ N: float32 numpy in the order the launch takes them."""
    rng = np.random.default_rng(7)
    arrs = (1.5 * rng.normal(size=(K, B, 3, N)), 0.3 * rng.normal(size=(K, B, 3, N)), 0.2 * rng.normal(size=(K, B, 3)),
            0.3 * rng.normal(size=(K, B, 3)), rng.normal(size=(B, K)))
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrs)


_REF = {}


def reference(key, arrs):
    """The restatement's values for one input, computed once per key and shared (callers do not modify them)."""
    if key not in _REF:
        lp = ar.lp(*arrs)
        _REF[key] = {'lp': lp, 'log_density': ar.log_density(lp), 'labels': ar.labels(lp), 'resp': ar.resp(lp), 'margin': ar.margin(lp),
                     'delta': ar.delta(lp, TOL_NLL_REL)}
    return _REF[key]


def run(arrs, **kw):
    res = _lib.mixture_assign(*(dev(a) for a in arrs), **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else host(v) for k, v in res.items()}


def bits_equal(a, b):
    """torch.equal on the bit patterns (a NaN equals the same NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_class(got, want):
    """Non-finite values agree in kind: NaN with NaN, -inf with -inf, +inf with +inf."""
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and \
        np.array_equal(np.isneginf(got), np.isneginf(want))


def check(name, got, ref, K):
    """Every output of one call against the restatement, under the module's tolerances; the measured errors are recorded."""
    dens, delta, finite = ref['log_density'], ref['delta'], np.isfinite(ref['log_density'])
    assert same_class(got['log_density'], dens), name
    err_d = np.abs(got['log_density'].astype(np.float64) - dens)[finite]
    decided = (ref['margin'] >= 2 * delta) | ~finite
    exempt = 1.0 - decided.mean()
    lab = got['labels']
    assert lab.dtype == np.int32 and lab.min() >= -1 and lab.max() < K
    # the responsibility of the label the KERNEL chose, from the restatement (an exempt point may carry either of two near-equal ones)
    r_ref = ref['resp']
    conf_ref = np.where(lab >= 0, np.take_along_axis(r_ref, np.maximum(lab, 0)[:, None, :], axis=1)[:, 0], 0.0)
    conf_ref = np.where(finite, conf_ref, 0.0)
    err_c = np.abs(got['confidence'].astype(np.float64) - conf_ref)
    errs = dict(log_density=err_d.max() if err_d.size else 0.0, log_density_over_delta=(err_d / delta[finite]).max() if err_d.size else 0.0,
                confidence_over_2delta=(err_c / (2 * delta)).max(), exempt=exempt, mismatched_exempt=float((lab != ref['labels']).mean()))
    if got['resp'] is not None:
        assert np.isnan(got['resp'][np.broadcast_to(~finite[:, None, :], r_ref.shape)]).all(), name
        err_r = np.abs(got['resp'].astype(np.float64) - r_ref)
        err_r = np.where(np.broadcast_to(finite[:, None, :], r_ref.shape), err_r, 0.0)
        errs['resp_over_2delta'] = (err_r / (2 * delta)[:, None, :]).max()
        # the label's responsibility IS the confidence
        picked = np.take_along_axis(got['resp'], np.maximum(lab, 0)[:, None, :], axis=1)[:, 0]
        assert np.array_equal(picked[lab >= 0], got['confidence'][lab >= 0]), name
    record_parity('assign/' + name, **errs)
    assert (err_d <= delta[finite]).all(), (name, errs)
    assert exempt <= MAX_EXEMPT, (name, errs)
    assert np.array_equal(lab[decided], ref['labels'][decided]), (name, errs)
    assert (err_c <= 2 * delta).all(), (name, errs)
    if got['resp'] is not None:
        assert errs['resp_over_2delta'] <= 1.0, (name, errs)
    counts, invalid = ar.counts(lab, K)
    assert got['counts'].dtype == np.int32 and np.array_equal(got['counts'], counts), name
    assert np.array_equal(got['invalid'], invalid) and np.array_equal(invalid, (~finite).sum(1)), name


# ---- 1. the kernel in isolation ------------------------------------------------------------------------------------------------------
# (1, 1), (3, 63), (3, 777), (2, 2049): the float-by-float path -- one point, less than a wave, two workgroups per shape with a ragged
# last one, five with one point in the last.  (3, 776), (2, 2052): the same on the 16-byte path, which needs N % 4 == 0
@pytest.mark.parametrize('B,N', [(1, 1), (3, 63), (3, 777), (2, 2049), (3, 776), (2, 2052)])
@pytest.mark.parametrize('K', [1, 2, 4, 16, 64])
def test_assignment_against_the_restatement(K, B, N):
    arrs = synthetic(K, B, N)
    ref = reference((K, B, N), arrs)
    got = run(arrs, want_resp=True)
    check(f'K{K}-B{B}-N{N}', got, ref, K)
    if K == 1:
        assert (got['labels'] == 0).all() and (got['confidence'] == 1).all() and (got['resp'] == 1).all()
        lean = run(arrs, want_confidence=False)
        assert lean['confidence'] is None and lean['resp'] is None
    else:
        lean = run(arrs)                                                      # without resp: the one-pass form, the same bits
    for k in ('log_density', 'labels', 'counts', 'invalid'):
        assert np.array_equal(lean[k], got[k]), k


@pytest.mark.parametrize('K', [1, 4])
def test_log_density_is_the_point_lse_of_the_density_path(K):
    arrs = synthetic(K, 3, 777)
    got = run(arrs)
    if K == 1:
        # log w = 0 for the only component, in float32 as well: log_density = lp_0 to the rounding of lp's own fifteen operations
        lp0 = ar.lp(*arrs)[0]
        assert np.abs(got['log_density'] - lp0).max() <= TOL_NLL_REL * np.abs(lp0).max()
    nll, plse = _lib.mixture_nll(*(dev(a) for a in arrs), want_point_lse=True)
    assert np.array_equal(host(plse), got['log_density'])                     # the same expression in the same order: bit for bit


def test_golden_inputs():
    d = golden('g5_losses')
    arrs = tuple(np.ascontiguousarray(d[k], dtype=np.float32) for k in ('z', 'logdet', 'mu0', 'lv0', 'logits'))
    ref = reference('g5', arrs)
    assert (ref['margin'] >= 2 * ref['delta']).all()                          # smallest margin 7.3e-3: no point is exempt
    got = run(arrs, want_resp=True)
    check('g5', got, ref, arrs[0].shape[0])
    assert np.array_equal(got['labels'], ref['labels'])
    nll = -got['log_density'].astype(np.float64).sum(1).mean()
    assert abs(nll - float(d['mixture_nll'])) <= TOL_NLL_REL * abs(float(d['mixture_nll']))


# ---- 2. edge values -------------------------------------------------------------------------------------------------------------------
def test_a_component_whose_weight_underflows_is_never_chosen():
    K, B, N = 4, 3, 777
    z, ld, mu0, lv0, logits = synthetic(K, B, N)
    logits = logits.copy()
    logits[:, 1] = -200.0
    arrs = (z, ld, mu0, lv0, logits)
    ref = reference('c1_m200', arrs)
    assert np.isneginf(ref['lp'][1]).all()
    got = run(arrs, want_resp=True)
    check('c1_m200', got, ref, K)
    assert (got['labels'] != 1).all() and (got['counts'][:, 1] == 0).all() and (got['resp'][:, 1] == 0).all()
    assert not got['invalid'].any()


def test_a_shape_with_every_weight_underflown_is_invalid():
    K, B, N = 4, 3, 777
    z, ld, mu0, lv0, logits = synthetic(K, B, N)
    logits = logits.copy()
    logits[1] = -200.0
    arrs = (z, ld, mu0, lv0, logits)
    got = run(arrs, want_resp=True)
    check('shape1_m200', got, reference('shape1_m200', arrs), K)
    assert np.isneginf(got['log_density'][1]).all() and (got['labels'][1] == -1).all() and (got['confidence'][1] == 0).all()
    assert np.isnan(got['resp'][1]).all() and got['invalid'].tolist() == [0, N, 0] and (got['counts'][1] == 0).all()
    clean = run(synthetic(K, B, N), want_resp=True)
    for k in ('log_density', 'labels', 'confidence', 'resp', 'counts'):
        assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]), k


@pytest.mark.parametrize('N', [777, 776])                                     # float by float, and the 16-byte path
@pytest.mark.parametrize('nan_k', [0, 2])
def test_a_nan_invalidates_its_point_alone(N, nan_k):
    K, B = 4, 3
    arrs = synthetic(K, B, N)
    clean = run(arrs, want_resp=True)
    z = arrs[0].copy()
    z[nan_k, 1, 2, 601] = np.nan
    dirty = run((z,) + arrs[1:], want_resp=True)
    assert dirty['labels'][1, 601] == -1 and np.isnan(dirty['log_density'][1, 601]) and dirty['confidence'][1, 601] == 0
    assert np.isnan(dirty['resp'][1, :, 601]).all() and dirty['invalid'].tolist() == [0, 1, 0]
    keep = np.ones((B, N), bool)
    keep[1, 601] = False
    for k in ('log_density', 'labels', 'confidence'):
        assert np.array_equal(dirty[k][keep], clean[k][keep]), k               # bit for bit
    assert np.array_equal(dirty['resp'].transpose(0, 2, 1)[keep], clean['resp'].transpose(0, 2, 1)[keep])
    want = clean['counts'].copy()
    want[1, clean['labels'][1, 601]] -= 1
    assert np.array_equal(dirty['counts'], want)


def test_an_exact_tie_goes_to_the_lower_component():
    B, N = 3, 777
    z, ld, mu0, lv0, logits = synthetic(2, B, N)
    twin = lambda a: np.ascontiguousarray(np.stack([a[1], a[0], a[0], a[1], a[0]]))       # components 1, 2, 4 are one and the same
    lg = np.ascontiguousarray(np.stack([logits[:, 1], logits[:, 0], logits[:, 0], logits[:, 1], logits[:, 0]], axis=1))
    got = run((twin(z), twin(ld), twin(mu0), twin(lv0), lg), want_resp=True)
    assert not np.isin(got['labels'], (2, 3, 4)).any() and (got['labels'] == 1).any() and (got['labels'] == 0).any()
    assert np.array_equal(got['resp'][:, 1], got['resp'][:, 2]) and np.array_equal(got['resp'][:, 1], got['resp'][:, 4])
    assert np.array_equal(got['resp'][:, 0], got['resp'][:, 3])
    assert (got['counts'][:, 2:] == 0).all() and got['counts'].sum() == B * N


def test_an_unaligned_tensor_takes_the_other_path_to_the_same_bits():
    K, B, N = 4, 3, 776
    arrs = synthetic(K, B, N)
    on = [dev(a) for a in arrs]
    aligned = _lib.mixture_assign(*on, want_resp=True)
    assert all(t.data_ptr() % 16 == 0 for t in on[:2])
    store = torch.empty(on[0].numel() + 1, device=DEV)
    z_off = store[1:].view(K, B, 3, N)
    z_off.copy_(on[0])
    assert z_off.data_ptr() % 16 == 4 and z_off.is_contiguous()
    shifted = _lib.mixture_assign(z_off, *on[1:], want_resp=True)
    for k in KEYS:
        assert torch.equal(aligned[k], shifted[k]), k


# ---- 3. determinism and accumulation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [777, 776])
def test_two_calls_give_the_same_bits_and_the_table_accumulates(N):
    K, B, P = 4, 3, 5
    arrs = synthetic(K, B, N)
    on = [dev(a) for a in arrs]
    parts_np = np.random.default_rng(11).integers(-1, P + 2, size=(B, N)).astype(np.int32)       # -1, P and P + 1: outside [0, P)
    parts = dev(parts_np)
    first = _lib.mixture_assign(*on, want_resp=True, parts=parts, n_parts=P)
    one = {k: v.clone() for k, v in first.items()}
    second = _lib.mixture_assign(*on, want_resp=True, parts=parts, n_parts=P, table=first['table'], skipped=first['skipped'], out=first)
    assert all(second[k] is first[k] for k in KEYS) and second['table'] is first['table']
    for k in KEYS:
        assert torch.equal(second[k], one[k]), k                               # the same bits; counts and invalid are not doubled
    assert torch.equal(second['table'], 2 * one['table']) and torch.equal(second['skipped'], 2 * one['skipped'])
    assert one['table'].dtype == torch.int64 and one['skipped'].dtype == torch.int64
    table, skipped = ar.contingency(host(one['labels']), parts_np, K, P)
    assert np.array_equal(host(one['table']), table) and int(one['skipped']) == skipped
    outside = int(((parts_np < 0) | (parts_np >= P)).sum())
    assert skipped == outside > 0 and table.sum() == B * N - outside
    # an invalid point is left out of the table as well
    z = arrs[0].copy()
    z[0, 2, 0, 5] = np.nan
    parts_np[2, 5] = 0
    res = _lib.mixture_assign(dev(z), *on[1:], parts=dev(parts_np), n_parts=P)
    t2, s2 = ar.contingency(host(res['labels']), parts_np, K, P)
    assert host(res['labels'])[2, 5] == -1 and np.array_equal(host(res['table']), t2) and int(res['skipped']) == s2
    with pytest.raises(gw.GwtfError):
        _lib.mixture_assign(*on, parts=parts)                                  # no n_parts
    with pytest.raises(gw.GwtfError):
        _lib.mixture_assign(*on, parts=parts, n_parts=65)
    with pytest.raises(gw.GwtfError):
        _lib.mixture_assign(*on, out={'log_density': one['log_density']})      # an incomplete out


def test_the_widest_table():
    K, B, N, P = 64, 2, 2052, 64
    arrs = synthetic(K, B, N)
    parts_np = np.random.default_rng(12).integers(0, P, size=(B, N)).astype(np.int32)
    res = _lib.mixture_assign(*(dev(a) for a in arrs), parts=dev(parts_np), n_parts=P)
    table, skipped = ar.contingency(host(res['labels']), parts_np, K, P)
    assert np.array_equal(host(res['table']), table) and skipped == 0 == int(res['skipped'])


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(weights_type):
    if weights_type not in _MODELS:
        cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating', weights_type=weights_type,
                   n_components=3)
        m = models.Flow_Mixture_Model(**cfg)
        load_synth_(m, 1310)
        _MODELS[weights_type] = (m.to(DEV).eval(), cfg)
    return _MODELS[weights_type]


def clouds_of(B, N, seed):
    return torch.randn(B, 3, N, generator=torch.Generator().manual_seed(seed)).to(DEV)


def posterior_means(m, clouds):
    with torch.no_grad():
        return m.g_posterior(m._pooled_features(clouds))[0]


@pytest.mark.parametrize('N', [96, 130])
@pytest.mark.parametrize('weights_type', ['global_weights', 'learned_weights'])
def test_assign_many_against_the_density_path_and_the_restatement(weights_type, N):
    m, cfg = model_of(weights_type)
    B, K, P = 4, 3, cfg['p_latent_space_size']
    clouds = clouds_of(B, N, 21)
    codes = posterior_means(m, clouds_of(B, N, 22))                            # codes of OTHER clouds: held-out points
    res = m.assign_many(clouds, codes=codes, want_resp=True)
    with torch.no_grad():
        logits = m.get_weights(codes).contiguous().float()
        mu, lv = m._base_gaussian(codes)
        mu0 = mu.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P).contiguous()
        lv0 = lv.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P).contiguous()
        z, logdet = m.mixture_stack().forward_all(clouds, codes, mode='inverse')
        _, nll, plse = flow_mixture_nll(z, logdet, mu0, lv0, logits, want_point_lse=True)
    arrs = tuple(host(t) for t in (z, logdet, mu0, lv0, logits))
    ref = reference(('model', weights_type, N), arrs)
    got = {k: host(res[k]) for k in KEYS}
    assert got['labels'].shape == (B, N) and got['resp'].shape == (B, K, N) and got['counts'].shape == (B, K)
    assert np.isfinite(got['log_density']).all()
    err = np.abs(got['log_density'].astype(np.float64) - host(plse))
    rel = np.abs(-got['log_density'].astype(np.float64).sum(1) - host(nll)) / np.abs(host(nll))
    record_parity(f'assign/model-{weights_type}-N{N}', point_lse_over_delta=(err / ref['delta']).max(), nll_rel=rel.max())
    assert (err <= ref['delta']).all() and (rel <= 3 * TOL_NLL_REL).all()
    check(f'model-{weights_type}-N{N}/restatement', got, ref, K)               # fed the HIP z and logdet
    assert res['labels'].dtype == torch.int32 and res['labels'].is_contiguous()


def test_default_codes_are_the_posterior_means_in_every_mode():
    m, cfg = model_of('learned_weights')
    clouds = clouds_of(4, 96, 23)
    want = m.assign_many(clouds, codes=posterior_means(m, clouds), want_resp=True)
    try:
        for mode in ('training', 'autoencoding', 'generating'):
            m.mode = mode
            got = m.assign_many(clouds, want_resp=True)
            for k in KEYS:
                assert torch.equal(got[k], want[k]), (mode, k)
    finally:
        m.mode = 'generating'


def test_a_captured_assign_many_follows_its_input():
    m, cfg = model_of('learned_weights')
    B, N = 4, 130
    clouds, other = clouds_of(B, N, 24), clouds_of(B, N, 25)
    out = m.assign_many(clouds)                                                # warm-up: packed weights and the output tensors exist
    m.assign_many(clouds, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                              # a host synchronisation inside the call would fail the capture
        captured = m.assign_many(clouds, out=out)
    assert all(captured[k] is out[k] for k in KEYS if out[k] is not None)
    for src in (clouds.clone(), other):
        clouds.copy_(src)                                                      # the input is overwritten in place
        graph.replay()
        replayed = {k: v.clone() for k, v in out.items() if v is not None}
        torch.cuda.synchronize()
        eager = m.assign_many(src)
        for k, v in replayed.items():
            assert torch.equal(v, eager[k]), k
    assert not torch.equal(replayed['labels'], m.assign_many(clouds_of(B, N, 24))['labels'])


def test_guards_refuse_bad_arguments():
    m, cfg = model_of('learned_weights')
    clouds = clouds_of(4, 96, 26)
    codes = posterior_means(m, clouds)
    for bad in (dict(clouds=clouds.cpu()), dict(codes=codes.cpu()), dict(codes=codes[:2]), dict(codes=codes[:, :-1]),
                dict(clouds=clouds.transpose(1, 2).contiguous()), dict(parts=torch.zeros(4, 96, dtype=torch.int32, device=DEV)),
                dict(parts=torch.zeros(4, 96, dtype=torch.int64, device=DEV), n_parts=3),
                dict(parts=torch.zeros(4, 95, dtype=torch.int32, device=DEV), n_parts=3),
                dict(parts=torch.zeros(4, 96, dtype=torch.int32, device=DEV), n_parts=3, table=torch.zeros(3, 4, dtype=torch.int64, device=DEV))):
        with pytest.raises(gw.GwtfError):
            m.assign_many(**dict(dict(clouds=clouds, codes=codes), **bad))
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.assign_many(clouds, codes=codes)
        with pytest.raises(NotImplementedError):
            m.assign_many(clouds)
    finally:
        m.eval()
    assert m.assign_many(clouds, codes=codes)['labels'].shape == (4, 96)


def test_svr_model_labels_with_the_codes_of_its_images():
    D = golden('g21_svr')
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], util_mode='reconstruction')
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    m = m.to(DEV).eval()
    images = dev(np.asarray(synth_images(4, 64, 64, 2123), np.float32))
    clouds = clouds_of(4, 96, 27)
    with torch.no_grad():
        mus, _ = m.g0_prior(m.img_encoder(images))
        codes = m.g_prior(mus, mode='direct')[0][-1]                           # what reconstruct_many decodes from
    got, want = m.assign_many(clouds, images=images, want_resp=True), m.assign_many(clouds, codes=codes, want_resp=True)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got['labels'].min() >= 0 and got['labels'].max() < cfg['n_components'] and int(got['counts'].sum()) == 4 * 96
    for bad in (dict(), dict(images=images, codes=codes), dict(images=images.cpu())):
        with pytest.raises(gw.GwtfError):
            m.assign_many(clouds, **bad)


# ---- 5. evaluation ---------------------------------------------------------------------------------------------------------------------
def test_segment_clouds_layouts_labels_and_table():
    m, cfg = model_of('learned_weights')
    B, N, K, P = 4, 96, 3, 4
    gen = torch.Generator().manual_seed(8)
    batches = [{'cloud': torch.randn(B, 3, N, generator=gen).to(DEV), 'eval_cloud': torch.randn(B, 3, N, generator=gen).to(DEV),
                'part': torch.randint(-1, P + 1, (B, N), generator=gen).to(DEV)} for _ in range(2)]
    batches[0]['eval_cloud'][2, 1, 7] = float('nan')                           # one invalid point
    res = gw.evaluation.segment_clouds(m, batches, parts_key='part', n_parts=P, want_resp=True)
    assert set(res) == {'clouds', 'labels', 'log_density', 'confidence', 'counts', 'resp', 'table', 'skipped'}
    assert res['clouds'].shape == (2 * B, 3, N) and res['labels'].shape == (2 * B, N) and res['labels'].dtype == torch.uint8
    assert res['log_density'].shape == res['confidence'].shape == (2 * B, N) and res['log_density'].dtype == torch.float32
    assert res['counts'].shape == (2 * B, K) and res['resp'].shape == (2 * B, K, N)
    assert res['table'].shape == (K, P) and res['table'].dtype == torch.int64 and res['skipped'].dtype == torch.int64
    assert all(v.is_contiguous() and v.device == torch.device(DEV) for v in res.values())
    total, skipped = np.zeros((K, P), np.int64), 0
    for i, batch in enumerate(batches):
        rows = slice(i * B, (i + 1) * B)
        one = m.assign_many(batch['eval_cloud'], codes=posterior_means(m, batch['cloud']), parts=batch['part'].to(torch.int32), n_parts=P)
        assert torch.equal(res['labels'][rows], (one['labels'] + 1).to(torch.uint8))          # label + 1, 0 for an invalid point
        assert bits_equal(res['log_density'][rows], one['log_density']) and bits_equal(res['clouds'][rows], batch['eval_cloud'])
        assert torch.equal(res['confidence'][rows], one['confidence']) and torch.equal(res['counts'][rows], one['counts'])
        t, s = ar.contingency(host(one['labels']), host(batch['part']), K, P)
        assert np.array_equal(host(one['table']), t) and int(one['skipped']) == s
        total, skipped = total + t, skipped + s
    assert res['labels'][2, 7] == 0 and int((res['labels'] == 0).sum()) == 1 and res['labels'].max() <= K
    assert np.array_equal(host(res['table']), total) and int(res['skipped']) == skipped > 0
    got, want = gw.evaluation.part_agreement(res['table']), ar.part_agreement(total)
    assert all(abs(got[k] - want[k]) < 1e-12 for k in ('purity', 'nmi', 'miou')) and list(got['mapping']) == want['mapping']
    lean = gw.evaluation.segment_clouds(m, batches, n_batches=1)
    assert set(lean) == {'clouds', 'labels', 'log_density', 'confidence', 'counts'} and lean['labels'].shape == (B, N)
    with pytest.raises(gw.GwtfError):
        gw.evaluation.segment_clouds(m, [])
    with pytest.raises(gw.GwtfError):
        gw.evaluation.segment_clouds(m, [dict(batches[0], part=batches[0]['part'].float())], parts_key='part', n_parts=P)
