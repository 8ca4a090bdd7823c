"""Paired evaluation on the GPU (csrc/gwtf_metrics.hip: the frame, the paired Chamfer reduction, the finalising launch) against
recon_ref (the reference's statements in torch, its per-batch loop on the library's existing functions), nn_distance and golden g14;
autoencode_many, evaluate_autoencoding and evaluate_reconstruction.  Needs an MI355X."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
import recon_ref
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import metrics, models
from go_with_the_flows_amd import evaluation as ev
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24                       # unit roundoff of float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def uniform(shape, seed, lo=-0.5, hi=0.5):
    return np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the frame -----------------------------------------------------------------------------------------------------------------------
SHIFT = [0.1, -0.2, 0.3]
BASE = dict(cloud_scale=True, cloud_scale_scale=0.7, cloud_translate=True, cloud_translate_shift=SHIFT, cloud_rescale2orig=False,
            cloud_recenter2orig=False)
FRAMES = {'off': dict(BASE), 'unit': dict(BASE, unit_scale_evaluation=True), 'orig': dict(BASE, orig_scale_evaluation=True),
          'both': dict(BASE, unit_scale_evaluation=True, orig_scale_evaluation=True),
          'translate_no_scale': dict(BASE, orig_scale_evaluation=True, cloud_scale=False),
          'scale_kept_rows': dict(BASE, orig_scale_evaluation=True, cloud_rescale2orig=True, cloud_recenter2orig=True)}


def off_boundary(values, shift_floats):
    """A contiguous device copy of ``values`` that starts ``shift_floats`` floats behind a 16-byte boundary, NaN all around it."""
    flat = torch.full((values.size + 8,), float('nan'), device=DEV)
    off = (shift_floats - flat.data_ptr() // 4) % 4 + 4
    view = flat[off:off + values.size].view(values.shape)
    view.copy_(dev(values))
    assert view.is_contiguous() and (view.data_ptr() % 16) // 4 == shift_floats
    return view


@pytest.mark.parametrize('n,m', [(1, 1), (67, 48), (257, 1025)])
@pytest.mark.parametrize('name', list(FRAMES))
def test_frame_is_the_reference_statements_bit_for_bit(name, n, m):
    cfg, B = FRAMES[name], 3
    gen, ref = off_boundary(uniform((B, 3, n), 100 + n), 1), off_boundary(uniform((B, 3, m), 200 + m), 3)
    batch = {'orig_s': dev(uniform((B,), 7, 0.5, 2.0)), 'orig_c': dev(uniform((B, 3), 8, -1.0, 1.0))}
    gen0, ref0 = gen.clone(), ref.clone()
    want_r, want_p = recon_ref.to_eval_frame(gen, ref, batch, **cfg)
    got_r, got_p = metrics.clouds_to_eval_frame(gen, ref, metrics.EvalFrame.from_config(**cfg), **batch)
    assert got_r.shape == (B, n, 3) and got_p.shape == (B, m, 3) and got_r.is_contiguous() and got_p.is_contiguous()
    assert torch.equal(bits(got_r), bits(want_r.transpose(1, 2)))
    assert torch.equal(bits(got_p), bits(want_p.transpose(1, 2)))
    assert torch.equal(bits(gen), bits(gen0)) and torch.equal(bits(ref), bits(ref0))                 # the inputs are left alone
    if cfg.get('orig_scale_evaluation') and (n, m) == (257, 1025):
        # the test has teeth: with the shift rounded to float32 first the reference itself gives other bits
        f32_r, f32_p = recon_ref.to_eval_frame(gen, ref, batch, float32_shift=True, **cfg)
        assert not torch.equal(bits(f32_r), bits(want_r)) and not torch.equal(bits(f32_p), bits(want_p))


def test_identity_frame_is_a_layout_change_and_nan_passes_through():
    B, n, m = 3, 67, 48
    g, r = uniform((B, 3, n), 1), uniform((B, 3, m), 2)
    g[1, 2, 5], g[0, 0, 0], r[2, 1, 47] = np.nan, np.inf, -np.inf
    gen, ref = dev(g), dev(r)
    out = (torch.empty(B, n, 3, device=DEV), torch.empty(B, m, 3, device=DEV))
    got = metrics.clouds_to_eval_frame(gen, ref, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(bits(out[0]), bits(gen.transpose(1, 2))) and torch.equal(bits(out[1]), bits(ref.transpose(1, 2)))
    cfg = FRAMES['both']
    batch = {'orig_s': dev(uniform((B,), 7, 0.5, 2.0)), 'orig_c': dev(uniform((B, 3), 8, -1.0, 1.0))}
    want_r, want_p = recon_ref.to_eval_frame(gen, ref, batch, **cfg)
    got_r, got_p = metrics.clouds_to_eval_frame(gen, ref, metrics.EvalFrame.from_config(**cfg), **batch)
    for got_t, want_t in ((got_r, want_r.transpose(1, 2)), (got_p, want_p.transpose(1, 2))):
        assert torch.equal(torch.isnan(got_t), torch.isnan(want_t))
        assert torch.equal(bits(torch.nan_to_num(got_t, nan=0.0)), bits(torch.nan_to_num(want_t.contiguous(), nan=0.0)))
    assert torch.isnan(got_r[1, 5, 2]) and int(torch.isnan(got_r).sum()) == 1 and torch.isinf(got_r[0, 0, 0]) and torch.isinf(got_p[2, 47, 1])


def test_frame_guards():
    B, n = 2, 16
    gen, ref = dev(uniform((B, 3, n), 1)), dev(uniform((B, 3, n), 2))
    s, c = dev(uniform((B,), 3, 0.5, 2.0)), dev(uniform((B, 3), 4))
    orig = metrics.EvalFrame(row_scale=True, row_shift=True)
    for bad in (dict(), dict(orig_s=s), dict(orig_c=c), dict(orig_s=s.double(), orig_c=c), dict(orig_s=s.cpu(), orig_c=c),
                dict(orig_s=s, orig_c=c[:, :2].contiguous()), dict(orig_s=s[:1], orig_c=c)):
        with pytest.raises(gw.GwtfError):
            metrics.clouds_to_eval_frame(gen, ref, orig, **bad)
    for a, b in ((gen.transpose(1, 2), ref), (gen, ref[:1]), (gen.double(), ref), (gen.transpose(1, 2).contiguous().transpose(1, 2), ref)):
        with pytest.raises(gw.GwtfError):
            metrics.clouds_to_eval_frame(a, b)
    with pytest.raises(gw.GwtfError):
        metrics.clouds_to_eval_frame(gen, ref, out=(torch.empty(B, n, 3, device=DEV), torch.empty(B, 3, n, device=DEV)))
    with pytest.raises(gw.GwtfError):
        metrics.clouds_to_eval_frame(gen, ref, frame={'n_scale': 1})


# ---- the paired Chamfer reduction ----------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (67, 48), (256, 256), (257, 1025), (2049, 1030)]       # the edges of a thread's points, the chunk and the LDS tile


@functools.lru_cache(maxsize=None)
def chamfer_case(B, n, m):
    """Clouds and nn_distance's minima for one (B, n, m), computed once: the reference of every threshold count of that size."""
    a, b = dev(uniform((B, n, 3), 1000 + n + B)), dev(uniform((B, m, 3), 2000 + m + B))
    dl, dr = metrics.nn_distance(a, b)
    # nine thresholds strictly inside the range BOTH directions' minima cover: each direction has a minimum below and one above every
    # threshold, so no count is 0 or n (when there is more than one point)
    lo, hi = max(dl.min().item(), dr.min().item()), min(dl.max().item(), dr.max().item())
    thr = tuple(lo + (hi - lo) * q for q in np.linspace(0.15, 0.85, 9))
    return a, b, dl, dr, thr


@pytest.mark.parametrize('T', [0, 1, 8, 9])
@pytest.mark.parametrize('n,m', SIZES)
@pytest.mark.parametrize('B', [1, 3])
def test_chamfer_paired_against_nn_distance(B, n, m, T):
    a, b, dl, dr, thr9 = chamfer_case(B, n, m)
    thr = thr9[:T]
    sl, sr, cl, cr = metrics.chamfer_paired(a, b, thr)
    assert sl.shape == sr.shape == (B,) and cl.shape == cr.shape == (T, B) and cl.dtype == cr.dtype == torch.int32
    for got, d, cnt in ((sl, dl, n), (sr, dr, m)):
        want = d.double().sum(1)
        err = ((got.double() - want).abs() / want.clamp(min=1e-300)).max().item()
        print(f'B={B} n={n} m={m}: relative error of the sum {err:.3e}, bound {(cnt - 1) * U:.3e}')
        assert err <= (cnt - 1) * U
    for h, t in enumerate(thr):
        t32 = torch.tensor(t, dtype=torch.float32, device=DEV)
        want_l, want_r = (dl < t32).sum(1).int(), (dr < t32).sum(1).int()
        assert torch.equal(cl[h], want_l) and torch.equal(cr[h], want_r), (h, t)
        if min(n, m) > 1:
            assert 0 < int(want_l.sum()) < B * n and 0 < int(want_r.sum()) < B * m            # the threshold separates something
    again = metrics.chamfer_paired(a, b, thr)
    for x, y in zip((sl, sr, cl, cr), again):
        assert torch.equal(bits(x), bits(y))


def test_chamfer_paired_takes_both_chunk_lengths():
    """B = 128 pairs of 600 points fill the device with 2048-point chunks, B = 3 does not and takes 512-point ones: the same pairs give
    the same counts and sums within the bound either way."""
    n, m, thr = 600, 1100, (0.0005, 0.002)
    a, b = dev(uniform((128, n, 3), 31)), dev(uniform((128, m, 3), 32))
    dl, dr = metrics.nn_distance(a, b)
    big, small = metrics.chamfer_paired(a, b, thr), metrics.chamfer_paired(a[:3].contiguous(), b[:3].contiguous(), thr)
    for got, B in ((big, 128), (small, 3)):
        for s, d, cnt in ((got[0], dl[:B], n), (got[1], dr[:B], m)):
            want = d.double().sum(1)
            assert (((s.double() - want).abs() / want).max().item()) <= (cnt - 1) * U
        for h, t in enumerate(thr):
            t32 = torch.tensor(t, dtype=torch.float32, device=DEV)
            assert torch.equal(got[2][h], (dl[:B] < t32).sum(1).int()) and torch.equal(got[3][h], (dr[:B] < t32).sum(1).int())
    assert 0 < int(big[2][0].sum()) < 128 * n


def test_identical_clouds_and_duplicate_points():
    n = 700
    a = uniform((2, n, 3), 41)
    a[:, 100:200] = a[:, :100]                                   # duplicate points
    a[1, 300:] = a[1, 299]
    x = dev(a)
    sl, sr, cl, cr = metrics.chamfer_paired(x, x.clone(), (1e-12, 0.5))
    assert torch.equal(sl, torch.zeros(2, device=DEV)) and torch.equal(sr, torch.zeros(2, device=DEV))
    assert cl.tolist() == [[n, n], [n, n]] == cr.tolist()
    out = metrics.paired_metrics(x, x.clone(), (1e-12,))
    assert out['CD'].tolist() == [0.0, 0.0] and torch.allclose(out['F1'][1e-12], torch.full((2,), 100.0, device=DEV), rtol=1e-6)


# ---- paired_metrics ------------------------------------------------------------------------------------------------------------------
def test_paired_metrics_against_golden_and_the_existing_functions():
    D = golden('g14_evaluation')
    smp, ref = dev(D['smp']), dev(D['ref'])
    B, n = smp.shape[0], smp.shape[1]
    thresholds = (0.01, 0.001, 0.02)
    out = metrics.paired_metrics(smp, ref, thresholds)
    assert set(out) == {'CD', 'CDL', 'CDR', 'EMD', 'F1'} and set(out['F1']) == set(thresholds)
    assert np.allclose(out['CD'].cpu().numpy(), D['pair_CD'], atol=1e-5)
    dl, dr = metrics.nn_distance(smp, ref)
    assert np.allclose(out['CDL'].cpu().numpy(), dl.double().mean(1).cpu().numpy(), atol=1e-5)
    assert np.allclose(out['CDR'].cpu().numpy(), dr.double().mean(1).cpu().numpy(), atol=1e-5)
    assert torch.equal(out['CD'], out['CDL'] + out['CDR'])
    want_emd = metrics.emd_approx(smp, ref)
    print('EMD', out['EMD'].tolist(), want_emd.tolist())
    assert torch.equal(bits(out['EMD']), bits(want_emd))
    x, y = dev(uniform((8, 100, 3), 71)), dev(uniform((8, 100, 3), 72))                 # 1 / 100 is no float32 value either
    assert torch.equal(bits(metrics.paired_metrics(x, y, (), cd=False)['EMD']), bits(metrics.emd_approx(x, y)))
    for thr in thresholds:
        want = ev._f1(dl, dr, thr)
        err = (out['F1'][thr] - want).abs().max().item()
        print(f'F1 at {thr}: max |diff| {err:.3e}', want.tolist())
        assert err <= 4 * 100 * 2 * U                            # 4 float32 ulps at 100
    part = metrics.paired_metrics(smp, ref, (), cd=False, emd=False)
    assert set(part) == {'F1'} and part['F1'] == {}
    only_cd = metrics.paired_metrics(smp, ref, (0.01,), emd=False)
    assert set(only_cd) == {'CD', 'CDL', 'CDR', 'F1'} and torch.equal(only_cd['CD'], out['CD'])
    assert torch.equal(only_cd['F1'][0.01], out['F1'][0.01])
    nine = tuple(0.002 * (k + 1) for k in range(9))              # more than 8 thresholds: a second pass
    many = metrics.paired_metrics(smp, ref, nine, emd=False)
    for thr in nine:
        assert (many['F1'][thr] - ev._f1(dl, dr, thr)).abs().max().item() <= 4 * 100 * 2 * U
    with pytest.raises(gw.GwtfError):
        metrics.paired_metrics(smp, ref[:, :n - 1].contiguous(), ())                     # EMD needs equal sizes
    with pytest.raises(gw.GwtfError):
        metrics.paired_metrics(smp, ref, (), meter=torch.zeros(11, device=DEV))          # float32 meter


def test_meter_sums_and_graph_replay():
    """One batch's frame + metrics + meter update, eagerly once and then captured: two replays double what one call adds."""
    B, n, thresholds = 3, 200, (0.002, 0.01)
    gen, ref = dev(uniform((B, 3, n), 51)), dev(uniform((B, 3, n), 52))
    batch = {'orig_s': dev(uniform((B,), 7, 0.5, 2.0)), 'orig_c': dev(uniform((B, 3), 8, -1.0, 1.0))}
    frame = metrics.EvalFrame.from_config(**FRAMES['both'])

    def step(meter):
        a, b = metrics.clouds_to_eval_frame(gen, ref, frame, **batch)
        return metrics.paired_metrics(a, b, thresholds, meter=meter)

    eager = metrics.new_meter(len(thresholds), DEV)
    out = step(eager)
    want = [float(B), out['CD'].double().sum().item(), out['EMD'].double().sum().item()] + \
        [out['F1'][t].double().sum().item() for t in thresholds]
    got = eager.tolist()
    assert got[0] == B and got[5:] == [0.0] * (len(got) - 5)
    for g, w in zip(got[1:5], want[1:]):
        assert abs(g - w) <= 1e-12 * abs(w)
    torch.cuda.synchronize()
    meter = metrics.new_meter(len(thresholds), DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(meter)
    graph.replay()
    torch.cuda.synchronize()
    once = meter.tolist()
    assert once == got                                            # the replay adds the eager call's bits
    graph.replay()
    torch.cuda.synchronize()
    assert meter.tolist() == [2 * v for v in got]


# ---- the models -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ae_model():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='autoencoding')
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def svr_model():
    D = golden('g21_svr')
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], util_mode='reconstruction')
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    return m.to(DEV).eval()


def test_autoencode_many(ae_model):
    S, n, K = 3, 64, ae_model.n_components
    x = dev(uniform((S, 3, 128), 61, -0.4, 0.4))
    got, labels = ae_model.autoencode_many(x, n, return_labels=True, state=gw.make_state(5, DEV))
    with torch.no_grad():
        codes = ae_model.encode(x)['g_posterior_mus']
    want, want_labels = ae_model.generate_many(codes, n, return_labels=True, state=gw.make_state(5, DEV))
    assert got.shape == (S, 3, n) and torch.equal(bits(got), bits(want)) and torch.equal(labels, want_labels)
    np.random.seed(3)
    y, lab = ae_model.autoencode_many(x, n, return_labels=True)
    assert y.shape == (S, 3, n) and y.dtype == torch.float32 and lab.shape == (S, n)
    assert 1 <= int(lab.min()) and int(lab.max()) <= K
    assert ae_model.autoencode_many(x, n).shape == (S, 3, n)


FRAME_CFG = dict(BASE, unit_scale_evaluation=True, orig_scale_evaluation=True)
THRESHOLDS = (0.01, 0.05)


def make_batches(seed, with_images):
    out = []
    for k, B in enumerate((3, 2)):                                # a ragged last batch
        b = {'cloud': dev(uniform((B, 3, 128), seed + k, -0.4, 0.4)), 'eval_cloud': dev(uniform((B, 3, 64), seed + 10 + k, -0.4, 0.4)),
             'orig_s': dev(uniform((B,), seed + 20 + k, 0.5, 2.0)), 'orig_c': dev(uniform((B, 3), seed + 30 + k, -1.0, 1.0))}
        if with_images:
            b['image'] = dev(np.asarray(synth_images(B, 64, 64, seed + 40 + k), np.float32))
        out.append(b)
    return out


def check_one_call(fn, clouds_of, batches, scale_cd, scale_emd):
    n, Bmax = 64, 3
    frame = metrics.EvalFrame.from_config(**FRAME_CFG)
    before = [{k: v.clone() for k, v in b.items()} for b in batches]
    state = gw.make_state(9, DEV)
    pairs = [recon_ref.to_eval_frame(clouds_of(b, state), b['eval_cloud'], b, **FRAME_CFG) for b in batches]
    want = recon_ref.hand_loop(pairs, THRESHOLDS)
    got = fn(batches, f1_threshold_lst=THRESHOLDS, frame=frame, state=gw.make_state(9, DEV))
    assert set(got) == {'cd', 'emd', 'f1_0.0100', 'f1_0.0500'} and all(isinstance(v, float) for v in got.values())
    print('one call:', got, 'hand loop:', {k: v for k, v in want.items() if k != 'emd_pairs'})
    want_emd = want['emd_pairs'].double().mean().item()
    assert abs(got['emd'] / scale_emd - want_emd) <= 1e-12 * abs(want_emd)
    assert abs(want['emd'] - want_emd) <= Bmax * U * abs(want_emd)                        # the loop's own float32 batch means
    tol = 2 * (n - 1) * U + (Bmax - 1) * U
    assert tol < 1e-5
    assert abs(got['cd'] / scale_cd - want['cd']) <= tol * abs(want['cd'])
    for key in ('f1_0.0100', 'f1_0.0500'):
        assert 0.0 < want[key] < 100.0 and abs(got[key] - want[key]) <= tol * abs(want[key]), key
    for b, b0 in zip(batches, before):                                                    # the batches are left alone
        assert all(torch.equal(bits(b[k]), bits(b0[k])) for k in b)
    part = fn(batches, f1_threshold_lst=THRESHOLDS, frame=frame, state=gw.make_state(9, DEV), emd=False, f1=False)
    assert set(part) == {'cd'} and part['cd'] == got['cd']
    part = fn(batches, f1_threshold_lst=THRESHOLDS[:1], frame=frame, state=gw.make_state(9, DEV), cd=False)
    assert set(part) == {'emd', 'f1_0.0100'} and part['emd'] == got['emd'] and part['f1_0.0100'] == got['f1_0.0100']
    with pytest.raises(gw.GwtfError):
        fn([], f1_threshold_lst=THRESHOLDS, frame=frame)
    with pytest.raises(gw.GwtfError):
        fn(iter(()), f1_threshold_lst=THRESHOLDS)


def test_evaluate_autoencoding_is_the_hand_loop(ae_model):
    check_one_call(lambda batches, **kw: ev.evaluate_autoencoding(ae_model, batches, 64, **kw),
                   lambda b, state: ae_model.autoencode_many(b['cloud'], 64, state=state), make_batches(300, False), 1e4, 1e2)


def test_evaluate_reconstruction_is_the_hand_loop(svr_model):
    batches = make_batches(400, True)
    check_one_call(lambda batches, **kw: ev.evaluate_reconstruction(svr_model, batches, 64, **kw),
                   lambda b, state: svr_model.reconstruct_many(b['image'], 64, state=state), batches, 1.0, 1.0)
    with pytest.raises(gw.GwtfError):
        ev.evaluate_reconstruction(svr_model, [{k: v for k, v in batches[0].items() if k != 'image'}], 64)
