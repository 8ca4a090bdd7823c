"""Generation / reconstruction metrics built on the structural-loss kernels (metrics.py).

Host-side mirror of what lib/networks/evaluating.py imports: lib/metrics/evaluation_metrics.py (distChamfer :33-45,
EMD_CD_F1 :47-107, _pairwise_EMD_CD_F1_SCORE :110-181, knn :185-218, lgan_mmd_cov :220-239, compute_all_metrics :242-329)
and lib/networks/utils.py (get_voxel_occ_dist :45-79, JSD :82-86).  Same names, arguments, return keys and conventions
(which output is "left" and which "right", 1-based vs 0-based, biased means), so evaluate_ae.py runs unchanged on ROCm.
The O(N^2) work per cloud pair runs in csrc/gwtf_metrics.hip; everything here is orchestration.

pairwise_matrices / generation_metrics are the device-resident form of the generation evaluation (evaluating.py:191-250): the
all-pairs matrices come from metrics.chamfer_directed / metrics.emd_cost_pairs (no per-row host loop, a set against itself costs
one directed pass, every F1 threshold comes out of the same pass), and the result dictionaries are those of compute_all_metrics.
pairwise_CD / COV / MMD / KNN mirror lib/networks/utils.py:90-144.

reconstruction_figure / sweep_figure / segmentation_figure are the qualitative outputs (lib/visualization/utils.py:41-61 and its
kin) as contact sheets drawn on the device by render.render_clouds.

evaluate_generation / evaluate_autoencoding / evaluate_reconstruction are the three branches of the reference's evaluate
(evaluating.py:13-266) in one call each, on the device; the two paired ones run on metrics.clouds_to_eval_frame and
metrics.paired_metrics (cloud i against cloud i, one Chamfer pass for CD and every F1 threshold, sums kept on the device).
"""
import numpy as np
import torch
from scipy.stats import entropy

from . import metrics as _metrics
from . import render as _render
from ._lib import GwtfError
from .metrics import distChamferCUDA, emd_approx, f_score  # noqa: F401  (re-exported: evaluating.py imports them from here)


def distChamfer(a, b):
    """Pure-torch Chamfer via |x|^2 + |y|^2 - 2 x.y (reference :33-45).  NOTE the reference's return order: first the
    distance of every point of ``b`` to its nearest in ``a`` (min over dim 1), then the other direction; a and b must
    have the same number of points (its diagonal indexing assumes so)."""
    x, y = a, b
    xx = (x * x).sum(2)                       # (B, N)
    yy = (y * y).sum(2)
    P = xx.unsqueeze(2) + yy.unsqueeze(1) - 2.0 * torch.bmm(x, y.transpose(2, 1))
    return P.min(1)[0], P.min(2)[0]


def _cd_pair(x, y, accelerated_cd):
    return distChamferCUDA(x, y) if accelerated_cd else distChamfer(x, y)


def _f1(dl, dr, threshold):
    precision = 100. * (dr < threshold).float().mean(1)
    recall = 100. * (dl < threshold).float().mean(1)
    return 2. * precision * recall / (precision + recall + 1e-7)


def EMD_CD_F1(sample_pcs, ref_pcs, batch_size, accelerated_cd=False, reduced=True, cd_option=False, emd_option=False,
              one_part_of_cd=False, f1_option=False, f1_threshold=0.0001):
    """Cloud i of ``sample_pcs`` against cloud i of ``ref_pcs`` (reference :47-107).  Options that are off report 0."""
    n = sample_pcs.shape[0]
    assert n == ref_pcs.shape[0], "REF:%d SMP:%d" % (ref_pcs.shape[0], n)
    acc = {'CD': [], 'EMD': [], 'F1': [], 'CDL': [], 'CDR': []}
    for lo in range(0, n, batch_size):
        s, r = sample_pcs[lo:lo + batch_size], ref_pcs[lo:lo + batch_size]
        dl, dr = _cd_pair(s, r, accelerated_cd)
        if cd_option:
            acc['CD'].append(dl.mean(dim=1) + dr.mean(dim=1))
        if one_part_of_cd:
            acc['CDL'].append(dl.mean(dim=1))
            acc['CDR'].append(dr.mean(dim=1))
        if emd_option:
            acc['EMD'].append(emd_approx(s, r))
        if f1_option:
            acc['F1'].append(_f1(dl, dr, f1_threshold))
    out = {}
    for key, vals in acc.items():
        if vals:
            v = torch.cat(vals)
            out[key] = v.mean() if reduced else v
        else:
            out[key] = 0
    return out


def _pairwise_EMD_CD_F1_SCORE(sample_pcs, ref_pcs, batch_size, f1_threshold, accelerated_cd=True, cd_option=False,
                              one_part_of_cd=False, emd_option=False, f1_option=False):
    """Every sample cloud against every reference cloud -> (N_sample, N_ref) matrices (reference :110-181); a matrix whose
    option is off comes back as an empty list, as in the reference."""
    rows = {'cd': [], 'emd': [], 'f1': [], 'left': [], 'right': []}
    n_ref = ref_pcs.shape[0]
    for i in range(sample_pcs.shape[0]):
        cur = {k: [] for k in rows}
        for lo in range(0, n_ref, batch_size):
            ref = ref_pcs[lo:lo + batch_size]
            smp = sample_pcs[i].view(1, -1, 3).expand(ref.size(0), -1, -1).contiguous()
            dl, dr = _cd_pair(smp, ref, accelerated_cd)
            if one_part_of_cd:
                cur['left'].append(dl.mean(dim=1).view(1, -1))
                cur['right'].append(dr.mean(dim=1).view(1, -1))
            if cd_option:
                cur['cd'].append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
            if emd_option:
                cur['emd'].append(emd_approx(smp, ref).view(1, -1))
            if f1_option:
                cur['f1'].append(_f1(dl, dr, f1_threshold).view(1, -1))
        for k in rows:
            if cur[k]:
                rows[k].append(torch.cat(cur[k], dim=1))
    mat = {k: (torch.cat(v, dim=0) if v else []) for k, v in rows.items()}
    return mat['cd'], mat['emd'], mat['f1'], mat['left'], mat['right']


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """Leave-one-out k-NN two-sample test on the joint distance matrix (reference :185-218, after Xu et al.)."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    _, idx = (M + torch.diag(float('inf') * torch.ones(n0 + n1).to(Mxx))).topk(k, 0, False)
    count = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        count = count + label.index_select(0, idx[i])
    pred = torch.ge(count, (float(k) / 2) * torch.ones(n0 + n1).to(Mxx)).float()
    s = {'tp': (pred * label).sum(), 'fp': (pred * (1 - label)).sum(),
         'fn': ((1 - pred) * label).sum(), 'tn': ((1 - pred) * (1 - label)).sum()}
    s.update({'precision': s['tp'] / (s['tp'] + s['fp'] + 1e-10), 'recall': s['tp'] / (s['tp'] + s['fn'] + 1e-10),
              'acc_t': s['tp'] / (s['tp'] + s['fn'] + 1e-10), 'acc_f': s['tn'] / (s['tn'] + s['fp'] + 1e-10),
              'acc': torch.eq(label, pred).float().mean()})
    return s


def lgan_mmd_cov(all_dist, mode='min'):
    """Minimum matching distance and coverage from an (N_sample, N_ref) matrix (reference :220-239)."""
    n_ref = all_dist.size(1)
    pick = torch.min if mode == 'min' else torch.max
    if mode not in ('min', 'max'):
        raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
    val_fromsmp, idx = pick(all_dist, dim=1)
    val, idx_mmd = pick(all_dist, dim=0)
    cov = torch.tensor(float(idx.unique().view(-1).size(0)) / float(n_ref)).to(all_dist)
    return {'lgan_mmd': val.mean(), 'lgan_cov': cov, 'lgan_mmd_smp': val_fromsmp.mean(), 'idx_mmd': idx_mmd,
            'mmd_contrib': val}


def compute_all_metrics(sample_pcs, ref_pcs, batch_size, accelerated_cd=False, f1_threshold=0.001, cd_option=False,
                        one_part_of_cd=False, emd_option=False, f1_option=False):
    """MMD / COV / 1-NN accuracy for every enabled distance (reference :242-329)."""
    opts = dict(accelerated_cd=accelerated_cd, f1_threshold=f1_threshold, cd_option=cd_option,
                one_part_of_cd=one_part_of_cd, emd_option=emd_option, f1_option=f1_option)
    names = ('CD', 'EMD', 'F1', 'CD-left', 'CD-right')
    enabled = (cd_option, emd_option, f1_option, one_part_of_cd, one_part_of_cd)
    rs = _pairwise_EMD_CD_F1_SCORE(sample_pcs, ref_pcs, batch_size, **opts)
    results = {}
    for name, on, M in zip(names, enabled, rs):
        if on:
            res = lgan_mmd_cov(M, 'max' if name == 'F1' else 'min')
            results.update({'%s-%s' % (k, name): v for k, v in res.items()})
    rr = _pairwise_EMD_CD_F1_SCORE(ref_pcs, ref_pcs, batch_size, **opts)
    ss = _pairwise_EMD_CD_F1_SCORE(sample_pcs, sample_pcs, batch_size, **opts)
    for name, on, M_rs, M_rr, M_ss in zip(names, enabled, rs, rr, ss):
        if on:
            one_nn = knn(M_ss, M_rs, M_rr, 1, sqrt=False)
            results.update({'1-NN-%s-%s' % (name, k): v for k, v in one_nn.items() if 'acc' in k})
    return results


_NAMES = ('CD', 'EMD', 'F1', 'CD-left', 'CD-right')


def _same_clouds(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def pairwise_matrices(sample_pcs, ref_pcs, f1_thresholds=(), cd_option=False, one_part_of_cd=False, emd_option=False):
    """The matrices of _pairwise_EMD_CD_F1_SCORE, computed on the device without its host loop: a dict with 'cd', 'left', 'right',
    'emd' ((N_sample, N_ref) each; [] when the option is off) and 'f1' = {threshold: matrix} for every threshold asked for.
    left[i][j] is the mean over the points of sample i of the squared distance to reference j, right[i][j] the mean over the
    points of reference j; the F1 matrices come from integer counts of the same minima, in _f1's expression.  The same tensor
    passed twice costs one directed pass (right = left.T: the two directions of a pair are the same numbers)."""
    f1_thresholds = tuple(f1_thresholds)
    n, m = sample_pcs.shape[1], ref_pcs.shape[1]
    out = {'cd': [], 'left': [], 'right': [], 'emd': [], 'f1': {}}
    if emd_option and n != m:
        raise GwtfError(f'EMD needs clouds of equal size (emd_approx): got {n} and {m} points')
    if cd_option or one_part_of_cd or f1_thresholds:
        sum_sr, cnt_sr = _metrics.chamfer_directed(sample_pcs, ref_pcs, f1_thresholds)
        if _same_clouds(sample_pcs, ref_pcs):
            sum_rs, cnt_rs = sum_sr, cnt_sr
        else:
            sum_rs, cnt_rs = _metrics.chamfer_directed(ref_pcs, sample_pcs, f1_thresholds)
        left = sum_sr / float(n)
        right = (left if sum_rs is sum_sr else sum_rs / float(m)).t().contiguous()
        if one_part_of_cd:
            out['left'], out['right'] = left, right
        if cd_option:
            out['cd'] = left + right
        for h, thr in enumerate(f1_thresholds):
            recall = 100. * (cnt_sr[h].float() / float(n))                       # sample points close to the reference (dl)
            precision = 100. * (cnt_rs[h].t().float() / float(m))                # reference points close to the sample (dr)
            out['f1'][thr] = 2. * precision * recall / (precision + recall + 1e-7)
    else:
        _metrics._cloud_sets(sample_pcs, ref_pcs, 'sample_pcs', 'ref_pcs')
    if emd_option:
        out['emd'] = _metrics.emd_cost_pairs(sample_pcs, ref_pcs) / float(n)
    return out


def generation_metrics(sample_pcs, ref_pcs, f1_threshold_lst=(0.001,), cd_option=False, one_part_of_cd=False, emd_option=False,
                       f1_option=False):
    """{threshold: compute_all_metrics(..., f1_threshold=threshold)} for every threshold of the list, from ONE set of
    sample x ref / ref x ref / sample x sample matrices: distances and EMD are computed once however many thresholds are
    asked for (evaluating.py:212-216 recomputes them per threshold)."""
    thresholds = tuple(f1_threshold_lst)
    opts = dict(f1_thresholds=thresholds if f1_option else (), cd_option=cd_option, one_part_of_cd=one_part_of_cd,
                emd_option=emd_option)
    rs = pairwise_matrices(sample_pcs, ref_pcs, **opts)
    rr = pairwise_matrices(ref_pcs, ref_pcs, **opts)
    ss = pairwise_matrices(sample_pcs, sample_pcs, **opts)
    enabled = (cd_option, emd_option, f1_option, one_part_of_cd, one_part_of_cd)
    shared = {}       # everything that does not depend on the threshold, in compute_all_metrics' key order
    per_thr = {}
    for thr in thresholds:
        def mats(M):
            return (M['cd'], M['emd'], M['f1'].get(thr, []), M['left'], M['right'])
        results = {}
        for name, on, M in zip(_NAMES, enabled, mats(rs)):
            if on:
                key = ('mmd', name)
                if name == 'F1':
                    res = lgan_mmd_cov(M, 'max')
                else:
                    res = shared[key] = shared.get(key) or lgan_mmd_cov(M, 'min')
                results.update({'%s-%s' % (k, name): v for k, v in res.items()})
        for name, on, M_rs, M_rr, M_ss in zip(_NAMES, enabled, mats(rs), mats(rr), mats(ss)):
            if on:
                key = ('knn', name)
                if name == 'F1':
                    one_nn = knn(M_ss, M_rs, M_rr, 1, sqrt=False)
                else:
                    one_nn = shared[key] = shared.get(key) or knn(M_ss, M_rs, M_rr, 1, sqrt=False)
                results.update({'1-NN-%s-%s' % (name, k): v for k, v in one_nn.items() if 'acc' in k})
        per_thr[thr] = results
    return per_thr


@torch.no_grad()
def generate_clouds(model, n_shapes, n_points, batch_size=64, state=None):
    """The generated set of the generation evaluation (evaluating.py:191-205: one `model(...)` call per shape in 'generating' mode) in
    batches on the device: `encode` draws the latent codes from the learned prior (torch's generator of the device) and
    `Flow_Mixture_Model.generate_many` turns them into clouds, components and base samples drawn from `state` (clouds.make_state;
    None: the state the model keeps).  Nothing is read back between the batches.
    -> (n_shapes, n_points, 3) float32, contiguous, on the model's device: the layout generation_metrics takes.
    Unlike the reference's loop (evaluating.py:198-203) a cloud that holds NaN is NOT drawn again: looking for one is a host
    synchronisation per batch.  replace_nan_clouds does the reference's replacement on the whole set without one."""
    if getattr(model, 'mode', None) != 'generating':
        raise GwtfError("generate_clouds needs a model in 'generating' mode (model.mode / util_mode)")
    if n_shapes < 1 or n_points < 1 or batch_size < 1:
        raise ValueError('n_shapes, n_points and batch_size must be positive')
    dev = next(model.parameters()).device
    out = torch.empty(n_shapes, n_points, 3, device=dev, dtype=torch.float32)
    for lo in range(0, n_shapes, batch_size):
        bs = min(batch_size, n_shapes - lo)
        g = model.encode(torch.empty(bs, 0, device=dev))['g_prior_samples'][-1]
        out[lo:lo + bs] = model.generate_many(g, n_points, state=state).transpose(1, 2)
    return out


def replace_nan_clouds(clouds, generator=None):
    """evaluating.py:196-202 on the device: every cloud of ``clouds`` ((S, n, 3) float32 on a HIP device) that holds a NaN is replaced
    by a cloud without NaN of the same set, drawn uniformly with replacement (``generator``: a torch.Generator of that device; None:
    the device's default one) -> a new (S, n, 3) tensor; clouds without NaN come back bit-equal.  No synchronisation and no shape that
    depends on the data: the clouds are flagged, a stable sort of the flags lists the good ones first, a uniform draw is scaled by the
    device-side count of good clouds, and one gather builds the result -- the count of bad clouds never reaches the host.
    If EVERY cloud holds a NaN the input comes back unchanged (a copy): the reference raises there (np.random.choice on an empty
    list), which here would take a read-back of that count."""
    if not torch.is_tensor(clouds) or clouds.dim() != 3 or clouds.shape[2] != 3:
        raise GwtfError(f'clouds must be an (S, n, 3) tensor, got {tuple(clouds.shape) if torch.is_tensor(clouds) else type(clouds)}')
    _metrics._ptr(clouds, 'clouds')
    S, dev = clouds.shape[0], clouds.device
    if S == 0 or clouds.shape[1] == 0:
        raise GwtfError('empty point set')
    bad = torch.isnan(clouds).flatten(1).any(1)                                    # (S,)
    good_first = torch.sort(bad.to(torch.uint8), stable=True).indices              # the good clouds in their order, then the bad ones
    n_good = S - bad.sum()                                                         # 0-d, stays on the device
    u = torch.rand(S, device=dev, dtype=torch.float64, generator=generator)
    pick = torch.minimum((u * n_good).long(), (n_good - 1).clamp(min=0))           # uniform in [0, n_good)
    src = torch.where(bad & (n_good > 0), good_first[pick], torch.arange(S, device=dev))
    return clouds.index_select(0, src)


@torch.no_grad()
def evaluate_generation(model, ref_clouds, n_points=None, batch_size=64, f1_threshold_lst=(0.001,), cd=True, emd=True, f1=True,
                        jsd=True, state=None, generator=None):
    """The generating branch of the reference's evaluate (evaluating.py:191-250) in one call, on the device: one generated cloud per
    cloud of ``ref_clouds`` ((R, n, 3) float32 on the model's device; ``n_points`` per generated cloud, default n) from generate_clouds
    (``batch_size``, ``state``), replace_nan_clouds (``generator``), the device JSD and generation_metrics.
    -> the reference's `res` dictionary, same keys and scalings, values as Python floats: 'jsd' (x 1e2); 'cd_mmds' (x 1e4), 'cd_covs',
    'cd_1nns' (x 1e2); 'emd_mmds', 'emd_covs', 'emd_1nns' (x 1e2); per threshold 'f1_%.4f_mmds' (unscaled), 'f1_%.4f_covs',
    'f1_%.4f_1nns' (x 1e2).  As in the reference the metric keys are written once per threshold of ``f1_threshold_lst`` (an empty list
    leaves 'jsd' alone).  Every scaled value is scaled in the tensor's own precision, as the reference scales it, and all of them
    reach the host in ONE read at the end; before that nothing is read back but what generation_metrics itself reads (coverage
    counts distinct indices).  The rescaling options of evaluate (unit_scale_evaluation, orig_scale_evaluation) and its h5 saving are
    not part of this call."""
    if not torch.is_tensor(ref_clouds) or ref_clouds.dim() != 3 or ref_clouds.shape[2] != 3:
        raise GwtfError(f'ref_clouds must be an (R, n, 3) tensor, got {tuple(ref_clouds.shape) if torch.is_tensor(ref_clouds) else type(ref_clouds)}')
    _metrics._ptr(ref_clouds, 'ref_clouds')
    n_shapes, n = ref_clouds.shape[0], ref_clouds.shape[1]
    gen = generate_clouds(model, n_shapes, n if n_points is None else int(n_points), batch_size=batch_size, state=state)
    gen = replace_nan_clouds(gen, generator=generator)
    res = {}
    if jsd:
        res['jsd'] = JSD(gen, ref_clouds, clouds1_flag='gen', clouds2_flag='ref', warning=False) * 1e2
    per_thr = generation_metrics(gen, ref_clouds, f1_threshold_lst, cd_option=cd, emd_option=emd, f1_option=f1)
    for thr, m in per_thr.items():
        if cd:
            res.update(cd_mmds=m['lgan_mmd-CD'] * 1e4, cd_covs=m['lgan_cov-CD'] * 1e2, cd_1nns=m['1-NN-CD-acc'] * 1e2)
        if emd:
            res.update(emd_mmds=m['lgan_mmd-EMD'] * 1e2, emd_covs=m['lgan_cov-EMD'] * 1e2, emd_1nns=m['1-NN-EMD-acc'] * 1e2)
        if f1:
            res['f1_%.4f_mmds' % thr] = m['lgan_mmd-F1']
            res['f1_%.4f_covs' % thr] = m['lgan_cov-F1'] * 1e2
            res['f1_%.4f_1nns' % thr] = m['1-NN-F1-acc'] * 1e2
    if not res:
        return res
    values = torch.stack([v.to(torch.float64) for v in res.values()]).tolist()       # the one read
    return dict(zip(res.keys(), values))


def _device_batch(batch, needs_image):
    """The tensors one batch of a device loader contributes, refused when they are not on a HIP device."""
    if not isinstance(batch, dict) or 'cloud' not in batch or 'eval_cloud' not in batch:
        raise GwtfError("every batch must be a dict with 'cloud' and 'eval_cloud' (DeviceCloudLoader / DeviceSVRLoader)")
    if needs_image and 'image' not in batch:
        raise GwtfError("evaluate_reconstruction needs batch['image'] (DeviceSVRLoader)")
    for key in ('cloud', 'eval_cloud', 'image', 'orig_c', 'orig_s'):
        t = batch.get(key)
        if t is not None and not _on_device(t):
            raise GwtfError(f"batch[{key!r}] must be a tensor on a HIP device; there is no CPU path")
    return batch


def _evaluate_paired(clouds_of, batches, needs_image, f1_threshold_lst, cd, emd, f1, frame):
    """The loop both paired evaluations share: clouds from the model, the frame, the metrics, every sum kept on the device in one
    meter; ONE read at the end -> ({'cd', 'emd', 'f1_%.4f'} float64 means over all pairs, unscaled; keys of disabled options left out)."""
    thresholds = tuple(f1_threshold_lst) if f1 else ()
    meter, n_batches = None, 0
    for batch in batches:
        batch = _device_batch(batch, needs_image)
        ref = batch['eval_cloud']
        if meter is None:
            meter = _metrics.new_meter(len(thresholds), ref.device)
        gen = clouds_of(batch)
        gen_f, ref_f = _metrics.clouds_to_eval_frame(gen, ref, frame, orig_s=batch.get('orig_s'), orig_c=batch.get('orig_c'))
        _metrics.paired_metrics(gen_f, ref_f, thresholds, cd=cd, emd=emd, meter=meter)
        n_batches += 1
    if n_batches == 0:
        raise GwtfError('no batches: the iterable is empty')
    sums = meter.tolist()                                                            # the one read
    count, res = sums[0], {}
    if cd:
        res['cd'] = sums[1] / count
    if emd:
        res['emd'] = sums[2] / count
    for h, thr in enumerate(thresholds):
        res['f1_%.4f' % thr] = sums[_metrics.METER_HEAD + h] / count
    return res


@torch.no_grad()
def evaluate_autoencoding(model, batches, n_points, f1_threshold_lst=(0.0001,), cd=True, emd=True, f1=True, frame=None, state=None):
    """The autoencoding branch of the reference's evaluate (evaluating.py:80-120, 167-189) in one call, on the device.  ``batches``: any
    iterable of device dicts as DeviceCloudLoader yields them ('cloud', 'eval_cloud', optionally 'orig_c', 'orig_s'; a ragged last
    batch is fine).  Per batch: model.autoencode_many(batch['cloud'], n_points, state=state), metrics.clouds_to_eval_frame against
    batch['eval_cloud'] (``frame``: metrics.EvalFrame, None: no rescaling), metrics.paired_metrics into one device meter; nothing is
    read back inside the loop and ONE read happens at the end.
    -> the reference's `res`: 'cd' (x 1e4), 'emd' (x 1e2), 'f1_%.4f' per threshold (unscaled), Python floats; options that are off
    leave their keys out.  Every value is the float64 mean over all pairs of the float32 per-pair values: what EMD_CD_F1's
    reduced=True mean computes, up to its float32 rounding.  The batch's tensors are NOT modified (the reference scales p_clouds in
    place, evaluating.py:104-120)."""
    res = _evaluate_paired(lambda batch: model.autoencode_many(batch['cloud'], n_points, state=state), batches, False,
                           f1_threshold_lst, cd, emd, f1, frame)
    if cd:
        res['cd'] *= 1e4
    if emd:
        res['emd'] *= 1e2
    return res


@torch.no_grad()
def evaluate_reconstruction(model, batches, n_points, f1_threshold_lst=(0.0001,), cd=True, emd=True, f1=True, frame=None, state=None):
    """The reconstruction branch of the reference's evaluate (evaluating.py:80-120, 138-157, 252-261) in one call, on the device.
    ``batches``: any iterable of device dicts as DeviceSVRLoader yields them ('image', 'cloud', 'eval_cloud', optionally 'orig_c',
    'orig_s'; a ragged last batch is fine).  Per batch: model.reconstruct_many(batch['image'], n_points, state=state), then the frame
    and the metrics as in evaluate_autoencoding; one Chamfer pass instead of one per metric and threshold, no transposed copies, and
    ONE read at the end instead of one per metric and batch.
    -> {'cd', 'emd', 'f1_%.4f' per threshold}, all unscaled, Python floats; options that are off leave their keys out.
    [res['cd'], res['emd']] is what the reference returns (`[CD.avg, EMD.avg]`), 'f1_%.4f' what it prints.  Every value is the
    float64 mean over all pairs: what the reference's batch-weighted AverageMeter of float32 batch means computes, up to rounding.
    The batch's tensors are NOT modified (the reference scales p_clouds in place)."""
    return _evaluate_paired(lambda batch: model.reconstruct_many(batch['image'], n_points, state=state), batches, True,
                            f1_threshold_lst, cd, emd, f1, frame)


def _posterior_means(model, clouds):
    """encode(clouds)['g_posterior_mus'] in any model.mode: the cloud encoder and the posterior head, nothing else."""
    return model.g_posterior(model._pooled_features(clouds))[0]


@torch.no_grad()
def interpolate_clouds(model, batches, n_points, n_batches=3, weights=None, flow_idx=None, state=None, generator=None):
    """The reference's `interpolate` (evaluating.py:269-382, the `--interpolation` / `--interpolate_one_flow --flow_idx` branches of
    evaluate_ae.py, kept inside a string literal there) on the device.  ``batches``: device dicts with 'cloud' and 'eval_cloud'
    (DeviceCloudLoader); the first ``n_batches`` are used.  Per batch 'cloud' is paired with a permutation of 'eval_cloud' --
    torch.randperm on the device with ``generator`` where the reference shuffles with np.random -- both codes are the posterior
    means, and Flow_Mixture_Model.interpolate_many (``weights``, default np.arange(1, 10) / 10; ``flow_idx``; ``state``) decodes the T
    steps of every pair with shared draws.  Nothing is read back.
    -> {'clouds1' (N, 3, M), 'clouds2' (N, 3, M), 'interpolations' (N, 3, n_points, T) float32, 'labels' (N, n_points, T) uint8},
    device tensors with the names and layouts of the reference's h5 datasets; writing the file is the caller's."""
    if n_batches < 1:
        raise ValueError('n_batches must be positive')
    parts = {'clouds1': [], 'clouds2': [], 'interpolations': [], 'labels': []}
    for i, batch in enumerate(batches):
        if i == n_batches:
            break
        batch = _device_batch(batch, False)
        clouds, ref = batch['cloud'], batch['eval_cloud']
        ref = ref[torch.randperm(ref.shape[0], device=ref.device, generator=generator)].contiguous()
        x, labels = model.interpolate_many(_posterior_means(model, clouds), _posterior_means(model, ref), n_points, weights=weights,
                                           flow_idx=flow_idx, return_labels=True, state=state)
        parts['clouds1'].append(clouds)
        parts['clouds2'].append(ref)
        parts['interpolations'].append(x.permute(0, 2, 3, 1))               # (S, T, 3, n) -> (S, 3, n, T)
        parts['labels'].append(labels.permute(0, 2, 1).to(torch.uint8))     # (S, T, n) -> (S, n, T)
    if not parts['clouds1']:
        raise GwtfError('no batches: the iterable is empty')
    return {k: torch.cat(v).contiguous() for k, v in parts.items()}


@torch.no_grad()
def upsample_clouds(model, batches, sparse_size, n_points, n_batches=10, state=None):
    """The reference's `sample` (evaluating.py:384-457, the `--sampling` branch of evaluate_ae.py, kept inside a string literal
    there) on the device: the first ``sparse_size`` points of every 'cloud' of the first ``n_batches`` batches are encoded and
    Flow_Mixture_Model.upsample_many decodes ``n_points`` points from the posterior means, with a component label per point.
    -> {'clouds_sparse' (N, 3, sparse_size), 'clouds_dense' (N, 3, n_points) float32, 'labels' (N, n_points) uint8}, device tensors
    with the names and layouts of the reference's h5 datasets."""
    if n_batches < 1 or sparse_size < 1:
        raise ValueError('n_batches and sparse_size must be positive')
    parts = {'clouds_sparse': [], 'clouds_dense': [], 'labels': []}
    for i, batch in enumerate(batches):
        if i == n_batches:
            break
        sparse = _device_batch(batch, False)['cloud'][:, :, :sparse_size].contiguous()
        dense, labels = model.upsample_many(sparse, n_points, return_labels=True, state=state)
        parts['clouds_sparse'].append(sparse)
        parts['clouds_dense'].append(dense)
        parts['labels'].append(labels.to(torch.uint8))
    if not parts['clouds_sparse']:
        raise GwtfError('no batches: the iterable is empty')
    return {k: torch.cat(v).contiguous() for k, v in parts.items()}


@torch.no_grad()
def segment_clouds(model, batches, n_batches=None, parts_key=None, n_parts=None, want_resp=False):
    """Label observed clouds by mixture component, on the device: per batch the codes are the posterior means of batch['cloud'] and
    the labelled points are batch['eval_cloud'] (the pairing of evaluating.py:83-84), through Flow_Mixture_Model.assign_many.
    ``batches``: device dicts with 'cloud' and 'eval_cloud' (DeviceCloudLoader), the first ``n_batches`` of them (None: all);
    parts_key: batch[parts_key] is the (B, N) integer ground-truth part of every point of 'eval_cloud', one of ``n_parts``.
    Nothing is read back inside the loop.
    -> {'clouds' (M, 3, N) float32, 'labels' (M, N) uint8 holding label + 1 with 0 for an invalid point (the `t + 1` convention of the
    reference's h5 `labels` datasets and of upsample_clouds), 'log_density' (M, N), 'confidence' (M, N) float32, 'counts' (M, K)
    int32[, 'resp' (M, K, N)]}; with parts also 'table' (K, n_parts) int64, the (component, part) contingency over all batches --
    part_agreement scores it -- and 'skipped' (1,) int64, the points outside it (invalid label or part outside [0, n_parts))."""
    if n_batches is not None and n_batches < 1:
        raise ValueError('n_batches must be positive')
    if parts_key is not None and n_parts is None:
        raise ValueError('parts_key needs n_parts')
    keys = ('clouds', 'labels', 'log_density', 'confidence', 'counts') + (('resp',) if want_resp else ())
    parts, table, skipped = {k: [] for k in keys}, None, None
    for i, batch in enumerate(batches):
        if i == n_batches:
            break
        batch = _device_batch(batch, False)
        points = batch['eval_cloud'].contiguous()
        gt = None
        if parts_key is not None:
            gt = batch[parts_key]
            if not _on_device(gt) or gt.is_floating_point() or tuple(gt.shape) != (points.shape[0], points.shape[2]):
                raise GwtfError(f'batch[{parts_key!r}] must be a (B, N) integer tensor on a HIP device')
            gt = gt.to(torch.int32).contiguous()
        res = model.assign_many(points, codes=_posterior_means(model, batch['cloud']), want_resp=want_resp, parts=gt, n_parts=n_parts,
                                table=table, skipped=skipped)
        table, skipped = res.get('table'), res.get('skipped')
        parts['clouds'].append(points)
        parts['labels'].append((res['labels'] + 1).to(torch.uint8))
        for k in keys[2:]:
            parts[k].append(res[k])
    if not parts['clouds']:
        raise GwtfError('no batches: the iterable is empty')
    out = {k: torch.cat(v).contiguous() for k, v in parts.items()}
    if parts_key is not None:
        out['table'], out['skipped'] = table, skipped
    return out


# ---- figures: contact sheets drawn on the device (render.py, csrc/gwtf_render.hip) ------------------------------------------------------
_FIGURE_OWNS = ('views', 'out', 'cols', 'cell0', 'cell_step', 'label_base', 'want_index', 'want_depth', 'skipped')


def _figure_options(render):
    """(size, angles, margin, the options handed on to every render_clouds call of a figure)."""
    taken = [k for k in _FIGURE_OWNS if k in render]
    if taken:
        raise GwtfError(f'a figure places its own cells: {taken} cannot be passed')
    size = tuple(int(v) for v in render.get('size', (256, 256)))
    return size, render.get('angles', _render.ANGLES), render.get('margin', 0.05), dict(render, size=size)


def _column(sheet, clouds, labels, views, column, n_cols, opts, **more):
    """One render_clouds call: cloud b into row b, column `column` of a sheet with n_cols columns."""
    _render.render_clouds(clouds, labels, views=views, out=sheet, cols=n_cols, cell0=column, cell_step=n_cols, **dict(opts, **more))


@torch.no_grad()
def reconstruction_figure(model, batch, n_points, nr_samples=5, state=None, **render):
    """The reference's GT_vs_RECONSTRUCTION figure (add_figures_reconstruction_tb / add_svr_reconstruction_tb,
    lib/visualization/utils.py:41-61, called from training.py:147-167 and :269-291) as an image tensor, on the device.  ``batch``: one
    device dict of a loader; its first ``nr_samples`` shapes make the rows.  Column 0: batch['eval_cloud'] in one colour
    (render.GROUND_TRUTH_RGB); column 1: model.autoencode_many(batch['cloud'], n_points, return_labels=True, state=state) -- for a
    Flow_Mixture_SVR_Model reconstruct_many(batch['image'], ...) -- coloured by component; for the SVR model column 2: channels 1:4
    of the input image, clipped to [0, 1] as imshow clips floats and resampled to the cell (nearest).  Both clouds of a row share the
    view fitted to the ground truth (render.fit_views).  render: size, radius, fog, palette, angles, margin, background, invalid of
    render.render_clouds.  Nothing is read back.
    -> (3, rows * H, n_cols * W) uint8: SummaryWriter.add_image('GT_vs_RECONSTRUCTION', sheet, epoch) takes it as it is."""
    size, angles, margin, opts = _figure_options(render)
    svr = hasattr(model, 'reconstruct_many')
    batch = _device_batch(batch, svr)
    S = min(int(nr_samples), batch['eval_cloud'].shape[0])
    if S < 1:
        raise GwtfError('nr_samples must be positive')
    gt = batch['eval_cloud'][:S].contiguous()
    if svr:
        recon, labels = model.reconstruct_many(batch['image'][:S].contiguous(), n_points, return_labels=True, state=state)
    else:
        recon, labels = model.autoencode_many(batch['cloud'][:S].contiguous(), n_points, return_labels=True, state=state)
    n_cols = 3 if svr else 2
    sheet = _render.new_sheet(S, n_cols, size, gt.device, opts.get('background', _render.BACKGROUND_RGB))
    views = _render.fit_views(gt, angles, size, margin)
    _column(sheet, gt, None, views, 0, n_cols, opts, palette=np.array([_render.GROUND_TRUTH_RGB], np.uint8))
    _column(sheet, recon, labels, views, 1, n_cols, opts, label_base=1)
    if svr:
        H, W = size
        img = torch.nn.functional.interpolate(batch['image'][:S, 1:4].float(), size=(H, W), mode='nearest')
        img = (img.clamp(0, 1) * 255).round().to(torch.uint8)                            # (S, 3, H, W)
        sheet.view(3, S, H, n_cols, W)[:, :, :, 2, :] = img.permute(1, 0, 2, 3)
    return sheet


@torch.no_grad()
def sweep_figure(out, **render):
    """The dict interpolate_clouds returns as one sheet of S rows: 'clouds1' in one colour, the T steps of 'interpolations' coloured
    by 'labels' (1..K), 'clouds2' in one colour -- T + 2 columns.  One view per row, fitted to 'clouds1', so that a row shows the
    shape moving inside a fixed window.  render: as for reconstruction_figure.  -> (3, S * H, (T + 2) * W) uint8."""
    size, angles, margin, opts = _figure_options(render)
    for k in ('clouds1', 'clouds2', 'interpolations', 'labels'):
        if k not in out or not _on_device(out[k]):
            raise GwtfError(f"sweep_figure needs out[{k!r}] on a HIP device (the dict interpolate_clouds returns)")
    c1, c2, steps, labels = out['clouds1'], out['clouds2'], out['interpolations'], out['labels']
    S, T = steps.shape[0], steps.shape[3]
    n_cols = T + 2
    sheet = _render.new_sheet(S, n_cols, size, c1.device, opts.get('background', _render.BACKGROUND_RGB))
    views = _render.fit_views(c1, angles, size, margin)
    one = np.array([_render.GROUND_TRUTH_RGB], np.uint8)
    _column(sheet, c1, None, views, 0, n_cols, opts, palette=one)
    for t in range(T):
        _column(sheet, steps[:, :, :, t], labels[:, :, t], views, 1 + t, n_cols, opts, label_base=1)
    _column(sheet, c2, None, views, n_cols - 1, n_cols, opts, palette=one)
    return sheet


@torch.no_grad()
def segmentation_figure(clouds, labels, parts=None, label_base=None, **render):
    """Predicted components beside ground-truth parts: row b shows clouds[b] (B, 3, N) coloured by labels[b] (B, N) and, with
    ``parts`` (B, N), by parts[b] (0-based; a negative part takes the invalid colour).  label_base: None takes the convention from
    the dtype -- 1 for uint8 (segment_clouds' 'labels': label + 1, 0 invalid), 0 otherwise (assign_many's int32 with -1 invalid).
    Both columns share the view fitted to the cloud.  -> (3, B * H, n_cols * W) uint8, n_cols 2 with parts and 1 without."""
    size, angles, margin, opts = _figure_options(render)
    if not _on_device(clouds) or not _on_device(labels) or (parts is not None and not _on_device(parts)):
        raise GwtfError('segmentation_figure needs clouds, labels and parts on a HIP device; there is no CPU path')
    if label_base is None:
        label_base = 1 if labels.dtype == torch.uint8 else 0
    n_cols = 1 if parts is None else 2
    sheet = _render.new_sheet(clouds.shape[0], n_cols, size, clouds.device, opts.get('background', _render.BACKGROUND_RGB))
    views = _render.fit_views(clouds, angles, size, margin)
    _column(sheet, clouds, labels, views, 0, n_cols, opts, label_base=label_base)
    if parts is not None:
        _column(sheet, clouds, parts, views, 1, n_cols, opts, label_base=0)
    return sheet


def part_agreement(table):
    """Agreement of an unsupervised labelling with ground-truth parts from their (K, P) contingency table (segment_clouds' 'table'; a
    device tensor is read once), host-side in float64.  -> {'purity', 'nmi', 'miou', 'mapping'}:
      mapping[k] = argmax_p table[k, p], the lowest p on a tie: the part component k stands for
      purity     = sum_k max_p table[k, p] / sum(table)
      nmi        = I(K; P) / sqrt(H(K) H(P)) in nats, 0 when either entropy is 0
      miou       = mean over the parts with a ground-truth point of TP_p / (GT_p + Pred_p - TP_p), a point predicted as mapping[label]
    An all-zero table gives NaN for the three values."""
    t = np.asarray(table.detach().cpu() if torch.is_tensor(table) else table).astype(np.float64)
    if t.ndim != 2:
        raise ValueError(f'table must be (K, P), got {t.shape}')
    mapping = t.argmax(1)
    total = t.sum()
    if total == 0:
        return {'purity': float('nan'), 'nmi': float('nan'), 'miou': float('nan'), 'mapping': mapping}
    purity = t.max(1).sum() / total
    pk, pp, joint = t.sum(1) / total, t.sum(0) / total, t / total
    entr = lambda p: float(-(p[p > 0] * np.log(p[p > 0])).sum())
    hk, hp = entr(pk), entr(pp)
    nz = joint > 0
    info = float((joint[nz] * np.log(joint[nz] / np.outer(pk, pp)[nz])).sum())
    nmi = info / np.sqrt(hk * hp) if hk > 0 and hp > 0 else 0.0
    P = t.shape[1]
    confusion = np.zeros((P, P))                                   # [predicted part, true part]
    np.add.at(confusion, mapping, t)
    gt, pr, tp = confusion.sum(0), confusion.sum(1), np.diag(confusion)
    seen = gt > 0
    miou = float((tp[seen] / (gt[seen] + pr[seen] - tp[seen])).mean())
    return {'purity': float(purity), 'nmi': float(nmi), 'miou': miou, 'mapping': mapping}


def pairwise_CD(clouds1, clouds2, bs=2048):
    """Chamfer distance (sum of the two directed means) of every cloud of ``clouds1`` against every cloud of ``clouds2``
    (reference utils.py:90-117) -> (N1, N2) float32 on the device.  ``bs`` (the reference's chunk size) is accepted and ignored:
    nothing is chunked."""
    return pairwise_matrices(clouds1, clouds2, cd_option=True)['cd']


def COV(dists, axis=1):
    """Coverage (reference utils.py:120-121): the share of the clouds along ``axis`` that are the nearest one (argmin along ``axis``)
    of at least one cloud of the other axis."""
    return float(dists.min(axis)[1].unique().numel()) / float(dists.shape[axis])


def MMD(dists, axis=1):
    """Minimum matching distance (reference utils.py:124-125): for every cloud along ``axis`` the distance to its nearest cloud
    of the other axis, averaged."""
    return float(dists.min(1 - axis)[0].float().mean())


def KNN(Mxx, Mxy, Myy, k, sqrt=False):
    """Leave-one-out k-NN accuracy on the joint distance matrix (reference utils.py:128-144) as a float.  Unlike knn above the
    labels are -1 (first set) / +1 (second set) and a cloud is predicted +1 when the sum of its neighbours' labels is >= 0 --
    at even k a tie goes to the SECOND set, where knn's count >= k/2 of 1/0 labels sends it to the first."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((-torch.ones(n0), torch.ones(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    M = M + torch.diag(torch.full((n0 + n1,), float('inf')).to(Mxx))
    idx = M.topk(k, 0, False)[1]                                   # the k nearest other clouds of every column
    votes = label[idx].sum(0)
    pred = torch.where(votes >= 0, torch.ones_like(votes), -torch.ones_like(votes))
    return float((pred == label).float().mean())


def _on_device(x):
    return torch.is_tensor(x) and x.is_cuda


def _occupancy_warnings(clouds_flag, bound, n_out, n_nan):
    """The reference's two messages (utils.py:47-54) from the kernel's two value counts."""
    if n_out > 0:
        print('{} clouds out of cube bounds: [-{}; {}]'.format(clouds_flag, bound, bound))
    if n_nan > 0:
        print('{} NaN values in point cloud tensors.'.format(n_nan))


def _normalised(counts):
    return counts.to(torch.float64) / counts.sum()


def get_voxel_occ_dist(all_clouds, clouds_flag='gen', res=28, bound=0.5, bs=128, warning=True):
    """Occupancy histogram of all points over a res^3 grid of [-0.5, 0.5)^3, normalised (reference utils.py:45-79); points
    outside the cube are dropped.  ``bs`` is accepted for signature compatibility (the reference chunks by it).
    A torch tensor on a HIP device takes the device path (metrics.voxel_occupancy: same rule, same counts) and the result is a
    float64 DEVICE tensor, counts / counts.sum().  With warning=False that path synchronises nothing; with warning=True it reads the
    kernel's two value counts once and prints the reference's messages.  One deviation: the reference prints the NaN message whatever
    ``warning`` says; the device path prints it under warning=True only, because knowing the count is a read-back."""
    if _on_device(all_clouds):
        stats = torch.zeros(2, device=all_clouds.device, dtype=torch.int64) if warning else None
        counts = _metrics.voxel_occupancy(all_clouds, res=res, bound=bound, stats=stats)
        if warning:
            _occupancy_warnings(clouds_flag, bound, *stats.tolist())
        return _normalised(counts)
    if np.any(np.fabs(all_clouds) > bound) and warning:
        print('{} clouds out of cube bounds: [-{}; {}]'.format(clouds_flag, bound, bound))
    n_nans = np.isnan(all_clouds).sum()
    if n_nans > 0:
        print('{} NaN values in point cloud tensors.'.format(n_nans))
    edges = -0.5 + np.arange(res + 1) * (1. / res)
    pts = np.asarray(all_clouds).reshape(-1, 3)
    idx = np.stack([np.searchsorted(edges, pts[:, d], side='right') - 1 for d in range(3)], axis=1)   # edges[i] <= x < edges[i+1]
    ok = np.all((idx >= 0) & (idx < res), axis=1)
    hist = np.zeros((res, res, res), dtype=np.uint64)
    np.add.at(hist, tuple(idx[ok].T), np.uint64(1))
    return np.float64(hist) / hist.sum()


def JSD(clouds1, clouds2, clouds1_flag='gen', clouds2_flag='ref', warning=True):
    """Jensen-Shannon divergence (base 2) between the two sets' occupancy histograms (reference utils.py:82-86).
    Two torch tensors on a HIP device take the device path: both histograms and the divergence are computed there
    (metrics.voxel_occupancy, metrics.jsd_from_counts) and the result is a 0-d float64 DEVICE tensor; nothing is synchronised under
    warning=False, and under warning=True the four value counts are read once for the reference's messages (get_voxel_occ_dist
    names the one deviation).  A set without a single point inside the cube gives NaN, as the reference's 0 / 0 does."""
    if _on_device(clouds1) or _on_device(clouds2):
        if not (_on_device(clouds1) and _on_device(clouds2)) or clouds1.device != clouds2.device:
            raise GwtfError('JSD: both cloud sets must be numpy arrays, or both tensors on one HIP device')
        stats = torch.zeros(2, 2, device=clouds1.device, dtype=torch.int64) if warning else None
        c1 = _metrics.voxel_occupancy(clouds1, stats=None if stats is None else stats[0])
        c2 = _metrics.voxel_occupancy(clouds2, stats=None if stats is None else stats[1])
        if warning:
            (out1, nan1), (out2, nan2) = stats.tolist()
            _occupancy_warnings(clouds1_flag, 0.5, out1, nan1)
            _occupancy_warnings(clouds2_flag, 0.5, out2, nan2)
        return _metrics.jsd_from_counts(c1, c2)
    d1 =get_voxel_occ_dist(clouds1, clouds_flag=clouds1_flag, warning=warning)
    d2 = get_voxel_occ_dist(clouds2, clouds_flag=clouds2_flag, warning=warning)
    return entropy((d1 + d2).flatten() / 2.0, base=2) - 0.5 * (entropy(d1.flatten(), base=2) + entropy(d2.flatten(), base=2))
