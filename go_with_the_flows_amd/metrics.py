"""Structural losses between point sets: Chamfer nearest-neighbour distances and the approximate earth-mover cost.

Host-side mirror of lib/metrics/pytorch_structural_losses/{nn_distance.py:5-37, match_cost.py:5-45} and the helpers
that wrap them (lib/metrics/evaluation_metrics.py:21-30, lib/networks/utils.py:34-42).  Same names, argument meaning
and return values; the compute runs in csrc/gwtf_metrics.hip through the C ABI (include/gwtf.h).  Inputs must be float32,
contiguous and on a HIP device -- the checks the reference's extension applies (structural_loss.cpp:10-12); there is no
CPU path.
"""
import ctypes

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from ._lib import GwtfError, _ptr, _stream, check


def _sets(seta, setb):
    if seta.dim() != 3 or setb.dim() != 3 or seta.shape[2] != 3 or setb.shape[2] != 3 or seta.shape[0] != setb.shape[0]:
        raise GwtfError(f'point sets must be (b,n,3) and (b,m,3): got {tuple(seta.shape)} and {tuple(setb.shape)}')
    _ptr(seta, 'seta'), _ptr(setb, 'setb')        # device / contiguity / dtype checks before anything touches HIP
    if min(seta.shape[0], seta.shape[1], setb.shape[1]) == 0:
        raise GwtfError('empty point set')
    return seta.shape[0], seta.shape[1], setb.shape[1]


def nn_distance_raw(seta, setb):
    """NNDistance (structural_loss.cpp:82-104): dist1 (b,n), idx1 (b,n) int32, dist2 (b,m), idx2 (b,m) int32."""
    b, n, m = _sets(seta, setb)
    L = _lib.lib()
    dev = seta.device
    dist1 = torch.empty(b, n, device=dev, dtype=torch.float32)
    dist2 = torch.empty(b, m, device=dev, dtype=torch.float32)
    idx1 = torch.empty(b, n, device=dev, dtype=torch.int32)
    idx2 = torch.empty(b, m, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(L.gwtf_nn_distance(_ptr(seta, 'seta'), _ptr(setb, 'setb'), dist1.data_ptr(), idx1.data_ptr(),
                                 dist2.data_ptr(), idx2.data_ptr(), b, n, m, _stream(seta)))
    return dist1, idx1, dist2, idx2


class NNDistanceFunction(Function):
    """nn_distance.py:5-35: forward returns (dist1, dist2); the argmin indices are kept for the backward."""

    @staticmethod
    def forward(ctx, seta, setb):
        dist1, idx1, dist2, idx2 = nn_distance_raw(seta, setb)
        ctx.save_for_backward(seta, setb)
        ctx.idx1, ctx.idx2 = idx1, idx2
        return dist1, dist2

    @staticmethod
    def backward(ctx, grad_dist1, grad_dist2):
        seta, setb = ctx.saved_tensors
        b, n, m = _sets(seta, setb)
        grada, gradb = torch.empty_like(seta), torch.empty_like(setb)
        with torch.cuda.device(seta.device):
            check(_lib.lib().gwtf_nn_distance_grad(
                _ptr(seta, 'seta'), _ptr(setb, 'setb'), _ptr(grad_dist1.contiguous(), 'grad_dist1'), ctx.idx1.data_ptr(),
                _ptr(grad_dist2.contiguous(), 'grad_dist2'), ctx.idx2.data_ptr(), _ptr(grada, 'grada'),
                _ptr(gradb, 'gradb'), b, n, m, _stream(seta)))
        return grada, gradb


nn_distance = NNDistanceFunction.apply


def approx_match(seta, setb):
    """ApproxMatch (structural_loss.cpp:22-37): match (b,m,n) and the (b,2(n+m)) scratch the reference also returns."""
    b, n, m = _sets(seta, setb)
    match = torch.empty(b, m, n, device=seta.device, dtype=torch.float32)
    temp = torch.empty(b, (n + m) * 2, device=seta.device, dtype=torch.float32)
    with torch.cuda.device(seta.device):
        check(_lib.lib().gwtf_approx_match(_ptr(seta, 'seta'), _ptr(setb, 'setb'), _ptr(match, 'match'),
                                           _ptr(temp, 'temp'), b, n, m, _stream(seta)))
    return match, temp


class MatchCostFunction(Function):
    """match_cost.py:5-43: cost (b,) of the approximate matching; the matching is treated as constant in backward."""

    @staticmethod
    def forward(ctx, seta, setb):
        b, n, m = _sets(seta, setb)
        cost = torch.empty(b, device=seta.device, dtype=torch.float32)
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            # evaluation (the reference's only use, evaluation_metrics.py:25-30): the fused schedule, no (b,m,n) matrix
            temp = torch.empty(b, (n + m) * 2, device=seta.device, dtype=torch.float32)
            with torch.cuda.device(seta.device):
                check(_lib.lib().gwtf_emd_cost(_ptr(seta, 'seta'), _ptr(setb, 'setb'), _ptr(temp, 'temp'),
                                               _ptr(cost, 'cost'), b, n, m, _stream(seta)))
            return cost
        match, _ = approx_match(seta, setb)
        with torch.cuda.device(seta.device):
            check(_lib.lib().gwtf_match_cost(_ptr(seta, 'seta'), _ptr(setb, 'setb'), _ptr(match, 'match'),
                                             _ptr(cost, 'cost'), b, n, m, _stream(seta)))
        ctx.save_for_backward(seta, setb)
        ctx.match = match
        return cost

    @staticmethod
    def backward(ctx, grad_output):
        seta, setb = ctx.saved_tensors
        b, n, m = _sets(seta, setb)
        grada, gradb = torch.empty_like(seta), torch.empty_like(setb)
        with torch.cuda.device(seta.device):
            check(_lib.lib().gwtf_match_cost_grad(_ptr(seta, 'seta'), _ptr(setb, 'setb'), _ptr(ctx.match, 'match'),
                                                  _ptr(grada, 'grada'), _ptr(gradb, 'gradb'), b, n, m, _stream(seta)))
        g = grad_output.unsqueeze(1).unsqueeze(2)
        return grada * g, gradb * g


match_cost = MatchCostFunction.apply


def _cloud_sets(a, b, na, nb):
    """The checks of _sets for two sets of clouds that need not agree in cloud count: (na, n), (nb, m)."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3:
        raise GwtfError(f'cloud sets must be (nq,n,3) and (nt,m,3): got {tuple(a.shape)} and {tuple(b.shape)}')
    _ptr(a, na), _ptr(b, nb)
    if min(a.shape[0], a.shape[1], b.shape[0], b.shape[1]) == 0:
        raise GwtfError('empty point set')


MAX_THRESHOLDS = 8      # per gwtf_chamfer_directed call (the thresholds travel as a kernel argument)


def chamfer_directed(q, t, thresholds=()):
    """Every cloud of ``q`` (nq,n,3) against every cloud of ``t`` (nt,m,3), one direction, reduced on the device:
    sum (nq,nt) float32 = sum over the points of q_i of the squared distance to the nearest point of t_j (the minimum is
    nn_distance's dist1, bit for bit), cnt (T,nq,nt) int32 = how many of those minima are < thresholds[h], compared in
    float32.  No (pairs, n) intermediate and no expanded copy of either set; repeated calls give identical bits."""
    _cloud_sets(q, t, 'q', 't')
    nq, n, nt, m = q.shape[0], q.shape[1], t.shape[0], t.shape[1]
    thr = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    dev = q.device
    out = torch.empty(nq, nt, device=dev, dtype=torch.float32)
    cnt = torch.empty(len(thr), nq, nt, device=dev, dtype=torch.int32)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for h0 in range(0, max(len(thr), 1), MAX_THRESHOLDS):      # more than 8 thresholds: further passes
            part = np.ascontiguousarray(thr[h0:h0 + MAX_THRESHOLDS])
            check(L.gwtf_chamfer_directed(_ptr(q, 'q'), _ptr(t, 't'), out.data_ptr(), cnt[h0:].data_ptr() if len(part) else None,
                                          part.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if len(part) else None, len(part),
                                          nq, nt, n, m, _stream(q)))
    return out, cnt


MAX_PAIRS_PER_LAUNCH = 65535      # gwtf_emd_cost_pairs: the pair index is a grid's second dimension


def emd_cost_pairs(a, b, max_temp_bytes=256 << 20):
    """Fused approximate-matching cost (what match_cost returns when no gradient is wanted) of every cloud of ``a`` (na,n,3)
    against every cloud of ``b`` (nb,m,3): (na,nb) float32, not normalised.  No expanded copies; the rows of the result are
    walked in blocks whose (pairs, 2(n+m)) scratch stays within ``max_temp_bytes`` (at least one row per block)."""
    _cloud_sets(a, b, 'a', 'b')
    na, n, nb, m = a.shape[0], a.shape[1], b.shape[0], b.shape[1]
    if nb > MAX_PAIRS_PER_LAUNCH:
        raise GwtfError(f'emd_cost_pairs: at most {MAX_PAIRS_PER_LAUNCH} clouds in b (got {nb}); split b')
    per_row = nb * 2 * (n + m)                                    # floats of scratch per row of the result
    rows = max(1, min(na, int(max_temp_bytes) // (4 * per_row), MAX_PAIRS_PER_LAUNCH // nb))
    out = torch.empty(na, nb, device=a.device, dtype=torch.float32)
    temp = torch.empty(rows * per_row, device=a.device, dtype=torch.float32)
    L = _lib.lib()
    with torch.cuda.device(a.device):
        for row0 in range(0, na, rows):
            r = min(rows, na - row0)
            check(L.gwtf_emd_cost_pairs(_ptr(a, 'a'), _ptr(b, 'b'), _ptr(temp, 'temp'), out[row0:].data_ptr(), na, nb, n, m,
                                        row0, r, _stream(a)))
    return out


def distChamferCUDA(x, y):
    """evaluation_metrics.py:21-22 / utils.py:34-35 (name kept so the reference's callers need no edit)."""
    return nn_distance(x, y)


def emd_approx(sample, ref):
    """evaluation_metrics.py:25-30: approximate EMD per cloud, normalised by the number of points."""
    N, N_ref = sample.size(1), ref.size(1)
    assert N == N_ref, "Not sure what would EMD do in this case"
    return match_cost(sample, ref) / float(N)


def f_score(predicted_clouds, true_clouds, threshold=0.001):
    """utils.py:38-42."""
    ld, rd = distChamferCUDA(predicted_clouds, true_clouds)
    precision = 100. * (rd < threshold).float().mean(1)
    recall = 100. * (ld < threshold).float().mean(1)
    return 2. * precision * recall / (precision + recall + 1e-7)


# ---- paired evaluation: the frame of the metrics, cloud i against cloud i (csrc/gwtf_metrics.hip) ---------------------------------
class EvalFrame:
    """The rescaling statements the reference's evaluate applies to the generated and the reference clouds before its metrics
    (evaluating.py:100-120), as the record the frame kernel takes: ``n_scale`` multiplications by float32(``scale``), the float64
    translation ``shift``, the per-shape ``row_scale`` (*= orig_s) and ``row_shift`` (+= orig_c).  The default is the identity."""

    def __init__(self, n_scale=0, scale=1.0, translate=False, shift=(0.0, 0.0, 0.0), row_scale=False, row_shift=False):
        if isinstance(n_scale, bool) or int(n_scale) != n_scale or not 0 <= int(n_scale) <= 2:
            raise ValueError(f'n_scale must be 0, 1 or 2 (one multiplication per evaluation flag), got {n_scale!r}')
        self.n_scale = int(n_scale)
        self.scale = float(np.float32(scale)) if self.n_scale else 1.0
        self.translate, self.row_scale, self.row_shift = bool(translate), bool(row_scale), bool(row_shift)
        shift = np.asarray(shift if self.translate else (0.0, 0.0, 0.0), np.float64).reshape(-1)     # float64, as evaluating.py:111 builds it
        if shift.size != 3:
            raise ValueError('cloud_translate_shift must hold three values')
        self.shift = tuple(float(v) for v in shift)

    @classmethod
    def from_config(cls, **kwargs):
        """From the reference's config keys (evaluating.py:101-120); keys it does not know (the rest of a config file) are ignored.
        unit_scale_evaluation and orig_scale_evaluation each multiply by cloud_scale_scale when cloud_scale is on -- both set: twice,
        as the reference does; the translation and the two per-shape steps belong to orig_scale_evaluation alone."""
        g = kwargs.get
        orig = bool(g('orig_scale_evaluation'))
        n_scale = (int(bool(g('unit_scale_evaluation'))) + int(orig)) if g('cloud_scale') else 0
        return cls(n_scale=n_scale, scale=g('cloud_scale_scale') or 1.0, translate=orig and bool(g('cloud_translate')),
                   shift=g('cloud_translate_shift') or (0.0, 0.0, 0.0), row_scale=orig and not g('cloud_rescale2orig'),
                   row_shift=orig and not g('cloud_recenter2orig'))

    def statements(self):
        """The in-place statements in the order they run: ('mul', float32 scale), ('add64', (sx, sy, sz)), ('mul_rows', 'orig_s'),
        ('add_rows', 'orig_c')."""
        out = [('mul', self.scale)] * self.n_scale
        if self.translate:
            out.append(('add64', self.shift))
        if self.row_scale:
            out.append(('mul_rows', 'orig_s'))
        if self.row_shift:
            out.append(('add_rows', 'orig_c'))
        return out


_IDENTITY_FRAME = EvalFrame()


def _channel_major(gen, ref):
    for t, name in ((gen, 'gen'), (ref, 'ref')):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1] != 3:
            raise GwtfError(f'{name} must be a (B,3,n) tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}')
    if gen.shape[0] != ref.shape[0]:
        raise GwtfError(f'gen and ref must hold the same number of clouds: got {gen.shape[0]} and {ref.shape[0]}')
    if min(gen.shape[0], gen.shape[2], ref.shape[2]) == 0:
        raise GwtfError('empty point set')
    if gen.shape[0] > MAX_PAIRS_PER_LAUNCH:
        raise GwtfError(f'at most {MAX_PAIRS_PER_LAUNCH} clouds per call (got {gen.shape[0]})')
    _ptr(gen, 'gen'), _ptr(ref, 'ref')
    if gen.device != ref.device:
        raise GwtfError('gen and ref must live on one device')
    return gen.shape[0], gen.shape[2], ref.shape[2]


def clouds_to_eval_frame(gen, ref, frame=None, orig_s=None, orig_c=None, out=None):
    """``gen`` (B,3,n) and ``ref`` (B,3,m), channel-major as the model and the loaders produce them, through the statements of
    ``frame`` (EvalFrame; None: the identity) -> (gen_out (B,n,3), ref_out (B,m,3)), point-major as the metric kernels take them: one
    launch for both sets, no transpose().contiguous() copy.  Every statement rounds as torch's in-place op rounds it (the float64
    translation is added in float64 and rounded once), so the result is the reference's, bit for bit.  ``orig_s`` (B,) and ``orig_c``
    (B,3): float32 tensors on the clouds' device (what MeshStore holds and the loaders yield), needed when the frame scales or shifts
    per shape.  ``out``: (gen_out, ref_out) to write into.  The inputs are NOT modified (the reference scales them in place)."""
    B, n, m = _channel_major(gen, ref)
    f = frame if frame is not None else _IDENTITY_FRAME
    if not isinstance(f, EvalFrame):
        raise GwtfError(f'frame must be an EvalFrame, got {type(frame)}')
    dev = gen.device
    if f.row_scale and orig_s is None:
        raise GwtfError('the frame multiplies by orig_s but the batch has none')
    if f.row_shift and orig_c is None:
        raise GwtfError('the frame adds orig_c but the batch has none')
    ps = _lib._explicit(orig_s, 'orig_s', (B,), torch.float32, dev) if f.row_scale else None
    pc = _lib._explicit(orig_c, 'orig_c', (B, 3), torch.float32, dev) if f.row_shift else None
    if out is None:
        out = (torch.empty(B, n, 3, device=dev, dtype=torch.float32), torch.empty(B, m, 3, device=dev, dtype=torch.float32))
    go, ro = out
    a = _lib.EvalFrameArgs(gen=gen.data_ptr(), ref=ref.data_ptr(), orig_s=ps, orig_c=pc,
                           gen_out=_lib._explicit(go, 'out[0]', (B, n, 3), torch.float32, dev),
                           ref_out=_lib._explicit(ro, 'out[1]', (B, m, 3), torch.float32, dev), B=B, n=n, m=m, n_scale=f.n_scale,
                           translate=int(f.translate), row_scale=int(f.row_scale), row_shift=int(f.row_shift), scale=f.scale,
                           stream=_stream(gen))
    a.shift[:] = f.shift
    with torch.cuda.device(dev):
        check(_lib.lib().gwtf_eval_frame(ctypes.addressof(a)))
    return go, ro


PAIRED_WORDS = 1 + MAX_THRESHOLDS     # words of one partial of gwtf_chamfer_paired: a float32 sum, then int32 counts


def _thr_array(thresholds):
    thr = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    return thr, [np.ascontiguousarray(thr[h0:h0 + MAX_THRESHOLDS]) for h0 in range(0, max(len(thr), 1), MAX_THRESHOLDS)]


def _paired_sets(a, b):
    B, n, m = _sets(a, b)
    if a.device != b.device:
        raise GwtfError('both cloud sets must live on one device')
    if B > MAX_PAIRS_PER_LAUNCH:
        raise GwtfError(f'at most {MAX_PAIRS_PER_LAUNCH} pairs per call (got {B})')
    return B, n, m


def _chamfer_paired_launch(L, a, b, partials, part, B, n, m):
    check(L.gwtf_chamfer_paired(a.data_ptr(), b.data_ptr(), partials.data_ptr(),
                                part.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if len(part) else None, len(part), B, n, m,
                                _stream(a)))


def chamfer_paired(a, b, thresholds=()):
    """Cloud i of ``a`` (B,n,3) against cloud i of ``b`` (B,m,3), both directions in one launch, reduced on the device ->
    (sum_l (B,), sum_r (B,), cnt_l (T,B), cnt_r (T,B)): sum_l[i] = sum over the points of a_i of the squared distance to the nearest
    point of b_i (the minimum is nn_distance's dist1, bit for bit), sum_r the other direction (dist2); cnt_*[h][i] int32 = how many of
    those minima are < thresholds[h], compared in float32.  No (B, n) intermediate; repeated calls give identical bits.  The kernel
    leaves one partial per chunk of query points; here they are added by torch (paired_metrics adds them in its own launch)."""
    B, n, m = _paired_sets(a, b)
    thr, parts = _thr_array(thresholds)
    L, dev = _lib.lib(), a.device
    P = L.gwtf_chamfer_paired_partials(n, m)
    sums, cnts = None, []
    with torch.cuda.device(dev):
        for part in parts:                                              # more than 8 thresholds: further passes
            partials = torch.zeros(2, B, P, PAIRED_WORDS, device=dev, dtype=torch.float32)      # chunks no workgroup writes stay 0
            _chamfer_paired_launch(L, a, b, partials, part, B, n, m)
            if sums is None:
                sums = partials[..., 0].sum(-1)
            cnts.append(partials.view(torch.int32)[..., 1:1 + len(part)].sum(2, dtype=torch.int32).permute(2, 0, 1))
    cnt = torch.cat(cnts, 0)                                            # (T, 2, B)
    return sums[0], sums[1], cnt[:, 0].contiguous(), cnt[:, 1].contiguous()


METER_HEAD = 3        # a meter is [count, sum of CD, sum of EMD, sum of F1 per threshold ...] in float64


def new_meter(n_thresholds=0, device='cuda'):
    """A zeroed meter for paired_metrics: float64 [count, sum CD, sum EMD, sum F1[0], ...] on the device."""
    return torch.zeros(METER_HEAD + max(MAX_THRESHOLDS, int(n_thresholds)), device=device, dtype=torch.float64)


def paired_metrics(a, b, f1_thresholds=(), cd=True, emd=True, meter=None):
    """The per-pair metrics of the autoencoding / reconstruction evaluation (EMD_CD_F1, evaluation_metrics.py:47-107; the loop of
    evaluating.py:138-157) for cloud i of ``a`` (B,n,3) against cloud i of ``b`` (B,m,3) -> {'CD', 'CDL', 'CDR' (cd), 'EMD' (emd),
    'F1': {threshold: (B,)}}, float32 (B,) tensors on the device.  ONE Chamfer pass serves CD and every threshold (f_score runs one
    pass per threshold); EMD is the existing fused matching cost (gwtf_emd_cost) and needs n == m.  ``meter`` (new_meter): the
    per-pair values are also added, in float64 and on the device, to [count, sum CD, sum EMD, sum F1 per threshold]; nothing is
    synchronised or read back, and after one eager call the same call can be captured in a graph."""
    B, n, m = _paired_sets(a, b)
    f1_thresholds = tuple(f1_thresholds)
    thr, parts = _thr_array(f1_thresholds)
    T, dev = len(thr), a.device
    if emd and n != m:
        raise GwtfError(f'EMD needs clouds of equal size (emd_approx): got {n} and {m} points')
    if meter is not None and (not torch.is_tensor(meter) or meter.dtype != torch.float64 or meter.device != dev or meter.dim() != 1
                              or meter.numel() < METER_HEAD + max(T, MAX_THRESHOLDS) or not meter.is_contiguous()):
        raise GwtfError(f'meter must be a contiguous float64 tensor of at least {METER_HEAD + max(T, MAX_THRESHOLDS)} values on {dev} '
                        '(new_meter)')
    L = _lib.lib()
    f32 = dict(device=dev, dtype=torch.float32)
    P = L.gwtf_chamfer_paired_partials(n, m)
    partials = torch.empty(2 * B * P * PAIRED_WORDS, **f32)
    vals = torch.empty(4 + T, B, **f32)                                 # CD, CDL, CDR, EMD, F1 per threshold
    out = {}
    with torch.cuda.device(dev):
        cost = None
        if emd:
            cost, temp = torch.empty(B, **f32), torch.empty(B, (n + m) * 2, **f32)
            check(L.gwtf_emd_cost(a.data_ptr(), b.data_ptr(), temp.data_ptr(), cost.data_ptr(), B, n, m, _stream(a)))
        for k, part in enumerate(parts):                                # more than 8 thresholds: further passes over slices
            h0, first = k * MAX_THRESHOLDS, k == 0
            _chamfer_paired_launch(L, a, b, partials, part, B, n, m)
            check(L.gwtf_paired_finalise(
                partials.data_ptr(), cost.data_ptr() if emd and first else None,
                vals[0].data_ptr() if cd and first else None, vals[1].data_ptr() if cd and first else None,
                vals[2].data_ptr() if cd and first else None, vals[3].data_ptr() if emd and first else None,
                vals[4 + h0:].data_ptr() if len(part) else None, None if meter is None else meter.data_ptr() + 8 * h0,
                int(first), len(part), B, n, m, _stream(a)))
    if cd:
        out.update(CD=vals[0], CDL=vals[1], CDR=vals[2])
    if emd:
        out['EMD'] = vals[3]
    out['F1'] = {t: vals[4 + h] for h, t in enumerate(f1_thresholds)}
    return out


# ---- occupancy histogram and Jensen-Shannon divergence (csrc/gwtf_occupancy.hip) ---------------------------------------------------
OCC_MAX_RES = 32                      # the workgroup's private histogram of res^3 uint32 bins lives in LDS
OCC_POINTS_PER_WORKGROUP = 8192       # kPointsPerGroup of csrc/gwtf_occupancy.hip: one workgroup per this many points, CUs at most


def occupancy_edges(res):
    """The reference's edge table (utils.py:56): the one statement of where a bin ends, for the host path and the kernel alike."""
    return -0.5 + np.arange(res + 1) * (1. / res)


def _int64_on(t, name, shape, device):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != torch.int64 or t.device != device or not t.is_contiguous():
        raise GwtfError(f'{name} must be a contiguous int64 tensor of shape {tuple(shape)} on {device}')
    return t


def voxel_occupancy(clouds, res=28, bound=0.5, out=None, stats=None):
    """How many points of ``clouds`` ((..., 3) float32, contiguous, on a HIP device) fall into each cell of the res^3 grid over
    [-0.5, 0.5)^3 -> counts (res, res, res) int64 on the device: get_voxel_occ_dist's histogram before its normalisation (reference
    utils.py:45-79), by the reference's rule -- coordinate x is in bin k iff edges[k] <= x < edges[k + 1], compared in float64; NaN,
    +-inf and anything outside the cube have no bin, and a point counts when all three coordinates have one.
    out: a (res, res, res) int64 tensor to ADD to (a set folded in batch by batch); stats: a (2,) int64 tensor to add
    #{values with |x| > bound} and #{NaN values} to.  Integer counts: the same call gives the same bits.  Nothing is synchronised or
    read back."""
    if isinstance(res, bool) or not isinstance(res, (int, np.integer)) or not 1 <= res <= OCC_MAX_RES:
        raise GwtfError(f'res must be an integer in 1..{OCC_MAX_RES}, got {res!r}')
    if not torch.is_tensor(clouds) or clouds.dim() < 1 or clouds.shape[-1] != 3:
        raise GwtfError(f'clouds must be a (..., 3) tensor, got {tuple(clouds.shape) if torch.is_tensor(clouds) else type(clouds)}')
    ptr = _ptr(clouds, 'clouds')
    n_points = clouds.numel() // 3
    if n_points == 0:
        raise GwtfError('empty point set')
    if not float(bound) >= 0.0:
        raise GwtfError(f'bound must be >= 0, got {bound!r}')
    res, dev = int(res), clouds.device
    if out is None:
        out = torch.zeros(res, res, res, device=dev, dtype=torch.int64)
    _int64_on(out, 'out', (res, res, res), dev)
    if stats is not None:
        _int64_on(stats, 'stats', (2,), dev)
    a = _lib.OccupancyArgs(points=ptr, n_points=n_points, res=res, bound=float(bound), counts=out.data_ptr(),
                           stats=None if stats is None else stats.data_ptr(), stream=_stream(clouds))
    a.edges[:res + 1] = occupancy_edges(res).tolist()
    with torch.cuda.device(dev):
        check(_lib.lib().gwtf_voxel_occupancy(ctypes.addressof(a)))
    return out


def jsd_from_counts(c1, c2):
    """Jensen-Shannon divergence (base 2) of two occupancy histograms given as int64 counts of equal size on a HIP device
    (reference utils.py:82-86 on counts / counts.sum()) -> 0-d float64 device tensor.  float64 throughout and a fixed summation
    order: the same counts give the same bits.  A histogram without a single count gives NaN (the reference's 0 / 0).  Nothing is
    synchronised or read back."""
    for t, name in ((c1, 'c1'), (c2, 'c2')):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise GwtfError(f'{name} must live on a HIP device; there is no CPU path')
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise GwtfError(f'{name} must be a contiguous int64 tensor')
    if c1.numel() != c2.numel() or c1.device != c2.device or not 1 <= c1.numel() < 2 ** 31:
        raise GwtfError(f'the histograms must have the same number of bins on one device: got {tuple(c1.shape)} and {tuple(c2.shape)}')
    out = torch.empty((), device=c1.device, dtype=torch.float64)
    with torch.cuda.device(c1.device):
        check(_lib.lib().gwtf_jsd_counts(c1.data_ptr(), c2.data_ptr(), c1.numel(), out.data_ptr(), _stream(c1)))
    return out
