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
