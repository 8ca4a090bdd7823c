"""Train-mode ``BatchNorm2d`` fused with the operators that follow it in the image encoder (csrc/gwtf_norm2d.hip):

    norm_act_2d(x, bn)                      relu(bn(x))
    norm_act_2d(x, bn, residual=r)          relu(bn(x) + r)              the BasicBlock tail
    norm_act_2d(x, bn, relu=False)          bn(x)                        the downsample branch
    norm_act_2d(x, bn, pool=True)           maxpool3x3/2/1(relu(bn(x)))  the stem; the full-size activation is never stored

with batch statistics, the in-place update of ``bn.running_mean`` / ``running_var`` / ``num_batches_tracked`` and the gradients of
``nn.BatchNorm2d`` in train mode.  Contiguous NCHW float32 on a HIP device only; anything else raises GwtfError -- there is no
fallback.  Every workspace is a torch allocation made in ``forward`` / ``backward`` and nothing is read back to the host, so a call
can be captured in a graph.

In a data-parallel run (``dist.sharded()``) an ``nn.SyncBatchNorm`` is taken: the statistics cover the images of all ranks.  Each
direction then runs sums -> ONE all-reduce of the (C, 2) float64 sums -> apply (gwtf_norm2d_*_sums / _apply), with the number of
values per channel taken from ``dist.row_layout``.  The gradients of weight and bias stay rank-local, as torch's SyncBatchNorm leaves
them: the ordinary gradient exchange sums them.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import GwtfError, check

E_FEW_VALUES = 10003          # GWTF_E_FEW_VALUES of include/gwtf.h
COLLECTIVES = {'n': 0}        # statistic all-reduces issued by NormAct2dFn (tests assert the count)


def global_count(N, H, W, device):
    """Values per channel over the (N_r, C, H, W) inputs of all ranks, this rank holding N: the rows of ``dist.row_layout`` times
    H * W.  A collective outside a capture, the warm-up step's layout inside one."""
    from .dist import row_layout
    return row_layout(int(N), device).total * int(H) * int(W)


def _sum_over_ranks(sums):
    """In place.  Issued on a 1-rank group too (GWTF_FORCE_SHARDED=1 runs the collective over RCCL on one GPU)."""
    import torch.distributed as td
    from .dist import run
    COLLECTIVES['n'] += 1
    run(td.all_reduce, sums, op=td.ReduceOp.SUM)


def pooled_size(n):
    """Output length of MaxPool2d(3, stride 2, padding 1) along an axis of n."""
    return (n - 1) // 2 + 1


def _device_f32(t, name, like=None):
    """dtype, then layout, then device: the order the refusals are reported in."""
    if not isinstance(t, torch.Tensor):
        raise GwtfError(f'{name} must be a tensor, got {type(t).__name__}')
    if t.dtype != torch.float32:
        raise GwtfError(f'{name} must be float32 (got {t.dtype})')
    if not t.is_contiguous():
        raise GwtfError(f'{name} must be contiguous NCHW (channels_last and strided views are not taken)')
    if not t.is_cuda:
        raise GwtfError(f'{name} must live on a HIP device (got {t.device}); there is no CPU path')
    if like is not None and t.device != like.device:
        raise GwtfError(f'{name} on {t.device}, the input on {like.device}')
    return t


def _check(x, weight, bias, residual, running_mean, running_var, relu, pool, count=None):
    """Every refusal, before any device work.  count: values per channel over all ranks (None: this rank's are all there are)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise GwtfError('norm_act_2d input must be a (N, C, H, W) tensor')
    if residual is not None and (not isinstance(residual, torch.Tensor) or tuple(residual.shape) != tuple(x.shape)):
        raise GwtfError(f'residual is {tuple(getattr(residual, "shape", ()))}, expected {tuple(x.shape)}')
    if pool and (not relu or residual is not None):
        raise GwtfError('pool=True is the stem: with relu and without a residual')
    _device_f32(x, 'x')
    C = x.shape[1]
    for t, name in ((weight, 'weight'), (bias, 'bias'), (running_mean, 'running_mean'), (running_var, 'running_var')):
        if t is None:
            raise GwtfError(f'norm_act_2d needs {name} (affine BatchNorm2d that tracks running statistics)')
        _device_f32(t, name, x)
        if tuple(t.shape) != (C,):
            raise GwtfError(f'{name} is {tuple(t.shape)}, expected ({C},)')
    if residual is not None:
        _device_f32(residual, 'residual', x)
    N, _, H, W = x.shape
    if (N * H * W if count is None else count) < 2:
        raise GwtfError('norm_act_2d: ' + _lib.lib().gwtf_error_string(E_FEW_VALUES).decode() + f' (got input size {tuple(x.shape)})')
    if count is not None and count < N * H * W:
        raise GwtfError(f'norm_act_2d: {count} values per channel over all ranks, {N * H * W} of them here')
    # (one value per channel on this rank, more elsewhere: one partial; the size query refuses what a single rank cannot normalise)
    S = 1 if N * H * W == 1 else _lib.lib().gwtf_norm2d_partials(N, C, H, W)
    if S < 1:
        raise GwtfError(f'norm_act_2d: size {tuple(x.shape)} is outside what the kernels take')
    return S


class NormAct2dFn(torch.autograd.Function):
    """(x, weight, bias, residual or None, running_mean, running_var, eps, momentum, relu, pool) -> (y, stats, offsets).
    stats (3, C): batch mean, rstd and the part of the mean its float lost; offsets: the uint8 window offsets with pool, else None.
    Only y carries a gradient.  An eleventh argument, count = the values per channel over ALL ranks (global_count), makes the
    statistics global: sums, one all-reduce, apply in each direction; weight and bias get their rank-local gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, eps, momentum, relu, pool, count=None):
        relu, pool = bool(relu), bool(pool)
        S = _check(x, weight, bias, residual, running_mean, running_var, relu, pool, count)
        N, C, H, W = x.shape
        dev = x.device
        y = torch.empty((N, C, pooled_size(H), pooled_size(W)) if pool else (N, C, H, W), device=dev, dtype=torch.float32)
        offsets = torch.empty(y.shape, device=dev, dtype=torch.uint8) if pool else None
        stats = torch.empty(3, C, device=dev, dtype=torch.float32)
        partials = torch.empty(C, S, 2, device=dev, dtype=torch.float64)
        at = lambda t: None if t is None else t.data_ptr()
        a = _lib.Norm2dArgs(x=at(x), residual=at(residual), gamma=at(weight), beta=at(bias), running_mean=at(running_mean),
                            running_var=at(running_var), y=at(y), offsets=at(offsets), stats=at(stats), partials=at(partials),
                            N=N, C=C, H=H, W=W, relu=int(relu), pool=int(pool), eps=float(eps), momentum=float(momentum),
                            stream=torch.cuda.current_stream(dev).cuda_stream)
        L = _lib.lib()
        with torch.cuda.device(dev):
            if count is None:
                check(L.gwtf_norm2d_forward(ctypes.addressof(a)))
            else:
                sums = torch.empty(C, 2, device=dev, dtype=torch.float64)
                check(L.gwtf_norm2d_forward_sums(ctypes.addressof(a), sums.data_ptr()))
                _sum_over_ranks(sums)
                check(L.gwtf_norm2d_forward_apply(ctypes.addressof(a), sums.data_ptr(), float(count)))
        torch._C._increment_version([running_mean, running_var])      # written through raw pointers
        ctx.save_for_backward(x, weight, bias, y if relu and not pool else None, stats, offsets)
        ctx.cfg = (float(eps), float(momentum), relu, pool, residual is not None, S)
        ctx.count = count
        ctx.mark_non_differentiable(stats)
        if offsets is not None:
            ctx.mark_non_differentiable(offsets)
        return y, stats, offsets

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gstats, _goffsets):
        x, weight, bias, y, stats, offsets = ctx.saved_tensors
        eps, momentum, relu, pool, has_residual, S = ctx.cfg
        N, C, H, W = x.shape
        dev = x.device
        gy = _device_f32(gy.contiguous(), 'grad_output', x)
        dx = torch.empty_like(x)
        d_res = torch.empty_like(x) if has_residual and ctx.needs_input_grad[3] else None
        dgamma = torch.empty(C, device=dev, dtype=torch.float32)
        dbeta = torch.empty(C, device=dev, dtype=torch.float32)
        partials = torch.empty(C, S, 2, device=dev, dtype=torch.float64)
        at = lambda t: None if t is None else t.data_ptr()
        a = _lib.Norm2dArgs(x=at(x), gamma=at(weight), beta=at(bias), y=at(y), offsets=at(offsets), stats=at(stats),
                            partials=at(partials), dy=at(gy), dx=at(dx), d_residual=at(d_res), dgamma=at(dgamma), dbeta=at(dbeta),
                            N=N, C=C, H=H, W=W, relu=int(relu), pool=int(pool), eps=eps, momentum=momentum,
                            stream=torch.cuda.current_stream(dev).cuda_stream)
        L = _lib.lib()
        with torch.cuda.device(dev):
            if ctx.count is None:
                check(L.gwtf_norm2d_backward(ctypes.addressof(a)))
            else:
                sums = torch.empty(C, 2, device=dev, dtype=torch.float64)
                check(L.gwtf_norm2d_backward_sums(ctypes.addressof(a), sums.data_ptr()))
                _sum_over_ranks(sums)
                check(L.gwtf_norm2d_backward_apply(ctypes.addressof(a), sums.data_ptr(), float(ctx.count)))
        return (dx, dgamma, dbeta, d_res) + (None,) * (len(ctx.needs_input_grad) - 4)


def norm_act_2d(x, bn, residual=None, relu=True, pool=False):
    """The fused layer on the parameters and buffers of ``bn``: an ``nn.BatchNorm2d`` in train mode, or -- in a data-parallel run
    (dist.sharded()) -- an ``nn.SyncBatchNorm``, whose statistics then cover the images of all ranks."""
    sync = isinstance(bn, nn.SyncBatchNorm)
    if sync:
        from .dist import sharded
        if not sharded():
            raise GwtfError('norm_act_2d: SyncBatchNorm needs a data-parallel run (an initialised process group with more than one '
                            'rank, or GWTF_FORCE_SHARDED=1); convert the module back to BatchNorm2d for a single-rank run')
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise GwtfError('norm_act_2d input must be a (N, C, H, W) tensor')
    elif not isinstance(bn, nn.BatchNorm2d):
        raise GwtfError(f'norm_act_2d takes an nn.BatchNorm2d, got {type(bn).__name__}')
    if not bn.affine or bn.weight is None or bn.bias is None:
        raise GwtfError('norm_act_2d: BatchNorm2d without affine parameters is not taken')
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        raise GwtfError('norm_act_2d: track_running_stats=False is not taken')
    if bn.momentum is None:
        raise GwtfError('norm_act_2d: momentum=None (cumulative average) is not taken')
    if not bn.training:
        raise GwtfError('norm_act_2d computes batch statistics: the BatchNorm2d must be in train mode')
    if sync:
        N, _, H, W = x.shape
        y, _, _ = NormAct2dFn.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu, pool,
                                    global_count(N, H, W, x.device))
    else:
        y, _, _ = NormAct2dFn.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu, pool)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return y
