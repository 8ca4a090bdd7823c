"""Train-mode ``BatchNorm2d`` fused with the operators that follow it in the image encoder (csrc/gwtf_norm2d.hip):

    norm_act_2d(x, bn)                      relu(bn(x))
    norm_act_2d(x, bn, residual=r)          relu(bn(x) + r)              the BasicBlock tail
    norm_act_2d(x, bn, relu=False)          bn(x)                        the downsample branch
    norm_act_2d(x, bn, pool=True)           maxpool3x3/2/1(relu(bn(x)))  the stem; the full-size activation is never stored

with batch statistics, the in-place update of ``bn.running_mean`` / ``running_var`` / ``num_batches_tracked`` and the gradients of
``nn.BatchNorm2d`` in train mode.  Contiguous NCHW float32 on a HIP device only; anything else raises GwtfError -- there is no
fallback.  Every workspace is a torch allocation made in ``forward`` / ``backward`` and nothing is read back to the host, so a call
can be captured in a graph.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import GwtfError, check

E_FEW_VALUES = 10003          # GWTF_E_FEW_VALUES of include/gwtf.h


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


def _check(x, weight, bias, residual, running_mean, running_var, relu, pool):
    """Every refusal, before any device work."""
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
    if N * H * W < 2:
        raise GwtfError('norm_act_2d: ' + _lib.lib().gwtf_error_string(E_FEW_VALUES).decode() + f' (got input size {tuple(x.shape)})')
    S = _lib.lib().gwtf_norm2d_partials(N, C, H, W)
    if S < 1:
        raise GwtfError(f'norm_act_2d: size {tuple(x.shape)} is outside what the kernels take')
    return S


class NormAct2dFn(torch.autograd.Function):
    """(x, weight, bias, residual or None, running_mean, running_var, eps, momentum, relu, pool) -> (y, stats, offsets).
    stats (3, C): batch mean, rstd and the part of the mean its float lost; offsets: the uint8 window offsets with pool, else None.
    Only y carries a gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, eps, momentum, relu, pool):
        relu, pool = bool(relu), bool(pool)
        S = _check(x, weight, bias, residual, running_mean, running_var, relu, pool)
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
        with torch.cuda.device(dev):
            check(_lib.lib().gwtf_norm2d_forward(ctypes.addressof(a)))
        torch._C._increment_version([running_mean, running_var])      # written through raw pointers
        ctx.save_for_backward(x, weight, bias, y if relu and not pool else None, stats, offsets)
        ctx.cfg = (float(eps), float(momentum), relu, pool, residual is not None, S)
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
        with torch.cuda.device(dev):
            check(_lib.lib().gwtf_norm2d_backward(ctypes.addressof(a)))
        return dx, dgamma, dbeta, d_res, None, None, None, None, None, None


def norm_act_2d(x, bn, residual=None, relu=True, pool=False):
    """The fused layer on the parameters and buffers of ``bn`` (an ``nn.BatchNorm2d`` in train mode)."""
    if isinstance(bn, nn.SyncBatchNorm):
        raise GwtfError('norm_act_2d: SyncBatchNorm is not built (single-rank batch statistics only)')
    if not isinstance(bn, nn.BatchNorm2d):
        raise GwtfError(f'norm_act_2d takes an nn.BatchNorm2d, got {type(bn).__name__}')
    if not bn.affine or bn.weight is None or bn.bias is None:
        raise GwtfError('norm_act_2d: BatchNorm2d without affine parameters is not taken')
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        raise GwtfError('norm_act_2d: track_running_stats=False is not taken')
    if bn.momentum is None:
        raise GwtfError('norm_act_2d: momentum=None (cumulative average) is not taken')
    if not bn.training:
        raise GwtfError('norm_act_2d computes batch statistics: the BatchNorm2d must be in train mode')
    y, _, _ = NormAct2dFn.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu, pool)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return y
