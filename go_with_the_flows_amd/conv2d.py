"""The convolutions of the image encoder in train mode on csrc/gwtf_conv2d.hip: forward, gradient of the input, gradient of the weight.

    conv2d(x, conv)          conv(x) for a bias-free ``nn.Conv2d`` with groups 1, dilation 1, padding k // 2

``x`` is contiguous NCHW float32 on a HIP device and so is the result -- the layout norm2d.norm_act_2d takes, so nothing is
transposed between the two.  The weight stays in torch's (Cout, Cin, k, k) parameter layout: ``state_dict``, the optimiser and the
gradient exchange see the same tensors as with the library.  Geometry the kernels take: k in {1, 3, 7}, stride in {1, 2}, Cout a
multiple of 16, Cin a multiple of 16 (or 4 with k = 7, the stem).  Anything else raises GwtfError -- there is no fallback.

Products are exact fp32 and no pass uses atomics: two calls give the same bits.  Every workspace is a torch allocation sized by
the host-only planner and nothing is read back to the host, so a call can be captured in a graph.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import GwtfError, check
from .norm2d import _device_f32


def _record(x_shape, w_shape, stride, pad, **pointers):
    N, Cin, H, W = x_shape
    Cout, _, k, _ = w_shape
    return _lib.Conv2dArgs(N=N, Cin=Cin, H=H, W=W, Cout=Cout, k=k, stride=stride, pad=pad, **pointers)


def plan(a, which):
    """(splits, work_floats) of pass `which` (_lib.CONV2D_*) for the record `a`; raises GwtfError where the launch would refuse.
    Host only."""
    splits, floats = ctypes.c_int(0), ctypes.c_size_t(0)
    check(_lib.lib().gwtf_conv2d_plan(ctypes.addressof(a), which, ctypes.byref(splits), ctypes.byref(floats)))
    return splits.value, floats.value


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _check(x, weight, stride, pad):
    """Every refusal, before any device work."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise GwtfError('conv2d input must be a (N, C, H, W) tensor')
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise GwtfError('conv2d weight must be a (Cout, Cin, k, k) tensor')
    _device_f32(x, 'x')
    _device_f32(weight, 'weight', x)
    if weight.shape[1] != x.shape[1]:
        raise GwtfError(f'conv2d: weight takes {weight.shape[1]} channels, x has {x.shape[1]}')
    if weight.data_ptr() % 16:
        raise GwtfError('conv2d: the weight must start at a 16-byte boundary')
    a = _record(x.shape, weight.shape, stride, pad)
    try:
        plan(a, _lib.CONV2D_FORWARD)                   # the three passes accept and refuse the same geometries
    except GwtfError as e:
        raise GwtfError(f'conv2d: input {tuple(x.shape)}, weight {tuple(weight.shape)}, stride {stride}, padding {pad} is outside what '
                        f'the kernels take ({e})') from None
    return a


class Conv2dFn(torch.autograd.Function):
    """(x, weight, stride, pad) -> y.  backward launches backward_input only when x needs a gradient (the stem never does) and
    backward_weight only when the weight does."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        stride, pad = int(stride), int(pad)
        a = _check(x, weight, stride, pad)
        N, _, H, W = x.shape
        Cout, _, k, _ = weight.shape
        dev = x.device
        y = torch.empty(N, Cout, out_size(H, k, stride, pad), out_size(W, k, stride, pad), device=dev, dtype=torch.float32)
        a.x, a.w, a.y = x.data_ptr(), weight.data_ptr(), y.data_ptr()
        a.stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            check(_lib.lib().gwtf_conv2d_forward(ctypes.addressof(a)))
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, pad)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, pad = ctx.cfg
        dev = x.device
        gy = _device_f32(gy.contiguous(), 'grad_output', x)
        L = _lib.lib()
        dx = dw = None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if ctx.needs_input_grad[0]:
                a = _record(x.shape, weight.shape, stride, pad, dy=gy.data_ptr(), w=weight.data_ptr(), stream=stream)
                _, floats = plan(a, _lib.CONV2D_BACKWARD_INPUT)
                work = torch.empty(floats, device=dev, dtype=torch.float32)
                dx = torch.empty_like(x)
                a.dx, a.work = dx.data_ptr(), work.data_ptr()
                check(L.gwtf_conv2d_backward_input(ctypes.addressof(a)))
            if ctx.needs_input_grad[1]:
                a = _record(x.shape, weight.shape, stride, pad, dy=gy.data_ptr(), x=x.data_ptr(), stream=stream)
                _, floats = plan(a, _lib.CONV2D_BACKWARD_WEIGHT)
                work = torch.empty(floats, device=dev, dtype=torch.float32) if floats else None
                dw = torch.empty_like(weight)
                a.dw, a.work = dw.data_ptr(), None if work is None else work.data_ptr()
                check(L.gwtf_conv2d_backward_weight(ctypes.addressof(a)))
        return dx, dw, None, None


def conv2d(x, conv):
    """conv(x) through the HIP kernels, for the ``nn.Conv2d`` modules the image encoder is made of."""
    if not isinstance(conv, nn.Conv2d):
        raise GwtfError(f'conv2d takes an nn.Conv2d, got {type(conv).__name__}')
    if conv.bias is not None:
        raise GwtfError('conv2d: a Conv2d with bias is not taken')
    if conv.groups != 1:
        raise GwtfError(f'conv2d: groups={conv.groups} is not taken (groups must be 1)')
    if tuple(conv.dilation) != (1, 1):
        raise GwtfError(f'conv2d: dilation={tuple(conv.dilation)} is not taken (dilation must be 1)')
    k, s = tuple(conv.kernel_size), tuple(conv.stride)
    if k[0] != k[1] or s[0] != s[1]:
        raise GwtfError(f'conv2d: kernel_size={k} and stride={s} must be square')
    if conv.padding_mode != 'zeros' or isinstance(conv.padding, str) or tuple(conv.padding) != (k[0] // 2, k[0] // 2):
        raise GwtfError(f'conv2d: padding={conv.padding!r} ({conv.padding_mode}) is not taken (zero padding of k // 2 = {k[0] // 2})')
    return Conv2dFn.apply(x, conv.weight, s[0], k[0] // 2)
