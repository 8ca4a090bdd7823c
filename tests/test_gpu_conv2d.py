"""The HIP convolutions (csrc/gwtf_conv2d.hip through conv2d.Conv2dFn) against F.conv2d with autograd in float64 on the CPU.

Bar, the project's rule for an fp32 kernel against float64 (test_gpu_norm2d.py, test_gpu_image_encoder.py):
err <= max(2 * err_torch_fp32, 1e-6 * scale), err the max abs difference to float64, err_torch_fp32 that of the same call in float32
on the CPU, scale the largest reference magnitude of the tensor.  Nothing is excluded: a convolution is linear.

The cases are the smallest shapes at which each mechanism can go wrong: a ragged column tile with all four borders, both parities of
a stride-2 input, the 1 x 1 downsample whose dx has exact zeros, the stem (K = 196, no dx), K = 4608, a one-pixel image, channel
counts that fill no whole 64-row tile, and the smallest weight gradient the planner splits.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity
from go_with_the_flows_amd import _lib, conv2d as c2d

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def split_size():
    """The smallest H = W >= 16 at which backward_weight of (2, 16, H, W) * (16, 16, 3, 3) runs in two or more splits."""
    for n in range(16, 257):
        a = _lib.Conv2dArgs(N=2, Cin=16, H=n, W=n, Cout=16, k=3, stride=1, pad=1)
        if c2d.plan(a, _lib.CONV2D_BACKWARD_WEIGHT)[0] >= 2:
            return n
    raise AssertionError('the planner never splits this weight gradient')


# name: (x shape, w shape, stride, x needs a gradient)
CASES = {
    'k3s1_2x16x9x11': ((2, 16, 9, 11), (16, 16, 3, 3), 1, True),
    'k3s2_odd_2x16x9x11': ((2, 16, 9, 11), (32, 16, 3, 3), 2, True),
    'k3s2_even_2x16x10x12': ((2, 16, 10, 12), (32, 16, 3, 3), 2, True),
    'k1s2_odd_2x16x9x11': ((2, 16, 9, 11), (32, 16, 1, 1), 2, True),
    'k1s2_even_2x16x10x12': ((2, 16, 10, 12), (32, 16, 1, 1), 2, True),
    'stem_2x4x33x37': ((2, 4, 33, 37), (64, 4, 7, 7), 2, False),
    'stem_1x4x32x32': ((1, 4, 32, 32), (64, 4, 7, 7), 2, False),
    'deep_1x512x2x3': ((1, 512, 2, 3), (512, 512, 3, 3), 1, True),
    'one_pixel_1x256x1x1': ((1, 256, 1, 1), (512, 256, 3, 3), 2, True),
    'ch48_1x48x5x5': ((1, 48, 5, 5), (48, 48, 3, 3), 1, True),
    'split_dw': (None, (16, 16, 3, 3), 1, True),
}


def geometry(name):
    xs, ws, stride, x_grad = CASES[name]
    if xs is None:
        xs = (2, 16, split_size(), split_size())
    return xs, ws, stride, x_grad


@functools.lru_cache(maxsize=None)
def inputs(name):
    xs, ws, stride, _ = geometry(name)
    g = torch.Generator().manual_seed(2700 + list(CASES).index(name))
    x = torch.randn(xs, generator=g)
    w = torch.randn(ws, generator=g) / (ws[1] * ws[2] * ws[3]) ** 0.5
    k = ws[2]
    ho, wo = c2d.out_size(xs[2], k, stride, k // 2), c2d.out_size(xs[3], k, stride, k // 2)
    dy = torch.randn(xs[0], ws[0], ho, wo, generator=g)
    return x, w, dy


def torch_pass(name, dtype):
    _, ws, stride, x_grad = geometry(name)
    x, w, dy = (t.to(dtype, copy=True) for t in inputs(name))          # copies: the shared inputs stay plain tensors
    x.requires_grad_(x_grad), w.requires_grad_(True)
    y = F.conv2d(x, w, None, stride, ws[2] // 2)
    grads = torch.autograd.grad(y, (x, w) if x_grad else (w,), dy)
    return {'y': y.detach(), 'dx': grads[0] if x_grad else None, 'dw': grads[-1]}


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64, float32) on the CPU; computed once and left unchanged."""
    return torch_pass(name, torch.float64), torch_pass(name, torch.float32)


def run_hip(name, x_grad=None):
    _, ws, stride, case_grad = geometry(name)
    x_grad = case_grad if x_grad is None else x_grad
    x, w, dy = (t.to(DEV) for t in inputs(name))
    x.requires_grad_(x_grad), w.requires_grad_(True)
    y = c2d.Conv2dFn.apply(x, w, stride, ws[2] // 2)
    y.backward(dy)
    assert (x.grad is not None) == x_grad
    return {'y': y.detach(), 'dx': x.grad, 'dw': w.grad}


def compare(case, key, got, r64, r32):
    ref = r64[key]
    assert got[key].shape == ref.shape and got[key].dtype == torch.float32 and got[key].is_contiguous()
    scale = float(ref.abs().max())
    err = float((got[key].detach().cpu().double() - ref).abs().max())
    err32 = float((r32[key].double() - ref).abs().max())
    record_parity(f'conv2d_{case}_{key}', err=err, err_torch_fp32=err32, scale=scale)
    assert err <= max(2.0 * err32, 1e-6 * scale), (case, key, err, err32, scale)


@pytest.mark.parametrize('name', list(CASES))
def test_three_passes_match_float64(name):
    xs, ws, stride, x_grad = geometry(name)
    if name == 'split_dw':                                   # the property of its own shape this case stands for
        a = _lib.Conv2dArgs(N=xs[0], Cin=xs[1], H=xs[2], W=xs[3], Cout=ws[0], k=3, stride=1, pad=1)
        assert c2d.plan(a, _lib.CONV2D_BACKWARD_WEIGHT)[0] >= 2
        if xs[2] > 16:
            a.H = a.W = xs[2] - 1
            assert c2d.plan(a, _lib.CONV2D_BACKWARD_WEIGHT)[0] == 1
    r64, r32 = references(name)
    got = run_hip(name)
    for key in ('y', 'dx', 'dw'):
        if r64[key] is not None:
            compare(name, key, got, r64, r32)
    if not x_grad:
        assert got['dx'] is None
    dx = got['dx']
    if name == 'k1s2_odd_2x16x9x11':                        # no output reads an odd row or column: exact zeros, written
        assert torch.all(dx[:, :, 1::2, :] == 0) and torch.all(dx[:, :, :, 1::2] == 0)
        assert torch.all(dx[:, :, ::2, ::2] != 0)
    if name == 'k1s2_even_2x16x10x12':
        assert torch.all(dx[:, :, -1, :] == 0) and torch.all(dx[:, :, :, -1] == 0)


def test_the_stem_returns_no_input_gradient_without_launching(monkeypatch):
    """x needs no gradient: the Function returns None for it and backward_input is never called."""
    calls = []
    L = _lib.lib()
    real = L.gwtf_conv2d_backward_input
    monkeypatch.setattr(L, 'gwtf_conv2d_backward_input', lambda *a: calls.append(a) or real(*a))
    got = run_hip('stem_2x4x33x37')
    assert got['dx'] is None and not calls
    run_hip('k3s1_2x16x9x11')
    assert len(calls) == 1                                   # the counter does see the launches that happen


@pytest.mark.parametrize('name', ['k3s2_even_2x16x10x12', 'stem_2x4x33x37', 'deep_1x512x2x3', 'split_dw'])
def test_two_runs_give_identical_bits(name):
    a, b = run_hip(name), run_hip(name)
    for key, t in a.items():
        if t is not None:
            assert torch.equal(t, b[key]), (name, key)


@pytest.mark.parametrize('name', ['k3s1_2x16x9x11', 'split_dw'])
def test_captured_call_replays_the_eager_bits(name):
    _, ws, stride, _ = geometry(name)
    x, w, dy = (t.to(DEV) for t in inputs(name))
    x.requires_grad_(True), w.requires_grad_(True)

    def step():
        # detached results: no autograd graph of an earlier call may be alive when a capture ends (training.GraphedTrainStep)
        y = c2d.Conv2dFn.apply(x, w, stride, ws[2] // 2)
        gx, gw = torch.autograd.grad(y, (x, w), dy)
        return y.detach(), gx, gw

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for c in captured:
        c.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)


def test_outputs_do_not_depend_on_what_the_buffers_held():
    """Every element of y, dx and dw is written, none accumulated into: the entry points called on NaN-filled buffers and
    workspaces give the bits they give on zero-filled ones."""
    name = 'k1s2_odd_2x16x9x11'
    xs, ws, stride, _ = geometry(name)
    x, w, dy = (t.to(DEV) for t in inputs(name))
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def run(fill):
        a = _lib.Conv2dArgs(N=xs[0], Cin=xs[1], H=xs[2], W=xs[3], Cout=ws[0], k=ws[2], stride=stride, pad=ws[2] // 2, stream=stream)
        y, dx, dw = torch.full_like(dy, fill), torch.full_like(x, fill), torch.full_like(w, fill)
        floats = max(c2d.plan(a, which)[1] for which in (_lib.CONV2D_BACKWARD_INPUT, _lib.CONV2D_BACKWARD_WEIGHT))
        work = torch.full((max(floats, 4),), fill, device=DEV)
        a.x, a.w, a.y, a.dy, a.dx, a.dw, a.work = (t.data_ptr() for t in (x, w, y, dy, dx, dw, work))
        for fn in (L.gwtf_conv2d_forward, L.gwtf_conv2d_backward_input, L.gwtf_conv2d_backward_weight):
            assert fn(ctypes.addressof(a)) == 0
        torch.cuda.synchronize()
        return y, dx, dw

    clean, dirty = run(0.0), run(float('nan'))
    for c, d in zip(clean, dirty):
        assert torch.equal(c, d)
    via_function = run_hip(name)
    for c, key in zip(clean, ('y', 'dx', 'dw')):
        assert torch.equal(c, via_function[key])


@pytest.mark.parametrize('name', ['k3s2_even_2x16x10x12', 'split_dw'])
def test_without_an_input_gradient_dw_keeps_its_bits(name):
    full, no_dx = run_hip(name, x_grad=True), run_hip(name, x_grad=False)
    assert no_dx['dx'] is None and full['dx'] is not None
    assert torch.equal(full['dw'], no_dx['dw']) and torch.equal(full['y'], no_dx['y'])
