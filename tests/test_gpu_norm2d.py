"""The fused train-mode BatchNorm2d layer (csrc/gwtf_norm2d.hip through norm2d.NormAct2dFn) against the same operator chain in torch
float64 on the CPU: batch_norm(training=True) -> (+ r) -> relu -> (max_pool2d).  Needs an MI355X.

Shapes: the smallest at which each mechanism can go wrong (49-float planes that start unaligned, ragged chunk edges, several partials
per channel, the channel count of the real layers, padded pool windows, the stem's output for 97 x 131 images, a channel mean 1000
standard deviations from zero).  A ReLU kink makes gradients discontinuous, so every case asserts a property of its own input: in
the float64 reference no pre-activation lies within MARGIN of 0 (the seeds were searched on the CPU; fp32 evaluation error of these
values is about 1e-7).  Nothing is excluded from a comparison.

Bar: the project's rule for an fp32 kernel against float64 (tests/test_gpu_image_encoder.py): err <= max(2 err_torch_fp32,
1e-6 scale), err_torch_fp32 being the CPU float32 run of the same chain, scale the largest reference magnitude of the tensor."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity
from go_with_the_flows_amd import norm2d
from go_with_the_flows_amd._lib import GwtfError

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS, MOMENTUM = 1e-5, 0.1

# name: (shape, variant, seed, kink margin, input mean, input std)
CASES = {
    'plain_3x5x7x7': ((3, 5, 7, 7), 'relu', 0, 1e-3, 0.0, 1.0),
    'residual_3x5x7x7': ((3, 5, 7, 7), 'residual', 0, 1e-3, 0.0, 1.0),
    'residual_2x3x33x33': ((2, 3, 33, 33), 'residual', 50, 1e-3, 0.0, 1.0),
    'plain_2x3x56x56': ((2, 3, 56, 56), 'relu', 12, 1e-4, 0.0, 1.0),
    'residual_2x64x14x14': ((2, 64, 14, 14), 'residual', 13, 1e-4, 0.0, 1.0),
    'pool_2x3x9x11': ((2, 3, 9, 11), 'pool', 1, 1e-3, 0.0, 1.0),
    'pool_2x4x49x66': ((2, 4, 49, 66), 'pool', 5, 1e-4, 0.0, 1.0),
    'none_3x5x7x7': ((3, 5, 7, 7), 'none', 0, None, 0.0, 1.0),
    'shifted_3x5x7x7': ((3, 5, 7, 7), 'relu', 0, 1e-3, 100.0, 0.1),
}


def inputs(name):
    """fp32 CPU tensors of a case: x, gamma, beta, residual or None, running_mean, running_var, dy."""
    shape, variant, seed, _, loc, std = CASES[name]
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = torch.randn(shape, generator=g) * std + loc
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    r = torch.randn(shape, generator=g) if variant == 'residual' else None
    rm = 0.1 * torch.randn(C, generator=g) + loc
    rv = 0.5 + torch.rand(C, generator=g)
    out_shape = (N, C, norm2d.pooled_size(H), norm2d.pooled_size(W)) if variant == 'pool' else shape
    dy = torch.randn(out_shape, generator=g)
    return x, gamma, beta, r, rm, rv, dy


def chain(name, dtype, calls=1):
    """The operator chain in torch on the CPU in `dtype`: a dict of every tensor the tests compare."""
    variant = CASES[name][1]
    x, gamma, beta, r, rm, rv, dy = (None if t is None else t.to(dtype) for t in inputs(name))
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    if r is not None:
        r.requires_grad_(True)
    for _ in range(calls):
        pre, mean, rstd = torch.native_batch_norm(x, gamma, beta, rm, rv, True, MOMENTUM, EPS)
    if r is not None:
        pre = pre + r
    y = pre if variant == 'none' else torch.relu(pre)
    idx = None
    if variant == 'pool':
        y, idx = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    y.backward(dy)
    out = {'y': y.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad, 'mean': mean, 'rstd': rstd,
           'running_mean': rm, 'running_var': rv, 'pre': pre.detach(), 'idx': idx}
    if r is not None:
        out['d_residual'] = r.grad
    return out


@functools.lru_cache(maxsize=None)
def references(name, calls=1):
    return chain(name, torch.float64, calls), chain(name, torch.float32, calls)


def run_hip(name, calls=1):
    variant = CASES[name][1]
    x, gamma, beta, r, rm, rv, dy = (None if t is None else t.to(DEV) for t in inputs(name))
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    if r is not None:
        r.requires_grad_(True)
    for _ in range(calls):
        y, stats, offsets = norm2d.NormAct2dFn.apply(x, gamma, beta, r, rm, rv, EPS, MOMENTUM, variant != 'none', variant == 'pool')
    y.backward(dy)
    out = {'y': y.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad, 'mean': stats[0], 'rstd': stats[1],
           'running_mean': rm, 'running_var': rv, 'offsets': offsets}
    if r is not None:
        out['d_residual'] = r.grad
    return out


def compare(case, key, got, r64, r32):
    ref = r64[key]
    scale = float(ref.abs().max())
    err = float((got[key].detach().cpu().double() - ref).abs().max())
    err32 = float((r32[key].double() - ref).abs().max())
    record_parity(f'norm2d_{case}_{key}', err=err, err_torch_fp32=err32, scale=scale)
    assert err <= max(2.0 * err32, 1e-6 * scale), (case, key, err, err32, scale)


KEYS = ('y', 'dx', 'd_residual', 'dgamma', 'dbeta', 'mean', 'rstd', 'running_mean', 'running_var')


@pytest.mark.parametrize('name', list(CASES))
def test_layer_matches_float64(name):
    shape, variant, _, margin, _, _ = CASES[name]
    r64, r32 = references(name)
    if margin is not None:                                   # the property of the input the gradient comparison rests on
        assert float(r64['pre'].abs().min()) > margin, (name, float(r64['pre'].abs().min()))
    got = run_hip(name)
    for key in KEYS:
        if key in r64:
            compare(name, key, got, r64, r32)
    if variant == 'pool':
        off = got['offsets'].cpu().long()
        assert off.dtype == torch.int64 and got['offsets'].dtype == torch.uint8 and int(off.max()) <= 8
        Ho, Wo = off.shape[2:]
        i = torch.arange(Ho).view(1, 1, Ho, 1)
        j = torch.arange(Wo).view(1, 1, 1, Wo)
        flat = (2 * i - 1 + off // 3) * shape[3] + (2 * j - 1 + off % 3)
        assert torch.equal(flat, r64['idx'])                 # the first maximum in row-major order, as max_pool2d reports it


@pytest.mark.parametrize('name', ['residual_2x3x33x33', 'plain_2x3x56x56', 'pool_2x4x49x66', 'none_3x5x7x7'])
def test_two_runs_give_identical_bits(name):
    a, b = run_hip(name), run_hip(name)
    for key, t in a.items():
        if t is not None:
            assert torch.equal(t, b[key]), (name, key)


@pytest.mark.parametrize('name', ['plain_3x5x7x7', 'pool_2x3x9x11', 'shifted_3x5x7x7'])
def test_running_statistics_after_two_calls(name):
    r64, r32 = references(name, 2)
    got = run_hip(name, 2)
    for key in ('running_mean', 'running_var'):
        compare(name + '_two_calls', key, got, r64, r32)
    assert not torch.equal(got['running_mean'].cpu(), run_hip(name)['running_mean'].cpu())      # the second call moved them


def test_module_wrapper_advances_the_buffers_like_torch():
    x = inputs('plain_3x5x7x7')[0]
    bn = torch.nn.BatchNorm2d(5)
    ref = torch.relu(bn.double()(x.double()))
    bn_d = torch.nn.BatchNorm2d(5).to(DEV)
    y = norm2d.norm_act_2d(x.to(DEV), bn_d)
    assert int(bn_d.num_batches_tracked) == 1 == int(bn.num_batches_tracked)
    assert float((y.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    assert float((bn_d.running_var.cpu().double() - bn.running_var).abs().max()) <= 1e-6
    norm2d.norm_act_2d(x.to(DEV), bn_d)
    assert int(bn_d.num_batches_tracked) == 2


@pytest.mark.parametrize('name', ['residual_2x64x14x14', 'pool_2x3x9x11'])
def test_captured_call_replays_the_eager_bits(name):
    variant = CASES[name][1]
    x, gamma, beta, r, rm0, rv0, dy = (None if t is None else t.to(DEV) for t in inputs(name))
    x.requires_grad_(True), gamma.requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()

    def step():
        # detached results: no autograd graph of an earlier call may be alive when a capture ends (training.GraphedTrainStep)
        y, _, _ = norm2d.NormAct2dFn.apply(x, gamma, beta, r, rm, rv, EPS, MOMENTUM, True, variant == 'pool')
        gx, gg = torch.autograd.grad(y, (x, gamma), dy)
        return y.detach(), gx, gg

    eager = [t.clone() for t in step()]
    eager_rm = rm.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    rm.copy_(rm0), rv.copy_(rv0)
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)
    assert torch.equal(rm, eager_rm)


def test_one_value_per_channel_raises():
    x = torch.randn(1, 3, 1, 1, device=DEV)
    ones = torch.ones(3, device=DEV)
    with pytest.raises(GwtfError, match='more than 1 value per channel'):
        norm2d.NormAct2dFn.apply(x, ones, ones.clone(), None, ones.clone(), ones.clone(), EPS, MOMENTUM, True, False)
    with pytest.raises(GwtfError):
        norm2d.norm_act_2d(x, torch.nn.BatchNorm2d(3).to(DEV))
    with pytest.raises(ValueError):                          # torch refuses the same input
        torch.nn.BatchNorm2d(3).to(DEV)(x)
