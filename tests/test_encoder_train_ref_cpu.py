"""tests/encoder_train_ref.py validated without a GPU: the helper against the genuine reference's recorded outputs (golden
g17_encoder_train), the kink margin of every case that test_gpu_encoder_train_f64.py runs, and the sharpness of that test's bar --
measured on the float64 reference alone, one dropped point moves a weight gradient by at least 100 bars."""
import numpy as np
import pytest
import torch

import encoder_train_ref as ref
from conftest import golden

F32_ROUND = 2.0 ** -24          # a float64 value stored as float32: half an ulp, relative


@pytest.mark.parametrize('tag,seed', [('a', 1700), ('b', 1710)])
def test_reference_reproduces_the_golden_fixture(tag, seed):
    """pooled_f64 is stored in float64: agreement at float64 rounding (1e-12 of the largest value; seen: equal bits).  grad_f64.* are the
    reference's float64 gradients STORED as float32: agreement at that storage rounding, 2^-24 of the largest value.  buf.* come from
    its fp32 run: the fixture's own 2e-5 bar (tests/test_gpu_encoder.py)."""
    G = golden('g17_encoder_train')
    m = ref.make_module(seed=seed)
    r = ref.run_reference(m, torch.from_numpy(G[f'{tag}_x']), torch.from_numpy(G[f'{tag}_wgt']), torch.float64)
    want = G[f'{tag}_pooled_f64']
    assert want.dtype == np.float64
    err = float(np.abs(r['pooled'].numpy() - want).max())
    print(f'{tag} pooled_f64: err {err:.3e} scale {np.abs(want).max():.3e}')
    assert err <= 1e-12 * float(np.abs(want).max())
    grads = [k for k in r if k.startswith('grad.')]
    assert len(grads) == 12
    for k in grads:
        want = G[f'{tag}_grad_f64.' + k[len('grad.'):]]
        assert want.dtype == np.float32
        err = float(np.abs(r[k].numpy() - want.astype(np.float64)).max())
        assert err <= 1.01 * F32_ROUND * float(np.abs(want).max()), (k, err)
    bufs = [k for k in r if k.startswith('buf.')]
    assert len(bufs) == 8
    for k in bufs:
        want = G[f'{tag}_buf.' + k[len('buf.'):]].astype(np.float64)
        assert float(np.abs(r[k].numpy() - want).max()) < 2e-5 * max(1.0, float(np.abs(want).max())), k
    for name, n in r['tracked'].items():
        assert n == int(G[f'{tag}_buf.{name}']) == 1


def test_argmax_and_features_are_consistent():
    r64, r32 = ref.references('b1_n36')
    assert 'features' in r64 and 'features' not in r32
    assert torch.equal(torch.gather(r64['features'], 2, r64['argmax'].unsqueeze(2)).squeeze(2), r64['pooled'])
    assert r64['features'].shape == (1, 512, 36) and r64['argmax'].dtype == torch.int64


@pytest.mark.parametrize('name', list(ref.CASES) + list(ref.TIE_CASES))
def test_no_relu_input_near_zero(name):
    """The property the gradient comparison rests on: the fp32 CPU run of this chain is 1-2e-6 from float64 on ReLU inputs with
    |value| < 1e-3, so no fp32 evaluation puts one of them on the other side of the kink."""
    r64, _ = ref.references(name)
    print(f'{name}: smallest |ReLU input| {r64["relu_margin"]:.3e}')
    assert r64['relu_margin'] > ref.MARGIN


def test_neg_variant_negates_every_second_batchnorm_weight():
    plain, neg = ref.make_module(), ref.make_module('neg')
    for (name, p), q in zip(plain.named_parameters(), neg.parameters()):
        if name.endswith('_bn.weight'):
            assert torch.equal(q[::2], -p[::2]) and torch.equal(q[1::2], p[1::2]) and bool((q[::2] < 0).all())
        else:
            assert torch.equal(p, q)


def test_tie_input_repeats_every_point_in_a_second_tile():
    for name in ref.TIE_CASES:
        _, x, _ = ref.case_inputs(name)
        assert x.shape == (1, 3, 64) and torch.equal(x[:, :, 32:], x[:, :, :32])
        r64, _ = ref.references(name)
        # the copies' features agree to float64 rounding; not asked to the last bit, which is up to the CPU BLAS (a GEMM may take the
        # last columns of a matrix through another code path than the first), and so neither is torch.max's choice between them
        f = r64['features']
        assert float((f[:, :, 32:] - f[:, :, :32]).abs().max()) <= 1e-13 * float(f.abs().max())
        first = torch.where(r64['argmax'] >= 32, r64['argmax'] - 32, r64['argmax'])
        assert float((torch.gather(f, 2, first.unsqueeze(2)).squeeze(2) - r64['pooled']).abs().max()) <= 1e-13 * float(f.abs().max())


def test_two_calls_move_the_running_statistics_and_keep_the_gradients():
    one, two = ref.references('b1_n260')[0], ref.references('b1_n260', 2)[0]
    assert set(two['tracked'].values()) == {2} and set(one['tracked'].values()) == {1}
    for k in one:
        if k.startswith('buf.'):
            assert not torch.equal(one[k], two[k])
        elif k.startswith('grad.'):                                  # batch statistics: the running ones do not enter
            assert float((one[k] - two[k]).abs().max()) <= 1e-13 * float(one[k].abs().max())


SHARP_CASES = [n for n, c in ref.CASES.items() if c[1] >= 132]


@pytest.mark.parametrize('name', SHARP_CASES)
def test_one_dropped_point_is_100_bars(name):
    """dW_l = einsum('bcn,bkn->ck', dy_l, a_{l-1}) of the float64 reference's own operands is autograd's dW_l to 1e-13.  Leaving the
    last point of the last shape out of that sum moves dW_l by at least 100 x the bar test_gpu_encoder_train_f64.py holds the kernel
    to, max(8 err32, 4e-6 scale), in every layer: that test would see one dropped point."""
    m, x, wgt = ref.case_inputs(name)
    r64 = ref.run_reference(m, x, wgt, torch.float64, capture=True)
    r32 = ref.references(name)[1]
    assert list(r64['dy']) == ['init_sd', 'sd0', 'sd1', 'sd2']
    ratios = {}
    for layer in r64['dy']:
        key = f'grad.features.{layer}.weight'
        auto = r64[key][0]
        dy, a = r64['dy'][layer], r64['a_in'][layer]
        dW = torch.einsum('bcn,bkn->ck', dy, a)
        scale = float(auto.abs().max())
        assert float((dW - auto).abs().max()) <= 1e-13 * scale, layer
        dropped = dW - torch.outer(dy[-1, :, -1], a[-1, :, -1])
        bar = max(8.0 * float((r32[key][0] - auto).abs().max()), 4e-6 * scale)
        ratios[layer] = float((dropped - dW).abs().max()) / bar
    print(f'{name}: one dropped point / bar per layer', {k: round(v, 1) for k, v in ratios.items()}, 'worst %.1f' % min(ratios.values()))
    assert min(ratios.values()) >= 100.0, ratios
