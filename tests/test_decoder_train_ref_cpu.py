"""tests/decoder_train_ref.py validated without a GPU: the helper against the genuine reference's recorded outputs (golden g18 in
float64, g9 in float32), and for every case that test_gpu_decoder_bwd_f64.py runs the three properties that test rests on -- the kink
margin of the input, the kernel variant the launch plan picks for it, and the sharpness of the bar: measured on the float64 reference
alone, taking one position out of the loss moves the gradients by several bars."""
import numpy as np
import pytest
import torch

import decoder_train_ref as ref
from conftest import golden
from helpers import decoder_and_state

F32_ULP = 2.0 ** -23            # a float64 value stored as float32, relative to the tensor's largest entry (the fixture's storage)


def _nll_like(states, D, L, B, dtype):
    """The fixtures' loss 0.5 * (logdet + z^2).sum() / B through the helper's linear one: its gradient is that of
    (z * wz).sum() + (logdet * wl).sum() at wz = z / B, wl = 0.5 / B, with z from a first run of the same dtype."""
    p, g = D['p'], D['g']
    shape = (1,) + p.shape
    first = ref.run_reference(states, p, g, np.zeros(shape), np.zeros(shape), L, 'inverse', True, dtype)
    return ref.run_reference(states, p, g, first['z'].numpy() / B, np.full(shape, 0.5 / B), L, 'inverse', True, dtype)


def test_float64_run_reproduces_golden_g18():
    """33 couplings, f = 37, train mode: z, logdet, dp, dg and every kept parameter gradient of the genuine reference's float64 run,
    to the precision the fixture stores them in (float32: 2^-23 of the tensor's largest entry)."""
    D = golden('g18_train_depth_11x37x128')
    L, f, G, B, N = (int(v) for v in D['dims'])
    r = _nll_like([decoder_and_state(L, f, G, 1800)[1]], D, L, B, torch.float64)
    pairs = [('z', r['z'][0], D['z_f64']), ('logdet', r['logdet'][0], D['logdet_f64']), ('dp', r['dp'], D['dp_f64']), ('dg', r['dg'], D['dg_f64'])]
    kept = [k for k in D.files if k.startswith('grad_f64::')]
    assert kept
    pairs += [(k, r['grad.0.' + k[len('grad_f64::'):]], D[k]) for k in kept]
    for name, got, want in pairs:
        want = np.asarray(want, np.float64)
        err, scale = float(np.abs(got.numpy() - want).max()), float(np.abs(want).max())
        assert err <= F32_ULP * scale, (name, err, scale)


def test_float32_run_reproduces_golden_g9():
    """The genuine reference's fp32 loss.backward() in train mode, within the bars test_g9_train_mode_gradients_match_reference_autograd
    holds the kernels to: 5e-5 on z and logdet, 1e-3 of the largest entry on dp and dg, 2e-3 on every parameter gradient."""
    D = golden('g9_train_gradients')
    L, f, G, B, N = (int(v) for v in D['dims'])
    r = _nll_like([decoder_and_state(L, f, G, 900)[1]], D, L, B, torch.float32)
    rel = lambda a, b: float(np.abs(a.numpy() - b).max() / (np.abs(b).max() + 1e-12))
    assert float(np.abs(r['z'][0].numpy() - D['z']).max()) < 5e-5 and float(np.abs(r['logdet'][0].numpy() - D['logdet']).max()) < 5e-5
    assert rel(r['dp'], D['dp']) < 1e-3 and rel(r['dg'], D['dg']) < 1e-3
    grads = [k for k in D.files if k.startswith('grad::')]
    assert len(grads) == len([k for k in r if k.startswith('grad.')])
    for k in grads:
        assert rel(r['grad.0.' + k[len('grad::'):]], D[k]) < 2e-3, k
    assert len([k for k in r if k.startswith('buf.')]) == 2 * 4 * 2 * 3 * L     # four BatchNorms per branch, two branches per coupling


def test_relu_wrapper_is_restored_and_sees_every_relu():
    import torch.nn.functional as F
    from oracle import torch_port as tp
    assert tp.F is F
    with pytest.raises(KeyError):                                             # an exception inside the run restores it too
        ref.run_reference([{}], np.zeros((1, 3, 4), np.float32), np.zeros((1, ref.G), np.float32), np.zeros((1, 1, 3, 4)),
                          np.zeros((1, 1, 3, 4)), 1, 'inverse', True, torch.float64)
    assert tp.F is F
    r64 = ref.run_case('s_f8_n5', torch.float64, capture=True)
    c = ref.CASES['s_f8_n5']
    assert len(r64['relu_inputs']) == 12 * c.L and all(x.shape == (c.B, c.f, c.N) and x.dtype == torch.float64 for x in r64['relu_inputs'])
    assert min(float(x.abs().min()) for x in r64['relu_inputs']) == r64['relu_margin']
    assert bool((torch.cat(r64['relu_inputs']) < 0).any())                     # the values BEFORE the in-place ReLU


def test_tiled_cloud_repeats_the_distinct_points_in_every_shape():
    from go_with_the_flows_amd.synth import synth_inputs
    B, N, M = 3, 130, 4
    p, g, idx, _ = ref.tiled_cloud(B, N, M, ref.G, 5)
    p0, g0 = synth_inputs(B, M, ref.G, 5)
    assert p.shape == (B, 3, N) and np.array_equal(g, g0) and len({tuple(row) for row in g}) == B
    for b in range(B):
        assert np.array_equal(p[b], p0[b][:, idx[b]])
        assert sorted(np.bincount(idx[b], minlength=M)) == [32, 32, 33, 33]
    assert not np.array_equal(idx[0], idx[1])                                 # every shape has its own order
    name = next(n for n, c in ref.CASES.items() if c.M)
    _, _, wz, wl = ref.case_inputs(name)
    assert (wz < 0).any() and (wz > 0).any() and (wl < 0).any() and not np.array_equal(wz, wl)    # random signs: sums may cancel


@pytest.mark.parametrize('name', list(ref.CASES))
def test_no_relu_input_near_its_kink(name):
    """The property the gradient comparison rests on, from the reference alone: the smallest |ReLU input| of the float64 run is at
    least MARGIN and at least 8 x the largest float32 evaluation error of a ReLU input of this case (the kernels' split-f16
    operands carry 22 mantissa bits against float32's 24), and no ReLU input has another sign in float32."""
    r64, r32 = ref.references(name)
    print(f'{name}: smallest |ReLU input| {r64["relu_margin"]:.3e}, e32 {r32["relu_e"]:.3e}, sign flips {r32["relu_flips"]}')
    assert r64['relu_margin'] >= ref.MARGIN
    assert r64['relu_margin'] >= ref.MARGIN_E32 * r32['relu_e']
    assert r32['relu_flips'] == 0


@pytest.mark.parametrize('name', list(ref.CASES))
def test_case_reaches_the_kernel_it_is_named_for(name):
    c = ref.CASES[name]
    ref.assert_plan(name)
    passes = {pas for pas, _ in c.plan}
    assert passes == ({ref.LIGHT, ref.MERGED} if c.training else {ref.DIRECT})
    assert {pat for _, pat in c.plan} == ({0, 3} if c.L > 1 else {0})
    if name in ref.SMALL_CASES:
        assert all(v['NB'] == 1 for v in c.plan.values()) and c.M >= 0
    else:
        assert all(v['NB'] >= 2 for v in c.plan.values()) and c.M > 0


def test_tile_ab_variants_of_l5_take_other_kernels():
    ref.assert_plan('L5', ref.TUNE_SMALL, ref.L5_SMALL_PLAN)
    ref.assert_plan('L5', ref.TUNE_SINGLE, ref.L5_SINGLE_PLAN)
    assert ref.L5_SMALL_PLAN[(ref.LIGHT, 0)]['NB'] == 2 and ref.L5_SINGLE_PLAN[(ref.LIGHT, 0)]['tpw'] == 1


def test_family_names():
    keys = [k for k in ref.references('s_f8_n5')[0] if k.startswith('grad.')]
    assert len(keys) == 96 and {ref.family(k) for k in keys} == {
        'sd0.weight', 'sd0_bn.weight', 'sd0_bn.bias', 'sd1.weight', 'sd2.weight', 'sd2.bias', 'film0.weight', 'film0_bn.weight',
        'film0_bn.bias', 'film1.weight', 'film1.bias'}
    assert set(ref.FAMILY_FACTOR) < {ref.family(k) for k in keys} and ref.family('dp') == 'dp'
    assert not {'sd1.weight', 'film1.weight'} & set(ref.FAMILY_FACTOR)        # the tensors the sharpness conditions name first


@pytest.mark.parametrize('name', list(ref.CASES))
def test_one_position_out_of_the_loss_is_several_bars(name):
    """Zero the cotangents of the last point of the last shape in float64: each tensor's change in units of the bar
    test_gpu_decoder_bwd_f64.py holds it to.  A condition on the inputs: a case that misses it gets another seed or fewer points."""
    c = ref.CASES[name]
    r64, r32 = ref.references(name)
    z = ref.run_case(name, torch.float64, zero_last=True)
    moved = {k: float((z[k] - r64[k]).abs().max()) / ref.bar(k, r64, r32)[0] for k in r64 if k.startswith('grad.')}
    by_family = {}
    for k, v in moved.items():
        by_family.setdefault(ref.family(k), []).append(v)
    dp_point = float((z['dp'][-1, :, -1] - r64['dp'][-1, :, -1]).abs().max()) / ref.bar('dp', r64, r32)[0]
    ten = sum(v >= 10.0 for v in moved.values())
    print(f'{name}: change / bar, smallest per family', {k: float('%.3g' % min(v)) for k, v in sorted(by_family.items())},
          f'dp at the point {dp_point:.3g}; {ten} of {len(moved)} tensors by >= 10 bars')
    assert min(by_family['sd1.weight']) >= 2.0
    assert min(by_family['sd2.bias']) >= 2.0
    assert min(by_family['film1.weight']) >= 2.0
    assert dp_point >= 100.0
    if c.B * c.N <= 70000:
        assert 2 * ten >= len(moved)


def test_second_call_moves_the_running_statistics_and_keeps_the_gradients():
    one, two = ref.references('L2')[0], ref.references('L2', 2)[0]
    for k in one:
        if k.startswith('buf.'):
            assert not torch.equal(one[k], two[k])
        elif k.startswith('grad.'):                                  # batch statistics: the running ones do not enter
            assert float((one[k] - two[k]).abs().max()) <= 1e-12 * float(one[k].abs().max())
