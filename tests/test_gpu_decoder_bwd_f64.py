"""The decoder's differentiable pass (csrc/gwtf_bwd.hip with the train-pipeline folds of csrc/gwtf_train.hip, through
LocalCondRNVPDecoder.forward_fused and MixtureStack.forward_all) against oracle/torch_port in float64 on the CPU
(tests/decoder_train_ref.py), at every tile variant bwd_plan picks.  Needs an MI355X.

Cases: decoder_train_ref.CASES says what each one reaches, and each asserts the launch plan it is named for before it runs, so a
changed threshold cannot silently move a case to another kernel.  A ReLU kink makes the gradients discontinuous, so every case
asserts a property of its own input: no ReLU input of the float64 reference lies within MARGIN = 1e-5, or within 8 x the float32
evaluation error of the case's ReLU inputs, of 0.  The 64-point cases up to f = 19 meet it with plain clouds, the wider ones and the
128- and 256-point ones with tiled clouds (a few distinct points per shape repeated in a shuffled order, every position with its own
random-sign cotangent).  Nothing is excluded from a comparison and no cotangent is made positive.  Where M is 1 or 2 the input
side is weakly tested: a kernel that reads x or the forward record of another position with the same point passes (decoder_train_ref
says which cases).

Bar, per tensor: err <= max(8 err32, 4e-6 scale) -- err the largest absolute difference to float64, err32 the same for the CPU
float32 run of the reference, scale the reference tensor's largest magnitude: the project's bar for its split-f16 pipelines
(tests/test_gpu_encoder_train_f64.py).  It holds for z, logdet, dp, dg, every parameter gradient and, in train mode, every running
statistic.  Six families of long cancelling sums carry a factor on it (decoder_train_ref.FAMILY_FACTOR says which, why, and what
was measured); sd1.weight, sd2.weight, the BatchNorm parameters, the FiLM output weights, dp, dg, z and logdet do not.
tests/test_decoder_train_ref_cpu.py shows on the reference alone that one position taken out of the loss moves every sd1.weight,
sd2.bias and FiLM output weight by at least 2 of these bars and dp at the point by at least 100.

First device run at factor 1 everywhere: 5 of 36 tests missed, worst err / bar 2.06 (film0_bn.weight at L4), 1.33 (sd2.bias at
s_f96_n65), 1.015 (sd0.weight at s_f33_n65); with the factors the worst over 40 repeats of L4 and 20 of L1, L2 and s_f33_n65 is 0.84
(film1.weight at L4).  The issue's case L3 (K2 = 0 with FULL) is not here: docs/LOG.md says why."""
import pytest
import torch

import decoder_train_ref as ref
import go_with_the_flows_amd as gw
from conftest import record_parity
from go_with_the_flows_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _default_tiling():
    _lib.set_tuning(0)
    yield
    _lib.set_tuning(0)


def run_hip(name, calls=1, tune=0):
    """``calls`` differentiable passes of device copies of the case's decoders -> the tensors of the last one, as run_reference names
    them, and the num_batches_tracked counters."""
    c = ref.CASES[name]
    p, g, wz, wl = ref.case_inputs(name)
    decs = [m.to(DEV).train(c.training) for m, _ in ref.decoders(name)]
    pt, gt = torch.from_numpy(p).to(DEV).requires_grad_(True), torch.from_numpy(g).to(DEV).requires_grad_(True)
    wzd, wld = torch.from_numpy(wz).to(DEV), torch.from_numpy(wl).to(DEV)
    stack = gw.MixtureStack(decs) if c.K > 1 else None
    _lib.set_tuning(tune)
    for _ in range(calls):
        pt.grad = gt.grad = None
        for m in decs:
            m.zero_grad(set_to_none=True)
        if stack is not None:
            z, ld = stack.forward_all(pt, gt, c.mode)                  # (K,B,3,N): all components through one K-batched pipeline
        else:
            z, ld = (t[None] for t in decs[0].forward_fused(pt, gt, c.mode))
        assert z.grad_fn is not None
        ((z * wzd).sum() + (ld * wld).sum()).backward()
    torch.cuda.synchronize()
    out = {'z': z.detach(), 'logdet': ld.detach(), 'dp': pt.grad, 'dg': gt.grad}
    tracked = set()
    for k, m in enumerate(decs):
        out.update({f'grad.{k}.{n}': prm.grad for n, prm in m.named_parameters()})
        for n, b in m.named_buffers():
            if n.endswith(('running_mean', 'running_var')) and c.training:
                out[f'buf.{k}.{n}'] = b.detach()
            elif n.endswith('num_batches_tracked'):
                tracked.add(int(b))
    return {k: v.cpu().double() for k, v in out.items()}, tracked


def check_case(name, calls=1, tune=0, tag=''):
    c = ref.CASES[name]
    if not tune:
        ref.assert_plan(name)                                          # the kernel variant the case is named for
    r64, r32 = ref.references(name, calls)
    assert r64['relu_margin'] >= ref.MARGIN and r64['relu_margin'] >= ref.MARGIN_E32 * r32['relu_e'] and r32['relu_flips'] == 0
    got, tracked = run_hip(name, calls, tune)
    keys = ref.compared_keys(r64)
    assert len(keys) == 4 + c.K * c.L * (96 + (48 if c.training else 0))
    assert set(got) == set(keys)
    failures = []
    for key in keys:                                                   # every figure is recorded before anything is asserted
        assert got[key].shape == r64[key].shape, (name, key)
        bar, err32, scale = ref.bar(key, r64, r32)
        err = float((got[key] - r64[key]).abs().max())
        record_parity(f'decoder_bwd_f64_{name}{tag}_{key}', err=err, err32=err32, scale=scale, bar=bar)
        if not err <= bar:                                             # (a NaN fails too)
            failures.append((key, dict(err=err, err32=err32, scale=scale, err_over_bar=err / bar)))
    assert not failures, (name, len(failures), failures)
    assert tracked == {calls if c.training else 0}
    return got, r64


@pytest.mark.parametrize('name', list(ref.SMALL_CASES))
def test_64_point_tiles_match_float64(name):
    check_case(name)


@pytest.mark.parametrize('name', list(ref.LARGE_CASES))
def test_128_and_256_point_tiles_match_float64(name):
    check_case(name)


def test_second_call_on_one_module_matches_the_reference_after_two():
    """The running statistics have moved and every workspace is reused: accumulators that a single zero-fill would miss show here."""
    got, r64 = check_case('L2', calls=2, tag='_2calls')
    once = ref.references('L2')[0]
    key = next(k for k in r64 if k.endswith('sd0_bn.running_var'))
    assert not torch.equal(r64[key], once[key])                        # the second call moved them


@pytest.mark.parametrize('tune,plan,tag', [(ref.TUNE_SMALL, ref.L5_SMALL_PLAN, '_small_light_tile'),
                                           (ref.TUNE_SINGLE, ref.L5_SINGLE_PLAN, '_single_tile')], ids=['small_light_tile', 'single_tile'])
def test_l5_through_the_other_light_tiles(tune, plan, tag):
    """The A/B of the tile variants on one input: L5 through the 128-point light kernel, and through the 256-point one with one tile
    per workgroup, stays within the bar."""
    ref.assert_plan('L5', tune, plan)
    check_case('L5', tune=tune, tag=tag)
