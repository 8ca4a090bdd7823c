"""The train-mode encoder pipeline (csrc/gwtf_encoder_train.hip through encoders._EncoderTrainFn: forward, max-pool, the whole
backward) against the same module in torch float64 on the CPU (tests/encoder_train_ref.py), at the tile edges of its kernels.  Needs
an MI355X.

Cases: encoder_train_ref.CASES says what each one reaches.  A ReLU kink makes the gradients discontinuous and the max-pool makes them
sparse, so every case asserts a property of its own input: no ReLU input of the float64 reference lies within MARGIN = 1e-5 of 0 (the
seeds were searched on the CPU; the fp32 evaluation error of such values is 1-2e-6).  Nothing is excluded from a comparison.

Bar, per tensor: err <= max(8 err32, 4e-6 scale) -- err the largest absolute difference to float64, err32 the same for the CPU
float32 run of the reference, scale the reference tensor's largest magnitude.  The project's rule for an fp32 kernel is
max(2 err32, 1e-6 scale) (tests/test_gpu_norm2d.py); this pipeline's GEMM operands are split-f16 with 22 mantissa bits against
fp32's 24, a factor 2^2 on operand rounding: 8 and 4e-6.  tests/test_encoder_train_ref_cpu.py shows on the reference alone that one
point dropped from a weight gradient is at least 100 of these bars.

N = 12288, the declared limit of the pipeline, has 11.8 M ReLU inputs and no kink-free input: there the gradients are compared as
tests/test_gpu_image_encoder_train.py does, by relative L2 norm against the library path's own distance to float64; the pooled code,
the running statistics and the arg-max keep the strict bar."""
import copy

import pytest
import torch

import encoder_train_ref as ref
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run_hip(m, x, wgt, calls=1):
    """``calls`` train steps of a device copy of m on the HIP pipeline -> the tensors of the last one, as run_reference names them."""
    md = copy.deepcopy(m).to(DEV).train()
    xd, wd = x.to(DEV), wgt.to(DEV)
    for _ in range(calls):
        md.zero_grad(set_to_none=True)
        assert md._train_pipeline_ok(xd)                               # the HIP pipeline is what runs
        pooled, amax = md.forward_max(xd, return_indices=True)
        assert pooled.grad_fn is not None and 'EncoderTrainFn' in type(pooled.grad_fn).__name__
        (pooled * wd).sum().backward()
    out = {'pooled': pooled.detach(), 'argmax': amax.detach().cpu().long(),
           'tracked': {n: int(b) for n, b in md.named_buffers() if not b.dtype.is_floating_point}}
    out.update({'grad.' + n: p.grad for n, p in md.named_parameters()})
    out.update({'buf.' + n: b.detach() for n, b in md.named_buffers() if b.dtype.is_floating_point})
    return {k: (v.cpu().double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in out.items()}


def strict(case, key, got, r64, r32, failures):
    """The bar of the docstring on one tensor; every figure is recorded before anything is asserted."""
    want = r64[key]
    assert got[key].shape == want.shape, (case, key)
    scale = float(want.abs().max())
    err = float((got[key] - want).abs().max())
    err32 = float((r32[key] - want).abs().max())
    bar = max(8.0 * err32, 4e-6 * scale)
    record_parity(f'encoder_train_f64_{case}_{key}', err=err, err32=err32, scale=scale)
    if not err <= bar:                                                 # (a NaN fails too)
        failures.append((case, key, dict(err=err, err32=err32, scale=scale, err_over_bar=err / bar)))


def check_argmax(got, r64, r32, N):
    """The index is the float64 reference's except where the runner-up is within rounding: the float64 feature at OUR index is the
    maximum to 8 x the fp32 evaluation error of the pooled code."""
    amax = got['argmax']
    assert amax.shape == r64['argmax'].shape and int(amax.min()) >= 0 and int(amax.max()) < N
    err32 = float((r32['pooled'] - r64['pooled']).abs().max())
    picked = torch.gather(r64['features'], 2, amax.unsqueeze(2)).squeeze(2)
    assert bool((picked >= r64['pooled'] - 8.0 * err32).all()), float((r64['pooled'] - picked).max())


def check_case(name, calls=1):
    r64, r32 = ref.references(name, calls)
    assert r64['relu_margin'] > ref.MARGIN, (name, r64['relu_margin'])   # the property of the input the gradient comparison rests on
    m, x, wgt = ref.case_inputs(name)
    got = run_hip(m, x, wgt, calls)
    failures = []
    keys = ref.compared_keys(r64)
    assert len(keys) == 1 + 12 + 8
    for key in keys:
        strict(name if calls == 1 else f'{name}_{calls}calls', key, got, r64, r32, failures)
    assert not failures, failures
    assert got['tracked'] == r64['tracked'] and set(got['tracked'].values()) == {calls}
    check_argmax(got, r64, r32, x.shape[2])
    return got, r64


@pytest.mark.parametrize('name', list(ref.CASES))
def test_pipeline_matches_float64_at_the_tile_edges(name):
    check_case(name)


def test_second_call_on_one_module_matches_the_reference_after_two():
    """Accumulators that the single zero-fill arena of a direction would miss show in the second call: its gradients, and the running
    statistics and counters after it."""
    got, r64 = check_case('b1_n260', calls=2)
    once = ref.references('b1_n260')[0]
    assert not torch.equal(r64['buf.features.sd2_bn.running_var'], once['buf.features.sd2_bn.running_var'])   # the second call moved them


@pytest.mark.parametrize('name', list(ref.TIE_CASES))
def test_exact_ties_take_the_first_occurrence(name):
    """Every point occurs twice, 32 points apart (two different tiles): the arg-max is the first one, as torch.max gives it, with
    positive BatchNorm weights (the kmax keys) and with every second one negative (the kmin keys).  Asserted of the kernel alone: its
    arithmetic per point does not depend on where the point sits, so the copies tie exactly.  The reference's own index is not
    asked for here: the copies need not tie to the last bit in a CPU GEMM (a BLAS may take the last columns of a matrix through
    another code path than the first), and on one machine torch.max of the float64 reference reported points 62 and 63 for a few
    channels.  check_case still holds the index to the reference by value."""
    got, r64 = check_case(name)
    assert int(got['argmax'].max()) < 32


# ---- the declared limit: N = 12288 runs on the pipeline, N = 12292 does not ------------------------------------------------------
LIMIT_N, LIMIT_XSEED = 12288, 2200
# The floor of the relative-L2 bar at N = 12288: a tensor whose library error happens to be small must not set a bar below the level
# fp32 reaches on this graph.  Measured on the first device run of this test: see the record beside the constant.
FLOOR = 1.76e-5         # err_library of all gradients together at (1, 12288), first device run (err_hip there: 8.8e-7)


def rel_l2(a, want):
    return float((a - want).norm() / want.norm())


def test_largest_cloud_the_pipeline_admits():
    """(1, 12288): the largest dynamic LDS enc_top_scatter_kernel is ever given (48 KiB + 11 KiB static).  Gradients: relative L2 per
    tensor and over all of them together, err_hip <= max(5 err_library, FLOOR), err_library being the fp32 library path on the same
    device (rocBLAS + MIOpen + autograd: the parent's behaviour) against float64; the factor is test_gpu_image_encoder_train.py's."""
    m, x, wgt = ref.make_case(1, LIMIT_N, '', LIMIT_XSEED)
    r64 = ref.run_reference(m, x, wgt, torch.float64)
    r32 = ref.run_reference(m, x, wgt, torch.float32)
    got = run_hip(m, x, wgt)
    lib = copy.deepcopy(m).to(DEV).train()
    pooled_lib = torch.max(lib.features(x.to(DEV)), dim=2)[0]
    (pooled_lib * wgt.to(DEV)).sum().backward()
    got_lib = {'grad.' + n: p.grad.cpu().double() for n, p in lib.named_parameters()}
    failures = []
    for key in ref.compared_keys(r64):
        if not key.startswith('grad.'):
            strict(f'b1_n{LIMIT_N}', key, got, r64, r32, failures)
    grads = [k for k in r64 if k.startswith('grad.')]
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in grads])
    pairs = [(k, got[k], got_lib[k], r64[k]) for k in grads] + [('all_gradients', cat(got), cat(got_lib), cat(r64))]
    for key, hip, library, want in pairs:
        err_hip, err_library = rel_l2(hip, want), rel_l2(library, want)
        record_parity(f'encoder_train_f64_b1_n{LIMIT_N}_{key}', err_hip=err_hip, err_library=err_library)
        if not err_hip <= max(5.0 * err_library, FLOOR):
            failures.append((key, dict(err_hip=err_hip, err_library=err_library)))
    assert not failures, failures
    assert got['tracked'] == r64['tracked'] and set(got['tracked'].values()) == {1}
    check_argmax(got, r64, r32, LIMIT_N)


def test_one_tile_above_the_limit_takes_the_library_path():
    m, x, _ = ref.make_case(1, LIMIT_N + 4, '', LIMIT_XSEED)
    md, xd = m.to(DEV).train(), x.to(DEV)
    assert not md._train_pipeline_ok(xd)
    pooled = md.forward_max(xd)
    assert pooled.shape == (1, 512) and 'EncoderTrainFn' not in type(pooled.grad_fn).__name__
    assert bool(torch.isfinite(pooled).all())
