"""The encoder train pipeline's argument record (GwtfEncTrainCtx) carries per-layer arrays: the place where a record can shift by
one.  One small case that gives every layer its own momentum and takes one layer's running statistics away."""
import copy

import pytest
import torch
import torch.nn as nn

from go_with_the_flows_amd import encoders
from go_with_the_flows_amd.synth import load_synth_, synth_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_train_pipeline_per_layer_momenta_and_a_batchnorm_without_running_statistics():
    """B = 2, N = 36 through forward_max + backward against a deep copy on the library path, at the bars of
    test_train_pipeline_odd_shapes_against_library_path: four different momenta, sd1_bn with track_running_stats=False (its
    running_mean / running_var fields are NULL: skip)."""
    B, N, seed = 2, 36, 2236
    m = encoders.PointNetCloudEncoder(3, 64, [128, 256, 512])
    m.features.sd1_bn = nn.BatchNorm1d(256, track_running_stats=False)
    load_synth_(m, seed)
    bns = [mod for mod in m.features.children() if isinstance(mod, nn.modules.batchnorm._BatchNorm)]
    for bn, momentum in zip(bns, (0.1, 0.3, 0.05, 0.2)):
        bn.momentum = momentum
    m = m.to(DEV).train()
    lib = copy.deepcopy(m)
    x = torch.from_numpy(synth_inputs(B, N, 4, seed + 1)[0]).to(DEV)
    wgt = torch.randn(B, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    assert m._train_pipeline_ok(x)
    pooled = m.forward_max(x)
    assert 'EncoderTrainFn' in type(pooled.grad_fn).__name__
    (pooled * wgt).sum().backward()
    ref = torch.max(lib.features(x), dim=2)[0]
    (ref * wgt).sum().backward()
    scale = max(1.0, float(ref.detach().abs().max()))
    err = float((pooled - ref).detach().abs().max())
    print(f'pooled err {err:.3e} (bar {5e-5 * scale:.3e})')
    assert err < 5e-5 * scale
    for (name, p), q in zip(m.named_parameters(), lib.parameters()):
        gs = float(q.grad.abs().max())
        e = float((p.grad - q.grad).abs().max())
        print(f'{name}: grad err {e:.3e} (bar {2e-3 * gs + 1e-6:.3e})')
        assert e < 2e-3 * gs + 1e-6, name
    names = [name for name, _ in m.named_buffers()]
    assert not any('sd1_bn' in name for name in names) and len(names) == 9
    for (name, a), b in zip(m.named_buffers(), lib.buffers()):
        if name.endswith('num_batches_tracked'):
            assert int(a) == int(b), name
        else:
            assert torch.allclose(a.float(), b.float(), rtol=1e-4, atol=1e-5), name
