"""The whole image encoder in train mode with ``train_norm='hip'`` AND ``train_conv='hip'`` (csrc/gwtf_norm2d.hip +
csrc/gwtf_conv2d.hip: no library call between the image and the pooled features) beside the default library path, forward + backward
on the device, each against the float64 CPU module graph; then the graphed SVR training step on that path against the eager one.
Needs an MI355X.

Set up exactly as tests/test_gpu_image_encoder_train.py, whose docstring has the reasoning: the same encoder, the shapes
(3, 4, 64, 64) and (2, 4, 97, 131), its image seeds (searched for the largest gap between a ReLU input of the float64 reference and
0), its kink margin, relative L2 per tensor and over all gradients together, and its bar and floor:
err_hip <= max(5 err_library, 6.8e-5), the yardstick being the library path on the same device."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden, record_parity
from go_with_the_flows_amd import conv2d as c2d, models, optim, resnet
from go_with_the_flows_amd.synth import conditioned_image_encoder_, synth_images
from go_with_the_flows_amd.training import GraphedTrainStep

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOOR = 6.8e-5          # the floor of tests/test_gpu_image_encoder_train.py
KINK_MARGIN = 5e-6
IMAGE_SEED = {(3, 64, 64): 2583, (2, 97, 131): 2577}

_ENC = []


def encoder():
    if not _ENC:
        m = resnet.resnet18(num_classes=64)
        conditioned_image_encoder_(m, 2400)
        _ENC.append(m.train())
    return _ENC[0]


def evaluate(m, x, dy, relu_inputs=None):
    """Output, parameter gradients and running statistics of one train-mode forward + backward of a fresh copy of m.
    relu_inputs: a list that receives the smallest |input| of every ReLU call (the modules apply it in place: a pre-hook)."""
    m = copy.deepcopy(m)
    if relu_inputs is not None:
        for mod in m.modules():
            if isinstance(mod, torch.nn.ReLU):
                mod.register_forward_pre_hook(lambda _, args: relu_inputs.append(float(args[0].detach().abs().min())))
    y = m(x) if x.is_cuda else m.forward_torch(x)
    y.backward(dy)
    out = {'output': y.detach()}
    out.update({'grad.' + n: p.grad for n, p in m.named_parameters()})
    out.update({'buf.' + n: b.detach() for n, b in m.named_buffers() if b.dtype.is_floating_point})
    tracked = {n: int(b) for n, b in m.named_buffers() if not b.dtype.is_floating_point}
    return {k: v.detach().cpu().double() for k, v in out.items()}, tracked


def rel_l2(a, ref, scale=None):
    return float((a - ref).norm() / (ref.norm() if scale is None else scale))


@pytest.mark.parametrize('B,H,W', [(3, 64, 64), (2, 97, 131)])
def test_train_forward_backward_against_float64(B, H, W, monkeypatch):
    m = encoder()
    x = torch.from_numpy(synth_images(B, H, W, IMAGE_SEED[B, H, W]))
    dy = torch.randn(B, 64, generator=torch.Generator().manual_seed(2402))
    relu_inputs = []
    ref, tracked_ref = evaluate(copy.deepcopy(m).double(), x.double(), dy.double(), relu_inputs)
    assert len(relu_inputs) == 18 and min(relu_inputs) > KINK_MARGIN, min(relu_inputs)     # the property of the input
    hip_convs = []
    real = c2d.Conv2dFn.apply
    monkeypatch.setattr(c2d.Conv2dFn, 'apply', lambda *a: hip_convs.append(tuple(a[1].shape)) or real(*a))
    got = {}
    for path, (norm, conv) in {'library': ('library', 'library'), 'hip': ('hip', 'hip')}.items():
        md = copy.deepcopy(m).to(DEV)
        md.train_norm, md.train_conv = norm, conv
        before = len(hip_convs)
        got[path], tracked = evaluate(md, x.to(DEV), dy.to(DEV))
        assert len(hip_convs) - before == (20 if conv == 'hip' else 0)                      # every convolution, or none
        assert tracked == tracked_ref and set(tracked.values()) == {1}, path
    grads = [k for k in ref if k.startswith('grad.')]
    grad_scale = float(torch.cat([ref[k].reshape(-1) for k in grads]).norm()) / np.sqrt(sum(ref[k].numel() for k in grads))
    failures = []

    def judge(name, err):
        record_parity(f'encoder_train_conv_{B}x{H}x{W}_{name}', err_hip=err['hip'], err_library=err['library'])
        if not err['hip'] <= max(5.0 * err['library'], FLOOR):
            failures.append((name, err))

    for k in ref:
        # fc.bias: fc_bn follows it, its exact gradient is 0 -- compared absolutely, against the scale of a gradient entry
        scale = grad_scale * np.sqrt(ref[k].numel()) if k == 'grad.fc.bias' else None
        judge(k, {n: rel_l2(got[n][k], ref[k], scale) for n in got})
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in grads])
    judge('all_gradients', {n: rel_l2(cat(got[n]), cat(ref)) for n in got})
    assert not failures, failures


def test_eval_mode_with_autograd_keeps_the_library_graph(monkeypatch):
    m = copy.deepcopy(encoder()).to(DEV)
    m.train_norm = m.train_conv = 'hip'
    x = torch.from_numpy(synth_images(3, 64, 64, 2410)).to(DEV)
    m.eval()
    lib = copy.deepcopy(m)
    lib.train_norm = lib.train_conv = 'library'

    def refuse(*a):
        raise AssertionError('an eval-mode call reached the HIP convolutions')
    monkeypatch.setattr(c2d.Conv2dFn, 'apply', refuse)
    ya, yb = m(x), lib(x)
    assert ya.requires_grad and float((ya - yb).abs().max()) <= 1e-5 * float(yb.abs().max())


def _svr_model():
    """The small configuration of tests/test_gpu_svr_fused.py build()."""
    import json
    import os
    from conftest import GOLDEN
    from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_
    D = golden('g21_svr')
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    return m.to(DEV), cfg, D


def test_graphed_svr_step_on_the_hip_conv_path_equals_the_eager_step():
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)
    D = golden('g21_svr')
    batches = [(dev(D['gcloud']) * s, dev(D['pcloud']) * s, dev(synth_images(4, 64, 64, seed))) for s, seed in ((1.0, 2123), (0.9, 2124))]
    runs = []
    for graphed in (False, True):
        m, cfg, _ = _svr_model()
        m.img_encoder.train_norm = m.img_encoder.train_conv = 'hip'
        noise = dev(D['noise_g'])
        m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
        m.train()
        crit = models.Flow_Mixture_Loss(**cfg)
        opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
        terms = []
        if graphed:
            step = GraphedTrainStep(m, crit, opt, *batches[0][:2], images_example=batches[0][2])
            for g_in, p_in, i_in in batches:
                terms.append([float(t) for t in step(g_in, p_in, i_in)])
        else:
            for g_in, p_in, i_in in batches:
                opt.zero_grad(set_to_none=True)
                enc, dec = m.forward_fused(g_in, p_in, images=i_in)
                out = crit.fused(enc, dec)
                out[0].backward()
                opt.step()
                terms.append([float(t.detach()) for t in out])
                del out, enc, dec
        runs.append((terms, {k: v.clone() for k, v in m.img_encoder.state_dict().items() if 'running_' in k or 'num_batches' in k}))
    (t0, s0), (t1, s1) = runs
    print('eager', t0, 'graphed', t1)
    for a, b in zip(sum(t0, []), sum(t1, [])):               # the bound of test_gpu_svr_fused.py for graphed against eager
        assert abs(a - b) < 1e-4 * abs(a), (t0, t1)
    assert int(s1['bn1.num_batches_tracked']) == 2 == int(s0['bn1.num_batches_tracked'])
    # ... and its rule for state after optimiser steps (Adam moves entries whose gradient is rounding noise by +-lr either way)
    rel = [float((s0[k].float() - s1[k].float()).abs().max() / (s0[k].float().abs().max() + 1e-3)) for k in s0]
    print('running statistics: max rel', max(rel), 'mean rel', sum(rel) / len(rel))
    assert max(rel) < 2e-2 and sum(rel) / len(rel) < 2e-4
