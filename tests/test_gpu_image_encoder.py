"""The HIP eval forward of the SVR image encoder (csrc/gwtf_resnet.hip) against float64 CPU torch of the same module, on the
conditioned state (synth.conditioned_image_encoder_).  Needs an MI355X."""
import copy

import numpy as np
import pytest
import torch

from conftest import record_parity
from go_with_the_flows_amd import _lib, resnet
from go_with_the_flows_amd._lib import GwtfError
from go_with_the_flows_amd.synth import conditioned_image_encoder_, synth_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = lambda t: t & 0xf                       # include/gwtf.h GWTF_TUNE_RESNET_TILE
SPLIT = lambda n: (n & 0xff) << 4              # GWTF_TUNE_RESNET_SPLIT

_ENC = {}


def encoder(nc=512):
    if nc not in _ENC:
        m = resnet.resnet18(num_classes=nc)
        conditioned_image_encoder_(m, 2200)
        _ENC[nc] = m.eval()
    return _ENC[nc]


def references(m, x):
    """(float64 CPU, float32 CPU) evaluations of the module graph."""
    with torch.no_grad():
        r64 = copy.deepcopy(m).double().forward_torch(x.double())
        r32 = copy.deepcopy(m).float().forward_torch(x.float())
    return r64, r32


def check(name, got, r64, r32):
    got = got.detach().cpu().double()
    scale = float(r64.abs().max())
    err = float((got - r64).abs().max())
    err32 = float((r32.double() - r64).abs().max())
    record_parity(name, err=err, err_torch_fp32=err32, scale=scale)
    assert err <= 1e-4 * scale, (name, err, scale)
    assert err <= max(2.0 * err32, 1e-6 * scale), (name, err, err32)


@pytest.mark.parametrize('B,H,W', [(1, 224, 224), (3, 224, 224), (64, 224, 224), (1, 97, 131), (3, 97, 131), (2, 32, 32)])
def test_eval_forward_matches_float64(B, H, W):
    m = encoder()
    x = torch.from_numpy(synth_images(B, H, W, 2201 + B + H))
    r64, r32 = references(m, x)
    md = copy.deepcopy(m).to(DEV)
    with torch.no_grad():
        got = md(x.to(DEV))
    assert got.shape == (B, 512)
    check(f'resnet_B{B}_{H}x{W}', got, r64, r32)


@pytest.mark.parametrize('tune', [TILE(1), TILE(2), TILE(3), TILE(1) | SPLIT(1), TILE(2) | SPLIT(1), TILE(2) | SPLIT(4),
                                  TILE(3) | SPLIT(7), TILE(1) | SPLIT(16), SPLIT(32)])
def test_every_tile_and_split_choice(tune):
    m = encoder()
    x = torch.from_numpy(synth_images(1, 224, 224, 2210))
    r64, r32 = references(m, x)
    md = copy.deepcopy(m).to(DEV)
    got = md.forward_hip(x.to(DEV), tune)
    check(f'resnet_tune_{tune:#x}', got, r64, r32)
    xb = torch.from_numpy(synth_images(3, 97, 131, 2211))
    r64b, r32b = references(m, xb)
    check(f'resnet_tune_{tune:#x}_B3', md.forward_hip(xb.to(DEV), tune), r64b, r32b)


def test_small_head_width_and_two_launches_are_bit_identical():
    m = encoder(16)
    md = copy.deepcopy(m).to(DEV)
    x = torch.from_numpy(synth_images(2, 64, 80, 2220))
    r64, r32 = references(m, x)
    a = md.forward_hip(x.to(DEV))
    check('resnet_nc16', a, r64, r32)
    big = copy.deepcopy(encoder()).to(DEV)
    x1 = torch.from_numpy(synth_images(1, 224, 224, 2221)).to(DEV)
    for tune in (0, SPLIT(8)):
        y1, y2 = big.forward_hip(x1, tune), big.forward_hip(x1, tune)
        assert torch.equal(y1, y2)
    assert torch.equal(a, md.forward_hip(x.to(DEV)))


def test_packed_cache_is_invalidated():
    m = copy.deepcopy(encoder()).to(DEV)
    x = torch.from_numpy(synth_images(1, 64, 64, 2230)).to(DEV)
    with torch.no_grad():
        y0 = m(x)
    p0 = m.packed()
    assert m.packed() is p0                                            # cached while nothing changes
    # load_state_dict
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd['layer3.1.bn2.running_var'] *= 2.0
    m.load_state_dict(sd)
    with torch.no_grad():
        y1 = m(x)
    assert not torch.equal(y0, y1)
    r64, r32 = references(m.cpu(), x.cpu())
    m.to(DEV)
    check('resnet_after_load_state_dict', y1, r64, r32)
    # an optimizer step (in-place parameter update: _version changes)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    m.train()
    loss = m(torch.cat([x, x * 0.5])).mean()
    loss.backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        y2 = m(x)
    r64, r32 = references(m.cpu(), x.cpu())
    m.to(DEV)
    check('resnet_after_optimizer_step', y2, r64, r32)
    # train() -> eval(): running statistics moved by the train-mode pass
    m.train()
    with torch.no_grad():
        m(torch.cat([x, -x]))
    m.eval()
    with torch.no_grad():
        y3 = m(x)
    r64, r32 = references(m.cpu(), x.cpu())
    check('resnet_after_train_eval', y3, r64, r32)


def test_bad_inputs_raise():
    m = copy.deepcopy(encoder()).to(DEV)
    with torch.no_grad():
        with pytest.raises(GwtfError):
            m(torch.zeros(1, 4, 64, 64))                                # CPU tensor
        with pytest.raises(GwtfError):
            m(torch.zeros(1, 4, 64, 64, device=DEV, dtype=torch.float64))
        with pytest.raises(GwtfError):
            m(torch.zeros(1, 3, 64, 64, device=DEV))                    # channels
        with pytest.raises(GwtfError):
            m(torch.zeros(1, 4, 31, 64, device=DEV))                    # too small
        with pytest.raises(GwtfError):
            m.forward_hip(torch.zeros(1, 4, 64, 64, device=DEV), TILE(9))
    L = _lib.lib()
    assert L.gwtf_resnet_work_floats(0, 64, 64, 0) == 0 and L.gwtf_resnet_work_floats(1, 16, 64, 0) == 0
    out = torch.empty(1, 512, device=DEV)
    assert L.gwtf_resnet_forward(None, None, out.data_ptr(), None, 1, 64, 64, 512, 0, None) == 10001
    assert L.gwtf_resnet_forward(out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), 1, 64, 64, 0, 0, None) == 10001


def test_train_mode_runs_the_library_path_with_gradients():
    m = copy.deepcopy(encoder(16)).to(DEV).train()
    x = torch.from_numpy(synth_images(3, 64, 64, 2240)).to(DEV).requires_grad_(True)
    y = m(x)
    with torch.no_grad():
        ref = copy.deepcopy(m).forward_torch(x)
    # (batch statistics over 3 images: library convolution algorithms differ from call to call by fp32 rounding, which the
    # normalisation by a small batch variance amplifies)
    assert float((y - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
    y.square().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(m.conv1.weight.grad.abs().sum()) > 0 and float(m.layer4[1].conv2.weight.grad.abs().sum()) > 0
