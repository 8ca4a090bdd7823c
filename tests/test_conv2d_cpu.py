"""CPU-side checks of the HIP convolution boundary (csrc/gwtf_conv2d.hip, conv2d.py, ResNet.train_conv): header, exports and record
mirror, the unchanged ABI number, the host-only planner over every convolution of resnet18 and over the geometries it refuses, the
train_conv attribute, and every Python refusal -- all before any device work."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from test_contract import _c_struct_fields, _mirror_fields
from go_with_the_flows_amd import _lib, conv2d as c2d
from go_with_the_flows_amd._lib import GwtfError
from go_with_the_flows_amd.resnet import resnet18

NEW = {'gwtf_conv2d_plan', 'gwtf_conv2d_forward', 'gwtf_conv2d_backward_input', 'gwtf_conv2d_backward_weight'}
E_BADARG, E_UNSUPPORTED = 10001, 10002
PASSES = (_lib.CONV2D_FORWARD, _lib.CONV2D_BACKWARD_INPUT, _lib.CONV2D_BACKWARD_WEIGHT)


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def test_header_declares_the_conv2d_entry_points_and_the_library_exports_them():
    header = _header()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert NEW <= declared
    assert 'typedef struct GwtfConv2dArgs {' in header
    assert NEW <= set(_lib.EXPORTS) and NEW <= set(_lib._SIGNATURES) and declared == set(_lib.EXPORTS)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), name


def test_the_kernel_file_is_built_into_the_library():
    make = open(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=\s*(.*)$', make, re.M).group(1).split()
    assert 'gwtf_conv2d.hip' in srcs
    assert os.path.exists(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'gwtf_conv2d.hip'))


def test_abi_version_is_still_12():
    assert re.search(r'#define GWTF_ABI_VERSION (\d+)', _header()).group(1) == '12'
    assert _lib.ABI_VERSION == 12
    assert _lib.lib().gwtf_abi_version() == 12


def test_record_follows_the_header_field_for_field():
    declared = _c_struct_fields(_header(), 'GwtfConv2dArgs')
    assert len(declared) == 16
    assert _mirror_fields(_lib.Conv2dArgs) == declared
    assert [n for n, kind in declared if kind == 'pointer'] == ['x', 'w', 'y', 'dy', 'dx', 'dw', 'work', 'stream']
    assert (_lib.CONV2D_FORWARD, _lib.CONV2D_BACKWARD_INPUT, _lib.CONV2D_BACKWARD_WEIGHT) == tuple(
        int(re.search(r'#define GWTF_CONV2D_%s (\d+)' % n, _header()).group(1)) for n in ('FORWARD', 'BACKWARD_INPUT', 'BACKWARD_WEIGHT'))


def _plan(which, record=True, **over):
    """(status, splits, work_floats) of the host-only planner; record=False passes NULL."""
    f = dict(N=2, Cin=16, H=9, W=11, Cout=16, k=3, stride=1, pad=1)
    f.update(over)
    a = _lib.Conv2dArgs(**f)
    splits, floats = ctypes.c_int(-1), ctypes.c_size_t(0)
    status = _lib.lib().gwtf_conv2d_plan(ctypes.addressof(a) if record else None, which, ctypes.byref(splits), ctypes.byref(floats))
    return status, splits.value, floats.value


def _resnet18_convs(N, H, W):
    """(N, Cin, H, W, Cout, k, stride) of the 20 convolutions of resnet18 on an (N, 4, H, W) image, read off the modules."""
    net = resnet18(num_classes=8)
    half = lambda n: (n - 1) // 2 + 1
    out = [(N, 4, H, W, 64, 7, 2)]
    h, w = half(half(H)), half(half(W))                      # the stem, then its max-pool
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            for conv, hh, ww in ((blk.conv1, h, w),) + (((blk.downsample[0], h, w),) if blk.downsample is not None else ()):
                out.append((N, conv.in_channels, hh, ww, conv.out_channels, conv.kernel_size[0], conv.stride[0]))
            if blk.stride == 2:
                h, w = half(h), half(w)
            out.append((N, blk.conv2.in_channels, h, w, blk.conv2.out_channels, 3, 1))
    assert len(out) == 20
    return out


@pytest.mark.parametrize('shape', [(1, 4, 32, 32), (3, 4, 64, 64), (128, 4, 224, 224)], ids=lambda s: 'x'.join(map(str, s)))
def test_the_planner_takes_every_convolution_of_resnet18(shape):
    N, _, H, W = shape
    for n, cin, h, w, cout, k, stride in _resnet18_convs(N, H, W):
        for which in PASSES:
            status, splits, floats = _plan(which, N=n, Cin=cin, H=h, W=w, Cout=cout, k=k, stride=stride, pad=k // 2)
            assert status == 0, (cin, h, w, cout, k, stride, which)
            assert splits >= 1
            if which == _lib.CONV2D_FORWARD:
                assert (splits, floats) == (1, 0)
            elif which == _lib.CONV2D_BACKWARD_INPUT:
                assert (splits, floats) == (1, cout * cin * k * k)           # the transposed weight
            else:
                assert floats == (splits * cout * cin * k * k if splits > 1 else 0)
    if shape[0] == 128:                                       # hundreds of thousands of pixels per weight gradient: split
        assert _plan(_lib.CONV2D_BACKWARD_WEIGHT, N=128, Cin=64, H=56, W=56, Cout=64)[1] > 1


@pytest.mark.parametrize('over', [dict(k=5, pad=2), dict(stride=3), dict(pad=0), dict(k=1, pad=1), dict(Cout=24), dict(Cin=8),
                                  dict(Cin=4)], ids=lambda o: '_'.join(f'{k}{v}' for k, v in o.items()))
def test_the_planner_refuses_other_geometries_as_unsupported(over):
    for which in PASSES:
        assert _plan(which, **over)[0] == E_UNSUPPORTED
    assert _plan(_lib.CONV2D_FORWARD, Cin=4, k=7, pad=3, Cout=64, stride=2)[0] == 0      # the stem is what Cin = 4 is for


def test_the_planner_refuses_bad_arguments():
    for which in PASSES:
        assert _plan(which, record=False)[0] == E_BADARG
        assert _plan(which, N=0)[0] == E_BADARG
        assert _plan(which, N=65536)[0] == E_BADARG
        assert _plan(which, H=0)[0] == E_BADARG
        assert _plan(which, N=65535, Cin=64, H=224, W=224, Cout=64)[0] == E_BADARG        # x has more than 2^31 elements
        assert _plan(which)[0] == 0
    assert _plan(3)[0] == E_BADARG and _plan(-1)[0] == E_BADARG
    # the launches refuse a record without pointers on the host, before touching a device
    a = _lib.Conv2dArgs(N=2, Cin=16, H=9, W=11, Cout=16, k=3, stride=1, pad=1)
    L = _lib.lib()
    for fn in (L.gwtf_conv2d_forward, L.gwtf_conv2d_backward_input, L.gwtf_conv2d_backward_weight):
        assert fn(ctypes.addressof(a)) == E_BADARG
        assert fn(None) == E_BADARG


def test_train_conv_is_a_class_default_outside_the_state():
    from go_with_the_flows_amd.resnet import ResNet
    assert ResNet.train_conv == 'library'
    net = resnet18(num_classes=8)
    assert net.train_conv == 'library'
    assert 'train_conv' not in net.__dict__
    assert not any('train_conv' in k for k in net.state_dict())
    assert not any('train_conv' in n for n, _ in net.named_parameters())
    net.train_conv = 'hip'
    assert net.train_conv == 'hip' and ResNet.train_conv == 'library' and resnet18(num_classes=8).train_conv == 'library'
    assert not any('train_conv' in k for k in net.state_dict())


def _conv(**kw):
    args = dict(in_channels=16, out_channels=16, kernel_size=3, stride=1, padding=1, bias=False)
    args.update(kw)
    return nn.Conv2d(**args)


def test_conv2d_refuses_tensors_it_cannot_take():
    x = torch.randn(2, 16, 9, 11)
    with pytest.raises(GwtfError, match='HIP device'):
        c2d.conv2d(x, _conv())                                             # a CPU tensor
    with pytest.raises(GwtfError, match='float32'):
        c2d.conv2d(x.double(), _conv().double())
    with pytest.raises(GwtfError, match='contiguous'):
        c2d.conv2d(x.contiguous(memory_format=torch.channels_last), _conv())
    with pytest.raises(GwtfError, match='contiguous'):
        c2d.conv2d(torch.randn(2, 16, 9, 22)[..., ::2], _conv())          # a strided view
    with pytest.raises(GwtfError, match=r'\(N, C, H, W\)'):
        c2d.conv2d(x[0], _conv())


def test_conv2d_refuses_modules_it_cannot_take():
    x = torch.randn(2, 16, 9, 11)
    with pytest.raises(GwtfError, match='bias'):
        c2d.conv2d(x, _conv(bias=True))
    with pytest.raises(GwtfError, match='groups'):
        c2d.conv2d(x, _conv(groups=2))
    with pytest.raises(GwtfError, match='dilation'):
        c2d.conv2d(x, _conv(dilation=2, padding=2))
    with pytest.raises(GwtfError, match='padding'):
        c2d.conv2d(x, _conv(padding=0))
    with pytest.raises(GwtfError, match='padding'):
        c2d.conv2d(x, _conv(padding_mode='reflect'))
    with pytest.raises(GwtfError, match='square'):
        c2d.conv2d(x, _conv(kernel_size=(3, 1), padding=(1, 0)))
    with pytest.raises(GwtfError, match='nn.Conv2d'):
        c2d.conv2d(x, nn.Linear(4, 4))


def test_encoder_refuses_a_bad_train_conv_before_any_device_work():
    net = resnet18(num_classes=8).train()
    x = torch.randn(2, 4, 32, 32)
    net.train_conv = 'triton'
    with pytest.raises(GwtfError, match="train_conv must be 'library' or 'hip'"):
        net(x)
    net.train_norm = 'hip'
    with pytest.raises(GwtfError, match="train_conv must be 'library' or 'hip'"):
        net(x)
    net.train_conv, net.train_norm = 'hip', 'library'
    with pytest.raises(GwtfError, match='train_conv.*train_norm'):
        net(x)
    with pytest.raises(GwtfError, match='train_conv.*train_norm'):
        net.forward_train_hip(x)
    net.train_norm = 'hip'
    with pytest.raises(GwtfError, match='HIP device'):                    # the path is accepted; the CPU image is not
        net(x)
