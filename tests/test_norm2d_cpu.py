"""CPU-side checks of the fused train-mode BatchNorm2d layer (csrc/gwtf_norm2d.hip, norm2d.py, ResNet.train_norm): the C ABI
additions, every refusal, the encoder's switch and the byte model of tools/bench_svr_train.py.  No GPU."""
import copy
import ctypes
import importlib.util
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from go_with_the_flows_amd import _lib, norm2d, resnet
from go_with_the_flows_amd._lib import GwtfError

ENTRY_POINTS = ('gwtf_norm2d_partials', 'gwtf_norm2d_forward', 'gwtf_norm2d_backward')
E_BADARG, E_FEW_VALUES = 10001, 10003


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', _header()))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(handle, name), name
    makefile = open(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'Makefile')).read()
    assert 'gwtf_norm2d.hip' in re.search(r'^SRCS := (.*)$', makefile, re.M).group(1).split()


def test_abi_version_is_12():
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12
    assert re.search(r'#define GWTF_ABI_VERSION 12\b', _header())


def _c_struct_fields(header, name):
    """[(field, kind)] of `typedef struct <name> { ... } <name>;` in declaration order (the parser of tests/test_contract.py)."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ctype, names = re.fullmatch(r'((?:const\s+)?(?:unsigned\s+)?(?:long\s+)?\w+(?:\s*\*)?)\s*(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)',
                                    decl).groups()
        kind = 'pointer' if '*' in ctype else ctype
        assert kind in ('pointer', 'int', 'float', 'double', 'size_t'), decl
        for n in names.split(','):
            field, dim = re.fullmatch(r'(\w+)(\[\d+\])?', n.strip()).groups()
            fields.append((field, kind + (dim or '')))
    return fields


def test_ctypes_record_follows_the_header_field_for_field():
    kinds = {ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_size_t: 'size_t', ctypes.c_void_p: 'pointer'}
    declared = _c_struct_fields(_header(), 'GwtfNorm2dArgs')
    assert len(declared) == 24
    assert [(n, kinds[t]) for n, t in _lib.Norm2dArgs._fields_] == declared


def test_record_is_validated_on_the_host_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error, not with these codes."""
    L = _lib.lib()

    def record(**over):
        a = _lib.Norm2dArgs(N=2, C=3, H=5, W=5, relu=1, pool=0, eps=1e-5, momentum=0.1)
        for name, ctype in a._fields_:
            if ctype is ctypes.c_void_p and name not in ('stream', 'residual', 'd_residual'):
                setattr(a, name, 0x1000)                 # never read by the validation
        for name, value in over.items():
            setattr(a, name, value)
        return a

    for call in (L.gwtf_norm2d_forward, L.gwtf_norm2d_backward):
        assert call(None) == E_BADARG
        for bad in (dict(N=0), dict(C=0), dict(H=0), dict(W=-1), dict(N=65536), dict(x=None), dict(gamma=None), dict(stats=None),
                    dict(partials=None), dict(pool=1, relu=0), dict(pool=1, residual=0x1000), dict(pool=1, offsets=None),
                    dict(eps=-1.0), dict(momentum=1.5), dict(N=1 << 15, H=1 << 8, W=1 << 8)):
            assert call(ctypes.addressof(record(**bad))) == E_BADARG, bad
        assert call(ctypes.addressof(record(N=1, H=1, W=1))) == E_FEW_VALUES
    assert L.gwtf_norm2d_forward(ctypes.addressof(record(y=None))) == E_BADARG
    assert L.gwtf_norm2d_forward(ctypes.addressof(record(beta=None))) == E_BADARG
    for bad in (dict(dy=None), dict(dx=None), dict(dgamma=None), dict(dbeta=None), dict(y=None)):
        assert L.gwtf_norm2d_backward(ctypes.addressof(record(**bad))) == E_BADARG, bad
    assert b'more than 1 value per channel' in L.gwtf_error_string(E_FEW_VALUES)
    # the work-size query: S partials per channel; 0 for what the launches reject
    assert L.gwtf_norm2d_partials(1, 3, 1, 1) == 0 and L.gwtf_norm2d_partials(0, 3, 4, 4) == 0
    assert L.gwtf_norm2d_partials(3, 5, 7, 7) == 1
    assert L.gwtf_norm2d_partials(128, 64, 112, 112) == 32          # the stem at B = 128: 2048 workgroups
    assert L.gwtf_norm2d_partials(128, 512, 7, 7) == 1
    assert 1 <= L.gwtf_norm2d_partials(2, 3, 56, 56) <= 64


class _Claimed(torch.Tensor):
    """A CPU tensor that says it is on the device: what is refused AFTER the device check can be reached without a GPU."""
    is_cuda = property(lambda self: True)


def test_every_refusal_raises_before_any_device_work():
    bn = nn.BatchNorm2d(3)
    x = torch.randn(2, 3, 4, 4)
    with pytest.raises(GwtfError, match='HIP device'):
        norm2d.norm_act_2d(x, bn)                                                   # CPU tensors
    with pytest.raises(GwtfError, match='float32'):
        norm2d.norm_act_2d(x.double(), bn)
    with pytest.raises(GwtfError, match='float32'):
        norm2d.norm_act_2d(x.half(), bn)
    with pytest.raises(GwtfError, match='contiguous'):
        norm2d.norm_act_2d(x.contiguous(memory_format=torch.channels_last), bn)
    with pytest.raises(GwtfError, match='momentum'):
        norm2d.norm_act_2d(x, nn.BatchNorm2d(3, momentum=None))
    with pytest.raises(GwtfError, match='track_running_stats'):
        norm2d.norm_act_2d(x, nn.BatchNorm2d(3, track_running_stats=False))
    with pytest.raises(GwtfError, match='affine'):
        norm2d.norm_act_2d(x, nn.BatchNorm2d(3, affine=False))
    with pytest.raises(GwtfError, match='SyncBatchNorm'):
        norm2d.norm_act_2d(x, nn.SyncBatchNorm(3))
    with pytest.raises(GwtfError, match='residual'):
        norm2d.norm_act_2d(x, bn, residual=torch.randn(2, 3, 4, 5))
    with pytest.raises(GwtfError, match='train mode'):
        norm2d.norm_act_2d(x, nn.BatchNorm2d(3).eval())
    with pytest.raises(GwtfError, match='pool'):
        norm2d.norm_act_2d(x, bn, relu=False, pool=True)
    with pytest.raises(GwtfError, match='pool'):
        norm2d.norm_act_2d(x, bn, residual=x.clone(), pool=True)
    with pytest.raises(GwtfError, match='BatchNorm2d'):
        norm2d.norm_act_2d(x, nn.BatchNorm1d(3))
    with pytest.raises(GwtfError, match='more than 1 value per channel'):            # as torch refuses (1, C, 1, 1) in train mode
        norm2d.norm_act_2d(torch.randn(1, 3, 1, 1).as_subclass(_Claimed), _claimed_bn(3))
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean, torch.zeros(3))     # nothing was touched


def _claimed_bn(C):
    bn = nn.BatchNorm2d(C)
    for name in ('weight', 'bias'):
        setattr(bn, name, nn.Parameter(getattr(bn, name).data.as_subclass(_Claimed)))
    bn.running_mean, bn.running_var = bn.running_mean.as_subclass(_Claimed), bn.running_var.as_subclass(_Claimed)
    return bn


def test_train_norm_defaults_to_library_and_stays_out_of_the_contract():
    m = resnet.resnet18(num_classes=16)
    assert resnet.ResNet.train_norm == 'library' and m.train_norm == 'library'
    assert 'train_norm' not in m.__dict__
    keys = list(m.state_dict().keys())
    assert not any('train_norm' in k for k in keys)
    m.train_norm = 'hip'
    assert list(m.state_dict().keys()) == keys and not any('train_norm' in n for n, _ in m.named_parameters())
    assert resnet.ResNet.train_norm == 'library'                                     # set on the instance, not on the class


def test_train_norm_refusals_of_the_encoder():
    x = torch.randn(2, 4, 32, 32)
    other = resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1], num_classes=8).train()
    other.train_norm = 'hip'
    with pytest.raises(GwtfError, match='resnet18'):
        other(x.as_subclass(_Claimed))
    m = resnet.resnet18(num_classes=8).train()
    m.train_norm = 'triton'
    with pytest.raises(GwtfError, match='train_norm'):
        m(x.as_subclass(_Claimed))
    m.train_norm = 'hip'
    with pytest.raises(GwtfError, match='HIP device'):                               # a CPU tensor: no fallback to the module graph
        m(x)


def test_default_forward_is_the_module_graph_bit_for_bit():
    """forward refuses CPU tensors in train mode, so the input claims to be on the device: with the default the call goes through
    forward_torch and nothing else, in train mode and in eval mode with autograd."""
    torch.manual_seed(5)
    m = resnet.resnet18(num_classes=8).train()
    x = torch.randn(3, 4, 32, 32)
    for mode in (True, False):
        a, b = copy.deepcopy(m).train(mode), copy.deepcopy(m).train(mode)
        ya = a(x.as_subclass(_Claimed))
        yb = b.forward_torch(x)
        assert torch.equal(ya.as_subclass(torch.Tensor), yb)
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
    # eval mode with autograd keeps the library graph under 'hip' as well
    a, b = copy.deepcopy(m).eval(), copy.deepcopy(m).eval()
    a.train_norm = 'hip'
    assert torch.equal(a(x.as_subclass(_Claimed)).as_subclass(torch.Tensor), b.forward_torch(x))


def test_byte_model_at_the_training_shape():
    spec = importlib.util.spec_from_file_location('bench_svr_train', os.path.join(ROOT, 'tools', 'bench_svr_train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = mod.norm2d_byte_model(128, 224, 224)
    # by hand: stem E0 = 128 * 64 * 112^2 = 102 760 448 (pooled Ep = 25 690 112); layer1 4 x E1 = 25 690 112; layers 2..4 five layers
    # each of E = 12 845 056, 6 422 528, 3 211 264 (sum 22 478 848)
    assert got['activations'] == 102_760_448 + 4 * 25_690_112 + 5 * 22_478_848 == 317_915_136
    pairs = 2 * 25_690_112 + 2 * 22_478_848                       # bn1 -> relu layers; as many bn2 -> add -> relu layers
    relu, residual, plain = 40 * pairs, 48 * pairs, 32 * 22_478_848
    stem = 20 * 102_760_448 + 15 * 25_690_112
    assert (relu, residual, plain, stem) == (3_853_516_800, 4_624_220_160, 719_323_136, 2_440_560_640)
    assert got['total'] == relu + residual + plain + stem == 11_637_620_736
    assert got['stats'] == 4 * 317_915_136
    assert got['total'] == got['stats'] + got['apply_fwd'] + got['sums_bwd'] + got['apply_bwd']
