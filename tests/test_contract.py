"""CPU-side checks of the boundary: checkpoint contract, C ABI exports, host logic, loud failure without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib
from go_with_the_flows_amd.synth import load_synth_


def test_state_dict_contract_matches_reference():
    spec = json.load(open(os.path.join(GOLDEN, 'contract.json')))
    m = gw.LocalCondRNVPDecoder(*spec['ctor'])
    sd = m.state_dict()
    assert [k for k, _, _ in spec['state_dict']] == list(sd.keys())          # names AND order
    for k, shape, dtype in spec['state_dict']:
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == 'torch.' + dtype, k
    # strict round trip
    m2 = gw.LocalCondRNVPDecoder(*spec['ctor'])
    load_synth_(m, 1)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_constructor_surface():
    d = gw.LocalCondRNVPDecoder(3, 19, 32, weight_std=0.02)
    assert (d.n_flows, d.f_n_features, d.g_n_features, d.weight_std) == (3, 19, 32, 0.02)
    assert len(d.flows) == 3 and [t.pattern for t in d.flows] == [0, 1, 0]
    assert [c.warp_inds for c in d.flows[1].couplings()] == [[0, 1], [0, 2], [1, 2]]
    assert d.flows[0].nvp2.keep_inds == [0, 2]
    assert gw.LocalCondRNVPDecoder.get_param_count(4, 64, 128) == 701952          # reference formula
    assert sum(p.numel() for p in gw.LocalCondRNVPDecoder(4, 64, 128).parameters()) == 705060
    with pytest.raises(ValueError):
        gw.CondRealNVPFlow3D(8, 8, warp_inds=[1, 0])
    with pytest.raises(ValueError):
        gw.CondRealNVPFlow3DTriple(8, 8, pattern=2)
    # near-identity init of the last layers (reference flows.py:52-58,87-93)
    c = gw.CondRealNVPFlow3D(64, 128)
    assert float(c.T_mu_1[1].bias.abs().max()) == 0.0 and float(c.T_mu_1[1].weight.std()) < 0.02
    assert float(c.T_logvar_0_cond_w[3].weight.std()) < 0.02


def test_library_loads_and_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), f'{name} declared in include/gwtf.h but not exported'
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.gwtf_abi_version() == _lib.ABI_VERSION
    assert b'bad argument' in L.gwtf_error_string(10001)


def _c_struct_fields(header, name):
    """[(field, kind)] of `typedef struct <name> { ... } <name>;` in declaration order; kind: pointer / int / float / double / size_t,
    with `[n]` behind it for an array field `name[n]`."""
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


def _mirror_fields(mirror):
    kinds = {ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_size_t: 'size_t',
             ctypes.c_void_p: 'pointer', ctypes.POINTER(ctypes.c_int): 'pointer'}
    return [(n, f'{kinds[t._type_]}[{t._length_}]' if issubclass(t, ctypes.Array) else kinds[t]) for n, t in mirror._fields_]


def test_ctypes_records_follow_the_header_field_for_field():
    """The records of _lib are hand-written mirrors of the structs of include/gwtf.h: same names, same order, same kind of C type,
    same array lengths -- a transposed or missing field would bind and load without complaint and shift every field behind it.
    The minimum field count of each record guards the header parser itself (a struct it reads only in part)."""
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    for c_name, mirror, at_least in (('GwtfStackArgs', _lib.StackArgs, 22), ('GwtfTrainCtx', _lib.TrainCtx, 43),
                                     ('GwtfEncTrainCtx', _lib.EncTrainCtx, 47), ('GwtfCloudArgs', _lib.CloudArgs, 31),
                                     ('GwtfRouteArgs', _lib.RouteArgs, 20), ('GwtfRoutedStackArgs', _lib.RoutedStackArgs, 17),
                                     ('GwtfHeadArgs', _lib.HeadArgs, 28), ('GwtfLatentLossArgs', _lib.LatentLossArgs, 23),
                                     ('GwtfImageArgs', _lib.ImageArgs, 28), ('GwtfNorm2dArgs', _lib.Norm2dArgs, 24)):
        declared = _c_struct_fields(header, c_name)
        assert len(declared) >= at_least, c_name
        assert _mirror_fields(mirror) == declared, c_name


def test_encoder_train_record_is_validated_before_anything_is_launched():
    """gwtf_enc_train_phase / _forward / _backward refuse (GWTF_E_BADARG, host only) a NULL record, bad sizes, a NULL required field
    and a phase or layer out of range."""
    L = _lib.lib()
    E = 10001

    def record(**over):
        t = _lib.EncTrainCtx(B=2, N=36, n_total=72.0)
        for name, ctype in t._fields_:                     # every pointer set: the address is never read by the validation
            if ctype is ctypes.c_void_p and name != 'stream':
                setattr(t, name, 0x1000)
            elif issubclass(ctype, ctypes.Array) and ctype._type_ is ctypes.c_void_p:
                getattr(t, name)[:] = [0x1000] * ctype._length_
        for name, value in over.items():
            if isinstance(value, tuple):
                getattr(t, name)[value[0]] = value[1]
            else:
                setattr(t, name, value)
        return t

    calls = (lambda a: L.gwtf_enc_train_phase(a, _lib.ENC_PHASE_FWD_INIT, 0), L.gwtf_enc_train_forward,
             lambda a: L.gwtf_enc_train_phase(a, _lib.ENC_PHASE_BWD_TOP, 0), L.gwtf_enc_train_backward)
    for call in calls:
        assert call(None) == E
        for bad in (dict(B=0), dict(N=6), dict(N=12292), dict(n_total=0.0), dict(x=None), dict(aff=(2, None)), dict(pooled=None)):
            assert call(ctypes.addressof(record(**bad))) == E, bad
    for call in calls[2:]:
        assert call(ctypes.addressof(record(g_pooled=None))) == E
        assert call(ctypes.addressof(record(dW=(3, None)))) == E
    ok = record()
    assert L.gwtf_enc_train_phase(ctypes.addressof(ok), 99, 0) == E
    assert L.gwtf_enc_train_phase(ctypes.addressof(ok), -1, 0) == E
    assert L.gwtf_enc_train_phase(ctypes.addressof(ok), _lib.ENC_PHASE_FWD_LAYER, 4) == E
    assert L.gwtf_enc_train_phase(ctypes.addressof(ok), _lib.ENC_PHASE_BWD_LAYER, 4) == E
    assert L.gwtf_enc_train_phase(ctypes.addressof(ok), _lib.ENC_PHASE_BWD_LAYER, -1) == E


def _filled(cls, *fields):
    """byref of a record of `cls` with every pointer but the stream set (the validation never reads an address), then the given dicts
    of fields in turn: a list sets an array field, a tuple (h, v) its entry h."""
    t = cls()
    for name, ctype in t._fields_:
        if ctype is ctypes.c_void_p and name != 'stream':
            setattr(t, name, 0x1000)
        elif issubclass(ctype, ctypes.Array) and ctype._type_ is ctypes.c_void_p:
            getattr(t, name)[:] = [0x1000] * ctype._length_
    for name, value in (item for d in fields for item in d.items()):
        if isinstance(value, tuple):
            getattr(t, name)[value[0]] = value[1]
        elif isinstance(value, list):
            getattr(t, name)[:] = value
        else:
            setattr(t, name, value)
    return ctypes.byref(t)                                     # (keeps the record alive for the call)


def test_head_and_latent_loss_records_are_validated_before_anything_is_launched():
    """gwtf_heads_forward / _backward and gwtf_latent_loss_forward / _backward refuse (GWTF_E_BADARG, host only) every record the
    header says they refuse: one call per rule, each a valid record with one thing wrong."""
    L = _lib.lib()
    E = 10001
    # two heads: batch-statistic BatchNorm + swish, and a log-softmax head
    heads = lambda **bad: _filled(_lib.HeadArgs, dict(n_heads=2, B=4, Din=8, bn_updates=1, Dout=[5, 3], bn_mode=[1, 0], act=[1, 2]), bad)
    both = (L.gwtf_heads_forward, L.gwtf_heads_backward)
    for call in both:
        assert call(None) == E
        for bad in (dict(n_heads=0), dict(n_heads=3), dict(x=None), dict(W=(0, None)), dict(W=(1, None)), dict(ypre=(1, None)),
                    dict(out=(0, None)),
                    dict(B=0), dict(B=65537), dict(Din=0), dict(Din=4097), dict(Dout=(1, 0)), dict(Dout=(0, 4097)),       # dims_ok
                    dict(bn_mode=(0, 3)), dict(bn_mode=(1, -1)), dict(act=(0, 3)), dict(act=(1, -1)),
                    dict(stats=(0, None)),                                                    # bn_mode != 0 without stats
                    dict(bn_mode=(1, 2), running_mean=(1, None)), dict(bn_mode=(0, 2), running_var=(0, None)),
                    dict(Dout=(1, 17)),                                                       # act 2 wider than a column block
                    dict(B=1),                                                                # batch statistics of one row
                    dict(bn_updates=0)):
            assert call(heads(**bad)) == E, bad
    for bad in (dict(g_out=(0, None)), dict(g_out=(1, None)), dict(g_y=(0, None)), dict(g_y=(1, None))):
        assert L.gwtf_heads_backward(heads(**bad)) == E, bad

    latent = lambda **bad: _filled(_lib.LatentLossArgs, dict(B=2, G=3, n2=2, rows=0, pw=1.0, gw=1.0, ew=1.0), bad)
    fwd_ptrs = ('nll', 'z', 'mu0', 'lv0', 'flow_lv', 'post_lv', 'workspace', 'out4')
    bwd_ptrs = ('g_out4', 'z', 'mu0', 'lv0', 'g_nll', 'g_z', 'g_mu0', 'g_lv0', 'g_flow_lv', 'g_post_lv')
    for call, ptrs in ((L.gwtf_latent_loss_forward, fwd_ptrs), (L.gwtf_latent_loss_backward, bwd_ptrs)):
        assert call(None) == E
        for rows in (0, 1):
            for bad in [dict(B=0), dict(G=0), dict(n2=0), dict(B=-1), dict(B=1 << 20, G=1 << 12)] + [{p: None} for p in ptrs]:
                assert call(latent(rows=rows, **bad)) == E, (rows, bad)
        assert call(latent(rows=2)) == E and call(latent(rows=-1)) == E
    W = L.gwtf_latent_loss_workspace_floats
    assert W(2, 3) == 2 and W(256, 2) == 4 and W(257, 1) == 4                    # two floats per block of 256 elements
    assert W(0, 3) == 0 and W(2, -1) == 0 and W(1 << 20, 1 << 12) == 0 and W(1 << 16, 1 << 15) == 0      # what the launches refuse


def test_buffer_sizes_and_raw_arena_layout():
    L = _lib.lib()
    for f, G in [(8, 16), (19, 128), (33, 512), (37, 128), (64, 128)]:
        FP = L.gwtf_padded_width(f)
        assert FP == (f + 15) // 16 * 16
        per = 2 * (3 * f * f + 2 * f * G + 20 * f + 2)
        assert L.gwtf_raw_coupling_floats(f, G) == per
        c = gw.CondRealNVPFlow3D(f, G, warp_inds=[0, 2])
        assert sum(t.numel() for t in c.raw_tensors()) == per
        assert L.gwtf_film_out_floats(f) == 6 * FP + 4
        assert L.gwtf_packed_w_coupling_floats(f) % 256 == 0
    d = gw.LocalCondRNVPDecoder(2, 8, 16)
    eng = d.engine()
    assert eng.C == 6 and eng.pattern0 == 0
    assert eng.raw_arena().numel() == 6 * L.gwtf_raw_coupling_floats(8, 16)


def test_no_cpu_fallback_and_bad_arguments():
    d = gw.LocalCondRNVPDecoder(1, 8, 16).eval()
    with pytest.raises(gw.GwtfError):
        d(torch.zeros(2, 3, 5), torch.zeros(2, 16))
    with pytest.raises(ValueError):
        d.engine().run(torch.zeros(2, 4, 5), torch.zeros(2, 16), 'inverse', False)
    with pytest.raises(ValueError):
        d.engine().run(torch.zeros(2, 3, 5), torch.zeros(2, 16), 'sideways', False)
    with pytest.raises(NotImplementedError):
        gw.LocalCondRNVPDecoder(1, 129, 16).engine()
    # bad arguments are rejected by the library itself before anything is launched
    L = _lib.lib()
    null_record = _lib.StackArgs(K=1, B=1, N=1, C=1, f=8, pattern0=0, mode=1, tune=0, eps=1e-6)     # valid shape, NULL pointers
    assert L.gwtf_stack_forward(ctypes.addressof(null_record)) == 10001
    assert L.gwtf_stack_forward(None) == 10001                                                      # a NULL record
    assert L.gwtf_pack_weights_k(None, None, None, 1, 1, 8, 16, 0, 0, None) == 10001
    assert L.gwtf_mixture_nll(None, None, None, None, None, None, None, 65, 1, 1, None) == 10001


def test_eval_packing_cache_invalidation_rules():
    d = gw.LocalCondRNVPDecoder(1, 8, 16)
    eng = d.engine()
    k0 = eng._key()
    assert eng._key() == k0
    with torch.no_grad():
        d.flows[0].nvp1.T_mu_1[1].bias.add_(1.0)          # tracked in-place edit
    k1 = eng._key()
    assert k1 != k0
    d.eval()                                               # train()/eval() bump the stamp (reference optimiser uses .data)
    k2 = eng._key()
    assert k2 != k1
    d.load_state_dict(d.state_dict())
    assert eng._key() != k2
    d.flows[0].nvp1.invalidate_packed_weights()
    assert eng._key() != k2


def test_library_keeps_no_tuning_state_and_the_tile_plan_follows_rounds():
    """the tuning word is an ARGUMENT (no setter is exported any more), and the forward's tile is chosen by
    resident rounds x the calibrated cost of a round (csrc/gwtf_stack.hip tile_cost), not by the point count alone.  Host-only:
    gwtf_stack_plan launches nothing."""
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), 'gwtf_debug_set_points_per_wave')
    plan = _lib.stack_plan
    # the bench workloads (K, B, N, f): airplane / autoencoding shard / SVR shard keep 64 points per wave (4, 1, 1.25 rounds of 512)
    assert plan(4, 64, 2048, 37) == (64, 2048)
    assert plan(4, 16, 2048, 33) == (64, 512)
    assert plan(4, 16, 2500, 33) in ((64, 640), (32, 1280))     # 1.25 rounds of 512 large tiles or 1.67 of 768 small ones: measured equal
    assert plan(1, 32, 2048, 64) == (32, 512)                   # M1: f = 64 at 64 points per wave runs the generic body, 2x the cost
    # whole rounds: 24 x 2048 points are 768 small workgroups = exactly three per compute unit (or 192 large ones, one each);
    # 16 x 2048 are 256 middle ones, 8 x 2048 are 256 small ones -- never a round with one straggler
    assert plan(1, 24, 2048, 33) in ((16, 768), (64, 192))
    assert plan(1, 16, 2048, 33) == (32, 256) and plan(1, 8, 2048, 33) == (16, 256)
    # one shape split over 16 components (the reference's sampling call): the smallest tile, 2 workgroups per component
    segs = [(k * 128, (k + 1) * 128) for k in range(16)]
    assert plan(16, 1, 2048, 19, segments=segs) == (16, 32)
    # a forced tile is honoured per call, and the host-side context manager restores the word on exit (also on an exception)
    assert plan(4, 64, 2048, 37, word=32) == (32, 4096)
    with pytest.raises(RuntimeError):
        with _lib.tuning(points_per_wave=16):
            assert _lib.tune_word() == 16 and plan(4, 64, 2048, 37) == (16, 8192)
            raise RuntimeError('boom')
    assert _lib.tune_word() == 0
