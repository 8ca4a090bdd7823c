"""CPU-side checks of the paired-evaluation boundary: header, exports and record mirror, the unchanged ABI number, records refused
without a device, the statement list EvalFrame.from_config derives from a config, loud failure of the device entry points on CPU
tensors."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT
from test_contract import _c_struct_fields, _mirror_fields
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, metrics, models
from go_with_the_flows_amd import evaluation as ev

NEW = {'gwtf_eval_frame', 'gwtf_chamfer_paired_partials', 'gwtf_chamfer_paired', 'gwtf_paired_finalise'}


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def test_header_declares_the_paired_entry_points_and_the_library_exports_them():
    header = _header()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert NEW <= declared
    assert 'typedef struct GwtfEvalFrameArgs {' in header
    assert NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), name


def test_frame_record_follows_the_header_field_for_field():
    declared = _c_struct_fields(_header(), 'GwtfEvalFrameArgs')
    assert len(declared) >= 16
    assert _mirror_fields(_lib.EvalFrameArgs) == declared
    assert ('shift', 'double[3]') in declared and ('scale', 'float') in declared


def test_abi_version_is_still_12():
    assert re.search(r'#define GWTF_ABI_VERSION (\d+)', _header()).group(1) == '12'
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12


def test_partial_count_is_host_only():
    L = _lib.lib()
    assert [L.gwtf_chamfer_paired_partials(n, m) for n, m in ((1, 1), (512, 512), (513, 1), (1, 2500), (2049, 1030))] == [1, 1, 2, 5, 5]
    assert L.gwtf_chamfer_paired_partials(0, 5) == 0 and L.gwtf_chamfer_paired_partials(5, -1) == 0


def test_bad_records_are_refused_before_anything_is_launched():
    L, E, p = _lib.lib(), 10001, 0x1000

    def record(**over):
        a = _lib.EvalFrameArgs(gen=p, ref=p, orig_s=p, orig_c=p, gen_out=p, ref_out=p, B=2, n=5, m=7, n_scale=1, translate=1,
                               row_scale=1, row_shift=1, scale=0.5)
        for k, v in over.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert L.gwtf_eval_frame(None) == E
    for bad in (dict(gen=None), dict(ref=None), dict(gen_out=None), dict(ref_out=None), dict(B=0), dict(B=65536), dict(n=0), dict(m=0),
                dict(n_scale=3), dict(n_scale=-1), dict(orig_s=None), dict(orig_c=None)):
        assert L.gwtf_eval_frame(record(**bad)) == E, bad
    thr = (ctypes.c_float * 8)(*[0.1] * 8)
    for bad in ((None, p, p, thr, 1, 2, 5, 7), (p, None, p, thr, 1, 2, 5, 7), (p, p, None, thr, 1, 2, 5, 7), (p, p, p, None, 1, 2, 5, 7),
                (p, p, p, thr, 9, 2, 5, 7), (p, p, p, thr, -1, 2, 5, 7), (p, p, p, thr, 1, 0, 5, 7), (p, p, p, thr, 1, 65536, 5, 7),
                (p, p, p, thr, 1, 2, 0, 7), (p, p, p, thr, 1, 2, 5, 0)):
        assert L.gwtf_chamfer_paired(*bad, None) == E, bad
    good = dict(partials=p, emd_cost=p, cd=p, cdl=p, cdr=p, emd=p, f1=p, meter=p, meter_head=1, n_thr=2, B=2, n=5, m=7)
    for bad in (dict(partials=None), dict(B=0), dict(B=65536), dict(n=0), dict(m=0), dict(n_thr=9), dict(n_thr=-1),
                dict(f1=None, meter=None), dict(emd_cost=None)):
        assert L.gwtf_paired_finalise(*dict(good, **bad).values(), None) == E, bad


def test_from_config_gives_the_statement_list_of_the_reference():
    s32 = float(torch.tensor(0.7, dtype=torch.float32))
    base = dict(cloud_scale=True, cloud_scale_scale=0.7, cloud_translate=True, cloud_translate_shift=[0.1, -0.2, 0.3],
                cloud_rescale2orig=False, cloud_recenter2orig=False, batch_size=7, some_other_key='ignored')
    tail = [('add64', (0.1, -0.2, 0.3)), ('mul_rows', 'orig_s'), ('add_rows', 'orig_c')]
    F = metrics.EvalFrame.from_config
    assert F(**base).statements() == [] == F().statements() == metrics.EvalFrame().statements()                     # all flags off
    assert F(unit_scale_evaluation=True, **base).statements() == [('mul', s32)]                                     # unit only
    assert F(orig_scale_evaluation=True, **base).statements() == [('mul', s32)] + tail                               # orig only
    assert F(unit_scale_evaluation=True, orig_scale_evaluation=True, **base).statements() == [('mul', s32)] * 2 + tail   # both: twice
    no_scale = dict(base, cloud_scale=False)
    assert F(orig_scale_evaluation=True, **no_scale).statements() == tail                                           # translate, no scale
    assert F(unit_scale_evaluation=True, **no_scale).statements() == []
    kept = dict(base, cloud_rescale2orig=True, cloud_recenter2orig=True, cloud_translate=False)
    assert F(orig_scale_evaluation=True, **kept).statements() == [('mul', s32)]
    f = F(orig_scale_evaluation=True, **base)
    assert isinstance(f.shift[0], float) and f.shift == (0.1, -0.2, 0.3)            # float64 values, not rounded to float32
    with pytest.raises(ValueError):
        metrics.EvalFrame(n_scale=3)
    with pytest.raises(ValueError):
        metrics.EvalFrame(translate=True, shift=(1.0, 2.0))


def test_device_entry_points_refuse_cpu_tensors():
    gen, ref = torch.zeros(2, 3, 16), torch.zeros(2, 3, 16)
    a, b = torch.zeros(2, 16, 3), torch.zeros(2, 16, 3)
    with pytest.raises(gw.GwtfError):
        metrics.clouds_to_eval_frame(gen, ref)
    with pytest.raises(gw.GwtfError):
        metrics.clouds_to_eval_frame(a, b)                       # and the wrong layout
    with pytest.raises(gw.GwtfError):
        metrics.chamfer_paired(a, b, (0.01,))
    with pytest.raises(gw.GwtfError):
        metrics.paired_metrics(a, b, (0.01,))
    batch = {'cloud': gen, 'eval_cloud': ref, 'image': torch.zeros(2, 4, 8, 8)}
    for fn in (ev.evaluate_autoencoding, ev.evaluate_reconstruction):
        with pytest.raises(gw.GwtfError):
            fn(None, [batch], 16)
        with pytest.raises(gw.GwtfError):
            fn(None, [], 16)                                     # an empty iterable
        with pytest.raises(gw.GwtfError):
            fn(None, [{'cloud': gen}], 16)
    assert gw.paired_metrics is metrics.paired_metrics and gw.evaluate_reconstruction is ev.evaluate_reconstruction


def test_autoencode_many_needs_autoencoding_mode():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='generating')
    m = models.Flow_Mixture_Model(**cfg)
    with pytest.raises(gw.GwtfError):
        m.autoencode_many(torch.zeros(2, 3, 16), 16)
    m.mode = 'training'
    with pytest.raises(gw.GwtfError):
        m.autoencode_many(torch.zeros(2, 3, 16), 16)
