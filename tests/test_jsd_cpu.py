"""CPU-side checks of the occupancy / JSD boundary: header, exports and record mirror, the unchanged ABI number, the unchanged host
path of JSD, loud failure of the device entry points without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden, ROOT
from test_contract import _c_struct_fields, _mirror_fields
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, metrics
from go_with_the_flows_amd import evaluation as ev


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def test_header_declares_the_occupancy_entry_points_and_the_library_exports_them():
    header = _header()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert {'gwtf_voxel_occupancy', 'gwtf_jsd_counts'} <= declared
    assert 'typedef struct GwtfOccupancyArgs {' in header
    assert {'gwtf_voxel_occupancy', 'gwtf_jsd_counts'} <= set(_lib.EXPORTS)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, 'gwtf_voxel_occupancy') and hasattr(handle, 'gwtf_jsd_counts')


def test_occupancy_record_follows_the_header_field_for_field():
    declared = _c_struct_fields(_header(), 'GwtfOccupancyArgs')
    assert len(declared) >= 8
    assert _mirror_fields(_lib.OccupancyArgs) == declared
    assert ('edges', 'double[33]') in declared and ('n_points', 'size_t') in declared


def test_abi_version_is_still_12():
    assert re.search(r'#define GWTF_ABI_VERSION (\d+)', _header()).group(1) == '12'
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12


def test_bad_records_are_refused_before_anything_is_launched():
    L, E = _lib.lib(), 10001
    edges = metrics.occupancy_edges(28).tolist()

    def record(**over):
        a = _lib.OccupancyArgs(points=0x1000, n_points=10, res=28, bound=0.5, counts=0x1000)
        a.edges[:29] = edges
        for k, v in over.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert L.gwtf_voxel_occupancy(None) == E
    for bad in (dict(points=None), dict(counts=None), dict(n_points=0), dict(n_points=1 << 32), dict(res=0), dict(res=33),
                dict(bound=-1.0), dict(points=0x1002)):
        assert L.gwtf_voxel_occupancy(record(**bad)) == E, bad
    flat = _lib.OccupancyArgs(points=0x1000, n_points=10, res=28, bound=0.5, counts=0x1000)          # an edge table left at zero
    assert L.gwtf_voxel_occupancy(ctypes.byref(flat)) == E
    assert L.gwtf_jsd_counts(None, 0x1000, 8, 0x1000, None) == E
    assert L.gwtf_jsd_counts(0x1000, 0x1000, 0, 0x1000, None) == E
    assert L.gwtf_jsd_counts(0x1000, 0x1000, 8, None, None) == E


def test_the_edge_table_is_the_reference_expression():
    for res in (1, 8, 28, 32):
        assert np.array_equal(metrics.occupancy_edges(res), -0.5 + np.arange(res + 1) * (1. / res))


def test_numpy_inputs_keep_the_host_path():
    D = golden('g14_evaluation')
    occ = ev.get_voxel_occ_dist(D['c1'], warning=False)
    assert isinstance(occ, np.ndarray) and np.array_equal(occ, D['occ1'])
    assert np.array_equal(ev.get_voxel_occ_dist(D['c2'], warning=False), D['occ2'])
    jsd = ev.JSD(D['c1'], D['c2'], warning=False)
    assert not torch.is_tensor(jsd) and abs(float(jsd) - float(D['jsd'])) < 1e-12


def test_device_entry_points_refuse_cpu_tensors():
    clouds = torch.zeros(2, 16, 3)
    counts = torch.zeros(28, 28, 28, dtype=torch.int64)
    with pytest.raises(gw.GwtfError):
        metrics.voxel_occupancy(clouds)
    with pytest.raises(gw.GwtfError):
        metrics.voxel_occupancy(clouds, res=33)
    with pytest.raises(gw.GwtfError):
        metrics.jsd_from_counts(counts, counts)
    with pytest.raises(gw.GwtfError):
        ev.replace_nan_clouds(clouds)
    with pytest.raises(gw.GwtfError):
        ev.evaluate_generation(None, clouds)
