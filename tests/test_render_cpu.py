"""CPU-side checks of the splat renderer's boundary: header, export and record mirror, the unchanged ABI number, the view matrix and the
palette pinned to the genuine reference's rotation and colours (g24_render.npz), records refused without a device, loud failure of the
Python entry points on host tensors, and the numpy restatement (render_ref.py) on hand-made cases with known pictures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import render_ref as rr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, render
from go_with_the_flows_amd import evaluation as ev


def _header():
    return open(os.path.join(ROOT, 'include', 'gwtf.h')).read()


def _record_fields(header, name):
    """[(field, kind)] of `typedef struct <name> { ... } <name>;` in declaration order; kind 'pointer' or the C type, `[n]` behind it
    for an array field."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ctype, names = re.fullmatch(r'((?:const\s+)?(?:unsigned\s+)?\w+(?:\s*\*)?)\s*(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)', decl).groups()
        kind = 'pointer' if '*' in ctype else ctype
        assert kind in ('pointer', 'int', 'float', 'unsigned char'), decl
        for n in names.split(','):
            field, dim = re.fullmatch(r'(\w+)(\[\d+\])?', n.strip()).groups()
            fields.append((field, kind + (dim or '')))
    return fields


def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = _header()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert 'gwtf_render_splats' in declared and 'typedef struct GwtfRenderArgs {' in header
    assert 'gwtf_render_splats' in _lib.EXPORTS and declared == set(_lib.EXPORTS)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'gwtf_render_splats')
    srcs = re.search(r'^SRCS\s*:=\s*(.*)$', open(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'Makefile')).read(), re.M).group(1).split()
    assert 'gwtf_render.hip' in srcs and os.path.exists(os.path.join(ROOT, 'go_with_the_flows_amd', 'csrc', 'gwtf_render.hip'))


def test_record_follows_the_header_field_for_field():
    declared = _record_fields(_header(), 'GwtfRenderArgs')
    assert len(declared) == 27
    kinds = {ctypes.c_void_p: 'pointer', ctypes.c_int: 'int', ctypes.c_float: 'float'}
    mirror = [(n, f'unsigned char[{t._length_}]' if issubclass(t, ctypes.Array) else kinds[t]) for n, t in _lib.RenderArgs._fields_]
    assert mirror == declared
    assert [n for n, k in declared if k == 'pointer'] == ['clouds', 'labels', 'palette', 'view', 'rgb', 'index', 'depth', 'skipped', 'stream']
    assert dict(declared)['invalid_rgb'] == dict(declared)['background_rgb'] == 'unsigned char[3]'
    assert _lib.RenderArgs.invalid_rgb.offset + 3 == _lib.RenderArgs.background_rgb.offset            # six bytes, packed


def test_abi_version_is_still_12():
    assert re.search(r'#define GWTF_ABI_VERSION (\d+)', _header()).group(1) == '12'
    assert _lib.ABI_VERSION == 12 and _lib.lib().gwtf_abi_version() == 12


def test_package_exports():
    assert gw.render_clouds is render.render_clouds and gw.fit_views is render.fit_views and gw.view_matrix is render.view_matrix
    assert gw.save_png is render.save_png and gw.PALETTE is render.PALETTE and gw.GROUND_TRUTH_RGB == (31, 119, 180)
    assert gw.reconstruction_figure is ev.reconstruction_figure and gw.sweep_figure is ev.sweep_figure
    assert gw.segmentation_figure is ev.segmentation_figure


# ---- the view against the genuine reference's rotation ----------------------------------------------------------------------------------
def test_view_matrix_is_the_reference_rotation():
    d = golden('g24_render')
    cloud, rotated = d['cloud'], d['rotated']
    assert cloud.shape == (3, 3, 17) and cloud.dtype == np.float64
    # size (2, 2), bound 1: the scale is 1 and the offsets are (1, 1, 0) -- row 0 is x, row 1 is -y (y up), row 2 is -z (z to the viewer)
    M = gw.view_matrix(tuple(d['angles']), size=(2, 2), bound=1.0, dtype=np.float64)
    assert M.shape == (3, 4) and M.dtype == np.float64 and M[:, 3].tolist() == [1.0, 1.0, 0.0]
    got = np.einsum('ij,kjl->kil', M[:, :3], cloud)
    assert np.abs(got[:, 0] - rotated[:, 0]).max() <= 1e-12
    assert np.abs(got[:, 1] + rotated[:, 1]).max() <= 1e-12
    assert np.abs(got[:, 2] + rotated[:, 2]).max() <= 1e-12
    assert np.abs(np.einsum('ij,kjl->kil', render.rotation((25, 135, 0)), cloud) - rotated).max() <= 1e-12
    # the default is that rotation, in float32
    assert np.array_equal(gw.view_matrix(size=(2, 2)), M.astype(np.float32)) and gw.view_matrix().dtype == np.float32


def test_view_matrix_puts_the_bound_into_the_cell():
    H, W, bound, c = 48, 80, 0.5, np.array([0.1, -0.2, 0.3])
    M = gw.view_matrix((10, 20, 30), size=(H, W), bound=bound, center=c, dtype=np.float64)
    R = render.rotation((10, 20, 30))
    assert np.abs(M @ np.append(c, 1.0) - [W / 2, H / 2, 0]).max() < 1e-12                      # the centre is the cell's centre
    p = c + R.T @ np.array([bound, bound, bound])                                             # rotated (+b, +b, +b) from the centre
    assert np.abs(M @ np.append(p, 1.0) - [W / 2 + H / 2, 0.0, -1.0]).max() < 1e-12           # right of centre, top row, nearest depth
    with pytest.raises(ValueError):
        gw.view_matrix(bound=0.0)


def test_palette_is_the_reference_colours():
    d = golden('g24_render')
    assert gw.PALETTE.dtype == np.uint8 and gw.PALETTE.shape == (8, 3)
    assert np.array_equal(gw.PALETTE, np.round(255 * d['colors_plt']).astype(np.uint8))


# ---- records refused without a device ---------------------------------------------------------------------------------------------------
def _record(**over):
    p = 0x1000
    a = _lib.RenderArgs(clouds=p, labels=p, palette=p, view=p, rgb=p, index=p, depth=p, skipped=p, B=3, N=33, P=8, label_base=1,
                        view_stride=12, H=70, W=50, radius_q=24, fog=96, sheet_h=140, sheet_w=100, cols=2, cell0=0, cell_step=1,
                        near=-1.0, inv_range=0.5)
    for k, v in over.items():
        setattr(a, k, v)
    return ctypes.byref(a)


BAD_RECORDS = [dict(clouds=None), dict(palette=None), dict(view=None), dict(rgb=None),
               dict(B=0), dict(B=-1), dict(N=0), dict(N=-5), dict(H=0), dict(H=-1), dict(W=0), dict(W=-1),
               dict(P=0), dict(P=257), dict(P=-1), dict(view_stride=1), dict(view_stride=-12), dict(view_stride=24),
               dict(radius_q=-1), dict(radius_q=16 * 64 + 1), dict(fog=-1), dict(fog=257), dict(cols=0), dict(cols=-2),
               dict(sheet_w=99), dict(sheet_h=139), dict(cols=3), dict(cell0=2), dict(cell_step=2), dict(cell0=-1), dict(cell_step=-1), dict(cell_step=0),
               dict(sheet_h=0), dict(sheet_w=0)]


@pytest.mark.parametrize('bad', BAD_RECORDS, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_bad_records_are_refused_before_anything_is_launched(bad):
    L = _lib.lib()
    assert L.gwtf_render_splats(None) == 10001
    assert L.gwtf_render_splats(_record(**bad)) == 10001


def test_a_grid_beyond_an_int_is_unsupported():
    big = 1 << 20
    assert _lib.lib().gwtf_render_splats(_record(B=1, H=big + 1, sheet_h=big + 1)) == 10002
    # 2^14 x 2^14 tiles per image and 8 images: 2^31 workgroups
    assert _lib.lib().gwtf_render_splats(_record(B=8, H=big, W=big, cols=1, sheet_h=8 * big, sheet_w=big)) == 10002


def test_entry_points_refuse_host_tensors():
    clouds, labels = torch.zeros(2, 3, 8), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(gw.GwtfError):
        gw.render_clouds(clouds, labels)
    with pytest.raises(gw.GwtfError):
        gw.fit_views(clouds)
    with pytest.raises(gw.GwtfError):
        gw.render_clouds(clouds[0], labels)                                                   # and the wrong layout
    with pytest.raises(gw.GwtfError):
        _lib.render_splats(clouds, labels, torch.zeros(8, 3, dtype=torch.uint8), torch.zeros(3, 4), torch.zeros(3, 8, 16, dtype=torch.uint8), 8, 8)
    with pytest.raises(gw.GwtfError):
        ev.segmentation_figure(clouds, labels)
    with pytest.raises(gw.GwtfError):
        ev.sweep_figure({'clouds1': clouds, 'clouds2': clouds, 'interpolations': torch.zeros(2, 3, 8, 1), 'labels': torch.zeros(2, 8, 1)})
    with pytest.raises(gw.GwtfError):
        ev.reconstruction_figure(None, {'cloud': clouds, 'eval_cloud': clouds}, 8)
    with pytest.raises(gw.GwtfError):
        gw.save_png(torch.zeros(3, 4, 4), os.devnull)                                         # not uint8


def test_save_png_round_trip(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    sheet = torch.arange(3 * 5 * 7, dtype=torch.uint8).view(3, 5, 7)
    path = gw.save_png(sheet, str(tmp_path / 'sheet.png'))
    assert np.array_equal(np.asarray(Image.open(path)), sheet.permute(1, 2, 0).numpy())


# ---- the restatement on hand-made cases -------------------------------------------------------------------------------------------------
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)       # u = x, v = y, d = z
PAL = np.array([[200, 100, 50], [10, 20, 30], [1, 2, 3]], np.uint8)


def cloud_of(*points):
    return np.array(points, np.float32).T[None]                               # (1, 3, N)


def test_one_point_at_a_pixel_centre_colours_exactly_one_pixel():
    res = rr.render(cloud_of((2.5, 1.5, 0.0)), None, PAL, EYE, 4, 6, radius_q=0)
    assert res['drawn'].tolist() == [1] and res['index'][0, 1, 2] == 0 and (res['index'] == -1).sum() == 23
    assert res['rgb'][:, 1, 2].tolist() == [200, 100, 50]
    assert (np.delete(res['rgb'].reshape(3, -1), 1 * 6 + 2, axis=1) == 255).all()
    assert res['depth'][0, 1, 2] == 0 and np.isinf(np.delete(res['depth'].ravel(), 8)).all()
    # radius 8/16 reaches exactly the centre of the pixel the point sits in, 16/16 the four neighbours' centres too
    assert rr.render(cloud_of((2.5, 1.5, 0.0)), None, PAL, EYE, 4, 6, radius_q=15)['drawn'].tolist() == [1]
    assert rr.render(cloud_of((2.5, 1.5, 0.0)), None, PAL, EYE, 4, 6, radius_q=16)['drawn'].tolist() == [5]
    # a point anywhere inside a pixel covers that pixel even when no pixel centre is within the radius
    assert rr.render(cloud_of((2.99, 1.01, 0.0)), None, PAL, EYE, 4, 6, radius_q=0)['index'][0, 1, 2] == 0


def test_depth_order_ties_signs_and_zeros():
    labels = np.array([[0, 1]])
    at = lambda res: (int(res['index'][0, 0, 0]), res['rgb'][:, 0, 0].tolist())
    near_second = rr.render(cloud_of((0.5, 0.5, 2.0), (0.5, 0.5, 1.0)), labels, PAL, EYE, 2, 2, radius_q=0)
    assert at(near_second) == (1, [10, 20, 30]) and near_second['depth'][0, 0, 0] == 1.0         # of two points the nearer wins
    tie = rr.render(cloud_of((0.5, 0.5, 1.0), (0.5, 0.5, 1.0)), labels, PAL, EYE, 2, 2, radius_q=0)
    assert at(tie) == (0, [200, 100, 50])                                                         # equal depth: the lower index
    signs = rr.render(cloud_of((0.5, 0.5, 0.25), (0.5, 0.5, -3.0)), labels, PAL, EYE, 2, 2, radius_q=0)
    assert at(signs)[0] == 1 and signs['depth'][0, 0, 0] == -3.0                                  # negative sorts in front of positive
    zeros = rr.render(cloud_of((0.5, 0.5, 0.0), (0.5, 0.5, -0.0)), labels, PAL, EYE, 2, 2, radius_q=0)
    assert at(zeros)[0] == 0 and not np.signbit(zeros['depth'][0, 0, 0])                          # -0 and +0 tie
    zeros = rr.render(cloud_of((0.5, 0.5, -0.0), (0.5, 0.5, 0.0)), labels, PAL, EYE, 2, 2, radius_q=0)
    assert at(zeros)[0] == 0 and not np.signbit(zeros['depth'][0, 0, 0])
    assert rr.ord32(-0.0) != rr.ord32(0.0) and rr.ord32(np.float32(-1e-45)) < rr.ord32(0.0) < rr.ord32(np.float32(1e-45))
    assert rr.ord32(-np.inf) == 0x007fffff and rr.ord32(np.inf) == 0xff800000


def test_rejected_points_are_counted_only_when_not_finite():
    pts = cloud_of((0.5, 0.5, 0.0), (np.nan, 0.5, 0.0), (0.5, np.inf, 0.0), (0.5, 0.5, -np.inf), (100.0, 0.5, 0.0), (-3.0, -3.0, 0.0),
                   (3e38, 0.5, 0.0))
    res = rr.render(pts, None, PAL, EYE, 2, 2, radius_q=8)
    assert res['skipped'].tolist() == [3] and res['off_cell'].tolist() == [3] and res['drawn'].tolist() == [1]
    assert res['index'][0].tolist() == [[0, -1], [-1, -1]]
    only_nan = rr.render(cloud_of((np.nan, np.nan, np.nan)), None, PAL, EYE, 2, 2, radius_q=200)
    assert only_nan['skipped'].tolist() == [1] and only_nan['drawn'].tolist() == [0] and (only_nan['rgb'] == 255).all()
    # a point outside the cell whose disc reaches in draws, and is not "off cell"
    reach = rr.render(cloud_of((-0.5, 0.5, 0.0)), None, PAL, EYE, 2, 2, radius_q=16)
    assert reach['drawn'].tolist() == [1] and reach['off_cell'].tolist() == [0] and reach['index'][0, 0, 0] == 0


def test_colour_rules():
    pts = cloud_of((0.5, 0.5, 0.0), (1.5, 0.5, 0.5), (0.5, 1.5, 1.0), (1.5, 1.5, 9.0))
    labels = np.array([[1, 0, 3 + 1 + 1, 3]])                                                  # base 1: 0 -> -1 invalid; P + 1 wraps to 1
    plain = rr.render(pts, labels, PAL, EYE, 2, 2, label_base=1, radius_q=0, near=0.0, inv_range=1.0, fog=0, invalid_rgb=(9, 8, 7))
    assert plain['rgb'][:, 0, 0].tolist() == [200, 100, 50] and plain['rgb'][:, 0, 1].tolist() == [9, 8, 7]     # fog 0: bytes unchanged
    assert plain['rgb'][:, 1, 0].tolist() == [10, 20, 30] and plain['rgb'][:, 1, 1].tolist() == [1, 2, 3]
    fog = rr.render(pts, labels, PAL, EYE, 2, 2, label_base=1, radius_q=0, near=0.0, inv_range=1.0, fog=128, invalid_rgb=(9, 8, 7))
    assert fog['rgb'][:, 0, 0].tolist() == [200, 100, 50]                                      # q = 0 at the near end
    w = 256 - ((128 * 128) >> 8)                                                               # d = 0.5: q = 128
    assert fog['rgb'][:, 0, 1].tolist() == [(c * w) >> 8 for c in (9, 8, 7)]
    w = 256 - ((128 * 255) >> 8)                                                               # d = 1 and beyond: q = 255
    assert fog['rgb'][:, 1, 0].tolist() == [(c * w) >> 8 for c in (10, 20, 30)]
    assert fog['rgb'][:, 1, 1].tolist() == [(c * w) >> 8 for c in (1, 2, 3)]
    none = rr.render(pts, None, PAL, EYE, 2, 2, radius_q=0)
    assert (none['rgb'].reshape(3, -1) == PAL[0][:, None]).all()                               # NULL labels: palette[0]
    assert rr.depth_cue(np.float32(np.inf), 0.0, 0.0) == 0 and rr.depth_cue(np.float32(3e38), -3e38, 1.0) == 255


def test_cells_of_a_sheet():
    pts = np.concatenate([cloud_of((0.5, 0.5, 0.0)), cloud_of((1.5, 1.5, 0.0)), cloud_of((0.5, 1.5, 0.0))])
    res = rr.render(pts, None, PAL, EYE, 2, 2, radius_q=0, cols=2)                            # 3 cells in 2 columns: the last row half empty
    assert res['rgb'].shape == (3, 4, 4) and (res['rgb'][:, 2:, 2:] == 0).all()               # ... and untouched
    assert res['rgb'][0].tolist() == [[200, 255, 255, 255], [255, 255, 255, 200], [255, 255, 0, 0], [200, 255, 0, 0]]
    again = rr.render(pts[:2], None, PAL, EYE, 2, 2, radius_q=0, cols=4, cell0=1, cell_step=2, rgb=np.full((3, 2, 8), 7, np.uint8))
    assert again['rgb'][0].tolist() == [[7, 7, 200, 255, 7, 7, 255, 255], [7, 7, 255, 255, 7, 7, 255, 200]]
