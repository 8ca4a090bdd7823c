"""Labelled point clouds as pictures, on the device: contact sheets of depth-tested splats (csrc/gwtf_render.hip).

The reference's qualitative output (lib/visualization/utils.py:41-61) rotates clouds by (25, 135, 0) degrees on the host and draws one
matplotlib scatter per panel, coloured by COLORS_PLT[label - 1].  Here the rotation, the scale and the offset of a panel are one
(3, 4) float32 VIEW matrix (view_matrix: one fixed window; fit_views: one window per cloud, matplotlib's per-axes autoscale), and
render_clouds turns B clouds with per-point labels into the cells of a (3, rows * H, cols * W) uint8 sheet in one launch -- the tensor
SummaryWriter.add_image and save_png take.  A view maps a point to (u, v, d): pixels of the cell, row 0 at the top, and a depth whose
[-1, 1] is the window's own depth range (nearer is smaller), which is what the depth cue darkens over.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import GwtfError

# COLORS_PLT of lib/visualization/utils.py:5-12 as bytes, and matplotlib's default scatter colour ('C0') for the unlabelled column
PALETTE = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0), (128, 0, 230), (230, 0, 128)],
                   np.uint8)
GROUND_TRUTH_RGB = (31, 119, 180)
BACKGROUND_RGB = (255, 255, 255)
INVALID_RGB = (128, 128, 128)
ANGLES = (25, 135, 0)                    # add_figures_reconstruction_tb, utils.py:43-44
NEAR, INV_RANGE = -1.0, 0.5              # the depth row of every view made here maps its window to [-1, 1]


def rotation(angles=ANGLES):
    """The reference's rotation, float64 (3, 3): get_rotation_matrix / rotate_np of lib/visualization/utils.py:15-38, R0(a0) . R1(a1) .
    R2(a2) with the angles in degrees and that file's sign conventions."""
    a0, a1, a2 = ((float(a) / 360) * 2 * np.pi for a in angles)
    c, s = np.cos, np.sin
    m0 = np.array([[1, 0, 0], [0, c(a0), -s(a0)], [0, s(a0), c(a0)]])
    m1 = np.array([[c(a1), 0, s(a1)], [0, 1, 0], [-s(a1), 0, c(a1)]])
    m2 = np.array([[c(a2), -s(a2), 0], [s(a2), c(a2), 0], [0, 0, 1]])
    return m0.dot(m1).dot(m2)


def view_matrix(angles=ANGLES, size=(256, 256), bound=1.0, center=(0, 0, 0), dtype=np.float32):
    """One fixed window as a (3, 4) view: a point p is rotated (``rotation``) about ``center`` and [-bound, bound]^2 of the rotated
    x, y plane is put into the middle of the H x W cell with one scale s = min(H, W) / (2 bound) for both axes, y up, z towards the
    viewer:  u = W / 2 + s xr,  v = H / 2 - s yr,  d = -zr / bound.  Composed in float64, returned as ``dtype`` (numpy)."""
    H, W = (int(v) for v in size)
    bound = float(bound)
    if H < 1 or W < 1 or not bound > 0 or not math.isfinite(bound):
        raise ValueError(f'view_matrix needs a positive size and bound, got {size} and {bound}')
    R, s = rotation(angles), min(H, W) / (2 * bound)
    A = np.stack([s * R[0], -s * R[1], -R[2] / bound])
    t = np.array([W / 2, H / 2, 0.0]) - A.dot(np.asarray(center, np.float64))
    return np.concatenate([A, t[:, None]], 1).astype(dtype)


def fit_views(clouds, angles=ANGLES, size=(256, 256), margin=0.05):
    """A window per cloud, (B, 3, 4) float32 on the device of ``clouds`` (B, 3, N): the extent of the rotated x and y of the cloud's
    finite points, centred in the cell with ``margin`` of the cell free on every side and ONE scale for both axes (the aspect is
    kept); the depth row maps the cloud's own rotated-z range to [-1, 1].  Torch operators on the device only: nothing is read back
    and the call can be captured.  The counterpart of matplotlib's per-axes autoscale."""
    if not torch.is_tensor(clouds) or clouds.dim() != 3 or clouds.shape[1] != 3:
        raise GwtfError(f'clouds must be a (B, 3, N) tensor, got {tuple(getattr(clouds, "shape", ()))}')
    if clouds.device.type != 'cuda':
        raise GwtfError(f'clouds must live on a HIP device (got {clouds.device}); there is no CPU path')
    H, W = (int(v) for v in size)
    if not 0 <= margin < 0.5:
        raise ValueError('margin must be in [0, 0.5)')
    R = rotation(angles).astype(np.float32).tolist()
    x, y, z = clouds[:, 0].float(), clouds[:, 1].float(), clouds[:, 2].float()
    rot = [R[r][0] * x + R[r][1] * y + R[r][2] * z for r in range(3)]                     # (B, N) each
    finite = torch.isfinite(rot[0]) & torch.isfinite(rot[1]) & torch.isfinite(rot[2])
    inf = float('inf')
    lo = [torch.where(finite, t, inf).amin(1) for t in rot]
    hi = [torch.where(finite, t, -inf).amax(1) for t in rot]
    mid = [torch.nan_to_num(0.5 * (a + b), nan=0.0, posinf=0.0, neginf=0.0) for a, b in zip(lo, hi)]
    ext = [torch.nan_to_num(b - a, nan=0.0, posinf=0.0, neginf=0.0).clamp_min(1e-12) for a, b in zip(lo, hi)]
    s = torch.minimum(W * (1 - 2 * margin) / ext[0], H * (1 - 2 * margin) / ext[1])      # (B,)
    sz = 2.0 / ext[2]
    rows = []
    for scale, r, offset in ((s, 0, W / 2), (-s, 1, H / 2), (-sz, 2, 0.0)):
        rows.append(torch.stack([scale * R[r][0], scale * R[r][1], scale * R[r][2], offset - scale * mid[r]], 1))
    return torch.stack(rows, 1).contiguous()                                             # (B, 3, 4)


_PALETTES = {}


def _device_palette(palette, dev):
    """palette as a contiguous (P, 3) uint8 tensor on dev; host values are copied once per (values, device)."""
    if torch.is_tensor(palette) and palette.device == dev:
        return palette.to(torch.uint8).contiguous()
    host = np.ascontiguousarray(palette.cpu().numpy() if torch.is_tensor(palette) else palette).astype(np.uint8)
    if host.ndim != 2 or host.shape[1] != 3 or not 1 <= host.shape[0] <= _lib.RENDER_MAX_PALETTE:
        raise GwtfError(f'palette must be (P, 3) with P in 1..{_lib.RENDER_MAX_PALETTE}, got {host.shape}')
    key = (host.tobytes(), str(dev))
    if key not in _PALETTES:
        _PALETTES[key] = torch.from_numpy(host).to(dev)
    return _PALETTES[key]


def sheet_shape(n_cells, size, cols=None):
    """(rows, cols) of a sheet of n_cells cells: ``cols`` per row, by default one row up to 8 cells and a near-square grid beyond."""
    if cols is None:
        cols = n_cells if n_cells <= 8 else int(math.ceil(math.sqrt(n_cells)))
    cols = int(cols)
    if cols < 1:
        raise GwtfError('cols must be positive')
    return -(-n_cells // cols), cols


def new_sheet(rows, cols, size, device, background=BACKGROUND_RGB):
    """A (3, rows * H, cols * W) uint8 sheet filled with the background colour."""
    H, W = (int(v) for v in size)
    sheet = torch.empty(3, rows * H, cols * W, device=device, dtype=torch.uint8)
    for ch in range(3):
        sheet[ch].fill_(int(background[ch]))
    return sheet


def render_clouds(clouds, labels=None, *, label_base=0, views=None, size=(256, 256), radius=1.5, palette=None, fog=96, cols=None,
                  out=None, cell0=0, cell_step=1, want_index=False, want_depth=False, skipped=None, angles=ANGLES, margin=0.05,
                  background=BACKGROUND_RGB, invalid=INVALID_RGB):
    """B clouds (B, 3, N) with per-point labels (B, N) -> the cells cell0 + b * cell_step of a contact sheet (3, rows * H, cols * W)
    uint8, one launch (gwtf_render_splats).  labels: float, uint8 or any int dtype (converted to int32), None: every point in
    palette[0]; label_base: 1 for the labels of the generators (generate_many, interpolate_many, ...), 0 for assign_many's, whose -1
    takes ``invalid``; labels beyond the palette wrap.  views: (3, 4) or (B, 3, 4) float32 (view_matrix / fit_views), None:
    fit_views(clouds, angles, size, margin).  radius: the disc's in pixels, in steps of 1 / 16.  palette: (P, 3) uint8, default
    PALETTE.  fog in 0..256: how much the farthest point of the view's depth range is darkened (0: palette bytes unchanged).
    out: the sheet to draw into -- only the B cells are written, so several calls share a sheet; without it a sheet of
    ``sheet_shape`` is made and filled with ``background``.  With out, int32 labels, views and (a cached or device) palette given the
    call allocates nothing.  want_index / want_depth: True, or the (B, H, W) int32 / float32 tensor to fill: the winning point of
    every pixel (-1: background) and its depth (+inf); skipped: a (B,) int32 tensor for the number of points with a non-finite
    projection.
    -> the sheet, or (sheet[, index][, depth]) with the maps asked for."""
    if not torch.is_tensor(clouds) or clouds.dim() != 3 or clouds.shape[1] != 3:
        raise GwtfError(f'clouds must be a (B, 3, N) tensor, got {tuple(getattr(clouds, "shape", ()))}')
    dev = clouds.device
    if dev.type != 'cuda':
        raise GwtfError(f'clouds must live on a HIP device (got {dev}); there is no CPU path')
    B, _, N = clouds.shape
    H, W = (int(v) for v in size)
    clouds = clouds.float().contiguous()
    if labels is not None:
        if not torch.is_tensor(labels) or tuple(labels.shape) != (B, N) or labels.device != dev:
            raise GwtfError(f'labels must be a ({B}, {N}) tensor on {dev}')
        labels = labels.to(torch.int32).contiguous()
    if views is None:
        views = fit_views(clouds, angles, size, margin)
    elif not torch.is_tensor(views):
        views = torch.from_numpy(np.ascontiguousarray(views, np.float32)).to(dev)
    views = views.float().contiguous()
    radius_q = int(round(16 * float(radius)))
    if not 0 <= radius_q <= _lib.RENDER_MAX_RADIUS_Q:
        raise GwtfError(f'radius must be in [0, {_lib.RENDER_MAX_RADIUS_Q // 16}] pixels, got {radius}')
    cell0, cell_step = int(cell0), int(cell_step)
    if out is None:
        rows, cols = sheet_shape(cell0 + (B - 1) * cell_step + 1, size, cols)
        out = new_sheet(rows, cols, size, dev, background)
    elif cols is None:
        if out.dim() != 3 or out.shape[2] % W:
            raise GwtfError(f'out must be (3, rows * {H}, cols * {W}), got {tuple(out.shape)}')
        cols = out.shape[2] // W
    maps = []
    for want, dtype in ((want_index, torch.int32), (want_depth, torch.float32)):
        maps.append(want if torch.is_tensor(want) else torch.empty(B, H, W, device=dev, dtype=dtype) if want else None)
    _lib.render_splats(clouds, labels, _device_palette(PALETTE if palette is None else palette, dev), views, out, H, W,
                       label_base=label_base, radius_q=radius_q, near=NEAR, inv_range=INV_RANGE, fog=fog, cols=cols, cell0=cell0,
                       cell_step=cell_step, invalid_rgb=invalid, background_rgb=background, index=maps[0], depth=maps[1], skipped=skipped)
    extra = tuple(m for m in maps if m is not None)
    return (out,) + extra if extra else out


def save_png(sheet, path):
    """Write a (3, H, W) uint8 sheet as a PNG (through PIL).  The one host copy of the picture happens here."""
    try:
        from PIL import Image
    except ImportError as e:
        raise GwtfError('save_png needs PIL (the pillow package), which is not importable here; SummaryWriter.add_image takes the '
                        'sheet as it is') from e
    if not torch.is_tensor(sheet) or sheet.dim() != 3 or sheet.shape[0] != 3 or sheet.dtype != torch.uint8:
        raise GwtfError('sheet must be a (3, H, W) uint8 tensor')
    Image.fromarray(sheet.permute(1, 2, 0).contiguous().cpu().numpy(), 'RGB').save(path, format='PNG')
    return path
