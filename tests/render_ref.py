"""A numpy restatement of gwtf_render_splats (include/gwtf.h, GwtfRenderArgs): float32 for the projection, rounded product by product
and sum by sum, integers after it.  Written from the header's rules, point by point and pixel by pixel, with Python integers where a
C int could overflow -- slow and plain on purpose.  The reference has no such code: this is the project's own statement of the rules."""
import math

import numpy as np

F = np.float32
EMPTY = (1 << 64) - 1


def ord32(d):
    """The order-preserving map of float32 bits to uint32."""
    b = int(np.asarray(d, F).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def project(view, p):
    """(u, v, d) of the point p under the (3, 4) view: t_r = ((M0 x + M1 y) + M2 z) + M3 in float32, d = t_2 + 0."""
    M, (x, y, z) = np.asarray(view, F), (F(c) for c in p)
    with np.errstate(all='ignore'):
        t = [F(F(F(F(M[r, 0] * x) + F(M[r, 1] * y)) + F(M[r, 2] * z)) + M[r, 3]) for r in range(3)]
        return t[0], t[1], F(t[2] + F(0.0))


def depth_cue(d, near, inv_range):
    with np.errstate(all='ignore'):
        f = np.floor(F(F(F(d - F(near)) * F(inv_range)) * F(256.0)))
    if math.isnan(f) or f <= 0:
        return 0
    return 255 if f >= 255 else int(f)


def footprint(u, v, radius_q, H, W):
    """The pixels (i, j) of the H x W cell the disc of a finite (u, v) covers."""
    with np.errstate(all='ignore'):
        u16, v16 = float(F(u * F(16.0))), float(F(v * F(16.0)))
    if math.isinf(u16) or math.isinf(v16):                 # finite, but farther out than any cell reaches
        return []
    U, V = int(math.floor(u16)), int(math.floor(v16))
    ic, jc = V >> 4, U >> 4
    pixels = []
    for i in range(max(0, (V - radius_q - 8) // 16 - 1), min(H - 1, (V + radius_q) // 16 + 1) + 1):
        for j in range(max(0, (U - radius_q - 8) // 16 - 1), min(W - 1, (U + radius_q) // 16 + 1) + 1):
            if (i == ic and j == jc) or (16 * j + 8 - U) ** 2 + (16 * i + 8 - V) ** 2 <= radius_q ** 2:
                pixels.append((i, j))
    return pixels


def render(clouds, labels, palette, view, H, W, *, label_base=0, radius_q=24, near=0.0, inv_range=0.0, fog=0, cols=1, cell0=0, cell_step=1,
           invalid_rgb=(0, 0, 0), background_rgb=(255, 255, 255), rgb=None, sheet=None):
    """-> {'rgb' (3, sheet_h, sheet_w) uint8, 'index' (B, H, W) int32, 'depth' (B, H, W) float32, 'skipped' (B,) int32, 'drawn' (B,): covered
    pixels per image, 'off_cell' (B,): finite points that draw nothing}.  rgb: the sheet to draw into (a copy is written), or
    sheet = (sheet_h, sheet_w) for a zero-filled one; by default the smallest sheet of `cols` columns that holds the cells."""
    clouds, palette, view = np.asarray(clouds, F), np.asarray(palette, np.uint8), np.asarray(view, F)
    B, _, N = clouds.shape
    P = palette.shape[0]
    if rgb is not None:
        rgb = np.array(rgb, np.uint8)
    else:
        if sheet is None:
            sheet = (((cell0 + (B - 1) * cell_step) // cols + 1) * H, cols * W)
        rgb = np.zeros((3,) + tuple(sheet), np.uint8)
    index = np.full((B, H, W), -1, np.int32)
    depth = np.full((B, H, W), np.inf, F)
    skipped, drawn, off_cell = np.zeros(B, np.int32), np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        M = view[b] if view.ndim == 3 else view
        keys = {}
        ds = {}
        for n in range(N):
            u, v, d = project(M, clouds[b, :, n])
            if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(d)):
                skipped[b] += 1
                continue
            pixels = footprint(u, v, radius_q, H, W)
            off_cell[b] += not pixels
            key = (ord32(d) << 32) | n
            ds[n] = d
            for px in pixels:
                keys[px] = min(keys.get(px, EMPTY), key)
        c = cell0 + b * cell_step
        oy, ox = (c // cols) * H, (c % cols) * W
        assert oy + H <= rgb.shape[1] and ox + W <= rgb.shape[2]
        rgb[:, oy:oy + H, ox:ox + W] = np.asarray(background_rgb, np.uint8)[:, None, None]
        for (i, j), key in keys.items():
            n = key & 0xffffffff
            d = ds[n]
            assert ord32(d) == key >> 32
            l = 0 if labels is None else int(labels[b][n]) - int(label_base)
            colour = invalid_rgb if l < 0 else palette[l % P]
            w = 256 - ((int(fog) * depth_cue(d, near, inv_range)) >> 8)
            rgb[:, oy + i, ox + j] = [(int(ch) * w) >> 8 for ch in colour]
            index[b, i, j], depth[b, i, j] = n, d
        drawn[b] = len(keys)
    return {'rgb': rgb, 'index': index, 'depth': depth, 'skipped': skipped, 'drawn': drawn, 'off_cell': off_cell}
