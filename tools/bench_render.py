#!/usr/bin/env python3
"""A sheet of labelled clouds drawn three ways.

* fused      render.render_clouds into a sheet of the caller's: ONE launch of gwtf_render_splats (csrc/gwtf_render.hip), eager and as
             a replayed graph.
* composed   the same sheet from torch operators on the device: the projection, a window of candidate pixels per point, int64 keys
             (ord(d) << 32) | n, scatter_reduce_('amin') into a key image, a gather of the winners' colours.  Same rules, so its
             pixels are compared with the fused sheet before anything is timed.
* matplotlib the reference-shaped host path where matplotlib is importable: device-to-host copies of clouds and labels, rotate on the
             host, one scatter call per panel (lib/visualization/utils.py:41-61), the figure rendered to a pixel buffer.

Cases: the reference's figure (5 x 2 cells, 2048 points), a sweep sheet (64 x 11 cells, 2048 points), both at 256 x 256 cells, and
one cloud of 100 000 points.  The device variants ALTERNATE inside each of `--windows` windows; a window times `--calls` consecutive
calls with stream events and reports ms per call; the figure of a variant is the median over the windows with the smallest and largest
beside it.  matplotlib is timed by the wall clock, once per window (it is three orders slower).  Beside the times: the byte model,
12 B per point per tile the cloud is scanned by plus 3 B per pixel written.  GPU box only.

    python tools/bench_render.py [--out profiles/r33_render.jsonl]     -> one JSON line per case
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from go_with_the_flows_amd import render  # noqa: E402

DEV = 'cuda:0'
CASES = {'figure_5x2': dict(rows=5, cols=2, n=2048), 'sweep_64x11': dict(rows=64, cols=11, n=2048), 'cloud_100k': dict(rows=1, cols=1, n=100000)}
SIZE, RADIUS_Q, FOG, TILE = (256, 256), 24, 96, 64
STREAM_TB_PER_S = (5.0, 6.0)


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def captured(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def composed_sheet(clouds, labels, views, palette, rows, cols, out):
    """The rules of include/gwtf.h (GwtfRenderArgs) from torch operators; label_base 1, near -1, inv_range 0.5."""
    B, _, N = clouds.shape
    H, W = SIZE
    x, y, z = clouds[:, 0], clouds[:, 1], clouds[:, 2]
    m = views.unsqueeze(-1)                                                        # (B, 3, 4, 1)
    t = [((m[:, r, 0] * x + m[:, r, 1] * y) + m[:, r, 2] * z) + m[:, r, 3] for r in range(3)]
    u, v, d = t[0], t[1], t[2] + 0.0
    ok = torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(d) & (u > -4) & (u < W + 4) & (v > -4) & (v < H + 4)
    U = torch.floor(torch.where(ok, u, 0.0) * 16.0).long()
    V = torch.floor(torch.where(ok, v, 0.0) * 16.0).long()
    bits = d.view(torch.int32).long() & 0xffffffff
    ordd = torch.where(bits >= 0x80000000, bits ^ 0xffffffff, bits | 0x80000000)
    key = (ordd << 32) | torch.arange(N, device=DEV).view(1, N)
    key = key - (1 << 63)                                                          # unsigned order in a signed int64
    span = RADIUS_Q // 16 + 1                                                      # candidate window: (2 span + 1)^2 pixels per point
    off = torch.arange(-span, span + 1, device=DEV)
    jc, ic = (U >> 4).unsqueeze(-1).unsqueeze(-1), (V >> 4).unsqueeze(-1).unsqueeze(-1)
    j, i = jc + off.view(1, 1, 1, -1), ic + off.view(1, 1, -1, 1)                  # (B, N, w, w)
    dx, dy = 16 * j + 8 - U.unsqueeze(-1).unsqueeze(-1), 16 * i + 8 - V.unsqueeze(-1).unsqueeze(-1)
    hit = ((dx * dx + dy * dy <= RADIUS_Q * RADIUS_Q) | ((j == jc) & (i == ic))) & ok.unsqueeze(-1).unsqueeze(-1)
    hit &= (j >= 0) & (j < W) & (i >= 0) & (i < H)
    cell = torch.arange(B, device=DEV).view(B, 1, 1, 1)
    flat = torch.where(hit, (cell * H + i) * W + j, B * H * W)                     # misses go to one spare slot
    empty = torch.iinfo(torch.int64).max
    image = torch.full((B * H * W + 1,), empty, dtype=torch.int64, device=DEV)
    image.scatter_reduce_(0, flat.reshape(-1), key.unsqueeze(-1).unsqueeze(-1).expand_as(flat).reshape(-1), 'amin')
    image = image[:-1].view(B, H * W)
    drawn = image != empty
    winner = torch.where(drawn, (image + (1 << 63)) & 0xffffffff, 0)
    lab = torch.gather(labels.long(), 1, winner) - 1
    colour = palette.long()[lab % palette.shape[0]]                                # (B, HW, 3)
    dw = torch.gather(d, 1, winner)
    q = torch.floor(((dw - (-1.0)) * 0.5) * 256.0).clamp(0, 255).long()
    w = 256 - ((FOG * q) >> 8)
    rgb = torch.where(drawn.unsqueeze(-1), (colour * w.unsqueeze(-1)) >> 8, 255).to(torch.uint8)
    out.view(3, rows, H, cols, W).copy_(rgb.view(rows, cols, H, W, 3).permute(4, 0, 2, 1, 3))
    return out


def matplotlib_figure(clouds, labels, rows, cols):
    """The reference-shaped host path: copies to the host, rotate, one scatter per panel, render to a buffer."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    pts = clouds.detach().cpu().numpy()
    lab = labels.detach().cpu().numpy()
    pts = np.einsum('ij,kjl->kil', render.rotation(), pts)
    colours = render.PALETTE / 255.0
    fig, axs = plt.subplots(rows, cols, figsize=(15, 15), squeeze=False)
    for b in range(rows * cols):
        axs[b // cols, b % cols].scatter(pts[b, 0], pts[b, 1], s=10.0, alpha=0.5, c=colours[(lab[b] - 1) % len(colours)])
    fig.canvas.draw()
    buf = np.asarray(fig.canvas.buffer_rgba())
    plt.close(fig)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--matplotlib-max-panels', type=int, default=64, help='matplotlib is run on cases of at most this many panels')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    try:
        import matplotlib  # noqa: F401
        have_mpl = True
    except ImportError:
        have_mpl = False
    H, W = SIZE
    lines = []
    for name, c in CASES.items():
        rows, cols, n = c['rows'], c['cols'], c['n']
        B = rows * cols
        gen = torch.Generator().manual_seed(B + n)
        clouds = (0.3 * torch.randn(B, 3, n, generator=gen)).to(DEV)
        labels = torch.randint(1, 9, (B, n), generator=gen).to(torch.int32).to(DEV)
        views = render.fit_views(clouds, size=SIZE)
        palette = torch.from_numpy(render.PALETTE).to(DEV)
        sheet_f = render.new_sheet(rows, cols, SIZE, DEV)
        sheet_c = render.new_sheet(rows, cols, SIZE, DEV)

        def fused():
            render.render_clouds(clouds, labels, label_base=1, views=views, size=SIZE, radius=RADIUS_Q / 16, fog=FOG, cols=cols, out=sheet_f)

        @torch.no_grad()
        def composed():
            composed_sheet(clouds, labels, views, palette, rows, cols, sheet_c)

        fused()
        composed()
        torch.cuda.synchronize()
        differing = int((sheet_f != sheet_c).any(0).sum())
        variants = {'fused_eager': fused, 'composed_eager': composed}
        graphs = {'fused_graph': captured(fused), 'composed_graph': captured(composed)}
        variants.update({k: g.replay for k, g in graphs.items()})
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        mpl = []
        for _ in range(a.windows):
            for k, fn in variants.items():
                ms[k].append(window(fn, a.calls))
            if have_mpl and B <= a.matplotlib_max_panels:
                t0 = time.perf_counter()
                matplotlib_figure(clouds, labels, rows, cols)
                mpl.append((time.perf_counter() - t0) * 1e3)
        tiles = -(-H // TILE) * -(-W // TILE)
        bytes_moved = 12 * n * tiles * B + 3 * H * W * B
        line = {'what': 'render', 'case': name, 'rows': rows, 'cols': cols, 'n': n, 'cell': list(SIZE), 'radius_q': RADIUS_Q, 'fog': FOG,
                'pixels_differing_fused_vs_composed': differing, 'pixels': B * H * W}
        for k, v in ms.items():
            line[k + '_ms'] = round(float(np.median(v)), 4)
            line[k + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
        if mpl:
            line['matplotlib_ms'] = round(float(np.median(mpl)), 1)
            line['matplotlib_ms_min_max'] = [round(min(mpl), 1), round(max(mpl), 1)]
        else:
            line['matplotlib_ms'] = None
            line['matplotlib_skipped'] = 'not importable' if not have_mpl else f'more than {a.matplotlib_max_panels} panels'
        line['byte_model_bytes'] = bytes_moved
        line['byte_model_us'] = [round(bytes_moved / (r * 1e12) * 1e6, 2) for r in reversed(STREAM_TB_PER_S)]
        line['fused_graph_TB_per_s'] = round(bytes_moved / (line['fused_graph_ms'] * 1e-3) / 1e12, 3)
        line['workgroups'] = tiles * B
        line['timed_by'] = (f'median of {a.windows} windows of {a.calls} calls per variant, variants alternating, stream events around each '
                            f'window, after {a.warmup} calls each; matplotlib: wall clock of one figure per window')
        line['device'] = torch.cuda.get_device_name(0)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del graphs, variants
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
