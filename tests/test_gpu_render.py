"""gwtf_render_splats, render.py and the figures of evaluation.py on the device, against the numpy restatement (render_ref.py).

Every output -- rgb, index, depth, skipped -- is compared BIT FOR BIT: the rules of include/gwtf.h fix every rounding of the float32
projection and everything behind it is integer arithmetic ("bit-exact where integer").  The clouds are crafted in
PIXEL coordinates and carried to the model's frame through the inverse of the case's view, so that a case knows where its points land:
on a tile corner, on the cell's last row and column, wholly and partly outside, at NaN and +-inf, on top of each other, at depths of
both signs and at both zeros."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
import render_ref as rr
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models, render
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_, synth_images

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
EYE64 = EYE.astype(np.float64)
SENTINEL = 7                                   # what the sheet holds before a call: cells the call does not own keep it
INVALID, BACKGROUND = (9, 80, 170), (250, 251, 252)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def pixel_cloud(N, H, W, rq, rng):
    """(3, N) float64 (u, v, d) in pixels of an H x W cell.  Every random point keeps its disc off the centre of the cell's last pixel
    column, so background is left whatever the radius; a lone point sits where a disc of any radius covers a part of the cell."""
    r = rq / 16
    if N == 1:
        return np.array([[1.25 - 0.6 * r], [2.5 - 0.6 * r], [0.25]])
    nan, inf = np.nan, np.inf
    large = r >= 0.4 * min(H, W)                                                     # a disc of the cell's own size
    cx = W - 1.6 - r if large else 2.5                                               # (kept off the last column like the random points)
    special = [(-50 - r, -50 - r, 0.3), (W + 40 + r, 3.0, 0.3),                      # 0, 1: wholly outside
               (-0.3 - 0.5 * r, 0.37 * H, -0.7), (0.4 * W - r, -0.2 - 0.7 * r, 0.6),  # 2, 3: partly outside, left and top
               (nan, 1.0, 0.0), (1.0, inf, 0.0), (1.0, 1.0, -inf), (-inf, nan, 1.0),  # 4..7: not finite
               (cx, 3.5, 0.0), (cx, 3.5, -0.0), (cx, 3.5, 0.0),                      # 8..10: coincident, at both zeros
               (cx + 0.75, 1.75, 0.5), (cx + 0.75, 1.75, 0.5), (cx + 0.75, 1.75, -0.5)]      # 11..13: coincident: a tie, and one in front
    if not large:                                                                    # (they would leave no background)
        special += [(W - 0.5, H - 0.5, 0.1), (W - 1.0, H - 1.0, -0.1)]               # 14, 15: the cell's last row and column
        special += [(min(W - 1, 64) + 0.0, min(H - 1, 64) + 0.0, -0.2)]              # 16: a tile corner (the cell's when it has one tile)
    pts = np.array(special[:N]).T
    rest = N - pts.shape[1]
    x = rng.uniform(-r - 3, W - 1.05 - r, rest)
    y = rng.uniform(-r - 3, H + r + 3, rest)
    d = rng.uniform(-1, 1, rest)
    return np.concatenate([pts, np.stack([x, y, d])], 1)


def random_view(rng, H, W):
    """A well-conditioned (3, 4) float32 view none of whose entries is round: every product and sum of the projection rounds."""
    A = render.rotation(rng.uniform(0, 360, 3)) * rng.uniform(0.7, 1.4, (3, 1)) * np.array([[W / 2.0], [H / 2.0], [1.0]])
    return np.concatenate([A, rng.uniform(-1, 1, (3, 1)) + np.array([[W / 2.0], [H / 2.0], [0.0]])], 1).astype(np.float32)


def make_case(N, H, W, rq, B, stride, labels, seed):
    """Inputs of one call.  Image 0 of a per-image call looks through EYE, so its crafted points land exactly; every other view is a
    random affine map, and the cloud is the pixel cloud carried back through its float64 inverse."""
    rng = np.random.RandomState(seed)
    views = [EYE if (b == 0 and stride == 12) else random_view(rng, H, W) for b in range(B if stride == 12 else 1)]
    clouds = []
    for b in range(B):
        M = views[b if stride == 12 else 0]
        M = EYE64 if M is EYE else M.astype(np.float64)
        pix = pixel_cloud(N, H, W, rq, rng)
        with np.errstate(invalid='ignore'):
            back = pix if M is EYE64 else np.linalg.inv(M[:, :3]) @ (pix - M[:, 3:])       # (a product with zeros would turn -0 into +0)
        clouds.append(back.astype(np.float32))
    case = dict(clouds=np.stack(clouds), view=np.stack(views) if stride == 12 else views[0], H=H, W=W, radius_q=rq, labels=None,
                label_base=0, palette=gw.PALETTE)
    if labels == 'base0':                                            # assign_many's: 0..K-1 and -1, K = 11 > P = 8
        case.update(labels=rng.randint(-1, 11, (B, N)).astype(np.int32), label_base=0)
    elif labels == 'base1':                                          # the generators': 1..K, and a 0 that is below the base
        case.update(labels=rng.randint(0, 12, (B, N)).astype(np.int32), label_base=1)
    elif labels == 'small_palette':
        case.update(labels=rng.randint(0, 5, (B, N)).astype(np.int32), palette=rng.randint(0, 256, (3, 3)).astype(np.uint8))
    return case


def run_device(case, sheet, *, fog, cols, cell0=0, cell_step=1, outputs=True):
    """One launch into the device tensor `sheet` -> (index, depth, skipped) device tensors or Nones."""
    c = case
    B, H, W = c['clouds'].shape[0], c['H'], c['W']
    extra = dict(index=torch.full((B, H, W), -5, dtype=torch.int32, device=DEV), depth=torch.full((B, H, W), -5.0, device=DEV),
                 skipped=torch.full((B,), -5, dtype=torch.int32, device=DEV)) if outputs else {}
    _lib.render_splats(dev(c['clouds']), None if c['labels'] is None else dev(c['labels']), dev(c['palette']), dev(c['view']), sheet, H, W,
                       label_base=c['label_base'], radius_q=c['radius_q'], near=-1.0, inv_range=0.5, fog=fog, cols=cols, cell0=cell0,
                       cell_step=cell_step, invalid_rgb=INVALID, background_rgb=BACKGROUND, **extra)
    return extra


def run_ref(case, sheet, *, fog, cols, cell0=0, cell_step=1):
    c = case
    return rr.render(c['clouds'], c['labels'], c['palette'], c['view'], c['H'], c['W'], label_base=c['label_base'], radius_q=c['radius_q'],
                     near=-1.0, inv_range=0.5, fog=fog, cols=cols, cell0=cell0, cell_step=cell_step, invalid_rgb=INVALID,
                     background_rgb=BACKGROUND, rgb=sheet)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_outputs(got, want):
    assert same_bits(host(got['index']), want['index'])
    assert same_bits(host(got['depth']), want['depth'])            # the BITS: -0 never appears, +inf is the background
    assert same_bits(host(got['skipped']), want['skipped'])


def check_non_trivial(want, case):
    cells = want['index'].shape[0] * case['H'] * case['W']
    assert 0 < int(want['drawn'].sum()) < cells, (want['drawn'], cells)


# ---- 1. the launch against the restatement over the grid of shapes ----------------------------------------------------------------------
CELLS = [(8, 8), (70, 50), (64, 64)]
GRID = list(itertools.product([1, 33, 257], CELLS, [0, 7, 24, 200]))
# what the grid does not multiply out rides along with its cases in turn, so that every option meets every N, cell and radius somewhere
B_STRIDE = [(1, 0), (3, 12), (1, 12), (3, 0)]
LABELS = [None, 'base0', 'base1', 'small_palette', 'base1']
GRID = [(N, cell, rq, *B_STRIDE[(k + k // 4) % 4], LABELS[k % 5], (0, 96)[(k + k // 12) % 2], k % 3 != 2) for k, (N, cell, rq) in enumerate(GRID)]
# discs spanning four tiles need a cell of more than one tile in both directions: one more cell, at the radius that asks for it
GRID += [(257, (70, 90), 200, 3, 12, 'base1', 96, True), (33, (70, 90), 200, 1, 0, 'base0', 0, True)]


def test_the_grid_meets_every_option():
    for col, values in ((3, {1, 3}), (4, {0, 12}), (5, set(LABELS)), (6, {0, 96}), (7, {True, False})):
        for fixed in (0, 1, 2):
            for v0 in {g[fixed] for g in GRID[:36]}:
                assert {g[col] for g in GRID if g[fixed] == v0} == values, (col, fixed, v0)


@pytest.mark.parametrize('N,cell,rq,B,stride,labels,fog,outputs', GRID,
                         ids=[f'N{g[0]}-{g[1][0]}x{g[1][1]}-r{g[2]}-B{g[3]}-s{g[4]}-{g[5]}-fog{g[6]}-{"maps" if g[7] else "rgb"}' for g in GRID])
def test_launch_equals_the_restatement_bit_for_bit(N, cell, rq, B, stride, labels, fog, outputs):
    H, W = cell
    case = make_case(N, H, W, rq, B, stride, labels, seed=1000 + 7 * N + H + rq)
    cols = 2 if B == 3 else 1                                        # 3 cells in 2 columns: the last sheet row is half empty
    rows = -(-B // cols)
    before = np.full((3, rows * H + 3, cols * W + 5), SENTINEL, np.uint8)            # and the sheet is larger than its cells
    sheet = dev(before)
    got = run_device(case, sheet, fog=fog, cols=cols, outputs=outputs)
    want = run_ref(case, before, fog=fog, cols=cols)
    check_non_trivial(want, case)
    assert same_bits(host(sheet), want['rgb'])
    if outputs:
        check_outputs(got, want)
    if N > 1:
        assert int(want['skipped'].sum()) == 4 * B and int(want['off_cell'].sum()) > 0
    if B == 3:
        assert (want['rgb'][:, H:2 * H, W:2 * W] == SENTINEL).all()                   # the empty cell of the last row


def test_crafted_points_land_where_the_case_says():
    """Image 0 of a per-image call: the tile-corner point, the last row and column, both zeros, the coincident tie."""
    H, W, rq = 70, 90, 24
    case = make_case(17, H, W, rq, 1, 12, None, seed=5)                # the crafted points alone
    sheet = dev(np.full((3, H, W), SENTINEL, np.uint8))
    got = run_device(case, sheet, fog=0, cols=1)
    want = run_ref(case, host(sheet), fog=0, cols=1)
    check_outputs(got, want)
    index, depth = host(got['index'])[0], host(got['depth'])[0]
    assert index[H - 1, W - 1] == 15 and index[64, 64] == 16 and index[63, 63] == 16 and index[63, 64] == 16 and index[64, 63] == 16
    assert index[3, 2] == 8 and depth[3, 2] == 0 and not np.signbit(depth[3, 2])       # (2.5, 3.5): three points at +0, -0, +0
    assert index[1, 3] == 13 and depth[1, 3] == -0.5                                   # (3.25, 1.75): the one in front
    assert host(got['skipped']).tolist() == [4]


# ---- 2. cells of a shared sheet ---------------------------------------------------------------------------------------------------------
def test_two_calls_fill_alternate_columns_of_one_sheet():
    H, W = 20, 12
    a, b = make_case(33, H, W, 24, 2, 12, 'base1', seed=41), make_case(33, H, W, 7, 2, 0, 'base0', seed=42)
    before = np.full((3, H, 4 * W), SENTINEL, np.uint8)
    sheet = dev(before)
    run_device(a, sheet, fog=96, cols=4, cell0=0, cell_step=2)
    after_a = run_ref(a, before, fog=96, cols=4, cell0=0, cell_step=2)['rgb']
    assert same_bits(host(sheet), after_a) and (after_a[:, :, W:2 * W] == SENTINEL).all() and (after_a[:, :, 3 * W:] == SENTINEL).all()
    run_device(b, sheet, fog=0, cols=4, cell0=1, cell_step=2)
    after_b = run_ref(b, after_a, fog=0, cols=4, cell0=1, cell_step=2)['rgb']
    assert same_bits(host(sheet), after_b) and same_bits(after_b[:, :, :W], after_a[:, :, :W]) and not (after_b == SENTINEL).any()


# ---- 3. the same bits on every call, eager and replayed ---------------------------------------------------------------------------------
def test_two_calls_and_two_replays_of_a_captured_call_give_the_same_bits():
    H, W, B = 70, 50, 3
    case = make_case(257, H, W, 24, B, 12, 'base1', seed=77)
    fresh = lambda: dev(np.full((3, 2 * H, 2 * W), SENTINEL, np.uint8))
    sheets = [fresh(), fresh()]
    outs = [run_device(case, s, fog=96, cols=2) for s in sheets]
    assert torch.equal(sheets[0], sheets[1]) and all(same_bits(host(outs[0][k]), host(outs[1][k])) for k in outs[0])
    clouds, labels, palette, view = dev(case['clouds']), dev(case['labels']), dev(case['palette']), dev(case['view'])
    sheet, index = fresh(), torch.empty(B, H, W, dtype=torch.int32, device=DEV)
    depth, skipped = torch.empty(B, H, W, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.render_splats(clouds, labels, palette, view, sheet, H, W, label_base=1, radius_q=24, near=-1.0, inv_range=0.5, fog=96, cols=2,
                           invalid_rgb=INVALID, background_rgb=BACKGROUND, index=index, depth=depth, skipped=skipped)
    for _ in range(2):
        for t in (sheet, index, depth, skipped):
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        # the cells are written whole, background included: nothing of the fill is left inside them
        assert torch.equal(sheet[:, :H], sheets[0][:, :H]) and torch.equal(sheet[:, H:, :W], sheets[0][:, H:, :W])
        assert torch.equal(index, outs[0]['index']) and same_bits(host(depth), host(outs[0]['depth'])) and torch.equal(skipped, outs[0]['skipped'])


# ---- 4. render.py -----------------------------------------------------------------------------------------------------------------------
def test_fit_views_puts_every_finite_point_inside_its_cell():
    rng = np.random.RandomState(12)
    B, N, H, W = 4, 200, 48, 80
    clouds = rng.normal(0, 1, (B, 3, N)) * rng.uniform(0.05, 30, (B, 3, 1)) + rng.uniform(-5, 5, (B, 3, 1))
    clouds[1, :, 5], clouds[2, 0, 7], clouds[2, 1, 9] = np.nan, np.inf, -np.inf
    clouds = clouds.astype(np.float32)
    views = gw.fit_views(dev(clouds), size=(H, W))
    assert views.shape == (B, 3, 4) and views.dtype == torch.float32 and views.is_contiguous()
    labels = rng.randint(1, 9, (B, N)).astype(np.int32)
    want = rr.render(clouds, labels, gw.PALETTE, host(views), H, W, label_base=1, radius_q=24, near=render.NEAR, inv_range=render.INV_RANGE, fog=96)
    assert want['off_cell'].tolist() == [0] * B and want['skipped'].tolist() == [0, 1, 2, 0]
    for b in range(B):
        uvd = np.array([rr.project(host(views)[b], clouds[b, :, n]) for n in range(N)])
        ok = np.isfinite(uvd).all(1)
        u, v, d = uvd[ok].T
        assert u.min() >= 0 and u.max() < W and v.min() >= 0 and v.max() < H and d.min() >= -1.001 and d.max() <= 1.001
        # one scale for both axes: the aspect is kept; and the larger extent fills the cell up to the margins
        M = host(views)[b].astype(np.float64)
        assert abs(np.linalg.norm(M[0, :3]) / np.linalg.norm(M[1, :3]) - 1) < 1e-6
        assert max((u.max() - u.min()) / W, (v.max() - v.min()) / H) == pytest.approx(0.9, abs=1e-3)
    # the whole path: render_clouds with its default views is the launch on fit_views, drawn into a white sheet of its own
    sheet, index, depth = gw.render_clouds(dev(clouds), dev(labels).float(), label_base=1, size=(H, W), cols=3, want_index=True, want_depth=True)
    assert sheet.shape == (3, 2 * H, 3 * W) and sheet.dtype == torch.uint8
    want = rr.render(clouds, labels, gw.PALETTE, host(views), H, W, label_base=1, radius_q=24, near=render.NEAR, inv_range=render.INV_RANGE, fog=96,
                     cols=3, invalid_rgb=render.INVALID_RGB, rgb=np.full((3, 2 * H, 3 * W), 255, np.uint8))
    check_non_trivial(want, dict(H=H, W=W))
    assert same_bits(host(sheet), want['rgb']) and same_bits(host(index), want['index']) and same_bits(host(depth), want['depth'])


def test_render_clouds_into_a_sheet_of_the_callers_allocates_nothing_and_can_be_captured():
    rng = np.random.RandomState(3)
    B, N, H, W = 2, 64, 16, 16
    clouds, labels = dev(rng.normal(0, 1, (B, 3, N)).astype(np.float32)), dev(rng.randint(0, 8, (B, N)).astype(np.uint8))
    view = dev(gw.view_matrix(size=(H, W), bound=3.0))
    eager = gw.render_clouds(clouds, labels, views=view, size=(H, W), radius=1.0)
    assert eager.shape == (3, H, 2 * W)
    out = torch.zeros(3, H, 2 * W, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert gw.render_clouds(clouds, labels, views=view, size=(H, W), radius=1.0, out=out) is out
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    want = rr.render(host(clouds), host(labels), gw.PALETTE, host(view), H, W, radius_q=16, near=-1.0, inv_range=0.5, fog=96, cols=2,
                     invalid_rgb=render.INVALID_RGB)
    assert same_bits(host(eager), want['rgb'])
    with pytest.raises(gw.GwtfError):
        gw.render_clouds(clouds, labels, views=view, size=(H, W), radius=65.0)
    with pytest.raises(gw.GwtfError):
        gw.render_clouds(clouds, labels, views=view, size=(H, W), out=torch.zeros(3, H, W, dtype=torch.uint8, device=DEV))      # one cell short


# ---- 5. the figures ---------------------------------------------------------------------------------------------------------------------
SIZE = (32, 32)


def figure_ref(sheet_cells, columns, views):
    """The restatement applied column by column: columns = [(clouds, labels, label_base, palette)] -> the sheet."""
    H, W = SIZE
    rows, n_cols = sheet_cells
    rgb = np.full((3, rows * H, n_cols * W), 255, np.uint8)
    drawn = 0
    for col, entry in enumerate(columns):
        if entry is None:
            continue
        clouds, labels, base, palette = entry
        res = rr.render(host(clouds), None if labels is None else host(labels), palette, host(views), H, W, label_base=base, radius_q=24,
                        near=render.NEAR, inv_range=render.INV_RANGE, fog=96, cols=n_cols, cell0=col, cell_step=n_cols,
                        invalid_rgb=render.INVALID_RGB, rgb=rgb)
        rgb, drawn = res['rgb'], drawn + int(res['drawn'].sum())
        assert res['skipped'].sum() == 0
    assert 0 < drawn < rows * len(columns) * H * W
    return rgb


ONE = np.array([gw.GROUND_TRUTH_RGB], np.uint8)


@pytest.fixture(scope='module')
def ae_model():
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg'], util_mode='autoencoding')
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    return m.to(DEV).eval()


def batch_of(B, N, seed):
    gen = torch.Generator().manual_seed(seed)
    return {'cloud': torch.randn(B, 3, N, generator=gen).to(DEV), 'eval_cloud': torch.randn(B, 3, N, generator=gen).to(DEV)}


def test_reconstruction_figure_is_the_restatement_on_what_autoencode_many_returns(ae_model):
    B, n = 3, 64
    batch = batch_of(B, 96, 8)
    sheet = gw.reconstruction_figure(ae_model, batch, n, state=gw.make_state(6, DEV, 2), size=SIZE)
    assert sheet.shape == (3, B * 32, 2 * 32) and sheet.dtype == torch.uint8 and sheet.device == torch.device(DEV) and sheet.is_contiguous()
    recon, labels = ae_model.autoencode_many(batch['cloud'], n, return_labels=True, state=gw.make_state(6, DEV, 2))
    views = gw.fit_views(batch['eval_cloud'], size=SIZE)
    want = figure_ref((B, 2), [(batch['eval_cloud'], None, 0, ONE), (recon, labels.to(torch.int32), 1, gw.PALETTE)], views)
    assert same_bits(host(sheet), want)
    again = gw.reconstruction_figure(ae_model, batch, n, state=gw.make_state(6, DEV, 2), size=SIZE)
    assert torch.equal(again, sheet)
    assert gw.reconstruction_figure(ae_model, batch, n, nr_samples=2, state=gw.make_state(6, DEV, 2), size=SIZE).shape == (3, 64, 64)
    with pytest.raises(gw.GwtfError):
        gw.reconstruction_figure(ae_model, batch, n, size=SIZE, cols=3)


def test_sweep_figure_is_the_restatement_on_what_interpolate_clouds_returns(ae_model):
    B, n, T = 3, 64, 3
    make = lambda: gw.evaluation.interpolate_clouds(ae_model, [batch_of(B, 96, 9)], n, n_batches=1, weights=[0.25, 0.5, 0.75],
                                                    state=gw.make_state(4, DEV, 1), generator=torch.Generator(device=DEV).manual_seed(5))
    out = make()
    sheet = gw.sweep_figure(out, size=SIZE)
    assert sheet.shape == (3, B * 32, (T + 2) * 32) and sheet.dtype == torch.uint8
    views = gw.fit_views(out['clouds1'], size=SIZE)
    steps = [(out['interpolations'][:, :, :, t].contiguous(), out['labels'][:, :, t].to(torch.int32), 1, gw.PALETTE) for t in range(T)]
    want = figure_ref((B, T + 2), [(out['clouds1'], None, 0, ONE)] + steps + [(out['clouds2'], None, 0, ONE)], views)
    assert same_bits(host(sheet), want)
    assert torch.equal(gw.sweep_figure(make(), size=SIZE), sheet)


def test_segmentation_figure_is_the_restatement_on_what_assign_many_returns(ae_model):
    B, N = 3, 64
    clouds = batch_of(B, N, 10)['cloud']
    clouds[1, 0, 3] = float('nan')                                                    # an invalid point: label -1, and not drawn
    res = ae_model.assign_many(clouds)
    parts = torch.randint(-1, 4, (B, N), generator=torch.Generator().manual_seed(2)).to(DEV)
    sheet = gw.segmentation_figure(clouds, res['labels'], parts, size=SIZE)
    H, W = SIZE
    views = gw.fit_views(clouds, size=SIZE)
    rgb = np.full((3, B * H, 2 * W), 255, np.uint8)
    for col, lab in enumerate((res['labels'], parts)):
        rgb = rr.render(host(clouds), host(lab), gw.PALETTE, host(views), H, W, radius_q=24, near=-1.0, inv_range=0.5, fog=96, cols=2, cell0=col,
                        cell_step=2, invalid_rgb=render.INVALID_RGB, rgb=rgb)['rgb']
    assert same_bits(host(sheet), rgb)
    shifted = gw.segmentation_figure(clouds, (res['labels'] + 1).to(torch.uint8), size=SIZE)          # segment_clouds' convention
    assert torch.equal(shifted, sheet[:, :, :W])


def test_svr_reconstruction_figure_has_the_image_column():
    D = golden('g21_svr')
    cfg = dict(json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg'], util_mode='reconstruction')
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    m = m.to(DEV).eval()
    B, n = 2, 64
    images = dev(np.asarray(synth_images(B, 64, 64, 2123), np.float32))
    batch = dict(batch_of(B, 96, 11), image=images)
    sheet = gw.reconstruction_figure(m, batch, n, state=gw.make_state(6, DEV, 2), size=SIZE)
    assert sheet.shape == (3, B * 32, 3 * 32) and sheet.dtype == torch.uint8
    recon, labels = m.reconstruct_many(images, n, return_labels=True, state=gw.make_state(6, DEV, 2))
    views = gw.fit_views(batch['eval_cloud'], size=SIZE)
    want = figure_ref((B, 3), [(batch['eval_cloud'], None, 0, ONE), (recon, labels.to(torch.int32), 1, gw.PALETTE), None], views)
    # column 2: channels 1:4 of the image, every second pixel of 64 (nearest), clipped to [0, 1] and scaled to bytes
    img = np.rint(np.clip(host(images)[:, 1:4, ::2, ::2], 0, 1) * np.float32(255)).astype(np.uint8)
    for b in range(B):
        want[:, b * 32:(b + 1) * 32, 64:96] = img[b]
    assert same_bits(host(sheet), want)
    assert len(np.unique(want[:, :, 64:96])) > 2                                       # the image column is a picture, not a flat fill
    assert torch.equal(gw.reconstruction_figure(m, batch, n, state=gw.make_state(6, DEV, 2), size=SIZE), sheet)
    with pytest.raises(gw.GwtfError):
        gw.reconstruction_figure(m, batch_of(B, 96, 11), n, size=SIZE)                 # no image
