"""The device image transform (csrc/gwtf_images.hip, go_with_the_flows_amd/images.py) on the GPU: against the genuine reference's
classes (fixture g23_images, explicit noise), bit for bit against the numpy restatement (images_ref.py) on the shapes where the
kernel can go wrong, its Philox noise, graph capture, the pinned-host store, the loader and one graphed SVR training step."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
import images_ref as ir
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import models, optim
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_
from go_with_the_flows_amd.training import GraphedTrainStep
from images_ref import SVR_CFG, bits, case, resize_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def fx():
    return golden('g23_images')


def _rows(r):
    return torch.tensor(list(r), dtype=torch.int32, device=DEV)


def _run(src, cfg, rows=None, noise=None, **kw):
    store = gw.ImageStore.from_arrays(src, views_per_shape=1, device=DEV)
    t = gw.ImageTransform.from_config(channels=src.shape[1], **cfg)
    rows = _rows(range(len(src)) if rows is None else rows)
    return gw.transform_images(store, rows, t, explicit=None if noise is None else torch.from_numpy(noise).to(DEV), **kw).cpu().numpy()


# ---- 1. the fixture: the reference's classes, and the restatement's bits -------------------------------------------------------
def test_every_fixture_configuration(fx):
    for name in fx['names']:
        src, cfg, noise, want = case(fx, name)
        got = _run(src, cfg, noise=noise)
        assert got.shape == want.shape, name
        assert np.array_equal(bits(got), bits(ir.transform(src, cfg, noise))), name
        if cfg.get('image_resize'):
            err = np.abs(got.astype(np.float64) - want)
            print(f'IMAGES gpu {name}: max err {err.max():.3e}')
            assert np.all(err <= resize_bound(cfg, got.shape[1])), (name, float(err.max()))
        else:
            assert np.array_equal(bits(got), bits(want)), name


# ---- 2. shapes where the kernel can go wrong ------------------------------------------------------------------------------------
NORM4 = dict(image_normalize=True, image_means=SVR_CFG['image_means'], image_stds=SVR_CFG['image_stds'])
NORM5 = dict(image_normalize=True, image_means=[0.05, 0.04, 0.03, 0.02, 0.5], image_stds=[0.2, 0.11, 0.12, 0.13, 0.4])
SHAPES = {
    'b1_7_to_13': ((1, 3, 5, 7), dict(image_resize=True, image_size=[13, 6])),
    'b3_137_to_222': ((3, 3, 137, 137), dict(image_resize=True, image_size=[222, 10], image_add_grayscale=True, **NORM4)),
    'full_size_pair': ((2, 3, 137, 137), {k: v for k, v in SVR_CFG.items() if k.startswith('image_')}),
    'pad_after_resize': ((3, 3, 9, 7), dict(image_resize=True, image_size=[13, 6], image_pad=True, image_pad_size=[2, 1],
                                            image_add_grayscale=True, **NORM4)),
    'pad_rows_over_tiles': ((2, 3, 9, 7), dict(image_pad=True, image_pad_size=[3, 2])),
    'alpha_kept_5_channels': ((3, 4, 6, 7), dict(image_add_grayscale=True, **NORM5)),
    'alpha_kept_resized': ((1, 4, 6, 7), dict(image_resize=True, image_size=[10, 9])),
    'alpha_dropped_down': ((2, 4, 20, 30), dict(image_resize=True, image_size=[8, 5], image_add_grayscale=True,
                                                image_remove_alpha=True)),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_shapes_equal_the_restatement_bit_for_bit(name):
    shape, cfg = SHAPES[name]
    src = np.random.RandomState(len(name)).randint(0, 256, shape).astype(np.uint8)
    got = _run(src, cfg)
    want = ir.transform(src, cfg)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    if name == 'full_size_pair':
        assert got.shape == (2, 4, 224, 224)
        rev = _run(src, cfg, rows=[1, 0, 1])                                    # rows select the source image
        assert np.array_equal(bits(rev), bits(want[[1, 0, 1]]))


def test_rows_are_checked_and_a_row_outside_the_store_gives_nan(fx):
    src, cfg = case(fx, 'svr')[:2]
    store = gw.ImageStore.from_arrays(src, views_per_shape=3, device=DEV)
    t = gw.ImageTransform.from_config(channels=3, **cfg)
    with pytest.raises(gw.GwtfError, match='contiguous'):
        gw.transform_images(store, _rows([0, 9, 1, 9])[::2], t)
    with pytest.raises(gw.GwtfError, match='int32'):
        gw.transform_images(store, _rows([0, 1]).long(), t)
    with pytest.raises(gw.GwtfError, match='expected'):
        gw.transform_images(store, _rows([0, 1]), t, out=torch.empty(2, 4, 16, 15, device=DEV))
    want = ir.transform(src, cfg)
    got = gw.transform_images(store, _rows([2, -1, 0, 3, 1]), t).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    assert np.array_equal(bits(got[[0, 2, 4]]), bits(want[[2, 0, 1]]))


# ---- 3. Philox noise ---------------------------------------------------------------------------------------------------------------
def _grey_store(n, C, H, W):
    """Images of zero bytes: every channel is 0 after ToNumpy, so mean -0.5 / std 1 puts every value at 0.5 before the noise."""
    return gw.ImageStore.from_arrays(np.zeros((n, C, H, W), np.uint8), views_per_shape=1, device=DEV)


def test_philox_noise_equals_the_restatement_and_advances_the_call():
    """Bar 1e-4 on scale-1 normals (float32 log / sqrt / cos / sin differ by a few ulp of |z| < 6 between the device and numpy, the
    bar of test_gpu_clouds.py); the clip is 1-Lipschitz, so it holds after clipping too, and 0.5 + z stays inside (0, 1) for 38 % of
    the draws.  Five stage channels: the fifth comes from the second Philox stream."""
    B, C, H, W = 3, 4, 9, 7
    store = _grey_store(B, C, H, W)
    t = gw.ImageTransform(channels=C, add_grayscale=True, normalize=True, means=[-0.5], stds=[1.0], noise=True, noise_scale=1.0)
    seed, call = 0x1234567890abcdef, (5 << 32) + 17
    state = gw.make_state(seed, DEV, call)
    outs = [gw.transform_images(store, _rows(range(B)), t, state).cpu().numpy() for _ in range(2)]
    assert state.cpu().tolist() == [seed, call + 2]
    for k, got in enumerate(outs):
        z = ir.philox_noise(seed, call + k, B, 5, H, W, 1.0)
        want = np.minimum(np.maximum(np.float32(0.5) + z, np.float32(0)), np.float32(1))
        inside = (want > 0) & (want < 1)
        err = np.abs(got - want).max()
        print(f'IMAGES philox call {k}: max err {err:.3e}, unclipped {inside.mean():.2f}')
        assert got.shape == (B, 5, H, W) and err < 1e-4 and inside.mean() > 0.3
    assert not np.array_equal(outs[0], outs[1])
    # without noise the state is neither needed nor touched
    quiet = gw.ImageTransform(channels=C, add_grayscale=True)
    gw.transform_images(store, _rows(range(B)), quiet, state)
    assert state.cpu().tolist() == [seed, call + 2]


def test_noise_moments():
    B, C, H, W = 4, 4, 72, 72
    t = gw.ImageTransform(channels=C, add_grayscale=True, normalize=True, means=[-0.5], stds=[1.0], noise=True, noise_scale=0.0625)
    out = gw.transform_images(_grey_store(B, C, H, W), _rows(range(B)), t, gw.make_state(2024, DEV)).cpu().numpy()
    z = ((out.astype(np.float64) - 0.5) * 16).ravel()                           # 0.5 + z / 16 leaves [0, 1] beyond 8 sigma only
    n = z.size
    assert n == 4 * 5 * 72 * 72
    print(f'IMAGES noise mean {z.mean():.4e} (bar {5 / np.sqrt(n):.4e}) var-1 {z.var() - 1:.4e} (bar {5 * np.sqrt(2 / n):.4e})')
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    per_channel = z.reshape(B, 5, -1)
    assert all(abs(np.corrcoef(per_channel[:, a].ravel(), per_channel[:, b].ravel())[0, 1]) < 5 / np.sqrt(n / 5)
               for a in range(5) for b in range(a + 1, 5))


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------------
def test_a_captured_call_draws_fresh_noise_and_is_deterministic_without(fx):
    src = np.random.RandomState(4).randint(0, 256, (5, 3, 9, 7)).astype(np.uint8)
    store = gw.ImageStore.from_arrays(src, views_per_shape=1, device=DEV)
    rows = _rows([4, 0, 2])
    base = dict(image_resize=True, image_size=[13, 10], image_add_grayscale=True)
    for noisy in (True, False):
        t = gw.ImageTransform.from_config(channels=3, image_noise=noisy, image_noise_scale=0.2, **base)
        state = gw.make_state(7, DEV, 40)
        buf = torch.empty(3, 4, 10, 13, device=DEV)
        gw.transform_images(store, rows, t, state, out=buf)                    # warm-up: the tables of this size exist from here on
        state.copy_(gw.make_state(7, DEV, 40))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = gw.transform_images(store, rows, t, state, out=buf)
        assert res is buf
        replays = []
        for _ in range(2):
            graph.replay()
            replays.append(buf.clone())
        torch.cuda.synchronize()
        eager_state = gw.make_state(7, DEV, 40)
        for rep in replays:
            assert torch.equal(gw.transform_images(store, rows, t, eager_state), rep)
        if noisy:
            assert state.cpu().tolist() == [7, 42] and not torch.equal(replays[0], replays[1])
        else:
            assert state.cpu().tolist() == [7, 40] and torch.equal(replays[0], replays[1])


# ---- 5. a store in pinned host memory ----------------------------------------------------------------------------------------------
def test_a_pinned_host_store_gives_the_device_store_bits():
    src = np.random.RandomState(5).randint(0, 256, (12, 4, 11, 9)).astype(np.uint8)
    on_device = gw.ImageStore.from_arrays(src, views_per_shape=2, device=DEV)
    on_host = gw.ImageStore.from_arrays(src, views_per_shape=2, device='cpu', compute_device=DEV)
    assert on_host.images.is_pinned() and not on_host.images.is_cuda
    t = gw.ImageTransform.from_config(channels=4, image_resize=True, image_size=[14, 12], image_add_grayscale=True)
    outs = []
    for batch in ([3, 11, 0, 7], [1, 1, 10, 2], [9, 8, 5, 4]):                  # three batches: both staging buffers, one of them twice
        rows = torch.tensor(batch, dtype=torch.int32)
        got = gw.transform_images(on_host, rows, t)
        assert got.is_cuda
        outs.append((got, gw.transform_images(on_device, rows.to(DEV), t)))
    for got, want in outs:
        assert torch.equal(got, want)
    with pytest.raises(gw.GwtfError, match='rows must lie in'):
        gw.transform_images(on_host, torch.tensor([0, 12], dtype=torch.int32), t)
    # one pair of staging buffers, as large as the largest batch: a smaller batch uses it, a larger one replaces it
    first = on_host._staging['slots']
    small = torch.tensor([6, 2], dtype=torch.int32)
    assert torch.equal(gw.transform_images(on_host, small, t), gw.transform_images(on_device, small.to(DEV), t))
    assert on_host._staging['slots'] is first and on_host._staging['capacity'] == 4
    side = torch.cuda.Stream(device=DEV)                                       # another stream: the event follows the launch
    side.wait_stream(torch.cuda.current_stream(DEV))
    large = torch.tensor([0, 5, 7, 7, 11, 3], dtype=torch.int32)
    with torch.cuda.stream(side):
        got = [gw.transform_images(on_host, large, t) for _ in range(3)]
    torch.cuda.current_stream(DEV).wait_stream(side)
    want = gw.transform_images(on_device, large.to(DEV), t)
    assert on_host._staging['capacity'] == 6 and all(torch.equal(g, want) for g in got)


def test_store_takes_device_tensors_and_explicit_noise_needs_a_noisy_transformation():
    src = torch.from_numpy(np.random.RandomState(8).randint(0, 256, (4, 3, 5, 6)).astype(np.uint8))
    a = gw.ImageStore.from_arrays(src.to(DEV), views_per_shape=2, device=DEV)
    b = gw.ImageStore.from_arrays(src.numpy(), views_per_shape=2, device=DEV)
    t = gw.ImageTransform(channels=3, add_grayscale=True)
    assert torch.equal(gw.transform_images(a, _rows(range(4)), t), gw.transform_images(b, _rows(range(4)), t))
    with pytest.raises(gw.GwtfError, match='uint8'):
        gw.ImageStore.from_arrays(src.to(DEV).float(), device=DEV)
    with pytest.raises(gw.GwtfError, match='adds none'):
        gw.transform_images(a, _rows(range(4)), t, explicit=torch.zeros(4, 4, 5, 6, device=DEV))


# ---- 6. the loader -----------------------------------------------------------------------------------------------------------------
def _svr_stores(views, image_shape, seed):
    D = golden('g22_clouds')
    meshes = gw.MeshStore.from_arrays(D['vertices_c'], D['faces_vc'], D['vertices_c_bounds'], D['faces_bounds'], D['orig_c'], D['orig_s'],
                                      device=DEV)
    src = np.random.RandomState(seed).randint(0, 256, (3 * views,) + image_shape).astype(np.uint8)
    return meshes, gw.ImageStore.from_arrays(src, views_per_shape=views, device=DEV), src


def test_loader_on_the_device():
    views, B, N = 2, 4, 50
    meshes, imgs, src = _svr_stores(views, (3, 9, 7), 6)
    ct = gw.CloudTransform(center=True)
    it = gw.ImageTransform.from_config(channels=3, image_resize=True, image_size=[12, 10], image_add_grayscale=True, image_noise=True,
                                       image_noise_scale=0.1)
    loader = gw.DeviceSVRLoader(meshes, imgs, B, N, ct, it, seed=5, drop_last=False)
    loader.set_epoch(1)
    batches = [{k: v.clone() for k, v in b.items()} for b in loader]
    plan = loader.index_plan()
    assert len(batches) == len(loader) == 2 and len(plan) == 6
    cloud_state, image_state = gw.make_state(5, DEV), gw.make_state(5, DEV)
    for i, b in enumerate(batches):
        items = plan[B * i:B * (i + 1)]
        n = len(items)
        assert set(b) == {'cloud', 'eval_cloud', 'image', 'orig_c', 'orig_s'}
        assert b['cloud'].shape == (n, 3, N) and b['eval_cloud'].shape == (n, 3, N) and b['image'].shape == (n, 4, 10, 12)
        assert b['image'].is_cuda and b['image'].dtype == torch.float32
        want_image = gw.transform_images(imgs, _rows(items), it, image_state)
        want_cloud = gw.sample_clouds(meshes, _rows(items // views), N, True, ct, cloud_state)
        assert torch.equal(b['image'], want_image)
        assert torch.equal(b['cloud'], want_cloud['cloud']) and torch.equal(b['eval_cloud'], want_cloud['eval_cloud'])
        assert torch.equal(b['orig_s'], want_cloud['orig_s'])


# ---- 7. one loader batch through the graphed SVR step -------------------------------------------------------------------------------
def test_a_loader_batch_trains_the_graphed_svr_step():
    """The four loss terms of GraphedTrainStep on the loader's batch against the same step, on the same model state, given the same
    tensors produced by hand (transform_images / sample_clouds from the loader's states).  Two evaluations sum their batch statistics
    with float atomics in different orders: the 1e-4 relative bar of test_gpu_svr_fused.py for equal steps."""
    D = golden('g21_svr')
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']
    views, B, N = 2, 4, 48
    meshes, imgs, _ = _svr_stores(views, (3, 20, 20), 7)
    it = gw.ImageTransform.from_config(channels=3, **dict(SVR_CFG, image_size=[64, 64]))
    loader = gw.DeviceSVRLoader(meshes, imgs, B, N, gw.CloudTransform(center=True), it, seed=9)
    batch = next(iter(loader))
    assert batch['image'].shape == (B, 4, 64, 64)
    items = loader.index_plan()[:B]
    by_hand = gw.sample_clouds(meshes, _rows(items // views), N, True, loader.cloud_transform, gw.make_state(9, DEV))
    by_hand['image'] = gw.transform_images(imgs, _rows(items), it)
    noise = torch.from_numpy(D['noise_g']).float().to(DEV)
    m = models.Flow_Mixture_SVR_Model(**cfg)
    load_synth_(m, 2110)
    load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
    m = m.to(DEV).train()
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    crit = models.Flow_Mixture_Loss(**cfg)
    step = GraphedTrainStep(m, crit, optim.Adam(m.parameters(), lr=1e-4), batch['cloud'], batch['eval_cloud'],
                            images_example=batch['image'])
    state = {k: v.clone() for k, v in m.state_dict().items()}
    terms = []
    for b in (batch, by_hand):
        m.load_state_dict(state)                  # the same model both times
        terms.append([float(v) for v in step(b['cloud'], b['eval_cloud'], b['image'])])
    print('IMAGES step terms', terms)
    assert len(terms[0]) == 4 and all(np.isfinite(v) for v in terms[0])
    for a, b in zip(*terms):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a))
