"""Host side of the device image transform (go_with_the_flows_amd/images.py, csrc/gwtf_images.hip): the numpy restatement the GPU
tests compare against (images_ref.py) against the genuine reference's classes (fixture g23_images), the Resize rule against an
independent implementation, the configuration checks, the loader's plan, the ABI addition and the store's argument checks.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import clouds_ref as cr
import images_ref as ir
from images_ref import RESIZE_BAR, SVR_CFG, bits, case, resize_bound
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, images

@pytest.fixture(scope='module')
def fx():
    return golden('g23_images')


def test_fixture_holds_the_configurations_the_tests_rely_on(fx):
    names = [str(n) for n in fx['names']]
    assert names == ['tonumpy', 'tonumpy4', 'pad', 'gray', 'gray_norm', 'gray_norm_alpha', 'resize_up', 'resize_down', 'svr', 'noise',
                     'noise5']
    assert fx['images_a'].shape == (3, 3, 9, 7) and fx['images_b'].shape == (2, 4, 6, 6) and fx['images_a'].dtype == np.uint8
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g23_images.npz')) < 65536
    svr = case(fx, 'svr')[1]
    assert {k: v for k, v in svr.items() if k != 'image_size'} == {k: v for k, v in SVR_CFG.items() if k in svr and k != 'image_size'}


def test_restatement_against_the_reference(fx):
    for name in fx['names']:
        src, cfg, noise, want = case(fx, name)
        got = ir.transform(src, cfg, noise)
        assert got.shape == want.shape and got.dtype == np.float32, name
        if cfg.get('image_resize'):
            err = np.abs(got.astype(np.float64) - want)
            bound = resize_bound(cfg, got.shape[1])
            print(f'IMAGES {name}: max err {err.max():.3e}, min slack {(bound - err).min():.3e}')
            assert np.all(err <= bound), (name, float(err.max()))
        else:
            assert np.array_equal(bits(got), bits(want)), name
    noise, out = case(fx, 'noise')[2:]
    assert noise.shape == (3, 3, 9, 7) and out.min() == 0.0 and out.max() == 1.0          # both ends of the clip are reached
    assert case(fx, 'noise5')[2].shape == (2, 5, 6, 6)                                    # drawn before RemoveAlpha


def test_to_numpy_is_the_float32_division_for_every_byte():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(bits(np.float32(k / 255.)), bits(k.astype(np.float32) / np.float32(255)))
    img = np.stack([k.reshape(16, 16), k[::-1].reshape(16, 16), k.reshape(16, 16).T])
    out = ir.to_numpy(img)
    third = k.reshape(16, 16).T.astype(np.float32) / np.float32(255)
    assert np.array_equal(bits(out[0]), bits(third * (k.reshape(16, 16).astype(np.float32) / np.float32(255))))
    assert np.array_equal(bits(out[2]), bits(third))


@pytest.mark.parametrize('src,dst', [((137, 137), (224, 224)), ((9, 7), (10, 12)), ((137, 137), (50, 222))])
def test_resize_against_an_independent_bilinear(src, dst):
    """dst is (height, width).  torch's interpolate applies the same half-pixel rule with float32 coordinates."""
    rng = np.random.RandomState(3)
    img = rng.rand(3, *src).astype(np.float32)
    got = ir.resize(img, (dst[1], dst[0]))
    want = torch.nn.functional.interpolate(torch.from_numpy(img)[None], size=dst, mode='bilinear', align_corners=False)[0].numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'IMAGES resize {src}->{dst}: max err {err:.3e}')
    assert got.shape == (3,) + dst and err <= RESIZE_BAR


def test_resize_tables():
    for n_src, n_dst in ((137, 224), (137, 222), (7, 13), (9, 3), (6, 6), (1, 5), (5, 1)):
        s, f = images.resize_table(n_src, n_dst)
        rs, rf = ir.axis_table(n_src, n_dst)
        assert s.dtype == np.int32 and f.dtype == np.float32
        assert np.array_equal(s, rs) and np.array_equal(bits(f), bits(rf))
        assert s.min() >= 0 and s.max() <= n_src - 1 and f.min() >= 0 and f.max() < 1
        assert np.all(f[s == n_src - 1] == 0)
    s, f = images.resize_table(6, 6)
    assert s.tolist() == list(range(6)) and not f.any()                     # an equal size copies
    s, f = images.resize_table(137, 224)
    assert s[0] == 0 and f[0] == 0 and s[-1] == 136 and f[-1] == 0          # clamped at both borders


def test_from_config():
    t = gw.ImageTransform.from_config(channels=3, **SVR_CFG)
    assert (t.C_stage, t.C_out, t.H_out, t.W_out) == (4, 4, 224, 224)
    assert (t.resize, t.pad, t.add_grayscale, t.normalize, t.noise, t.remove_alpha) == (True, False, True, True, False, True)
    assert t.means[:4] == tuple(float(np.float32(v)) for v in SVR_CFG['image_means'])
    assert t.output_size(137, 137) == (224, 224)
    with pytest.raises(ValueError, match='image_means holds 4 values, but NormalizeImages sees 5 channels'):
        gw.ImageTransform.from_config(channels=4, **SVR_CFG)
    with pytest.raises(ValueError, match='image_pad_size'):
        gw.ImageTransform.from_config(channels=3, image_pad=True, image_pad_size=[0, 0])
    with pytest.raises(ValueError, match='image_pad_size'):
        gw.ImageTransform.from_config(channels=3, image_pad=True, image_pad_size=[2, 0])
    for c in (1, 2, 5):
        with pytest.raises(ValueError, match='channels must be 3 or 4'):
            gw.ImageTransform.from_config(channels=c)
    with pytest.raises(ValueError, match='image_stds holds 3 values'):
        gw.ImageTransform.from_config(channels=3, image_add_grayscale=True, image_normalize=True, image_means=[0.1], image_stds=[1, 1, 1])
    # image_size is (width, height), cv2's order
    t = gw.ImageTransform.from_config(channels=4, image_resize=True, image_size=[12, 10], image_pad=True, image_pad_size=[2, 1])
    assert (t.H_out, t.W_out, t.C_out) == (10 + 4, 12 + 2, 4) and t.resized_size(9, 7) == (10, 12)
    one = gw.ImageTransform.from_config(channels=4, image_add_grayscale=True, image_normalize=True, image_means=[0.5], image_stds=[2.0])
    assert one.C_out == 5 and one.means == (0.5,) * 5 and one.stds == (2.0,) * 5 and one.H_out is None
    assert one.output_size(6, 8) == (6, 8)
    with pytest.raises(ValueError, match='image_noise_scale'):
        gw.ImageTransform.from_config(channels=3, image_noise=True, image_noise_scale=0.0)
    none = gw.ImageTransform.from_config(channels=3)
    assert not (none.resize or none.pad or none.add_grayscale or none.normalize or none.noise or none.remove_alpha) and none.C_out == 3


def _stores(n_shapes, views):
    v, f = cr.random_mesh(4, 6, 1)
    meshes = gw.MeshStore.from_arrays(*cr.pack([(v, f)] * n_shapes), device='cpu')
    imgs = gw.ImageStore.from_arrays(np.zeros((n_shapes * views, 3, 2, 2), np.uint8), views_per_shape=views, device='cpu')
    return meshes, imgs


@pytest.mark.parametrize('views', [24, 2])
def test_loader_plan(views):
    meshes, imgs = _stores(5, views)
    n = 5 * views
    ld = gw.DeviceSVRLoader(meshes, imgs, batch_size=4, cloud_size=8, seed=3)
    assert len(imgs) == n and imgs.n_shapes == 5 and len(ld) == n // 4
    assert len(gw.DeviceSVRLoader(meshes, imgs, batch_size=4, cloud_size=8, drop_last=False)) == -(-n // 4)
    plan = ld.index_plan(0)
    assert sorted(plan.tolist()) == list(range(n)) and plan.tolist() != ld.index_plan(1).tolist()
    # item i: shape i // views, image i (datasets.py:180-181)
    assert gw.DeviceSVRLoader(meshes, imgs, 4, 8, shuffle=False).index_plan().tolist() == list(range(n))
    assert (plan // views).max() == 4 and np.array_equal(np.bincount(plan // views), np.full(5, views))
    # the plan rule is DeviceCloudLoader's on the same length, rank by rank
    v, f = cr.random_mesh(4, 6, 1)
    same_len = gw.MeshStore.from_arrays(*cr.pack([(v, f)] * n), device='cpu')
    for world in (1, 3):
        for rank in range(world):
            kw = dict(seed=11, rank=rank, world_size=world)
            mine = gw.DeviceSVRLoader(meshes, imgs, 4, 8, **kw)
            theirs = gw.DeviceCloudLoader(same_len, 4, 8, **kw)
            for epoch in (0, 2):
                assert mine.index_plan(epoch).tolist() == theirs.index_plan(epoch).tolist()
            assert len(mine) == len(theirs)
    with pytest.raises(ValueError, match='shapes'):
        gw.DeviceSVRLoader(_stores(4, views)[0], imgs, 4, 8)


class _Dataset:
    """Slices like an h5py dataset and records what was read."""

    def __init__(self, array):
        self.array, self.reads = array, []

    def __getitem__(self, key):
        self.reads.append(key)
        return self.array[key]


@pytest.mark.parametrize('views', [24, 2])
def test_chosen_label_keeps_whole_view_blocks(views):
    """What ImageStore.from_h5 executes (images.read_views) on arrays standing in for the h5 datasets: the kept shapes are
    MeshStore.from_h5's, in its order, and item i of the result is the image ShapeNetAllDataset.__getitem__ reads for item i."""
    labels = np.array([3, 7, 3, 0, 7, 7, 1], np.uint8)
    n = len(labels) * views
    pixels = np.arange(n, dtype=np.uint8)[:, None, None, None] + np.zeros((1, 3, 2, 2), np.uint8)        # image k holds k everywhere
    for chosen in (7, 3, 1):
        ds = _Dataset(pixels)
        got = images.read_views(ds, labels, chosen, views)
        inds = (np.array(labels, dtype=np.uint8) == chosen).nonzero()[0]          # datasets.py:159, clouds.MeshStore.from_h5
        assert got.shape == (views * len(inds), 3, 2, 2) and got.dtype == np.uint8
        assert got[:, 0, 0, 0].tolist() == [views * inds[i // views] + i % views for i in range(views * len(inds))]
        assert len(ds.reads) == len(inds)                                         # one block per kept shape, nothing else
        store = gw.ImageStore.from_arrays(got, views_per_shape=views, device='cpu')
        assert store.n_shapes == len(inds)
    ds = _Dataset(pixels)
    everything = images.read_views(ds, None, None, views)                         # no label: the whole part, labels never touched
    assert np.array_equal(everything, pixels)
    with pytest.raises(gw.GwtfError, match='no shape carries label 9'):
        images.read_views(_Dataset(pixels), labels, 9, views)


def test_abi_addition_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, 'include', 'gwtf.h')).read()
    declared = set(re.findall(r'\b(gwtf_[a-z0-9_]+)\s*\(', header))
    assert 'gwtf_transform_images' in declared and 'gwtf_transform_images' in _lib.EXPORTS
    assert _lib.ABI_VERSION == 12 and '#define GWTF_ABI_VERSION 12' in header
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct GwtfImageArgs \{(.*?)\} GwtfImageArgs;', header, re.S).group(1), flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        names += [re.search(r'(\w+)\s*(?:\[\d+\])?$', piece.strip()).group(1) for piece in decl.split(',')]
    assert names == [n for n, _ in _lib.ImageArgs._fields_] and len(names) == 28
    L = _lib.lib()
    assert L.gwtf_abi_version() == 12
    assert L.gwtf_transform_images(None) == 10001
    fake = 0x1000                                     # never dereferenced: every check below fails before anything is launched
    ok = dict(images=fake, out=fake, B=2, n_images=4, C=3, H=9, W=7, H_r=9, W_r=7)

    def call(**kw):
        record = _lib.ImageArgs(**dict(ok, **kw))     # named: it must outlive the call
        return L.gwtf_transform_images(ctypes.addressof(record))
    assert call(images=None) == 10001 and call(out=None) == 10001
    assert call(B=0) == 10001 and call(B=65536) == 10001 and call(n_images=0) == 10001
    assert call(C=2) == 10001 and call(C=5) == 10001 and call(H=0) == 10001 and call(W=0) == 10001
    assert call(H_r=10) == 10001 and call(W_r=8) == 10001                      # another size without resize
    assert call(resize=1) == 10001 and call(resize=1, xs=fake, xf=fake, ys=fake) == 10001      # tables given in part
    assert call(pad_y=-1) == 10001 and call(pad_x=-1) == 10001
    assert call(normalize=1) == 10001                                          # stdev 0
    assert call(add_noise=1) == 10001 and call(add_noise=1, state=fake) == 10001               # no state; no scale
    assert call(W=5000, W_r=5000) == 10002                                     # source rows beyond the staging buffer


def test_store_refuses_what_it_cannot_hold():
    good = np.zeros((48, 4, 3, 5), np.uint8)
    st = gw.ImageStore.from_arrays(good, device='cpu')
    assert (len(st), st.n_shapes, st.channels, st.height, st.width, st.views_per_shape) == (48, 2, 4, 3, 5, 24)
    assert gw.ImageStore.from_arrays(torch.from_numpy(good), views_per_shape=16, device='cpu').n_shapes == 3
    with pytest.raises(gw.GwtfError, match='uint8'):
        gw.ImageStore.from_arrays(good.astype(np.float32), device='cpu')
    with pytest.raises(gw.GwtfError, match='n_images, C, H, W'):
        gw.ImageStore.from_arrays(good[0], device='cpu')
    with pytest.raises(gw.GwtfError, match='n_images, C, H, W'):
        gw.ImageStore.from_arrays(np.zeros((48, 2, 3, 5), np.uint8), device='cpu')
    with pytest.raises(gw.GwtfError, match='no multiple of views_per_shape'):
        gw.ImageStore.from_arrays(good[:47], device='cpu')
    with pytest.raises(TypeError):
        gw.ImageStore()
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(gw.GwtfError, match='needs h5py'):
            gw.ImageStore.from_h5('/nonexistent.h5', 'train')
    t = gw.ImageTransform(channels=3)
    with pytest.raises(gw.GwtfError, match='4'):
        gw.transform_images(st, torch.zeros(2, dtype=torch.int32), t)           # a 3-channel transformation on a 4-channel store
    with pytest.raises(gw.GwtfError, match='int32'):
        gw.transform_images(st, torch.zeros(2, dtype=torch.int64), gw.ImageTransform(channels=4))
