"""Single-view-reconstruction batches on the device (csrc/gwtf_images.hip): the image side of the reference's
ShapeNetAllDataset.__getitem__ (lib/datasets/datasets.py:173-222) and its composed image transformations
(lib/datasets/image_transformations.py:7-95) for a whole batch in one launch, from raw uint8 renderings that stay resident.

    meshes = MeshStore.from_h5('.../ShapeNetAll13_meshes.h5', 'train')
    images = ImageStore.from_h5('.../ShapeNetAll13_images.h5', 'train')                  # (24 * n_shapes, C, 137, 137) uint8
    loader = DeviceSVRLoader(meshes, images, 128, 2048, CloudTransform.from_config(**config),
                             ImageTransform.from_config(channels=3, **config))
    for batch in loader:              # {'cloud', 'eval_cloud': (B,3,N), 'image': (B,4,224,224)[, 'orig_c', 'orig_s']} on the device
        step(batch['cloud'], batch['eval_cloud'], batch['image'])                         # GraphedTrainStep(..., images_example=)

The stage order is the reference's: ToNumpy, Resize, Pad, AddGrayscale, NormalizeImages, AddNoise2Images, RemoveAlpha; the arithmetic
of every stage is stated in include/gwtf.h (GwtfImageArgs) and restated in numpy in tests/images_ref.py.  There is no CPU transform:
a store kept in (pinned) host memory stages each batch's raw bytes to the device and runs the same launch.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GwtfError
from .clouds import epoch_plan, make_state, sample_clouds

GRAY_WEIGHTS = (0.299, 0.587, 0.114)            # AddGrayscale (image_transformations.py:41-43)
HOST_STORE_IN_CAPTURE = 'a host-resident ImageStore copies every batch from the host and cannot be captured; keep the store on the device'


def resize_table(n_src, n_dst):
    """(s int32, f float32), each (n_dst,): the taps of cv2.resize's INTER_LINEAR along one axis.  Destination index d reads source
    s[d] and min(s[d] + 1, n_src - 1) with weights 1.f - f[d] and f[d].  The coordinate is formed in float64 and rounded to float32
    once, as cv2 does on the host: f = (float)((d + 0.5) * (n_src / n_dst) - 0.5), s = floor(f), f -= s."""
    n_src, n_dst = int(n_src), int(n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * (n_src / n_dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= n_src - 1
    s[low], f[low] = 0, 0.0
    s[high], f[high] = n_src - 1, 0.0
    return s.astype(np.int32), f


def read_views(images_ds, labels=None, chosen_label=None, views_per_shape=24):
    """The images of one part as one host array, as ImageStore.from_h5 reads them.  images_ds: the `<part>_images` dataset (anything
    that slices like one, a numpy array included), views_per_shape consecutive images per shape; labels: `<part>_labels`, one per
    shape.  chosen_label keeps the shapes keep = (labels == chosen_label).nonzero()[0] -- MeshStore.from_h5's selection, in its
    order -- and of each its whole block of views: item i of the result is image views * keep[i // views] + i % views, what
    ShapeNetAllDataset.__getitem__ reads for item i of the restricted dataset (datasets.py:176-178)."""
    if chosen_label is None:
        return np.asarray(images_ds[:])
    v = int(views_per_shape)
    keep = (np.array(labels, dtype=np.uint8) == chosen_label).nonzero()[0]
    if len(keep) == 0:
        raise GwtfError(f'no shape carries label {chosen_label}')
    return np.concatenate([np.asarray(images_ds[v * k:v * (k + 1)]) for k in keep])


class ImageStore:
    """The raw uint8 renderings of one part of images.h5 (preprocess_ShapeNetAll.py:65), views_per_shape consecutive images per
    shape, on a HIP device or in pinned host memory."""

    def __init__(self):
        raise TypeError('use ImageStore.from_arrays / ImageStore.from_h5')

    @classmethod
    def from_arrays(cls, images_uint8, views_per_shape=24, device='cuda', compute_device=None):
        """images_uint8: (n_images, C, H, W) uint8 (numpy, or a tensor on any device), C in {3, 4}, n_images a multiple of
        views_per_shape.  device='cpu' keeps the
        images on the host (pinned where a device exists); batches then run on compute_device (default: the current HIP device)."""
        self = object.__new__(cls)
        images = images_uint8.detach() if isinstance(images_uint8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images_uint8))
        if images.dtype != torch.uint8:
            raise GwtfError(f'images must be uint8 (got {images.dtype}): the store keeps the raw renderings')
        if images.dim() != 4 or images.shape[1] not in (3, 4) or min(images.shape) < 1:
            raise GwtfError(f'images must be (n_images, C, H, W) with C in {{3, 4}} (got {tuple(images.shape)})')
        views_per_shape = int(views_per_shape)
        if views_per_shape < 1 or images.shape[0] % views_per_shape:
            raise GwtfError(f'{images.shape[0]} images are no multiple of views_per_shape = {views_per_shape}')
        if images.shape[0] >= 2**31 or images.shape[2] * images.shape[3] >= 2**31:
            raise GwtfError('too many images, or images too large, for 32-bit indices')
        self.n_images, self.channels, self.height, self.width = (int(v) for v in images.shape)
        self.views_per_shape, self.n_shapes = views_per_shape, self.n_images // views_per_shape
        self.device = torch.device(device)
        if self.device.type == 'cuda':
            self.images = images.to(self.device).contiguous()
            self.device = self.compute_device = self.images.device
        else:
            host = images.cpu().contiguous()
            self.images = host.pin_memory() if torch.cuda.is_available() else host
            self.compute_device = None if compute_device is None else torch.device(compute_device)
        self._staging = None
        self._state = None
        return self

    @classmethod
    def from_h5(cls, path, part='train', chosen_label=None, views_per_shape=24, device='cuda', compute_device=None):
        """The image reads of ShapeNetAllDataset (datasets.py:176-203), once for the whole part; chosen_label keeps the image blocks of
        one class's shapes, in the order MeshStore.from_h5 keeps the shapes (read_views).  The whole part passes through host memory
        once (about 60 GB for the ShapeNetAll13 training part) before it is uploaded or pinned: the host needs that much free."""
        try:
            import h5py
        except ImportError as e:
            raise GwtfError('ImageStore.from_h5 needs h5py, which is not installed; read the datasets yourself and use '
                            'ImageStore.from_arrays') from e
        with h5py.File(path, 'r') as fin:
            labels = None if chosen_label is None else fin[part + '_labels']
            images = read_views(fin[part + '_images'], labels, chosen_label, views_per_shape)
        return cls.from_arrays(images, views_per_shape=views_per_shape, device=device, compute_device=compute_device)

    def __len__(self):
        return self.n_images


def _pair(value, name):
    try:
        a, b = (int(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must hold two integers (got {value!r})') from None
    return a, b


class ImageTransform:
    """The record of image transformations the kernel fuses, in ComposeImageTransformation's order (image_transformations.py:76-95):
    ToNumpy (always), Resize, Pad, AddGrayscale, NormalizeImages, AddNoise2Images, RemoveAlpha -- for sources of `channels` channels.

    C_stage = channels + grayscale is the channel count NormalizeImages and AddNoise2Images see, C_out what RemoveAlpha leaves.
    size is (width, height), cv2's order; pad_size (rows, columns)."""

    def __init__(self, channels=3, resize=False, size=None, pad=False, pad_size=(0, 0), add_grayscale=False, normalize=False,
                 means=None, stds=None, noise=False, noise_scale=None, remove_alpha=False):
        self.channels = int(channels)
        if self.channels not in (3, 4):
            raise ValueError(f'images of {self.channels} channels: ToNumpy scales channels 0 and 1 by channel 2, and the kernel reads '
                             'RGB or RGBA, so channels must be 3 or 4')
        self.resize, self.pad, self.add_grayscale = bool(resize), bool(pad), bool(add_grayscale)
        self.normalize, self.noise, self.remove_alpha = bool(normalize), bool(noise), bool(remove_alpha)
        self.size = None
        if self.resize:
            self.size = _pair(size, 'image_size')
            if min(self.size) < 1:
                raise ValueError(f'image_size must be positive (got {self.size})')
        self.pad_size = (0, 0)
        if self.pad:
            self.pad_size = _pair(pad_size, 'image_pad_size')
            if min(self.pad_size) < 1:
                raise ValueError(f'image_pad with image_pad_size = {list(self.pad_size)}: the reference\'s Pad writes into the slice '
                                 '[p:-p], which is empty for p = 0 (image_transformations.py:35); both sizes must be positive')
        self.C_stage = self.channels + (1 if self.add_grayscale else 0)
        self.C_out = min(self.C_stage, 4) if self.remove_alpha else self.C_stage
        self.means, self.stds = (0.0,) * 5, (1.0,) * 5
        if self.normalize:
            vals = []
            for name, v in (('image_means', means), ('image_stds', stds)):
                v = np.asarray(v, np.float32).reshape(-1)
                if len(v) not in (1, self.C_stage):
                    raise ValueError(
                        f'{name} holds {len(v)} values, but NormalizeImages sees {self.C_stage} channels ({self.channels} source channels'
                        f'{" + grayscale" if self.add_grayscale else ""}): numpy cannot broadcast them; give {self.C_stage} values or 1')
                vals.append(tuple(float(x) for x in (np.repeat(v, self.C_stage) if len(v) == 1 else v)) + (1.0,) * (5 - self.C_stage))
            self.means, self.stds = vals
            if not all(s > 0 for s in self.stds):
                raise ValueError('image_stds must be positive')
        self.noise_scale = 1.0
        if self.noise:
            self.noise_scale = float(np.float32(noise_scale))
            if not self.noise_scale > 0:
                raise ValueError('image_noise_scale must be positive')
        self.H_out = self.W_out = None                     # known here only with resize: (size[1], size[0]) + padding
        if self.resize:
            self.H_out, self.W_out = self.output_size(1, 1)
        self._tables = {}

    @classmethod
    def from_config(cls, channels, **kwargs):
        """From the reference's image_* config keys, for sources of `channels` channels; other keys are ignored."""
        return cls(channels=channels, resize=kwargs.get('image_resize', False), size=kwargs.get('image_size'),
                   pad=kwargs.get('image_pad', False), pad_size=kwargs.get('image_pad_size') or (0, 0),
                   add_grayscale=kwargs.get('image_add_grayscale', False), normalize=kwargs.get('image_normalize', False),
                   means=kwargs.get('image_means'), stds=kwargs.get('image_stds'), noise=kwargs.get('image_noise', False),
                   noise_scale=kwargs.get('image_noise_scale'), remove_alpha=kwargs.get('image_remove_alpha', False))

    def resized_size(self, H, W):
        return (self.size[1], self.size[0]) if self.resize else (int(H), int(W))

    def output_size(self, H, W):
        """(H_out, W_out) for sources of H x W."""
        h, w = self.resized_size(H, W)
        return h + 2 * self.pad_size[0], w + 2 * self.pad_size[1]

    def tables(self, H, W, device):
        """The device copies of the Resize tables (xs, xf, ys, yf) for sources of H x W: computed on the host in float64 and
        uploaded on the first call for a (source size, device), then kept."""
        key = (int(H), int(W), str(device))
        t = self._tables.get(key)
        if t is None:
            h, w = self.resized_size(H, W)
            (xs, xf), (ys, yf) = resize_table(W, w), resize_table(H, h)
            t = self._tables[key] = tuple(torch.from_numpy(a).to(device) for a in (xs, xf, ys, yf))
        return t


def _stage_rows(store, rows, dev):
    """A host store: gather the batch's raw bytes into one of two pinned buffers and enqueue its copy to that buffer's device twin
    -> (device images, event).  The caller records the event BEHIND the launch that reads the device twin; it is waited for, on the
    host, before the pair is written again two batches later, so neither the copy nor a kernel on any stream can still be reading
    it.  The store keeps ONE pair of buffers, as large as the largest batch seen; smaller batches use their leading part."""
    if torch.cuda.is_current_stream_capturing():
        raise GwtfError(HOST_STORE_IN_CAPTURE)
    B = rows.numel()
    if int(rows.min()) < 0 or int(rows.max()) >= store.n_images:
        raise GwtfError(f'rows must lie in [0, {store.n_images}) for a host-resident store')
    ring = store._staging
    if ring is None or ring['capacity'] < B or ring['device'] != dev:
        if ring is not None:
            for _, _, event in ring['slots']:                  # nothing may still read the buffers that go
                event.synchronize()
        shape = (B, store.channels, store.height, store.width)
        ring = store._staging = {'turn': 0, 'capacity': B, 'device': dev, 'slots': [
            (torch.empty(shape, dtype=torch.uint8).pin_memory(), torch.empty(shape, dtype=torch.uint8, device=dev), torch.cuda.Event())
            for _ in range(2)]}
    host, device, event = ring['slots'][ring['turn']]
    ring['turn'] ^= 1
    event.synchronize()                                     # returns at once until the pair has been used
    torch.index_select(store.images, 0, rows.long(), out=host[:B])
    device[:B].copy_(host[:B], non_blocking=True)
    return device[:B], event


def transform_images(store, rows, transform, state=None, explicit=None, out=None):
    """One batch: rows (B,) int32 image indices on the store's device -> (B, C_out, H_out, W_out) float32 on the HIP device.
    Enqueued on the current stream.  With a device store nothing waits for the device, and the call can be captured (after one eager
    call has uploaded the Resize tables of this source size).  With a host store the call gathers the batch on the host, and first
    waits, on the host, until the launch of two batches back has finished with the staging buffers it is about to reuse.

    state: make_state(seed), read and advanced only when the transformation draws noise (default: one the store keeps, seed 0).
    explicit: the already scaled noise, (B, C_stage, H_out, W_out) float32 (or {'noise': that}), replaces Philox; refused when the
    transformation adds no noise.  out: a tensor of the result's shape to write into.  A row outside [0, n_images) of a device
    store gives an all-NaN image; a host store refuses it."""
    t = transform
    if t.channels != store.channels:
        raise GwtfError(f'the transformation was built for {t.channels}-channel images, the store holds {store.channels}')
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != store.device or not rows.is_contiguous():
        raise GwtfError('rows must be a contiguous 1-d int32 tensor on the store\'s device')
    B = rows.numel()
    if B < 1:
        raise GwtfError('rows is empty')
    if store.device.type == 'cuda':
        dev, images, n_images, rows_ptr, staged = store.device, store.images, store.n_images, rows.data_ptr(), None
    else:
        dev = store.compute_device
        if dev is None:
            if not torch.cuda.is_available():
                raise GwtfError('the transformation runs on a HIP device only, there is no CPU path')
            dev = store.compute_device = torch.device('cuda', torch.cuda.current_device())
        images, n_images, rows_ptr, staged = None, B, None, True           # staged below, behind every argument check
    H, W = store.height, store.width
    (Hr, Wr), (Ho, Wo) = t.resized_size(H, W), t.output_size(H, W)
    shape = (B, t.C_out, Ho, Wo)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.device != dev:
        raise GwtfError(f'out is {tuple(out.shape)} on {out.device}, expected {shape} on {dev}')
    out_ptr = _lib._ptr(out, 'out')
    noise_ptr = state_ptr = None
    if explicit is not None and not t.noise:
        raise GwtfError('explicit noise was given, but the transformation adds none (image_noise is off)')
    if t.noise:
        if explicit is not None:
            noise = explicit['noise'] if isinstance(explicit, dict) else explicit
            want = (B, t.C_stage, Ho, Wo)
            if tuple(noise.shape) != want or noise.dtype != torch.float32 or noise.device != dev or not noise.is_contiguous():
                raise GwtfError(f'explicit noise must be a contiguous float32 tensor of shape {want} on {dev}')
            noise_ptr = noise.data_ptr()
        else:
            if state is None:
                if store._state is None:
                    store._state = make_state(0, dev)
                state = store._state
            if state.dtype != torch.int64 or state.numel() != 2 or state.device != dev:
                raise GwtfError('state must come from make_state(seed, device) on the device the batch is produced on')
            state_ptr = state.data_ptr()
    xs = xf = ys = yf = None
    if t.resize:
        xs, xf, ys, yf = (x.data_ptr() for x in t.tables(H, W, dev))
    if staged:
        images, staged = _stage_rows(store, rows, dev)
    a = _lib.ImageArgs(
        images=images.data_ptr(), rows=rows_ptr, xs=xs, xf=xf, ys=ys, yf=yf, noise=noise_ptr, state=state_ptr,
        out=out_ptr, B=B, n_images=n_images, C=store.channels, H=H, W=W, H_r=Hr, W_r=Wr, pad_y=t.pad_size[0],
        pad_x=t.pad_size[1], resize=t.resize, grayscale=t.add_grayscale, normalize=t.normalize, add_noise=t.noise,
        remove_alpha=t.remove_alpha, gray=(ctypes.c_float * 3)(*GRAY_WEIGHTS), mean=(ctypes.c_float * 5)(*t.means),
        stdev=(ctypes.c_float * 5)(*t.stds), noise_scale=t.noise_scale, stream=torch.cuda.current_stream(dev).cuda_stream)
    try:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().gwtf_transform_images(ctypes.addressof(a)))
    finally:
        if staged is not None:                              # behind the copy and the launch that reads the staged bytes
            staged.record(torch.cuda.current_stream(dev))
    return out


class DeviceSVRLoader:
    """Stands where DataLoader(ShapeNetAllDataset(...), batch_size, shuffle=True, drop_last=True) stood (train_svr.py): an iterable
    of device batches {'cloud', 'eval_cloud', 'image'[, 'orig_c', 'orig_s']}.  Item i is view i % views of shape i // views
    (datasets.py:180-181): its cloud is drawn from mesh i // views, its image is image i.  The epoch's order is DeviceCloudLoader's
    (clouds.epoch_plan) over views * n_shapes items; rank and world_size only shape that plan.  Clouds and image noise draw from two
    device states with this rank's seed (the Philox streams of the two kernels differ), each advancing by itself."""

    def __init__(self, mesh_store, image_store, batch_size, cloud_size, cloud_transform=None, image_transform=None, shuffle=True,
                 drop_last=True, seed=0, rank=0, world_size=1, return_eval_cloud=True):
        if not 0 <= rank < world_size:
            raise ValueError('rank must lie in [0, world_size)')
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        if image_store.n_shapes != len(mesh_store):
            raise ValueError(f'{len(image_store)} images in blocks of {image_store.views_per_shape} are {image_store.n_shapes} shapes, '
                             f'the mesh store holds {len(mesh_store)}')
        self.mesh_store, self.image_store = mesh_store, image_store
        self.batch_size, self.cloud_size = int(batch_size), int(cloud_size)
        self.cloud_transform = cloud_transform
        self.image_transform = image_transform if image_transform is not None else ImageTransform(channels=image_store.channels)
        self.shuffle, self.drop_last, self.seed, self.rank, self.world_size = bool(shuffle), bool(drop_last), int(seed), rank, world_size
        self.return_eval_cloud = bool(return_eval_cloud)
        self.views = image_store.views_per_shape
        self.epoch = 0
        self.num_samples = -(-len(image_store) // world_size)
        self._state = self._image_state = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.num_samples // self.batch_size if self.drop_last else -(-self.num_samples // self.batch_size)

    def index_plan(self, epoch=None):
        """This rank's item indices for one epoch, in order (host, int64 numpy): item i is image i of shape i // views."""
        return epoch_plan(len(self.image_store), self.shuffle, self.seed, self.epoch if epoch is None else int(epoch), self.rank,
                          self.world_size)

    def __iter__(self):
        dev = self.mesh_store.device
        if self._state is None:
            seed = self.seed + 0x9E3779B97F4A7C15 * self.rank
            self._state, self._image_state = make_state(seed, dev), make_state(seed, dev)
        plan = self.index_plan()
        shape_rows = torch.from_numpy((plan // self.views).astype(np.int32)).to(dev)
        image_rows = torch.from_numpy(plan.astype(np.int32)).to(self.image_store.device)
        for b in range(len(self)):
            sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
            batch = sample_clouds(self.mesh_store, shape_rows[sl], self.cloud_size, self.return_eval_cloud, self.cloud_transform,
                                  self._state)
            batch['image'] = transform_images(self.image_store, image_rows[sl], self.image_transform, self._image_state)
            yield batch
