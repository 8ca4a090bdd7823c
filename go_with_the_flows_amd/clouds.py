"""Training batches drawn on the device (csrc/gwtf_clouds.hip): the reference's ShapeNetCoreDataset.__getitem__
(lib/datasets/datasets.py:69-106) -- sample_cloud (lib/datasets/cloud_sampling.py:4-32) and the composed cloud transformations
(lib/datasets/cloud_transformations.py:79-103) -- for a whole batch in one call, from meshes that stay in device memory.

    store = MeshStore.from_h5('.../meshes.h5', 'train', device='cuda')
    loader = DeviceCloudLoader(store, 64, 2048, transform=CloudTransform.from_config(**config))
    for batch in loader:                       # {'cloud': (B,3,N), 'eval_cloud': (B,3,N), 'orig_c': (B,3), 'orig_s': (B,)} on the device

Host work happens once, at construction: the per-face integer thresholds of every shape's area CDF, built with the reference's own
arithmetic.  There is no CPU sampling path: sample_clouds on a CPU store raises.

Data that are point clouds already go into a CloudStore, which stands wherever a MeshStore stands: a batch row then draws its
points from the stored cloud without replacement (sample_stored_clouds), or reads them in stored order (permute=False).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GwtfError

TWO32 = 4294967296.0


def face_cdf(vertices_c, faces_vc):
    """(probs float32, cdf float64) of one mesh exactly as sample_cloud + RandomState.choice compute them
    (cloud_sampling.py:5-10; choice: cdf = cumsum(float64(p)), cdf /= cdf[-1])."""
    polygons = np.asarray(vertices_c, np.float32)[np.asarray(faces_vc).astype(np.int64)]
    cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
    areas = np.sqrt((cross**2).sum(1)) / 2.0
    probs = areas / areas.sum()
    cdf = np.cumsum(probs.astype(np.float64))
    cdf /= cdf[-1]
    return probs, cdf


def face_thresholds(cdf):
    """(T uint32, search_len): T[k] = ceil(cdf[k] * 2^32) -- exact in float64, a scaling by a power of two -- so that for a 32-bit
    word w   #{k : T[k] <= w} == np.searchsorted(cdf, w * 2^-32, 'right').   Thresholds that reach 2^32 (the last face's always
    does) lie above every word: they are stored as 0xffffffff and left out of the search, whose length is the second result."""
    t = np.ceil(cdf * TWO32)
    search_len = int(np.count_nonzero(t < TWO32))
    if np.any(np.diff(t) < 0):
        raise GwtfError('face CDF is not monotone')
    return np.minimum(t, TWO32 - 1).astype(np.uint32), search_len


def search_faces(thresholds, search_len, words):
    """The device's face search on the host (numpy): #{k < search_len : T[k] <= w}."""
    return np.searchsorted(thresholds[:search_len], np.asarray(words, np.uint32), side='right')


def _take_slices(data, bounds, keep):
    """The slices data[bounds[i]:bounds[i+1]] for i in keep, repacked -> (data, bounds)."""
    bounds = np.asarray(bounds).astype(np.int64)
    parts = [data[bounds[i]:bounds[i + 1]] for i in keep]
    return (np.concatenate(parts) if parts else data[:0]), np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)


class MeshStore:
    """The packed meshes of one part of meshes.h5 (preprocess_ShapeNetCore.py:55-69) on one device, with their face thresholds."""

    def __init__(self):
        raise TypeError('use MeshStore.from_arrays / MeshStore.from_h5')

    @classmethod
    def from_arrays(cls, vertices_c, faces_vc, vertices_c_bounds, faces_bounds, orig_c=None, orig_s=None, device='cuda'):
        self = object.__new__(cls)
        vertices = np.ascontiguousarray(vertices_c, dtype=np.float32)
        faces = np.ascontiguousarray(faces_vc).astype(np.int64)
        vb = np.asarray(vertices_c_bounds).astype(np.int64)
        fb = np.asarray(faces_bounds).astype(np.int64)
        if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
            raise GwtfError('vertices_c must be (V,3) and faces_vc (F,3)')
        n = len(vb) - 1
        if n < 1 or len(fb) != n + 1:
            raise GwtfError('vertices_c_bounds and faces_bounds must both hold n_shapes + 1 entries')
        if vb[0] < 0 or fb[0] < 0 or vb[-1] > len(vertices) or fb[-1] > len(faces) or np.any(np.diff(vb) < 0) or np.any(np.diff(fb) < 0):
            raise GwtfError('bounds are not ascending offsets into vertices_c / faces_vc')
        thresholds = np.full(len(faces), 0xffffffff, np.uint32)
        search_len = np.zeros(n, np.int32)
        for i in range(n):
            f = faces[fb[i]:fb[i + 1]]
            v = vertices[vb[i]:vb[i + 1]]
            if len(f) == 0:
                raise GwtfError(f'shape {i} has no faces')
            if len(f) >= 2**31:
                raise GwtfError(f'shape {i} has too many faces')
            if f.min() < 0 or f.max() >= len(v):
                raise GwtfError(f'shape {i}: a face names a vertex outside the shape\'s {len(v)} vertices')
            with np.errstate(invalid='ignore', divide='ignore'):
                _, cdf = face_cdf(v, f)
            if not np.all(np.isfinite(cdf)) or not cdf[-1] == 1.0:
                raise GwtfError(f'shape {i} has zero total face area')
            thresholds[fb[i]:fb[i + 1]], search_len[i] = face_thresholds(cdf)
        self.n_shapes = n
        self.thresholds_host, self.search_len_host = thresholds, search_len
        self.vertices_bounds_host, self.faces_bounds_host = vb, fb
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.vertices = up(vertices)
        self.faces = up(faces.astype(np.int32))
        self.thresholds = up(thresholds.view(np.int32))          # the bits of the uint32 thresholds
        self.vertices_bounds, self.faces_bounds, self.search_len = up(vb), up(fb), up(search_len)
        self.orig_c = None if orig_c is None else up(np.asarray(orig_c, np.float32).reshape(n, 3))
        self.orig_s = None if orig_s is None else up(np.asarray(orig_s, np.float32).reshape(n))
        self._work = {}
        self._state = None
        return self

    @classmethod
    def from_h5(cls, path, part='train', return_original_scale=True, chosen_label=None, device='cuda'):
        """The dataset reads of ShapeNetCoreDataset.choose_part / __getitem__ (datasets.py:33-57,78-85), once for the whole part;
        chosen_label keeps the shapes of one class, as the dataset's chosen_label_inds does."""
        try:
            import h5py
        except ImportError as e:
            raise GwtfError('MeshStore.from_h5 needs h5py, which is not installed; read the datasets yourself and use '
                            'MeshStore.from_arrays') from e
        with h5py.File(path, 'r') as fin:
            v, f, vb, fb = [np.array(fin[part + '_' + k]) for k in ('vertices_c', 'faces_vc', 'vertices_c_bounds', 'faces_bounds')]
            orig_c, orig_s = [np.array(fin[part + '_' + k]) for k in ('orig_c', 'orig_s')] if return_original_scale else [None, None]
            keep = None if chosen_label is None else (np.array(fin[part + '_labels'], dtype=np.uint8) == chosen_label).nonzero()[0]
        if keep is not None:
            v, vb = _take_slices(v, vb, keep)
            f, fb = _take_slices(f, fb, keep)
            orig_c, orig_s = (None, None) if orig_c is None else (orig_c[keep], orig_s[keep])
        return cls.from_arrays(v, f, vb, fb, orig_c=orig_c, orig_s=orig_s, device=device)

    def __len__(self):
        return self.n_shapes


class CloudTransform:
    """The record of cloud transformations the kernel fuses, in ComposeCloudTransformation's order
    (cloud_transformations.py:79-96): Scale2OrigCloud, TranslateCloud, ScaleCloud, AddNoise2Cloud, CenterCloud."""

    def __init__(self, rescale2orig=False, recenter2orig=False, translate=False, translate_shift=(0.0, 0.0, 0.0), scale=False,
                 scale_scale=1.0, noise=False, noise_scale=1.0, center=False):
        self.rescale2orig, self.recenter2orig = bool(rescale2orig), bool(recenter2orig)
        self.translate, self.scale, self.noise, self.center = bool(translate), bool(scale), bool(noise), bool(center)
        self.translate_shift = tuple(float(np.float32(v)) for v in np.asarray(translate_shift, np.float32).reshape(-1)) \
            if self.translate else (0.0, 0.0, 0.0)
        if len(self.translate_shift) != 3:
            raise ValueError('cloud_translate_shift must hold three values')
        self.scale_scale = float(np.float32(scale_scale)) if self.scale else 1.0
        self.noise_scale = float(np.float32(noise_scale)) if self.noise else 1.0
        if self.scale and not self.scale_scale > 0:
            raise ValueError('cloud_scale_scale must be positive')
        if self.noise and not self.noise_scale > 0:
            raise ValueError('cloud_noise_scale must be positive')

    @classmethod
    def from_config(cls, **kwargs):
        """From the reference's config keys; keys it does not know (the rest of a config file) are ignored."""
        if kwargs.get('cloud_random_rotate'):
            raise NotImplementedError(
                'cloud_random_rotate: the reference\'s Random3DRotation raises NameError (Rotation is never imported, '
                'cloud_transformations.py:70) and would compute eval_cloud from the already rotated cloud; it is not reproduced')
        return cls(rescale2orig=kwargs.get('cloud_rescale2orig', False), recenter2orig=kwargs.get('cloud_recenter2orig', False),
                   translate=kwargs.get('cloud_translate', False), translate_shift=kwargs.get('cloud_translate_shift') or (0, 0, 0),
                   scale=kwargs.get('cloud_scale', False), scale_scale=kwargs.get('cloud_scale_scale') or 1.0,
                   noise=kwargs.get('cloud_noise', False), noise_scale=kwargs.get('cloud_noise_scale') or 1.0,
                   center=kwargs.get('cloud_center', False))


def make_state(seed, device='cuda', call=0):
    """The device-resident (seed, call) pair of the sampler: every call (and every replay of a captured call) reads it and leaves
    call one higher."""
    seed, call = int(seed) & (2**64 - 1), int(call)
    if not 0 <= call < 2**60:
        raise ValueError('call must lie in [0, 2^60)')
    return torch.tensor([seed - 2**64 if seed >= 2**63 else seed, call], dtype=torch.int64, device=device)


def cloud_partials(M):
    return _lib.lib().gwtf_cloud_partials(int(M))


def _prepare_batch(store, rows, cloud_size, return_eval_cloud, transform, state, out):
    """The checks and buffers the two samplers share -> (transform, B, N, M, result dict, partials or None, state)."""
    if store.device.type != 'cuda':
        raise GwtfError(f'the store lives on {store.device}: sampling runs on a HIP device only, there is no CPU path')
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != store.device or not rows.is_contiguous():
        raise GwtfError('rows must be a contiguous 1-d int32 tensor on the store\'s device')
    t = transform if transform is not None else _IDENTITY
    if (t.rescale2orig and store.orig_s is None) or (t.recenter2orig and store.orig_c is None):
        raise GwtfError('the transformation scales back to the original frame but the store has no orig_c / orig_s')
    B, N = rows.numel(), int(cloud_size)
    M = 2 * N if return_eval_cloud else N
    dev = store.device
    if out is None:
        out = {'cloud': torch.empty(B, 3, N, device=dev, dtype=torch.float32)}
        if return_eval_cloud:
            out['eval_cloud'] = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
    res = {'cloud': out['cloud']}
    if return_eval_cloud:
        res['eval_cloud'] = out['eval_cloud']
    for k, v in res.items():
        if tuple(v.shape) != (B, 3, N):
            raise GwtfError(f'out[{k!r}] is {tuple(v.shape)}, expected {(B, 3, N)}')
    partials = None
    if t.center:
        partials = store._work.get((B, M))
        if partials is None:
            partials = store._work[(B, M)] = torch.empty(B, max(1, cloud_partials(M)), 6, device=dev, dtype=torch.float32)
    if state is None:
        if store._state is None:
            store._state = make_state(0, dev)
        state = store._state
    if state.dtype != torch.int64 or state.numel() != 2 or state.device != dev:
        raise GwtfError('state must come from make_state(seed, device) on the store\'s device')
    return t, B, N, M, res, partials, state


def _explicit_pointers(explicit, fields, dev):
    """Device addresses of the explicit draws named in fields ((key, shape, dtype), ...), each checked."""
    ex = {}
    if explicit is not None:
        for k, shape, dt in fields:
            v = explicit[k]
            if tuple(v.shape) != shape or v.dtype != dt or v.device != dev or not v.is_contiguous():
                raise GwtfError(f'explicit[{k!r}] must be a contiguous {dt} tensor of shape {shape} on the store\'s device')
            ex[k] = v.data_ptr()
    return ex


def _with_original_frame(store, rows, res):
    if store.orig_c is not None or store.orig_s is not None:
        inside = rows.clamp(0, store.n_shapes - 1)            # a row outside the store has NaN points; its gather must stay in bounds
        if store.orig_c is not None:
            res['orig_c'] = store.orig_c.index_select(0, inside)
        if store.orig_s is not None:
            res['orig_s'] = store.orig_s.index_select(0, inside)
    return res


_ptr_or_null = lambda x: None if x is None else x.data_ptr()


def sample_clouds(store, rows, cloud_size, return_eval_cloud=True, transform=None, state=None, explicit=None, out=None, permute=True):
    """One batch: rows (B,) int32 shape indices on the store's device -> {'cloud': (B,3,cloud_size)[, 'eval_cloud'][, 'orig_c',
    'orig_s']}, the keys and shapes of a collated reference batch.  Enqueued on the current stream; nothing waits for the device.

    state: make_state(seed) (default: one the store keeps, seed 0).  explicit: {'words': (B,M) int32 bits of the uint32 face words,
    's1', 's2': (B,M) float32, 'normals': (B,3,M) float32 when noise is on} replaces Philox (M = 2 * cloud_size with an eval cloud).
    The scratch of a given (B, M) is allocated on the first call and kept on the store.  The returned tensors are fresh ones from
    torch's allocator (which a graph capture records like any other); pass out={'cloud': ..., 'eval_cloud': ...} to write into
    tensors of your own and allocate nothing at all.

    A CloudStore goes to sample_stored_clouds with the same arguments (explicit and permute as described there); permute=False
    means nothing for meshes and raises."""
    if isinstance(store, CloudStore):
        return sample_stored_clouds(store, rows, cloud_size, return_eval_cloud, transform, state, explicit, out, permute)
    if not permute:
        raise ValueError('permute=False asks for the stored order of a CloudStore; a MeshStore has none')
    t, B, N, M, res, partials, state = _prepare_batch(store, rows, cloud_size, return_eval_cloud, transform, state, out)
    dev = store.device
    ex = _explicit_pointers(explicit, (('words', (B, M), torch.int32), ('s1', (B, M), torch.float32), ('s2', (B, M), torch.float32)) +
                            ((('normals', (B, 3, M), torch.float32),) if t.noise else ()), dev)
    ptr = _ptr_or_null
    a = _lib.CloudArgs(
        rows=rows.data_ptr(), vertices=store.vertices.data_ptr(), faces=store.faces.data_ptr(), thresholds=store.thresholds.data_ptr(),
        vertices_bounds=store.vertices_bounds.data_ptr(), faces_bounds=store.faces_bounds.data_ptr(),
        search_len=store.search_len.data_ptr(), orig_c=ptr(store.orig_c), orig_s=ptr(store.orig_s),
        cloud=_lib._ptr(res['cloud'], 'cloud'), eval_cloud=_lib._ptr(res.get('eval_cloud'), 'eval_cloud'), partials=ptr(partials),
        state=state.data_ptr(), words=ex.get('words'), s1=ex.get('s1'), s2=ex.get('s2'), normals=ex.get('normals'),
        B=B, M=M, n_shapes=store.n_shapes, rescale=t.rescale2orig, recenter=t.recenter2orig, translate=t.translate, scale=t.scale,
        noise=t.noise, center=t.center, tune=_lib.tune_word(), shift=(ctypes.c_float * 3)(*t.translate_shift),
        scale_div=t.scale_scale, noise_scale=t.noise_scale, stream=torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gwtf_sample_clouds(ctypes.addressof(a)))
    return _with_original_frame(store, rows, res)


class CloudStore:
    """Point clouds that stay in device memory -- scans, a pre-sampled set, a frozen evaluation set -- packed as points (T,3)
    float32 with bounds (S+1,) int64; cloud s is points[bounds[s]:bounds[s+1]].  It stands wherever a MeshStore stands
    (sample_clouds, the loaders, the resident loops, evaluate_*): batches are drawn from the stored points, without replacement
    while a batch row asks for no more points than its cloud holds (sample_stored_clouds)."""

    def __init__(self):
        raise TypeError('use CloudStore.from_arrays / CloudStore.from_mesh_store')

    @classmethod
    def from_arrays(cls, points, bounds=None, orig_c=None, orig_s=None, device='cuda'):
        """points: (S, P, 3) equal-sized clouds, or packed (T, 3) with bounds (S+1,) ascending offsets into it."""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if bounds is None:
            if pts.ndim != 3 or pts.shape[2] != 3:
                raise GwtfError('points must be (S, P, 3), or packed (T, 3) together with bounds')
            b = np.arange(pts.shape[0] + 1, dtype=np.int64) * pts.shape[1]
            pts = pts.reshape(-1, 3)
        else:
            if pts.ndim != 2 or pts.shape[1] != 3:
                raise GwtfError('packed points must be (T, 3)')
            b = np.asarray(bounds).astype(np.int64).reshape(-1)
        cls._check_bounds(b, len(pts))
        return cls._from_device(torch.from_numpy(pts).to(device), b, orig_c, orig_s)

    @staticmethod
    def _check_bounds(b, total):
        n = len(b) - 1
        if n < 1:
            raise GwtfError('bounds must hold n_shapes + 1 entries, n_shapes >= 1')
        if b[0] < 0 or b[-1] > total or np.any(np.diff(b) < 0):
            raise GwtfError('bounds are not ascending offsets into points')
        sizes = np.diff(b)
        if np.any(sizes == 0):
            raise GwtfError(f'cloud {int(np.flatnonzero(sizes == 0)[0])} has no points')
        if np.any(sizes >= 2**31):
            raise GwtfError(f'cloud {int(np.flatnonzero(sizes >= 2**31)[0])} has too many points')

    @classmethod
    def _from_device(cls, points, bounds_host, orig_c, orig_s):
        self = object.__new__(cls)
        n = len(bounds_host) - 1
        self.n_shapes, self.bounds_host, self.device = n, bounds_host, points.device
        self.points = points.contiguous()
        self.bounds = torch.from_numpy(bounds_host).to(self.device)

        def frame(a, shape):
            if a is None:
                return None
            a = a.detach().to(torch.float32) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float32))
            return a.reshape(shape).contiguous().to(self.device)
        self.orig_c, self.orig_s = frame(orig_c, (n, 3)), frame(orig_s, (n,))
        self._work = {}
        self._state = self._stored_order_state = None
        return self

    @classmethod
    def from_mesh_store(cls, mesh_store, points_per_shape, seed=0, chunk=64):
        """Freeze points_per_shape points of every mesh: sample_clouds(mesh_store, rows, points_per_shape, False, None, state) for
        rows = chunk consecutive shapes at a time in store order, all calls on the one state make_state(seed)."""
        P, S, dev = int(points_per_shape), len(mesh_store), mesh_store.device
        if P < 1 or chunk < 1:
            raise ValueError('points_per_shape and chunk must be positive')
        state = make_state(seed, dev)
        rows = torch.arange(S, dtype=torch.int32, device=dev)
        parts = [sample_clouds(mesh_store, rows[i:i + chunk], P, False, None, state)['cloud'].transpose(1, 2) for i in range(0, S, chunk)]
        return cls._from_device(torch.cat(parts).reshape(-1, 3), np.arange(S + 1, dtype=np.int64) * P, mesh_store.orig_c,
                                mesh_store.orig_s)

    def __len__(self):
        return self.n_shapes

    def clouds(self, rows=None, n_points=None):
        """(len(rows), 3, n_points): the first n_points (default: as many as the smallest selected cloud holds) of each selected
        cloud (default: all) in stored order -- a fixed set, e.g. the ref_clouds of evaluate_generation (which takes them
        point-major: .transpose(1, 2)).  The states of the samplers do not move."""
        idx = np.arange(self.n_shapes) if rows is None else np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).astype(np.int64).reshape(-1)
        if len(idx) < 1 or idx.min() < 0 or idx.max() >= self.n_shapes:
            raise GwtfError(f'rows must name clouds in [0, {self.n_shapes})')
        smallest = int(np.diff(self.bounds_host)[idx].min())
        n = smallest if n_points is None else int(n_points)
        if not 1 <= n <= smallest:
            raise GwtfError(f'n_points must lie in [1, {smallest}], the size of the smallest selected cloud')
        if self._stored_order_state is None and self.device.type == 'cuda':
            self._stored_order_state = make_state(0, self.device)
        out = []
        for i in range(0, len(idx), 65535):
            r = torch.from_numpy(idx[i:i + 65535].astype(np.int32)).to(self.device)
            out.append(sample_stored_clouds(self, r, n, False, None, self._stored_order_state, permute=False)['cloud'])
        return out[0] if len(out) == 1 else torch.cat(out)


def sample_stored_clouds(store, rows, cloud_size, return_eval_cloud=True, transform=None, state=None, explicit=None, out=None,
                         permute=True):
    """sample_clouds for a CloudStore: the same arguments, checks, out= contract and returned keys.  Point j of a row is the stored
    point at the index the keyed bijection of include/gwtf.h (GwtfStoredCloudArgs) gives: without replacement while M = (2 *)
    cloud_size stays at or below the cloud's size -- cloud and eval_cloud are then disjoint -- and wrapping into a fresh permutation
    past it.  permute=False: the stored order.  explicit: {'index': (B,M) int32 point indices, 'normals': (B,3,M) float32 when noise
    is on}; an index outside its cloud gives a NaN point."""
    t, B, N, M, res, partials, state = _prepare_batch(store, rows, cloud_size, return_eval_cloud, transform, state, out)
    dev = store.device
    ex = _explicit_pointers(explicit, (('index', (B, M), torch.int32),) + ((('normals', (B, 3, M), torch.float32),) if t.noise else ()), dev)
    ptr = _ptr_or_null
    a = _lib.StoredCloudArgs(
        rows=rows.data_ptr(), points=store.points.data_ptr(), bounds=store.bounds.data_ptr(), orig_c=ptr(store.orig_c),
        orig_s=ptr(store.orig_s), cloud=_lib._ptr(res['cloud'], 'cloud'), eval_cloud=_lib._ptr(res.get('eval_cloud'), 'eval_cloud'),
        partials=ptr(partials), state=state.data_ptr(), index=ex.get('index'), normals=ex.get('normals'), B=B, M=M,
        n_shapes=store.n_shapes, rescale=t.rescale2orig, recenter=t.recenter2orig, translate=t.translate, scale=t.scale, noise=t.noise,
        center=t.center, permute=bool(permute), tune=_lib.tune_word(), shift=(ctypes.c_float * 3)(*t.translate_shift),
        scale_div=t.scale_scale, noise_scale=t.noise_scale, stream=torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gwtf_sample_stored_clouds(ctypes.addressof(a)))
    return _with_original_frame(store, rows, res)


_IDENTITY = CloudTransform()


def epoch_plan(n, shuffle, seed, epoch, rank=0, world_size=1):
    """One rank's item indices of one epoch over n items, in order (host, int64 numpy): torch.randperm under a generator seeded
    seed + epoch, then the padding and stride of torch.utils.data.DistributedSampler (drop_last=False).  The loaders of this
    module and of images.py share it."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = -(-n // world_size) * world_size
    pad = total - len(idx)
    if pad > 0:
        idx += (idx * -(-pad // len(idx)))[:pad]
    return np.asarray(idx[rank:total:world_size], np.int64)


class DeviceCloudLoader:
    """Stands where DataLoader(ShapeNetCoreDataset(...), batch_size, shuffle=True, drop_last=True) stood (train_ae.py:85-116): an
    iterable of device batches.  The epoch's order is a host permutation from (seed, epoch) -- torch.randperm under a generator
    seeded seed + epoch, and for world_size > 1 the padding and stride of torch.utils.data.DistributedSampler, whose indices a rank
    therefore reproduces; the points come from the device sampler, whose state lives on the device and advances by itself.
    store: a MeshStore or a CloudStore.  permute=False (CloudStore only) reads every cloud in its stored order, so the loader
    yields the same clouds every epoch -- a frozen validation set."""

    def __init__(self, store, batch_size, cloud_size, transform=None, shuffle=True, drop_last=True, seed=0, rank=0, world_size=1,
                 return_eval_cloud=True, permute=True):
        if not 0 <= rank < world_size:
            raise ValueError('rank must lie in [0, world_size)')
        if batch_size < 1:
            raise ValueError('batch_size must be positive')
        self.store, self.batch_size, self.cloud_size, self.transform = store, int(batch_size), int(cloud_size), transform
        self.shuffle, self.drop_last, self.seed, self.rank, self.world_size = bool(shuffle), bool(drop_last), int(seed), rank, world_size
        self.return_eval_cloud = bool(return_eval_cloud)
        self.permute = bool(permute)                                  # False: a CloudStore's points in stored order, every epoch
        if not self.permute and not isinstance(store, CloudStore):
            raise ValueError('permute=False asks for the stored order of a CloudStore; a MeshStore has none')
        self.epoch = 0
        self.num_samples = -(-len(store) // world_size)               # DistributedSampler, drop_last=False: ceil
        self._state = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.num_samples // self.batch_size if self.drop_last else -(-self.num_samples // self.batch_size)

    def index_plan(self, epoch=None):
        """This rank's shape indices for one epoch, in order (host, int64 numpy); batches are consecutive slices of it."""
        return epoch_plan(len(self.store), self.shuffle, self.seed, self.epoch if epoch is None else int(epoch), self.rank,
                          self.world_size)

    def __iter__(self):
        dev = self.store.device
        if self._state is None:                                       # ranks draw from different Philox keys
            self._state = make_state(self.seed + 0x9E3779B97F4A7C15 * self.rank, dev)
        rows = torch.from_numpy(self.index_plan().astype(np.int32)).to(dev)
        for b in range(len(self)):
            yield sample_clouds(self.store, rows[b * self.batch_size:(b + 1) * self.batch_size], self.cloud_size,
                                self.return_eval_cloud, self.transform, self._state, permute=self.permute)
