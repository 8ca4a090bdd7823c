"""Numpy restatement of the stored-cloud sampler's index rule (include/gwtf.h, GwtfStoredCloudArgs; csrc/gwtf_perm.h), shared by
test_cloud_store_cpu.py and test_gpu_cloud_store.py: the six-round keyed Feistel bijection on [0, P), its Philox round keys, and
the indices of one call."""
import numpy as np

from clouds_ref import noise_draws, philox4x32_10  # noqa: F401  (noise_draws: re-exported for the GPU tests)

WALK_CAP = 1024
NO_INDEX = 0xffffffff


def fmix32(x):
    """murmur3's 32-bit finaliser on uint64 arrays holding 32-bit values."""
    m = np.uint64(0xffffffff)
    x = np.asarray(x, np.uint64) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x


def half_bits(P):
    """h of the domain 2^(2h): b = max(1, ceil(log2 P)), h = (b + 1) // 2."""
    b = max(1, (int(P) - 1).bit_length())
    return (b + 1) // 2


def perm_index(keys, t, P):
    """Images of the slots t (array, all < P) under the permutation of [0, P) keyed by keys: six uint32, each a scalar or an array
    broadcastable against t.  NO_INDEX where the walk passes WALK_CAP steps."""
    P = int(P)
    assert 1 <= P < 2**31
    h = np.uint64(half_bits(P))
    mask = (np.uint64(1) << h) - np.uint64(1)
    x = np.array(t, dtype=np.uint64, copy=True).reshape(np.shape(t))
    assert np.all(x < P)
    keys = [np.broadcast_to(np.asarray(k, np.uint64) & np.uint64(0xffffffff), x.shape) for k in keys]
    out = np.full(x.shape, NO_INDEX, np.uint64)
    walking = np.ones(x.shape, bool)
    for _ in range(WALK_CAP):
        if not walking.any():
            break
        xs = x[walking]
        L, R = xs >> h, xs & mask
        for k in keys:
            L, R = R, L ^ (fmix32(R ^ k[walking]) >> (np.uint64(32) - h))
        xs = (L << h) | R
        x[walking] = xs
        done = np.zeros(x.shape, bool)
        done[walking] = xs < P
        out[done] = x[done]
        walking &= ~done
    return out.astype(np.uint32)


def round_keys(seed, call, r, q):
    """K0..K5 of batch row r in round q (arrays broadcast): Philox blocks (2q, r, call, stream 2) and (2q + 1, ...)."""
    seed, call = int(seed) & (2**64 - 1), int(call)
    key = (seed & 0xffffffff, seed >> 32)
    q, r = np.asarray(q, np.uint64), np.asarray(r, np.uint64)
    c2, c3 = call & 0xffffffff, (call >> 32) | (2 << 28)
    a = philox4x32_10((2 * q, r, c2, c3), key)
    b = philox4x32_10((2 * q + 1, r, c2, c3), key)
    return [a[0], a[1], a[2], a[3], b[0], b[1]]


def stored_indices(seed, call, sizes, M, permute=True):
    """(B, M) int64 point indices of one call: row r draws from a cloud of sizes[r] points."""
    sizes = np.asarray(sizes, np.int64)
    out = np.zeros((len(sizes), M), np.int64)
    j = np.arange(M, dtype=np.uint64)
    for P in np.unique(sizes):                                # the rows of one size at once
        rows = np.flatnonzero(sizes == P)
        q, t = j // np.uint64(P), j % np.uint64(P)
        if permute:
            keys = round_keys(seed, call, rows[:, None], q[None, :])
            out[rows] = perm_index(keys, np.broadcast_to(t, (len(rows), M)), P)
        else:
            out[rows] = t
    return out


def gather(points, bounds, rows, index):
    """(B, 3, M) float32: points[bounds[rows[r]] + index[r, j]], NaN where the row or the index lies outside."""
    B, M = index.shape
    out = np.full((B, 3, M), np.nan, np.float32)
    for r, s in enumerate(rows):
        if not 0 <= s < len(bounds) - 1:
            continue
        P = int(bounds[s + 1] - bounds[s])
        ok = (index[r] >= 0) & (index[r] < P)
        out[r][:, ok] = points[int(bounds[s]) + index[r][ok]].T
    return out
