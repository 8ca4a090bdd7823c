"""Numpy restatement of the routing kernel (csrc/gwtf_route.hip), shared by test_generate_cpu.py and test_gpu_generate.py: the
integer thresholds of a shape's mixture weights, the component of a point, the tile layout of a shape, and the Philox draws of a call
(clouds_ref has Philox itself)."""
import numpy as np

import clouds_ref as cr

TWO32 = 4294967296.0
STREAM_LABEL, STREAM_NORMAL = 2, 3        # the cloud sampler uses 0 and 1 (include/gwtf.h)
SEED = 2024                               # the component-count tests (restatement and device) draw from this seed


def route_tiles(n, K, P):
    return (n + K * (P - 1)) // P


def thresholds(logits):
    """(S, K) float32 logits -> (S, K) uint32: T[k] = min(ceil(cdf[k] / cdf[K-1] * 2^32), 2^32 - 1), cdf in float64."""
    l = np.asarray(logits, np.float32).astype(np.float64)
    cdf = np.cumsum(np.exp(l - l.max(1, keepdims=True)), axis=1)
    return np.minimum(np.ceil(cdf / cdf[:, -1:] * TWO32), TWO32 - 1).astype(np.uint32)


def labels_of(thr, words):
    """#{k < K-1 : T[k] <= w} for every word: thr (S, K) uint32, words (S, n) uint32 -> (S, n) int32."""
    thr, words = np.asarray(thr, np.uint32), np.asarray(words, np.uint32)
    return np.stack([np.searchsorted(thr[s, :-1], words[s], side='right') for s in range(len(words))]).astype(np.int32)


def layout(labels, K, P):
    """labels (S, n) in [0, K) -> (tile_comp (S, tiles), perm (S, tiles * P), tiles used per shape (S,)): component k takes
    ceil(c_k / P) consecutive tiles in component order, its points in their original order; -1 elsewhere."""
    labels = np.asarray(labels)
    S, n = labels.shape
    tiles = route_tiles(n, K, P)
    tile_comp = np.full((S, tiles), -1, np.int32)
    perm = np.full((S, tiles * P), -1, np.int32)
    used = np.zeros(S, np.int64)
    for s in range(S):
        t = 0
        for k in range(K):
            idx = np.nonzero(labels[s] == k)[0]
            nt = -(-len(idx) // P)
            tile_comp[s, t:t + nt] = k
            perm[s, t * P:t * P + len(idx)] = idx
            t += nt
        used[s] = t
    return tile_comp, perm, used


def label_words(seed, call, S, n):
    """(S, n) uint32: word 0 of the label stream."""
    return cr.draws(seed, call, S, n, STREAM_LABEL)[0]


def normal_draws(seed, call, S, n):
    """(S, 3, n) float32 standard normals of the normal stream: Box-Muller on (w0, w1) -> 0, 1 and (w2, w3) -> 2 (the layout of
    clouds_ref.noise_draws)."""
    w = cr.draws(seed, call, S, n, STREAM_NORMAL)

    def pair(a, b):
        u1 = ((a >> 8).astype(np.float32) + np.float32(1)) * np.float32(2.0**-24)
        u2 = (b >> 8).astype(np.float32) * np.float32(2.0**-24)
        rad, ang = np.sqrt(np.float32(-2) * np.log(u1)), np.float32(2 * np.pi) * u2
        return rad * np.cos(ang), rad * np.sin(ang)
    x, y = pair(w[0], w[1])
    z, _ = pair(w[2], w[3])
    return np.stack([x, y, z], axis=1).astype(np.float32)


def base_samples(eps, mu0, lv0):
    """eps (S, 3, n); mu0, lv0 (S or 1, 3) -> eps * exp(0.5 lv0) + mu0 in float32 (reparameterize's order)."""
    mu0, lv0 = np.asarray(mu0, np.float32), np.asarray(lv0, np.float32)
    return (eps.astype(np.float32) * np.exp(np.float32(0.5) * lv0)[:, :, None] + mu0[:, :, None]).astype(np.float32)


def ranks_within_component(labels_row):
    """rank of every point among the points of its own component, in original order."""
    r = np.zeros(len(labels_row), np.int64)
    for k in np.unique(labels_row):
        idx = np.nonzero(labels_row == k)[0]
        r[idx] = np.arange(len(idx))
    return r


def crafted_labels(n, K, P, seed=0):
    """Five label rows for K >= 3 that sit on the layout's edges: all points in one component; a count of exactly P; P + 1; 1; an
    empty component in the middle.  Positions are shuffled."""
    assert K >= 3 and n > 2 * P + 2
    rng = np.random.RandomState(seed)

    def row(counts):            # counts of components 0 .. K-2, the rest goes to K-1
        lab = np.full(n, K - 1, np.int32)
        pos, off = rng.permutation(n), 0
        for k, c in enumerate(counts):
            lab[pos[off:off + c]] = k
            off += c
        return lab
    return np.stack([np.full(n, K - 2, np.int32), row([P]), row([P + 1]), row([n // 2, 1]), row([n // 3, 0])])
