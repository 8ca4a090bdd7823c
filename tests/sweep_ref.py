"""Numpy restatement of the sweep routing launch (gwtf_mixture_route_sweep, csrc/gwtf_route.hip), shared by test_sweep_cpu.py and
test_gpu_sweep.py.  R rows in groups of `group`: row r takes the DRAWS of shape r // group (label words, normals, explicit labels or
base samples), its own logits, and per component a base Gaussian of its own.  The pieces are generate_ref's; with group = 1 and one
base per row this is generate_ref itself."""
import numpy as np

import generate_ref as gr


def shape_of_row(R, group):
    assert group >= 1 and R % group == 0
    return np.arange(R) // group


def labels_of(thr, words, group):
    """thr (R, K) uint32, words (R // group, n) uint32 -> (R, n) int32: row r searches its own thresholds with the words of its shape."""
    thr = np.asarray(thr, np.uint32)
    return gr.labels_of(thr, np.asarray(words, np.uint32)[shape_of_row(len(thr), group)])


def base_tables(mu0, lv0, R, K):
    """mu0 / lv0 as the launch takes them -- (R, 3), (1, 3), (K, R, 3) or (K, 1, 3) -- -> two (K, R, 3) float32 tables."""
    out = []
    for t in (mu0, lv0):
        t = np.asarray(t, np.float32)
        if t.ndim == 2:
            t = t[None]
        out.append(np.ascontiguousarray(np.broadcast_to(t, (K, R, 3))))
    return out


def base_samples(eps, labels, mu0, lv0, group, K):
    """eps (R // group, 3, n) standard normals, labels (R, n) -> (R, 3, n): eps * exp(0.5 lv0) + mu0 in float32 (reparameterize's
    order) with the base of every point's OWN component."""
    labels = np.asarray(labels)
    R, n = labels.shape
    mu, lv = base_tables(mu0, lv0, R, K)
    sd = np.exp(np.float32(0.5) * lv)
    rows = np.arange(R)[:, None]
    e = np.asarray(eps, np.float32)[shape_of_row(R, group)]                 # (R, 3, n)
    m = np.transpose(mu[labels, rows], (0, 2, 1))                           # (R, n, 3) -> (R, 3, n)
    s = np.transpose(sd[labels, rows], (0, 2, 1))
    return (e * s + m).astype(np.float32)


def route(logits, group, n, K, P, words=None, labels_in=None, normals=None, z0_in=None, mu0=None, lv0=None, thr=None, seed=None, call=0):
    """The whole launch -> dict(thresholds, labels, tile_comp, perm, z0 (R, 3, n) in the points' own order, zp (R, 3, tiles * P)).
    Draws that are not given are the Philox draws of (seed, call) for R // group shapes.  thr: thresholds to search with in place of
    the restated ones (a device's)."""
    R = len(logits) if logits is not None else len(labels_in) * group
    S = R // group
    rows = shape_of_row(R, group)
    res = {}
    if labels_in is not None:
        labels = np.clip(np.asarray(labels_in, np.int32), 0, K - 1)[rows]
    else:
        res['thresholds'] = gr.thresholds(logits) if thr is None else np.asarray(thr, np.uint32)
        labels = labels_of(res['thresholds'], gr.label_words(seed, call, S, n) if words is None else words, group)
    if z0_in is not None:
        z0 = np.asarray(z0_in, np.float32)[rows]
    else:
        z0 = base_samples(gr.normal_draws(seed, call, S, n) if normals is None else normals, labels, mu0, lv0, group, K)
    tile_comp, perm, _ = gr.layout(labels, K, P)
    zp = np.zeros((R, 3, perm.shape[1]), np.float32)
    for r in range(R):
        valid = perm[r] >= 0
        zp[r][:, valid] = z0[r][:, perm[r][valid]]
    res.update(labels=labels, tile_comp=tile_comp, perm=perm, z0=z0, zp=zp)
    return res
