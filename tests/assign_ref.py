"""Float64 numpy restatement of the per-point component posteriors (csrc/gwtf_assign.hip, evaluation.part_agreement), written from the
formulas of include/gwtf.h and from FlowMixtureNLL.forward (reference lib/networks/losses.py:101-122), not from the kernel.

For shape b, point n, component k:
    lp_k = -0.5 * sum_d [ lv0 + logdet + (z - mu0)^2 / exp(lv0) ] - 1.5 * log(2 pi) + log w_bk
    log w = log(exp(logit)) - logsumexp(logits)        (losses.py:101-104)
The reference evaluates log(exp(logit)) in float32, where exp underflows to 0 below a logit of about -104 and the log weight is -inf.
That quirk is part of the definition: the logit is taken to float32, and where its float32 exponential is 0 the log weight is -inf;
everywhere else log(exp(x)) = x in float64.
"""
import math

import numpy as np


def log_weights(logits):
    """(B, K) float64 log weights with the float32 underflow of the reference's exp."""
    lg32 = np.asarray(logits, np.float32)
    lg = lg32.astype(np.float64)
    m = lg.max(-1, keepdims=True)
    lse = m + np.log(np.exp(lg - m).sum(-1, keepdims=True))
    with np.errstate(under='ignore'):
        underflown = np.exp(lg32) == 0
    return np.where(underflown, -np.inf, lg) - lse


def lp(z, logdet, mu0, lv0, logits):
    """-> (K, B, N) float64."""
    z, logdet, mu0, lv0 = (np.asarray(a, np.float64) for a in (z, logdet, mu0, lv0))
    with np.errstate(invalid='ignore', over='ignore'):
        q = (lv0[..., None] + logdet + (z - mu0[..., None]) ** 2 / np.exp(lv0)[..., None]).sum(2)        # (K, B, N)
        return -0.5 * q - 1.5 * math.log(2.0 * math.pi) + log_weights(logits).T[:, :, None]


def log_density(lp_):
    """logsumexp over the components -> (B, N); -inf when every component is at -inf, NaN when any lp is NaN."""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        m = lp_.max(0)                                               # NaN when any lp is NaN
        safe = np.where(np.isfinite(m), m, 0.0)
        return np.where(np.isfinite(m), safe + np.log(np.exp(lp_ - safe).sum(0)), m)       # a maximum that is not finite: itself


def labels(lp_):
    """argmax_k lp_k with the lowest k on an exact tie; -1 where the log-density is not finite -> (B, N) int32."""
    finite = np.isfinite(log_density(lp_))
    best = np.argmax(np.where(np.isnan(lp_), -np.inf, lp_), axis=0)              # numpy: the first of equal maxima
    return np.where(finite, best, -1).astype(np.int32)


def resp(lp_):
    """exp(lp_k - log_density) -> (B, K, N), NaN in every k where the label is -1."""
    ld = log_density(lp_)
    ok = np.isfinite(ld)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.exp(lp_ - np.where(ok, ld, 0.0))
    return np.where(ok[None], r, np.nan).transpose(1, 0, 2)


def confidence(lp_):
    """The responsibility of the label, 0 where the label is -1 -> (B, N)."""
    lab = labels(lp_)
    r = np.take_along_axis(resp(lp_), np.maximum(lab, 0)[:, None, :], axis=1)[:, 0]
    return np.where(lab >= 0, r, 0.0)


def margin(lp_):
    """Best minus second-best lp per point -> (B, N); +inf with one component or when the runner-up is at -inf."""
    if lp_.shape[0] == 1:
        return np.full(lp_.shape[1:], np.inf)
    s = np.sort(np.where(np.isnan(lp_), -np.inf, lp_), axis=0)
    with np.errstate(invalid='ignore'):
        d = s[-1] - s[-2]
    return np.where(np.isnan(d), np.inf, d)


def delta(lp_, tol):
    """tol * max(1, max_k |lp_k|) over the finite lp_k of a point -> (B, N)."""
    a = np.where(np.isfinite(lp_), np.abs(lp_), 0.0).max(0)
    return tol * np.maximum(1.0, a)


def counts(labels_, K):
    """Points per (shape, component) -> (B, K) int32, and points labelled -1 per shape -> (B,) int32."""
    c = np.stack([np.bincount(row[row >= 0], minlength=K) for row in labels_]).astype(np.int32)
    return c, (labels_ < 0).sum(1).astype(np.int32)


def contingency(labels_, parts, K, P):
    """(K, P) int64 table of (label, part) over the points with a label >= 0 and a part in [0, P), and the number of points left out."""
    table, skipped = np.zeros((K, P), np.int64), 0
    for lab, part in zip(np.asarray(labels_).ravel(), np.asarray(parts).ravel()):
        if lab >= 0 and 0 <= part < P:
            table[lab, part] += 1
        else:
            skipped += 1
    return table, skipped


def part_agreement(table):
    """purity, nmi (nats, geometric normalisation), miou and the component -> part mapping of a (K, P) contingency table, by loops."""
    t = [[float(v) for v in row] for row in np.asarray(table)]
    K, P = len(t), len(t[0])
    mapping = []
    for row in t:
        best = 0
        for p in range(1, P):
            if row[p] > row[best]:
                best = p
        mapping.append(best)
    total = sum(sum(row) for row in t)
    if total == 0:
        return {'purity': math.nan, 'nmi': math.nan, 'miou': math.nan, 'mapping': mapping}
    purity = sum(max(row) for row in t) / total
    pk = [sum(row) / total for row in t]
    pp = [sum(t[k][p] for k in range(K)) / total for p in range(P)]
    h = lambda ps: -sum(p * math.log(p) for p in ps if p > 0)
    info = sum(t[k][p] / total * math.log(t[k][p] / total / (pk[k] * pp[p])) for k in range(K) for p in range(P) if t[k][p] > 0)
    hk, hp = h(pk), h(pp)
    nmi = info / math.sqrt(hk * hp) if hk > 0 and hp > 0 else 0.0
    ious = []
    for p in range(P):
        gt = sum(t[k][p] for k in range(K))
        if gt == 0:
            continue
        pred = sum(sum(t[k]) for k in range(K) if mapping[k] == p)
        tp = sum(t[k][p] for k in range(K) if mapping[k] == p)
        ious.append(tp / (gt + pred - tp))
    return {'purity': purity, 'nmi': nmi, 'miou': sum(ious) / len(ious), 'mapping': mapping}
