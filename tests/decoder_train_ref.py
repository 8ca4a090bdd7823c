"""Reference form of the decoder's differentiable pass in plain torch on the CPU: what test_decoder_train_ref_cpu.py validates and
test_gpu_decoder_bwd_f64.py compares csrc/gwtf_bwd.hip and the folds of csrc/gwtf_train.hip against.  No device code runs here and no
second port of the decoder is written: oracle/torch_port.decoder_fused (pinned to the genuine reference by the golden fixtures) in
float64 or float32, differentiated by autograd.

A case is a Case record: the decoders decoder_and_state(L, f, G, MODEL_SEED + k), k < K, the inputs case_inputs builds from its seed.
M = 0: the plain cloud synth_inputs(B, N, G, seed).  M > 0: a TILED cloud -- M distinct points per shape, repeated to length N in a
shuffled order.  The BatchNorm statistics of such a cloud are those of a cloud of a few points, so the float64 reference has B * M
distinct ReLU inputs per channel however large N is, and a seed can be found with none of them near its kink; every POSITION still
carries its own random-sign cotangent, so a kernel that drops or duplicates a position, or misplaces an output or a cotangent,
changes the gradients.  What a tiled cloud does NOT see is a kernel that reads the INPUT (x, or the forward record) of another
position of the same shape that holds the same distinct point: with M = 1 (L8, L10) that is every position of the shape -- the
activations, z and logdet are then the same in all its tiles and only the cotangents differ -- with M = 2 (L1, L2, L6, L9 at f = 64)
every second one.  Input-side indexing within a shape is tested by the cases with M = 0 and by those with M >= 4 only (for
MB = 4 .. 6 and for grid_y > 1 that is the 64-point cases and the forward tests, not L8 and L10).
The latent rows stay distinct (identical rows make the FiLM BatchNorm degenerate)."""
import collections
import functools
import re

import numpy as np
import torch
import torch.nn.functional as F

from go_with_the_flows_amd import _lib
from go_with_the_flows_amd.synth import synth_inputs
from helpers import decoder_and_state
from oracle import torch_port as tp

MODEL_SEED = 458
G = 16
MARGIN = 1e-5           # no ReLU input of the float64 reference lies this close to 0 (tests/encoder_train_ref.py MARGIN)
MARGIN_E32 = 8.0        # ... nor within 8 x the largest float32 evaluation error of a ReLU input of the same case
DIRECT, LIGHT, MERGED = 0, 2, 3            # include/gwtf.h GWTF_BWD_PASS_*
PLAN_KEYS = ('MB', 'NB', 'MG', 'K2', 'FULL', 'tpw', 'grid_x', 'grid_y')

Case = collections.namedtuple('Case', 'L f B N M seed training mode K plan', defaults=(True, 'inverse', 1, None))
# plan: {(pass, pattern class): {key: value}} -- what gwtf_bwd_plan must return for the case; pattern class 0 = patterns 0-2 (one
# warped coordinate), 3 = patterns 3-5 (one kept coordinate, reached from L = 2 on)


def _small(f, N, seed, M=0, L=1, training=True, mode='inverse'):
    passes = (LIGHT, MERGED) if training else (DIRECT,)
    mg = 1 if training and 33 <= f <= 40 else -1
    want = dict(MB=-(-f // 16), NB=1, MG=mg, K2=-1, FULL=0, tpw=1, grid_x=3 * -(-N // 64), grid_y=1)
    return Case(L, f, 3, N, M, seed, training, mode, 1, {(pas, pat): want for pas in passes for pat in ((0, 3) if L > 1 else (0,))})


# ---- 64-point tiles (NB = 1), B = 3: the width sets the kernel, N the tile edge ---------------------------------------------------
# _small(f, N, seed[, M]): plain clouds where a seed meets the margin conditions (f = 8, 19, most eval cases); from f = 33 up the
# float32 error of the ReLU inputs is 3e-6 .. 8e-6 and 8 x that is only met with fewer distinct points, so those clouds are tiled too.
# Every seed (and M, largest first) was searched on the CPU for margin >= 20 e32: e32 differs between machines by up to 2 x.
SMALL_CASES = {
    # MB = 1: one partial tile; exactly one tile
    's_f8_n5': _small(8, 5, 3123), 's_f8_n64': _small(8, 64, 3132),
    # MB = 2 generic: one point under a tile, one over, a third tile of 2 points
    's_f19_n63': _small(19, 63, 3129), 's_f19_n65': _small(19, 65, 3100), 's_f19_n130': _small(19, 130, 3106, 32),
    # both ends of the abs-form range (MG = 1, 64-point kernel), and the first width past it (same MB = 3, generic)
    's_f33_n65': _small(33, 65, 3121, 32), 's_f40_n65': _small(40, 65, 3103, 32), 's_f41_n65': _small(41, 65, 3109, 32),
    # the abs form; patterns 3-5 at L = 2
    's_f37_n64': _small(37, 64, 3119, 32), 's_f37_n130': _small(37, 130, 3139, 32), 's_f37_n130_l2': _small(37, 130, 3136, 4, L=2),
    # MB = 4, 5, 6
    's_f64_n65': _small(64, 65, 3102, 16), 's_f65_n65': _small(65, 65, 3116, 8), 's_f96_n65': _small(96, 65, 3108, 8),
    # eval mode: the DIRECT pass, both directions
    's_f19_n130_eval_inv': _small(19, 130, 3114, training=False), 's_f19_n130_eval_dir': _small(19, 130, 3109, training=False, mode='direct'),
    's_f37_n130_eval_inv': _small(37, 130, 3122, 32, training=False), 's_f37_n130_eval_dir': _small(37, 130, 3133, training=False, mode='direct'),
}


def _abs(nb, k2, full=0, tpw=1, **kw):
    return dict(MB=3, NB=nb, MG=1, K2=k2, FULL=full, tpw=tpw, **kw)


def _gen(mb, nb, **kw):
    return dict(MB=mb, NB=nb, MG=-1, K2=-1, FULL=0, tpw=1, **kw)


# ---- 128- and 256-point tiles: tiled clouds --------------------------------------------------------------------------------------
LARGE_CASES = {
    # merged NB = 2, K2 = 1, FULL; light NB = 2
    'L1': Case(1, 37, 32, 2048, 2, 3008, plan={(MERGED, 0): _abs(2, 1, 1, grid_x=512), (LIGHT, 0): _abs(2, 1, grid_x=512)}),
    # the same without FULL: a last tile of 80 points in every shape
    'L2': Case(1, 37, 33, 2000, 2, 3015, plan={(MERGED, 0): _abs(2, 1, 0, grid_x=528), (LIGHT, 0): _abs(2, 1, grid_x=528)}),
    # (the issue's L3 -- 2, 37, 4, 16384: K2 = 0 with FULL -- is left out: no input of that shape has a float32 reference steady enough
    # for a bar of 8 err32 at factor 1, docs/LOG.md "Left out"; the merged K2 = 0 kernel runs below with its bound selects)
    # K2 = 0, a last tile of 16 points
    'L4': Case(2, 37, 4, 16400, 4, 3017, plan={(MERGED, 0): _abs(2, 1, 0, grid_x=516), (MERGED, 3): _abs(2, 0, 0, grid_x=516),
                                                 (LIGHT, 0): _abs(2, 1, grid_x=516), (LIGHT, 3): _abs(2, 0, grid_x=516)}),
    # light NB = 4, tpw = 2 with 257 tiles per shape: the last workgroup of a shape has one tile, of 64 points
    'L5': Case(1, 37, 4, 65600, 4, 3012, plan={(LIGHT, 0): _abs(4, 1, 0, 2, grid_x=4 * 129), (MERGED, 0): _abs(2, 1, 0, grid_x=4 * 513)}),
    # the abs-form edges at 128-point tiles, a last tile of 2 points
    'L6_f33': Case(1, 33, 32, 2050, 2, 3009, plan={(MERGED, 0): _abs(2, 1, 0, grid_x=544), (LIGHT, 0): _abs(2, 1, grid_x=544)}),
    'L6_f40': Case(1, 40, 32, 2050, 2, 3025, plan={(MERGED, 0): _abs(2, 1, 0, grid_x=544), (LIGHT, 0): _abs(2, 1, grid_x=544)}),
    # generic light NB = 4 (MB <= 3, tpw = 1), generic merged NB = 2
    'L7': Case(1, 19, 4, 65600, 4, 3022, plan={(LIGHT, 0): _gen(2, 4, grid_x=4 * 257), (MERGED, 0): _gen(2, 2, grid_x=4 * 513)}),
    # MB = 4 and 6 at NB = 2 (above MB = 3 the light pass stays at 128 points whatever the size)
    'L8_f64': Case(1, 64, 32, 2050, 1, 3044, plan={(MERGED, 0): _gen(4, 2, grid_x=544), (LIGHT, 0): _gen(4, 2, grid_x=544)}),
    'L8_f96': Case(1, 96, 32, 2050, 1, 3198, plan={(MERGED, 0): _gen(6, 2, grid_x=544), (LIGHT, 0): _gen(6, 2, grid_x=544)}),
    # DIRECT at NB = 2: eval mode, both directions
    'L9_f37_inv': Case(1, 37, 32, 2050, 4, 3010, False, 'inverse', plan={(DIRECT, 0): _gen(3, 2, grid_x=544)}),
    'L9_f37_dir': Case(1, 37, 32, 2050, 4, 3001, False, 'direct', plan={(DIRECT, 0): _gen(3, 2, grid_x=544)}),
    'L9_f64_inv': Case(1, 64, 32, 2050, 2, 3006, False, 'inverse', plan={(DIRECT, 0): _gen(4, 2, grid_x=544)}),
    'L9_f64_dir': Case(1, 64, 32, 2050, 2, 3019, False, 'direct', plan={(DIRECT, 0): _gen(4, 2, grid_x=544)}),
    # K = 4 through the mixture stack's train path: grid_y = 4, and the K term of the 256 Ki threshold of the large light pass
    'L10': Case(1, 37, 33, 2000, 1, 3079, K=4, plan={(LIGHT, 0): _abs(4, 1, 0, 2, grid_x=132, grid_y=4),
                                                      (MERGED, 0): _abs(2, 1, 0, grid_x=528, grid_y=4)}),
}
CASES = {**SMALL_CASES, **LARGE_CASES}
# the tile A/B of L5: the same input through the 128-point light kernel, and through the 256-point one with one tile per workgroup
TUNE_SMALL, TUNE_SINGLE = _lib.TUNE_SMALL_LIGHT_TILE, _lib.TUNE_SINGLE_TILE
L5_SMALL_PLAN = {(LIGHT, 0): _abs(2, 1, grid_x=4 * 513), (MERGED, 0): _abs(2, 1, 0, grid_x=4 * 513)}
L5_SINGLE_PLAN = {(LIGHT, 0): _abs(4, 1, 0, 1, grid_x=4 * 257), (MERGED, 0): _abs(2, 1, 0, grid_x=4 * 513)}


def bwd_plan(pas, f, B, N, K=1, pat=0, tune=0):
    """gwtf_bwd_plan (host only: nothing is launched) as a dict of PLAN_KEYS."""
    import ctypes
    out = (ctypes.c_int * 8)()
    rc = _lib.lib().gwtf_bwd_plan(pas, f, B, N, K, pat, tune, out)
    assert rc == 0, rc
    return dict(zip(PLAN_KEYS, out))


def assert_plan(name, tune=0, expect=None):
    """Every (pass, pattern class) the case runs gets the kernel variant the case is named for; grid_y = K unless the case says so."""
    c = CASES[name]
    for (pas, pat), want in (c.plan if expect is None else expect).items():
        got = bwd_plan(pas, c.f, c.B, c.N, c.K, pat, tune)
        assert got == {'grid_y': c.K, **want}, (name, pas, pat, got, want)


def tiled_cloud(B, N, M, G, seed):
    """-> p (B,3,N) float32: per shape the M points of synth_inputs(B, M, G, seed) at the positions permutation(arange(N) % M);
    g (B,G); idx (B,N) the distinct point each position holds; rng, the generator after the permutations (the cotangents follow)."""
    p0, g = synth_inputs(B, M, G, seed)
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(np.arange(N) % M) for _ in range(B)])
    p = np.take_along_axis(p0, np.broadcast_to(idx[:, None, :], (B, 3, N)), axis=2)
    return np.ascontiguousarray(p), g, idx, rng


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """Case -> (p (B,3,N), g (B,G), wz, wl (K,B,3,N)) float32 numpy: the cloud, the latents, a random-sign cotangent per position
    and component for the coordinates and for the log-determinant.  Shared by the tests; never modified."""
    if c.M:
        p, g, _, rng = tiled_cloud(c.B, c.N, c.M, G, c.seed)
    else:
        p, g = synth_inputs(c.B, c.N, G, c.seed)
        rng = np.random.default_rng(c.seed)
    wz = rng.normal(size=(c.K, c.B, 3, c.N)).astype(np.float32)
    wl = rng.normal(size=(c.K, c.B, 3, c.N)).astype(np.float32)
    return p, g, wz, wl


def case_inputs(name):
    return make_inputs(CASES[name]._replace(plan=None))


def decoders(name):
    """[(module, numpy state)] of the case's K components (fp32, on the CPU)."""
    c = CASES[name] if isinstance(name, str) else name
    return [decoder_and_state(c.L, c.f, G, MODEL_SEED + k) for k in range(c.K)]


class _Functional:
    """torch.nn.functional as oracle/torch_port sees it for the duration of one reference run: relu_ reports its input first (the
    ReLUs are in place, so the value has to be taken before the call)."""

    def __init__(self, seen):
        self._seen = seen

    def __getattr__(self, name):
        return getattr(F, name)

    def relu_(self, x):
        self._seen(x.detach())
        return F.relu_(x)


def _leaf_state(st, dtype):
    out = {}
    for k, v in st.items():
        t = torch.from_numpy(v).clone()
        t = t.to(dtype) if t.is_floating_point() else t
        out[k] = t.requires_grad_(t.is_floating_point() and not k.endswith(('running_mean', 'running_var', 'eps')))
    return out


def run_reference(states, p, g, wz, wl, n_flows, mode, training, dtype, calls=1, capture=False, against=None):
    """``calls`` differentiable passes of the K decoders ``states`` (numpy state dicts) on one cloud, in ``dtype`` on the CPU, through
    oracle/torch_port.decoder_fused.  The loss is sum_k (z_k * wz[k]).sum() + (logdet_k * wl[k]).sum().  Returns a dict of float64
    tensors: 'z', 'logdet' (K,B,3,N); 'dp', 'dg'; 'grad.<k>.<parameter>'; in train mode 'buf.<k>.<running statistic>' after the last
    call; 'relu_margin' the smallest |input| over all ReLU calls of the LAST call (12 per coupling and component).  The gradients are
    those of the last call alone.
    capture: 'relu_inputs', the list of those inputs in ``dtype``, in call order.
    against: such a list from another run -- 'relu_e' the largest |input - other| and 'relu_flips' the number of inputs whose sign
    differs, compared elementwise; the list is consumed (emptied) on the way to bound the memory."""
    K = len(states)
    tsts = [_leaf_state(st, dtype) for st in states]
    pt = torch.from_numpy(p).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(g).to(dtype).requires_grad_(True)
    wz, wl = torch.from_numpy(wz).to(dtype), torch.from_numpy(wl).to(dtype)
    stat = dict(margin=np.inf, e=0.0, flips=0, n=0)
    kept = []
    if against is not None:
        against.reverse()                                   # pop() from the end = call order

    def seen(x):
        stat['margin'] = min(stat['margin'], float(x.abs().min()))
        stat['n'] += 1
        if capture:
            kept.append(x.clone())
        if against is not None:
            other = against.pop().to(torch.float64)
            stat['e'] = max(stat['e'], float((x.to(torch.float64) - other).abs().max()))
            stat['flips'] += int(((x > 0) != (other > 0)).sum())

    real = tp.F
    tp.F = _Functional(seen)
    try:
        for call in range(calls):
            last = call == calls - 1
            for t in [pt, gt] + [v for tst in tsts for v in tst.values()]:
                t.grad = None
            stat.update(margin=np.inf, n=0)
            tp.F = _Functional(seen) if last else real    # only the last call is reported
            zs, lds, loss = [], [], 0.0
            for k, tst in enumerate(tsts):
                z, ld = tp.decoder_fused(pt, gt, tst, n_flows, mode, grad=True, training=training)
                loss = loss + (z * wz[k]).sum() + (ld * wl[k]).sum()
                zs.append(z.detach())
                lds.append(ld.detach())
            loss.backward()
            del loss, z, ld
    finally:
        tp.F = real
    assert stat['n'] == 12 * n_flows * K and not against
    out = {'z': torch.stack(zs).double(), 'logdet': torch.stack(lds).double(), 'dp': pt.grad.double(), 'dg': gt.grad.double(),
           'relu_margin': stat['margin']}
    for k, tst in enumerate(tsts):
        for n, v in tst.items():
            if v.requires_grad:
                out[f'grad.{k}.{n}'] = v.grad.double()
            elif training and n.endswith(('running_mean', 'running_var')):
                out[f'buf.{k}.{n}'] = v.detach().double()
    if capture:
        out['relu_inputs'] = kept
    if against is not None:
        out['relu_e'], out['relu_flips'] = stat['e'], stat['flips']
    return out


def compared_keys(ref):
    """The tensors a test compares: the outputs, the input gradients, every parameter gradient, every running statistic."""
    return ['z', 'logdet', 'dp', 'dg'] + [k for k in ref if k.startswith(('grad.', 'buf.'))]


def family(key):
    """'grad.0.flows.0.nvp1.T_mu_0.mu_sd1.weight' -> 'sd1.weight'; the FiLM heads' input layer, its BatchNorm and their output layer
    -> 'film0.weight', 'film0_bn.weight', 'film1.bias', ...; every other key is its own family."""
    if not key.startswith('grad.'):
        return key
    layer, kind = key.rsplit('.', 2)[-2:]
    film = re.search(r'film_[wb](\d)(_bn)?$', layer)
    layer = 'film' + film[1] + (film[2] or '') if film else layer.split('_', 1)[1]
    return f'{layer}.{kind}'


# Families whose bar is FACTOR x max(8 err32, 4e-6 scale).  Each of these gradients is one long sum of random-sign terms (over all
# points for sd2.bias and sd0.weight, over a shape's points and then through the FiLM BatchNorm for the FiLM layers) that the kernels
# accumulate with fp32 atomics in an order that changes from run to run, while the float32 CPU run happens to sum them almost exactly
# (err32 of sd2.bias is often below 1e-6 of the scale), so 8 err32 says little about an fp32 kernel there.  Measured on the first
# device runs (docs/LOG.md, "Decoder backward: float64 gradient tests"): for sd2.bias and sd0.weight the same tensor has the same
# error through the 256-, the 128- and the 64-point kernels, so it is a property of the arithmetic and not of a tile variant.  For
# film0_bn.weight, film0_bn.bias and film0.weight that was NOT shown for the same tensor: the case that missed (L4) has no other tile
# for its light pass, its cloud through the 64-point kernels was 2-3 x better, and only another cloud reached the same level at 64
# points; film1.bias missed on no committed case (0.98 at L4, 1.11 on a neighbouring input).  Each factor is at most twice the worst
# err / bar seen for the family in the first runs (in that order: 2.10, 2.06, 1.30, 1.20, 1.11, 1.05); they apply to every case, and no
# sharpness condition names the film0 families.  Every other tensor keeps factor 1.
FAMILY_FACTOR = {'sd2.bias': 4.0, 'film0_bn.weight': 4.0, 'film0_bn.bias': 2.5, 'film0.weight': 2.4, 'film1.bias': 2.0, 'sd0.weight': 2.0}


def bar(key, r64, r32):
    """The bar of one tensor, FACTOR x max(8 err32, 4e-6 scale) with FACTOR = 1 outside FAMILY_FACTOR, with its parts:
    -> (bar, err32, scale)."""
    scale = float(r64[key].abs().max())
    err32 = float((r32[key] - r64[key]).abs().max())
    return FAMILY_FACTOR.get(family(key), 1.0) * max(8.0 * err32, 4e-6 * scale), err32, scale


def run_case(name, dtype, calls=1, zero_last=False, **kw):
    c = CASES[name] if isinstance(name, str) else name
    p, g, wz, wl = make_inputs(c._replace(plan=None))
    if zero_last:                                            # the cotangents of the last point of the last shape, every component
        wz, wl = wz.copy(), wl.copy()
        wz[:, -1, :, -1] = 0.0
        wl[:, -1, :, -1] = 0.0
    return run_reference([st for _, st in decoders(name)], p, g, wz, wl, c.L, c.mode, c.training, dtype, calls, **kw)


@functools.lru_cache(maxsize=None)
def references(name, calls=1):
    """(float64 run, float32 run) of a named case; computed once, shared by the tests, never modified.  The float32 run carries
    'relu_e' and 'relu_flips': its ReLU inputs against the float64 run's, elementwise."""
    r64 = run_case(name, torch.float64, calls, capture=True)
    r32 = run_case(name, torch.float32, calls, against=r64.pop('relu_inputs'))
    return r64, r32
