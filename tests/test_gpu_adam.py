"""Fused Adam / AMSGrad (csrc/gwtf_adam.hip, optim.Adam) against the optimiser oracle (oracle.flow_oracle.adam_step, pinned to the
reference by golden g10) run in float64, over T = 6 scheduled steps, for both kernels (up to 48 tensors in the kernel arguments,
more through the device pointer table), the C ABI's multi-launch loop, and the gradient layouts a model hands the optimiser.
Needs an MI355X.

Tolerance, elementwise after t updates of a tensor:  |x32 - x64| <= t * 4u * (|x64| + s),  u = 2^-24, s = lr for the parameters,
s = 0 for exp_avg, exp_avg_sq and max_exp_avg_sq.  Derivation (first order in u, inputs g and the initial p exact in both runs):
  * m = b1 m + (1-b1) g.  b1 and 1-b1 are rounded to fp32 (u each), each product rounds (u), the sum rounds (u): the fresh error is
    at most 3u (|b1 m| + |(1-b1) g|) = 3u |m_new| when the two terms have the same sign, plus b1 * (the error carried in m), at most
    (t-1) 4u |b1 m| <= (t-1) 4u |m_new|.  Total <= t 4u |m_new|.
  * v = b2 v + (1-b2) g g: one more product, fresh error <= 4u |v_new| (both terms >= 0: no cancellation, ever); carried as for m.
  * max_exp_avg_sq = max(vmax, v) is exact and inherits the bound of v.
  * p -= wd p + lr step, step = (m/bc1) / (sqrt(vhat)/bc2 + eps): the final subtraction and wd p round to ~2u |p|; the relative
    error of step is ~(6t+9)u (m, v, the bias corrections and the divisions), i.e. an absolute error <= (6t+9)u lr |step|, inside the
    4u lr per step the bound grants as long as |step| = O(1) and lr <= 2e-3 is small against |p|.
The premises are met by the data: every element's gradient keeps its sign over the T steps (a cancelling m = b1 m + (1-b1) g has no
relative bound in any fp32 evaluation), |p| >= 0.1 at the start.  Within them the bound has a factor of several to spare; a
wrong beta, bias correction, AMSGrad maximum or decay breaks it by orders of magnitude."""
import ctypes
import io

import numpy as np
import pytest
import torch

from helpers import decoder_and_state
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib
from go_with_the_flows_amd.optim import Adam, LRUpdater
from go_with_the_flows_amd.synth import synth_inputs
from oracle import flow_oracle as fo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
T = 6
B1 = [0.9, 0.8, 0.95, 0.85, 0.9, 0.7]                  # beta1 moves every step as well (the reference's LRUpdater fixes it)
SCHED = dict(cycle_length=1, min_lr=2e-4, max_lr=2e-3, min_beta2=0.99, max_beta2=0.999)
EPS = 1e-8
SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 7, 70001]


def schedule(opt, t, lr_scale=(1.0,)):
    """Step t (0-based) of the schedule: lr and beta2 along LRUpdater's cosine, beta1 from B1; group i's lr times lr_scale[i]."""
    LRUpdater(T, beta1=B1[t], **SCHED)(opt, 0, t)
    for grp, sc in zip(opt.param_groups, lr_scale):
        grp['lr'] *= sc


def sizes_for(n, rng):
    return SIZES + [int(x) for x in rng.integers(1, 300, size=n - len(SIZES))]


class Stream:
    """Per-element gradients of one tensor over the T steps: a fixed sign per element; magnitudes O(1), ~1e-9 (the eps regime) or
    exactly 0; 100x smaller from the third step on (so max_exp_avg_sq stays above exp_avg_sq); a few exact zeros per step."""

    def __init__(self, n, rng):
        self.rng = rng
        self.sign = rng.choice([-1.0, 1.0], size=n)
        self.mag = np.abs(rng.normal(size=n)) + 0.05
        kind = rng.uniform(size=n)
        self.mag[kind < 0.1] = 1e-9 * (1.0 + rng.uniform(size=int((kind < 0.1).sum())))
        self.mag[(kind >= 0.1) & (kind < 0.15)] = 0.0

    def at(self, t):
        n = self.sign.size
        g = self.sign * self.mag * (1.0 if t < 2 else 0.01) * (1.0 + 0.3 * self.rng.uniform(-1, 1, size=n))
        g[self.rng.uniform(size=n) < 0.03] = 0.0
        return g.astype(np.float32)


def init_param(n, rng):
    return (rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.1, 2.0, size=n)).astype(np.float32)


class Oracle:
    """float64 state of one parameter tensor, updated by fo.adam_step with the reference semantics (no gradient: no update)."""

    def __init__(self, p0):
        self.p = p0.astype(np.float64)
        self.m, self.v, self.vmax = (np.zeros_like(self.p) for _ in range(3))
        self.step = 0

    def update(self, g, grp):
        self.step += 1
        b1, b2 = grp['betas']
        self.p, self.m, self.v, self.vmax = fo.adam_step(self.p, g.astype(np.float64), self.m, self.v, self.vmax, self.step,
                                                         grp['lr'], b1, b2, grp['eps'], grp['weight_decay'], grp['amsgrad'])


def close(name, got, ref, t, s):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    err = np.abs(got - ref)
    bound = t * 4 * U * (np.abs(ref) + s)
    bad = err > bound
    assert not bad.any(), (name, t, int(bad.sum()), float(np.max(err / np.maximum(bound, 1e-300))))


def check_state(opt, p, orc, grp, tag):
    st = opt.state[p]
    assert st['step'] == orc.step, (tag, st['step'], orc.step)
    t = orc.step
    close(f'{tag} p', p.detach().cpu().numpy(), orc.p, t, grp['lr'])
    close(f'{tag} exp_avg', st['exp_avg'].cpu().numpy(), orc.m, t, 0.0)
    close(f'{tag} exp_avg_sq', st['exp_avg_sq'].cpu().numpy(), orc.v, t, 0.0)
    if grp['amsgrad']:
        close(f'{tag} max_exp_avg_sq', st['max_exp_avg_sq'].cpu().numpy(), orc.vmax, t, 0.0)


def odd_views(sizes, dev=DEV):
    """One flat float32 buffer and views of it, the i-th at an offset = 1, 2, 3 (mod 4) floats (never 16-byte aligned)."""
    offs, o = [], 0
    for i, n in enumerate(sizes):
        o += (i % 3 + 1 - o) % 4
        offs.append(o)
        o += n
    flat = torch.zeros(o + 4, device=dev)
    return flat, [flat[a:a + n] for a, n in zip(offs, sizes)], offs


@pytest.mark.parametrize('ams', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-3])
@pytest.mark.parametrize('layout', ['fresh', 'inplace', 'views', 'param_views'])
@pytest.mark.parametrize('n_tensors', [48, 49, 300])
def test_fused_adam_six_steps_vs_fp64(n_tensors, layout, wd, ams):
    """48 tensors: the argument-table kernel; 49 / 300: the device pointer table.  Gradient layouts: fresh tensors every step (the
    pointer table is re-uploaded through both pinned staging buffers in turn; one gradient transposed, i.e. non-contiguous), the same
    tensors refilled in place (no re-upload), views of one flat buffer at float offsets 1, 2, 3 (mod 4) (the unaligned 16-byte
    gradient loads), and parameters that are such views themselves (the scalar path)."""
    rng = np.random.default_rng(n_tensors * 31 + len(layout) * 7 + int(ams) + (2 if wd else 0))
    sizes = sizes_for(n_tensors, rng)
    shapes = [(n,) for n in sizes]
    tshape = (7, 13)                                    # the transposed gradient ('fresh')
    if layout == 'fresh':
        sizes[11], shapes[11] = 91, tshape
    p0 = [init_param(n, rng) for n in sizes]
    if layout == 'param_views':
        pflat, pviews, _ = odd_views(sizes)
        params = []
        for v, a, shp in zip(pviews, p0, shapes):
            v.copy_(torch.from_numpy(a))
            params.append(torch.nn.Parameter(v.view(shp)))
        assert all(q.data_ptr() % 16 for q, n in zip(params, sizes) if n)
    else:
        params = [torch.nn.Parameter(torch.from_numpy(a).reshape(shp).to(DEV)) for a, shp in zip(p0, shapes)]
    streams = [Stream(n, rng) for n in sizes]
    orcs = [Oracle(a) for a in p0]
    opt = Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=EPS, weight_decay=wd, amsgrad=ams)
    gflat = None
    if layout == 'views':
        gflat, gviews, _ = odd_views(sizes)
        for q, v in zip(params, gviews):
            q.grad = v.view(q.shape)
        assert all(q.grad.data_ptr() % 16 for q, n in zip(params, sizes) if n)
    for t in range(T):
        schedule(opt, t)
        grp = opt.param_groups[0]
        gs = [s.at(t) for s in streams]
        for i, (q, g) in enumerate(zip(params, gs)):
            if layout in ('fresh', 'param_views'):
                if layout == 'fresh' and i == 11:
                    q.grad = torch.from_numpy(g.reshape(tshape).T.copy()).to(DEV).t()
                    assert not q.grad.is_contiguous()
                else:
                    q.grad = torch.from_numpy(g).reshape(q.shape).to(DEV)
            elif layout == 'inplace':
                if q.grad is None:
                    q.grad = torch.zeros_like(q)
                q.grad.copy_(torch.from_numpy(g).reshape(q.shape))
            else:
                q.grad.copy_(torch.from_numpy(g).reshape(q.shape))
        opt.step()
        for i, (q, o, g) in enumerate(zip(params, orcs, gs)):
            o.update(g, grp)
            check_state(opt, q, o, grp, (layout, i, sizes[i]))
    plan = opt._plans[0]
    if n_tensors > 48:
        assert 'table' in plan
        if layout == 'inplace':
            assert plan['gevent'][0] is None and plan['gevent'][1] is not None     # uploaded once, never again
        elif layout in ('fresh', 'param_views'):
            assert all(e is not None for e in plan['gevent'])                     # both staging buffers in use
    else:
        assert 'table' not in plan
    if ams:
        # the gradients shrank 100x after step 2: for most elements the AMSGrad maximum is no longer exp_avg_sq
        bite = tot = 0
        for q in params:
            st = opt.state[q]
            vv, vx = st['exp_avg_sq'].cpu().numpy(), st['max_exp_avg_sq'].cpu().numpy()
            bite += int((vx > vv).sum())
            tot += int((vx > 0).sum())
        assert bite > 0.8 * tot, (bite, tot)


def test_lagging_parameter_and_two_groups():
    """Two param groups (device-table AMSGrad, lr x1, no decay / argument-table Adam, lr x3, decay 1e-3); one parameter of each group
    has no gradient at step 3: it is not touched then (no decay either) and its step count -- hence its bias corrections -- lags by
    one from then on (reference optimizers.py:33-47: `if p.grad is None: continue`, state['step'] += 1 per update)."""
    rng = np.random.default_rng(5)
    sz = [sizes_for(60, rng), [int(x) for x in rng.integers(1, 5000, size=10)]]
    p0 = [[init_param(n, rng) for n in s] for s in sz]
    params = [[torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in g] for g in p0]
    opt = Adam([dict(params=params[0], amsgrad=True, weight_decay=0.0), dict(params=params[1], amsgrad=False, weight_decay=1e-3)],
               lr=1e-3, betas=(0.9, 0.999), eps=EPS)
    streams = [[Stream(n, rng) for n in s] for s in sz]
    orcs = [[Oracle(a) for a in g] for g in p0]
    lag = {(0, 7), (1, 3)}
    for t in range(T):
        schedule(opt, t, lr_scale=(1.0, 3.0))
        gs = [[s.at(t) for s in g] for g in streams]
        for gi in range(2):
            for i, q in enumerate(params[gi]):
                q.grad = None if (t == 2 and (gi, i) in lag) else torch.from_numpy(gs[gi][i]).to(DEV)
        opt.step()
        for gi, grp in enumerate(opt.param_groups):
            for i, (q, o) in enumerate(zip(params[gi], orcs[gi])):
                if q.grad is not None:
                    o.update(gs[gi][i], grp)
                check_state(opt, q, o, grp, (gi, i, t))
    for gi, i in lag:
        assert opt.state[params[gi][i]]['step'] == T - 1


def test_state_dict_round_trip_mid_run_is_bit_equal():
    """state_dict -> (a checkpoint on the host) -> a new Adam -> load_state_dict after step 3 continues bit for bit."""
    def run(split):
        rng = np.random.default_rng(11)
        sz = [sizes_for(60, rng), [int(x) for x in rng.integers(1, 5000, size=10)]]
        params = [[torch.nn.Parameter(torch.from_numpy(init_param(n, rng)).to(DEV)) for n in s] for s in sz]
        streams = [[Stream(n, rng) for n in s] for s in sz]
        groups = lambda: [dict(params=params[0], amsgrad=True), dict(params=params[1], amsgrad=False, weight_decay=1e-3)]
        opt = Adam(groups(), lr=1e-3, betas=(0.9, 0.999), eps=EPS)
        for t in range(T):
            if t == split:
                buf = io.BytesIO()
                torch.save(opt.state_dict(), buf)
                buf.seek(0)
                opt = Adam(groups(), lr=5e-2, betas=(0.5, 0.5), eps=1.0)
                opt.load_state_dict(torch.load(buf, map_location='cpu'))
            schedule(opt, t, lr_scale=(1.0, 3.0))
            for g, ss in zip(params, streams):
                for q, s in zip(g, ss):
                    q.grad = torch.from_numpy(s.at(t)).to(DEV)
            opt.step()
        return [q.detach().cpu() for g in params for q in g], \
            [opt.state[q][k].cpu() for g in params for q in g for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') if k in opt.state[q]], \
            [opt.state[q]['step'] for g in params for q in g]

    a, b = run(None), run(3)
    assert a[2] == b[2] == [T] * len(a[2])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('ams', [0, 1])
def test_c_abi_adam_step_multi_launch(ams):
    """gwtf_adam_step called directly with ~100 tensors (three launches of at most 48; empty tensors skipped, NULL pointers there)."""
    L = _lib.lib()
    rng = np.random.default_rng(100 + ams)
    sizes = sizes_for(100, rng) + [0]
    n = len(sizes)
    p0 = [init_param(k, rng) for k in sizes]
    ps = [torch.from_numpy(a).to(DEV) for a in p0]
    ms, vs, vxs = ([torch.zeros(k, device=DEV) for k in sizes] for _ in range(3))
    streams = [Stream(k, rng) for k in sizes]
    orcs = [Oracle(a) for a in p0]
    arr = ctypes.c_void_p * n
    ptrs = lambda ts: arr(*[t.data_ptr() if t.numel() else None for t in ts])
    numel = (ctypes.c_size_t * n)(*sizes)
    for t in range(T):
        lr, b1, b2 = 1e-3 * (1 + t), B1[t], 0.999 - 0.002 * t
        grp = dict(lr=lr, betas=(b1, b2), eps=EPS, weight_decay=1e-3, amsgrad=bool(ams))
        gs = [s.at(t) for s in streams]
        gd = [torch.from_numpy(g).to(DEV) for g in gs]
        with torch.cuda.device(0):
            _lib.check(L.gwtf_adam_step(ptrs(ps), ptrs(gd), ptrs(ms), ptrs(vs), ptrs(vxs) if ams else None, numel, n,
                                        lr, b1, b2, EPS, 1e-3, t + 1, ams, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for i, o in enumerate(orcs):
            o.update(gs[i], grp)
            close(('p', i), ps[i].cpu().numpy(), o.p, o.step, lr)
            close(('m', i), ms[i].cpu().numpy(), o.m, o.step, 0.0)
            close(('v', i), vs[i].cpu().numpy(), o.v, o.step, 0.0)
            if ams:
                close(('vmax', i), vxs[i].cpu().numpy(), o.vmax, o.step, 0.0)


def test_adam_on_a_training_mixture_real_gradient_layout():
    """A 2-component train-mode mixture (decoders from tests/helpers.py, base Gaussians and logits as parameters): three steps of
    loss -> backward -> Adam.step().  Each step's gradients are copied to the host before the step and fed to the fp64 oracle; every
    parameter follows it.  The decoders' gradients are views of the flat arena gradient (flows._ArenaCatMulti), some of them at
    addresses that are not 16-byte aligned -- the layout the device-table kernel meets in training.  The model's parameters are not
    kept away from 0 and its gradients need not keep their sign: at p ~ 0 nothing hides the update's own rounding, (6t+9)u of
    lr |step|, so s = 4 lr here (module docstring); m and v are covered by the tests above."""
    L, f, G, B, N, K = 1, 19, 12, 4, 96, 2
    decs = [decoder_and_state(L, f, G, 700 + k)[0].to(DEV).train() for k in range(K)]
    rng = np.random.default_rng(3)
    mu0 = torch.nn.Parameter(torch.from_numpy(0.1 * rng.normal(size=(K, B, 3)).astype(np.float32)).to(DEV))
    lv0 = torch.nn.Parameter(torch.from_numpy(-0.5 + 0.1 * rng.normal(size=(K, B, 3)).astype(np.float32)).to(DEV))
    logits = torch.nn.Parameter(torch.from_numpy(rng.normal(size=(B, K)).astype(np.float32)).to(DEV))
    params = [q for d in decs for q in d.parameters()] + [mu0, lv0, logits]
    assert len(params) > 48
    p, g = synth_inputs(B, N, G, 4)
    pd, gd = torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV)
    orcs = [Oracle(q.detach().cpu().numpy()) for q in params]
    opt = Adam(params, lr=1e-4, betas=(0.9, 0.999), eps=EPS, weight_decay=1e-4, amsgrad=True)
    stack = gw.MixtureStack(decs)
    unaligned = 0
    for t in range(3):
        schedule(opt, t, lr_scale=(0.1,))
        grp = opt.param_groups[0]
        opt.zero_grad(set_to_none=True)
        z, ld = stack.forward_all(pd, gd, 'inverse')
        loss, _ = gw.flow_mixture_nll(z, ld, mu0, lv0, logits)
        loss.backward()
        assert all(q.grad is not None for q in params)
        unaligned += sum(1 for q in params if q.grad.data_ptr() % 16)
        snaps = [q.grad.detach().cpu().numpy().copy() for q in params]
        opt.step()
        for i, (q, o, gs) in enumerate(zip(params, orcs, snaps)):
            o.update(gs, grp)
            close(('p', i, tuple(q.shape)), q.detach().cpu().numpy(), o.p, o.step, 4 * grp['lr'])
    assert unaligned > 0
