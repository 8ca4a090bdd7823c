"""The resident training loop on the GPU: the device-driven Adam launch against the host-driven one bit for bit, the loop-state
kernels (gwtf_loop_begin / _commit) fed directly, and training.ResidentTrainLoop -- one graph replay per iteration -- against
GraphedTrainStep + DeviceCloudLoader / DeviceSVRLoader + LRUpdater + Adam.step().  Needs an MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, GOLDEN
from images_ref import SVR_CFG
from test_gpu_adam import SIZES, odd_views
import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models, optim
from go_with_the_flows_amd.synth import load_image_encoder_stats_, load_synth_
from go_with_the_flows_amd.training import GraphedTrainStep, ResidentTrainLoop

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCHEDULE = dict(cycle_length=2, min_lr=1.7e-5, max_lr=2.56e-4, beta1=0.9, min_beta2=0.9945, max_beta2=0.999)


def record(state):
    return _lib.LoopState.from_buffer_copy(state.cpu().numpy().tobytes())


# ---- 1. the device-driven optimiser launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ams', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-3])
def test_device_driven_adam_equals_host_driven_adam_bit_for_bit(ams, wd):
    """Same tensors, same gradients (unaligned views of one flat buffer), T = 6 scheduled steps: one copy through Adam.step() with
    LRUpdater editing param_groups, the other through gwtf_adam_step_table_dev reading LRUpdater.table rows from device memory.  The
    same expression on the same scalars, elementwise: any difference is a bug.  Then skip = 1: not a byte moves."""
    T, L = 6, _lib.lib()
    sizes = SIZES + [int(x) for x in np.random.default_rng(5).integers(1, 300, size=40)]
    gen = torch.Generator(device=DEV).manual_seed(17)
    host_p = [torch.randn(n, device=DEV, generator=gen) for n in sizes]
    dev_p = [p.clone() for p in host_p]
    gflat, gviews, _ = odd_views(sizes)
    for p, g in zip(host_p, gviews):
        p.grad = g
    opt = optim.Adam(host_p, lr=1e-3, eps=1e-8, weight_decay=wd, amsgrad=ams)
    up = optim.LRUpdater(4, **SCHEDULE)
    table = torch.from_numpy(np.concatenate([up.table(0, 1, 3, 1), up.table(1, 0, 3, 4)])).to(DEV)      # epoch 0 from iter 1, epoch 1
    where = [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2)]
    m, v, vm = ([torch.zeros_like(p) for p in dev_p] for _ in range(3))
    chunk = L.gwtf_adam_chunk_elems()
    ptab = torch.tensor([[p.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr() if ams else 0, p.numel()]
                         for p, a, b, c in zip(dev_p, m, v, vm)], dtype=torch.int64).to(DEV)
    cmap = torch.tensor([(i, c) for i, p in enumerate(dev_p) for c in range((p.numel() + chunk - 1) // chunk)],
                        dtype=torch.int32).reshape(-1, 2).to(DEV)
    gtab = torch.tensor([g.data_ptr() for g in gviews], dtype=torch.int64).to(DEV)
    skip = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch(row):
        _lib.check(L.gwtf_adam_step_table_dev(ptab.data_ptr(), gtab.data_ptr(), cmap.data_ptr(), cmap.shape[0], table[row].data_ptr(),
                                              skip.data_ptr(), 1e-8, wd, int(ams), torch.cuda.current_stream().cuda_stream))

    for t in range(T):
        gflat.copy_(torch.randn(gflat.shape, device=DEV, generator=gen) * 10.0 ** (t - 3))
        up(opt, *where[t])
        opt.step()
        launch(t)
        for i, p in enumerate(host_p):
            st = opt.state[p]
            assert st['step'] == t + 1
            assert torch.equal(p, dev_p[i]) and torch.equal(st['exp_avg'], m[i]) and torch.equal(st['exp_avg_sq'], v[i]), (t, i, sizes[i])
            if ams:
                assert torch.equal(st['max_exp_avg_sq'], vm[i]), (t, i, sizes[i])
    before = [[x.clone() for x in xs] for xs in (dev_p, m, v, vm)]
    skip.fill_(1)
    launch(T - 1)
    for xs, saved in zip((dev_p, m, v, vm), before):
        for a, b in zip(xs, saved):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 2. the loop-state kernels, fed directly ----------------------------------------------------------------------------------------
class Harness:
    """One GwtfLoopState and the buffers the launches name, driven by hand."""

    def __init__(self, B, n_iters, plan, table, views=1, stop_on_inf=False, adam_step=0):
        self.state = torch.zeros(20, dtype=torch.int64, device=DEV)
        self.ints = self.state.view(torch.int32)[32:40]
        self.ints.copy_(torch.tensor([0, n_iters, adam_step, 0, -1, 0, 0, 0], dtype=torch.int32))
        self.plan = torch.from_numpy(np.asarray(plan, np.int32)).to(DEV)
        self.rows = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.mesh_rows = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.table = torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(DEV)
        self.terms = [torch.zeros(1, device=DEV) for _ in range(4)]
        self.args = _lib.LoopArgs(state=self.state.data_ptr(), plan=self.plan.data_ptr(), rows=self.rows.data_ptr(),
                                  mesh_rows=self.mesh_rows.data_ptr(), table=self.table.data_ptr(), B=B, views=views,
                                  plan_len=self.plan.numel(), table_rows=self.table.shape[0], stop_on_inf=int(stop_on_inf), use_flag=0,
                                  stream=torch.cuda.current_stream().cuda_stream)
        self.args.terms[:] = [t.data_ptr() for t in self.terms]

    def call(self, name):
        _lib.check(getattr(_lib.lib(), name)(ctypes.addressof(self.args)))
        return record(self.state)

    def feed(self, values):
        """values: four floats, or (bits,) int for a term given by its bit pattern."""
        for t, x in zip(self.terms, values):
            if isinstance(x, int):
                t.view(torch.int32).fill_(x - (1 << 32) if x >= 1 << 31 else x)
            else:
                t.fill_(float(np.float32(x)))


def test_begin_copies_the_plan_rows_and_stops_at_the_end_of_the_epoch():
    B, views = 4, 3
    plan = np.random.RandomState(3).permutation(3 * B + 1) * 5 + 2                # 3 B + 1 entries: three whole batches
    h = Harness(B, 3, plan, np.zeros((3, 8)), views=views)
    for cursor in range(3):
        h.ints[0:1].fill_(cursor)
        h.ints[5:6].fill_(0)
        rec = h.call('gwtf_loop_begin')
        want = plan[cursor * B:(cursor + 1) * B]
        assert np.array_equal(h.rows.cpu().numpy(), want) and np.array_equal(h.mesh_rows.cpu().numpy(), want // views)
        assert (rec.cursor, rec.status, rec.skip) == (cursor, 0, 0)
    h.ints[0:1].fill_(3)
    rec = h.call('gwtf_loop_begin')
    assert rec.status == _lib.LOOP_EXHAUSTED and rec.skip == 1 and rec.cursor == 3
    want = plan[2 * B:3 * B]                                                      # unchanged: still valid indices
    assert np.array_equal(h.rows.cpu().numpy(), want) and np.array_equal(h.mesh_rows.cpu().numpy(), want // views)
    # a poisoned state is not advanced either, and a cursor set back clears the exhausted bit
    h.ints[0:1].fill_(1)
    rec = h.call('gwtf_loop_begin')
    assert rec.status == 0 and np.array_equal(h.rows.cpu().numpy(), plan[B:2 * B])
    h.ints[3:4].fill_(_lib.LOOP_POISONED)
    h.ints[0:1].fill_(0)
    h.ints[5:6].fill_(0)
    rec = h.call('gwtf_loop_begin')
    assert rec.status == _lib.LOOP_POISONED and rec.skip == 1 and np.array_equal(h.rows.cpu().numpy(), plan[B:2 * B])


class AverageMeter:
    """lib/networks/utils.py AverageMeter."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


TERMS = [(3.25, 2.7182817, 0.61803, 0.0833333), (1e-3, 123.456, -7.5, 2.0000002), (-4.0, 1e7, 0.3333333, 1e-7),
         (0.1, 0.2, 0.3, 0.4), (5.0, -1.25, 1e-5, 77.0), (2.0, 16777217.0, 1.0, -3.0)]
QUIET_NAN, SIGNALLING_NEGATIVE_NAN, PLUS_INF = 0x7fc00000, 0xff800001, 0x7f800000


def host_meters(sets, B):
    meters = [AverageMeter() for _ in range(4)]
    for _, pnll, gnll, gent in sets:
        p, g, e = np.float32(pnll), np.float32(gnll), np.float32(gent)
        for m, v in zip(meters, (np.float32(p + g) - e, p, g, e)):
            m.update(float(v), B)
    return [x for m in meters for x in (m.val, m.sum, m.count)]


def test_commit_feeds_the_meters_and_the_schedule_row():
    B = 4
    table = optim.LRUpdater(6, **SCHEDULE).table(1, 0, 6, 10)
    h = Harness(B, 6, np.arange(6 * B), table, adam_step=9)
    for i, terms in enumerate(TERMS):
        h.feed(terms)
        rec = h.call('gwtf_loop_commit')
        want = host_meters(TERMS[:i + 1], B)
        assert [float(x) for x in rec.meters] == [float(x) for x in want], i          # float64, bit for bit
        assert np.array_equal(np.asarray(list(rec.hyper), np.float32).view(np.uint32), table[i].view(np.uint32))
        assert (rec.cursor, rec.adam_step, rec.status, rec.skip, rec.poisoned_at) == (i + 1, 10 + i, 0, 0, -1)
    rec = h.call('gwtf_loop_commit')                                                  # beyond the epoch: nothing moves but skip
    assert rec.skip == 1 and (rec.cursor, rec.adam_step) == (6, 15) and [float(x) for x in rec.meters] == [float(x) for x in want]


@pytest.mark.parametrize('pattern', [QUIET_NAN, SIGNALLING_NEGATIVE_NAN], ids=['quiet', 'signalling_negative'])
def test_commit_is_poisoned_by_a_nan_loss_whatever_its_bits(pattern):
    B = 4
    table = optim.LRUpdater(6, **SCHEDULE).table(0, 0, 6, 1)
    h = Harness(B, 6, np.arange(6 * B), table)
    for terms in TERMS[:3]:
        h.feed(terms)
        after3 = h.call('gwtf_loop_commit')
    frozen = (list(after3.meters), list(after3.hyper), 3, 3)
    for call, terms in enumerate(TERMS[3:], 4):
        h.feed((pattern,) + terms[1:] if call == 4 else terms)                         # calls 5 and 6: finite again, still frozen
        rec = h.call('gwtf_loop_commit')
        assert rec.status == _lib.LOOP_POISONED and rec.poisoned_at == 3 and rec.skip == 1, call
        assert (list(rec.meters), list(rec.hyper), rec.cursor, rec.adam_step) == frozen, call


def test_commit_takes_an_infinite_loss_only_with_stop_on_inf():
    B = 4
    table = optim.LRUpdater(2, **SCHEDULE).table(0, 0, 2, 1)
    for stop_on_inf in (False, True):
        h = Harness(B, 2, np.arange(2 * B), table, stop_on_inf=stop_on_inf)
        h.feed((PLUS_INF, 1.0, 2.0, 3.0))
        rec = h.call('gwtf_loop_commit')
        if stop_on_inf:
            assert (rec.status, rec.poisoned_at, rec.cursor, rec.adam_step, rec.skip) == (_lib.LOOP_POISONED, 0, 0, 0, 1)
        else:
            assert (rec.status, rec.poisoned_at, rec.cursor, rec.adam_step, rec.skip) == (0, -1, 1, 1, 0)
        # the detect / use_flag pair of data-parallel runs reaches the same verdict
        h2 = Harness(B, 2, np.arange(2 * B), table, stop_on_inf=stop_on_inf)
        h2.args.use_flag = 1
        h2.feed((PLUS_INF, 1.0, 2.0, 3.0))
        assert h2.call('gwtf_loop_detect').flag == int(stop_on_inf)
        assert h2.call('gwtf_loop_commit').status == rec.status
        h2.feed((QUIET_NAN, 1.0, 2.0, 3.0))
        assert h2.call('gwtf_loop_detect').flag == 1


# ---- 3. the whole loop ------------------------------------------------------------------------------------------------------------
def mesh_store(copies):
    """The three meshes of golden g22_clouds, `copies` times over."""
    D = golden('g22_clouds')
    v, f = D['vertices_c'], D['faces_vc']
    vb, fb = D['vertices_c_bounds'].astype(np.int64), D['faces_bounds'].astype(np.int64)
    vbs = np.concatenate([vb[:1]] + [vb[1:] + k * len(v) for k in range(copies)])
    fbs = np.concatenate([fb[:1]] + [fb[1:] + k * len(f) for k in range(copies)])
    return gw.MeshStore.from_arrays(np.tile(v, (copies, 1)), np.tile(f, (copies, 1)), vbs, fbs, np.tile(D['orig_c'], (copies, 1)),
                                    np.tile(D['orig_s'], copies), device=DEV)


def cloud_model():
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_model.json')))['cfg']
    m = models.Flow_Mixture_Model(**cfg)
    load_synth_(m, 1310)
    m = m.to(DEV).train()
    noise = torch.from_numpy(golden('g13_full_model')['noise_g']).to(DEV)
    m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
    return m, cfg


def moments(opt):
    return [t for p in opt.param_groups[0]['params'] for k, t in sorted(opt.state[p].items()) if torch.is_tensor(t)]


def close_state(s0, s1):
    """tests/test_gpu_svr_fused.py's rule for two runs whose batch statistics are summed with float atomics."""
    rel = [float((s0[k].float() - s1[k].float()).abs().max() / (s0[k].float().abs().max() + 1e-3)) for k in s0]
    print('max rel', max(rel), 'mean rel', sum(rel) / len(rel))
    assert max(rel) < 2e-2 and sum(rel) / len(rel) < 2e-4


def sync_debug(mode):
    try:
        torch.cuda.set_sync_debug_mode(mode)
        return True
    except Exception as e:                                  # a build without the mode: that one assertion is skipped
        print('set_sync_debug_mode refused:', e)
        return False


def test_resident_loop_equals_the_graphed_step_loop():
    B, N, steps = 4, 48, 3
    store = mesh_store(4)                                   # 12 shapes: three iterations
    transform = gw.CloudTransform(center=True)
    up = optim.LRUpdater(3, **SCHEDULE)
    # the loop the pieces allow today
    m0, cfg = cloud_model()
    crit = models.Flow_Mixture_Loss(**cfg)
    opt0 = optim.Adam(m0.parameters(), lr=1e-4, amsgrad=True)
    loader0 = gw.DeviceCloudLoader(store, B, N, transform, seed=11)
    step = GraphedTrainStep(m0, crit, opt0, torch.rand(B, 3, N, device=DEV), torch.rand(B, 3, N, device=DEV))
    base = []
    for i, batch in enumerate(loader0):
        up(opt0, 0, i)
        base.append([float(t) for t in step(batch['cloud'], batch['eval_cloud'])])
    assert len(base) == steps
    # the resident loop
    m1, _ = cloud_model()
    opt1 = optim.Adam(m1.parameters(), lr=1e-4, amsgrad=True)
    loader1 = gw.DeviceCloudLoader(store, B, N, transform, seed=11)
    before = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    rng_before = torch.cuda.get_rng_state(torch.device(DEV)).clone()
    loop = ResidentTrainLoop(m1, crit, opt1, loader1, scheduler=up)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(v, m1.state_dict()[k]), k
    assert torch.equal(rng_before, torch.cuda.get_rng_state(torch.device(DEV)))
    assert torch.equal(loader1._state, gw.make_state(11, DEV))
    # moments exist from construction on, as zeros at step 0 -- for the parameters the loop updates: the model carries one that receives
    # no gradient on the fused path, which Adam.step() leaves without state too
    updated = {id(p) for p in loop.parameters}
    left_out = [p for p in m1.parameters() if id(p) not in updated]
    assert len(left_out) == 1 and len(opt1.state.get(left_out[0], {})) == 0
    assert all(opt1.state[p]['step'] == 0 and not opt1.state[p]['exp_avg'].any() for p in loop.parameters)
    loop.set_epoch(0)
    got, no_sync = [], None
    for i in range(steps):
        no_sync = sync_debug('error')
        try:
            loop.run(1)                                     # raises if anything in it synchronises
        finally:
            sync_debug('default')
        got.append([float(t) for t in loop.terms])
    print('sync debug mode available:', no_sync, 'graphed', base, 'resident', got)
    for a, b in zip(base, got):
        for x, y in zip(a, b):
            assert abs(x - y) <= 1e-4 * abs(x), (a, b)
    rec = loop.meters()
    assert rec['step'] == 3 and rec['iteration'] == 3 and not rec['poisoned'] and rec['poisoned_at'] == -1
    assert all(opt1.state[p]['step'] == 3 for p in loop.parameters)
    assert rec['LB'][3] == rec['GENT'][3] == 3 * B and abs(rec['PNLL'][0] - got[-1][1]) <= 1e-6 * abs(got[-1][1])
    assert abs(rec['GNLL'][1] - np.mean([g[2] for g in got])) <= 1e-5 * abs(rec['GNLL'][1])
    s0, s1 = m0.state_dict(), m1.state_dict()
    tracked = [k for k in s1 if k.endswith('num_batches_tracked')]
    # three batches each; p_prior's BatchNorms count one per mixture component and batch, as the reference's loop over the components
    # does (models._base_gaussian_repeated)
    want = {k: 3 * (cfg['n_components'] if k.startswith('p_prior.') else 1) for k in tracked}
    counts = {k: (int(s0[k]), int(s1[k])) for k in tracked}
    assert tracked and all(counts[k] == (want[k], want[k]) for k in tracked), {k: v for k, v in counts.items() if v != (want[k],) * 2}
    assert torch.equal(loader1._state, loader0._state) and int(loader1._state[1]) == 3          # the sampler's call counter
    close_state(s0, s1)
    close_state({i: t for i, t in enumerate(moments(opt0))}, {i: t for i, t in enumerate(moments(opt1))})
    # the record is the reference's optimiser state: it loads, and a new loop goes on from its step count
    opt2 = optim.Adam(m1.parameters(), lr=1e-4, amsgrad=True)
    opt2.load_state_dict(opt1.state_dict())
    loop2 = ResidentTrainLoop(m1, crit, opt2, loader1, scheduler=up)
    loop2.set_epoch(1)
    if sync_debug('error'):
        try:
            loop2.run(3)
        finally:
            sync_debug('default')
    else:
        loop2.run(3)
    rec2 = loop2.meters()
    assert rec2['step'] == 6 and rec2['iteration'] == 3 and rec2['LB'][3] == 3 * B and not rec2['poisoned']
    assert np.isfinite(rec2['LB'][1])
    # replays beyond the end of the epoch: no-ops for parameters and moments
    snap = [t.clone() for t in list(m1.parameters()) + moments(opt2)]
    loop2.run(2)
    rec3 = loop2.meters()
    assert rec3['exhausted'] and rec3['step'] == 6 and rec3['iteration'] == 3
    assert all(torch.equal(a, b) for a, b in zip(snap, list(m1.parameters()) + moments(opt2)))


class TriggerLoss(models.Flow_Mixture_Loss):
    """The loss VALUE is poisoned, not the data: gradients stay finite, no NaN enters any kernel but the commit."""

    def fused(self, output_prior, dec):
        loss, pnll, gnll, gent = super().fused(output_prior, dec)
        return loss + self.trigger, pnll, gnll, gent


def test_a_nan_loss_stops_the_loop_without_updating_the_net():
    B, N = 4, 48
    m, cfg = cloud_model()
    crit = TriggerLoss(**cfg)
    crit.trigger = torch.zeros((), device=DEV)
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    loop = ResidentTrainLoop(m, crit, opt, gw.DeviceCloudLoader(mesh_store(8), B, N, gw.CloudTransform(center=True), seed=2),
                             scheduler=optim.LRUpdater(6, **SCHEDULE))
    loop.set_epoch(0)
    loop.run(2)
    snap = [t.clone() for t in list(m.parameters()) + moments(opt)]
    start = [t.clone() for t in snap]
    crit.trigger.fill_(float('nan'))
    loop.run(3)
    rec = loop.meters()
    assert rec['poisoned'] and rec['poisoned_at'] == 2 and rec['step'] == 2 and rec['iteration'] == 2 and rec['LB'][3] == 2 * B
    assert all(torch.equal(a, b) for a, b in zip(snap, list(m.parameters()) + moments(opt)))
    assert all(bool(torch.isfinite(p.grad).all()) for p in loop.parameters)
    assert any(bool(t.any()) for t in start[len(list(m.parameters())):])              # two real updates did happen


def test_replays_beyond_the_epoch_change_nothing():
    B, N = 4, 48
    m, cfg = cloud_model()
    opt = optim.Adam(m.parameters(), lr=1e-4)
    loop = ResidentTrainLoop(m, models.Flow_Mixture_Loss(**cfg), opt, gw.DeviceCloudLoader(mesh_store(3), B, N, seed=4))     # no scheduler
    assert loop.n_iters == 2
    loop.set_epoch(0)
    loop.run(2)
    snap = [t.clone() for t in list(m.parameters()) + moments(opt)]
    loop.run(2)                                             # run(4) == run(2)
    rec = loop.meters(reset=True)
    assert rec['exhausted'] and rec['step'] == 2 and rec['iteration'] == 2 and rec['PNLL'][3] == 2 * B
    assert all(torch.equal(a, b) for a, b in zip(snap, list(m.parameters()) + moments(opt)))
    assert loop.meters()['PNLL'] == (0.0, 0.0, 0.0, 0.0)


def test_resident_svr_loop_equals_the_graphed_step_loop():
    D = golden('g21_svr')
    cfg = json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']
    views, B, N, steps = 2, 4, 48, 2
    meshes = mesh_store(2)                                  # 6 shapes x 2 views: three iterations
    src = np.random.RandomState(7).randint(0, 256, (6 * views, 3, 20, 20)).astype(np.uint8)
    imgs = gw.ImageStore.from_arrays(src, views_per_shape=views, device=DEV)
    it = gw.ImageTransform.from_config(channels=3, **dict(SVR_CFG, image_size=[64, 64]))
    noise = torch.from_numpy(D['noise_g']).float().to(DEV)
    up = optim.LRUpdater(3, **SCHEDULE)

    def build():
        m = models.Flow_Mixture_SVR_Model(**cfg)
        load_synth_(m, 2110)
        load_image_encoder_stats_(m, {k[len('svr_stat.'):]: D[k] for k in D.files if k.startswith('svr_stat.')})
        m = m.to(DEV).train()
        m.img_encoder.train_norm = 'hip'
        m.reparameterize = lambda mu, logvar: noise * torch.exp(0.5 * logvar) + mu
        return m, optim.Adam(m.parameters(), lr=1e-4), gw.DeviceSVRLoader(meshes, imgs, B, N, gw.CloudTransform(center=True), it, seed=9)

    crit = models.Flow_Mixture_Loss(**cfg)
    m0, opt0, loader0 = build()
    step = GraphedTrainStep(m0, crit, opt0, torch.rand(B, 3, N, device=DEV), torch.rand(B, 3, N, device=DEV),
                            images_example=torch.rand(B, 4, 64, 64, device=DEV))
    base = []
    for i, batch in zip(range(steps), loader0):
        up(opt0, 0, i)
        base.append([float(t) for t in step(batch['cloud'], batch['eval_cloud'], batch['image'])])
    m1, opt1, loader1 = build()
    loop = ResidentTrainLoop(m1, crit, opt1, loader1, scheduler=up)
    loop.set_epoch(0)
    plan = loader1.index_plan()
    got = []
    for i in range(steps):
        loop.run(1)
        got.append([float(t) for t in loop.terms])
        items = plan[i * B:(i + 1) * B]
        assert np.array_equal(loop.rows.cpu().numpy(), items) and np.array_equal(loop.mesh_rows.cpu().numpy(), items // views)
    print('graphed', base, 'resident', got)
    for a, b in zip(base, got):
        for x, y in zip(a, b):
            assert abs(x - y) <= 1e-4 * abs(x), (a, b)
    rec = loop.meters()
    assert rec['step'] == 2 and rec['iteration'] == 2 and not rec['poisoned']
    with pytest.raises(gw.GwtfError, match='host-resident ImageStore'):
        host = gw.ImageStore.from_arrays(src, views_per_shape=views, device='cpu')
        ResidentTrainLoop(m1, crit, opt1, gw.DeviceSVRLoader(meshes, host, B, N, gw.CloudTransform(center=True), it, seed=9))
