"""The validation pass on the device: gwtf_loop_eval_commit fed directly, the eval packings refreshed in place
(models.EvalWeights), and training.ResidentEvalLoop between the replays of a ResidentTrainLoop on the same model against a fresh host
loop on a copy of that model; checkpoints through torch.save.  Needs an MI355X."""
import copy

import numpy as np
import pytest
import torch

import go_with_the_flows_amd as gw
from go_with_the_flows_amd import _lib, models, optim, training
from go_with_the_flows_amd.flows import stacked_raw_arena
from go_with_the_flows_amd.training import ResidentEvalLoop, ResidentTrainLoop
from test_gpu_loop import (AverageMeter, Harness, PLUS_INF, QUIET_NAN, SIGNALLING_NEGATIVE_NAN, TERMS, TriggerLoss, cloud_model,
                           host_meters, mesh_store, moments, record, sync_debug)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MINUS_INF = 0xff800000
B, N = 4, 48
REL = 1e-4                       # the bar test_resident_loop_equals_the_graphed_step_loop sets between two paths of this project


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------
def eval_harness(n_iters=3):
    h = Harness(B, n_iters, np.arange(n_iters * B), np.zeros((n_iters, 8)), adam_step=9)
    h.args.table = None                                     # the validation record has no schedule table
    h.ints[5:6].fill_(7)                                    # skip: a value the kernel must leave alone
    h.state.view(torch.float32)[24:32].copy_(torch.arange(1, 9, device=DEV) * 0.125)      # hyper
    return h


def untouched(rec):
    return rec.adam_step == 9 and rec.skip == 7 and list(rec.hyper) == [0.125 * i for i in range(1, 9)]


def test_eval_commit_feeds_the_meters_and_nothing_else():
    h = eval_harness()
    for i, terms in enumerate(TERMS[:3]):
        h.feed(terms)
        rec = h.call('gwtf_loop_eval_commit')
        want = host_meters(TERMS[:i + 1], B)
        assert [float(x) for x in rec.meters] == [float(x) for x in want], i          # float64 against the host AverageMeter, ==
        assert (rec.cursor, rec.status, rec.poisoned_at) == (i + 1, 0, -1) and untouched(rec)
    h.feed(TERMS[3])
    rec = h.call('gwtf_loop_eval_commit')                                            # beyond n_iters: nothing moves
    assert [float(x) for x in rec.meters] == [float(x) for x in want] and (rec.cursor, rec.status, rec.poisoned_at) == (3, 0, -1)
    assert untouched(rec)


@pytest.mark.parametrize('pattern', [QUIET_NAN, SIGNALLING_NEGATIVE_NAN, PLUS_INF, MINUS_INF],
                         ids=['quiet_nan', 'signalling_negative_nan', 'plus_inf', 'minus_inf'])
def test_eval_commit_is_poisoned_by_a_nan_or_infinite_loss(pattern):
    h = eval_harness(6)                                     # stop_on_inf = 0 in the record: eval() stops on an infinity regardless
    for terms in TERMS[:2]:
        h.feed(terms)
        h.call('gwtf_loop_eval_commit')
    want = [float(x) for x in host_meters(TERMS[:2], B)]
    for call, terms in enumerate(TERMS[2:5]):
        h.feed((pattern,) + terms[1:] if call == 0 else terms)                       # later calls: finite again, still frozen
        rec = h.call('gwtf_loop_eval_commit')
        assert rec.status == _lib.LOOP_POISONED and rec.poisoned_at == 2 and rec.cursor == 2, call
        assert [float(x) for x in rec.meters] == want and untouched(rec), call


# ---- 2. the eval packings, refreshed in place ---------------------------------------------------------------------------------------
def unpinned_packings(model):
    """What the version-keyed accessors of a fresh, unpinned copy of the model produce for its parameters."""
    ref = copy.deepcopy(model).eval()
    assert ref.eval_weights is None and ref.mixture_stack()._pinned is None          # a copy of a pinned model is not pinned
    stack = ref.mixture_stack()
    with torch.no_grad():
        pw, pf = stack.packed()
        px = stack.packed_exact()
        raw = stacked_raw_arena(stack.engines)
    nx = px.numel() - _lib.WORKLIST_INTS
    return {'raw': raw, 'packed_w': pw, 'packed_film': pf, 'packed_x': px[:nx], 'encoder_packed': ref.pc_encoder.packed()}


def pinned_packings(w):
    bufs = w.buffers()
    nx = bufs['packed_x'].numel() - _lib.WORKLIST_INTS
    out = {k: bufs[k] for k in ('raw', 'packed_w', 'packed_film', 'encoder_packed')}
    out['packed_x'] = bufs['packed_x'][:nx]                                            # the exact record without its work list
    return out


def refresh_without_a_sync(w):
    available = sync_debug('error')
    try:
        w.refresh()                                         # raises if anything in it synchronises
    finally:
        sync_debug('default')
    return available


def test_refresh_repacks_in_place_what_the_unpinned_accessors_produce():
    m, _ = cloud_model()
    w = m.pin_eval_weights()
    assert m.pin_eval_weights() is w and m.eval_weights is w
    ptrs = {k: t.data_ptr() for k, t in w.buffers().items()}
    print('sync debug mode available:', refresh_without_a_sync(w))
    want, got = unpinned_packings(m), pinned_packings(w)
    for k in want:
        assert torch.equal(got[k].reshape(-1), want[k].reshape(-1)), k
    assert not w.buffers()['packed_x'][got['packed_x'].numel():].any()                # the work list: zeroed once, still zero
    # the accessors hand the pinned buffers out, whatever the version keys say: through train() / eval() / invalidate
    stack = m.mixture_stack()
    m.eval()
    m.train()
    for mod in m.modules():
        if hasattr(mod, 'invalidate_packed_weights'):
            mod.invalidate_packed_weights()
    assert stack.packed()[0] is w.stack.pw and stack.packed()[1] is w.stack.pf and stack.packed_exact() is w.stack.px
    assert m.pc_encoder.packed() is w.encoder.packed
    e1 = m.pc_decoder[1].engine()
    n_w = w.stack.pw.numel() // stack.K
    assert e1.packed()[0].data_ptr() == w.stack.pw.data_ptr() + 4 * n_w and e1.packed_exact().numel() == w.stack.nx // stack.K
    # edits through .data move no version counter: the pinned packing is stale until refresh(), and refresh() moves no pointer
    before = {k: t.clone() for k, t in got.items()}
    c = m.pc_decoder[1].flows[0].nvp2
    versions = (c.T_mu_0[3].weight._version, c.T_logvar_0[1].running_var._version, m.pc_encoder.features[1].running_var._version)
    c.T_mu_0[3].weight.data.mul_(1.5)                                                  # a coupling weight (sd1 of the mu branch)
    c.T_logvar_0[1].running_var.data.add_(0.25)                                        # a BatchNorm running_var of a coupling
    c.T_mu_0_cond_w[1].running_var.data.add_(0.5)                                      # one of its FiLM heads
    m.pc_encoder.features[1].running_var.data.mul_(2.0)                               # and one of the cloud encoder
    assert versions == (c.T_mu_0[3].weight._version, c.T_logvar_0[1].running_var._version, m.pc_encoder.features[1].running_var._version)
    for k, t in pinned_packings(w).items():
        assert torch.equal(t, before[k]), k
    refresh_without_a_sync(w)
    want, got = unpinned_packings(m), pinned_packings(w)
    for k in want:
        assert torch.equal(got[k].reshape(-1), want[k].reshape(-1)), k
        assert not torch.equal(got[k], before[k]), k
    assert {k: t.data_ptr() for k, t in w.buffers().items()} == ptrs
    # unpinned again: the version-keyed caches are back, on fresh tensors
    m.unpin_eval_weights()
    assert m.eval_weights is None and stack.packed()[0] is not w.stack.pw and m.pc_encoder.packed() is not w.encoder.packed


# ---- 3. validation between training steps -------------------------------------------------------------------------------------------
def val_loader(store, call=0):
    loader = gw.DeviceCloudLoader(store, B, N, gw.CloudTransform(center=True), shuffle=False, seed=5)
    loader._state = gw.make_state(5, DEV, call=call)
    return loader


def host_pass(model, crit, store, call):
    """eval() on the host: a fresh eval-mode copy of the model, version-keyed packings dropped, the loader at sampler call `call`.
    -> per-batch [loss, pnll, gnll, gent] and the four float64 AverageMeters."""
    ref = copy.deepcopy(model).eval()
    for mod in ref.modules():
        if hasattr(mod, 'invalidate_packed_weights'):
            mod.invalidate_packed_weights()
    terms, meters = [], [AverageMeter() for _ in range(4)]
    with torch.no_grad():
        for batch in val_loader(store, call):
            enc, dec = ref.forward_fused(batch['cloud'], batch['eval_cloud'])
            t = crit.fused(enc, dec)
            assert not bool(torch.isnan(t[0])) and not bool(torch.isinf(t[0]))
            terms.append([x.item() for x in t])
            for meter, v in zip(meters, ((t[1] + t[2] - t[3]).item(), t[1].item(), t[2].item(), t[3].item())):
                meter.update(v, B)
    return terms, meters


def close(x, y, rel=REL):
    return abs(x - y) <= rel * abs(y)


def snapshot(model, train_loader):
    return ([b.detach().clone() for b in model.buffers()], torch.cuda.get_rng_state(torch.device(DEV)).clone(),
            train_loader._state.clone(), model.training, [mod.training for mod in model.modules()])


def assert_no_trace(model, train_loader, snap):
    buffers, rng, state, flag, flags = snap
    assert model.training == flag and [mod.training for mod in model.modules()] == flags
    assert all(torch.equal(a, b) for a, b in zip(buffers, model.buffers()))
    assert torch.equal(rng, torch.cuda.get_rng_state(torch.device(DEV))) and torch.equal(state, train_loader._state)


def test_validation_between_training_steps_sees_the_trained_weights():
    """THE case the version-keyed caches cannot serve: an eval graph captured once, replayed before and after two replays of the
    resident training loop, which writes parameters and running statistics through raw pointers."""
    store = mesh_store(4)                                   # 12 shapes: three batches
    m, cfg = cloud_model()
    crit = models.Flow_Mixture_Loss(**cfg)
    opt = optim.Adam(m.parameters(), lr=1e-3, amsgrad=True)
    train_loader = gw.DeviceCloudLoader(store, B, N, gw.CloudTransform(center=True), seed=11)
    loop = ResidentTrainLoop(m, crit, opt, train_loader)
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    snap = snapshot(m, train_loader)
    loader = val_loader(store)
    val = ResidentEvalLoop(m, crit, loader)
    assert_no_trace(m, train_loader, snap)                  # construction: flags, buffers, RNG and the train loader's state as before
    assert torch.equal(loader._state, gw.make_state(5, DEV)) and all(torch.equal(v, m.state_dict()[k]) for k, v in state0.items())
    host0, hm0 = host_pass(m, crit, store, 0)
    first = val.validate(0)
    assert_no_trace(m, train_loader, snap)
    assert int(loader._state[1]) == 3 and first['iteration'] == 3 and not first['poisoned'] and first['LB'][3] == 3 * B
    for name, meter in zip(('LB', 'PNLL', 'GNLL', 'GENT'), hm0):
        assert close(first[name][1], meter.avg) and close(first[name][0], meter.val), (name, first[name], meter.avg)
    loop.set_epoch(0)
    loop.run(2)
    snap = snapshot(m, train_loader)
    second = val.validate(0)
    assert_no_trace(m, train_loader, snap)
    host1, hm1 = host_pass(m, crit, store, 3)               # the now-trained model, the sampler calls the second pass used
    print('host LB.avg before / after two steps:', hm0[0].avg, hm1[0].avg, 'device:', first['LB'][1], second['LB'][1])
    # the host loop alone shows that two steps at this learning rate move the validation loss by more than the bar ...
    assert abs(hm1[0].avg - hm0[0].avg) > 10 * REL * abs(hm0[0].avg)
    # ... so a pass on stale weights could not pass this:
    assert second['iteration'] == 3 and not second['poisoned'] and second['poisoned_at'] == -1 and second['LB'][3] == 3 * B
    for name, meter in zip(('LB', 'PNLL', 'GNLL', 'GENT'), hm1):
        assert close(second[name][1], meter.avg) and close(second[name][0], meter.val), (name, second[name], meter.avg, meter.val)
    assert abs(second['LB'][1] - first['LB'][1]) > REL * abs(first['LB'][1])
    # batch by batch (the same pass again, by hand: the sampler set back to the calls the second pass drew)
    loader._state.copy_(gw.make_state(5, DEV, call=3))
    val.begin(0)
    got, no_sync = [], None
    for i in range(3):
        no_sync = sync_debug('error')
        try:
            val.run(1)                                      # raises if anything in it synchronises
        finally:
            sync_debug('default')
        got.append([float(t) for t in val.terms])
    print('sync debug mode available:', no_sync, 'host', host1, 'device', got)
    for a, b in zip(host1, got):
        for x, y in zip(a, b):
            assert close(y, x), (a, b)
    third = val.meters()
    for name in ('LB', 'PNLL', 'GNLL', 'GENT'):
        assert close(third[name][1], second[name][1], 1e-5), name
    # first_iteration: the reference's `iter + i >= len(iterator)` break
    part = val.validate(0, first_iteration=2)
    assert part['iteration'] == 3 and part['LB'][3] == B and int(loader._state[1]) == 7
    # and training goes on
    loop.run(1)
    assert loop.meters()['step'] == 3


def test_posterior_mean_is_deterministic():
    store = mesh_store(4)
    m, cfg = cloud_model()
    fixed = m.__dict__['reparameterize']
    loader = val_loader(store)
    val = ResidentEvalLoop(m, models.Flow_Mixture_Loss(**cfg), loader, posterior='mean')
    assert m.__dict__['reparameterize'] is fixed            # the model's own draw is back in place
    records = []
    for _ in range(2):
        loader._state.copy_(gw.make_state(5, DEV))
        res = val.validate(0)
        records.append(val.state.clone())
    assert res['iteration'] == 3 and not res['poisoned'] and res['LB'][3] == 3 * B and np.isfinite(res['LB'][1])
    assert torch.equal(records[0], records[1])
    # no draw: another noise in the model's reparameterize changes nothing
    m.reparameterize = lambda mu, logvar: mu + 100.0
    loader._state.copy_(gw.make_state(5, DEV))
    val.validate(0, warmup=True)                            # (a second batch graph, captured on first use: get_weights branches)
    loader._state.copy_(gw.make_state(5, DEV))
    val.validate(0)
    assert torch.equal(val.state, records[0])
    val.close()
    assert m.eval_weights is None
    with pytest.raises(RuntimeError, match='no longer pinned'):
        val.validate(0)


# ---- 4. a NaN loss ------------------------------------------------------------------------------------------------------------------
def test_a_nan_loss_stops_the_pass():
    store = mesh_store(4)
    m, cfg = cloud_model()
    crit = TriggerLoss(**cfg)
    crit.trigger = torch.zeros((), device=DEV)
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    val = ResidentEvalLoop(m, crit, val_loader(store))
    before = [t.detach().clone() for t in m.state_dict().values()]
    val.begin(0)
    val.run(1)
    crit.trigger.fill_(float('nan'))                        # batch 1 turns NaN
    val.run(2)
    rec = val.meters()
    assert rec['poisoned'] and rec['poisoned_at'] == 1 and rec['iteration'] == 1
    assert all(rec[k][3] == B for k in ('LB', 'PNLL', 'GNLL', 'GENT')) and np.isfinite(rec['LB'][1])      # one batch's meters
    assert training.track_best(rec, 10000) == (False, 10000)
    assert all(torch.equal(a, b) for a, b in zip(before, m.state_dict().values())) and len(opt.state) == 0
    crit.trigger.fill_(0.0)                                 # the next pass starts from a clean record
    rec = val.validate(0)
    assert not rec['poisoned'] and rec['iteration'] == 3 and rec['poisoned_at'] == -1


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work():
    import json
    import os
    from conftest import GOLDEN
    store = mesh_store(1)
    m, cfg = cloud_model()
    crit = models.Flow_Mixture_Loss(**cfg)
    svr = models.Flow_Mixture_SVR_Model(**json.load(open(os.path.join(GOLDEN, 'contract_svr.json')))['small_cfg']).to(DEV)
    images = gw.ImageStore.from_arrays(np.zeros((6, 3, 8, 8), np.uint8), views_per_shape=2, device=DEV)
    free = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='single-view reconstruction'):
        ResidentEvalLoop(svr, crit, gw.DeviceCloudLoader(store, 2, N))
    with pytest.raises(NotImplementedError, match='single-view reconstruction'):
        ResidentEvalLoop(m, crit, gw.DeviceSVRLoader(store, images, 2, N))
    with pytest.raises(ValueError, match='eval_cloud'):
        ResidentEvalLoop(m, crit, gw.DeviceCloudLoader(store, 2, N, return_eval_cloud=False))
    assert torch.cuda.memory_allocated() == free and m.eval_weights is None and m.training


# ---- 6. checkpoints -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_continues_the_resident_loop(tmp_path):
    store = mesh_store(4)
    m, cfg = cloud_model()
    crit = models.Flow_Mixture_Loss(**cfg)
    opt = optim.Adam(m.parameters(), lr=1e-4, amsgrad=True)
    up = optim.LRUpdater(3, cycle_length=2, min_lr=1.7e-5, max_lr=2.56e-4, beta1=0.9, min_beta2=0.9945, max_beta2=0.999)
    loader = gw.DeviceCloudLoader(store, B, N, gw.CloudTransform(center=True), seed=11)
    loop = ResidentTrainLoop(m, crit, opt, loader, scheduler=up)
    loop.set_epoch(0)
    loop.run(2)
    path = str(tmp_path / 'checkpoint.pth')
    training.save_checkpoint(path, m, opt, 0, 2, loop=loop)
    ck = torch.load(path, map_location='cpu')
    assert list(ck) == ['epoch', 'iter', 'model_state', 'optimizer_state'] and (ck['epoch'], ck['iter']) == (0, 2)
    # the reference's resume sequence (train_ae.py:142-147) into a fresh model and optimiser
    m2, _ = cloud_model()
    opt2 = optim.Adam(m2.parameters(), lr=1e-4, amsgrad=True)
    m2.load_state_dict(ck['model_state'])
    opt2.load_state_dict(ck['optimizer_state'])
    s1, s2 = m.state_dict(), m2.state_dict()
    assert list(s1) == list(s2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    assert len(opt2.state) == len(loop.parameters) and all(st['step'] == 2 for st in opt2.state.values())
    assert all(torch.equal(a, b) for a, b in zip(moments(opt), moments(opt2)))
    loop2 = ResidentTrainLoop(m2, crit, opt2, gw.DeviceCloudLoader(store, B, N, gw.CloudTransform(center=True), seed=11), scheduler=up)
    loop2.set_epoch(ck['epoch'], ck['iter'])
    loop2.run(1)
    rec = loop2.meters()
    assert rec['step'] == 3 and rec['iteration'] == 3 and not rec['poisoned'] and rec['LB'][3] == B and np.isfinite(rec['LB'][1])
    assert all(opt2.state[p]['step'] == 3 for p in loop2.parameters)
    assert record(loop2.state).adam_step == 3
