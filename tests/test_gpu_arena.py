"""The host driver around the stack pipeline on the GPU: the one arena gather (flows.stacked_raw_arena), the device tables it and
StackEngine._update_running_stats keep (flows._DeviceTable), and their fallbacks when the first call falls inside a hipGraph
capture.  Smallest shapes at which this code can go wrong: n_flows = 1 (C = 3), f = 8, G = 16, clouds B = 2, N = 64.
Needs an MI355X."""
import copy

import pytest
import torch

from helpers import decoder_and_state
from go_with_the_flows_amd.dist import graph_capture
from go_with_the_flows_amd.flows import stacked_raw_arena
from go_with_the_flows_amd.mixture import MixtureStack

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
L, F, G, B, N = 1, 8, 16, 2, 64


def decoders(n, seed=60):
    return [decoder_and_state(L, F, G, seed + k)[0] for k in range(n)]


def cpu_arena(dec):
    return torch.cat([torch.zeros(op) if t is None else t.detach().reshape(-1)
                      for tr in dec.flows for c in tr.couplings() for t, op in c.raw_sources()])


def clouds(seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, N, generator=gen).to(DEV), torch.randn(B, G, generator=gen).to(DEV)


def stamp(engine):
    return sum(c._stamp for c in engine.couplings)


def test_gather_is_the_cpu_concatenation_bit_for_bit():
    """The gather is a pure copy: exact, with and without the autograd node, for one engine and for three."""
    decs = decoders(3)
    want = [cpu_arena(d) for d in decs]
    engines = [d.to(DEV).engine() for d in decs]
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            one, three = engines[0].raw_arena(), stacked_raw_arena(engines)
        assert one.requires_grad == grad and three.requires_grad == grad
        assert one.shape == want[0].shape and torch.equal(one.detach().cpu(), want[0])
        assert torch.equal(three.detach().cpu(), torch.stack(want))


def test_tables_survive_load_state_dict_and_a_no_op_apply():
    """load_state_dict copies in place and .float() on a float module replaces nothing: the stamp moves, the pointers do not, and
    the next gather and the next running-statistic update use the device tables they had."""
    dec = decoders(1)[0].to(DEV).train()
    e = dec.engine()
    p, g = clouds()
    with torch.no_grad():
        dec.forward_fused(p, g)
    gather = e._stack_tables[(id(e),)]
    tables = [gather, e._bn.ptrs, e._bn.momentum, e._bn.index]
    before = [(t.table, t.table.data_ptr()) for t in tables]
    for touch in (lambda: dec.load_state_dict(dec.state_dict()), lambda: dec.float()):
        s0 = stamp(e)
        touch()
        assert stamp(e) > s0
        with torch.no_grad():
            dec.forward_fused(p, g)
        assert e._bn.stamp == stamp(e)                              # the rows were derived again ...
        for t, (tensor, ptr) in zip(tables, before):                # ... and found equal
            assert t.table is tensor and t.table.data_ptr() == ptr
    assert torch.equal(e.raw_arena().detach().cpu(), cpu_arena(copy.deepcopy(dec).cpu()))


def rel(a, b):
    """The measure tests/test_gpu_models.py::test_graphed_train_step_equals_eager_steps compares states with."""
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / (a.abs().max() + 1e-3))


def test_first_call_inside_a_capture_takes_the_fallbacks_and_equals_eager_steps():
    """A K = 2 mixture whose first call ever is the captured one: no device table exists and none can be built (a host-to-device
    copy), so the gather is torch.cat and the running statistics move by per-module updates.  Two replays == two eager steps of a
    deep copy (the copy's first step, taken before the capture, is also what loads the kernels); the eager call that follows
    builds the tables and still agrees.  Bounds: those of test_graphed_train_step_equals_eager_steps (1e-4 relative on what the
    step returns; 2e-2 worst / 2e-4 mean relative over the tensors of the state, here gradients and BatchNorm buffers too)."""
    mods = torch.nn.ModuleList(decoders(2)).to(DEV).train()
    twin = copy.deepcopy(mods)
    fresh, ref = MixtureStack(mods), MixtureStack(twin)
    p, g = clouds()
    gen = torch.Generator().manual_seed(5)
    w_out, w_ld = torch.randn(2, B, 3, N, generator=gen).to(DEV), torch.randn(2, B, 3, N, generator=gen).to(DEV)

    def fwd_bwd(stack, module):
        for q in module.parameters():
            q.grad = None
        out, logdet = stack.forward_all(p, g, 'inverse')
        ((out * w_out).sum() + (logdet * w_ld).sum()).backward()
        return out.detach(), logdet.detach()

    def compare(got, want, steps):
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) < 1e-4 * float(b.abs().max())
        rels = []
        for (name, q), q_ref in zip(mods.named_parameters(), twin.parameters()):
            assert q.grad is not None and q_ref.grad is not None, name
            rels.append(rel(q_ref.grad, q.grad))
        for (name, b), b_ref in zip(mods.named_buffers(), twin.buffers()):
            if name.endswith('num_batches_tracked'):
                assert int(b) == int(b_ref) == steps, name
            else:
                rels.append(rel(b_ref, b))
        print('worst / mean relative difference', max(rels), sum(rels) / len(rels))
        assert max(rels) < 2e-2 and sum(rels) / len(rels) < 2e-4

    want = fwd_bwd(ref, twin)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):
        got = fwd_bwd(fresh, mods)
    e0 = fresh.engines[0]
    key = tuple(id(e) for e in fresh.engines)
    assert e0._stack_tables[key].table is None and all(e._bn.ptrs.table is None for e in fresh.engines)
    graph.replay()
    graph.replay()
    want = fwd_bwd(ref, twin)
    torch.cuda.synchronize()
    compare(got, want, 2)
    got = tuple(t.clone() for t in fwd_bwd(fresh, mods))
    want = fwd_bwd(ref, twin)
    assert e0._stack_tables[key].table is not None and all(e._bn.ptrs.table is not None for e in fresh.engines)
    compare(got, want, 3)


def test_running_statistic_update_follows_batchnorm1d_per_module():
    """One BatchNorm with momentum 0.3, one that does not track (the rows then skip a module: the `index` table): after one
    train-mode pass every buffer is (1 - m) running + m batch of the statistics the pass returned (the variance in them is the
    unbiased one), evaluated in float64.  Bound: 1e-6 of the two terms' magnitudes -- an fp32 evaluation of the rule rounds three
    times, 1.8e-7 of the larger term; a relative bound on the result itself would fail where the terms cancel."""
    dec = decoders(1, seed=70)[0].to(DEV).train()
    e = dec.engine()
    mods = e._bn_modules()
    heavy, untracked = e.couplings[1].T_mu_0[1], e.couplings[2].T_logvar_0_cond_w[1]
    heavy.momentum, untracked.track_running_stats = 0.3, False
    old = [(m.running_mean.double().clone(), m.running_var.double().clone(), int(m.num_batches_tracked)) for m in mods]
    seen = []
    update = e._update_running_stats
    e._update_running_stats = lambda bn_batch: (seen.append(bn_batch.clone()), update(bn_batch))[1]
    p, g = clouds(9)
    with torch.no_grad():
        dec.forward_fused(p, g)
    assert len(seen) == 1 and e._bn.index.table.numel() == len(mods) - 1
    batch = seen[0].double().reshape(len(mods), 2, F)
    worst = 0.0
    for i, (m, (mean0, var0, nbt0)) in enumerate(zip(mods, old)):
        if m is untracked:
            assert torch.equal(m.running_mean.double(), mean0) and torch.equal(m.running_var.double(), var0)
            assert int(m.num_batches_tracked) == nbt0
            continue
        mom = 0.3 if m is heavy else 0.1
        assert m.momentum == mom and int(m.num_batches_tracked) == nbt0 + 1
        for got, run0, stat in ((m.running_mean, mean0, batch[i, 0]), (m.running_var, var0, batch[i, 1])):
            want, scale = (1 - mom) * run0 + mom * stat, (1 - mom) * run0.abs() + mom * stat.abs()
            assert float(scale.max()) > 0
            worst = max(worst, float(((got.double() - want).abs() / scale.clamp_min(1e-30)).max()))
    print('worst error relative to the terms', worst)
    assert worst < 1e-6
