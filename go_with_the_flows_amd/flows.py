"""Conditional affine couplings of the discrete point flow, MI355X-native.

Same constructor signatures, attribute names, ``state_dict`` keys and ``forward(p, g, mode)``
contract as the reference's ``lib/networks/flows.py`` (``CondRealNVPFlow3D`` :10-117,
``CondRealNVPFlow3DTriple`` :120-160).  The sub-modules below only HOLD parameters and
BatchNorm buffers under the reference's names; they are never called.  All arithmetic runs in
hand-written HIP kernels (``csrc/``) through the C ABI in ``include/gwtf.h``: one weight-pack
launch (cached while parameters are unchanged), one FiLM launch, one fused stack launch.
There is no torch/CPU fallback: tensors must live on a HIP device.
"""
import operator
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .layers import SharedDot, Swish

_VERSION = operator.attrgetter('_version')

# Points whose coordinates leave the split-f16 contraction's operand range (|x| > 3e4, csrc/gwtf_layout.h GWTF_X_LIMIT) are flagged
# NaN by the stack kernel; the eval-mode density / list paths follow every stack launch with the exact-fp32 re-run launch
# (csrc/gwtf_stack_exact.hip: tiles without a flagged point leave at once, ~2 us), so such points come back with the
# reference's finite values (reference flows.py:113-115 has no range limit).  GWTF_NO_RANGE_RERUN=1 switches it off (NaN as in
# rounds 1-4).  The sampling partition (MixtureStack.forward_partition: base samples, |z| of a few units, latency-bound at one
# shape per call) and the train pipeline do not re-run.
import os as _os


def range_rerun():
    return _os.environ.get('GWTF_NO_RANGE_RERUN') != '1'

# index -> warped coordinates; couplings of a decoder cycle through these (reference flows.py:129-148)
WARP_PATTERNS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2))


def _sharded():
    """dist.sharded(): BatchNorm statistics are summed over the ranks of torch.distributed's default group."""
    from .dist import sharded
    return sharded()


def _graph_capture(graph):
    from .dist import graph_capture
    return graph_capture(graph)


def _film_head(X, which, f, G):
    n = f'{X}_sd1_film_{which}'
    return nn.Sequential(OrderedDict([
        (n + '0', nn.Linear(G, f, bias=False)),
        (n + '0_bn', nn.BatchNorm1d(f)),
        (n + '0_swish', Swish()),
        (n + '1', nn.Linear(f, f, bias=True)),
    ]))


class CondRealNVPFlow3D(nn.Module):
    """One elementary coupling: kept coordinates -> (mu, logvar) of the warped ones, conditioned on g."""

    def __init__(self, f_n_features, g_n_features, weight_std=0.01, warp_inds=[0],
                 centered_translation=False, eps=1e-6):
        super().__init__()
        self.f_n_features, self.g_n_features = f_n_features, g_n_features
        self.weight_std = weight_std
        self.warp_inds = list(warp_inds)
        if tuple(self.warp_inds) not in WARP_PATTERNS:
            raise ValueError(f'warp_inds {warp_inds} is not one of {WARP_PATTERNS}')
        self.keep_inds = [d for d in (0, 1, 2) if d not in self.warp_inds]
        self.centered_translation = centered_translation  # stored, never used (as in the reference)
        self.register_buffer('eps', torch.tensor([eps], dtype=torch.float32))
        self._eps_value = float(eps)
        f, G, k, w = f_n_features, g_n_features, len(self.keep_inds), len(self.warp_inds)
        for X in ('mu', 'logvar'):
            setattr(self, f'T_{X}_0', nn.Sequential(OrderedDict([
                (f'{X}_sd0', SharedDot(k, f, 1)),
                (f'{X}_sd0_bn', nn.BatchNorm1d(f)),
                (f'{X}_sd0_relu', nn.ReLU(inplace=True)),
                (f'{X}_sd1', SharedDot(f, f, 1)),
                (f'{X}_sd1_bn', nn.BatchNorm1d(f, affine=False)),
            ])))
            setattr(self, f'T_{X}_0_cond_w', _film_head(X, 'w', f, G))
            setattr(self, f'T_{X}_0_cond_b', _film_head(X, 'b', f, G))
            setattr(self, f'T_{X}_1', nn.Sequential(OrderedDict([
                (f'{X}_sd1_relu', nn.ReLU(inplace=True)),
                (f'{X}_sd2', SharedDot(f, w, 1, bias=True)),
            ])))
            # near-identity start: last layers ~ N(0, weight_std), zero bias (reference flows.py:52-58,87-93)
            with torch.no_grad():
                for head in (getattr(self, f'T_{X}_0_cond_w')[-1], getattr(self, f'T_{X}_0_cond_b')[-1],
                             getattr(self, f'T_{X}_1')[-1]):
                    head.weight.normal_(std=weight_std)
                    head.bias.zero_()
        self._engine = None
        self._stamp = 0

    # -- parameter gathering -------------------------------------------------------------------
    def raw_sources(self):
        """This coupling's record of the raw arena as (tensor, op) pairs in the order fixed by csrc/gwtf_layout.h;
        op: None = flatten as is, int n = n zeros (padding of the absent kept / warped slot)."""
        out = []
        k, w = len(self.keep_inds), len(self.warp_inds)
        f = self.f_n_features
        for X in ('logvar', 'mu'):
            t0 = getattr(self, f'T_{X}_0')
            sd0, bn0, sd1, bn1 = t0[0], t0[1], t0[3], t0[4]
            out += [(sd0.weight, None)] + ([(None, f)] if k < 2 else [])
            out += [(bn0.weight, None), (bn0.bias, None), (bn0.running_mean, None), (bn0.running_var, None),
                    (sd1.weight, None), (bn1.running_mean, None), (bn1.running_var, None)]
            for which in ('w', 'b'):
                head = getattr(self, f'T_{X}_0_cond_{which}')
                out += [(head[0].weight, None), (head[1].weight, None), (head[1].bias, None),
                        (head[1].running_mean, None), (head[1].running_var, None), (head[3].weight, None),
                        (head[3].bias, None)]
            sd2 = getattr(self, f'T_{X}_1')[1]
            out += [(sd2.weight, None)] + ([(None, f)] if w < 2 else [])
            out += [(sd2.bias, None)] + ([(None, 1)] if w < 2 else [])
        return out

    def raw_tensors(self):
        """Flattened tensors of this coupling's raw-arena record (see raw_sources)."""
        dev = self.eps.device
        return [torch.zeros(op, device=dev) if t is None else t.reshape(-1)
                for t, op in self.raw_sources()]

    def tracked_tensors(self):
        """Every tensor whose in-place modification must invalidate the packed-weight cache."""
        return [t for t in list(self.parameters()) + list(self.buffers()) if t.dtype == torch.float32]

    # -- packed-weight cache invalidation ---------------------------------------------------------
    # The reference optimiser writes through ``p.data`` (lib/networks/optimizers.py:69-72), which does
    # not bump tensor version counters, so besides versions the cache is keyed on a stamp bumped by
    # everything a training script does between two eval forwards: train()/eval(), .to()/.cuda(),
    # load_state_dict().  Call ``invalidate_packed_weights()`` after any other out-of-band edit.
    def invalidate_packed_weights(self):
        self._stamp = getattr(self, '_stamp', 0) + 1

    def train(self, mode=True):
        self.invalidate_packed_weights()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_packed_weights()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self.invalidate_packed_weights()
        if prefix + 'eps' in state_dict:
            self._eps_value = float(state_dict[prefix + 'eps'].reshape(-1)[0])

    def forward(self, p, g, mode='direct'):
        """-> (p_out, mu, logvar), each (B,3,N); reference flows.py:95-117."""
        if self._engine is None:
            self._engine = StackEngine([self])
        ps, mus, lvs = self._engine.run_lists(p, g, mode)
        return ps[0], mus[0], lvs[0]


class CondRealNVPFlow3DTriple(nn.Module):
    """Three couplings warping [0],[1],[2] (pattern 0) or [0,1],[0,2],[1,2] (pattern 1)."""

    def __init__(self, f_n_features, g_n_features, weight_std=0.02, pattern=0, centered_translation=False):
        super().__init__()
        if pattern not in (0, 1):
            raise ValueError(f'pattern must be 0 or 1, got {pattern}')
        self.f_n_features, self.g_n_features = f_n_features, g_n_features
        self.weight_std, self.pattern, self.centered_translation = weight_std, pattern, centered_translation
        for j in range(3):
            setattr(self, f'nvp{j + 1}', CondRealNVPFlow3D(
                f_n_features, g_n_features, weight_std=weight_std, warp_inds=list(WARP_PATTERNS[3 * pattern + j]),
                centered_translation=centered_translation))
        self._engine = None

    def couplings(self):
        return [self.nvp1, self.nvp2, self.nvp3]

    def forward(self, p, g, mode='direct'):
        """-> ([p1,p2,p3], [mu1..3], [logvar1..3]) in nvp1..3 order for both modes; reference flows.py:150-160."""
        if self._engine is None:
            self._engine = StackEngine(self.couplings())
        return self._engine.run_lists(p, g, mode)


class _DeviceTable:
    """Rows on the host, their table on the device.  The device tensor is kept while the rows are equal: building it is a
    host-to-device copy, which is not allowed while a hipGraph is captured."""

    def __init__(self):
        self.source = None                # what the owner derived `rows` from (compared by identity before deriving them again)
        self.rows, self.table = None, None

    def lookup(self, rows, device, dtype=torch.int64):
        """The device tensor of `rows`: the cached one (the same object) while they are equal, else a new one -- or None while
        the current stream is capturing: the caller takes its fallback, and the next call outside a capture builds the table."""
        if self.table is None or self.table.device != device or (rows is not self.rows and rows != self.rows):
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                return None
            self.table = torch.tensor(rows, dtype=dtype).to(device)
        self.rows = rows
        return self.table


def _needs_grad(p, g, engines):
    """Whether a pass over these engines has to be differentiable (buffers never require grad: the cached tracked tensors
    answer as the modules' parameters() would)."""
    return torch.is_grad_enabled() and (p.requires_grad or g.requires_grad or
                                        any(t.requires_grad for e in engines for t in e._tracked or e._collect()))


def exact_record(stack, rerun=True):
    """stack.packed_exact() where the launch takes it -- for the re-run of out-of-range tiles (range_rerun; rerun=False: a path
    that does not re-run) or because the exact body is forced -- else None."""
    return stack.packed_exact() if ((rerun and range_rerun()) or _lib.EXACT[0]) else None


class _ArenaCatMulti(torch.autograd.Function):
    """The raw arenas of K engines of one shape as ONE (K, R) tensor and ONE autograd node: forward is ONE pointer-table launch
    over cached detached views (a mixture's K decoders: instead of K gathers and a torch.stack), backward hands every parameter
    its slice of the flat gradient (views, no kernels)."""

    @staticmethod
    def forward(ctx, engines, *tensors):
        ctx.engines = engines
        return _gather_stacked(engines)

    @staticmethod
    def backward(ctx, g_raw):
        grads = []
        for k, eng in enumerate(ctx.engines):
            pieces = g_raw[k].split_with_sizes(eng._sizes)
            for (t, op), piece in zip(eng._srcs, pieces):
                if t is not None:
                    grads.append(piece.view(t.shape) if t.requires_grad else None)
        return (None, *grads)


def _gather_stacked(engines):
    """(K, R) stacked raw arena from the engines' cached detached views (refreshed by the caller): one pointer-table kernel
    (csrc/gwtf_train.hip) on a HIP device -- torch.cat would be a launch per 128 inputs, eleven for an 11-Triple decoder.  The
    device table is rebuilt only when a source pointer changed (not inside a hipGraph capture: torch.cat stands in there)."""
    flats = [e._flat for e in engines]
    dev = flats[0][0].device
    if dev.type != 'cuda':
        return torch.stack([torch.cat(flat) for flat in flats])
    # the combined table lives on the first engine (it dies with the model: a module-level cache keyed on id() would keep the
    # detached parameter views and the device table of every model ever built alive)
    tab = engines[0]._stack_tables.setdefault(tuple(id(e) for e in engines), _DeviceTable())
    R = sum(engines[0]._sizes)
    rows = tab.rows
    if tab.source is None or any(x is not y for x, y in zip(tab.source, flats)):   # a flat list is rebuilt with its tensors
        rows = []
        for k, e in enumerate(engines):
            off = k * R
            for t, n in zip(e._flat, e._sizes):
                rows.append((t.data_ptr(), off, n))
                off += n
    table = tab.lookup(rows, dev)
    if table is None:
        return torch.stack([torch.cat(flat) for flat in flats])
    tab.source = flats                    # tab.rows describe these lists
    out = torch.empty(len(engines), R, device=dev, dtype=torch.float32)
    return _lib.gather_table(table, out, len(rows))


def stacked_raw_arena(engines):
    """(K, R): the raw arenas of K same-shaped engines, differentiable w.r.t. every parameter (one autograd node)."""
    engines = list(engines)
    for e in engines:
        e._refresh_flat()
    srcs = [t for e in engines for t, _ in e._srcs if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in srcs):
        return _ArenaCatMulti.apply(engines, *srcs)
    return _gather_stacked(engines)


class _BnTables:
    """What StackEngine._update_running_stats keeps between calls: the rows of the tracked BatchNorm modules (derived per
    stamp) and their device tables."""

    def __init__(self):
        self.stamp, self.n_mods, self.touched = None, 0, []     # touched: the buffers the update writes
        self.ptr_rows, self.mom_rows, self.idx_rows = [], [], []  # per tracked module: buffer pointers, momentum, index in bn_batch
        self.ptrs, self.momentum, self.index = _DeviceTable(), _DeviceTable(), _DeviceTable()


class StackEngine:
    """Host-side driver of the HIP path for a run of consecutive couplings (direct order).

    Gathers the couplings' parameters into the raw arena, packs them (cached until a parameter or
    buffer changes), runs the FiLM kernel and the fused stack kernel."""

    def __init__(self, couplings):
        self.couplings = list(couplings)
        c0 = self.couplings[0]
        self.C = len(self.couplings)
        self.f, self.G = c0.f_n_features, c0.g_n_features
        pats = [WARP_PATTERNS.index(tuple(c.warp_inds)) for c in self.couplings]
        self.pattern0 = pats[0]
        if any(pt != (self.pattern0 + i) % 6 for i, pt in enumerate(pats)):
            raise ValueError(f'couplings do not follow the cyclic warp pattern: {pats}')
        if self.f > 128:
            raise NotImplementedError(f'f_n_features={self.f} > 128 is not supported by the gfx950 kernels '
                                      '(reference configs use <= 64; the forward kernels reach 128, train / backward 96)')
        self._tracked, self._tracked_stamp = [], None
        self._srcs, self._src_stamp, self._zeros = None, None, None
        self._cache_key = None
        self._packed, self._packed_x = None, None
        self._flat_key, self._flat = None, None
        self._stack_tables = {}           # engine tuple -> _DeviceTable of the gathers this engine leads (_gather_stacked)
        self._bn = _BnTables()
        # (pw, pf, px): this engine's slices of a pinned mixture packing (mixture.PinnedStackWeights) -- while set, packed() and
        # packed_exact() hand these out whatever the version keys say; whoever pinned them refreshes them in place
        self._pinned = None

    def __reduce__(self):
        """copy.deepcopy / pickle of a module that owns an engine: a FRESH engine over the (copied) couplings.  Every cache in
        here -- detached views of the parameters, device pointer tables, packed weights -- describes the original's tensors; a
        field-by-field copy would keep reading them (a deep copy of a model taken after it ran would ignore its own weights)."""
        return (StackEngine, (self.couplings,))

    def raw_arena(self):
        """Parameters + BatchNorm buffers of all couplings as one flat tensor (autograd-aware: stacked_raw_arena of this engine
        alone, as a view -- a select would add a zero-filled (1, R) gradient and a copy to the backward)."""
        return stacked_raw_arena([self]).view(-1)

    def _refresh_flat(self):
        """(Re)build the cached source list and its detached flat views.  The list of sources is cached (module traversal costs
        more than the copy); it is rebuilt when .to()/.cuda()/load_state_dict() re-create tensors (stamp change)."""
        stamp = sum(c._stamp for c in self.couplings)
        if stamp != self._src_stamp:
            self._srcs = [so for c in self.couplings for so in c.raw_sources()]
            dev = self.couplings[0].eps.device
            # (the padding tensors are kept while the device is: their pointers are rows of the gather table)
            kept = {n: z for n, z in (self._zeros or {}).items() if z.device == dev}
            self._zeros = {n: kept[n] if n in kept else torch.zeros(n, device=dev) for n in {op for t, op in self._srcs if t is None}}
            self._src_stamp = stamp
            self._flat_key = None
        # The 1320 flattened views (11-Triple decoder) are cached as DETACHED views: building them costs more host time
        # than the copy.  They must not carry autograd history -- a cached differentiable view of a parameter that the
        # optimiser then updates in place gets an AsStridedBackward grad_fn (new_zeros + copy per parameter, measured:
        # +2000 kernels per step).  The autograd link is one custom node instead (_ArenaCatMulti above).
        if self._flat_key is None:
            z = self._zeros
            self._flat = [z[op] if t is None else t.detach().view(-1) for t, op in self._srcs]
            self._sizes = [op if t is None else t.numel() for t, op in self._srcs]
            self._flat_key = True

    def _collect(self):
        self._key()
        return self._tracked

    def _key(self):
        stamp = sum(c._stamp for c in self.couplings)
        if stamp != self._tracked_stamp:  # buffers are re-created by .to()/.cuda(): re-collect
            self._tracked = [t for c in self.couplings for t in c.tracked_tensors()]
            self._tracked_stamp = stamp
        return (stamp, sum(map(_VERSION, self._tracked)))

    def packed(self):
        """The eval packing (running statistics folded) of the current parameters, cached until one of them changes.  Pinned
        (mixture.PinnedStackWeights): the pinned buffers, as of their last refresh()."""
        if self._pinned is not None:
            return self._pinned[0], self._pinned[1]
        key = self._key()
        if key != self._cache_key:
            with torch.no_grad():
                raw = self.raw_arena()
                self._packed = _lib.pack_weights(raw, self.C, self.f, self.G, False, self.pattern0)
            self._cache_key = key
            self._packed_x = None
        return self._packed

    def packed_exact(self):
        """The exact-fp32 operand record of the CURRENT eval packing (cached with it).  Pinned: this engine's part of the pinned
        record, without a work list of its own (that one sits behind all K parts: the re-run of a single engine scans its tiles)."""
        if self._pinned is not None:
            return self._pinned[2]
        pw, pf = self.packed()
        if self._packed_x is None:
            with torch.no_grad():
                self._packed_x = _lib.pack_weights_exact(self.raw_arena(), pf, self.C, self.f, self.G, self.pattern0)
        return self._packed_x

    def _check(self, p, g):
        if p.dim() != 3 or p.shape[1] != 3:
            raise ValueError(f'p must be (B,3,N), got {tuple(p.shape)}')
        if g.dim() != 2 or g.shape[0] != p.shape[0] or g.shape[1] != self.G:
            raise ValueError(f'g must be ({p.shape[0]},{self.G}), got {tuple(g.shape)}')
        dev = self.couplings[0].eps.device
        if dev.type != 'cuda':
            raise _lib.GwtfError('module parameters are on the CPU: move the module to a HIP device (.cuda()); '
                                 'go_with_the_flows_amd has no CPU path')
        if p.device != dev or g.device != dev:
            raise _lib.GwtfError(f'p ({p.device}) / g ({g.device}) must be on the module device {dev}')

    def run(self, p, g, mode, want_lists):
        if mode not in ('direct', 'inverse'):
            raise ValueError(f"mode must be 'direct' or 'inverse', got {mode!r}")
        self._check(p, g)
        c0 = self.couplings[0]
        if p.shape[2] == 0:
            # an empty cloud (the sampling draw of flow_mixture.py:153 gave this component no point): the reference's torch ops
            # pass empty tensors through; no launch here
            B = p.shape[0]
            lists = p.new_zeros(3, self.C, B, 3, 0, dtype=torch.float32) if want_lists else None
            return p.new_zeros(B, 3, 0, dtype=torch.float32), p.new_zeros(B, 3, 0, dtype=torch.float32), lists
        needs_grad = _needs_grad(p, g, [self])
        if (needs_grad or c0.training) and self.f > 96:
            raise NotImplementedError(f'f_n_features={self.f}: train-mode BatchNorm and the backward pass are built for widths up to '
                                      '96 (their LDS working set exceeds 160 KiB beyond); eval-mode forward works up to 128')
        if c0.training:
            # batch-statistic BatchNorm, with or without autograd, one rank or several: the fused pipeline (autograd.py
            # TrainMixtureFn; several ranks all-reduce one packed statistic per phase, as SyncBatchNorm does, train_ae.py:152)
            from .autograd import train_density_forward_multi
            out, logdet, lists, bn_batch = train_density_forward_multi([self], p, g, mode, distributed=_sharded(), want_lists=want_lists)
            self._update_running_stats(bn_batch[0])
            return out[0], logdet[0], tuple(t[0] for t in lists) if want_lists else None
        if needs_grad:
            # differentiable density pass: HIP forward + HIP backward (autograd.py); every ps[j] / logvars[j] list entry is
            # differentiable as in the reference (decoders.py:61-79); a gradient through a mus[j] entry raises
            from .autograd import density_forward
            return density_forward(self, p, g, mode)
        pw, film, eps = self._film(g.contiguous().float())
        return _lib.stack_forward(p.contiguous().float(), pw, film, self.C, self.f, self.pattern0, eps, mode, want_lists,
                                  packed_x=exact_record(self))

    def _film(self, g):
        """-> (packed stack weights, FiLM record of g, eps): what a stack launch on the current eval packing takes."""
        pw, pf = self.packed()
        eps = self.couplings[0]._eps_value
        return pw, _lib.film_forward(g, pf, self.C, self.f, eps), eps

    # -- train mode: batch-statistic BatchNorm ----------------------------------------------------------
    def _bn_modules(self):
        """The 8 BatchNorm modules of every coupling in bn_batch order: [coupling][branch lv,mu][kind 0..3]."""
        mods = []
        for c in self.couplings:
            for X in ('logvar', 'mu'):
                t0 = getattr(c, f'T_{X}_0')
                mods += [t0[1], t0[4], getattr(c, f'T_{X}_0_cond_w')[1], getattr(c, f'T_{X}_0_cond_b')[1]]
        return mods

    def _update_running_stats(self, bn_batch):
        """running = (1-m)*running + m*batch with the unbiased batch variance (torch.nn.BatchNorm1d semantics)."""
        bn = self._bn
        stamp = sum(c._stamp for c in self.couplings)
        if bn.stamp != stamp:
            # (re)derive the rows; the device tables are rebuilt only when a pointer really changed (load_state_dict copies in
            # place and keeps them), because building them is a host-to-device copy -- not allowed while a hipGraph is captured
            mods = self._bn_modules()
            ptr_rows, mom_rows, idx_rows, touched = [], [], [], []
            for i, m in enumerate(mods):
                if m.track_running_stats and m.running_mean is not None:
                    if m.momentum is None:
                        raise NotImplementedError('BatchNorm momentum=None (cumulative average) is not supported by the fused '
                                                  'running-statistic update; the reference never sets it (flows.py:27-42)')
                    nbt = m.num_batches_tracked
                    idx_rows.append(i)
                    mom_rows.append(float(m.momentum))
                    ptr_rows.append((m.running_mean.data_ptr(), m.running_var.data_ptr(), nbt.data_ptr() if nbt is not None else 0))
                    touched += [m.running_mean, m.running_var] + ([nbt] if nbt is not None else [])
            bn.stamp, bn.n_mods, bn.touched = stamp, len(mods), touched
            bn.ptr_rows, bn.mom_rows, bn.idx_rows = ptr_rows, mom_rows, idx_rows
        if not bn.idx_rows:
            return
        dev = bn_batch.device
        table, momentum, index = (bn.ptrs.lookup(bn.ptr_rows, dev), bn.momentum.lookup(bn.mom_rows, dev, torch.float32),
                                  bn.index.lookup(bn.idx_rows, dev))
        with torch.no_grad():
            flat = bn_batch.reshape(bn.n_mods, 2, self.f)
            if table is None or momentum is None or index is None:
                # no device table can be built inside a capture (host-to-device copy): this capture takes plain per-module
                # updates; the next call outside a capture builds the tables
                mods = self._bn_modules()
                for i, mom in zip(bn.idx_rows, bn.mom_rows):
                    mods[i].running_mean.mul_(1.0 - mom).add_(flat[i, 0], alpha=mom)
                    mods[i].running_var.mul_(1.0 - mom).add_(flat[i, 1], alpha=mom)
                    if mods[i].num_batches_tracked is not None:
                        mods[i].num_batches_tracked.add_(1)
                return
            if len(bn.idx_rows) < bn.n_mods:
                flat = flat.index_select(0, index)
            flat = flat.contiguous()
            with torch.cuda.device(flat.device):
                _lib.check(_lib.lib().gwtf_bn_running_update(table.data_ptr(), _lib._ptr(flat, 'bn_batch'), _lib._ptr(momentum, 'momentum'),
                                                            table.shape[0], self.f, _lib._stream(flat)))
            torch._C._increment_version(bn.touched)      # written through raw pointers: the packed-weight caches key on versions

    def capture(self, p, g, mode, want_lists=False):
        """hipGraph capture of (FiLM + fused stack) on the CURRENT packed weights and on the storage of ``p``/``g``.

        Returns a ``GraphedStack``: ``replay()`` re-runs both kernels with one graph launch and returns the SAME
        output tensors every time (static buffers: consume them before the next replay; refill ``p``/``g`` in
        place to change inputs).  Eval mode only; re-capture after any parameter change."""
        if mode not in ('direct', 'inverse'):
            raise ValueError(f"mode must be 'direct' or 'inverse', got {mode!r}")
        self._check(p, g)
        if self.couplings[0].training:
            raise NotImplementedError('graph capture is an inference feature: call .eval() first')
        if not (p.is_contiguous() and g.is_contiguous() and p.dtype == torch.float32 and g.dtype == torch.float32):
            raise ValueError('capture needs contiguous float32 p and g (their storage is baked into the graph)')
        return GraphedStack([self], p, g, mode, want_lists)

    def run_lists(self, p, g, mode):
        _, _, lists = self.run(p, g, mode, True)
        return list(lists[0].unbind(0)), list(lists[1].unbind(0)), list(lists[2].unbind(0))


class GraphedStack:
    """One hipGraph holding the FiLM + stack launches of one or more engines (e.g. the K mixture components)
    that read the same ``p``/``g`` storage.  Removes the per-launch host work (Python, ctypes, allocator) from
    the step: two kernels of 10-200 us each are otherwise host-bound on small batches."""

    def __init__(self, engines, p, g, mode, want_lists=False, per_engine_p=None):
        self.engines = list(engines)
        self.p, self.g, self.mode = p, g, mode
        packs = [e.packed() for e in self.engines]
        pxs = [exact_record(e) for e in self.engines]
        ps = per_engine_p if per_engine_p is not None else [p] * len(self.engines)

        def body():
            res = []
            for e, px, pk in zip(self.engines, pxs, ps):
                pw, film, eps = e._film(g)
                res.append(_lib.stack_forward(pk, pw, film, e.C, e.f, e.pattern0, eps, mode, want_lists, packed_x=px))
            return res

        side = torch.cuda.Stream(device=p.device)
        side.wait_stream(torch.cuda.current_stream(p.device))
        with torch.cuda.stream(side), torch.no_grad():
            body()                                   # warm-up outside capture (lazy module loading etc.)
        torch.cuda.current_stream(p.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with _graph_capture(self.graph), torch.no_grad():
            self.results = body()
        self._keepalive = (packs, pxs)

    def replay(self):
        self.graph.replay()
        return self.results
