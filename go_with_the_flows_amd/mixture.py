"""K flow components as one launch + the fused mixture NLL.

The reference loops over ``self.pc_decoder[i]`` in Python (lib/networks/flow_mixture.py:163-166: K sequential
decoders on the SAME points when training; the N points split among the components by a multinomial draw when
sampling, :146-177) and then over B x K in ``FlowMixtureNLL`` (lib/networks/losses.py:109-131).  Here the K
components' packed weights are concatenated, one FiLM launch covers all K*C couplings, one stack launch covers
all components, and one reduction kernel produces the per-shape NLL.
"""
import torch

from . import _lib
from .flows import _needs_grad, _sharded, exact_record


class PinnedStackWeights:
    """Everything the eval density pass of a ``MixtureStack`` reads in packed form, in PERSISTENT device buffers: the (K, R) raw
    arena, the K * C couplings' stack and FiLM packings, the exact-fp32 record with its work list behind it (zeroed once).

    ``refresh()`` re-gathers the arena from the parameters and BatchNorm buffers (one pointer-table launch over all K engines) and
    re-packs it into the same storage (gwtf_pack_weights_k and gwtf_pack_weights_exact with K stacks in one call each): three
    launches, no allocation, no host-to-device copy, no look at a version counter -- so it can be captured in a hipGraph and replayed
    between training steps that change parameters through raw pointers.  While ``stack.pin(self)`` holds, ``stack.packed()`` /
    ``packed_exact()`` and the engines' return these buffers (the engines' as views of their K-th part).

    The pointer table describes the storage the parameters have NOW: ``.to()`` / ``.cuda()`` / a module swap (SyncBatchNorm
    conversion) need a new set.  In-place edits -- optimiser steps, ``load_state_dict``, running-statistic updates -- need a refresh."""

    def __init__(self, stack):
        L = _lib.lib()
        engines = stack.engines
        K, C, f, G = stack.K, stack.C, stack.f, stack.G
        for e in engines:
            e._refresh_flat()
        dev = engines[0]._flat[0].device
        if dev.type != 'cuda':
            raise _lib.GwtfError('module parameters are on the CPU: packed weights live on a HIP device only (.cuda() the model first)')
        R = C * L.gwtf_raw_coupling_floats(f, G)
        rows = []
        for k, e in enumerate(engines):
            if sum(e._sizes) != R:
                raise _lib.GwtfError(f'raw arena of component {k} has {sum(e._sizes)} floats, expected {R}')
            off = k * R
            for t, n in zip(e._flat, e._sizes):
                if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                    raise _lib.GwtfError('pinned eval weights need contiguous float32 parameters and buffers on one HIP device')
                rows.append((t.data_ptr(), off, n))
                off += n
        self._sources = [e._flat for e in engines]          # (the detached views, padding zeros included: the table's pointers)
        self.K, self.C, self.f, self.G, self.pattern0, self.n_rows = K, C, f, G, engines[0].pattern0, len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        new = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        self.raw = new(K * R).view(K, R)
        self.pw, self.pf = new(K * C * L.gwtf_packed_w_coupling_floats(f)), new(K * C * L.gwtf_packed_film_coupling_floats(f, G))
        self.nx = K * C * L.gwtf_packed_x_coupling_floats(f)
        self.px = torch.zeros(self.nx + _lib.WORKLIST_INTS, device=dev, dtype=torch.float32)      # records | work list (stays zero)

    def __reduce__(self):
        """copy.deepcopy / pickle of a pinned model: the copy is not pinned (these buffers describe the original's storage)."""
        return (type(None), ())

    def refresh(self):
        """Gather + pack the current parameters into the same storage: three launches on the current stream, nothing else."""
        _lib.gather_table(self.table, self.raw, self.n_rows)
        _lib.pack_weights(self.raw, self.C, self.f, self.G, False, self.pattern0, K=self.K, out=(self.pw, self.pf))
        _lib.pack_weights_exact(self.raw, self.pf, self.C, self.f, self.G, self.pattern0, K=self.K, out=self.px)
        return self

    def buffers(self):
        return {'raw': self.raw, 'packed_w': self.pw, 'packed_film': self.pf, 'packed_x': self.px}

    def engine_views(self, k):
        """(pw, pf, px) of component k: views into the K-stack buffers."""
        part = lambda t, n: t[k * (n // self.K):(k + 1) * (n // self.K)]
        return part(self.pw, self.pw.numel()), part(self.pf, self.pf.numel()), part(self.px, self.nx)


class MixtureStack:
    """Batched driver for an ``nn.ModuleList`` of ``LocalCondRNVPDecoder`` with identical (n_flows, f, G)."""

    def __init__(self, decoders):
        self.decoders = list(decoders)
        self.engines = [d.engine() for d in self.decoders]
        e0 = self.engines[0]
        if any((e.C, e.f, e.G, e.pattern0) != (e0.C, e0.f, e0.G, e0.pattern0) for e in self.engines):
            raise ValueError('all mixture components must share n_flows, f_n_features and g_n_features')
        self.K, self.C, self.f, self.G = len(self.engines), e0.C, e0.f, e0.G
        # concatenated packings, keyed on the engines' own (cached) tensors, which are kept alive beside them
        self._cat_key, self._cat, self._keep = None, None, None
        self._catx_key, self._catx, self._keepx = None, None, None
        self._route_work = {}             # (S, n, K, P, device) -> routing scratch
        self._pinned = None               # a PinnedStackWeights: packed() / packed_exact() return its buffers while it is set

    def __reduce__(self):
        """copy.deepcopy / pickle: a fresh stack over the (copied) decoders -- the caches here belong to the original's tensors."""
        return (MixtureStack, (self.decoders,))

    def pin(self, pinned=None):
        """Pin this stack (and its engines) to a ``PinnedStackWeights`` -- a new, refreshed one by default -- and return it: from now
        on the packings read are that set's buffers, kept through train() / eval() / invalidate_packed_weights() and changed only by
        its refresh().  ``unpin()`` restores the version-keyed caches."""
        pinned = PinnedStackWeights(self).refresh() if pinned is None else pinned
        self._pinned = pinned
        for k, e in enumerate(self.engines):
            e._pinned = pinned.engine_views(k)
        return pinned

    def unpin(self):
        self._pinned = None
        for e in self.engines:
            e._pinned = None

    def packed(self):
        if self._pinned is not None:
            return self._pinned.pw, self._pinned.pf
        packs = [e.packed() for e in self.engines]
        key = tuple(id(pk[0]) for pk in packs)
        if key != self._cat_key:
            self._cat = (torch.cat([pk[0] for pk in packs]), torch.cat([pk[1] for pk in packs]))
            self._cat_key, self._keep = key, packs
        return self._cat

    def packed_exact(self):
        """The K components' exact-fp32 operand records, concatenated (re-run of out-of-range tiles, flows.range_rerun)."""
        if self._pinned is not None:
            return self._pinned.px
        self.packed()
        pxs = [e.packed_exact() for e in self.engines]
        key = tuple(id(x) for x in pxs)
        if key != self._catx_key:
            # (each engine's record carries its own work list behind it, _lib.pack_weights_exact: the K record parts, then ONE list)
            n = self.C * _lib.lib().gwtf_packed_x_coupling_floats(self.f)
            tail = torch.zeros(_lib.WORKLIST_INTS, device=pxs[0].device, dtype=torch.float32)
            self._catx, self._catx_key, self._keepx = torch.cat([x[:n] for x in pxs] + [tail]), key, pxs
        return self._catx

    def _film(self, g):
        pw, pf = self.packed()
        eps = self.engines[0].couplings[0]._eps_value
        return pw, _lib.film_forward(g, pf, self.K * self.C, self.f, eps), eps

    def _film_k(self, gk):
        """_film from a (K, R, G) code table: component k's couplings are conditioned on gk[k] (one launch, gwtf_film_forward_k)."""
        if gk.dim() != 3 or gk.shape[0] != self.K or gk.shape[2] != self.G:
            raise _lib.GwtfError(f'the code table must be (K={self.K}, R, G={self.G}), got {tuple(gk.shape)}')
        pw, pf = self.packed()
        eps = self.engines[0].couplings[0]._eps_value
        return pw, _lib.film_forward_k(gk, pf, self.C, self.f, eps), eps

    def forward_all(self, p, g, mode='inverse'):
        """Every component on every point -> (out, logdet), each (K,B,3,N).  Training / density path."""
        e0 = self.engines[0]
        e0._check(p, g)
        needs_grad = _needs_grad(p, g, self.engines)
        if e0.couplings[0].training:
            # batch-statistic BatchNorm: all K components through every kernel of the train pipeline together
            # (csrc/gwtf_train.hip, K-batched pipeline); data-parallel runs all-reduce one packed statistic per phase
            from .autograd import train_density_forward_multi
            with torch.set_grad_enabled(needs_grad):
                out, logdet, _, bn_batch = train_density_forward_multi(self.engines, p, g, mode, distributed=_sharded(), want_lists=False)
            for k, e in enumerate(self.engines):
                e._update_running_stats(bn_batch[k])
            return out, logdet
        if needs_grad:
            # eval BatchNorm with autograd: the per-component differentiable path
            res = [e.run(p, g, mode, False) for e in self.engines]
            return torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])
        pw, film, eps = self._film(g.contiguous().float())
        return _lib.stack_forward_multi(p.contiguous().float(), pw, film, self.K, self.C, self.f, e0.pattern0, eps, mode,
                                        packed_x=exact_record(self))

    def forward_all_lists(self, p, g, mode='inverse', defer_running_stats=False):
        """Every component on every point, train-mode BatchNorm, WITH the reference's per-coupling lists: -> (out, logdet (K,B,3,N),
        (ps, mus, logvars) each (K, C, B, 3, N) direct-ordered; ps / logvars differentiable in every slot, a gradient through mus
        raises) -- the K list-API decoder calls of flow_mixture.py:163-166 as ONE pass of the K-batched pipeline.  None when that
        pipeline does not apply (eval-mode BatchNorm): the caller then takes the per-decoder route.
        defer_running_stats: return bn_batch (K, ...) as a fourth value instead of updating the BatchNorm buffers here."""
        e0 = self.engines[0]
        e0._check(p, g)
        if not e0.couplings[0].training:
            return None
        from .autograd import train_density_forward_multi
        needs_grad = _needs_grad(p, g, self.engines)
        with torch.set_grad_enabled(needs_grad):
            out, logdet, lists, bn_batch = train_density_forward_multi(self.engines, p, g, mode, distributed=_sharded())
        if defer_running_stats:
            # the sibling round of decoders._SiblingGroup: every decoder's buffers are updated when its own call arrives
            return out, logdet, lists, bn_batch
        for k, e in enumerate(self.engines):
            e._update_running_stats(bn_batch[k])
        return out, logdet, lists

    def forward_partition(self, p, g, counts, mode='direct'):
        """Sampling path: the N points are laid out component by component, ``counts[k]`` points for component k
        (sum == N); each point goes through ONE component.  -> (out, logdet), each (B,3,N)."""
        e0 = self.engines[0]
        if e0.couplings[0].training:
            raise NotImplementedError('the sampling partition is an evaluation path (reference flow_mixture.py:146); call .eval()')
        e0._check(p, g)
        if len(counts) != self.K or sum(int(c) for c in counts) != p.shape[2]:
            raise ValueError('counts must have K entries summing to N')
        segs, off = [], 0
        for cnt in counts:
            segs.append((off, off + int(cnt)))
            off += int(cnt)
        pw, film, eps = self._film(g.contiguous().float())
        # no re-run launch here (base samples of a few units; one shape per call is latency-bound) unless the exact body is forced
        return _lib.stack_forward_multi(p.contiguous().float(), pw, film, self.K, self.C, self.f, e0.pattern0, eps, mode,
                                        segments=segs, shared_points=False, packed_x=exact_record(self, rerun=False))

    def _routed_work(self, S, n, device):
        """The routing scratch of (S, n, K, P), P from the stack's tile choice under the current tuning word: allocated once."""
        P = _lib.route_points_per_tile(S, n, self.K, self.f)
        key = (S, n, self.K, P, str(device))
        if key not in self._route_work:
            self._route_work[key] = _lib.route_scratch(S, n, self.K, P, device)
        return self._route_work[key]

    def _routed_ready(self, g):
        """What both routed entry points check before anything is launched."""
        e0 = self.engines[0]
        if e0.couplings[0].training:
            raise NotImplementedError('the sampling partition is an evaluation path (reference flow_mixture.py:146); call .eval()')
        if _lib.EXACT[0]:
            raise _lib.GwtfError('exact_fp32: the routed stack launch has no exact-fp32 body')
        return e0

    def launch_routed(self, work, g, out=None, want_logdet=False):
        """FiLM + the routed stack launch on a layout `_lib.mixture_route` left in `work` -> (out, logdet or None), each (S, 3, n).
        g: (S, G) codes, or a (K, S, G) table with a code per component and row (`_lib.mixture_route_sweep`'s rows)."""
        e0 = self._routed_ready(g)
        S, n = work['labels'].shape
        if out is None:
            out = torch.empty(S, 3, n, device=g.device, dtype=torch.float32)
        logdet = torch.empty(S, 3, n, device=g.device, dtype=torch.float32) if want_logdet else None
        pw, film, eps = (self._film_k if g.dim() == 3 else self._film)(g.contiguous().float())
        return _lib.stack_forward_routed(work, pw, film, out, logdet, self.K, self.C, self.f, e0.pattern0, eps)

    def forward_routed(self, z0, g, labels):
        """Sampling path with per-point components: z0 (S,3,n) float32 base samples and labels (S,n) int32 in [0, K), both on the
        device; point i of shape s goes through component labels[s, i] and comes back in its own position.  -> (out, logdet), each
        (S,3,n).  Nothing is read back: the tile layout is built on the device (csrc/gwtf_route.hip).  A point that leaves the
        f16-safe range comes back NaN, as from forward_partition."""
        e0 = self._routed_ready(g)
        e0._check(z0, g)
        S, _, n = z0.shape
        dev = z0.device
        if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.device != dev or tuple(labels.shape) != (S, n) \
                or not labels.is_contiguous():
            raise _lib.GwtfError(f'labels must be a contiguous int32 tensor of shape {(S, n)} on {dev}')
        if z0.dtype != torch.float32 or not z0.is_contiguous():
            raise _lib.GwtfError('z0 must be contiguous float32')
        work = self._routed_work(S, n, dev)
        _lib.mixture_route(work, labels_in=labels, z0_in=z0)
        return self.launch_routed(work, g, want_logdet=True)


class _MixtureNLLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, logdet, mu0, lv0, logits):
        z, logdet, mu0, lv0, logits = (t.contiguous().float() for t in (z, logdet, mu0, lv0, logits))
        nll, plse = _lib.mixture_nll(z, logdet, mu0, lv0, logits, True)
        ctx.save_for_backward(z, logdet, mu0, lv0, logits, plse)
        ctx.mark_non_differentiable(plse)
        return nll, plse

    @staticmethod
    def backward(ctx, g_nll, _g_plse):
        z, logdet, mu0, lv0, logits, plse = ctx.saved_tensors
        L = _lib.lib()
        K, B, _, N = z.shape
        g_z, g_ld = torch.empty_like(z), torch.empty_like(logdet)
        g_mu0, g_lv0, g_logits = torch.empty_like(mu0), torch.empty_like(lv0), torch.empty_like(logits)
        g_nll = g_nll.contiguous().float()
        with torch.cuda.device(z.device):
            _lib.check(L.gwtf_mixture_nll_backward(z.data_ptr(), logdet.data_ptr(), mu0.data_ptr(), lv0.data_ptr(),
                                                   logits.data_ptr(), plse.data_ptr(), g_nll.data_ptr(), g_z.data_ptr(),
                                                   g_ld.data_ptr(), g_mu0.data_ptr(), g_lv0.data_ptr(), g_logits.data_ptr(),
                                                   K, B, N, _lib._stream(z)))
        return g_z, g_ld, g_mu0, g_lv0, g_logits


def flow_mixture_nll(z, logdet, mu0, lv0, logits, want_point_lse=False):
    """FlowMixtureNLL on fused decoder outputs (reference losses.py:88-137).

    z, logdet (K,B,3,N): final inverse coordinates / sum of coupling logvars per component;
    mu0, lv0 (K,B,3): base Gaussians; logits (B,K).  -> (pnll scalar = batch mean, per-shape (B,) [, per-point lse])."""
    nll, plse = _MixtureNLLFn.apply(z, logdet, mu0, lv0, logits)     # differentiable w.r.t. all five inputs
    return (nll.mean(), nll, plse) if want_point_lse else (nll.mean(), nll)
