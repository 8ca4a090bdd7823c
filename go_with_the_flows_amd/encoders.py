"""Point-cloud encoder and the per-shape heads that sit immediately before the point-flow decoder.

Host-side mirror of lib/networks/encoders.py (PointNetCloudEncoder :9-28, FeatureEncoder :31-85, WeightsEncoder :87-91):
same constructors, attribute names and ``state_dict`` keys, so the reference's checkpoints load.

PointNetCloudEncoder in eval mode under ``torch.no_grad()`` runs the fused HIP kernel (csrc/gwtf_encoder.hip: all
SharedDot+BatchNorm+ReLU layers chained in registers on the MFMA, optional max-pool fused).  ``forward_max`` under
``.train()`` (batch-statistic BatchNorm, what the training step runs: models.py:127-128 inside training.py:43-54) is the
layer-at-a-time HIP pipeline of csrc/gwtf_encoder_train.hip, forward and backward (``_EncoderTrainFn``).  What is left to
plain library GEMMs and batch-norms on the HIP device (torch.matmul -> rocBLAS, F.batch_norm -> MIOpen, differentiated by
autograd): eval mode with a gradient required, ``forward`` (the full (B,C,N) feature map) in train mode, width lists
without kernels, an input that itself requires a gradient.  CPU tensors raise: there is no CPU path.  The per-shape heads
(FeatureEncoder, WeightsEncoder) run one HIP launch per layer, forward and backward (csrc/gwtf_heads.hip, ``_HeadsFn``), for any
number of rows (the gathered rows of a large data-parallel batch are walked 64 / 128 at a time inside the kernels).
"""
import ctypes
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from ._lib import GwtfError, _ptr, _stream, check
from .layers import SharedDot, Swish


def _bn_sync(bn):
    """True when this BatchNorm sums its batch statistics over the ranks (SyncBatchNorm after train_ae.py:152, more than
    one rank in the default group)."""
    from .dist import sharded
    return isinstance(bn, nn.SyncBatchNorm) and sharded()


def _over_ranks(src, dst):
    """dst = src summed over the ranks: the statistic record a synchronised run exchanges between two phases of the pipeline."""
    import torch.distributed as dist
    from .dist import run
    dst.copy_(src)
    run(dist.all_reduce, dst, op=dist.ReduceOp.SUM)


class _EncoderTrainFn(torch.autograd.Function):
    """pooled (B,512) = max over points of the train-mode encoder, csrc/gwtf_encoder_train.hip.  params = (W, bn.weight,
    bn.bias) of the four layers; ``enc`` supplies the BatchNorm buffers (running statistics are updated in place, as
    F.batch_norm does).  Both directions fill one _lib.EncTrainCtx (include/gwtf.h GwtfEncTrainCtx: what every buffer is) and make one
    call -- or, synchronised, walk the phases and sum the named statistic record over the ranks between them."""

    @staticmethod
    def forward(ctx, x, enc, sync, *params):
        from .autograd import _zero_arena
        from .dist import row_layout
        L = _lib.lib()
        x = x.contiguous()
        B, _, N = x.shape
        dev, R, C = x.device, _lib.STAT_REPLICAS, enc._widths
        bns = enc._bns()
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)
        # every zero-initialised accumulator of the forward pass from ONE fill: {coordinate moments, layer sums, maxima, keys}
        zero = _zero_arena(dict(mom=(R, 12), sums1=(R, 2, C[2]), sums2=(R, 2, C[3]), sums3=(R, 2, C[4]), ymax=(4,),
                                keys=(2, B, 2 * C[4])), dev)                 # keys: 64-bit arg-max / arg-min keys of y_3 (never stored)
        units = [L.gwtf_enc_train_units_floats(l) for l in (1, 2, 3)]
        buf = dict(
            x=x, W=[w.detach().reshape(C[l + 1], C[l]).contiguous() for l, w in enumerate(params[0::3])],
            gamma=[g.detach().contiguous() for g in params[1::3]], beta=[b.detach().contiguous() for b in params[2::3]],
            running_mean=[bn.running_mean if bn.track_running_stats else None for bn in bns],
            running_var=[bn.running_var if bn.track_running_stats else None for bn in bns],
            mom=zero['mom'], mom_c=new(12), sums=[zero[f'sums{l}'] for l in (1, 2, 3)], sums_c=[new(2, C[l + 1]) for l in (1, 2, 3)],
            ymax=zero['ymax'], kmax=zero['keys'][0], kmin=zero['keys'][1], aff=[new(4 * C[l + 1]) for l in range(4)], table0=new(4 * C[1]),
            units_f=[new(n) for n in units], units_b=[new(n) for n in units],
            # y_1, y_2 (and the backward's dA arrays) in tiles of 32 points x all channels: include/gwtf.h gwtf_enc_train_act_floats
            y=[new(L.gwtf_enc_train_act_floats(B, C[l + 1], N)) for l in (1, 2)],
            pooled=new(B, C[4]), amax=new(B, C[4], dtype=torch.int32), ystar=new(B, C[4]))
        for given in (x, *buf['W'], *buf['gamma'], *buf['beta'], *buf['running_mean'], *buf['running_var']):
            _ptr(given, 'encoder operand')                   # device / dtype / layout checks of what the caller handed in
        # what the folds read: this rank's compact records, or their copies summed over the ranks
        buf['mom_fold'] = new(12) if sync else buf['mom_c']
        buf['sums_fold'] = [torch.empty_like(t) for t in buf['sums_c']] if sync else buf['sums_c']
        # points the statistics cover: every rank's shapes (the per-rank batch may differ by one, train_ae.py:77-78; the counts
        # are exchanged once and cached, dist.row_layout)
        t = _lib.EncTrainCtx(B=B, N=N, n_total=float((row_layout(B, dev).total if sync else B) * N), stream=_stream(x))
        t.momentum[:] = [float(bn.momentum) for bn in bns]
        t.bind(buf)
        with torch.cuda.device(dev):
            if not sync:
                check(L.gwtf_enc_train_forward(ctypes.addressof(t)))
            else:
                check(L.gwtf_enc_train_phase(ctypes.addressof(t), _lib.ENC_PHASE_FWD_INIT, 0))
                _over_ranks(buf['mom_c'], buf['mom_fold'])
                for l in range(4):
                    check(L.gwtf_enc_train_phase(ctypes.addressof(t), _lib.ENC_PHASE_FWD_LAYER, l))
                    if l < 3:
                        _over_ranks(buf['sums_c'][l], buf['sums_fold'][l])
            counters = [bn.num_batches_tracked for bn in bns if bn.track_running_stats and bn.num_batches_tracked is not None]
            if counters:
                torch._foreach_add_(counters, 1)                                 # (one launch for the four counters)
        # the record and the tensors behind its pointers stay on ctx; the outputs go through save_for_backward (pooled -> grad_fn ->
        # ctx -> pooled would be a cycle that only the garbage collector frees, and every buffer of the step with it)
        pooled, amax = buf.pop('pooled'), buf.pop('amax')
        ctx.save_for_backward(x, pooled, amax, *params)
        ctx.rec, ctx.buf, ctx.meta = t, buf, (sync, tuple(C))
        ctx.mark_non_differentiable(amax)
        return pooled, amax

    @staticmethod
    def backward(ctx, g_pooled, _g_amax):
        from .autograd import _zero_arena
        L = _lib.lib()
        x, _pooled, _amax, *params = ctx.saved_tensors
        t, (sync, C) = ctx.rec, ctx.meta
        B, N, dev, R = t.B, t.N, x.device, _lib.STAT_REPLICAS
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)
        # every zero-initialised accumulator of the backward pass from ONE fill
        zero = _zero_arena(dict(gmax=(4,), g0=(R, 5, C[1]), g1=(R, 2, C[2]), g2=(R, 3, C[3])), dev)
        buf = dict(
            g_pooled=g_pooled.contiguous().float(), gp=new(B, C[4]), gmax=zero['gmax'], g_sums=[zero['g0'], zero['g1'], zero['g2']],
            g_sums_c=[new(5, C[1]), new(2, C[2]), new(3, C[3]), new(2, C[4])], bconst=[new(3 * C[l + 1] + 4) for l in range(4)],
            units_m=new(L.gwtf_enc_train_units_floats(3) // 2), mconst=new(C[3] + 4),
            mform_ws=new(L.gwtf_enc_train_mform_workspace_floats(C[3])), extra=new(B, C[4], C[3]),
            slot_of=new(B, N, dtype=torch.int32), tables=new(B * (2 * C[4] + 2), dtype=torch.int32), a2rows=new(B, C[4], C[3]),
            dA=[new(L.gwtf_enc_train_act_floats(B, C[l + 1], N)) for l in (1, 2)],
            partials=new(max(L.gwtf_enc_train_dw_partial_floats(l, B, N) for l in (1, 2, 3))), gram=new(C[3], C[3]), S=new(C[4], C[3]),
            dW=[new(C[l + 1], C[l]) for l in range(4)])
        # what the consts kernels read: the first two rows of this rank's compact sums, or their copies summed over the ranks
        buf['g_sums_r'] = [new(2, C[l + 1]) for l in range(4)] if sync else buf['g_sums_c']
        _ptr(buf['g_pooled'], 'g_pooled')
        t.bind(buf)
        t.stream = _stream(x)
        with torch.cuda.device(dev):
            if not sync:
                check(L.gwtf_enc_train_backward(ctypes.addressof(t)))
            else:
                check(L.gwtf_enc_train_phase(ctypes.addressof(t), _lib.ENC_PHASE_BWD_TOP, 0))
                for l in (3, 2, 1, 0):
                    _over_ranks(buf['g_sums_c'][l][:2], buf['g_sums_r'][l])
                    check(L.gwtf_enc_train_phase(ctypes.addressof(t), _lib.ENC_PHASE_BWD_LAYER, l))
        grads = []
        for l in range(4):               # W, bn.weight, bn.bias of layer l (views of this rank's compact sums: nothing writes them again)
            grads += [buf['dW'][l].view_as(params[3 * l]), buf['g_sums_c'][l][1], buf['g_sums_c'][l][0]]
        return (None, None, None, *grads)


class PinnedEncoderWeights:
    """The fused eval kernel's packing of a ``PointNetCloudEncoder`` in PERSISTENT device buffers: the raw arena (weights, BatchNorm
    affine parameters and running statistics, gathered by one pointer-table launch) and the packing gwtf_encoder_pack makes of it.
    ``refresh()`` is those two launches into the same storage -- no allocation, no version counter: capturable, and valid between
    training steps that write parameters and running statistics through raw pointers.  While ``encoder.pin(self)`` holds,
    ``encoder.packed()`` returns ``self.packed``.  The table describes the storage the tensors have now (``.to()`` needs a new set)."""

    def __init__(self, enc):
        L = _lib.lib()
        src = enc._sources()
        dev = src[0].device
        if dev.type != 'cuda':
            raise GwtfError('module parameters are on the CPU: packed weights live on a HIP device only (.cuda() the model first)')
        self._widths = enc._widths_c()
        size = L.gwtf_encoder_packed_floats(*self._widths)
        if size == 0:
            raise GwtfError(f'no encoder kernel was built for widths {enc._widths}: nothing to pin')
        rows, off = [], 0
        if any(t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() for t in src):
            raise GwtfError('pinned eval weights need contiguous float32 parameters and buffers on one HIP device')
        self._sources = [t.detach().view(-1) for t in src]         # (kept alive: the table's pointers)
        for t in self._sources:
            rows.append((t.data_ptr(), off, t.numel()))
            off += t.numel()
        if off != L.gwtf_encoder_raw_floats(*self._widths):
            raise GwtfError('encoder raw arena size mismatch')
        self.n_rows = len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.raw = torch.empty(off, device=dev, dtype=torch.float32)
        self.packed = torch.empty(size, device=dev, dtype=torch.float32)

    def __reduce__(self):
        """copy.deepcopy / pickle of a pinned encoder: the copy is not pinned."""
        return (type(None), ())

    def refresh(self):
        _lib.gather_table(self.table, self.raw, self.n_rows)
        with torch.cuda.device(self.raw.device):
            check(_lib.lib().gwtf_encoder_pack(_ptr(self.raw, 'raw'), _ptr(self.packed, 'packed'), *self._widths, _stream(self.raw)))
        return self

    def buffers(self):
        return {'encoder_raw': self.raw, 'encoder_packed': self.packed}


class PointNetCloudEncoder(nn.Module):
    def __init__(self, init_n_channels, init_n_features, n_features):
        super().__init__()
        self.init_n_channels = init_n_channels
        self.init_n_features = init_n_features
        self.n_features = n_features
        layers = OrderedDict()
        widths = [init_n_channels, init_n_features] + list(n_features)
        for i in range(1, len(widths)):
            name = 'init_sd' if i == 1 else f'sd{i - 2}'
            layers[name] = SharedDot(widths[i - 1], widths[i], 1, bias=False)
            layers[name + '_bn'] = nn.BatchNorm1d(widths[i])
            layers[name + '_relu'] = nn.ReLU(inplace=True)
        self.features = nn.Sequential(layers)
        self._widths = widths
        self._packed = None
        self._stamp = None

    # ---- packed weights (BatchNorm folded, split-f16 fragment order), cached per parameter version ----
    def _sources(self):
        out = []
        for name, mod in self.features.named_children():
            if isinstance(mod, SharedDot):
                out.append(mod.weight)
            elif isinstance(mod, nn.modules.batchnorm._BatchNorm):   # BatchNorm1d, or SyncBatchNorm after train_ae.py:152
                out += [mod.weight, mod.bias, mod.running_mean, mod.running_var]
        return out

    def invalidate_packed_weights(self):
        self._packed = None

    def train(self, mode=True):
        self._packed = None
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def _bns(self):
        return [m for m in self.features.children() if isinstance(m, nn.modules.batchnorm._BatchNorm)]

    def _widths_c(self):
        return (ctypes.c_int * len(self._widths))(*self._widths), len(self._widths)

    def pin(self, pinned=None):
        """Pin packed() to a ``PinnedEncoderWeights`` (a new, refreshed one by default) and return it; kept through train() / eval() /
        invalidate_packed_weights(), changed only by its refresh().  ``unpin()`` restores the version-keyed cache."""
        pinned = PinnedEncoderWeights(self).refresh() if pinned is None else pinned
        self.__dict__['_pinned'] = pinned
        return pinned

    def unpin(self):
        self.__dict__['_pinned'] = None

    def packed(self):
        pinned = self.__dict__.get('_pinned')
        if pinned is not None:
            return pinned.packed
        src = self._sources()
        stamp = tuple((t.data_ptr(), t._version) for t in src)
        if self._packed is None or stamp != self._stamp:
            L = _lib.lib()
            w, n = self._widths_c()
            size = L.gwtf_encoder_packed_floats(w, n)
            if size == 0:
                raise GwtfError(f'no encoder kernel was built for widths {self._widths} '
                                '(built: [3,64,128,256,512] and [3,64,128,64,128]); see csrc/gwtf_encoder.hip')
            raw = torch.cat([t.detach().reshape(-1) for t in src])
            if raw.numel() != L.gwtf_encoder_raw_floats(w, n):
                raise GwtfError('encoder raw arena size mismatch')
            packed = torch.empty(size, device=raw.device, dtype=torch.float32)
            with torch.cuda.device(raw.device):
                check(L.gwtf_encoder_pack(_ptr(raw, 'raw'), _ptr(packed, 'packed'), w, n, _stream(raw)))
            self._packed, self._stamp = packed, stamp
        return self._packed

    def _fused(self, x, want_features, want_pooled):
        B, c, N = x.shape
        if c != 3 or self._widths[0] != 3:
            raise GwtfError(f'encoder input must be (B,3,N); got {tuple(x.shape)}')
        x = x.contiguous()
        packed = self.packed()
        C = self._widths[-1]
        feat = torch.empty(B, C, N, device=x.device, dtype=torch.float32) if want_features else None
        pooled = torch.empty(B, C, device=x.device, dtype=torch.float32) if want_pooled else None
        w, n = self._widths_c()
        with torch.cuda.device(x.device):
            check(_lib.lib().gwtf_encoder_forward(_ptr(x, 'input'), _ptr(packed, 'packed'), _ptr(feat, 'features'),
                                                  _ptr(pooled, 'pooled'), B, N, w, n, _stream(x)))
        return feat, pooled

    def has_fused_kernel(self):
        """True when csrc/gwtf_encoder.hip holds an instantiation for this width list."""
        w, n = self._widths_c()
        return _lib.lib().gwtf_encoder_packed_floats(w, n) != 0

    def _needs_graph(self, x):
        if self.training or (torch.is_grad_enabled() and
                             (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return True
        return not self.has_fused_kernel()        # widths without an instantiation: the library-GEMM path on the device

    def forward(self, input):
        """(B,3,N) -> (B,C_last,N) per-point features (reference encoders.py:27-28)."""
        _ptr(input if input.is_contiguous() else input.contiguous(), 'input')      # device / dtype checks, loud on CPU
        if self._needs_graph(input):
            return self.features(input)
        return self._fused(input, True, False)[0]

    def _train_pipeline_ok(self, x):
        """The layer-at-a-time HIP train pipeline covers this call: batch-statistic BatchNorm with a momentum, the width
        list the kernels were built for, no gradient wanted for the points themselves, N a multiple of 4."""
        if not self.training or x.dim() != 3 or x.shape[1] != 3 or x.shape[2] % 4 or x.shape[0] == 0:
            return False
        if x.shape[2] > 12288:               # the arg-max row tables of the top layer's backward index the points of a shape in LDS
            return False
        if torch.is_grad_enabled() and x.requires_grad:
            return False
        bns = self._bns()
        if any(bn.momentum is None or not bn.affine or not bn.training for bn in bns):     # a frozen (eval) BatchNorm: library path
            return False
        if len({_bn_sync(bn) for bn in bns}) > 1:                                            # mixed plain / synchronised modules
            return False
        w, n = self._widths_c()
        return bool(_lib.lib().gwtf_enc_train_supported(w, n))

    def _train_params(self):
        out = []
        for mod in self.features.children():
            if isinstance(mod, SharedDot):
                out.append(mod.weight)
            elif isinstance(mod, nn.modules.batchnorm._BatchNorm):
                out += [mod.weight, mod.bias]
        return out

    def forward_max(self, input, return_indices=False):
        """(B,3,N) -> (B,C_last): features max-pooled over points, what models.py:127-128 consumes; eval/no-grad never
        materialises the (B,C_last,N) tensor, train mode runs csrc/gwtf_encoder_train.hip (forward and backward)."""
        _ptr(input if input.is_contiguous() else input.contiguous(), 'input')
        if self._train_pipeline_ok(input):
            pooled, amax = _EncoderTrainFn.apply(input, self, _bn_sync(self._bns()[0]), *self._train_params())
            return (pooled, amax) if return_indices else pooled
        if self._needs_graph(input):
            pooled, amax = torch.max(self.features(input), dim=2)
            return (pooled, amax) if return_indices else pooled
        if return_indices:
            raise GwtfError('arg-max indices are not produced by the fused eval kernel')
        return self._fused(input, False, True)[1]


class _HeadsFn(torch.autograd.Function):
    """One layer of a per-shape head, or two layers on the same input (the mu and logvar heads of a FeatureEncoder), on the HIP
    device (csrc/gwtf_heads.hip): out = act(BatchNorm(x W^T + bias)) per head, forward and backward one C call each on one record
    (include/gwtf.h GwtfHeadArgs).  specs: per head (bn, bn_mode, act) -- bn: the BatchNorm module whose buffers the forward updates
    (None: no BatchNorm); bn_mode 0 none / 1 batch statistics / 2 running statistics; act 0 none / 1 swish / 2 log_softmax.
    params: per head W, bias, gamma, beta (each but W may be None).  Returns the tuple of the heads' outputs."""

    @staticmethod
    def forward(ctx, x, bn_updates, specs, *params):
        x = x.contiguous()
        params = [None if t is None else t.contiguous() for t in params]
        B, Din = x.shape
        new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float32)
        a = _lib.HeadArgs(n_heads=len(specs), B=B, Din=Din, bn_updates=int(bn_updates), stream=_stream(x))
        buf = dict(x=x, W=params[0::4], bias=params[1::4], gamma=params[2::4], beta=params[3::4], running_mean=[], running_var=[],
                   num_batches_tracked=[], ypre=[], stats=[], out=[])
        written = []                                            # BatchNorm buffers the kernel updates through raw pointers
        for h, (bn, bn_mode, act) in enumerate(specs):
            Dout = buf['W'][h].shape[0]
            tracked = bn is not None and bn.track_running_stats and bn.running_mean is not None
            state = (bn.running_mean, bn.running_var, bn.num_batches_tracked) if tracked else (None, None, None)
            for name, t in zip(('running_mean', 'running_var', 'num_batches_tracked'), state):
                buf[name].append(t)
            if bn_mode == 1:
                written += [t for t in state if t is not None]
            buf['ypre'].append(new(B, Dout))
            buf['stats'].append(new(3, Dout) if bn_mode else None)
            buf['out'].append(new(B, Dout))
            a.Dout[h], a.bn_mode[h], a.act[h] = Dout, bn_mode, act
            a.momentum[h] = float(bn.momentum) if bn is not None and bn.momentum is not None else 0.0
            a.bn_eps[h] = float(bn.eps) if bn is not None else 1e-5
        for given in (x, *params, *buf['running_mean'], *buf['running_var']):
            _ptr(given, 'head operand')                          # device / dtype / layout checks of what the caller handed in
        a.bind(buf)
        with torch.cuda.device(x.device):
            check(_lib.lib().gwtf_heads_forward(ctypes.addressof(a)))
        if written:
            torch._C._increment_version(written)
        # the record stays on ctx; the tensors behind its pointers go through save_for_backward (out -> grad_fn -> ctx -> out would be a
        # cycle that only the garbage collector frees)
        ctx.save_for_backward(x, *params, *buf['ypre'], *buf['stats'], *buf['out'])
        ctx.rec = a
        ctx.set_materialize_grads(False)       # an output the loss does not read arrives as None: its head's parameters get no gradient
        return tuple(buf['out'])

    @staticmethod
    def backward(ctx, *g_outs):
        a = ctx.rec
        n = a.n_heads
        if all(g is None for g in g_outs):
            return (None,) * (3 + 4 * n)
        x, *saved = ctx.saved_tensors
        params, outs = saved[:4 * n], saved[6 * n:]
        new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float32)
        need = ctx.needs_input_grad
        used = [g is not None for g in g_outs]
        g_out = [g.contiguous().float() if u else torch.zeros_like(o) for g, u, o in zip(g_outs, used, outs)]
        grads = []                                               # per head: g_W, g_bias, g_gamma, g_beta
        for h in range(n):
            Dout = a.Dout[h]
            grads.append(new(Dout, a.Din) if need[3 + 4 * h] else None)
            grads += [new(Dout) if (params[4 * h + i] is not None and need[3 + 4 * h + i]) else None for i in (1, 2, 3)]
        buf = dict(g_out=g_out, g_y=[new(a.B, a.Dout[h]) for h in range(n)], g_x=new(a.B, a.Din) if need[0] else None,
                   g_W=grads[0::4], g_bias=grads[1::4], g_gamma=grads[2::4], g_beta=grads[3::4])
        a.bind(buf)
        a.stream = _stream(x)
        with torch.cuda.device(x.device):
            check(_lib.lib().gwtf_heads_backward(ctypes.addressof(a)))
        return (buf['g_x'], None, None, *[g if used[i // 4] else None for i, g in enumerate(grads)])


class FeatureEncoder(nn.Module):
    """Per-shape MLP with Gaussian heads (reference encoders.py:31-85)."""

    def __init__(self, n_layers, in_features, latent_space_size, deterministic=False, batch_norm=True,
                 mu_weight_std=0.001, mu_bias=0.0, logvar_weight_std=0.01, logvar_bias=0.0, easy_init=False):
        super().__init__()
        self.n_layers, self.in_features, self.latent_space_size = n_layers, in_features, latent_space_size
        self.deterministic, self.batch_norm = deterministic, batch_norm
        self.mu_weight_std, self.mu_bias = mu_weight_std, mu_bias
        self.logvar_weight_std, self.logvar_bias = logvar_weight_std, logvar_bias
        self.easy_init = easy_init
        if n_layers > 0:
            self.features = nn.Sequential()
            for i in range(n_layers):
                self.features.add_module(f'mlp{i}', nn.Linear(in_features, in_features, bias=False))
                if batch_norm:
                    self.features.add_module(f'mlp{i}_bn', nn.BatchNorm1d(in_features))
                self.features.add_module(f'mlp{i}_swish', Swish())
        self.mus = nn.Sequential(OrderedDict(mu_mlp0=nn.Linear(in_features, latent_space_size, bias=True)))
        if not easy_init:
            with torch.no_grad():
                self.mus[-1].weight.normal_(std=mu_weight_std)
                self.mus[-1].bias.fill_(mu_bias)
        if not deterministic:
            self.logvars = nn.Sequential(OrderedDict(logvar_mlp0=nn.Linear(in_features, latent_space_size, bias=True)))
            if not easy_init:
                with torch.no_grad():
                    self.logvars[-1].weight.normal_(std=logvar_weight_std)
                    self.logvars[-1].bias.fill_(logvar_bias)

    def _bn_modules(self):
        return [m for m in self.features if isinstance(m, nn.modules.batchnorm._BatchNorm)] if self.n_layers > 0 else []

    def _features_functional(self, h, bn_updates):
        """self.features(h) layer by layer with torch.nn.functional calls -- for the two cases the module call cannot serve:
        SyncBatchNorm modules whose input already holds the rows of all ranks (their own forward would synchronise again), and
        `bn_updates` > 1 = the running statistics advanced as if this batch had been seen that many times (the reference
        evaluates p_prior once per mixture component on the same latents, models.py:169-193 inside flow_mixture.py:163-166)."""
        for mod in self.features:
            if isinstance(mod, nn.Linear):
                h = nn.functional.linear(h, mod.weight, mod.bias)
            elif isinstance(mod, nn.modules.batchnorm._BatchNorm):
                batch_stats = mod.training or not mod.track_running_stats
                x = h
                h = nn.functional.batch_norm(x, mod.running_mean if mod.track_running_stats else None,
                                             mod.running_var if mod.track_running_stats else None, mod.weight, mod.bias,
                                             batch_stats, 0.0 if mod.momentum is None else mod.momentum, mod.eps)
                if mod.training and mod.track_running_stats:
                    if mod.momentum is None:
                        raise NotImplementedError('BatchNorm momentum=None (cumulative average) is not supported here; the '
                                                  'reference never sets it (encoders.py:49)')
                    with torch.no_grad():
                        if bn_updates > 1:
                            xd = x.detach()
                            keep = (1.0 - mod.momentum) ** (bn_updates - 1)
                            # .data: the batch-norm node saved these buffers for its backward (it only reads them in eval mode); the
                            # replayed updates must not trip autograd's version check -- K real passes update them in place too
                            mod.running_mean.data.mul_(keep).add_(xd.mean(0), alpha=1.0 - keep)
                            mod.running_var.data.mul_(keep).add_(xd.var(0, unbiased=True), alpha=1.0 - keep)
                        if mod.num_batches_tracked is not None:
                            mod.num_batches_tracked.data.add_(bn_updates)
            else:
                h = mod(h)
        return h

    def _takes(self, h, lin, act):
        """csrc/gwtf_heads.hip takes the layer `lin` -> [BatchNorm] -> activation code `act` on the rows h: fp32 rows on the HIP device
        (any number of them: the kernels walk the batch in blocks), fp32 weights no wider than hip_max_width, sizes the kernels cover."""
        return (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32 and h.shape[0] >= 1 and lin.weight.dtype == torch.float32
                and max(lin.weight.shape) <= self.hip_max_width
                and bool(_lib.lib().gwtf_head_layer_supported(h.shape[0], lin.weight.shape[1], lin.weight.shape[0], act)))

    def _hip_layers(self, input):
        """[(Linear, BatchNorm or None)] of the trunk when csrc/gwtf_heads.hip covers this call (_takes for every trunk layer and head,
        plain Linear -> [BatchNorm1d with a momentum] -> Swish layers), else None: the library modules then run -- on the CPU
        (host-logic tests), for other dtypes."""
        layers, mods = [], list(self.features) if self.n_layers > 0 else []
        i = 0
        while i < len(mods):
            lin = mods[i]
            bn = mods[i + 1] if (i + 1 < len(mods) and isinstance(mods[i + 1], nn.modules.batchnorm._BatchNorm)) else None
            sw = mods[i + (2 if bn is not None else 1)] if i + (2 if bn is not None else 1) < len(mods) else None
            if not (isinstance(lin, nn.Linear) and lin.bias is None and isinstance(sw, Swish)):
                return None
            if bn is not None and (bn.momentum is None or (bn.training and input.shape[0] < 2)):
                return None
            layers.append((lin, bn))
            i += 3 if bn is not None else 2
        heads = [self.mus[-1]] if self.deterministic else [self.mus[-1], self.logvars[-1]]
        if not all(self._takes(input, lin, act) for lin, act in [(l, 1) for l, _ in layers] + [(l, self._head_act) for l in heads]):
            return None
        return layers

    _head_act = 0          # activation code of the mu head in csrc/gwtf_heads.hip (WeightsEncoder: 2 = log_softmax)
    # Widest layer the HIP layer kernels take (a knob for A/B timing against the library modules: set it to 0 to get those).
    # Measured on the MI355X, forward + backward inside a hipGraph (tools/diag/heads_time.py, B = 64), HIP against library:
    # g_posterior (512 wide) 114 / 148 us, p_prior 80 / 110 (G = 128) and 102 / 116 (G = 512), the mixture-weight encoder
    # (3 trunk layers) 100 / 189 and 133 / 200.  (The first mapping -- 64 output columns per workgroup, K walked in dependent
    # passes -- lost at 512: 255 us; csrc/gwtf_gemm.h gemm_splitk_t has the reason and the fix.)
    hip_max_width = 4096

    def _hidden(self, input, bn_updates=1):
        """The shared trunk: Linear -> BatchNorm -> Swish per layer.  In a synchronised data-parallel run (SyncBatchNorm modules,
        train_ae.py:152) every rank evaluates the trunk on the rows of ALL ranks and keeps its own (dist.gather_rows): one
        all-gather forward and one all-reduce backward per module instead of two collectives per BatchNorm layer."""
        if self.n_layers == 0:
            return input
        bns = self._bn_modules()
        from .dist import gather_rows, syncs_statistics
        sync = self.training and bool(bns) and syncs_statistics(bns)
        rows = input.shape[0]
        if sync:
            input, lay = gather_rows(input)
        layers = self._hip_layers(input)
        if layers is not None:
            h = input
            for lin, bn in layers:
                mode = 0 if bn is None else (1 if (bn.training or not bn.track_running_stats) else 2)
                h, = _HeadsFn.apply(h, bn_updates, ((bn, mode, 1),), lin.weight, None, bn.weight if bn is not None else None,
                                    bn.bias if bn is not None else None)
        elif not sync and bn_updates == 1:
            h = self.features(input)
        else:
            h = self._features_functional(input, bn_updates)
        return h[lay.row0:lay.row0 + rows] if sync else h

    def _head(self, seq, h, act=0):
        lin = seq[-1]
        if len(seq) == 1 and self._takes(h, lin, act):
            return _HeadsFn.apply(h, 1, ((None, 0, act),), lin.weight, lin.bias, None, None)[0]
        out = seq(h)
        return nn.functional.log_softmax(out, dim=1) if act == 2 else out

    def forward(self, input, bn_updates=1):
        h = self._hidden(input, bn_updates)
        if self.deterministic:
            return self._head(self.mus, h, self._head_act)
        la, lb = self.mus[-1], self.logvars[-1]
        if (self._head_act == 0 and len(self.mus) == 1 and len(self.logvars) == 1 and os.environ.get('GWTF_NO_HEAD_PAIR') != '1'
                and self._takes(h, la, 0) and self._takes(h, lb, 0)):
            # both heads: one launch (GWTF_NO_HEAD_PAIR=1: two one-head launches)
            return _HeadsFn.apply(h, 1, ((None, 0, 0), (None, 0, 0)), la.weight, la.bias, None, None, lb.weight, lb.bias, None, None)
        return self._head(self.mus, h, self._head_act), self._head(self.logvars, h)


class WeightsEncoder(FeatureEncoder):
    """Mixture-weight head: log-softmax of the deterministic output (reference encoders.py:87-91)."""

    _head_act = 2          # the log_softmax is fused into the head's kernel (and applied by FeatureEncoder._head otherwise)
