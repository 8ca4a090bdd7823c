"""One training step of the flow-mixture model as a single hipGraph replay.

The reference's loop (lib/networks/training.py:25-60: forward, loss, backward, optimiser step per batch) is host-bound on
an MI355X: ~3000 kernel launches per step for the airplane config.  ``GraphedTrainStep`` captures forward + loss + backward
once and replays it per batch (airplane config, K=4 x 33 couplings, 64 x 2048 points: see bench.py's also.train_step); the
optimiser stays outside the graph because its bias corrections and the learning-rate schedule are host-side state.

Data-parallel runs (one process per GPU, the model converted to SyncBatchNorm as train_ae.py:152 does): the SAME single graph
per rank.  Every exchange is inside it -- the packed BatchNorm-statistic all-reduces of the decoders' phase-split pipeline
(4 per depth level), the encoder's, the row all-gathers of the per-shape modules, and the gradient exchange
(dist.OverlappedGradients: one asynchronous all-reduce per decoder launched from inside the backward pass + one flat remainder)
-- as RCCL kernels captured with the rest (RCCL collectives are stream-capturable); no host synchronisation anywhere in the
step.  This replaces DistributedDataParallel's bucketed all-reduce (train_ae.py:153), whose hooks are host-driven.

``ResidentTrainLoop`` captures the whole iteration of the reference's loop instead -- batch draw, forward, loss, backward, NaN guard,
learning-rate schedule, optimiser and meters -- with the loop's state in device memory (csrc/gwtf_loop.hip); the host only replays.

``ResidentEvalLoop`` is the other half of the reference's epoch (train_ae.py:165-166), eval(): the validation pass as graph replays
between those of the training loop, on eval packings that are refreshed in place (models.EvalWeights); ``track_best``,
``checkpoint`` and ``save_checkpoint`` are eval()'s best-model rule and the reference's checkpoint file.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .dist import graph_capture as _graph_capture


class GraphedTrainStep:
    """step = GraphedTrainStep(model, criterion, optimizer, g_example, p_example); loss, pnll, gnll, gent = step(g, p).
    Single-view reconstruction (a model with an ``img_encoder``): ``GraphedTrainStep(..., images_example=images)`` and
    ``step(g, p, images)``; the image encoder's library convolutions and their autograd backward are captured with the rest.
    Data-parallel SVR steps need ``model.img_encoder.train_norm = 'hip'``: the fused BatchNorm2d kernels all-reduce their sums.

    * inputs are copied into static buffers, so every batch must have the example's shape (drop the ragged last batch,
      as the reference's DataLoader does with drop_last=True, train_ae.py:97);
    * the returned loss terms are static tensors overwritten by the next call -- ``float()`` / ``.item()`` them first;
    * BatchNorm running statistics, the reparameterisation noise (graph-safe Philox) and ``.grad`` live inside the graph;
      parameters are updated in place by ``optimizer.step()`` after each replay.
    """

    def __init__(self, model, criterion, optimizer, g_example, p_example, warmup=False, warmup_iters=2, data_parallel=None,
                 average_gradients=True, images_example=None):
        from .dist import OverlappedGradients, sharded
        # (argument checks first: nothing below them may run on a refused call, and they need no device)
        takes_images = getattr(model, 'img_encoder', None) is not None
        if takes_images and images_example is None:
            raise ValueError(f'{type(model).__name__} is image-conditioned: GraphedTrainStep needs images_example')
        if images_example is not None and not takes_images:
            raise ValueError(f'images_example was given, but {type(model).__name__} has no img_encoder')
        # data_parallel=None: decided by the process group (more than one rank, or GWTF_FORCE_SHARDED=1)
        data_parallel = sharded() if data_parallel is None else data_parallel
        if images_example is not None and data_parallel and getattr(model.img_encoder, 'train_norm', None) != 'hip':
            raise NotImplementedError("multi-rank SVR training is not built on the library BatchNorm2d path: set "
                                      "model.img_encoder.train_norm = 'hip' (the fused kernels sum their batch statistics over the "
                                      "ranks), the supported setting")
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.reducer = OverlappedGradients(model, average=average_gradients) if data_parallel else None
        self.g_static, self.p_static = g_example.clone(), p_example.clone()
        self.i_static = images_example.clone() if images_example is not None else None
        self.use_warmup_weights = warmup
        side = torch.cuda.Stream(device=g_example.device)
        side.wait_stream(torch.cuda.current_stream(g_example.device))
        # The warm-up iterations run forward + backward with no optimiser step in between: they must not leave a trace in the
        # model (BatchNorm running statistics / num_batches_tracked) or in the random-number stream, or the state after
        # construction would differ from the reference loop's (training.py:25-60) by `warmup_iters` phantom batches.
        # (model.buffers() covers the image encoder's BatchNorm2d / fc_bn statistics too.)
        bn_state = [(b, b.detach().clone()) for b in model.buffers()]
        rng_cpu, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(g_example.device)
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):              # allocator + lazy initialisation outside the capture
                self._fwd_bwd()
            with torch.no_grad():
                for b, saved in bn_state:
                    b.copy_(saved)
        torch.cuda.current_stream(g_example.device).wait_stream(side)
        torch.set_rng_state(rng_cpu)
        torch.cuda.set_rng_state(rng_dev, g_example.device)
        for mod in model.modules():                    # restored buffers: drop every packed-weight cache keyed on them
            if hasattr(mod, 'invalidate_packed_weights'):
                mod.invalidate_packed_weights()
        # no autograd graph of an earlier iteration may be alive during capture (hipStreamEndCapture crashes otherwise)
        self.terms = None
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with _graph_capture(self.graph):
            self.terms = self._fwd_bwd()

    def _fwd_bwd(self):
        self.optimizer.zero_grad(set_to_none=True)
        if self.i_static is not None:
            enc, dec = self.model.forward_fused(self.g_static, self.p_static, self.use_warmup_weights, images=self.i_static)
        else:
            enc, dec = self.model.forward_fused(self.g_static, self.p_static, self.use_warmup_weights)
        loss, pnll, gnll, gent = self.criterion.fused(enc, dec)
        if self.reducer is not None:
            with self.reducer:                         # gradients summed / averaged over the ranks, overlapped with the backward pass
                loss.backward()
        else:
            loss.backward()
        return tuple(t.detach() for t in (loss, pnll, gnll, gent))

    def __call__(self, g_input, p_input, images=None):
        if (images is None) != (self.i_static is None):
            raise ValueError('this step was built with images_example: call step(g, p, images)' if images is None else
                             'this step was built without images_example: call step(g, p)')
        self.g_static.copy_(g_input)
        self.p_static.copy_(p_input)
        if images is not None:
            self.i_static.copy_(images)
        self.graph.replay()
        self.optimizer.step()
        return self.terms


class ResidentTrainLoop:
    """loop = ResidentTrainLoop(model, criterion, optimizer, loader, scheduler); loop.set_epoch(e); loop.run(len(loader)).

    The reference's train() / train_svr() (lib/networks/training.py:12-100, 188-303) with the whole iteration on the device: ONE
    graph replay draws the batch (``DeviceCloudLoader`` for ``Flow_Mixture_Model``, ``DeviceSVRLoader`` with a device-resident
    ``ImageStore`` for ``Flow_Mixture_SVR_Model``), runs forward, loss and backward, tests the loss for NaN, looks up the cosine
    schedule of lr and beta2, applies the Adam / AMSGrad update with that step's bias corrections and feeds the four AverageMeters.
    The host only replays; ``meters()`` reads one 160-byte record (include/gwtf.h GwtfLoopState) when it wants to log.

    Launch order inside the capture: gwtf_loop_begin (this iteration's rows of the epoch plan), sample_clouds, for SVR
    transform_images, the body of ``GraphedTrainStep._fwd_bwd`` (gradient reducer included), gwtf_loop_commit (data-parallel: the
    guard's flag is MAX-reduced over the ranks between gwtf_loop_detect and the commit, so that all ranks update or none does), one
    gwtf_adam_step_table_dev per parameter group.

    * ``scheduler``: an ``optim.LRUpdater`` (tabulated on the host per epoch, ``LRUpdater.table``, indexed on the device); None keeps
      the groups' lr and betas, which must then agree over the groups.  Groups may differ in eps, weight_decay and amsgrad.
    * The moments of every updated parameter are created HERE, as zeros with ``state['step'] = 0``, before the capture -- visible in
      ``optimizer.state`` from construction on; a loaded optimiser state (``optimizer.load_state_dict``, then a new loop) is continued
      from its step count.  ``meters()`` writes the device's step count back into ``optimizer.state[p]['step']``, so that
      ``optimizer.state_dict()`` has the reference's format.  ``param_groups`` are not edited: the schedule lives in the table.
    * Construction leaves no trace (``GraphedTrainStep``'s rule): its warm-up iterations restore BatchNorm buffers, the RNG state,
      the loaders' sampler states and the loop state.
    * A non-finite loss (NaN; with ``stop_on_inf`` an infinity too) poisons the loop: parameters, moments, step count and cursor stay
      those from before that step (the reference's "Stopping without updating the net") and every later replay is a no-op for
      them.  Replays beyond the end of the epoch are no-ops in the same sense.  BatchNorm running statistics and the sampler
      states are NOT held back on such replays: the forward pass has run (the reference's failing pass moves them too, then exits).
    * Refused: sparse, non-float32 or non-contiguous parameters, and unequal step counts.  A parameter that receives no gradient in
      the warm-up iterations is left out of the update, and gets no optimiser state, as ``Adam.step()`` leaves it out (the mixture
      models carry one); ``loop.parameters`` lists the ones the loop updates.
    """

    def __init__(self, model, criterion, optimizer, loader, scheduler=None, warmup=False, data_parallel=None, stop_on_inf=False,
                 warmup_iters=2, average_gradients=True):
        from .clouds import make_state
        from .dist import OverlappedGradients, sharded
        from .images import HOST_STORE_IN_CAPTURE
        # (argument checks first: nothing below them may run on a refused call)
        svr = hasattr(loader, 'image_store')
        if svr != (getattr(model, 'img_encoder', None) is not None):
            raise ValueError(f'{type(model).__name__} and {type(loader).__name__} do not go together: an image-conditioned model needs '
                             'a DeviceSVRLoader, any other model a DeviceCloudLoader')
        if svr and loader.image_store.device.type != 'cuda':
            raise _lib.GwtfError(HOST_STORE_IN_CAPTURE)
        if not loader.return_eval_cloud:
            raise ValueError('the training step reads cloud and eval_cloud: the loader must return both')
        if len(loader) < 1:
            raise ValueError('the loader has no full batch')
        groups = optimizer.param_groups
        if scheduler is None and any((g['lr'], tuple(g['betas'])) != (groups[0]['lr'], tuple(groups[0]['betas'])) for g in groups):
            raise ValueError('all parameter groups share one schedule table: without a scheduler their lr and betas must agree')
        steps = set()
        for group in groups:
            for p in group['params']:
                if p.is_sparse or (p.grad is not None and p.grad.is_sparse):
                    raise RuntimeError('ResidentTrainLoop does not support sparse parameters or gradients')
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.GwtfError('ResidentTrainLoop needs contiguous float32 parameters on a HIP device (no CPU path)')
                if len(optimizer.state.get(p, {})):
                    steps.add(int(optimizer.state[p]['step']))
        if len(steps) > 1:
            raise ValueError(f'the parameters carry unequal step counts {sorted(steps)}: one schedule table cannot serve them')
        data_parallel = sharded() if data_parallel is None else data_parallel
        if svr and data_parallel and getattr(model.img_encoder, 'train_norm', None) != 'hip':
            raise NotImplementedError("multi-rank SVR training needs model.img_encoder.train_norm = 'hip'")
        self.model, self.criterion, self.optimizer, self.loader, self.scheduler = model, criterion, optimizer, loader, scheduler
        self.use_warmup_weights, self.data_parallel, self.stop_on_inf = warmup, bool(data_parallel), bool(stop_on_inf)
        self.reducer = OverlappedGradients(model, average=average_gradients) if data_parallel else None
        self._svr = svr
        store = loader.mesh_store if svr else loader.store
        dev = self.device = store.device
        B, N = loader.batch_size, loader.cloud_size
        self.n_iters = len(loader)
        # ---- static buffers ----
        self.g_static = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
        self.p_static = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
        self.i_static = None
        if svr:
            t, s = loader.image_transform, loader.image_store
            self.i_static = torch.empty((B, t.C_out) + tuple(t.output_size(s.height, s.width)), device=dev, dtype=torch.float32)
        self.rows = torch.zeros(B, dtype=torch.int32, device=dev)                   # item 0: valid until the first begin
        self.mesh_rows = torch.zeros(B, dtype=torch.int32, device=dev) if svr else None
        self.plan = torch.zeros(len(loader.index_plan()), dtype=torch.int32, device=dev)
        self.table = torch.zeros(self.n_iters, 8, dtype=torch.float32, device=dev)
        self.state = torch.zeros(ctypes.sizeof(_lib.LoopState) // 8, dtype=torch.int64, device=dev)     # one GwtfLoopState
        self._meters_view = self.state.view(torch.float64)[:12]
        self._ints = self.state.view(torch.int32)[32:40]        # cursor, n_iters, adam_step, status, poisoned_at, skip, flag, -
        self._flag = self._ints[6:7]
        if loader._state is None:                               # the seeds of the loaders' own __iter__
            seed = loader.seed + 0x9E3779B97F4A7C15 * loader.rank
            loader._state = make_state(seed, dev)
            if svr:
                loader._image_state = make_state(seed, dev)
        self._step0 = steps.pop() if steps else 0
        self._groups = []                                   # filled after the warm-up: it shows which parameters receive gradients
        self._ints.copy_(torch.tensor([0, 0, self._step0, 0, -1, 1, 0, 0], dtype=torch.int32))     # n_iters = 0: warm-up replays are no-ops
        # ---- warm-up (GraphedTrainStep's rule: no trace), then the capture ----
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        keep = [(b, b.detach().clone()) for b in model.buffers()]
        keep += [(s, s.clone()) for s in (loader._state, getattr(loader, '_image_state', None)) if s is not None]
        keep.append((self.state, self.state.clone()))
        rng_cpu, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        self.terms = None
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                self._args = None
                self._iteration()
            with_grad = {id(p) for group in groups for p in group['params'] if p.grad is not None}
            with torch.no_grad():
                for b, saved in keep:
                    b.copy_(saved)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.set_rng_state(rng_cpu)
        torch.cuda.set_rng_state(rng_dev, dev)
        for mod in model.modules():
            if hasattr(mod, 'invalidate_packed_weights'):
                mod.invalidate_packed_weights()
        self.terms = self._args = None
        optimizer.zero_grad(set_to_none=True)
        if not with_grad:
            raise ValueError('no parameter of the optimiser receives a gradient from this model and loss')
        if self._step0 > 0 and any(id(p) in with_grad and not len(optimizer.state.get(p, {})) for group in groups for p in group['params']):
            raise ValueError(f'some parameters carry step count {self._step0}, others no optimiser state: one schedule table cannot serve them')
        # ---- moments, and one pointer table per parameter group ----
        chunk = _lib.lib().gwtf_adam_chunk_elems()
        for group in groups:
            ams, plist = bool(group['amsgrad']), [p for p in group['params'] if id(p) in with_grad]
            if not plist:
                continue
            for p in plist:
                st = optimizer.state[p]
                if len(st) == 0:
                    st['step'], st['exp_avg'], st['exp_avg_sq'] = 0, torch.zeros_like(p), torch.zeros_like(p)
                if ams and 'max_exp_avg_sq' not in st:
                    st['max_exp_avg_sq'] = torch.zeros_like(p)
            sts = [optimizer.state[p] for p in plist]
            rows = [[p.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr(), s['max_exp_avg_sq'].data_ptr() if ams else 0,
                     p.numel()] for p, s in zip(plist, sts)]
            cmap = [(i, c) for i, p in enumerate(plist) for c in range((p.numel() + chunk - 1) // chunk)]
            self._groups.append({'plist': plist, 'ams': ams, 'eps': float(group['eps']), 'wd': float(group['weight_decay']),
                                 'table': torch.tensor(rows, dtype=torch.int64).to(dev),
                                 'cmap': torch.tensor(cmap, dtype=torch.int32).reshape(-1, 2).to(dev), 'n_chunks': len(cmap),
                                 'gtab': torch.zeros(len(plist), dtype=torch.int64, device=dev)})
        self.graph = torch.cuda.CUDAGraph()
        with _graph_capture(self.graph):
            self._iteration()
        # gradient addresses are known only now: fill the device tables before the first replay
        for g in self._groups:
            grads = [p.grad for p in g['plist']]
            if any(gr is None or gr.is_sparse or gr.dtype != torch.float32 or not gr.is_contiguous() for gr in grads):
                raise _lib.GwtfError('the captured backward pass left a missing, sparse, non-float32 or non-contiguous gradient')
            g['grads'] = grads                                   # (the graph's pool owns them; kept for the reader)
            g['gtab'].copy_(torch.tensor([gr.data_ptr() for gr in grads], dtype=torch.int64))
        self.parameters = [p for g in self._groups for p in g['plist']]     # the parameters the loop updates
        self._host_step, self._host_cursor = self._step0, 0
        self.epoch = None
        torch.cuda.synchronize(dev)

    # ---- the launches of one iteration (eager in the warm-up, then captured) ----
    def _loop_args(self):
        if self._args is None:
            a = _lib.LoopArgs(state=self.state.data_ptr(), plan=self.plan.data_ptr(), rows=self.rows.data_ptr(),
                              mesh_rows=None if self.mesh_rows is None else self.mesh_rows.data_ptr(), table=self.table.data_ptr(),
                              B=self.loader.batch_size, views=self.loader.views if self._svr else 1, plan_len=self.plan.numel(),
                              table_rows=self.table.shape[0], stop_on_inf=int(self.stop_on_inf), use_flag=int(self.data_parallel))
            self._args = a
        self._args.stream = torch.cuda.current_stream(self.device).cuda_stream
        return self._args

    def _iteration(self):
        from .clouds import sample_clouds
        from .dist import run as dist_run
        L, loader, dev = _lib.lib(), self.loader, self.device
        with torch.cuda.device(dev):
            _lib.check(L.gwtf_loop_begin(ctypes.addressof(self._loop_args())))
        out = {'cloud': self.g_static, 'eval_cloud': self.p_static}
        if self._svr:
            from .images import transform_images
            sample_clouds(loader.mesh_store, self.mesh_rows, loader.cloud_size, True, loader.cloud_transform, loader._state, out=out)
            transform_images(loader.image_store, self.rows, loader.image_transform, loader._image_state, out=self.i_static)
        else:
            sample_clouds(loader.store, self.rows, loader.cloud_size, True, loader.transform, loader._state, out=out,
                          permute=getattr(loader, 'permute', True))
        self.terms = GraphedTrainStep._fwd_bwd(self)
        if any(t.dtype != torch.float32 or not t.is_cuda for t in self.terms):
            raise _lib.GwtfError('the criterion must return four float32 device scalars')
        a = self._loop_args()
        a.terms[:] = [t.data_ptr() for t in self.terms]
        with torch.cuda.device(dev):
            if self.data_parallel:
                import torch.distributed as dist
                _lib.check(L.gwtf_loop_detect(ctypes.addressof(a)))
                dist_run(dist.all_reduce, self._flag, op=dist.ReduceOp.MAX)            # all ranks update, or none does
            _lib.check(L.gwtf_loop_commit(ctypes.addressof(a)))
            hyper, skip = self.state.data_ptr() + 96, self.state.data_ptr() + 128 + 20        # GwtfLoopState.hyper / .skip
            stream = torch.cuda.current_stream(dev).cuda_stream
            for g in self._groups:
                _lib.check(L.gwtf_adam_step_table_dev(g['table'].data_ptr(), g['gtab'].data_ptr(), g['cmap'].data_ptr(), g['n_chunks'],
                                                      hyper, skip, g['eps'], g['wd'], int(g['ams']), stream))

    # ---- the host's side ----
    def set_epoch(self, epoch, first_iteration=0):
        """Upload the epoch's plan and schedule table and set the cursor to ``first_iteration`` (the reference's resume ``iter``)."""
        from .optim import hyper_table
        epoch, first = int(epoch), int(first_iteration)
        if not 0 <= first <= self.n_iters:
            raise ValueError(f'first_iteration must lie in [0, {self.n_iters}]')
        self.loader.set_epoch(epoch)
        self.plan.copy_(torch.from_numpy(self.loader.index_plan().astype(np.int32)))
        n = self.n_iters - first
        if self.scheduler is not None:
            rows = self.scheduler.table(epoch, first, n, self._host_step + 1)
        else:
            g0 = self.optimizer.param_groups[0]
            rows = hyper_table([(g0['lr'], tuple(g0['betas']))] * n, self._host_step + 1)
        table = np.zeros((self.n_iters, 8), np.float32)
        table[first:] = rows
        self.table.copy_(torch.from_numpy(table))
        self._ints[:2].copy_(torch.tensor([first, self.n_iters], dtype=torch.int32))
        self.epoch, self._host_cursor = epoch, first

    def run(self, n):
        """Replay n iterations.  Nothing is synchronised; replays beyond the end of the epoch (or after a poisoned step) are no-ops."""
        if self.epoch is None:
            raise RuntimeError('call set_epoch(epoch) before run(n)')
        for _ in range(int(n)):
            self.graph.replay()
        done = max(0, min(int(n), self.n_iters - self._host_cursor))
        self._host_cursor += done
        self._host_step += done                                # (a poisoned loop stops counting on the device; nothing reads this then)
        for g in self._groups:                                 # raw-pointer writes: tell the packed-weight caches
            self.optimizer._bump_versions(g['plist'])

    def meters(self, reset=False):
        """One device-to-host copy of the record -> {'LB', 'PNLL', 'GNLL', 'GENT': (val, avg, sum, count), 'iteration', 'step',
        'poisoned', 'poisoned_at', 'exhausted'}; the step count is written into ``optimizer.state``.  reset: zero the meters."""
        rec = _lib.LoopState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        if reset:
            self._meters_view.zero_()
        out = {}
        for k, name in enumerate(('LB', 'PNLL', 'GNLL', 'GENT')):
            val, total, count = rec.meters[3 * k:3 * k + 3]
            out[name] = (val, total / count if count else 0.0, total, count)
        out.update(iteration=rec.cursor, step=rec.adam_step, poisoned=bool(rec.status & _lib.LOOP_POISONED),
                   poisoned_at=rec.poisoned_at, exhausted=bool(rec.status & _lib.LOOP_EXHAUSTED))
        for p in self.parameters:
            self.optimizer.state[p]['step'] = rec.adam_step
        return out



class _eval_flags:
    """``model.eval()`` for the block, by the modules' flags alone, and the flags put back as they were: ``nn.Module.train`` would also
    drop the version-keyed packed-weight caches and the data-parallel row layouts -- a trace a validation pass must not leave in a
    model that is being trained (the pass itself reads the pinned packings)."""

    def __init__(self, model):
        self.mods = list(model.modules())

    def __enter__(self):
        self.flags = [m.training for m in self.mods]
        for m in self.mods:
            m.training = False

    def __exit__(self, *exc):
        for m, flag in zip(self.mods, self.flags):
            m.training = flag
        return False


class ResidentEvalLoop:
    """val = ResidentEvalLoop(model, criterion, val_loader); result = val.validate(epoch).

    The reference's eval() (lib/networks/training.py:103-184: an eval-mode density pass over the validation part, the four
    AverageMeters, a stop on a NaN or infinite loss) on the device, between the replays of a ``ResidentTrainLoop`` on the SAME model.
    Two graphs, captured once:

    * ``refresh``: ``model.pin_eval_weights().refresh()`` -- every packed-weight cache of the eval path re-gathered and re-packed into
      persistent buffers (models.EvalWeights).  Replayed once at the start of a pass: the pass sees the
      parameters and BatchNorm running statistics as training left them, however they were written.
    * ``batch``: gwtf_loop_begin (this batch's rows of the plan) -> sample_clouds into static buffers -> ``forward_fused`` under eval
      flags and no_grad (the K decoders in ONE stack launch) -> ``criterion.fused`` -> gwtf_loop_eval_commit (meters; poisoned on a
      NaN or infinite loss, whatever follows is then a no-op).

    ``validate`` uploads the plan, resets the record, replays ``refresh`` once and ``batch`` ``len(loader) - first_iteration`` times
    (the reference's ``iter + i >= len(iterator)`` break) and reads the 160-byte record once; nothing in between synchronises.
    Its pieces are public: ``begin(epoch)``, ``run(n)`` (``terms`` are then the static loss terms of the last batch), ``meters()``.

    * The model stays pinned while the loop lives (``close()`` unpins a model the loop pinned itself); its train / eval flags, buffers
      and the RNG states are after construction what they were before, as after ``GraphedTrainStep``'s.  The validation loader's
      sampler state advances by one call per batch, as the loader's own iteration would; ``posterior='sample'`` draws from the CUDA
      generator as eval() does.
    * ``posterior='mean'``: the latent code is the posterior mean, no draw -- a deterministic validation loss the reference lacks.
    * ``warmup``: the flag ``get_weights`` branches on; a pass with the other value captures a second batch graph on first use.
    * Refused: image-conditioned models and ``DeviceSVRLoader`` (train_svr.py has no validation pass, and the ResNet encoder packs on
      the host), more than one rank, a loader without ``eval_cloud`` or without a full batch.
    """

    def __init__(self, model, criterion, loader, warmup=False, posterior='sample'):
        import torch.distributed as dist
        from .clouds import make_state
        # (argument checks first: nothing below them may run on a refused call, and they need no device)
        if posterior not in ('sample', 'mean'):
            raise ValueError(f"posterior must be 'sample' or 'mean', got {posterior!r}")
        if getattr(model, 'img_encoder', None) is not None or hasattr(loader, 'image_store'):
            raise NotImplementedError('ResidentEvalLoop covers the point-cloud autoencoder (train_ae.py): single-view reconstruction has no '
                                      'validation pass in the reference (train_svr.py), and its ResNet encoder packs its weights on the host')
        if not hasattr(model, 'pin_eval_weights'):
            raise ValueError(f'{type(model).__name__} has no pinned eval packings: ResidentEvalLoop needs a Flow_Mixture_Model')
        if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) or getattr(loader, 'world_size', 1) > 1:
            raise NotImplementedError('ResidentEvalLoop runs on one rank: a validation pass over several ranks is not built')
        if not loader.return_eval_cloud:
            raise ValueError('the validation pass reads cloud and eval_cloud: the loader must return both')
        if len(loader) < 1:
            raise ValueError('the loader has no full batch')
        dev = self.device = loader.store.device
        if dev.type != 'cuda' or any(not p.is_cuda for p in model.parameters()):
            raise _lib.GwtfError('ResidentEvalLoop needs the model and the mesh store on a HIP device (no CPU path)')
        self.model, self.criterion, self.loader = model, criterion, loader
        self.use_warmup_weights, self.posterior = bool(warmup), posterior
        B, N = loader.batch_size, loader.cloud_size
        self.n_iters = len(loader)
        self.g_static = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
        self.p_static = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
        self.rows = torch.zeros(B, dtype=torch.int32, device=dev)                   # item 0: valid until the first begin
        self.plan = torch.zeros(len(loader.index_plan()), dtype=torch.int32, device=dev)
        self.state = torch.zeros(ctypes.sizeof(_lib.LoopState) // 8, dtype=torch.int64, device=dev)     # the pass's own GwtfLoopState
        self._host_record(0, 0)                                                 # n_iters = 0: warm-up batches are no-ops for the record
        if loader._state is None:                                               # the seed of the loader's own __iter__
            loader._state = make_state(loader.seed + 0x9E3779B97F4A7C15 * loader.rank, dev)
        self._owns_pin = model.eval_weights is None
        self.weights = model.pin_eval_weights()
        self._graphs, self._args, self._terms = {}, {}, {}
        self.terms = None
        self.refresh_graph = self._graph = None
        self._capture(self.use_warmup_weights)
        torch.cuda.synchronize(dev)

    # ---- the launches of one batch (eager in the warm-up, then captured) ----
    def _host_record(self, first, n_iters):
        rec = _lib.LoopState(cursor=first, n_iters=n_iters, poisoned_at=-1)
        self.state.copy_(torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.int64).copy()))

    def _batch(self, warmup):
        from .clouds import sample_clouds
        L, loader, dev = _lib.lib(), self.loader, self.device
        a = self._args.get(warmup)
        if a is None:
            a = self._args[warmup] = _lib.LoopArgs(state=self.state.data_ptr(), plan=self.plan.data_ptr(), rows=self.rows.data_ptr(),
                                                   mesh_rows=None, table=None, B=loader.batch_size, views=1, plan_len=self.plan.numel(),
                                                   table_rows=self.n_iters, stop_on_inf=1, use_flag=0)
        a.stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(L.gwtf_loop_begin(ctypes.addressof(a)))
        sample_clouds(loader.store, self.rows, loader.cloud_size, True, loader.transform, loader._state,
                      out={'cloud': self.g_static, 'eval_cloud': self.p_static}, permute=getattr(loader, 'permute', True))
        enc, dec = self.model.forward_fused(self.g_static, self.p_static, warmup)
        terms = tuple(t.detach() for t in self.criterion.fused(enc, dec))
        if len(terms) != 4 or any(t.dtype != torch.float32 or not t.is_cuda for t in terms):
            raise _lib.GwtfError('the criterion must return four float32 device scalars')
        a.terms[:] = [t.data_ptr() for t in terms]
        a.stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(L.gwtf_loop_eval_commit(ctypes.addressof(a)))
        return terms

    def _capture(self, warmup, warmup_iters=2):
        """Capture the batch graph of this `warmup` flag (and, the first time, the refresh graph), leaving no trace."""
        model, dev = self.model, self.device
        keep = [(t, t.clone()) for t in (self.loader._state, self.state)]         # (an eval-mode pass writes no buffer of the model)
        rng_cpu, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        own = 'reparameterize' in model.__dict__
        saved = model.__dict__.get('reparameterize')
        if self.posterior == 'mean':
            model.reparameterize = lambda mu, logvar: mu
        try:
            with _eval_flags(model), torch.no_grad():
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(warmup_iters):              # allocator + lazy initialisation outside the capture
                        self.weights.refresh()
                        self._batch(warmup)
                    for t, was in keep:
                        t.copy_(was)
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.set_rng_state(rng_cpu)
                torch.cuda.set_rng_state(rng_dev, dev)
                if self.refresh_graph is None:
                    self.refresh_graph = torch.cuda.CUDAGraph()
                    with _graph_capture(self.refresh_graph):
                        self.weights.refresh()
                graph = torch.cuda.CUDAGraph()
                with _graph_capture(graph):
                    self._terms[warmup] = self._batch(warmup)
                self._graphs[warmup] = graph
                torch.set_rng_state(rng_cpu)
                torch.cuda.set_rng_state(rng_dev, dev)
        finally:
            if own:
                model.reparameterize = saved
            else:
                model.__dict__.pop('reparameterize', None)
        return graph

    # ---- the host's side ----
    def validate(self, epoch, first_iteration=0, warmup=None):
        """One validation pass -> ``meters()``'s dictionary.  first_iteration: the reference's resume ``iter`` (eval() runs
        ``len(iterator) - iter`` batches); warmup: None = the constructor's flag.  (= begin, run to the end, meters.)"""
        self.begin(epoch, first_iteration, warmup)
        self.run(self.n_iters - int(first_iteration))
        return self.meters()

    def begin(self, epoch, first_iteration=0, warmup=None):
        """Start a pass: upload the plan, reset the record (cursor = first_iteration, empty meters), replay ``refresh``."""
        if self.model.eval_weights is not self.weights:
            raise RuntimeError('the model is no longer pinned to this loop\'s eval packings (unpin_eval_weights(), .to() or close() '
                               'since construction): build a new ResidentEvalLoop')
        epoch, first = int(epoch), int(first_iteration)
        if not 0 <= first <= self.n_iters:
            raise ValueError(f'first_iteration must lie in [0, {self.n_iters}]')
        warmup = self.use_warmup_weights if warmup is None else bool(warmup)
        self._graph = self._graphs.get(warmup) or self._capture(warmup)
        self.loader.set_epoch(epoch)
        self.plan.copy_(torch.from_numpy(self.loader.index_plan().astype(np.int32)))
        self._host_record(first, self.n_iters)
        self.terms = self._terms[warmup]                       # the static loss terms of the batch replayed last
        self.refresh_graph.replay()

    def run(self, n):
        """Replay n batches of the pass begun.  Nothing is synchronised; replays beyond its end, or after a poisoned batch, change
        nothing in the record."""
        if self._graph is None:
            raise RuntimeError('call begin(epoch) before run(n)')
        for _ in range(int(n)):
            self._graph.replay()

    def meters(self):
        """One device-to-host copy of the record -> {'LB', 'PNLL', 'GNLL', 'GENT': (val, avg, sum, count), 'iteration', 'poisoned',
        'poisoned_at'} of the last pass."""
        rec = _lib.LoopState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        out = {}
        for k, name in enumerate(('LB', 'PNLL', 'GNLL', 'GENT')):
            val, total, count = rec.meters[3 * k:3 * k + 3]
            out[name] = (val, total / count if count else 0.0, total, count)
        out.update(iteration=rec.cursor, poisoned=bool(rec.status & _lib.LOOP_POISONED), poisoned_at=rec.poisoned_at)
        return out

    def close(self):
        """Drop the graphs; unpin the model if this loop pinned it."""
        self._graphs, self._terms, self.refresh_graph, self._graph, self.terms = {}, {}, None, None, None
        if self._owns_pin and self.model.eval_weights is self.weights:
            self.model.unpin_eval_weights()


# ---- best model and checkpoints (host side, once per epoch) ----------------------------------------------------------------------
START_MIN_LOSS = 10000                                     # train_ae.py:162


def track_best(result, min_loss=START_MIN_LOSS):
    """eval()'s best-model rule (training.py:169-170) on ``ResidentEvalLoop.validate``'s result: -> (is_best, min_loss), is_best when
    ``LB.avg < min_loss``; the new ``min_loss`` is then that average.  A poisoned pass is never the best (the reference exits)."""
    avg = result['LB'][1]
    if result.get('poisoned') or not avg < min_loss:
        return False, min_loss
    return True, avg


def checkpoint(model, optimizer, epoch, iteration, loop=None):
    """The reference's checkpoint dictionary (training.py:95-100, 178-183): {'epoch', 'iter', 'model_state', 'optimizer_state'}.
    loop: the ``ResidentTrainLoop`` that drives the optimiser -- the device's step count is read into ``optimizer.state`` first
    (``loop.meters()``).  It loads through train_ae.py:142-147; a new ``ResidentTrainLoop`` goes on with ``set_epoch(epoch, iter)``.
    eval()'s best-model file takes ``epoch + 1, 0``; train()'s periodic one ``epoch, i + 1``."""
    if loop is not None:
        loop.meters()
    return {'epoch': int(epoch), 'iter': int(iteration), 'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()}


def save_checkpoint(path, model, optimizer, epoch, iteration, loop=None):
    """``torch.save`` of ``checkpoint(...)``: the reference's save_model."""
    torch.save(checkpoint(model, optimizer, epoch, iteration, loop), path)
