"""The callers on either side of the point-flow decoder: the VAE wrapper and the K-component flow-mixture model.

Host-side mirror of lib/networks/models.py:12-265 (Local_Cond_RNVP_MC_Global_RNVP_VAE) and
lib/networks/flow_mixture.py:11-179 (Flow_Mixture_Model) with lib/networks/losses.py:88-170 (FlowMixtureNLL,
Flow_Mixture_Loss): same constructor keywords, attribute names, ``state_dict`` keys (so the reference's checkpoints load
with strict=True), the same nested dict-of-lists outputs from ``forward`` and the same host-side randomness (torch RNG for
the reparameterisations, ``np.random.choice`` for the per-point component draw).

Besides the reference-shaped API there is the path a training loop should use: ``Flow_Mixture_Model.forward_fused`` runs
the encoder (fused HIP kernel in eval), the prior flow, ONE batched launch for the K decoders and returns the tensors
``Flow_Mixture_Loss.fused`` reduces with the mixture-NLL kernel -- no 9*n_flows lists, no B x K Python loop.

The image-conditioned variant, Flow_Mixture_SVR_Model (flow_mixture.py:181-230, single-view reconstruction), is mirrored the
same way: its 4-channel ResNet-18 image encoder (resnet.py) runs on the HIP kernels of csrc/gwtf_resnet.hip in eval mode and
on the library modules in train mode; the image's features give the prior flow its per-shape base Gaussian (``g0_prior``).
``reconstruct_many`` is its batched evaluation path (S images -> S clouds, one partitioned decoder launch); its
``forward_fused(g, p, warmup, images=...)`` is the training path (the loss then reduces the latent terms against the per-image base
Gaussian in one launch, prior.LatentLossRowsFn), which ``training.GraphedTrainStep(..., images_example=...)`` captures.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import GwtfError
from .clouds import make_state
from .decoders import LocalCondRNVPDecoder
from .encoders import FeatureEncoder, PointNetCloudEncoder, WeightsEncoder
from .mixture import MixtureStack, flow_mixture_nll
from .prior import GaussianEntropy, GaussianFlowNLL, GlobalRNVPDecoder
from .resnet import resnet18


class Local_Cond_RNVP_MC_Global_RNVP_VAE(nn.Module):
    """Encoder + prior flow on the latent + ONE point-flow decoder (reference models.py:12-265)."""

    def __init__(self, **kwargs):
        super().__init__()
        g = kwargs.get
        self.train_mode, self.mode, self.deterministic = g('train_mode'), g('util_mode'), g('deterministic')
        self.pc_enc_init_n_channels = g('pc_enc_init_n_channels')
        self.pc_enc_init_n_features = g('pc_enc_init_n_features')
        self.pc_enc_n_features = g('pc_enc_n_features')
        self.g_latent_space_size = g('g_latent_space_size')
        self.g_prior_n_flows, self.g_prior_n_features = g('g_prior_n_flows'), g('g_prior_n_features')
        self.g_posterior_n_layers = g('g_posterior_n_layers')
        self.p_latent_space_size, self.p_prior_n_layers = g('p_latent_space_size'), g('p_prior_n_layers')
        self.p_decoder_n_flows, self.p_decoder_n_features = g('p_decoder_n_flows'), g('p_decoder_n_features')
        self.p_decoder_base_type, self.p_decoder_base_var = g('p_decoder_base_type'), g('p_decoder_base_var')

        self.pc_encoder = PointNetCloudEncoder(self.pc_enc_init_n_channels, self.pc_enc_init_n_features,
                                               self.pc_enc_n_features)
        G = self.g_latent_space_size
        self.g0_prior_mus = nn.Parameter(torch.empty(1, G).normal_(mean=0.0, std=0.033))         # models.py:66-70
        self.g0_prior_logvars = nn.Parameter(torch.empty(1, G).normal_(mean=0.0, std=0.33))
        self.g_prior = GlobalRNVPDecoder(self.g_prior_n_flows, self.g_prior_n_features, G, weight_std=0.01)
        self.g_posterior = FeatureEncoder(self.g_posterior_n_layers, self.pc_enc_n_features[-1], G, deterministic=False,
                                          mu_weight_std=0.0033, mu_bias=0.0, logvar_weight_std=0.033, logvar_bias=0.0)
        P = self.p_latent_space_size
        if self.p_decoder_base_type == 'free':
            self.p_prior = FeatureEncoder(self.p_prior_n_layers, G, P, deterministic=False, mu_weight_std=0.001,
                                          mu_bias=0.0, logvar_weight_std=0.01, logvar_bias=0.0)
        elif self.p_decoder_base_type == 'freevar':
            self.register_buffer('p_prior_mus', torch.zeros((1, P, 1)))
            self.p_prior = FeatureEncoder(self.p_prior_n_layers, G, P, deterministic=True, mu_weight_std=0.01, mu_bias=0.0)
        elif self.p_decoder_base_type == 'fixed':
            self.register_buffer('p_prior_mus', torch.zeros((1, P, 1)))
            self.register_buffer('p_prior_logvar', self.p_decoder_base_var * torch.ones((1, P, 1)))
        self.pc_decoder = self._build_pc_decoder(kwargs)

    def _build_pc_decoder(self, kwargs):
        return LocalCondRNVPDecoder(self.p_decoder_n_flows, self.p_decoder_n_features, self.g_latent_space_size,
                                    weight_std=0.01)

    def train(self, mode=True):
        """nn.Module.train + the data-parallel row-layout cache is dropped on a train <-> eval transition (an evaluation pass
        usually runs another per-rank batch size; dist.row_layout caches per-rank sizes by THIS rank's size only)."""
        if bool(mode) != self.training:
            from .dist import reset_row_layouts
            reset_row_layouts()
        return super().train(mode)

    def reparameterize(self, mu, logvar):
        """mu + exp(0.5 logvar) * N(0,1)   (models.py:99-109; torch RNG of the tensors' device)."""
        std = torch.exp(0.5 * logvar)
        return torch.randn_like(std).mul(std).add_(mu)

    def _pooled_features(self, g_input):
        return self.pc_encoder.forward_max(g_input)          # == torch.max(self.pc_encoder(g_input), dim=2)[0]

    def encode(self, g_input, defer_prior=False):
        """models.py:111-151: posterior from the cloud (training / autoencoding) or a draw from the learned prior
        (generating), pushed through the prior flow; lists are ordered base -> data.
        defer_prior=True (training mode): the prior flow is launched on a side stream and its lists are filled in by
        ``finish_encode(out)`` -- call it after the decoders have been launched (forward_fused does)."""
        B, G = g_input.shape[0], self.g_latent_space_size
        out = {'g_prior_mus': [self.g0_prior_mus.expand(B, G)], 'g_prior_logvars': [self.g0_prior_logvars.expand(B, G)]}
        out['_g0_params'] = (self.g0_prior_mus, self.g0_prior_logvars)        # (the unexpanded base Gaussian, for the fused loss)
        if self.mode in ('training', 'autoencoding'):
            out['g_posterior_mus'], out['g_posterior_logvars'] = self.g_posterior(self._pooled_features(g_input))
            out['g_posterior_samples'] = (self.reparameterize(out['g_posterior_mus'], out['g_posterior_logvars'])
                                          if self.mode == 'training' else out['g_posterior_mus'])
            if defer_prior and hasattr(self.g_prior, 'forward_async'):
                out['_prior_handle'] = self.g_prior.forward_async(out['g_posterior_samples'], mode='inverse')
                return out
            buf_g = self.g_prior(out['g_posterior_samples'], mode='inverse')
            from .prior import stacked_lists
            stacked = stacked_lists(self.g_prior)
            if stacked is not None:
                out['_g_prior_logvars_stacked'] = stacked[2]
            out['g_prior_samples'] = buf_g[0] + [out['g_posterior_samples']]
        elif self.mode == 'generating':
            out['g_prior_samples'] = [self.reparameterize(out['g_prior_mus'][0], out['g_prior_logvars'][0])]
            buf_g = self.g_prior(out['g_prior_samples'][0], mode='direct')
            out['g_prior_samples'] += buf_g[0]
        else:
            raise ValueError(f'unknown util_mode {self.mode!r}')
        out['g_prior_mus'] += buf_g[1]
        out['g_prior_logvars'] += buf_g[2]
        return out

    def finish_encode(self, out):
        """Join the deferred prior flow (see encode(defer_prior=True)) and complete the three prior lists."""
        handle = out.pop('_prior_handle', None)
        if handle is not None:
            buf_g = handle.result()
            from .prior import stacked_lists
            stacked = stacked_lists(self.g_prior)
            if stacked is not None:
                out['_g_prior_logvars_stacked'] = stacked[2]
            out['g_prior_samples'] = buf_g[0] + [out['g_posterior_samples']]
            out['g_prior_mus'] += buf_g[1]
            out['g_prior_logvars'] += buf_g[2]
        return out

    def _base_gaussian(self, g_sample):
        """(mu0, lv0) of the decoder's base distribution, each broadcastable to (B,P,1)  (models.py:169-193)."""
        if self.p_decoder_base_type == 'free':
            mu0, lv0 = self.p_prior(g_sample)
            return mu0.unsqueeze(2), lv0.unsqueeze(2)
        if self.p_decoder_base_type == 'freevar':
            return self.p_prior_mus, self.p_prior(g_sample).unsqueeze(2)
        if self.p_decoder_base_type == 'fixed':
            return self.p_prior_mus, self.p_prior_logvar
        raise ValueError(f'unknown p_decoder_base_type {self.p_decoder_base_type!r}')

    def _base_gaussian_repeated(self, g_sample, times):
        """_base_gaussian evaluated ONCE with the buffer side effects of `times` evaluations on the same batch (the reference
        evaluates p_prior inside its loop over the K components, models.py:169-193 in flow_mixture.py:163-166): every tracked
        BatchNorm of p_prior in train mode gets running = (1-m) running + m batch applied `times` times and num_batches_tracked
        += times (FeatureEncoder.forward(bn_updates=times))."""
        if times <= 1 or self.p_decoder_base_type == 'fixed':
            return self._base_gaussian(g_sample)
        if self.p_decoder_base_type == 'free':
            mu0, lv0 = self.p_prior(g_sample, bn_updates=times)
            return mu0.unsqueeze(2), lv0.unsqueeze(2)
        return self.p_prior_mus, self.p_prior(g_sample, bn_updates=times).unsqueeze(2)

    def one_flow_decode(self, p_input, g_sample, pc_decoder, n_sampled_points):
        """models.py:153-207: lists for ONE component (inverse on p_input when training, direct on a base draw otherwise)."""
        B, P = g_sample.shape[0], self.p_latent_space_size
        mu0, lv0 = self._base_gaussian(g_sample)
        out = {'p_prior_mus': [mu0.expand(B, P, n_sampled_points)], 'p_prior_logvars': [lv0.expand(B, P, n_sampled_points)]}
        if self.mode == 'training':
            buf = pc_decoder(p_input, g_sample, mode='inverse')
            out['p_prior_samples'] = buf[0] + [p_input]
        else:
            out['p_prior_samples'] = [self.reparameterize(out['p_prior_mus'][0], out['p_prior_logvars'][0])]
            buf = pc_decoder(out['p_prior_samples'][0], g_sample, mode='direct')
            out['p_prior_samples'] += buf[0]
        out['p_prior_mus'] += buf[1]
        out['p_prior_logvars'] += buf[2]
        return out

    def decode(self, p_input, g_sample, n_sampled_points, labeled_samples=False, warmup=False):
        """Single-decoder decode (the body the reference keeps commented out at models.py:209-223)."""
        return self.one_flow_decode(p_input, g_sample, self.pc_decoder, n_sampled_points), None

    def forward(self, g_input, p_input, images=None, n_sampled_points=None, labeled_samples=False, warmup=False):
        """models.py:224-265."""
        size = p_input.shape[2] if n_sampled_points is None else n_sampled_points
        if images is not None and self.train_mode == 'p_rnvp_mc_g_rnvp_vae_ic':
            raise NotImplementedError('image-conditioned encoding (ResNet-18) is outside the point-flow path')
        # training: the prior flow (a latency chain on one compute unit) runs on a side stream beside the decoders, as in
        # forward_fused; its lists are joined in before the outputs are handed back
        output_encoder = self.encode(g_input, defer_prior=self.mode == 'training')
        g_sample = (output_encoder['g_posterior_samples'] if self.mode in ('training', 'autoencoding')
                    else output_encoder['g_prior_samples'][-1])
        if labeled_samples:
            samples, labels, logits = self.decode(p_input, g_sample, size, labeled_samples, warmup)
            return self.finish_encode(output_encoder), samples, labels, logits
        output_decoder, logits = self.decode(p_input, g_sample, size, labeled_samples, warmup)
        return self.finish_encode(output_encoder), output_decoder, logits


class EvalWeights:
    """model.pin_eval_weights(): every packed-weight cache on the eval density path of a ``Flow_Mixture_Model`` in persistent device
    buffers -- the K decoders' (mixture.PinnedStackWeights) and the cloud encoder's (encoders.PinnedEncoderWeights).  Every other
    module of that path (Gaussian heads, prior flow, mixture-weight encoder, loss) reads parameters and running statistics in place
    (DESIGN.md section 4b).  ``refresh()``: five launches into the same storage, no allocation, capturable."""

    def __init__(self, model):
        self.stack = model.mixture_stack().pin()
        self.encoder = model.pc_encoder.pin()

    def __reduce__(self):
        """copy.deepcopy / pickle of a pinned model: the copy is not pinned."""
        return (type(None), ())

    def refresh(self):
        self.stack.refresh()
        self.encoder.refresh()
        return self

    def buffers(self):
        """name -> pinned tensor (their data_ptr()s never change)."""
        return {**self.stack.buffers(), **self.encoder.buffers()}


class Flow_Mixture_Model(Local_Cond_RNVP_MC_Global_RNVP_VAE):
    """K point-flow decoders with per-shape mixture weights (reference flow_mixture.py:11-179)."""

    def __init__(self, **kwargs):
        self.n_components = kwargs['n_components']
        self.params_reduce_mode = kwargs['params_reduce_mode']
        self.weights_type = kwargs['weights_type']
        super().__init__(**kwargs)
        # registered after the base class's parameters, as in the reference (state_dict order)
        self.mixture_weights_logits = nn.Parameter(torch.zeros(self.n_components), requires_grad=True)
        self.mixture_weights_encoder = WeightsEncoder(3, self.g_latent_space_size, self.n_components, deterministic=True,
                                                      mu_weight_std=0.001, mu_bias=0.0, logvar_weight_std=0.01,
                                                      logvar_bias=0.0)
        self._stack = None

    def _build_pc_decoder(self, kwargs):
        n_flows, f = self._get_decoder_params()
        return nn.ModuleList([LocalCondRNVPDecoder(n_flows, f, self.g_latent_space_size, weight_std=0.01)
                              for _ in range(self.n_components)])

    # -- parameter-budget rules (flow_mixture.py:44-102) --------------------------------------------------------------
    def _get_decoder_params(self):
        n = self.n_components
        if n == 1 or self.params_reduce_mode == 'none':
            return self.p_decoder_n_flows, self.p_decoder_n_features
        count = LocalCondRNVPDecoder.get_param_count
        if self.params_reduce_mode == 'depth_and_feature':
            depth = math.ceil(self.p_decoder_n_flows / math.sqrt(n))
            f, _ = self._get_p_decoder_n_features(depth)
        elif self.params_reduce_mode == 'depth_first':
            depth = math.ceil(self.p_decoder_n_flows / n)
            f, _ = self._get_p_decoder_n_features(depth)
        elif self.params_reduce_mode == 'feature_first':
            depth = self.p_decoder_n_flows
            f, (over, budget, total) = self._get_p_decoder_n_features(depth)
            if over:
                while total > budget:
                    depth -= 1
                    total = count(depth, f, self.g_latent_space_size) * n
        else:
            raise ValueError(f'Unknown params_reduce_mode: {self.params_reduce_mode}')
        return depth, f

    def _get_p_decoder_n_features(self, depth):
        f, n, G = self.p_decoder_n_features, self.n_components, self.g_latent_space_size
        count = LocalCondRNVPDecoder.get_param_count
        budget = count(self.p_decoder_n_flows, f, G)
        total = budget * n
        while total > budget and f > 4:
            f -= 1
            total = count(depth, f, G) * n
        return f, (total > budget, budget, total)

    # -- mixture weights and decoding (flow_mixture.py:104-179) ------------------------------------------------------
    def get_weights(self, g_sample, warmup=False):
        if warmup or self.weights_type == 'global_weights':
            return self.mixture_weights_logits.unsqueeze(0).expand(g_sample.shape[0], self.n_components)
        if self.weights_type == 'learned_weights':
            return self.mixture_weights_encoder(g_sample)
        raise ValueError(f'unknown weights_type {self.weights_type!r}')

    def _draw_components(self, logits_row, n_points):
        """np.random.choice over the normalised weights of ONE shape (flow_mixture.py:146-160) -> per-point component."""
        w = np.exp(logits_row.detach().cpu().numpy())
        return np.random.choice(range(self.n_components), size=n_points, p=w / w.sum())

    def decode(self, p_input, g_sample, n_sampled_points, labeled_samples=False, warmup=False):
        logits = self.get_weights(g_sample, warmup)
        K = self.n_components
        if self.mode == 'training':
            sizes = [n_sampled_points] * K
        else:
            assert p_input.shape[0] == 1                     # evaluation feeds one shape at a time (flow_mixture.py:146)
            flows_idx = self._draw_components(logits[0], n_sampled_points)
            sizes = [int((flows_idx == t).sum()) for t in range(K)]
        # literal_k_loop: this mirror's own shortcut off -- the K decoders are called one at a time exactly as the reference's loop
        # does (flow_mixture.py:163-166), which is what a maintainer who only swaps the decoder import runs (tools/bench_train.py
        # --api swap; the decoders' sibling batching, decoders._SiblingGroup, then does the batching below the API)
        batched = self.mode == 'training' and not getattr(self, 'literal_k_loop', False)
        output_decoder = self._decode_training_batched(p_input, g_sample, sizes) if batched else None
        if output_decoder is None:
            output_decoder = [self.one_flow_decode(p_input, g_sample, self.pc_decoder[i], sizes[i]) for i in range(K)]
        if not labeled_samples:
            return output_decoder, logits
        samples = torch.zeros_like(p_input)
        labels = torch.zeros(p_input.size(0), p_input.size(2))
        for t in range(K):
            mask = torch.from_numpy(flows_idx == t)
            samples[:, :, mask] = output_decoder[t]['p_prior_samples'][-1]
            labels[:, mask] = t + 1
        return samples, labels, logits

    def _decode_training_batched(self, p_input, g_sample, sizes):
        """The K one_flow_decode calls of the training pass (flow_mixture.py:163-166) as ONE pass of the K-batched train pipeline:
        the same K dicts of lists (entries are slices of stacked tensors).  None when it does not apply (eval-mode BatchNorm, CPU
        tensors, sub-sampled clouds): the per-decoder calls then run."""
        if not p_input.is_cuda or any(sz != p_input.shape[2] for sz in sizes) or not self.pc_decoder[0].training:
            return None
        res = self.mixture_stack().forward_all_lists(p_input, g_sample, mode='inverse')
        if res is None:
            return None
        z, logdet, (ps, mus, lvs) = res                          # (K,B,3,N), (K,B,3,N), (K,C,B,3,N) each
        B, P, n = g_sample.shape[0], self.p_latent_space_size, p_input.shape[2]
        mu0, lv0 = self._base_gaussian_repeated(g_sample, self.n_components)
        out = []
        for k in range(self.n_components):
            # slot 0 of the samples IS the stack's output and sum(logvars[1:]) IS its log-det: handing the loss those two tensors
            # (the list entries hold the same values) keeps the gradient off the per-slot route, whose backward would materialise
            # a (K, C, B, 3, N) gradient tensor per list
            out.append({'p_prior_mus': [mu0.expand(B, P, n)] + list(mus[k].unbind(0)),
                        'p_prior_logvars': [lv0.expand(B, P, n)] + list(lvs[k].unbind(0)),
                        'p_prior_samples': [z[k]] + list(ps[k].unbind(0))[1:] + [p_input],
                        '_sum_flow_logvars': logdet[k]})
        return out

    # -- the fused path ------------------------------------------------------------------------------------------------
    def mixture_stack(self):
        if self._stack is None:
            self._stack = MixtureStack(self.pc_decoder)
        return self._stack

    # -- eval packings pinned to persistent buffers (an eval graph that survives training: training.ResidentEvalLoop) ----------
    eval_weights = None               # the EvalWeights this model is pinned to

    def pin_eval_weights(self):
        """Pin every packed-weight cache of the eval density path to persistent device buffers and return the set (EvalWeights; the
        one in place when the model is pinned already).  While pinned, the eval pass reads those buffers whatever the version keys say
        -- through model.train() / model.eval() / invalidate_packed_weights() -- and sees a parameter change only after
        ``refresh()``.  The set describes the parameters' current storage: ``.to()`` / ``.cuda()`` unpin."""
        if getattr(self, 'img_encoder', None) is not None:
            raise NotImplementedError('an image-conditioned model cannot be pinned: the ResNet image encoder packs its weights on the '
                                      'host (resnet.ResNet._pack_host)')
        if self.eval_weights is None:
            self.__dict__['eval_weights'] = EvalWeights(self)
        return self.eval_weights

    def unpin_eval_weights(self):
        """Back to the version-keyed caches (which are dropped: they may predate what happened while the model was pinned)."""
        if self.__dict__.get('eval_weights') is None:
            return
        self.__dict__['eval_weights'] = None
        self.mixture_stack().unpin()
        self.pc_encoder.unpin()
        for mod in self.modules():
            if hasattr(mod, 'invalidate_packed_weights'):
                mod.invalidate_packed_weights()

    def _apply(self, fn, *args, **kwargs):
        self.unpin_eval_weights()         # .to() / .cuda() / .double(): the pinned pointer tables name storage that is replaced
        return super()._apply(fn, *args, **kwargs)

    def forward_fused(self, g_input, p_input, warmup=False):
        """Training / density pass without the list API: -> (output_encoder, dec) with dec = {z, logdet (K,B,3,N); mu0, lv0
        (K,B,P); logits (B,K)}: everything ``Flow_Mixture_Loss.fused`` needs.  Same arithmetic as ``forward`` in 'training'
        mode (one encoder pass, the prior flow, every component on every point in ONE batched launch when BatchNorm is in
        eval mode and no gradient is needed; per component otherwise)."""
        if self.mode != 'training':
            raise ValueError("forward_fused is the density ('training') pass; use sample_fused for generation")
        # the prior flow runs beside the decoders (side stream)
        return self._fused_after_encode(self.encode(g_input, defer_prior=True), p_input, warmup)

    def _fused_after_encode(self, output_encoder, p_input, warmup):
        """forward_fused behind the encoder: mixture weights, the decoders' base Gaussian, the K decoders, the prior flow joined."""
        g_sample = output_encoder['g_posterior_samples']
        logits = self.get_weights(g_sample, warmup)
        B, K, P = g_sample.shape[0], self.n_components, self.p_latent_space_size
        # The reference evaluates p_prior once per component (models.py:169-193 inside the K loop of flow_mixture.py:163-166): K
        # identical outputs, and K running-statistic updates with the same batch statistics.  One evaluation here; its BatchNorm
        # modules replay the other K - 1 buffer updates (same values as K passes would leave, to rounding).
        m, v = self._base_gaussian_repeated(g_sample, K)
        # (K views of the one evaluation: no copy here, and ONE sum over K in the backward where a stack's would be K - 1 adds)
        mu0 = m.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P)
        lv0 = v.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P)
        z, logdet = self.mixture_stack().forward_all(p_input, g_sample, mode='inverse')
        self.finish_encode(output_encoder)
        return output_encoder, {'z': z, 'logdet': logdet, 'mu0': mu0, 'lv0': lv0, 'logits': logits}

    @torch.no_grad()
    def sample_fused(self, g_sample, n_points, return_labels=False):
        """Generation for ONE shape (flow_mixture.py:146-177 without the K Python passes): draw each point's component,
        draw base samples, push every point through its own component in one launch.  -> (1,3,n_points)[, labels]."""
        assert g_sample.shape[0] == 1
        logits = self.get_weights(g_sample)
        flows_idx = np.sort(self._draw_components(logits[0], n_points))       # points laid out component by component
        counts = [int((flows_idx == t).sum()) for t in range(self.n_components)]
        P = self.p_latent_space_size
        mu0, lv0 = self._base_gaussian(g_sample)
        z0 = self.reparameterize(mu0.expand(1, P, n_points), lv0.expand(1, P, n_points))
        x, _ = self.mixture_stack().forward_partition(z0, g_sample, counts, mode='direct')
        if return_labels:
            return x, torch.from_numpy(flows_idx + 1).to(x.device).unsqueeze(0).float()
        return x

    @staticmethod
    def _padded_partition(labels, K):
        """labels (S, n) ints in [0, K): every sample's per-point component.  -> counts (K,) = the LARGEST count of each component
        over the samples, and index tensors: slot (S, n) = where point i of sample s sits in the padded component-major layout
        (points of component k of every sample occupy [start_k, start_k + counts_k), the sample's own in front)."""
        S, n = labels.shape
        per = np.stack([(labels == k).sum(1) for k in range(K)], axis=1)            # (S, K)
        counts = per.max(0)
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        slot = np.empty((S, n), np.int64)
        for s in range(S):
            order = np.argsort(labels[s], kind='stable')                                # points of component 0 first, ...
            rank_in_comp = np.concatenate([np.arange(c) for c in per[s]]) if n else np.zeros(0, np.int64)
            slot[s, order] = starts[labels[s][order]] + rank_in_comp
        return counts, slot

    @torch.no_grad()
    def sample_many(self, g_samples, n_points, return_labels=False):
        """Generation for S shapes in ONE launch (the reference samples one shape per call, flow_mixture.py:146-177; the decoder
        launch for a single 2048-point shape is latency-bound at ~36 us -- bench.py k16_b1 -- where a batch runs 22 x that rate).
        Each sample draws its points' components from its own mixture weights (np.random.choice, sample by sample, as the
        reference's loop would); the points are laid out component by component with every component's segment padded to its
        largest count over the batch (a few per cent of padding: multinomial counts concentrate), pushed through their own
        component by one partitioned launch, and gathered back in the points' original order.
        -> (S, 3, n_points)[, labels (S, n_points) in 1..K]."""
        S, K, P = g_samples.shape[0], self.n_components, self.p_latent_space_size
        logits = self.get_weights(g_samples)
        labels = np.stack([self._draw_components(logits[s], n_points) for s in range(S)])
        mu0, lv0 = self._base_gaussian(g_samples)
        z0 = self.reparameterize(mu0.expand(S, P, n_points), lv0.expand(S, P, n_points))
        x = self._decode_partitioned_many(z0, g_samples, labels)
        if return_labels:
            return x, torch.from_numpy(labels + 1).to(x.device).float()
        return x

    @torch.no_grad()
    def generate_many(self, g_samples, n_points, return_labels=False, state=None, explicit=None, out=None):
        """Generation for S shapes with NO host round trip between the latent codes and the clouds: the mixture logits, the base
        Gaussian and the FiLM records stay on the device, one routing launch draws every point's component and base sample (Philox,
        clouds.make_state's (seed, call) record, which the launch advances) and lays the points out in tiles of their components,
        one routed stack launch sends every point through its own component (csrc/gwtf_route.hip, gwtf_stack.hip ROUTED).
        -> (S, 3, n_points)[, labels (S, n_points) in 1..K as float].  state=None: a state the model keeps (seed 0).
        explicit: {'words' (S,n) int32 bits | 'labels_in' (S,n) int32 in [0,K), 'normals' | 'z0_in' (S,3,n) float32} replaces the
        draws (include/gwtf.h).  out: the result tensor.  After one eager call the same call can be captured in a graph: every
        replay draws fresh clouds.  sample_many keeps the reference's np.random draws; this path has its own random stream."""
        S, K = g_samples.shape[0], self.n_components
        n, dev = int(n_points), g_samples.device
        stack = self.mixture_stack()
        stack._routed_ready(g_samples)
        if dev.type != 'cuda':
            raise GwtfError(f'g_samples lives on {dev}: generation runs on a HIP device only, there is no CPU path')
        if out is None:
            out = torch.empty(S, 3, n, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (S, 3, n) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise GwtfError(f'out must be a contiguous float32 tensor of shape {(S, 3, n)} on {dev}')
        if state is None:
            if getattr(self, '_generate_state', None) is None or self._generate_state.device != dev:
                self._generate_state = make_state(0, dev)
            state = self._generate_state
        ex = dict(explicit or {})
        unknown = set(ex) - {'words', 'labels_in', 'normals', 'z0_in'}
        if unknown:
            raise GwtfError(f'explicit: unknown keys {sorted(unknown)}')
        logits = self.get_weights(g_samples).contiguous().float()
        mu0, lv0 = self._base_gaussian(g_samples)
        work = stack._routed_work(S, n, dev)
        _lib.mixture_route(work, logits=logits, mu0=mu0[:, :, 0].contiguous().float(), lv0=lv0[:, :, 0].contiguous().float(),
                           state=state, **ex)
        stack.launch_routed(work, g_samples, out=out)
        if return_labels:
            return out, (work['labels'] + 1).float()
        return out

    @torch.no_grad()
    def autoencode_many(self, g_clouds, n_points, return_labels=False, state=None):
        """S clouds (S, 3, N) -> S clouds of ``n_points`` points decoded from their own latent codes: the autoencoding twin of
        Flow_Mixture_SVR_Model.reconstruct_many (the reference calls `model(...)` in 'autoencoding' mode batch by batch,
        evaluating.py:93).  The codes are encode(...)['g_posterior_samples'], in this mode the posterior means (no draw).  With a
        state (clouds.make_state) the decoder step is ``generate_many`` -- components and base samples drawn on the device from that
        state, no host round trip -- and ``sample_many`` (np.random component draws, sample by sample) otherwise.
        -> (S, 3, n_points)[, labels (S, n_points) in 1..K]."""
        if self.mode != 'autoencoding':
            raise GwtfError(f"autoencode_many needs a model in 'autoencoding' mode (model.mode / util_mode), got {self.mode!r}")
        g = self.encode(g_clouds)['g_posterior_samples']
        if state is not None:
            return self.generate_many(g, n_points, return_labels, state=state)
        return self.sample_many(g, n_points, return_labels)

    _SWEEP_WEIGHTS = tuple(float(w) for w in np.float32(np.arange(1, 10, 1) / 10))        # evaluating.py:340

    def _sweep_constant(self, key, make, dev):
        """A small device tensor built from host values once per (key, device): a captured call copies nothing from the host."""
        cache = self.__dict__.setdefault('_sweep_constants', {})
        if (key, str(dev)) not in cache:
            cache[(key, str(dev))] = make().to(dev)
        return cache[(key, str(dev))]

    @torch.no_grad()
    def interpolate_many(self, codes_a, codes_b, n_points, weights=None, flow_idx=None, return_labels=False, state=None, explicit=None,
                         out=None):
        """Latent sweeps between S pairs of codes in one pass (the reference's `--interpolation` / `--interpolate_one_flow`, whose code
        it keeps inside a string literal, evaluating.py:268-382): row (s, t) decodes (1. - w_t) * codes_a[s] + w_t * codes_b[s]
        (float32, that expression; weights: T values or a (T,) float32 device tensor, default np.arange(1, 10) / 10).  The T steps of
        a shape SHARE their draws -- point i has the same label word and the same three normals at every step, those generate_many
        draws for shape s at the same (seed, call) -- so every step is a sample of the model at its code and a point moves
        continuously along the sweep.  The mixture logits of a row come from its own code.  flow_idx (components, None: all): only
        these take the row's interpolated code, for their base Gaussian and their FiLM conditioning; every other component stays at
        codes_a[s] (one_flow_decode(..., interpolated_codes | codes1, ...), evaluating.py:359-365).
        The heads run once on the R = S * T codes (and once on codes_a with flow_idx); then one routing launch
        (gwtf_mixture_route_sweep), one FiLM launch and one routed stack launch: no host round trip, capturable in a graph after one
        eager call, every replay drawing fresh clouds; one call advances the state by one.  explicit: generate_many's keys, (S, ...)
        tensors shared by the T rows of a shape.  out: the (S, T, 3, n) result tensor.
        -> (S, T, 3, n_points)[, labels (S, T, n_points) in 1..K as float]."""
        for t, name in ((codes_a, 'codes_a'), (codes_b, 'codes_b')):
            if not torch.is_tensor(t) or t.dim() != 2:
                raise GwtfError(f'{name} must be an (S, G) tensor')
        G, K = self.g_latent_space_size, self.n_components
        if codes_a.shape != codes_b.shape or codes_a.shape[1] != G or codes_a.shape[0] < 1:
            raise GwtfError(f'codes_a and codes_b must both be (S, {G}), got {tuple(codes_a.shape)} and {tuple(codes_b.shape)}')
        S, n, dev = codes_a.shape[0], int(n_points), codes_a.device
        if codes_b.device != dev:
            raise GwtfError(f'codes_a lives on {dev}, codes_b on {codes_b.device}')
        if torch.is_tensor(weights):
            if weights.dim() != 1 or weights.dtype != torch.float32:
                raise GwtfError('weights must be a sequence of numbers or a one-dimensional float32 tensor')
            T = weights.shape[0]
        else:
            weights = self._SWEEP_WEIGHTS if weights is None else tuple(float(w) for w in weights)
            T = len(weights)
        if T < 1:
            raise GwtfError('weights is empty: a sweep has at least one step')
        if flow_idx is not None:
            flow_idx = tuple(sorted({int(k) for k in flow_idx}))
            if any(k < 0 or k >= K for k in flow_idx):
                raise GwtfError(f'flow_idx {list(flow_idx)} names components outside [0, {K})')
        stack = self.mixture_stack()
        stack._routed_ready(codes_a)
        if dev.type != 'cuda':
            raise GwtfError(f'the codes live on {dev}: generation runs on a HIP device only, there is no CPU path')
        R = S * T
        if out is None:
            out = torch.empty(S, T, 3, n, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (S, T, 3, n) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise GwtfError(f'out must be a contiguous float32 tensor of shape {(S, T, 3, n)} on {dev}')
        ex = dict(explicit or {})
        unknown = set(ex) - {'words', 'labels_in', 'normals', 'z0_in'}
        if unknown:
            raise GwtfError(f'explicit: unknown keys {sorted(unknown)}')
        if state is None:
            if getattr(self, '_generate_state', None) is None or self._generate_state.device != dev:
                self._generate_state = make_state(0, dev)
            state = self._generate_state
        if torch.is_tensor(weights):
            w = weights.to(dev)
        else:
            w = self._sweep_constant(('weights', weights), lambda: torch.tensor(weights, dtype=torch.float32), dev)
        w = w.view(1, T, 1)
        a, b = codes_a.float().unsqueeze(1), codes_b.float().unsqueeze(1)
        codes = ((1. - w) * a + w * b).reshape(R, G)
        logits = self.get_weights(codes).contiguous().float()

        def base_rows(g):                                        # (rows or 1, 3) each
            mu0, lv0 = self._base_gaussian(g)
            return [t.expand(-1, self.p_latent_space_size, 1)[:, :, 0].float() for t in (mu0, lv0)]
        mu0, lv0 = base_rows(codes)
        g = codes
        if flow_idx is not None:
            # (K, R, .) tables: the chosen components at the row's code, the others at codes_a[s]
            own = self._sweep_constant(('flow_idx', flow_idx, K),
                                       lambda: torch.tensor([k in flow_idx for k in range(K)]), dev).view(K, 1, 1)
            at_a = lambda t: t if t.shape[0] == 1 else t.unsqueeze(1).expand(S, T, t.shape[1]).reshape(R, t.shape[1])
            mu0, lv0 = (torch.where(own, x.expand(R, 3).unsqueeze(0), at_a(y).expand(R, 3).unsqueeze(0))
                        for x, y in zip((mu0, lv0), base_rows(codes_a.float())))
            g = torch.where(own, codes.unsqueeze(0), at_a(codes_a.float()).unsqueeze(0))
        work = stack._routed_work(R, n, dev)
        _lib.mixture_route_sweep(work, group=T, logits=logits, mu0=mu0.contiguous(), lv0=lv0.contiguous(), state=state, **ex)
        stack.launch_routed(work, g, out=out.view(R, 3, n))
        if return_labels:
            return out, (work['labels'] + 1).float().view(S, T, n)
        return out

    @torch.no_grad()
    def upsample_many(self, clouds, n_points, return_labels=False, state=None):
        """S sparse clouds (S, 3, N) -> S dense clouds of ``n_points`` points with a component label per point: the reference's
        `--sampling` branch (`sample`, evaluating.py:384-457, kept inside a string literal there).  The codes are the posterior means
        of the clouds (encode(...)['g_posterior_mus']), taken from the cloud encoder and the posterior head directly, so that --
        unlike autoencode_many -- the call works in every ``model.mode``; the decoder step is ``generate_many``.
        -> (S, 3, n_points)[, labels (S, n_points) in 1..K]."""
        g = self.g_posterior(self._pooled_features(clouds))[0]
        return self.generate_many(g, n_points, return_labels, state=state)

    @torch.no_grad()
    def assign_many(self, clouds, codes=None, want_resp=False, parts=None, n_parts=None, table=None, skipped=None, out=None):
        """The inference direction of the mixture for B observed clouds (B, 3, N) on the device: which component explains each point,
        and how likely the point is.  For every point the responsibility r_k = softmax_k(log w_k + log p_k(x | code)) of the K
        components (the per-component terms of FlowMixtureNLL, losses.py:101-122) reduced by one launch (csrc/gwtf_assign.hip) behind
        the batched density launch.  codes (B, G): the latent codes the components are conditioned on; default the posterior means of
        ``clouds``, taken as upsample_many takes them, so that the call works in every ``model.mode`` -- codes of OTHER clouds label
        held-out points of the same shapes.
        -> {'log_density' (B, N) float32 = logsumexp_k, 'labels' (B, N) int32 in [0, K) (argmax, lowest k on a tie; -1 where the
        log-density is not finite; the type forward_routed's labels take), 'confidence' (B, N) = r of the label, 'resp' (B, K, N) or
        None, 'counts' (B, K) int32, 'invalid' (B,) int32}.  parts (B, N) int32 with n_parts: the (label, part) contingency is ADDED
        to table (K, n_parts) int64 and the points left out to skipped (1,) int64, both returned as well (made when not passed).
        out: the dict of an earlier call, written in place.  After one eager call the same call with out= can be captured in a graph."""
        if _stack_training(self):
            raise NotImplementedError('assign_many is an evaluation path (eval-mode BatchNorm in the decoders); call .eval()')
        if not torch.is_tensor(clouds) or clouds.device.type != 'cuda':
            raise GwtfError('clouds must live on a HIP device; there is no CPU path')
        if clouds.dim() != 3 or clouds.shape[1] != 3:
            raise GwtfError(f'clouds must be (B, 3, N), got {tuple(clouds.shape)}')
        B, K, P = clouds.shape[0], self.n_components, self.p_latent_space_size
        if codes is None:
            codes = self.g_posterior(self._pooled_features(clouds))[0]
        elif not torch.is_tensor(codes) or codes.device != clouds.device or tuple(codes.shape) != (B, self.g_latent_space_size):
            raise GwtfError(f'codes must be ({B}, {self.g_latent_space_size}) on {clouds.device}')
        logits = self.get_weights(codes).contiguous().float()
        m, v = self._base_gaussian(codes)
        mu0 = m.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P).contiguous().float()
        lv0 = v.expand(B, P, 1)[:, :, 0].unsqueeze(0).expand(K, B, P).contiguous().float()
        z, logdet = self.mixture_stack().forward_all(clouds, codes, mode='inverse')
        return _lib.mixture_assign(z, logdet, mu0, lv0, logits, want_resp=want_resp, parts=parts, n_parts=n_parts, table=table,
                                   skipped=skipped, out=out)

    def _decode_partitioned_many(self, z0, g_samples, labels):
        """z0 (S, 3, n) base samples, labels (S, n) numpy: point i of sample s through component labels[s, i] -> (S, 3, n)."""
        S, _, n = z0.shape
        counts, slot = self._padded_partition(np.asarray(labels), self.n_components)
        n_pad = int(counts.sum())
        slot_t = torch.from_numpy(slot).to(z0.device)
        zp = torch.zeros(S, 3, n_pad, device=z0.device, dtype=torch.float32)
        zp.scatter_(2, slot_t.unsqueeze(1).expand(S, 3, n), z0.float())
        xp, _ = self.mixture_stack().forward_partition(zp, g_samples, [int(c) for c in counts], mode='direct')
        return xp.gather(2, slot_t.unsqueeze(1).expand(S, 3, n))


class Flow_Mixture_SVR_Model(Flow_Mixture_Model):
    """Single-view reconstruction (reference flow_mixture.py:181-230): an image encoder and a Gaussian head give the prior flow a
    per-shape base distribution.  'training': the posterior comes from the cloud and runs through the prior flow inverse (its
    base is the image's Gaussian); 'reconstruction': the image's base mean runs through the prior flow direct (no draw).
    ``model.mode`` may be switched at run time (training.py:274)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        G = self.g_latent_space_size
        self.img_encoder = resnet18(num_classes=G)
        self.g_prior_n_layers = kwargs.get('g_prior_n_layers')
        self.g0_prior = FeatureEncoder(self.g_prior_n_layers, G, G, deterministic=False, mu_weight_std=0.0033, mu_bias=0.0,
                                       logvar_weight_std=0.033, logvar_bias=0.0)
        # the base class's learned global base Gaussian is replaced by the per-image one: out of the state_dict, as in the reference
        self.g0_prior_mus = None
        self.g0_prior_logvars = None

    def encode(self, g_input, images, defer_prior=False, fused_base=False):
        """flow_mixture.py:199-230 -> the encoder dict; lists are ordered base -> data.  No '_g0_params': the base is per row.
        fused_base=True (forward_fused): the per-row base Gaussian is also handed over as out['_g0_rows'] = (mus, logvars), the
        tensors of g_prior_mus[0] / g_prior_logvars[0], and the loss reduces its latent terms in one launch
        (prior.LatentLossRowsFn); without it the loss takes its list path."""
        if images is None:
            raise ValueError('Flow_Mixture_SVR_Model.encode needs images')
        if self.mode not in ('training', 'reconstruction'):
            raise ValueError(f'unknown util_mode {self.mode!r} for single-view reconstruction '
                             "(expected 'training' or 'reconstruction')")
        out = {}
        mus, logvars = self.g0_prior(self.img_encoder(images))
        out['g_prior_mus'], out['g_prior_logvars'] = [mus], [logvars]
        if fused_base:
            out['_g0_rows'] = (mus, logvars)
        if self.mode == 'training':
            out['g_posterior_mus'], out['g_posterior_logvars'] = self.g_posterior(self._pooled_features(g_input))
            out['g_posterior_samples'] = self.reparameterize(out['g_posterior_mus'], out['g_posterior_logvars'])
            if defer_prior and hasattr(self.g_prior, 'forward_async'):
                out['_prior_handle'] = self.g_prior.forward_async(out['g_posterior_samples'], mode='inverse')
                return out
            buf_g = self.g_prior(out['g_posterior_samples'], mode='inverse')
            from .prior import stacked_lists
            stacked = stacked_lists(self.g_prior)
            if stacked is not None:
                out['_g_prior_logvars_stacked'] = stacked[2]
            out['g_prior_samples'] = buf_g[0] + [out['g_posterior_samples']]
        else:
            out['g_prior_samples'] = [mus]
            buf_g = self.g_prior(mus, mode='direct')
            out['g_prior_samples'] += buf_g[0]
        out['g_prior_mus'] += buf_g[1]
        out['g_prior_logvars'] += buf_g[2]
        return out

    def forward(self, g_input, p_input, images=None, n_sampled_points=None, labeled_samples=False, warmup=False):
        """models.py:224-265 with the image branch taken."""
        if self.mode not in ('training', 'reconstruction'):
            raise ValueError(f'unknown util_mode {self.mode!r} for single-view reconstruction '
                             "(expected 'training' or 'reconstruction')")
        size = p_input.shape[2] if n_sampled_points is None else n_sampled_points
        output_encoder = self.encode(g_input, images, defer_prior=self.mode == 'training')
        g_sample = (output_encoder['g_posterior_samples'] if self.mode == 'training'
                    else output_encoder['g_prior_samples'][-1])
        if labeled_samples:
            samples, labels, logits = self.decode(p_input, g_sample, size, labeled_samples, warmup)
            return self.finish_encode(output_encoder), samples, labels, logits
        output_decoder, logits = self.decode(p_input, g_sample, size, labeled_samples, warmup)
        return self.finish_encode(output_encoder), output_decoder, logits

    def forward_fused(self, g_input, p_input, warmup=False, images=None):
        """Flow_Mixture_Model.forward_fused with the image branch: the base class's body behind the SVR encoder, whose per-row
        base Gaussian reaches ``Flow_Mixture_Loss.fused`` as '_g0_rows'.  -> (output_encoder, dec)."""
        if self.mode != 'training':
            raise ValueError("forward_fused is the density ('training') pass; use reconstruct_many for reconstruction")
        if images is None:
            raise ValueError('Flow_Mixture_SVR_Model.forward_fused needs images')
        return self._fused_after_encode(self.encode(g_input, images, defer_prior=True, fused_base=True), p_input, warmup)

    @torch.no_grad()
    def reconstruct_many(self, images, n_points, return_labels=False, state=None):
        """S images -> S clouds (the reference reconstructs one image per call, evaluating.py:94-96): the image encoder on all S
        (HIP in eval mode), the g0_prior means through the prior flow direct, then ``sample_many``'s partitioned decoder launch.
        Component draws are taken sample by sample (np.random.choice), in the order S calls of ``forward`` with B = 1 take them.
        With a state (clouds.make_state) the decoder step is ``generate_many`` instead: components and base samples drawn on the
        device from that state, no host round trip.
        -> (S, 3, n_points)[, labels (S, n_points) in 1..K]."""
        mus, _ = self.g0_prior(self.img_encoder(images))
        g = self.g_prior(mus, mode='direct')[0][-1]
        if state is not None:
            return self.generate_many(g, n_points, return_labels, state=state)
        return self.sample_many(g, n_points, return_labels)

    @torch.no_grad()
    def assign_many(self, clouds, images=None, codes=None, **kwargs):
        """Flow_Mixture_Model.assign_many with the codes of single-view reconstruction: with ``images`` (B, 4, H, W) the codes are the
        ones reconstruct_many decodes from (the g0_prior means of the image features through the prior flow direct).  Exactly one of
        ``images`` and ``codes``: this model has no cloud-only route to a code outside training."""
        if (images is None) == (codes is None):
            raise GwtfError('assign_many needs exactly one of images and codes')
        if images is not None:
            if _stack_training(self):
                raise NotImplementedError('assign_many is an evaluation path (eval-mode BatchNorm in the decoders); call .eval()')
            if not torch.is_tensor(images) or images.device.type != 'cuda' or not torch.is_tensor(clouds) or clouds.device != images.device:
                raise GwtfError('clouds and images must live on one HIP device; there is no CPU path')
            mus, _ = self.g0_prior(self.img_encoder(images))
            codes = self.g_prior(mus, mode='direct')[0][-1]
        return super().assign_many(clouds, codes=codes, **kwargs)


def _stack_training(model):
    """Whether the decoders' BatchNorm is in train mode (what the routed and the assignment paths refuse before any launch)."""
    return model.mixture_stack().engines[0].couplings[0].training


def _restack(tensors):
    """torch.stack(tensors) -- or, when they are exactly the K slices `base[0], ..., base[K-1]` of one (K, ...) tensor in order (what a
    batched decode hands out), that tensor itself: no copy forward, no unbind / stack pair backward."""
    base = tensors[0]._base
    if (base is not None and base.dim() == tensors[0].dim() + 1 and base.shape[0] == len(tensors) and base.is_contiguous()
            and base.requires_grad == tensors[0].requires_grad):
        step = base.stride(0) * base.element_size()
        if all(t._base is base and t.shape == base.shape[1:] and t.is_contiguous() and t.data_ptr() == base.data_ptr() + k * step
               for k, t in enumerate(tensors)):
            return base
    return torch.stack(tensors)


def _first_column(t):
    """t[:, :, 0] of a (B, P, n) base-Gaussian entry.  The reference builds that entry as `head(g).unsqueeze(2).expand(B, P, n)`
    (models.py:169-193): when `t` is such a broadcast of a (B, P) tensor, that tensor itself is returned -- same values, and the
    gradient reaches it directly instead of through a zero-filled (B, P, n) tensor and a sum over its n columns per component."""
    base = t._base
    if (base is not None and t.dim() == 3 and base.dim() == 2 and t.stride(2) == 0 and base.shape == t.shape[:2]
            and base.stride() == t.stride()[:2] and base.data_ptr() == t.data_ptr()):
        return base
    return t[:, :, 0]


class FlowMixtureNLL(nn.Module):
    """Mixture point NLL on the reference's list outputs (losses.py:88-137), reduced by the fused HIP kernel."""

    def per_shape(self, output_decoder, mixture_weights_logits):
        """-> (B,) NLL of every shape (its mean is the reference's scalar)."""
        z = _restack([o['p_prior_samples'][0] for o in output_decoder])
        # the batched training decode attaches the stack's own log-det (= sum of the list's flow entries, same values)
        def flow_logdet(o):
            if '_sum_flow_logvars' in o:
                return o['_sum_flow_logvars']
            from .decoders import slot_sum
            own = slot_sum(o['p_prior_logvars'][1:])         # the K-loop's lists from a batched sibling round: the sum exists already
            return own if own is not None else sum(o['p_prior_logvars'][1:])
        logdet = _restack([flow_logdet(o) for o in output_decoder])
        mu0 = torch.stack([_first_column(o['p_prior_mus'][0]) for o in output_decoder])
        lv0 = torch.stack([_first_column(o['p_prior_logvars'][0]) for o in output_decoder])
        return flow_mixture_nll(z, logdet, mu0, lv0, mixture_weights_logits)[1]

    def forward(self, output_decoder, mixture_weights_logits):
        return self.per_shape(output_decoder, mixture_weights_logits).mean()


class Flow_Mixture_Loss(nn.Module):
    """pnll_weight * pnll + gnll_weight * gnll - gent_weight * gent   (losses.py:140-170)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.pnll_weight, self.gnll_weight, self.gent_weight = kwargs.get('pnll_weight'), kwargs.get('gnll_weight'), kwargs.get('gent_weight')
        self.n_components = kwargs.get('n_components')
        self.PNLL, self.GNLL, self.GENT = FlowMixtureNLL(), GaussianFlowNLL(), GaussianEntropy()

    def _combine(self, nll, output_prior):
        """nll: (B,) per-shape point NLL (or its mean: the three terms are then combined with torch ops)."""
        fused = self._combine_fused(nll, output_prior) if nll.dim() == 1 else None
        if fused is not None:
            return fused
        pnll = nll.mean() if nll.dim() == 1 else nll
        gnll = self.GNLL(output_prior['g_prior_samples'], output_prior['g_prior_mus'], output_prior['g_prior_logvars'],
                         output_prior.get('_g_prior_logvars_stacked'))
        gent = self.GENT(output_prior['g_posterior_logvars'])
        return self.pnll_weight * pnll + self.gnll_weight * gnll - self.gent_weight * gent, pnll, gnll, gent

    def _combine_fused(self, nll, output_prior):
        """All four values in one launch when the prior flow handed its logvars over as one tensor: prior.LatentLossFn with the
        batch's one base Gaussian ('_g0_params'), prior.LatentLossRowsFn with a base Gaussian per row ('_g0_rows')."""
        flow_lv, g0, rows = output_prior.get('_g_prior_logvars_stacked'), output_prior.get('_g0_params'), False
        if g0 is None:
            g0, rows = output_prior.get('_g0_rows'), True
        post_lv, z = output_prior.get('g_posterior_logvars'), output_prior['g_prior_samples'][0]
        if flow_lv is None or g0 is None or post_lv is None or os.environ.get('GWTF_NO_FUSED_LATENT_LOSS') == '1':
            return None
        ts = (nll, z, g0[0], g0[1], flow_lv, post_lv)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or z.dim() != 2:
            return None
        from . import prior
        w = (float(self.pnll_weight), float(self.gnll_weight), float(self.gent_weight))
        if rows:
            vals = prior.LatentLossRowsFn.apply(nll.contiguous(), z.contiguous(), g0[0].contiguous(), g0[1].contiguous(),
                                                flow_lv.contiguous(), post_lv.contiguous(), *w)
        else:
            vals = prior.LatentLossFn.apply(nll.contiguous(), z.contiguous(), g0[0].reshape(-1), g0[1].reshape(-1),
                                            flow_lv.contiguous(), post_lv.contiguous(), *w)
        return vals[0], vals[1], vals[2], vals[3]

    def forward(self, output_prior, output_decoder, mixture_weights_logits):
        return self._combine(self.PNLL.per_shape(output_decoder, mixture_weights_logits), output_prior)

    def fused(self, output_prior, dec):
        """Same four values from ``Flow_Mixture_Model.forward_fused``'s outputs."""
        return self._combine(flow_mixture_nll(dec['z'], dec['logdet'], dec['mu0'], dec['lv0'], dec['logits'])[1], output_prior)
