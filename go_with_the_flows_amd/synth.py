"""Deterministic synthetic parameters and inputs (bench, smoke test, golden fixtures).

The reference initialises its last layers at N(0, 0.01) so a fresh decoder is almost the identity
and its log-dets are ~1e-2: useless for parity tests and unrepresentative for timing.  ``synth_state``
fills a ``state_dict`` (keys/shapes taken from the module it is given) with values that make every
BatchNorm, FiLM head and output layer matter: O(1) log-dets, non-trivial running statistics.
Generation is pure numpy from a seed, so fixtures store the seed instead of megabytes of weights.
"""
import numpy as np
import torch


CONDITIONED_GAIN = 0.3   # output_gain of the well-conditioned state: a deep stack then maps 0.3 N(0,1) clouds to |z| of a few units


def synth_state(template_state, seed, output_gain=1.0):
    """template_state: mapping key -> tensor/array (only shapes/dtypes are used).  Returns numpy dict.
    output_gain scales every coupling's output layer (sd2 weight and bias) AFTER the draw, so the random stream -- and every
    golden fixture generated with the default -- is unchanged.  The default (1.0) is the bench / fixture state: O(1) log-dets per
    coupling, which a 33-coupling inverse pass compounds to |z| ~ 5e3 on some points (fp32 evaluation is then ill-conditioned:
    the stated ABSOLUTE tolerance is below fp32's own noise there).  CONDITIONED_GAIN gives what a trained model does -- clouds
    mapped to a few units -- and is the state on which the absolute tolerance is asserted without reference to fp32 noise
    (tests/test_gpu_fullgrid.py)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in template_state:  # insertion order of the module's state_dict: deterministic
        shape = tuple(template_state[key].shape)
        leaf = ('', '') + tuple(key.rsplit('.', 2))
        name, kind = leaf[-2], leaf[-1]
        if kind in ('g0_prior_mus', 'g0_prior_logvars', 'mixture_weights_logits'):      # top-level model parameters
            v = rng.normal(0.0, 0.3, shape)
        elif kind == 'p_prior_mus':
            v = np.zeros(shape)
        elif kind == 'p_prior_logvar':
            v = np.full(shape, -1.0)
        elif kind == 'eps':
            v = np.full(shape, 1e-6, np.float32)
        elif kind == 'num_batches_tracked':
            v = np.zeros(shape, np.int64)
        elif name.endswith('_bn'):
            if kind == 'weight':
                v = rng.uniform(0.6, 1.4, shape)
            elif kind == 'bias':
                v = rng.normal(0.0, 0.1, shape)
            elif kind == 'running_mean':
                v = rng.normal(0.0, 0.15, shape)
            else:  # running_var
                v = rng.uniform(0.5, 1.5, shape)
        elif name.endswith('sd0') or name.endswith('sd1') or name == 'init_sd' or (name.startswith('mlp') and kind == 'weight'):
            fan_in = shape[-1]
            v = rng.uniform(-1.0, 1.0, shape) * np.sqrt(3.0 / fan_in)
        elif name.endswith('sd2'):
            v = (rng.normal(0.0, 0.15, shape) if kind == 'weight' else rng.normal(0.0, 0.1, shape)) * output_gain
        elif name.endswith('film_w0') or name.endswith('film_b0'):
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(shape[-1])
        elif name.endswith('film_w1') or name.endswith('film_b1') or name in ('mu_mlp0', 'logvar_mlp0', 'mu_mlp1', 'logvar_mlp1'):
            v = rng.normal(0.0, 0.08, shape) if kind == 'weight' else rng.normal(0.0, 0.1, shape)
        elif name in ('conv1', 'conv2') or key.endswith('downsample.0.weight'):         # image encoder convolutions: He-scaled
            v = rng.normal(0.0, np.sqrt(2.0 / np.prod(shape[1:])), shape)
        elif name in ('bn1', 'bn2') or key.endswith('downsample.1.' + kind):             # image encoder BatchNorm2d
            if kind == 'weight':
                v = rng.uniform(0.6, 1.4, shape)
            elif kind == 'bias':
                v = rng.normal(0.0, 0.1, shape)
            elif kind == 'running_mean':
                v = rng.normal(0.0, 0.15, shape)
            else:
                v = rng.uniform(0.5, 1.5, shape)
        elif name == 'fc':                                                                   # image encoder head
            v = rng.uniform(-1.0, 1.0, shape) * np.sqrt(3.0 / shape[-1]) if kind == 'weight' else rng.normal(0.0, 0.1, shape)
        else:
            raise KeyError(f'synth_state: unknown parameter kind {key}')
        out[key] = np.asarray(v, dtype=np.int64 if kind == 'num_batches_tracked' else np.float32)
    return out


def load_synth_(module, seed, output_gain=1.0):
    """Overwrite ``module``'s parameters/buffers in place with ``synth_state``; returns the numpy state."""
    st = synth_state(module.state_dict(), seed, output_gain)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return st


def synth_inputs(B, N, G, seed):
    """Clouds ~ 0.3*N(0,1) (ShapeNet clouds are unit-normalised then halved) and latents ~ N(0,1)."""
    rng = np.random.default_rng(seed)
    p = (0.3 * rng.standard_normal((B, 3, N))).astype(np.float32)
    g = rng.standard_normal((B, G)).astype(np.float32)
    return p, g


def synth_images(B, H, W, seed):
    """Normalised 4-channel images ~ N(0,1) (the reference standardises each channel: config_SVR.yaml image_means / image_stds)."""
    return np.random.default_rng(seed).standard_normal((B, 4, H, W)).astype(np.float32)


def image_encoder_bn_names(encoder):
    """Names (state_dict prefixes) of every BatchNorm of an image encoder, in state_dict order."""
    return [n for n, m in encoder.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def calibrate_image_encoder(encoder, seed, n=8, H=64, W=64):
    """Running statistics that keep eval-mode activations O(1) through the 8 blocks (synth_state's draws do not: with random
    statistics a deep residual stack drifts by orders of magnitude and an absolute tolerance means nothing).  One train-mode
    pass of a float64 CPU copy over synth_images(n, H, W, seed) with cumulative averaging: each BatchNorm's running statistics
    become the batch statistics of its input.  Returns {'<bn>.running_mean' / '<bn>.running_var': float32 array}; load them
    with load_image_encoder_stats_."""
    import copy
    enc = copy.deepcopy(encoder).cpu().double().train()
    for m in enc.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.momentum = None
            m.reset_running_stats()
    with torch.no_grad():
        enc.forward_torch(torch.from_numpy(synth_images(n, H, W, seed)).double())
    out = {}
    for name in image_encoder_bn_names(enc):
        m = enc.get_submodule(name)
        out[name + '.running_mean'] = m.running_mean.float().numpy().copy()
        out[name + '.running_var'] = m.running_var.float().numpy().copy()
    return out


def load_image_encoder_stats_(encoder, stats):
    """Copy calibrated running statistics (calibrate_image_encoder, or a fixture's copy of them) into ``encoder`` in place."""
    with torch.no_grad():
        for key, v in stats.items():
            name, kind = key.rsplit('.', 1)
            buf = getattr(encoder.get_submodule(name), kind)
            buf.copy_(torch.as_tensor(np.asarray(v)).to(buf.dtype))


def conditioned_image_encoder_(encoder, seed, calib_seed=None):
    """synth_state weights + calibrated running statistics (the state the image-encoder tolerances are asserted on).
    Returns the statistics."""
    load_synth_(encoder, seed)
    stats = calibrate_image_encoder(encoder, seed + 1 if calib_seed is None else calib_seed)
    load_image_encoder_stats_(encoder, stats)
    return stats
