"""Reference form of the train-mode PointNet encoder in plain torch on the CPU: what test_encoder_train_ref_cpu.py validates and
test_gpu_encoder_train_f64.py compares csrc/gwtf_encoder_train.hip against.  No device code runs here: the module's own ``features``
Sequential (SharedDot -> BatchNorm1d -> ReLU, four times) in float64 or float32, differentiated by autograd.

A case is (B, N, variant, xseed): the module PointNetCloudEncoder(3, 64, [128, 256, 512]) with load_synth_(m, MODEL_SEED), the cloud
synth_inputs(B, N, 4, xseed)[0], the loss weights randn(B, 512) from a generator seeded with xseed; the 'neg' variant negates every
second entry of each BatchNorm weight (the pooled extreme of those channels is then the MINIMUM of the layer's pre-activation)."""
import copy
import functools

import torch

from go_with_the_flows_amd import encoders
from go_with_the_flows_amd.layers import SharedDot
from go_with_the_flows_amd.synth import load_synth_, synth_inputs

MODEL_SEED = 60
WIDTHS = [128, 256, 512]
MARGIN = 1e-5           # no ReLU input of the float64 reference lies this close to 0 (5 x the fp32 evaluation error at the kink)

# (B, N, variant, xseed): what each case reaches in csrc/gwtf_encoder_train.hip.  The seeds were searched on the CPU for the
# largest gap between the float64 reference's ReLU inputs and 0; the margin each reaches is in docs/LOG.md.
CASES = {
    # a single partial 32-point tile; in every enc_train_dw_kernel launch all slices but the first are empty (dw_per = 32); all 512
    # channels share at most 4 arg-max rows in enc_top_scatter_kernel
    'b1_n4': (1, 4, '', 2008),
    # just under, exactly on and just over one 32-point tile; at 36 the second tile holds 4 points
    'b2_n28': (2, 28, '', 2153),
    'b1_n32': (1, 32, '', 2170),
    'b1_n36': (1, 36, '', 2154),
    # the 128-point workgroup of the backward kernels (kNB1 = kNB2 = 1); the 132 case has negative BatchNorm weights, so the kmin
    # keys, the arg-min and negative s run through the M form
    'b1_n128': (1, 128, '', 2063),
    'b2_n132_neg': (2, 132, 'neg', 2138),
    # the 256-point workgroup of the forward kernels and of backward_top (NB = 2); at 260 layer 1 has slices of 64, 64, 64, 64 and 4
    # points plus three empty ones, layers 2 and 3 have 96, 96, 68 and one empty; in the scatter kernel per = 2
    'b1_n256': (1, 256, '', 2072),
    'b1_n260': (1, 260, '', 2099),
    # three workgroups with a 4-point tail, and more arg-max rows than one 256-thread pass
    'b1_n516': (1, 516, '', 2138),
    # the second block of enc_xmom_kernel (1024 points per block) holds 4 points; the slices are 160 x 6 + 68 and 288 x 3 + 164
    'b1_n1028': (1, 1028, '', 7715),
    # B = 9: the 8-slice walk over the shapes in enc_top_kernel wraps once; the spare tile of tix_point sits behind nine shapes
    'b9_n36': (9, 36, '', 2152),
    # the golden size with half of every BatchNorm weight negative
    'b3_n72_neg': (3, 72, 'neg', 2106),
}
# every point twice, in two different 32-point tiles: the first occurrence is the arg-max, as torch.max gives it
TIE_CASES = {'tie_b1_n64': (1, 64, '', 2004), 'tie_b1_n64_neg': (1, 64, 'neg', 2004)}          # margin 9.7e-5 for both variants


def make_module(variant='', seed=MODEL_SEED):
    """The fp32 CPU module of a case (in train mode)."""
    m = encoders.PointNetCloudEncoder(3, 64, WIDTHS)
    load_synth_(m, seed)
    if variant == 'neg':
        with torch.no_grad():
            for name, prm in m.named_parameters():
                if name.endswith('_bn.weight'):
                    prm[::2].neg_()
    return m.train()


def make_case(B, N, variant, xseed, tie=False):
    """-> (module, x (B,3,N), wgt (B,512)), fp32 on the CPU."""
    x = torch.from_numpy(synth_inputs(B, N, 4, xseed)[0])
    if tie:
        x[:, :, N // 2:] = x[:, :, :N // 2]
    wgt = torch.randn(B, 512, generator=torch.Generator().manual_seed(xseed))
    return make_module(variant), x, wgt


def case_inputs(name):
    if name in TIE_CASES:
        return make_case(*TIE_CASES[name], tie=True)
    return make_case(*CASES[name])


def run_reference(m, x, wgt, dtype, calls=1, keep_features=None, capture=False):
    """One (or ``calls``) train-mode forward + backward of a copy of m's ``features`` in ``dtype`` on the CPU.  Returns a dict:
    'pooled' (B,512), 'argmax' (B,512), 'grad.<parameter>', 'buf.<floating buffer>' (all float64 tensors but argmax), 'tracked'
    {name: int} of the num_batches_tracked counters, 'relu_margin' the smallest |input| over the four ReLU calls of the LAST call,
    'features' (B,512,N) when keep_features (default: float64 only).  The gradients are those of the last call alone.
    capture: also 'dy' and 'a_in' -- per SharedDot the gradient of its output and its input (the operands of dW_l)."""
    if keep_features is None:
        keep_features = dtype == torch.float64
    mm = copy.deepcopy(m).to(dtype).train()
    f = mm.features
    relu_inputs, dots = [], {}
    for name, mod in f.named_children():
        if isinstance(mod, torch.nn.ReLU):                  # in place: the value before the call
            mod.register_forward_pre_hook(lambda _, args: relu_inputs.append(float(args[0].detach().abs().min())))
        elif capture and isinstance(mod, SharedDot):
            rec = dots.setdefault(name, {})
            mod.register_forward_pre_hook(lambda _, args, rec=rec: rec.__setitem__('a_in', args[0].detach().clone()))
            mod.register_forward_hook(
                lambda _, args, y, rec=rec: y.register_hook(lambda g: rec.__setitem__('dy', g.detach().clone())) and None)
    x, wgt = x.to(dtype), wgt.to(dtype)
    for _ in range(calls):
        f.zero_grad(set_to_none=True)
        del relu_inputs[:]
        feat = f(x)
        pooled, argmax = torch.max(feat, dim=2)
        (pooled * wgt).sum().backward()
    assert len(relu_inputs) == 4
    out = {'pooled': pooled.detach().double(), 'argmax': argmax, 'relu_margin': min(relu_inputs),
           'tracked': {n: int(b) for n, b in mm.named_buffers() if not b.dtype.is_floating_point}}
    out.update({'grad.' + n: p.grad.double() for n, p in mm.named_parameters()})
    out.update({'buf.' + n: b.detach().double() for n, b in mm.named_buffers() if b.dtype.is_floating_point})
    if keep_features:
        out['features'] = feat.detach().double()
    if capture:
        out['dy'] = {n: r['dy'] for n, r in dots.items()}
        out['a_in'] = {n: r['a_in'] for n, r in dots.items()}
    return out


def compared_keys(ref):
    """The tensors a test compares: the pooled code, every parameter gradient, every running statistic."""
    return ['pooled'] + [k for k in ref if k.startswith('grad.') or k.startswith('buf.')]


@functools.lru_cache(maxsize=None)
def references(name, calls=1):
    """(float64 run, float32 run) of a named case; computed once, shared by the tests, never modified."""
    m, x, wgt = case_inputs(name)
    return run_reference(m, x, wgt, torch.float64, calls), run_reference(m, x, wgt, torch.float32, calls)
