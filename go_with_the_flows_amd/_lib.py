"""ctypes binding of libgwtf_hip.so (C ABI: include/gwtf.h).

The product path has no fallback: if the shared library is missing or a call fails this module
raises.  Calls are enqueued on torch's current HIP stream for the tensor's device.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GWTF_LIB') or os.path.join(_HERE, 'libgwtf_hip.so')      # GWTF_LIB: an A/B build (tools/ab_build.sh)
ABI_VERSION = 12

MODE_DIRECT, MODE_INVERSE = 0, 1
STAT_REPLICAS = 64   # GWTF_STAT_REPLICAS in csrc/gwtf_layout.h
_MODES = {'direct': MODE_DIRECT, 'inverse': MODE_INVERSE}

_c_fp = ctypes.c_void_p
_SIGNATURES = {
    'gwtf_abi_version': (ctypes.c_int, []),
    'gwtf_error_string': (ctypes.c_char_p, [ctypes.c_int]),
    'gwtf_diag_stamp': (ctypes.c_int, [_c_fp, _c_fp]),
    'gwtf_padded_width': (ctypes.c_int, [ctypes.c_int]),
    'gwtf_raw_coupling_floats': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'gwtf_packed_w_coupling_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_packed_film_coupling_floats': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'gwtf_film_out_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_pack_weights_k': (ctypes.c_int, [_c_fp, _c_fp, _c_fp] + [ctypes.c_int] * 6 + [_c_fp]),
    'gwtf_film_forward': (ctypes.c_int, [_c_fp, _c_fp, _c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, _c_fp]),
    'gwtf_stack_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_packed_x_coupling_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_pack_weights_exact': (ctypes.c_int, [_c_fp, _c_fp, _c_fp] + [ctypes.c_int] * 5 + [_c_fp]),
    'gwtf_stack_forward_exact': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'gwtf_latent_loss_workspace_floats': (ctypes.c_int, [ctypes.c_int] * 2),
    'gwtf_latent_loss_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_latent_loss_backward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_stack_plan': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]),
    'gwtf_bwd_plan': (ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)]),
    'gwtf_pack_w1t': (ctypes.c_int, [_c_fp, _c_fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_packed_b_coupling_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_pack_folded': (ctypes.c_int, [_c_fp] * 5 + [ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_coupling_backward_lists': (ctypes.c_int, [_c_fp] * 13 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, _c_fp]),
    'gwtf_dw1_partials': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'gwtf_dw1_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_dw1_reduce_scratch_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_dw1_reduce': (ctypes.c_int, [_c_fp, ctypes.c_int, _c_fp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_mixture_nll': (ctypes.c_int, [_c_fp] * 7 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_mixture_nll_backward': (ctypes.c_int, [_c_fp] * 12 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_adam_step': (ctypes.c_int, [_c_fp] * 6 + [ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_adam_chunk_elems': (ctypes.c_int, []),
    'gwtf_adam_step_table': (ctypes.c_int, [_c_fp] * 3 + [ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                             ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_adam_hyper': (ctypes.c_int, [ctypes.c_double] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    'gwtf_adam_step_table_dev': (ctypes.c_int, [_c_fp] * 3 + [ctypes.c_int, _c_fp, _c_fp, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                                 _c_fp]),
    'gwtf_loop_begin': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_loop_detect': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_loop_commit': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_loop_eval_commit': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_nn_distance': (ctypes.c_int, [_c_fp] * 6 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_nn_distance_grad': (ctypes.c_int, [_c_fp] * 8 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_approx_match': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_emd_cost': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_emd_cost_pairs': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int] * 6 + [_c_fp]),
    'gwtf_chamfer_directed': (ctypes.c_int, [_c_fp] * 4 + [ctypes.POINTER(ctypes.c_float)] + [ctypes.c_int] * 5 + [_c_fp]),
    'gwtf_match_cost': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_match_cost_grad': (ctypes.c_int, [_c_fp] * 5 + [ctypes.c_int] * 3 + [_c_fp]),
    'gwtf_encoder_raw_floats': (ctypes.c_size_t, [_c_fp, ctypes.c_int]),
    'gwtf_encoder_packed_floats': (ctypes.c_size_t, [_c_fp, ctypes.c_int]),
    'gwtf_encoder_pack': (ctypes.c_int, [_c_fp, _c_fp, _c_fp, ctypes.c_int, _c_fp]),
    'gwtf_encoder_forward': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int, ctypes.c_int, _c_fp, ctypes.c_int, _c_fp]),
    'gwtf_enc_train_supported': (ctypes.c_int, [_c_fp, ctypes.c_int]),
    'gwtf_enc_train_units_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_enc_train_act_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_enc_train_dw_partial_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_enc_train_phase': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'gwtf_enc_train_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_enc_train_backward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_stat_compact': (ctypes.c_int, [_c_fp, _c_fp, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_enc_train_mform_workspace_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_enc_train_mform': (ctypes.c_int, [_c_fp] * 5 + [ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_enc_train_dw3_finish': (ctypes.c_int, [_c_fp] * 6 + [ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_enc_train_dw0_finish': (ctypes.c_int, [_c_fp] * 5 + [ctypes.c_int, _c_fp]),
    'gwtf_prior_raw_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_prior_raw_offset': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'gwtf_prior_workspace_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_prior_forward': (ctypes.c_int, [_c_fp] * 7 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_prior_backward': (ctypes.c_int, [_c_fp] * 10 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_bn_running_update': (ctypes.c_int, [_c_fp, _c_fp, _c_fp, ctypes.c_int, ctypes.c_int, _c_fp]),
    'gwtf_gather_table': (ctypes.c_int, [_c_fp, _c_fp, ctypes.c_int, _c_fp]),
    'gwtf_mtrain_dw1_floats': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'gwtf_film_heads_slices': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'gwtf_film_heads_forward': (ctypes.c_int, [_c_fp] * 7 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, _c_fp]),
    'gwtf_film_heads_backward': (ctypes.c_int, [_c_fp] * 10 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, _c_fp]),
    'gwtf_mtrain_phase': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'gwtf_mtrain_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_mtrain_backward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_mtrain_final_forward_half': (ctypes.c_int, [ctypes.c_int]),
    'gwtf_mtrain_final_backward_half': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'gwtf_head_layer_supported': (ctypes.c_int, [ctypes.c_int] * 4),
    'gwtf_heads_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_heads_backward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_resnet_packed_floats': (ctypes.c_size_t, [ctypes.c_int]),
    'gwtf_resnet_work_floats': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'gwtf_resnet_forward': (ctypes.c_int, [_c_fp] * 4 + [ctypes.c_int] * 5 + [_c_fp]),
    'gwtf_cloud_partials': (ctypes.c_int, [ctypes.c_int]),
    'gwtf_sample_clouds': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_sample_stored_clouds': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_perm_index': (ctypes.c_uint, [ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.c_uint]),
    'gwtf_route_tiles': (ctypes.c_int, [ctypes.c_int] * 3),
    'gwtf_mixture_route': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_stack_forward_routed': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_mixture_route_sweep': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_film_forward_k': (ctypes.c_int, [_c_fp, _c_fp, _c_fp] + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_longlong, _c_fp]),
    'gwtf_transform_images': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_norm2d_partials': (ctypes.c_int, [ctypes.c_int] * 4),
    'gwtf_norm2d_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_norm2d_backward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_norm2d_forward_sums': (ctypes.c_int, [ctypes.c_void_p, _c_fp]),
    'gwtf_norm2d_forward_apply': (ctypes.c_int, [ctypes.c_void_p, _c_fp, ctypes.c_double]),
    'gwtf_norm2d_backward_sums': (ctypes.c_int, [ctypes.c_void_p, _c_fp]),
    'gwtf_norm2d_backward_apply': (ctypes.c_int, [ctypes.c_void_p, _c_fp, ctypes.c_double]),
    'gwtf_conv2d_plan': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]),
    'gwtf_conv2d_forward': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_conv2d_backward_input': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_conv2d_backward_weight': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_voxel_occupancy': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_jsd_counts': (ctypes.c_int, [_c_fp, _c_fp, ctypes.c_int, _c_fp, _c_fp]),
    'gwtf_eval_frame': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_chamfer_paired_partials': (ctypes.c_int, [ctypes.c_int] * 2),
    'gwtf_chamfer_paired': (ctypes.c_int, [_c_fp] * 3 + [ctypes.POINTER(ctypes.c_float)] + [ctypes.c_int] * 4 + [_c_fp]),
    'gwtf_paired_finalise': (ctypes.c_int, [_c_fp] * 8 + [ctypes.c_int] * 5 + [_c_fp]),
    'gwtf_mixture_assign': (ctypes.c_int, [ctypes.c_void_p]),
    'gwtf_render_splats': (ctypes.c_int, [ctypes.c_void_p]),
}

PHASE_FWD_INIT, PHASE_FWD_A, PHASE_FWD_B, PHASE_BWD_A, PHASE_BWD_B, PHASE_BWD_C = range(6)


class TrainCtx(ctypes.Structure):
    """GwtfTrainCtx of include/gwtf.h (K-batched, phase-split train pipeline): same field order."""
    _fields_ = ([(n, ctypes.c_int) for n in ('K', 'B', 'N', 'C', 'f', 'G', 'pattern0', 'mode', 'tune')] +
                [('eps', ctypes.c_float), ('n_total', ctypes.c_double)] +
                [(n, ctypes.c_void_p) for n in (
                    'p', 'raw', 'packed_w', 'packed_b', 'film_raw', 'film_rec', 'moments', 'ystats', 'mom_c', 'ys_c', 'bn_batch', 'xbuf',
                    'logdet', 'ps', 'mus', 'logvars', 'g_out', 'g_ld', 'g_ps', 'g_lvs', 'g_bufs', 'g_xa', 'g_xb', 'dw1_ws', 'g_film', 'g_sd0',
                    'g_bias', 'g_stats', 'g_mom', 'g_film_raw', 'g_raw', 'stream')])


ENC_PHASE_FWD_INIT, ENC_PHASE_FWD_LAYER, ENC_PHASE_BWD_TOP, ENC_PHASE_BWD_LAYER = range(4)


class _Binds:
    """A record whose pointer fields are filled from tensors by name."""

    def bind(self, bufs):
        """self.<name> = the device address of bufs[name]: a tensor, or a list of tensors for the leading entries of an array field
        (None: NULL)."""
        at = lambda b: None if b is None else b.data_ptr()
        for name, b in bufs.items():
            if isinstance(b, (list, tuple)):
                getattr(self, name)[:len(b)] = [at(e) for e in b]
            else:
                setattr(self, name, at(b))


class EncTrainCtx(_Binds, ctypes.Structure):
    """GwtfEncTrainCtx of include/gwtf.h (the encoder's train pipeline, both directions): same field order."""
    _p, _p2, _p3, _p4 = ctypes.c_void_p, ctypes.c_void_p * 2, ctypes.c_void_p * 3, ctypes.c_void_p * 4
    _fields_ = [('B', ctypes.c_int), ('N', ctypes.c_int), ('n_total', ctypes.c_double), ('momentum', ctypes.c_float * 4),
                ('x', _p), ('W', _p4), ('gamma', _p4), ('beta', _p4), ('running_mean', _p4), ('running_var', _p4),
                ('mom', _p), ('mom_c', _p), ('mom_fold', _p), ('sums', _p3), ('sums_c', _p3), ('sums_fold', _p3),
                ('ymax', _p), ('kmax', _p), ('kmin', _p), ('aff', _p4), ('table0', _p), ('units_f', _p3), ('units_b', _p3), ('y', _p2),
                ('pooled', _p), ('amax', _p), ('ystar', _p),
                ('g_pooled', _p), ('gp', _p), ('gmax', _p), ('g_sums', _p3), ('g_sums_c', _p4), ('g_sums_r', _p4), ('bconst', _p4),
                ('units_m', _p), ('mconst', _p), ('mform_ws', _p), ('extra', _p), ('slot_of', _p), ('tables', _p), ('a2rows', _p),
                ('dA', _p2), ('partials', _p), ('gram', _p), ('S', _p), ('dW', _p4), ('stream', _p)]


class HeadArgs(_Binds, ctypes.Structure):
    """GwtfHeadArgs of include/gwtf.h (one or two head layers on the same input, either direction): same field order."""
    _fields_ = ([('x', ctypes.c_void_p), ('g_x', ctypes.c_void_p)] + [(n, ctypes.c_int) for n in ('n_heads', 'B', 'Din', 'bn_updates')] +
                [(n, ctypes.c_void_p * 2) for n in ('W', 'bias', 'gamma', 'beta', 'running_mean', 'running_var', 'num_batches_tracked',
                                                    'ypre', 'stats', 'out', 'g_out', 'g_y', 'g_W', 'g_bias', 'g_gamma', 'g_beta')] +
                [(n, ctypes.c_int * 2) for n in ('Dout', 'bn_mode', 'act')] + [(n, ctypes.c_float * 2) for n in ('momentum', 'bn_eps')] +
                [('stream', ctypes.c_void_p)])


class LatentLossArgs(_Binds, ctypes.Structure):
    """GwtfLatentLossArgs of include/gwtf.h (the latent loss terms, either direction and either family): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('nll', 'z', 'mu0', 'lv0', 'flow_lv', 'post_lv', 'workspace', 'out4', 'g_out4', 'g_nll',
                                                'g_z', 'g_mu0', 'g_lv0', 'g_flow_lv', 'g_post_lv')] +
                [(n, ctypes.c_int) for n in ('B', 'G', 'n2', 'rows')] + [(n, ctypes.c_float) for n in ('pw', 'gw', 'ew')] +
                [('stream', ctypes.c_void_p)])


class StackArgs(ctypes.Structure):
    """GwtfStackArgs of include/gwtf.h (everything a stack launch takes): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('p', 'weights', 'film', 'out', 'logdet', 'ps', 'mus', 'logvars')] +
                [('segments', ctypes.POINTER(ctypes.c_int)), ('worklist', ctypes.c_void_p),
                 ('p_stride_k', ctypes.c_size_t), ('out_stride_k', ctypes.c_size_t)] +
                [(n, ctypes.c_int) for n in ('K', 'B', 'N', 'C', 'f', 'pattern0', 'mode', 'tune')] +
                [('eps', ctypes.c_float), ('stream', ctypes.c_void_p)])


class CloudArgs(ctypes.Structure):
    """GwtfCloudArgs of include/gwtf.h (one batch of sampled clouds): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in (
                    'rows', 'vertices', 'faces', 'thresholds', 'vertices_bounds', 'faces_bounds', 'search_len', 'orig_c', 'orig_s',
                    'cloud', 'eval_cloud', 'partials', 'state', 'words', 's1', 's2', 'normals')] +
                [(n, ctypes.c_int) for n in ('B', 'M', 'n_shapes', 'rescale', 'recenter', 'translate', 'scale', 'noise', 'center',
                                             'tune')] +
                [('shift', ctypes.c_float * 3), ('scale_div', ctypes.c_float), ('noise_scale', ctypes.c_float),
                 ('stream', ctypes.c_void_p)])


class StoredCloudArgs(ctypes.Structure):
    """GwtfStoredCloudArgs of include/gwtf.h (one batch drawn from stored clouds): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('rows', 'points', 'bounds', 'orig_c', 'orig_s', 'cloud', 'eval_cloud', 'partials', 'state',
                                                'index', 'normals')] +
                [(n, ctypes.c_int) for n in ('B', 'M', 'n_shapes', 'rescale', 'recenter', 'translate', 'scale', 'noise', 'center',
                                             'permute', 'tune')] +
                [('shift', ctypes.c_float * 3), ('scale_div', ctypes.c_float), ('noise_scale', ctypes.c_float),
                 ('stream', ctypes.c_void_p)])


class RouteArgs(ctypes.Structure):
    """GwtfRouteArgs of include/gwtf.h (components, base samples and tile layout of S generated clouds): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('logits', 'mu0', 'lv0', 'state', 'words', 'labels_in', 'normals', 'z0_in', 'thresholds',
                                                'tile_comp', 'perm', 'zp', 'labels')] +
                [(n, ctypes.c_int) for n in ('S', 'n', 'K', 'P', 'mu0_stride', 'lv0_stride')] + [('stream', ctypes.c_void_p)])


class RouteSweepArgs(ctypes.Structure):
    """GwtfRouteSweepArgs of include/gwtf.h (GwtfRouteArgs for R rows that share draws in groups, one base per component): same field
    order."""
    _fields_ = (RouteArgs._fields_[:-1] + [(n, ctypes.c_int) for n in ('group', 'mu0_stride_k', 'lv0_stride_k')] +
                [('stream', ctypes.c_void_p)])


class RoutedStackArgs(ctypes.Structure):
    """GwtfRoutedStackArgs of include/gwtf.h (the stack launch on the routed layout): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('zp', 'weights', 'film', 'tile_comp', 'perm', 'out', 'logdet')] +
                [(n, ctypes.c_int) for n in ('K', 'S', 'n', 'P', 'C', 'f', 'pattern0', 'tune')] +
                [('eps', ctypes.c_float), ('stream', ctypes.c_void_p)])


class ImageArgs(ctypes.Structure):
    """GwtfImageArgs of include/gwtf.h (one batch of transformed images): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('images', 'rows', 'xs', 'xf', 'ys', 'yf', 'noise', 'state', 'out')] +
                [(n, ctypes.c_int) for n in ('B', 'n_images', 'C', 'H', 'W', 'H_r', 'W_r', 'pad_y', 'pad_x', 'resize', 'grayscale',
                                             'normalize', 'add_noise', 'remove_alpha')] +
                [('gray', ctypes.c_float * 3), ('mean', ctypes.c_float * 5), ('stdev', ctypes.c_float * 5),
                 ('noise_scale', ctypes.c_float), ('stream', ctypes.c_void_p)])


class Norm2dArgs(ctypes.Structure):
    """GwtfNorm2dArgs of include/gwtf.h (one fused train-mode BatchNorm2d layer, either direction): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('x', 'residual', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'offsets', 'stats',
                                                'partials', 'dy', 'dx', 'd_residual', 'dgamma', 'dbeta')] +
                [(n, ctypes.c_int) for n in ('N', 'C', 'H', 'W', 'relu', 'pool')] +
                [('eps', ctypes.c_float), ('momentum', ctypes.c_float), ('stream', ctypes.c_void_p)])


CONV2D_FORWARD, CONV2D_BACKWARD_INPUT, CONV2D_BACKWARD_WEIGHT = range(3)      # GWTF_CONV2D_* of include/gwtf.h


class Conv2dArgs(ctypes.Structure):
    """GwtfConv2dArgs of include/gwtf.h (one convolution, any of its three passes): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('x', 'w', 'y', 'dy', 'dx', 'dw', 'work')] +
                [(n, ctypes.c_int) for n in ('N', 'Cin', 'H', 'W', 'Cout', 'k', 'stride', 'pad')] + [('stream', ctypes.c_void_p)])


class OccupancyArgs(ctypes.Structure):
    """GwtfOccupancyArgs of include/gwtf.h (one set of points folded into an occupancy histogram): same field order."""
    _fields_ = [('points', ctypes.c_void_p), ('n_points', ctypes.c_size_t), ('res', ctypes.c_int), ('edges', ctypes.c_double * 33),
                ('bound', ctypes.c_float), ('counts', ctypes.c_void_p), ('stats', ctypes.c_void_p), ('stream', ctypes.c_void_p)]


class EvalFrameArgs(ctypes.Structure):
    """GwtfEvalFrameArgs of include/gwtf.h (one batch of both cloud sets into the evaluation frame): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('gen', 'ref', 'orig_s', 'orig_c', 'gen_out', 'ref_out')] +
                [(n, ctypes.c_int) for n in ('B', 'n', 'm', 'n_scale', 'translate', 'row_scale', 'row_shift')] +
                [('scale', ctypes.c_float), ('shift', ctypes.c_double * 3), ('stream', ctypes.c_void_p)])


class AssignArgs(ctypes.Structure):
    """GwtfAssignArgs of include/gwtf.h (per-point component posteriors of observed clouds): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('z', 'logdet', 'mu0', 'lv0', 'logits', 'parts', 'log_density', 'labels', 'confidence',
                                                'resp', 'counts', 'invalid', 'table', 'skipped')] +
                [(n, ctypes.c_int) for n in ('K', 'B', 'N', 'P')] + [('stream', ctypes.c_void_p)])


class RenderArgs(ctypes.Structure):
    """GwtfRenderArgs of include/gwtf.h (labelled clouds drawn into the cells of a contact sheet): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('clouds', 'labels', 'palette', 'view', 'rgb', 'index', 'depth', 'skipped')] +
                [(n, ctypes.c_int) for n in ('B', 'N', 'P', 'label_base', 'view_stride', 'H', 'W', 'radius_q', 'fog', 'sheet_h', 'sheet_w',
                                             'cols', 'cell0', 'cell_step')] +
                [('near', ctypes.c_float), ('inv_range', ctypes.c_float), ('invalid_rgb', ctypes.c_ubyte * 3),
                 ('background_rgb', ctypes.c_ubyte * 3), ('stream', ctypes.c_void_p)])


class LoopState(ctypes.Structure):
    """GwtfLoopState of include/gwtf.h (the training loop's device-resident state, 160 bytes): same field order."""
    _fields_ = ([('meters', ctypes.c_double * 12), ('hyper', ctypes.c_float * 8)] +
                [(n, ctypes.c_int) for n in ('cursor', 'n_iters', 'adam_step', 'status', 'poisoned_at', 'skip', 'flag', 'reserved')])


LOOP_POISONED, LOOP_EXHAUSTED = 1, 2                   # GwtfLoopState.status bits


class LoopArgs(ctypes.Structure):
    """GwtfLoopArgs of include/gwtf.h (the launches of the training loop's state kernels): same field order."""
    _fields_ = ([(n, ctypes.c_void_p) for n in ('state', 'plan', 'rows', 'mesh_rows', 'table')] + [('terms', ctypes.c_void_p * 4)] +
                [(n, ctypes.c_int) for n in ('B', 'views', 'plan_len', 'table_rows', 'stop_on_inf', 'use_flag')] +
                [('stream', ctypes.c_void_p)])


EXPORTS = tuple(_SIGNATURES)

# ---- per-call tuning word (include/gwtf.h GWTF_TUNE_*) ------------------------------------------------------------------------
# The library keeps no tuning state: every dispatching entry point takes the word as an argument.  The HOST side keeps the value
# the wrappers pass -- 0 unless a test / calibration tool changes it inside `with tuning(...)` (restored on exit, also on an
# exception).
TUNE_GENERIC_BODY, TUNE_SMALL_LIGHT_TILE, TUNE_SINGLE_TILE = 1 << 30, 1 << 29, 1 << 28
_TUNE = [0]


def tune_word():
    return _TUNE[0]


def set_tuning(word=0):
    """Set the tuning word the wrappers pass from now on (tests: an autouse fixture resets it); prefer `with tuning(...)`."""
    _TUNE[0] = int(word)


class tuning:
    """with tuning(points_per_wave=64, generic_body=True): ...   -- tile size / coupling body forced for the calls inside."""

    def __init__(self, points_per_wave=0, generic_body=False, small_light_tile=False, word=None):
        self.word = (int(points_per_wave) & 0xffff) | (TUNE_GENERIC_BODY if generic_body else 0) | \
            (TUNE_SMALL_LIGHT_TILE if small_light_tile else 0) if word is None else int(word)

    def __enter__(self):
        self.saved, _TUNE[0] = _TUNE[0], self.word
        return self

    def __exit__(self, *exc):
        _TUNE[0] = self.saved
        return False

_lib = None


class GwtfError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises GwtfError when the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GwtfError(f'{LIB_PATH} not found: build it with `make -C go_with_the_flows_amd/csrc` '
                            '(or `python -c "import __graft_entry__ as g; g.build()"`). There is no fallback path.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        if handle.gwtf_abi_version() != ABI_VERSION:
            raise GwtfError(f'libgwtf_hip.so ABI {handle.gwtf_abi_version()} != expected {ABI_VERSION}; rebuild')
        _lib = handle
    return _lib


def check(code):
    if code != 0:
        raise GwtfError(f'libgwtf_hip call failed ({code}): {lib().gwtf_error_string(code).decode()}')


def _ptr(t, name):
    """Device pointer of a tensor after the input checks the reference's native ops apply
    (is-device + contiguous: lib/metrics/pytorch_structural_losses/src/structural_loss.cpp:10-12)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise GwtfError(f'{name} must live on a HIP device (got {t.device}); there is no CPU path')
    if not t.is_contiguous():
        raise GwtfError(f'{name} must be contiguous')
    if t.dtype != torch.float32:
        raise GwtfError(f'{name} must be float32 (got {t.dtype})')
    return t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def padded_width(f):
    return lib().gwtf_padded_width(f)


def gather_table(table, out, n_rows):
    """gwtf_gather_table on the current stream: out[offset_i .. + numel_i) = source_i for the n_rows rows {pointer, offset, numel} of
    the int64 device tensor `table` -- a raw arena from its parameter / buffer tensors, into storage of the caller's."""
    with torch.cuda.device(out.device):
        check(lib().gwtf_gather_table(table.data_ptr(), _ptr(out, 'raw'), int(n_rows), _stream(out)))
    return out


def _out_buffer(t, name, numel, like):
    if t.numel() != numel or t.device != like.device:
        raise GwtfError(f'{name} must hold {numel} floats on {like.device}, got {t.numel()} on {t.device}')
    return t


def pack_weights(raw, C, f, G, train, pattern0=0, K=1, out=None):
    """Packed stack / FiLM weights of K concatenated stacks of C couplings each (raw: K*C coupling records).  train (the train
    pipeline's packing): the stack weights alone -- its FiLM heads read the raw arena in place; returns (pw, None).
    out = (pw, pf): pack into these tensors (nothing is allocated: an in-place refresh of a persistent packing)."""
    L = lib()
    if raw.numel() != K * C * L.gwtf_raw_coupling_floats(f, G):
        raise GwtfError(f'raw arena has {raw.numel()} floats, expected {K * C * L.gwtf_raw_coupling_floats(f, G)}')
    n_w, n_f = K * C * L.gwtf_packed_w_coupling_floats(f), K * C * L.gwtf_packed_film_coupling_floats(f, G)
    if out is not None:
        pw, pf = _out_buffer(out[0], 'packed_w', n_w, raw), None if train else _out_buffer(out[1], 'packed_film', n_f, raw)
    else:
        pw = torch.empty(n_w, device=raw.device, dtype=torch.float32)
        pf = None if train else torch.empty(n_f, device=raw.device, dtype=torch.float32)
    with torch.cuda.device(raw.device):
        check(L.gwtf_pack_weights_k(_ptr(raw, 'raw'), _ptr(pw, 'packed_w'), _ptr(pf, 'packed_film'), K, C, f, G, int(pattern0),
                                    int(bool(train)), _stream(raw)))
    return pw, pf


def film_forward(g, packed_film, C, f, eps):
    """The (B,C,6FP+4) FiLM record the stack kernel consumes (eval-mode BatchNorm)."""
    L = lib()
    B, G = g.shape
    out = torch.empty(B, C, L.gwtf_film_out_floats(f), device=g.device, dtype=torch.float32)
    with torch.cuda.device(g.device):
        check(L.gwtf_film_forward(_ptr(g, 'g'), _ptr(packed_film, 'packed_film'), _ptr(out, 'film_out'), B, G, C, f, float(eps),
                                  _stream(g)))
    return out


def film_forward_k(gk, packed_film, Cper, f, eps):
    """film_forward with a latent table per component: gk (K, B, G) -> the (B, K*Cper, 6FP+4) record, component k's couplings
    conditioned on gk[k] (gwtf_film_forward_k; eval-mode BatchNorm)."""
    L = lib()
    if gk.dim() != 3:
        raise GwtfError(f'gk must be (K, B, G), got {tuple(gk.shape)}')
    K, B, G = gk.shape
    out = torch.empty(B, K * Cper, L.gwtf_film_out_floats(f), device=gk.device, dtype=torch.float32)
    with torch.cuda.device(gk.device):
        check(L.gwtf_film_forward_k(_ptr(gk, 'gk'), _ptr(packed_film, 'packed_film'), _ptr(out, 'film_out'), B, G, K, Cper, f,
                                    float(eps), B * G, _stream(gk)))
    return out


# ---- the exact-fp32 contraction body (csrc/gwtf_stack_exact.hip) ---------------------------------------------------------------
# EXACT[0]: run the stack on the fp32 matrix instruction instead of the split-f16 one (tests, bench.py's comparison point;
# `with exact_fp32():`).  Otherwise, when the caller hands the exact record (packed_x) along, every split launch is followed by the
# RE-RUN launch: tiles holding a point the split kernel flagged out of range (NaN) are recomputed exactly, all others exit at once.
EXACT = [False]


class exact_fp32:
    def __enter__(self):
        self._old, EXACT[0] = EXACT[0], True
        return self

    def __exit__(self, *exc):
        EXACT[0] = self._old
        return False


def pack_weights_exact(raw, packed_film, C, f, G, pattern0=0, K=1, out=None):
    """GwtfPackX records of K concatenated stacks of C couplings (the fp32 operands of the exact contraction body).
    out: pack into this tensor (records + work list, `packed_x_floats`); its work list was zeroed when it was made and is left alone."""
    L = lib()
    n = K * C * L.gwtf_packed_x_coupling_floats(f)
    # behind the records: the work list of the flagging launch / re-run pair (include/gwtf.h), zero once -- the pair keeps it zero.
    # It lives and dies with the record it serves; like the record it belongs to one stream at a time.
    if out is not None:
        px = _out_buffer(out, 'packed_x', n + WORKLIST_INTS, raw)
    else:
        px = torch.empty(n + WORKLIST_INTS, device=raw.device, dtype=torch.float32)
        px[n:].zero_()
    with torch.cuda.device(raw.device):
        check(L.gwtf_pack_weights_exact(_ptr(raw, 'raw'), _ptr(packed_film, 'packed_film'), _ptr(px, 'packed_x'), K, C, f, G,
                                        int(pattern0), _stream(raw)))
    return px


WORKLIST_INTS = 2 + 2 * 2048          # GWTF_WORKLIST_INTS of include/gwtf.h


def _worklist_ptr(packed_x, K, C, f):
    """Device address of the work list behind the K * C exact records of `packed_x` (pack_weights_exact), or None."""
    n = K * C * lib().gwtf_packed_x_coupling_floats(f)
    if packed_x is None or packed_x.numel() != n + WORKLIST_INTS or os.environ.get('GWTF_NO_RERUN_WORKLIST') == '1':
        return None
    return packed_x.data_ptr() + 4 * n


def _stack_launch(p, packed_w, film, out, logdet, lists, seg, K, C, f, pattern0, eps, mode, out_stride, packed_x):
    """One stack launch sequence on the record: the exact body alone under EXACT[0]; otherwise the split launch (flagging into the
    work list behind packed_x when there is one), then -- packed_x given -- the exact re-run of the tiles it flagged."""
    L = lib()
    B, _, N = p.shape
    lp = [None] * 3 if lists is None else [lists[i].data_ptr() for i in range(3)]
    a = StackArgs(_ptr(p, 'p'), _ptr(packed_w, 'packed_w'), _ptr(film, 'film'), _ptr(out, 'out'), _ptr(logdet, 'logdet'), lp[0], lp[1],
                  lp[2], seg, _worklist_ptr(packed_x, K, C, f), 0, out_stride, K, B, N, C, f, pattern0, _MODES[mode], _TUNE[0],
                  float(eps), _stream(p))
    pa = ctypes.addressof(a)
    with torch.cuda.device(p.device):
        if EXACT[0]:
            if packed_x is None:
                raise GwtfError('exact_fp32: this call site has no exact record (packed_x)')
            a.weights = _ptr(packed_x, 'packed_x')
            check(L.gwtf_stack_forward_exact(pa, 0))
            return
        check(L.gwtf_stack_forward(pa))
        if packed_x is not None:
            a.weights = _ptr(packed_x, 'packed_x')
            check(L.gwtf_stack_forward_exact(pa, 1))      # from the work list, or (none) by looking at every tile


def stack_forward(p, packed_w, film, C, f, pattern0, eps, mode, want_lists, packed_x=None):
    B, three, N = p.shape
    if three != 3:
        raise GwtfError(f'p must be (B,3,N), got {tuple(p.shape)}')
    if film.shape[0] != B or film.shape[1] != C:
        raise GwtfError(f'film is {tuple(film.shape)}, expected ({B},{C},...)')
    out = torch.empty_like(p)
    logdet = torch.empty_like(p)
    lists = torch.empty(3, C, B, 3, N, device=p.device, dtype=torch.float32) if want_lists else None
    _stack_launch(p, packed_w, film, out, logdet, lists, None, 1, C, f, pattern0, eps, mode, 0, packed_x)
    return out, logdet, lists


def stack_forward_multi(p, packed_w, film, K, C, f, pattern0, eps, mode, segments=None, shared_points=True, out=None, logdet=None,
                        packed_x=None):
    """K components in one launch.  shared_points=True: every component maps all of p -> outputs (K,B,3,N).
    Otherwise ``segments`` (list of K (begin,end)) partitions the N points among the components -> (B,3,N).
    out / logdet: optional preallocated result tensors (a timing probe brackets the launch alone with them)."""
    B, three, N = p.shape
    if three != 3:
        raise GwtfError(f'p must be (B,3,N), got {tuple(p.shape)}')
    if film.shape[0] != B or film.shape[1] != K * C:
        raise GwtfError(f'film is {tuple(film.shape)}, expected ({B},{K * C},...)')
    if (out is None) != (logdet is None):
        raise GwtfError('stack_forward_multi: pass out and logdet together (both preallocated) or neither')
    seg = None
    if segments is not None:
        flat = [int(v) for be in segments for v in be]
        if len(flat) != 2 * K:
            raise GwtfError('segments must hold K (begin, end) pairs')
        seg = (ctypes.c_int * (2 * K))(*flat)
    if shared_points:
        if out is None:
            out = torch.empty(K, B, 3, N, device=p.device, dtype=torch.float32)
            logdet = torch.empty(K, B, 3, N, device=p.device, dtype=torch.float32)
        stride = B * 3 * N
    else:
        if out is None:
            # points outside every segment are not touched by the kernel: define them -- unless the segments tile [0, N) (the
            # sampling partition of flow_mixture.py:146-177 always does): two fill launches less per call
            covered = sorted((int(b), int(e)) for b, e in segments if int(e) > int(b))
            tiled = bool(covered) and covered[0][0] == 0 and covered[-1][1] == N and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
            make = torch.empty if tiled else torch.zeros
            out = make(B, 3, N, device=p.device, dtype=torch.float32)
            logdet = make(B, 3, N, device=p.device, dtype=torch.float32)
        stride = 0
    _stack_launch(p, packed_w, film, out, logdet, None, seg, K, C, f, pattern0, eps, mode, stride, packed_x)
    return out, logdet


def dw1_workspace(f, B, N, device, passes=1):
    """Workspace for the per-workgroup dW1 partials of `passes` backward passes over B x N points (csrc/gwtf_bwd.hip)."""
    L = lib()
    return torch.empty(passes * L.gwtf_dw1_workspace_floats(f, B, N) + L.gwtf_dw1_reduce_scratch_floats(f), device=device,
                       dtype=torch.float32)


def dw1_reduce(ws, passes, f, B, N, out=None, branch_stride=None):
    """Sum the partials -> (2,f,f) sd1 weight gradient (deterministic).  With ``branch_stride`` the two (f,f) blocks go to
    out + br*branch_stride (in place into a gradient record)."""
    if out is None:
        out = torch.empty(2, f, f, device=ws.device, dtype=torch.float32)
    check(lib().gwtf_dw1_reduce(_ptr(ws, 'dw1_ws'), passes, out.data_ptr(), f * f if branch_stride is None else branch_stride,
                                f, B, N, _stream(ws)))
    return out


def mixture_nll(z, logdet, mu0, lv0, logits, want_point_lse=False):
    L = lib()
    K, B, _, N = z.shape
    nll = torch.empty(B, device=z.device, dtype=torch.float32)
    plse = torch.empty(B, N, device=z.device, dtype=torch.float32) if want_point_lse else None
    with torch.cuda.device(z.device):
        check(L.gwtf_mixture_nll(_ptr(z, 'z'), _ptr(logdet, 'logdet'), _ptr(mu0, 'mu0'), _ptr(lv0, 'lv0'),
                                 _ptr(logits, 'logits'), _ptr(plse, 'point_lse'), _ptr(nll, 'nll_shape'), K, B, N,
                                 _stream(z)))
    return (nll, plse) if want_point_lse else nll


ASSIGN_MAX_PARTS = 64                 # P of GwtfAssignArgs


def mixture_assign(z, logdet, mu0, lv0, logits, want_confidence=True, want_resp=False, parts=None, n_parts=None, table=None,
                   skipped=None, out=None):
    """gwtf_mixture_assign on the current stream: the inputs of mixture_nll -> {'log_density' (B, N) float32, 'labels' (B, N) int32 in
    [0, K) or -1, 'confidence' (B, N) float32, 'resp' (B, K, N) float32, 'counts' (B, K) int32, 'invalid' (B,) int32}, device tensors;
    'confidence' / 'resp' are None when not wanted.  parts (B, N) int32 with n_parts = P in 1..64: the (label, part) contingency is
    ADDED to table (K, P) int64 and the points left out to skipped (1,) int64 -- zeroed tensors are made when none are passed -- and
    both are returned under 'table' / 'skipped'.  out: a dict as returned by an earlier call on the same shapes, whose tensors are
    written instead of new ones (a captured call then allocates nothing)."""
    if z.dim() != 4 or z.shape[2] != 3:
        raise GwtfError(f'z must be (K, B, 3, N), got {tuple(z.shape)}')
    K, B, _, N = z.shape
    dev, f32, i32, i64 = z.device, torch.float32, torch.int32, torch.int64
    for t, name, shape in ((logdet, 'logdet', (K, B, 3, N)), (mu0, 'mu0', (K, B, 3)), (lv0, 'lv0', (K, B, 3)), (logits, 'logits', (B, K))):
        if tuple(t.shape) != shape or t.device != dev:
            raise GwtfError(f'{name} must be {shape} on {dev}, got {tuple(t.shape)} on {t.device}')
    ptrs = [_ptr(t, name) for t, name in ((z, 'z'), (logdet, 'logdet'), (mu0, 'mu0'), (lv0, 'lv0'), (logits, 'logits'))]
    P = 0
    if parts is not None:
        if n_parts is None or not 1 <= int(n_parts) <= ASSIGN_MAX_PARTS:
            raise GwtfError(f'parts needs n_parts in 1..{ASSIGN_MAX_PARTS}, got {n_parts}')
        P = int(n_parts)
        _explicit(parts, 'parts', (B, N), i32, dev)
        if table is None:
            table = torch.zeros(K, P, device=dev, dtype=i64)
        if skipped is None:
            skipped = torch.zeros(1, device=dev, dtype=i64)
        _explicit(table, 'table', (K, P), i64, dev)
        _explicit(skipped, 'skipped', (1,), i64, dev)
    spec = {'log_density': ((B, N), f32, True), 'labels': ((B, N), i32, True), 'confidence': ((B, N), f32, want_confidence),
            'resp': ((B, K, N), f32, want_resp), 'counts': ((B, K), i32, True), 'invalid': ((B,), i32, True)}
    res = {}
    for name, (shape, dtype, wanted) in spec.items():
        if not wanted:
            res[name] = None
        elif out is not None:
            if out.get(name) is None:
                raise GwtfError(f'out has no {name!r}')
            _explicit(out[name], f'out[{name!r}]', shape, dtype, dev)
            res[name] = out[name]
        else:
            res[name] = torch.empty(shape, device=dev, dtype=dtype)
    at = lambda t: None if t is None else t.data_ptr()
    a = AssignArgs(*ptrs, at(parts), *(at(res[n]) for n in spec), at(table) if parts is not None else None,
                   at(skipped) if parts is not None else None, K, B, N, P, _stream(z))
    with torch.cuda.device(dev):
        check(lib().gwtf_mixture_assign(ctypes.addressof(a)))
    if parts is not None:
        res['table'], res['skipped'] = table, skipped
    return res


RENDER_MAX_PALETTE, RENDER_MAX_RADIUS_Q = 256, 16 * 64        # P and radius_q of GwtfRenderArgs


def render_splats(clouds, labels, palette, view, rgb, H, W, *, label_base=0, radius_q=24, near=0.0, inv_range=0.0, fog=0, cols=1,
                  cell0=0, cell_step=1, invalid_rgb=(0, 0, 0), background_rgb=(255, 255, 255), index=None, depth=None, skipped=None):
    """gwtf_render_splats on the current stream: clouds (B, 3, N) float32, labels (B, N) int32 or None, palette (P, 3) uint8, view
    (3, 4) -- one for all images -- or (B, 3, 4) float32, drawn into the cells cell0 + b * cell_step (H x W pixels each, `cols` per sheet
    row) of rgb (3, sheet_h, sheet_w) uint8.  index (B, H, W) int32, depth (B, H, W) float32, skipped (B,) int32: optional outputs.
    Every tensor lives on the device of `clouds`; nothing is allocated or read back.  Rules: include/gwtf.h (GwtfRenderArgs)."""
    if not torch.is_tensor(clouds) or clouds.dim() != 3 or clouds.shape[1] != 3:
        raise GwtfError(f'clouds must be a (B, 3, N) tensor, got {tuple(getattr(clouds, "shape", ()))}')
    B, _, N = clouds.shape
    dev, f32, i32, u8 = clouds.device, torch.float32, torch.int32, torch.uint8
    p_clouds = _ptr(clouds, 'clouds')
    H, W = int(H), int(W)
    if palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= RENDER_MAX_PALETTE:
        raise GwtfError(f'palette must be (P, 3) with P in 1..{RENDER_MAX_PALETTE}, got {tuple(palette.shape)}')
    if tuple(view.shape) not in ((3, 4), (B, 3, 4)):
        raise GwtfError(f'view must be (3, 4) or ({B}, 3, 4), got {tuple(view.shape)}')
    if rgb.dim() != 3 or rgb.shape[0] != 3:
        raise GwtfError(f'rgb must be (3, sheet_h, sheet_w), got {tuple(rgb.shape)}')
    a = RenderArgs(clouds=p_clouds, labels=_explicit(labels, 'labels', (B, N), i32, dev),
                   palette=_explicit(palette, 'palette', palette.shape, u8, dev), view=_explicit(view, 'view', view.shape, f32, dev),
                   rgb=_explicit(rgb, 'rgb', rgb.shape, u8, dev), index=_explicit(index, 'index', (B, H, W), i32, dev),
                   depth=_explicit(depth, 'depth', (B, H, W), f32, dev), skipped=_explicit(skipped, 'skipped', (B,), i32, dev),
                   B=B, N=N, P=palette.shape[0], label_base=int(label_base), view_stride=12 if view.dim() == 3 else 0, H=H, W=W,
                   radius_q=int(radius_q), fog=int(fog), sheet_h=rgb.shape[1], sheet_w=rgb.shape[2], cols=int(cols), cell0=int(cell0),
                   cell_step=int(cell_step), near=float(near), inv_range=float(inv_range),
                   invalid_rgb=(ctypes.c_ubyte * 3)(*[int(c) for c in invalid_rgb]),
                   background_rgb=(ctypes.c_ubyte * 3)(*[int(c) for c in background_rgb]), stream=_stream(clouds))
    with torch.cuda.device(dev):
        check(lib().gwtf_render_splats(ctypes.addressof(a)))
    return rgb


def stack_plan(K, B, N, f, segments=None, word=None):
    """The tile plan gwtf_stack_forward would use (no launch): (points per wave, workgroups) -- host-only, works without a GPU."""
    seg = None
    if segments is not None:
        flat = [int(v) for be in segments for v in be]
        seg = (ctypes.c_int * len(flat))(*flat)
    out = (ctypes.c_int * 4)()
    check(lib().gwtf_stack_plan(seg, K, B, N, f, _TUNE[0] if word is None else int(word), out))
    return out[0], out[1]


# ---- device-resident generation (csrc/gwtf_route.hip, the ROUTED stack launch) ---------------------------------------------------
def route_tiles(n, K, P):
    """Tile slots per shape of the routed layout, floor((n + K (P - 1)) / P) -- host-only; 0 for sizes the launches reject."""
    return lib().gwtf_route_tiles(int(n), int(K), int(P))


def route_points_per_tile(S, n, K, f):
    """P of a routed generation call: the stack's tile choice for S shapes whose n points split evenly over the K components (the
    expected split; the forced-tile bits of the tuning word apply) -- host-only."""
    cuts = [(k * n) // K for k in range(K + 1)]
    return 4 * stack_plan(K, S, n, f, segments=list(zip(cuts[:-1], cuts[1:])))[0]


def route_scratch(S, n, K, P, device):
    """The buffers one (S, n, K, P) routing call writes: thresholds, tile_comp, perm, zp, labels (callers cache them)."""
    tiles = route_tiles(n, K, P)
    if tiles < 1:
        raise GwtfError(f'no routed layout for S={S}, n={n}, K={K}, P={P}')
    i32 = dict(device=device, dtype=torch.int32)
    return {'P': P, 'tiles': tiles, 'thresholds': torch.zeros(S, K, **i32), 'tile_comp': torch.empty(S, tiles, **i32),
            'perm': torch.empty(S, tiles * P, **i32), 'zp': torch.empty(S, 3, tiles * P, device=device, dtype=torch.float32),
            'labels': torch.empty(S, n, **i32)}


def _explicit(t, name, shape, dtype, device):
    if t is None:
        return None
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise GwtfError(f'{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}')
    return t.data_ptr()


def mixture_route(work, logits=None, mu0=None, lv0=None, state=None, words=None, labels_in=None, normals=None, z0_in=None):
    """gwtf_mixture_route on the current stream into the buffers of `work` (route_scratch).  logits (S, K) float32; mu0 / lv0 (S, 3) or
    (1, 3) float32 (one row: shared by all shapes); state: clouds.make_state; the other four: the explicit draws of include/gwtf.h."""
    S, n = work['labels'].shape
    K, dev = work['thresholds'].shape[1], work['labels'].device
    if state is not None and (state.dtype != torch.int64 or state.numel() != 2 or state.device != dev):
        raise GwtfError('state must come from make_state(seed, device) on the device of the call')
    f32, i32 = torch.float32, torch.int32
    base = []
    for t, name in ((mu0, 'mu0'), (lv0, 'lv0')):
        if t is not None and (t.dim() != 2 or t.shape[0] not in (1, S) or t.shape[1] != 3):
            raise GwtfError(f'{name} must be (S, 3) or (1, 3), got {tuple(t.shape)}')
        base.append((_ptr(t, name), 0 if t is None or t.shape[0] == 1 else 3))
    a = RouteArgs(logits=_explicit(logits, 'logits', (S, K), f32, dev), mu0=base[0][0], lv0=base[1][0],
                  state=None if state is None else state.data_ptr(), words=_explicit(words, 'words', (S, n), i32, dev),
                  labels_in=_explicit(labels_in, 'labels_in', (S, n), i32, dev), normals=_explicit(normals, 'normals', (S, 3, n), f32, dev),
                  z0_in=_explicit(z0_in, 'z0_in', (S, 3, n), f32, dev), thresholds=work['thresholds'].data_ptr(),
                  tile_comp=work['tile_comp'].data_ptr(), perm=work['perm'].data_ptr(), zp=work['zp'].data_ptr(),
                  labels=work['labels'].data_ptr(), S=S, n=n, K=K, P=work['P'], mu0_stride=base[0][1], lv0_stride=base[1][1],
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        check(lib().gwtf_mixture_route(ctypes.addressof(a)))
    return work


def mixture_route_sweep(work, group=1, logits=None, mu0=None, lv0=None, state=None, words=None, labels_in=None, normals=None,
                        z0_in=None):
    """gwtf_mixture_route_sweep on the current stream into the buffers of `work` (route_scratch for R rows): row r takes the draws of
    shape r // group.  logits (R, K) float32; mu0 / lv0 (R, 3) or (1, 3) -- one base for all components -- or (K, R, 3) / (K, 1, 3), a
    base per component; the explicit draws are those of mixture_route with S = R // group rows."""
    R, n = work['labels'].shape
    K, dev = work['thresholds'].shape[1], work['labels'].device
    group = int(group)
    if group < 1 or R % group:
        raise GwtfError(f'group must be a positive divisor of the {R} rows, got {group}')
    S = R // group
    if state is not None and (state.dtype != torch.int64 or state.numel() != 2 or state.device != dev):
        raise GwtfError('state must come from make_state(seed, device) on the device of the call')
    f32, i32 = torch.float32, torch.int32
    base = []
    for t, name in ((mu0, 'mu0'), (lv0, 'lv0')):
        if t is not None and (t.dim() not in (2, 3) or t.shape[-2] not in (1, R) or t.shape[-1] != 3 or (t.dim() == 3 and t.shape[0] != K)):
            raise GwtfError(f'{name} must be (R, 3), (1, 3), (K, R, 3) or (K, 1, 3), got {tuple(t.shape)}')
        rows = 0 if t is None else t.shape[-2]
        base.append((_ptr(t, name), 0 if rows <= 1 else 3, 0 if t is None or t.dim() == 2 else 3 * rows))
    a = RouteSweepArgs(logits=_explicit(logits, 'logits', (R, K), f32, dev), mu0=base[0][0], lv0=base[1][0],
                       state=None if state is None else state.data_ptr(), words=_explicit(words, 'words', (S, n), i32, dev),
                       labels_in=_explicit(labels_in, 'labels_in', (S, n), i32, dev),
                       normals=_explicit(normals, 'normals', (S, 3, n), f32, dev), z0_in=_explicit(z0_in, 'z0_in', (S, 3, n), f32, dev),
                       thresholds=work['thresholds'].data_ptr(), tile_comp=work['tile_comp'].data_ptr(), perm=work['perm'].data_ptr(),
                       zp=work['zp'].data_ptr(), labels=work['labels'].data_ptr(), S=R, n=n, K=K, P=work['P'],
                       mu0_stride=base[0][1], lv0_stride=base[1][1], group=group, mu0_stride_k=base[0][2], lv0_stride_k=base[1][2],
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        check(lib().gwtf_mixture_route_sweep(ctypes.addressof(a)))
    return work


def stack_forward_routed(work, packed_w, film, out, logdet, K, C, f, pattern0, eps):
    """gwtf_stack_forward_routed on the current stream: the layout in `work` through the K stacks -> out / logdet (S, 3, n) (logdet may
    be None).  There is no exact body behind this launch."""
    if EXACT[0]:
        raise GwtfError('exact_fp32: the routed stack launch has no exact-fp32 body')
    S, n = work['labels'].shape
    if film.shape[0] != S or film.shape[1] != K * C:
        raise GwtfError(f'film is {tuple(film.shape)}, expected ({S},{K * C},...)')
    for t, name in ((out, 'out'), (logdet, 'logdet')):
        if t is not None and tuple(t.shape) != (S, 3, n):
            raise GwtfError(f'{name} is {tuple(t.shape)}, expected {(S, 3, n)}')
    a = RoutedStackArgs(zp=work['zp'].data_ptr(), weights=_ptr(packed_w, 'packed_w'), film=_ptr(film, 'film'),
                        tile_comp=work['tile_comp'].data_ptr(), perm=work['perm'].data_ptr(), out=_ptr(out, 'out'),
                        logdet=_ptr(logdet, 'logdet'), K=K, S=S, n=n, P=work['P'], C=C, f=f, pattern0=pattern0, tune=_TUNE[0],
                        eps=float(eps), stream=_stream(out))
    with torch.cuda.device(out.device):
        check(lib().gwtf_stack_forward_routed(ctypes.addressof(a)))
    return out, logdet
