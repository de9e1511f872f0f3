"""ctypes binding of liblsnet_hip.so (C ABI declared in include/lsnet_hip.h).

The library is built in-tree by lsnet_amd/csrc/build.py.  If it is missing or fails to load the
ops FAIL LOUDLY -- there is no CPU or eager fallback in the product path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('LSNET_HIP_SO') or os.path.join(_HERE, 'csrc', 'liblsnet_hip.so')   # env: diagnostic builds


class Strides4(ctypes.Structure):
    c_name = 'lsn_strides4'
    _fields_ = [('b', ctypes.c_int64), ('c', ctypes.c_int64), ('h', ctypes.c_int64), ('w', ctypes.c_int64)]


class DcnShape(ctypes.Structure):
    c_name = 'lsn_dcn_shape'
    _fields_ = [('B', ctypes.c_int), ('C', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int),
                ('Co', ctypes.c_int), ('Ho', ctypes.c_int), ('Wo', ctypes.c_int),
                ('kh', ctypes.c_int), ('kw', ctypes.c_int), ('stride', ctypes.c_int), ('pad', ctypes.c_int),
                ('dil', ctypes.c_int), ('groups', ctypes.c_int), ('deformable_groups', ctypes.c_int),
                ('scale_h', ctypes.c_float), ('scale_w', ctypes.c_float), ('mask_is_logit', ctypes.c_int),
                ('workspace', ctypes.c_void_p), ('gather_workspace', ctypes.c_void_p),
                ('gather_workspace_bytes', ctypes.c_int64), ('accumulate_param_grads', ctypes.c_int),
                ('out_pitch', ctypes.c_int), ('weights_prepared', ctypes.c_int)]


class DcnLevel(ctypes.Structure):
    c_name = 'lsn_dcn_level'
    _fields_ = [('input', ctypes.c_void_p), ('offset', ctypes.c_void_p), ('mask', ctypes.c_void_p),
                ('output', ctypes.c_void_p), ('grad_output', ctypes.c_void_p), ('grad_input', ctypes.c_void_p),
                ('grad_offset', ctypes.c_void_p), ('grad_mask', ctypes.c_void_p),
                ('off_st', Strides4), ('mask_st', Strides4),
                ('B', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('Ho', ctypes.c_int),
                ('Wo', ctypes.c_int), ('scale_h', ctypes.c_float), ('scale_w', ctypes.c_float)]


class OffsetChainLevel(ctypes.Structure):
    c_name = 'lsn_offset_chain_level'
    _fields_ = [('off', ctypes.c_void_p), ('out', ctypes.c_void_p * 3), ('gout', ctypes.c_void_p * 6), ('goff', ctypes.c_void_p),
                ('images', ctypes.c_int64), ('per_image', ctypes.c_int64), ('off_image_pitch', ctypes.c_int64),
                ('mh', ctypes.c_float * 3), ('mw', ctypes.c_float * 3)]


class WgradBnJob(ctypes.Structure):
    c_name = 'lsn_wgrad_bn_job'
    _fields_ = [('x', ctypes.c_void_p), ('g', ctypes.c_void_p), ('w', ctypes.c_void_p), ('bn_gamma', ctypes.c_void_p),
                ('bn_mean', ctypes.c_void_p), ('bn_var', ctypes.c_void_p), ('bn_eps', ctypes.c_float),
                ('grad_w', ctypes.c_void_p), ('grad_gamma', ctypes.c_void_p), ('grad_beta', ctypes.c_void_p)]


class SgdTensor(ctypes.Structure):
    c_name = 'lsn_sgd_tensor'
    _fields_ = [('param', ctypes.c_void_p), ('grad', ctypes.c_void_p), ('momentum_buf', ctypes.c_void_p),
                ('numel', ctypes.c_int64), ('first_chunk', ctypes.c_int64), ('group', ctypes.c_int)]


class SgdGroup(ctypes.Structure):
    c_name = 'lsn_sgd_group'
    _fields_ = [('lr', ctypes.c_float), ('momentum', ctypes.c_float), ('weight_decay', ctypes.c_float)]


class ConvLevel(ctypes.Structure):
    c_name = 'lsn_conv_level'
    _fields_ = [('x', ctypes.c_void_p), ('out', ctypes.c_void_p), ('grad_out', ctypes.c_void_p),
                ('B', ctypes.c_int), ('H', ctypes.c_int), ('W', ctypes.c_int), ('residual', ctypes.c_void_p),
                ('gate', ctypes.c_void_p)]


class ConvWprep(ctypes.Structure):
    c_name = 'lsn_conv_wprep'
    _fields_ = [('kind', ctypes.c_int), ('w', ctypes.c_void_p), ('prepared', ctypes.c_void_p), ('C', ctypes.c_int),
                ('Co', ctypes.c_int), ('kh', ctypes.c_int), ('kw', ctypes.c_int), ('stride', ctypes.c_int),
                ('pad', ctypes.c_int), ('dil', ctypes.c_int),
                ('bn_gamma', ctypes.c_void_p), ('bn_var', ctypes.c_void_p), ('bn_beta', ctypes.c_void_p),
                ('bn_mean', ctypes.c_void_p), ('shift_out', ctypes.c_void_p), ('bn_eps', ctypes.c_float)]


class GnLevel(ctypes.Structure):
    c_name = 'lsn_gn_level'
    _fields_ = [('x', ctypes.c_void_p), ('y', ctypes.c_void_p), ('dy', ctypes.c_void_p), ('dx', ctypes.c_void_p),
                ('B', ctypes.c_int), ('HW', ctypes.c_int), ('y_batch_stride', ctypes.c_longlong),
                ('dy_batch_stride', ctypes.c_longlong)]


class GateJob(ctypes.Structure):
    c_name = 'lsn_gate_job'
    _fields_ = [('grad_y', ctypes.c_void_p), ('y', ctypes.c_void_p), ('grad', ctypes.c_void_p), ('B', ctypes.c_int),
                ('per_image', ctypes.c_int64), ('gy_batch_stride', ctypes.c_int64)]


class DecodeLevel(ctypes.Structure):
    c_name = 'lsn_decode_level'
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('stride', ctypes.c_float),
                ('cls', ctypes.c_void_p), ('box', ctypes.c_void_p), ('vec', ctypes.c_void_p),
                ('cls_strides', ctypes.c_int64 * 4), ('box_strides', ctypes.c_int64 * 4), ('vec_strides', ctypes.c_int64 * 4)]


class DecodeSource(ctypes.Structure):
    c_name = 'lsn_decode_source'
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('stride', ctypes.c_float),
                ('heat', ctypes.c_void_p), ('offset', ctypes.c_void_p),
                ('heat_strides', ctypes.c_int64 * 4), ('offset_strides', ctypes.c_int64 * 4)]


class CornerLevel(ctypes.Structure):
    c_name = 'lsn_corner_level'
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('score', ctypes.c_void_p), ('offset', ctypes.c_void_p),
                ('score_strides', ctypes.c_int64 * 4), ('offset_strides', ctypes.c_int64 * 4),
                ('grad_score', ctypes.c_void_p), ('grad_offset', ctypes.c_void_p),
                ('grad_score_strides', ctypes.c_int64 * 4), ('grad_offset_strides', ctypes.c_int64 * 4)]


class SemLevel(ctypes.Structure):
    c_name = 'lsn_sem_level'
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('logits', ctypes.c_void_p), ('strides', ctypes.c_int64 * 4),
                ('grad', ctypes.c_void_p), ('grad_strides', ctypes.c_int64 * 4)]


class ProfEntry(ctypes.Structure):
    c_name = 'lsn_prof_entry'
    _fields_ = [('name', ctypes.c_char * 48), ('launches', ctypes.c_longlong), ('total_ms', ctypes.c_double),
                ('flops', ctypes.c_double), ('bytes', ctypes.c_double)]


class ProfLaunch(ctypes.Structure):
    c_name = 'lsn_prof_launch'
    _fields_ = [(k, ctypes.c_int) for k in ('kind', 'C', 'Co', 'kh', 'kw', 'stride', 'pad', 'dil', 'relu', 'xpitch', 'n_levels',
                                            'has_residual', 'has_gate')] + \
               [('B', ctypes.c_int * 16), ('H', ctypes.c_int * 16), ('W', ctypes.c_int * 16), ('ms', ctypes.c_float)]


# the mirrors above, one per struct typedef of include/lsnet_hip.h (each names its typedef in `c_name`)
STRUCTS = (Strides4, DcnShape, DcnLevel, OffsetChainLevel, WgradBnJob, SgdTensor, SgdGroup, ConvLevel, ConvWprep, GnLevel, GateJob,
           DecodeLevel, DecodeSource, CornerLevel, SemLevel, ProfEntry, ProfLaunch)


def _signatures():
    """Every function include/lsnet_hip.h declares, in its order: name -> (restype, argtypes).  i = int / lsn_layout,
    q = int64_t, f = float, d = double, p = lsn_stream_t and any pointer to scalars or void (device or host; also the device
    table `tensors_dev`), P(mirror) = a struct the host fills.  tests/test_capi.py checks the table against the header and
    the mirrors against the compiler's layout, without a GPU."""
    i, q, f, d, p, c_char_p, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, \
        ctypes.c_char_p, ctypes.POINTER
    return {
        'lsn_last_error': (c_char_p, []),
        'lsn_version': (i, []),
        'lsn_set_math_mode': (i, [i]),
        'lsn_get_math_mode': (i, []),
        'lsn_dcn_forward': (i, [P(DcnShape), i, P(DcnLevel), p, p, i, p]),
        'lsn_dcn_backward': (i, [P(DcnShape), i, P(DcnLevel), p, p, p, i, p]),
        'lsn_dcn_backward_workspace_bytes': (q, [P(DcnShape), i, P(DcnLevel)]),
        'lsn_dcn_pitched_ok': (i, [P(DcnShape), i, P(DcnLevel), i]),
        'lsn_dcn_prepared_ok': (i, [P(DcnShape), i, P(DcnLevel), i]),
        'lsn_dcn_anchor_lists': (i, [P(DcnShape), i, P(DcnLevel), i, p, p, p, p, p]),
        'lsn_deform_conv_forward': (i, [p] * 4 + [i] * 16 + [p]),
        'lsn_deform_conv_backward_input': (i, [p] * 6 + [i] * 16 + [p]),
        'lsn_deform_conv_backward_parameters': (i, [p] * 4 + [i] * 15 + [f, i, p]),
        'lsn_modulated_deform_conv_forward': (i, [p] * 6 + [i] * 16 + [p]),
        'lsn_modulated_deform_conv_backward': (i, [p] * 11 + [i] * 16 + [p]),
        'lsn_pyramid_deform_conv_forward': (i, [p] * 4 + [i] * 15 + [f, f, i, i, i, p]),
        'lsn_pyramid_deform_conv_backward_input': (i, [p] * 6 + [i] * 15 + [f, f, i, i, i, p]),
        'lsn_pyramid_deform_conv_backward_parameters': (i, [p] * 4 + [i] * 15 + [f, f, i, i, f, i, p]),
        'lsn_sigmoid_focal_loss_forward': (i, [p, p, p, i, i, f, f, p]),
        'lsn_sigmoid_focal_loss_backward': (i, [p] * 4 + [i, i, f, f, p]),
        'lsn_sigmoid_focal_loss_sum': (i, [p] * 4 + [i, i, f, f, p]),
        'lsn_sigmoid_focal_loss_backward_weighted': (i, [p] * 5 + [i, i, f, f, p]),
        'lsn_sigmoid_focal_loss_level_sums': (i, [p] * 4 + [i] * 4 + [p, f, f, p]),
        'lsn_sigmoid_focal_loss_backward_levels': (i, [p] * 5 + [i] * 4 + [p, f, f, p]),
        'lsn_level_sums': (i, [p, p, i, i, i, p, p]),
        'lsn_level_expand': (i, [p, p, i, i, i, p, p]),
        'lsn_clip_sgd_workspace_bytes': (q, []),
        'lsn_clip_sgd_step': (i, [i, p, q, i, P(SgdGroup), f, p, p, p]),
        'lsn_offset_chain_forward': (i, [i, P(OffsetChainLevel), i, p]),
        'lsn_offset_chain_backward': (i, [i, P(OffsetChainLevel), i, p]),
        'lsn_topk_columns': (i, [p] + [i] * 4 + [p, p, i, i, p, p, p]),
        'lsn_assign_workspace_bytes': (q, [i] * 4),
        'lsn_centroid_assign': (i, [p, i, p, p, i, f, i] + [p] * 5),
        'lsn_centroid_assign_batch': (i, [p, i, p, p, i, p, f, i] + [p] * 5),
        'lsn_atss_assign': (i, [p, i, i, i, p, p, i, i] + [p] * 6),
        'lsn_atss_assign_batch': (i, [p, i, i, i, p, p, i, p, i] + [p] * 6),
        'lsn_dense_targets': (i, [p, i, p, i, p, p]),
        'lsn_centroid_assign_masked_batch': (i, [p, i, p, p, p, i, p, f, i] + [p] * 5),
        'lsn_atss_assign_masked_batch': (i, [p, i, i, i, p, p, p, i, p, i] + [p] * 6),
        'lsn_assign_targets_batch': (i, [p, p, i, i, p, p, i, p, q] + [p] * 6),
        'lsn_nms_workspace_bytes': (q, [i]),
        'lsn_nms': (i, [p, p, i, f] + [p] * 4),
        'lsn_conv2d_prepared_bytes': (q, [i] * 8),
        'lsn_conv2d_prepare_weights': (i, [i, p, p] + [i] * 7 + [p]),
        'lsn_conv2d_prepare_weights_multi': (i, [i, P(ConvWprep), p]),
        'lsn_conv2d_prepare_weights_item': (i, [P(ConvWprep), p]),
        'lsn_conv2d_forward_prepared': (i, [i, P(ConvLevel), p, p] + [i] * 9 + [p]),
        'lsn_conv2d_backward_data_prepared': (i, [i, P(ConvLevel), p] + [i] * 7 + [p]),
        'lsn_conv2d_forward': (i, [p] * 5 + [i] * 11 + [p]),
        'lsn_conv2d_forward_multi': (i, [i, P(ConvLevel), p, p, p] + [i] * 8 + [p]),
        'lsn_conv2d_backward_data_multi': (i, [i, P(ConvLevel), p, p] + [i] * 7 + [p]),
        'lsn_conv2d_backward_weight_multi': (i, [i, P(ConvLevel), p, p] + [i] * 8 + [p]),
        'lsn_conv2d_forward_pitched': (i, [p] * 5 + [i] * 12 + [p]),
        'lsn_conv2d_backward_data': (i, [p] * 4 + [i] * 10 + [p]),
        'lsn_conv2d_backward_weight': (i, [p] * 4 + [i] * 11 + [p]),
        'lsn_conv2d_backward_weight_bn': (i, [p] * 6 + [f, p, p, p] + [i] * 11 + [p]),
        'lsn_conv2d_backward_weight_bn_jobs': (i, [i, P(WgradBnJob)] + [i] * 11 + [p]),
        'lsn_grouped_conv2d_forward': (i, [p] * 4 + [i] * 12 + [p]),
        'lsn_grouped_conv2d_backward_data': (i, [p, p, p] + [i] * 11 + [p]),
        'lsn_grouped_conv2d_backward_weight': (i, [p] * 4 + [i] * 12 + [p]),
        'lsn_group_norm_workspace_bytes': (q, [i, P(GnLevel), i, i]),
        'lsn_group_norm_forward': (i, [i, P(GnLevel), i, i, p, p, f, i, p, p, p]),
        'lsn_group_norm_backward': (i, [i, P(GnLevel), i, i, p, p, i] + [p] * 4 + [i, p]),
        'lsn_bn_eval_act_forward': (i, [p] * 7 + [f, i, i, i, p]),
        'lsn_bn_eval_act_workspace_bytes': (q, [i, i]),
        'lsn_bn_eval_act_backward': (i, [p] * 6 + [f, i] + [p] * 5 + [i, i, i, p]),
        'lsn_relu_gate': (i, [p, p, p, q, p]),
        'lsn_relu_gate_multi': (i, [i, P(GateJob), p]),
        'lsn_debug_phase_clocks': (i, [p, i]),
        'lsn_prof_enable': (i, [i]),
        'lsn_prof_read': (i, [P(ProfEntry), i]),
        'lsn_prof_launch_log': (i, [i]),
        'lsn_prof_read_launches': (i, [P(ProfLaunch), i]),
        'lsn_scratch_stats': (i, [p]),
        'lsn_wgrad_defer': (i, [i, p]),
        'lsn_wgrad_flush': (i, [p]),
        'lsn_selftest_mfma': (i, [p, p, p] + [i] * 4 + [p]),
        'lsn_image_prep_u8': (i, [p] + [i] * 7 + [p, p, i, f, p, i, i, p]),
        'lsn_cross_iou_bbox_forward': (i, [p] * 6 + [q, f, f, p, p]),
        'lsn_cross_iou_bbox_backward': (i, [p] * 7 + [q, f, f, p, p]),
        'lsn_cross_iou_bbox_stage_forward': (i, [p] * 5 + [q, f, f, f, p, p]),
        'lsn_cross_iou_bbox_stage_backward': (i, [p] * 6 + [q, f, f, f, p, p]),
        'lsn_cross_iou_rows_forward': (i, [i] + [p] * 7 + [q, i, i, f, f, p, p]),
        'lsn_cross_iou_rows_backward': (i, [i] + [p] * 8 + [q, i, i, f, f, p, p]),
        'lsn_cross_iou_stage_forward': (i, [i] + [p] * 6 + [q, i, i, f, f, f, p, p]),
        'lsn_cross_iou_stage_backward': (i, [i] + [p] * 7 + [q, i, i, f, f, f, p, p]),
        'lsn_pool_output_size': (i, [i] * 5),
        'lsn_max_pool2d_forward': (i, [p, i, p, i, p] + [i] * 8 + [p]),
        'lsn_max_pool2d_backward': (i, [p, i, p, p] + [i] * 9 + [p]),
        'lsn_avg_pool2d_forward': (i, [p, i, p] + [i] * 11 + [p]),
        'lsn_avg_pool2d_backward': (i, [p, i, p] + [i] * 11 + [p]),
        'lsn_upsample_add_forward': (i, [p, i, p, i, p] + [i] * 7 + [p]),
        'lsn_upsample_add_backward': (i, [p, i, p] + [i] * 8 + [p]),
        'lsn_corner_pool_forward': (i, [i, p, i, p] + [i] * 6 + [p]),
        'lsn_corner_pool_backward': (i, [i, p, i, p, i, p] + [i] * 6 + [p]),
        'lsn_decode_workspace_bytes': (q, [i, i, P(DecodeLevel), i, i]),
        'lsn_decode_batch': (i, [i, i, P(DecodeLevel), i, p, p, i, i, i, f, f, i, i, i] + [p] * 6),
        'lsn_decode_cpv_batch': (i, [i, i, P(DecodeLevel), i, P(DecodeSource), p, i, p, p, i, f, f, i, i, i] + [p] * 5),
        'lsn_corner_targets_workspace_bytes': (q, [i]),
        'lsn_corner_targets_batch': (i, [p, i, p, p, i, p, i, d] + [p] * 5),
        'lsn_corner_loss_workspace_bytes': (q, [i, i, P(CornerLevel)]),
        'lsn_corner_loss_forward': (i, [i, i, i, P(CornerLevel)] + [p] * 4 + [f, f, f] + [p] * 4),
        'lsn_corner_loss_backward': (i, [i, i, i, P(CornerLevel)] + [p] * 4 + [f, f, f, p, p, p]),
        'lsn_sep_focal_workspace_bytes': (q, [i, i, i, P(SemLevel)]),
        'lsn_sep_focal_forward': (i, [i, i, i, P(SemLevel), p, p, i, i, f, f] + [p] * 4),
        'lsn_sep_focal_backward': (i, [i, i, i, P(SemLevel), p, p, i, i, f, f, p, p, p]),
        'lsn_point_decode_forward': (i, [p, i, i, i, p, i, d, p, p, i, p, i, q, p]),
        'lsn_point_decode_backward': (i, [p, i, i, i, p, i, d, p, i, p, i, p, i, p, i, q, p]),
        'lsn_softplus_add_forward': (i, [p, i, p, i, p, i, i, q, p]),
        'lsn_softplus_add_backward': (i, [p, i, p, i, p, i, p, i, i, q, p]),
        'lsn_point_boxes': (i, [p, i, i, p, i, i, i, i, p, i, p]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

_lib = None


def load():
    """Returns the loaded library; raises RuntimeError when it is absent (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f'{SO_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). lsnet_amd has no fallback path.')
    lib = ctypes.CDLL(SO_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().lsn_last_error().decode('utf-8', 'replace')
        if rc == -2:
            raise NotImplementedError(msg)
        raise RuntimeError(msg)


PROF_FAMILIES = ('dcn_fwd', 'dcn_bwd_data', 'dcn_wgrad', 'conv_fwd', 'conv_bwd_data', 'conv_wgrad', 'norm', 'gconv', 'decode',
                 'points')


def prof_enable(on, families=None):
    """Start (and clear) / stop the library's per-kernel event log (lsn_prof_enable); `families`: names of the only
    families to record (default: all)."""
    mask = 0
    if on:
        mask = 1 if families is None else sum(1 << PROF_FAMILIES.index(f) for f in families)
        if mask == 1 and families is not None:
            mask |= 1 << 31    # (the value 1 means "all": keep a single-family mask of bit 0 distinct)
    check(load().lsn_prof_enable(mask))


def prof_read():
    """{family: dict(launches, total_ms, flops, bytes)} of the launches logged since prof_enable(True)."""
    arr = (ProfEntry * 16)()
    n = load().lsn_prof_read(arr, 16)
    if n < 0:
        check(n)
    return {arr[i].name.decode(): dict(launches=int(arr[i].launches), total_ms=arr[i].total_ms,
                                       flops=arr[i].flops, bytes=arr[i].bytes) for i in range(n)}


def ptr(t):
    """The address of tensor `t` for a pointer argument or struct field; None (NULL) for None."""
    return None if t is None else t.data_ptr()


def stream(s=None):
    """The handle of torch's current stream on the current device, or `s` when one is given, for an lsn_stream_t argument."""
    if s is not None:
        return s
    import torch
    # what torch.cuda.current_stream().cuda_stream holds, without building the Stream object around it: 0.3 us instead of
    # 2.6 us on a path of some 300 calls per training step, which more than pays for the typed argument conversion
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def wgrad_defer(max_mbytes, s=None):
    """lsn_wgrad_defer on `s` (default: torch's current stream): max_mbytes > 0 starts deferring the reduces of accumulating
    weight-gradient calls, 0 flushes and ends the mode."""
    check(load().lsn_wgrad_defer(int(max_mbytes), stream(s)))


def wgrad_flush(s=None):
    check(load().lsn_wgrad_flush(stream(s)))


def scratch_stats():
    """What the library has asked of the HIP runtime outside launches (lsn_scratch_stats): dict(mallocs, held_bytes,
    blocking_syncs, pool_allocs)."""
    out = (ctypes.c_longlong * 4)()
    check(load().lsn_scratch_stats(out))
    return dict(mallocs=int(out[0]), held_bytes=int(out[1]), blocking_syncs=int(out[2]), pool_allocs=int(out[3]))


# the debug word of lsn_debug_phase_clocks (include/lsnet_hip.h): bits 0-15 the phase-clock workgroup, from bit 20 up the
# kernel routings that tests and A/B runs select; any other bit is refused
DBG_BLOCK_MASK = 0xffff
DBG_ANCHOR_ONE_WAVE = 1 << 20
DBG_FWD_SK_ALWAYS = 1 << 21
DBG_FWD_SK_NEVER = 1 << 22
DBG_ATOMIC_SCATTER = 1 << 23
DBG_WG_COMPUTED_TAPS = 1 << 24
DBG_WG_SCALAR_LOADS = 1 << 25
DBG_GENERAL_GEMMS = 1 << 28


def set_debug_word(word, buf=None):
    """lsn_debug_phase_clocks: `word` = a phase-clock workgroup | DBG_* routing bits, `buf` = the device address of 512
    int64 for the phase clocks (None: no clocks).  Raises RuntimeError when the library refuses the word."""
    check(load().lsn_debug_phase_clocks(buf, word))


MATH_FP32, MATH_BF16X3, MATH_BF16X6, MATH_BF16 = 0, 1, 2, 3
_MODES = {'fp32': MATH_FP32, 'bf16x3': MATH_BF16X3, 'bf16x6': MATH_BF16X6, 'bf16': MATH_BF16}


def set_math_mode(mode):
    """'bf16x6' (fp32-equivalent split products, the default), 'bf16x3', 'bf16' (one product of the bf16-rounded
    operands, fp32 accumulation) or 'fp32' (exact fp32 MFMA); see include/lsnet_hip.h."""
    check(load().lsn_set_math_mode(_MODES[mode] if isinstance(mode, str) else mode))


def get_math_mode():
    m = load().lsn_get_math_mode()
    return {v: k for k, v in _MODES.items()}[m]


def split_math():
    """True when the contractions run as bf16 products on the matrix pipe ('bf16x6', 'bf16x3' or 'bf16')."""
    return get_math_mode() != 'fp32'
