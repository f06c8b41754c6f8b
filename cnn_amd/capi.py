"""ctypes binding of libcnn_amd.so (include/cnn_amd.h).

This is plumbing for tests and bench.py: it passes raw device pointers (torch tensors' data_ptr()) and the
current HIP stream through the C ABI.  There is NO fallback: if the shared library is missing or a call returns
non-zero, a CnnAmdError is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CNN_AMD_LIB: another build of the same ABI -- tools/ load the measurement build (make -C cnn_amd/csrc measure: libcnn_amd_measure.so,
# the only build in which the result-changing timing switches exist); the product path is the in-tree libcnn_amd.so
LIB_PATH = os.environ.get("CNN_AMD_LIB") or os.path.join(_HERE, "lib", "libcnn_amd.so")


class CnnAmdError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """mirror of cnn_conv2d_desc"""

    _fields_ = [(n, C.c_int) for n in ("B", "Ci", "H", "W", "Co", "k", "s", "pad", "flags")]


POOL_MASK_PACKED = 1  # CNN_CONV2D_POOL_MASK_PACKED (include/cnn_amd.h)
DEPTHWISE = 4  # CNN_CONV2D_DEPTHWISE: Co == Ci, w is [C][1][k][k]; the plain forward / backward entries only


class MixDesc(C.Structure):
    """mirror of cnn_mix_desc"""

    _fields_ = [("mode", C.c_int), ("lam", C.c_float), ("pair_rule", C.c_int), ("pair_shift", C.c_int), ("y0", C.c_int), ("y1", C.c_int),
                ("x0", C.c_int), ("x1", C.c_int)]


class EvalResult(C.Structure):
    """mirror of cnn_eval_result: the head of the evaluation state block"""

    _fields_ = [("samples", C.c_uint64), ("top1", C.c_uint64), ("topk", C.c_uint64), ("ignored", C.c_uint64), ("loss_sum", C.c_double)]


class AugmentOp(C.Structure):
    """mirror of cnn_augment_op"""

    _fields_ = [("kind", C.c_int), ("a", C.c_float), ("b", C.c_float), ("c", C.c_float), ("d", C.c_float)]


AUG_HFLIP, AUG_VFLIP, AUG_CROP, AUG_ROTATE = 1, 2, 3, 4  # CNN_AUG_*


class ColourOp(C.Structure):
    """mirror of cnn_colour_op"""

    _fields_ = [("kind", C.c_int), ("a", C.c_float), ("b", C.c_float)]


COL_BRIGHTNESS, COL_CONTRAST, COL_SATURATION, COL_HUE = 1, 2, 3, 4  # CNN_COL_*
PHOTO_FLOATS = 20  # a sample's photo block: A[9], o[3], ex0, ey0, ew, eh, ev[3], reserved

PAIR_NONE, PAIR_FLIP, PAIR_ROLL = 0, 1, 2  # CNN_PAIR_*
MIX_MIXUP, MIX_CUTMIX = 1, 2  # CNN_MIX_*


class SgdOptions(C.Structure):
    """mirror of cnn_sgd_options"""

    _fields_ = [("lr", C.c_float), ("momentum", C.c_float), ("weight_decay", C.c_float), ("nesterov", C.c_int)]


SGD_INLINE_RANGES = 64  # CNN_SGD_INLINE_RANGES


class AdamOptions(C.Structure):
    """mirror of cnn_adam_options"""

    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("decoupled", C.c_int), ("step", C.c_uint64)]


class LambOptions(C.Structure):
    """mirror of cnn_lamb_options"""

    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("step", C.c_uint64)]


class LarsOptions(C.Structure):
    """mirror of cnn_lars_options"""

    _fields_ = [("lr", C.c_float), ("momentum", C.c_float), ("weight_decay", C.c_float), ("trust_coefficient", C.c_float), ("eps", C.c_float),
                ("nesterov", C.c_int)]


SEG_DECAY = 1  # CNN_SEG_DECAY
SEG_ADAPT = 2  # CNN_SEG_ADAPT
SEG_CHUNK = 1024  # CNN_SEG_CHUNK: elements of the flat range per workgroup of the layer-wise kernels

CLIP_MAX_BLOCKS = 2048  # CNN_CLIP_MAX_BLOCKS: the largest grid of the clip kernels (workgroups of CLIP_BLOCK lanes, a float4 per lane)
CLIP_BLOCK = 256


_lib = None

# name -> (restype, argtypes); the single source for the "exports every declared symbol" test
_P = C.c_void_p
_D = C.POINTER(ConvDesc)
SIGNATURES = {
    "cnn_amd_abi_version": (C.c_int, []),
    "cnn_amd_last_error": (C.c_char_p, []),
    "cnn_amd_device_arch": (C.c_char_p, []),
    "cnn_amd_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "cnn_amd_get_option": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    "cnn_amd_measure_build": (C.c_int, []),
    "cnn_amd_kernel_timing_enable": (C.c_int, [C.c_int, C.c_char_p]),
    "cnn_amd_kernel_timing_sampling": (C.c_int, [C.c_int]),
    "cnn_amd_kernel_timing_report": (C.c_longlong, [C.c_char_p, C.c_size_t]),
    "cnn_amd_timing_span_begin": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnn_amd_timing_span_end": (C.c_int, [C.c_void_p]),
    "cnn_conv2d_out_dim": (C.c_int, [C.c_int] * 4),
    "cnn_maxpool2d_out_dim": (C.c_int, [C.c_int] * 3),
    "cnn_conv2d_workspace_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_autotune": (C.c_int, [_D, _P]),
    "cnn_conv2d_forward": (C.c_int, [_D, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_forward_relu": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_relu_maxpool2_supported": (C.c_int, [_D]),
    "cnn_conv2d_pool_mask_packed_supported": (C.c_int, [_D]),
    "cnn_conv2d_pool_mask_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_pool_mask_unpack": (C.c_int, [_D, _P, _P, _P]),
    "cnn_conv2d_relu_only_supported": (C.c_int, [_D]),
    "cnn_conv2d_relu_maxpool2_forward": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_relu_maxpool2_forward_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P]),
    "cnn_conv2d_backward_pooled2_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P, C.c_int]),
    "cnn_conv2d_backward_weight_pooled2": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_weight_pooled2_sgd": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_float, C.c_float, _P, _P, _P,
                                                          C.c_size_t, _P]),
    "cnn_conv2d_backward_data_pooled2": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_data_pooled2_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P, _P]),
    "cnn_conv2d_prepared_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_prepare_filters": (C.c_int, [C.c_int, _D, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), _P]),
    "cnn_conv2d_forward_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P, _P]),
    "cnn_conv2d_backward_data_prepared": (C.c_int, [_D, _P, _P, _P, _P]),
    "cnn_conv2d_backward_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P, C.c_int]),
    "cnn_conv2d_backward_prepared_relu": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P, C.c_int]),
    "cnn_conv2d_backward_data_relu": (C.c_int, [_D, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_data_relu_prepared": (C.c_int, [_D, _P, _P, _P, _P, _P]),
    "cnn_conv2d_backward_weight": (C.c_int, [_D, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_data": (C.c_int, [_D, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_workspace_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_backward": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P, C.c_int]),
    "cnn_amd_side_stream_join": (C.c_int, [_P]),
    "cnn_amd_side_stream_get": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cnn_amd_flush_reduces": (C.c_int, [_P]),
    "cnn_grad_cam": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "cnn_amd_publish_next_kernel": (C.c_int, [_P]),
    "cnn_linear_forward_softmax_xent_dx": (C.c_int, [_P] * 9 + [C.c_int] * 4 + [_P]),
    "cnn_amd_wait_published": (C.c_int, [_P]),
    "cnn_amd_published_is_last": (C.c_int, [_P]),
    "cnn_conv2d_im2col_workspace_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_forward_im2col": (C.c_int, [_D, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_weight_im2col": (C.c_int, [_D, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P]),
    "cnn_conv2d_backward_data_im2col": (C.c_int, [_D, _P, _P, _P, _P, C.c_size_t, _P]),
    "cnn_maxpool2d_forward": (C.c_int, [_P, _P, _P] + [C.c_int] * 6 + [_P]),
    "cnn_maxpool2d_backward": (C.c_int, [_P, _P, _P] + [C.c_int] * 6 + [_P]),
    "cnn_maxpool2d_backward_relu": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    "cnn_relu_forward": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_relu_backward": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_dropout_forward": (C.c_int, [_P, _P] + [C.c_int] * 6 + [C.c_float, _P]),
    "cnn_dropout_backward": (C.c_int, [_P] + [C.c_int] * 5 + [_P]),
    "cnn_batch_stager_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]),
    "cnn_batch_stager_create_u8": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "cnn_batch_stager_destroy": (C.c_int, [_P]),
    "cnn_batch_stager_acquire": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "cnn_batch_stager_submit": (C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p)]),
    "cnn_batch_stager_wait": (C.c_int, [_P, C.c_int, _P]),
    "cnn_batch_stager_release": (C.c_int, [_P, C.c_int, _P]),
    "cnn_augment_u8": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, _P]),
    "cnn_augment_matrix": (C.c_int, [C.POINTER(AugmentOp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "cnn_batch_stager_create_u8_aug": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cnn_batch_stager_matrices": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_float))]),
    "cnn_batch_stager_set_fill": (C.c_int, [_P, C.c_float]),
    "cnn_batch_stager_create_u8_photo": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cnn_batch_stager_photo": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_float))]),
    "cnn_batch_stager_set_normalize": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "cnn_colour_matrix": (C.c_int, [C.POINTER(ColourOp), C.c_int, C.POINTER(C.c_float)]),
    "cnn_dataset_create_u8": (C.c_int, [C.POINTER(C.c_void_p), C.c_longlong, C.c_int, C.c_int]),
    "cnn_dataset_write": (C.c_int, [_P, C.c_longlong, C.c_longlong, _P, _P]),
    "cnn_dataset_read": (C.c_int, [_P, C.c_longlong, C.c_longlong, _P, _P]),
    "cnn_dataset_info": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cnn_dataset_destroy": (C.c_int, [_P]),
    "cnn_batch_stager_create_u8_resident": (C.c_int, [C.POINTER(C.c_void_p), _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cnn_dataset_max_levels": (C.c_int, [C.c_int, C.c_int]),
    "cnn_augment_level": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "cnn_dataset_create_u8_levels": (C.c_int, [C.POINTER(C.c_void_p), C.c_longlong, C.c_int, C.c_int, C.c_int]),
    "cnn_dataset_read_level": (C.c_int, [_P, C.c_int, C.c_longlong, C.c_longlong, _P]),
    "cnn_dataset_level_info": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cnn_batch_stager_levels": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_int))]),
    "cnn_batch_stager_indices": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_int))]),
    "cnn_batch_stager_labels": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_int))]),
    "cnn_linear_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "cnn_linear_backward": (C.c_int, [_P] * 6 + [C.c_int] * 3 + [C.c_float, _P]),
    "cnn_linear_backward_relu": (C.c_int, [_P] * 6 + [C.c_int] * 3 + [C.c_float, _P]),
    "cnn_batchnorm2d_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "cnn_batchnorm2d_forward": (C.c_int, [_P] * 8 + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_int, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_forward_relu": (C.c_int, [_P] * 9 + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_int, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_backward": (C.c_int, [_P] * 7 + [C.c_int] * 4 + [C.c_float, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_forward_relu_pool_supported": (C.c_int, [C.c_int] * 4),
    "cnn_batchnorm2d_forward_relu_pool": (C.c_int, [_P] * 11 + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_int, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_backward_pooled_supported": (C.c_int, [C.c_int] * 4),
    "cnn_batchnorm2d_backward_pooled": (C.c_int, [_P] * 10 + [C.c_int] * 4 + [C.c_float, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_partial_sums": (C.c_int, [_P, _P, C.c_float, _P] + [C.c_int] * 4 + [_P, C.c_size_t, _P]),
    "cnn_batchnorm2d_forward_from_sums": (C.c_int, [_P] * 10 + [C.c_float] + [C.c_int] * 4 + [C.c_float, C.c_float, _P]),
    "cnn_batchnorm2d_forward_from_sums_relu": (C.c_int, [_P] * 11 + [C.c_float] + [C.c_int] * 4 + [C.c_float, C.c_float, _P]),
    "cnn_batchnorm2d_backward_sums": (C.c_int, [_P] * 6 + [C.c_int] * 4 + [C.c_float, _P, C.c_size_t, _P]),
    "cnn_batchnorm2d_backward_from_sums": (C.c_int, [_P] * 6 + [C.c_float, _P, _P] + [C.c_int] * 4 + [C.c_float, _P]),
    "cnn_sgd_update": (C.c_int, [_P, _P, C.c_size_t, C.c_float, C.c_float, _P]),
    "cnn_sgd_update_keep": (C.c_int, [_P, _P, C.c_size_t, C.c_float, C.c_float, _P, _P]),
    "cnn_sgd_momentum_update": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(SgdOptions), C.c_float, _P, _P, C.c_size_t, _P, _P]),
    "cnn_adam_update": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(AdamOptions), C.c_float, _P, _P, C.c_size_t, _P, _P]),
    "cnn_clip_grad_norm_workspace_bytes": (C.c_size_t, [C.c_size_t]),
    "cnn_clip_grad_norm": (C.c_int, [_P, C.c_size_t, C.c_float, C.c_float, _P, C.c_size_t, _P, _P]),
    "cnn_grad_accumulate": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "cnn_ema_decay_at": (C.c_float, [C.c_float, C.c_int, C.c_uint64]),
    "cnn_ema_update": (C.c_int, [_P, _P, C.c_size_t, C.c_float, _P, _P, C.c_size_t, _P]),
    "cnn_arena_swap": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_layerwise_create": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_void_p)]),
    "cnn_layerwise_destroy": (C.c_int, [_P]),
    "cnn_layerwise_stats": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "cnn_segment_norms": (C.c_int, [_P, _P, _P, _P]),
    "cnn_lamb_update": (C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(LambOptions), C.c_float, _P, _P]),
    "cnn_lars_update": (C.c_int, [_P, _P, _P, _P, C.POINTER(LarsOptions), C.c_float, _P, _P]),
    "cnn_stream_wait_event_local": (C.c_int, [_P, _P]),
    "cnn_stream_create_priority": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "cnn_conv2d_backward_weight_pooled2_sgd_keep": (C.c_int, [_D, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P,
                                                               C.c_size_t, _P]),
    "cnn_comm_available": (C.c_int, []),
    "cnn_comm_version": (C.c_int, []),
    "cnn_comm_unique_id": (C.c_int, [_P]),
    "cnn_comm_init_rank": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, _P]),
    "cnn_comm_init_all": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]),
    "cnn_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cnn_comm_destroy": (C.c_int, [_P]),
    "cnn_comm_group_start": (C.c_int, []),
    "cnn_comm_group_end": (C.c_int, []),
    "cnn_allreduce_grads": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_comm_split": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "cnn_comm_broadcast": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "cnn_conv2d_autotune_workspace_bytes": (C.c_size_t, [_D]),
    "cnn_conv2d_autotune_ws": (C.c_int, [_D, _P, C.c_size_t, _P]),
    "cnn_conv2d_tune_export": (C.c_int, [_D, C.POINTER(C.c_int32)]),
    "cnn_conv2d_tune_import": (C.c_int, [_D, C.POINTER(C.c_int32)]),
    "cnn_softmax_xent": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "cnn_linear_forward_softmax_xent": (C.c_int, [_P] * 8 + [C.c_int] * 3 + [_P]),
    "cnn_loss_from_terms": (C.c_int, [_P, _P, C.c_int, _P]),
    "cnn_soft_targets": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P]),
    "cnn_batch_mix": (C.c_int, [C.POINTER(MixDesc), _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "cnn_cutmix_lambda": (C.c_float, [C.c_int] * 6),
    "cnn_softmax_xent_soft": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "cnn_linear_forward_softmax_xent_soft": (C.c_int, [_P] * 8 + [C.c_int] * 3 + [_P]),
    "cnn_linear_forward_softmax_xent_soft_dx": (C.c_int, [_P] * 9 + [C.c_int] * 4 + [_P]),
    "cnn_eval_state_bytes": (C.c_size_t, [C.c_int]),
    "cnn_eval_accumulate": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "cnn_eval_read": (C.c_int, [_P, C.c_int, C.POINTER(EvalResult), _P, _P]),
    "cnn_conv2d_backward_weight_side": (C.c_int, [_D, _P, _P, _P, _P, C.c_float, _P, C.c_size_t, _P]),
    "cnn_device_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "cnn_device_free": (C.c_int, [_P]),
    "cnn_memcpy_h2d": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_memcpy_d2h": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_memcpy_d2d": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "cnn_memset_zero": (C.c_int, [_P, C.c_size_t, _P]),
    "cnn_stream_synchronize": (C.c_int, [_P]),
    "cnn_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cnn_stream_destroy": (C.c_int, [_P]),
    "cnn_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cnn_event_destroy": (C.c_int, [_P]),
    "cnn_event_record": (C.c_int, [_P, _P]),
    "cnn_stream_wait_event": (C.c_int, [_P, _P]),
    "cnn_host_alloc_pinned": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "cnn_host_free_pinned": (C.c_int, [_P]),
}


def load():
    """dlopen the in-tree library (built by __graft_entry__.build() / make -C cnn_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CnnAmdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        try:  # torch bundles its own libamdhip64: import it FIRST so that this process has ONE HIP runtime (loading
            import torch  # noqa: F401  ours first and torch later leaves torch with "No HIP GPUs are available")
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here == the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise CnnAmdError(f"{what} failed with code {rc}: {load().cnn_amd_last_error().decode()}")


def conv_out_dim(n, k, s, pad=0):
    return (n + 2 * pad - k) // s + 1


def pool_out_dim(n, k, step):
    return (n - k) // step + 1


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise CnnAmdError("tensors passed to the HIP path must be contiguous device tensors")


class Conv2d:
    """One Conv2D geometry: owns the scratch buffer, forwards to the C ABI.  Weight layout [Co][Ci][k][k]."""

    def __init__(self, B, Ci, H, W, Co, k=3, s=2, pad=0, device="cuda"):
        import torch

        self.desc = ConvDesc(B, Ci, H, W, Co, k, s, pad)
        self.Ho, self.Wo = conv_out_dim(H, k, s, pad), conv_out_dim(W, k, s, pad)
        self.lib = load()
        self.ws_bytes = int(self.lib.cnn_conv2d_workspace_bytes(C.byref(self.desc)))
        if self.ws_bytes == 0:
            raise CnnAmdError("cnn_conv2d_workspace_bytes: " + self.lib.cnn_amd_last_error().decode())
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self._im2col_ws = None
        self._bwd_ws = None

    def out_shape(self):
        d = self.desc
        return (d.B, d.Co, self.Ho, self.Wo)

    def autotune(self):
        """cnn_conv2d_autotune: measure and pin the implicit-GEMM tile of this geometry (synchronises; once per process)"""
        check(self.lib.cnn_conv2d_autotune(C.byref(self.desc), _stream()), "cnn_conv2d_autotune")

    def forward(self, x, w, bias, y=None):
        import torch

        _need_gpu(x, w, bias, y)
        if y is None:
            y = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        check(self.lib.cnn_conv2d_forward(C.byref(self.desc), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(self.ws),
                                          self.ws_bytes, _stream()), "cnn_conv2d_forward")
        return y

    def forward_relu(self, x, w, bias, y, y_relu):
        """Conv2D::forward + the ReLU::forward behind it in one kernel: writes y and y_relu = relu(y)"""
        _need_gpu(x, w, bias, y, y_relu)
        check(self.lib.cnn_conv2d_forward_relu(C.byref(self.desc), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(y_relu),
                                               _ptr(self.ws), self.ws_bytes, _stream()), "cnn_conv2d_forward_relu")
        return y_relu

    def relu_maxpool2_supported(self):
        return bool(self.lib.cnn_conv2d_relu_maxpool2_supported(C.byref(self.desc)))

    def pool_mask_packed_supported(self):
        return bool(self.lib.cnn_conv2d_pool_mask_packed_supported(C.byref(self.desc)))

    def set_pool_mask_packed(self, on=True):
        """desc.flags: the fused block's calls of this object write / read the packed one-byte pool mask (include/cnn_amd.h)"""
        self.desc.flags = POOL_MASK_PACKED if on else 0

    def pool_mask_bytes(self):
        return int(self.lib.cnn_conv2d_pool_mask_bytes(C.byref(self.desc)))

    def pool_mask_unpack(self, packed, mask):
        _need_gpu(packed, mask)
        check(self.lib.cnn_conv2d_pool_mask_unpack(C.byref(self.desc), _ptr(packed), _ptr(mask), _stream()), "cnn_conv2d_pool_mask_unpack")
        return mask

    def relu_maxpool2_forward(self, x, w, bias, pooled, mask=None, prepared_fwd=None):
        """Conv2D -> ReLU -> MaxPool2D(2,2) in one kernel: writes pooled (and mask); from prepared filters when given"""
        _need_gpu(x, pooled)
        if prepared_fwd is not None:
            check(self.lib.cnn_conv2d_relu_maxpool2_forward_prepared(C.byref(self.desc), _ptr(x), _ptr(prepared_fwd), _ptr(pooled),
                                                                     _ptr(mask) if mask is not None else None, _stream()),
                  "cnn_conv2d_relu_maxpool2_forward_prepared")
        else:
            check(self.lib.cnn_conv2d_relu_maxpool2_forward(C.byref(self.desc), _ptr(x), _ptr(w), _ptr(bias), _ptr(pooled),
                                                            _ptr(mask) if mask is not None else None, _ptr(self.ws), self.ws_bytes,
                                                            _stream()), "cnn_conv2d_relu_maxpool2_forward")
        return pooled

    def backward_weight_pooled2(self, x, dpool, mask, pooled, divisor, gw, gb):
        """weight / bias gradient with dy = relu_backward(maxpool_backward(dpool)) rebuilt on the fly"""
        _need_gpu(x, dpool, mask, gw, gb)  # pooled=None: dpool already carries the ReLU mask
        check(self.lib.cnn_conv2d_backward_weight_pooled2(C.byref(self.desc), _ptr(x), _ptr(dpool), _ptr(mask),
                                                          _ptr(pooled) if pooled is not None else None, _ptr(gw),
                                                          _ptr(gb), float(divisor), _ptr(self.ws), self.ws_bytes, _stream()),
              "cnn_conv2d_backward_weight_pooled2")
        return gw, gb

    def backward_weight_pooled2_sgd(self, x, dpool, mask, pooled, divisor, gw, gb, w, bias, lr, grad_scale, prepared_fwd, prepared_dgrad):
        """backward_weight_pooled2 + this layer's SGD step + its re-prepared filters (one extra launch)"""
        _need_gpu(x, dpool, mask, gw, gb, w, bias)
        check(self.lib.cnn_conv2d_backward_weight_pooled2_sgd(C.byref(self.desc), _ptr(x), _ptr(dpool), _ptr(mask),
                                                              _ptr(pooled) if pooled is not None else None, _ptr(gw), _ptr(gb),
                                                              float(divisor), _ptr(w), _ptr(bias), float(lr), float(grad_scale),
                                                              _ptr(prepared_fwd) if prepared_fwd is not None else None,
                                                              _ptr(prepared_dgrad) if prepared_dgrad is not None else None,
                                                              _ptr(self.ws), self.ws_bytes, _stream()),
              "cnn_conv2d_backward_weight_pooled2_sgd")
        return gw, gb

    def backward_pooled2_prepared(self, x, dpool, mask, pooled, prepared_dgrad, divisor, gw, gb, dx, defer_join=False):
        """weight gradient (library side stream) and data gradient (current stream) of the pool-fused block in one call"""
        _need_gpu(x, dpool, mask, prepared_dgrad, gw, gb, dx)
        check(self.lib.cnn_conv2d_backward_pooled2_prepared(C.byref(self.desc), _ptr(x), _ptr(dpool), _ptr(mask),
                                                            _ptr(pooled) if pooled is not None else None, _ptr(prepared_dgrad), _ptr(gw),
                                                            _ptr(gb), _ptr(dx), float(divisor), _ptr(self.ws), self.ws_bytes, _stream(),
                                                            1 if defer_join else 0), "cnn_conv2d_backward_pooled2_prepared")
        return gw, gb, dx

    def backward_data_pooled2(self, dpool, mask, pooled, w, dx, prepared_dgrad=None):
        _need_gpu(dpool, mask, dx)
        pooled_p = _ptr(pooled) if pooled is not None else None
        if prepared_dgrad is not None:
            check(self.lib.cnn_conv2d_backward_data_pooled2_prepared(C.byref(self.desc), _ptr(dpool), _ptr(mask), pooled_p,
                                                                     _ptr(prepared_dgrad), _ptr(dx), _stream()),
                  "cnn_conv2d_backward_data_pooled2_prepared")
        else:
            check(self.lib.cnn_conv2d_backward_data_pooled2(C.byref(self.desc), _ptr(dpool), _ptr(mask), pooled_p, _ptr(w), _ptr(dx),
                                                            _ptr(self.ws), self.ws_bytes, _stream()), "cnn_conv2d_backward_data_pooled2")
        return dx

    def backward_weight(self, x, dy, divisor, gw=None, gb=None, want_bias=True):
        import torch

        _need_gpu(x, dy, gw, gb)
        d = self.desc
        if gw is None:
            gw = torch.empty((d.Co, d.Ci, d.k, d.k), dtype=torch.float32, device=x.device)
        if gb is None and want_bias:
            gb = torch.empty((d.Co,), dtype=torch.float32, device=x.device)
        check(self.lib.cnn_conv2d_backward_weight(C.byref(d), _ptr(x), _ptr(dy), _ptr(gw), _ptr(gb), float(divisor),
                                                  _ptr(self.ws), self.ws_bytes, _stream()), "cnn_conv2d_backward_weight")
        return gw, gb

    def backward_data(self, dy, w, dx=None):
        import torch

        _need_gpu(dy, w, dx)
        d = self.desc
        if dx is None:
            dx = torch.empty((d.B, d.Ci, d.H, d.W), dtype=torch.float32, device=dy.device)
        check(self.lib.cnn_conv2d_backward_data(C.byref(d), _ptr(dy), _ptr(w), _ptr(dx), _ptr(self.ws), self.ws_bytes,
                                                _stream()), "cnn_conv2d_backward_data")
        return dx

    def backward(self, x, dy, w, divisor, gw=None, gb=None, dx=None, defer_join=False):
        """both gradients in one call (weight-gradient kernels on the library's side stream, concurrently with dgrad)"""
        import torch

        _need_gpu(x, dy, w, gw, gb, dx)
        d = self.desc
        if self._bwd_ws is None:
            n = int(self.lib.cnn_conv2d_backward_workspace_bytes(C.byref(d)))
            self._bwd_ws = torch.empty(n, dtype=torch.uint8, device=x.device)
        if gw is None:
            gw = torch.empty((d.Co, d.Ci, d.k, d.k), dtype=torch.float32, device=x.device)
        if gb is None:
            gb = torch.empty((d.Co,), dtype=torch.float32, device=x.device)
        if dx is None:
            dx = torch.empty((d.B, d.Ci, d.H, d.W), dtype=torch.float32, device=x.device)
        check(self.lib.cnn_conv2d_backward(C.byref(d), _ptr(x), _ptr(dy), _ptr(w), _ptr(gw), _ptr(gb), _ptr(dx), float(divisor),
                                           _ptr(self._bwd_ws), self._bwd_ws.numel(), _stream(), 1 if defer_join else 0), "cnn_conv2d_backward")
        return gw, gb, dx

    # ---- prepared-filter path (cnn_conv2d_prepare_filters) ----
    def prepared_buffers(self, device="cuda"):
        """(fwd, dgrad) device buffers for prepare_filters()"""
        import torch

        n = int(self.lib.cnn_conv2d_prepared_bytes(C.byref(self.desc)))
        return torch.empty(n, dtype=torch.uint8, device=device), torch.empty(n, dtype=torch.uint8, device=device)

    def relu_only_supported(self):
        return bool(self.lib.cnn_conv2d_relu_only_supported(C.byref(self.desc)))

    def forward_prepared(self, x, prepared_fwd, bias, y, y_relu=None):
        """y may be None (with y_relu) on layers where relu_only_supported(): the pre-activation tensor is then not written"""
        _need_gpu(x, prepared_fwd, bias)
        check(self.lib.cnn_conv2d_forward_prepared(C.byref(self.desc), _ptr(x), _ptr(prepared_fwd), _ptr(bias),
                                                   _ptr(y) if y is not None else None,
                                                   _ptr(y_relu) if y_relu is not None else None, _stream()),
              "cnn_conv2d_forward_prepared")
        return y

    def backward_data_prepared(self, dy, prepared_dgrad, dx):
        _need_gpu(dy, prepared_dgrad, dx)
        check(self.lib.cnn_conv2d_backward_data_prepared(C.byref(self.desc), _ptr(dy), _ptr(prepared_dgrad), _ptr(dx), _stream()),
              "cnn_conv2d_backward_data_prepared")
        return dx

    def backward_prepared(self, x, dy, prepared_dgrad, divisor, gw, gb, dx, defer_join=False, relu_below=None):
        """relu_below: output of the ReLU layer in front of this convolution (= x when that layer feeds it directly); its
        backward pass is applied to dx inside the data-gradient kernel"""
        _need_gpu(x, dy, prepared_dgrad, gw, gb, dx)
        check(self.lib.cnn_conv2d_backward_prepared_relu(C.byref(self.desc), _ptr(x), _ptr(dy), _ptr(prepared_dgrad),
                                                         _ptr(relu_below) if relu_below is not None else None, _ptr(gw), _ptr(gb),
                                                         _ptr(dx), float(divisor), _ptr(self.ws), self.ws_bytes, _stream(),
                                                         1 if defer_join else 0), "cnn_conv2d_backward_prepared")
        return gw, gb, dx

    def backward_data_relu(self, dy, w, relu_below, dx, prepared_dgrad=None):
        _need_gpu(dy, relu_below, dx)
        if prepared_dgrad is not None:
            check(self.lib.cnn_conv2d_backward_data_relu_prepared(C.byref(self.desc), _ptr(dy), _ptr(prepared_dgrad), _ptr(relu_below),
                                                                  _ptr(dx), _stream()), "cnn_conv2d_backward_data_relu_prepared")
        else:
            check(self.lib.cnn_conv2d_backward_data_relu(C.byref(self.desc), _ptr(dy), _ptr(w), _ptr(relu_below), _ptr(dx),
                                                         _ptr(self.ws), self.ws_bytes, _stream()), "cnn_conv2d_backward_data_relu")
        return dx

    # ---- im2col functional fallback (parity cross-check only) ----
    def _iws(self, device):
        import torch

        if self._im2col_ws is None:
            n = int(self.lib.cnn_conv2d_im2col_workspace_bytes(C.byref(self.desc)))
            self._im2col_ws = torch.empty(n, dtype=torch.uint8, device=device)
        return self._im2col_ws

    def forward_im2col(self, x, w, bias):
        import torch

        _need_gpu(x, w, bias)
        y = torch.empty(self.out_shape(), dtype=torch.float32, device=x.device)
        ws = self._iws(x.device)
        check(self.lib.cnn_conv2d_forward_im2col(C.byref(self.desc), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(ws),
                                                 ws.numel(), _stream()), "cnn_conv2d_forward_im2col")
        return y

    def backward_weight_im2col(self, x, dy, divisor):
        import torch

        _need_gpu(x, dy)
        d = self.desc
        gw = torch.empty((d.Co, d.Ci, d.k, d.k), dtype=torch.float32, device=x.device)
        gb = torch.empty((d.Co,), dtype=torch.float32, device=x.device)
        ws = self._iws(x.device)
        check(self.lib.cnn_conv2d_backward_weight_im2col(C.byref(d), _ptr(x), _ptr(dy), _ptr(gw), _ptr(gb), float(divisor),
                                                         _ptr(ws), ws.numel(), _stream()), "cnn_conv2d_backward_weight_im2col")
        return gw, gb

    def backward_data_im2col(self, dy, w):
        import torch

        _need_gpu(dy, w)
        d = self.desc
        dx = torch.empty((d.B, d.Ci, d.H, d.W), dtype=torch.float32, device=dy.device)
        ws = self._iws(dy.device)
        check(self.lib.cnn_conv2d_backward_data_im2col(C.byref(d), _ptr(dy), _ptr(w), _ptr(dx), _ptr(ws), ws.numel(),
                                                       _stream()), "cnn_conv2d_backward_data_im2col")
        return dx


def maxpool_forward(x, k, step, record_mask=True):
    import torch

    _need_gpu(x)
    B, Cc, H, W = x.shape
    Ho, Wo = pool_out_dim(H, k, step), pool_out_dim(W, k, step)
    y = torch.empty((B, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
    mask = torch.empty((B, Cc, Ho, Wo), dtype=torch.int32, device=x.device) if record_mask else None
    check(load().cnn_maxpool2d_forward(_ptr(x), _ptr(y), _ptr(mask), B, Cc, H, W, k, step, _stream()), "cnn_maxpool2d_forward")
    return y, mask


def maxpool_backward(dy, mask, in_shape, k, step, dx=None):
    import torch

    _need_gpu(dy, mask, dx)
    B, Cc, H, W = in_shape
    if dx is None:
        dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    check(load().cnn_maxpool2d_backward(_ptr(dy), _ptr(mask), _ptr(dx), B, Cc, H, W, k, step, _stream()), "cnn_maxpool2d_backward")
    return dx


def maxpool_backward_relu(dy, mask, pooled, in_shape, k, step, dx=None):
    """MaxPool2D::backward + the ReLU::backward of the layer in front of the pool in one kernel (pooled = pool forward output)"""
    import torch

    _need_gpu(dy, mask, pooled, dx)
    B, Cc, H, W = in_shape
    if dx is None:
        dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    check(load().cnn_maxpool2d_backward_relu(_ptr(dy), _ptr(mask), _ptr(pooled), _ptr(dx), B, Cc, H, W, k, step, _stream()),
          "cnn_maxpool2d_backward_relu")
    return dx


def relu_forward(x, y=None):
    import torch

    _need_gpu(x, y)
    if y is None:
        y = torch.empty_like(x)
    check(load().cnn_relu_forward(_ptr(x), _ptr(y), x.numel(), _stream()), "cnn_relu_forward")
    return y


def relu_backward(y, dy):
    """in place on dy (relu.cpp:37-39); returns dy"""
    _need_gpu(y, dy)
    check(load().cnn_relu_backward(_ptr(y), _ptr(dy), y.numel(), _stream()), "cnn_relu_backward")
    return dy


def linear_forward(x, w, bias, y=None):
    import torch

    _need_gpu(x, w, bias, y)
    B = x.shape[0]
    n_in, n_out = w.shape
    if y is None:
        y = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    check(load().cnn_linear_forward(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, n_in, n_out, _stream()), "cnn_linear_forward")
    return y


def linear_backward(x, dy, w, divisor, gw=None, gb=None, dx=None, relu_below=False):
    """relu_below: x is a ReLU layer's output; its backward pass is applied to dx in the same kernel"""
    import torch

    _need_gpu(x, dy, w, gw, gb, dx)
    B = x.shape[0]
    n_in, n_out = w.shape
    if gw is None:
        gw = torch.empty_like(w)
    if gb is None:
        gb = torch.empty((n_out,), dtype=torch.float32, device=x.device)
    if dx is None:
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    fn = load().cnn_linear_backward_relu if relu_below else load().cnn_linear_backward
    check(fn(_ptr(x), _ptr(dy), _ptr(w), _ptr(gw), _ptr(gb), _ptr(dx), B, n_in, n_out, float(divisor), _stream()),
          "cnn_linear_backward")
    return gw, gb, dx


class BatchNorm2d:
    """BatchNorm2D on the HIP path (batchnorm2d.cpp:6-182): owns the workspace and the saved batch statistics; gamma,
    beta and the moving statistics are caller tensors of [C] (checkpoint order gamma, beta, moving_mean, moving_var,
    batchnorm2d.cpp:168-173)."""

    def __init__(self, batch, channels, H, W, eps=1e-5, momentum=0.1, device="cuda"):
        import torch

        self.B, self.C, self.H, self.W, self.eps, self.momentum = batch, channels, H, W, eps, momentum
        self.ws_bytes = load().cnn_batchnorm2d_workspace_bytes(batch, channels, H, W)
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=device)
        self.saved_mean = torch.zeros(channels, dtype=torch.float32, device=device)
        self.saved_var = torch.zeros(channels, dtype=torch.float32, device=device)

    def forward(self, x, gamma, beta, moving_mean, moving_var, y, training=True, y_relu=None):
        """y_relu: also write relu(y) (the ReLU layer behind this one) from the same pass"""
        _need_gpu(x, y, gamma, beta, moving_mean, moving_var)
        if y_relu is not None:
            _need_gpu(y_relu)
            check(load().cnn_batchnorm2d_forward_relu(_ptr(x), _ptr(y), _ptr(y_relu), _ptr(gamma), _ptr(beta), _ptr(moving_mean),
                                                      _ptr(moving_var), _ptr(self.saved_mean), _ptr(self.saved_var), self.B, self.C,
                                                      self.H, self.W, self.eps, self.momentum, 1 if training else 0, _ptr(self.ws),
                                                      self.ws_bytes, _stream()), "cnn_batchnorm2d_forward_relu")
            return y
        check(load().cnn_batchnorm2d_forward(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var),
                                             _ptr(self.saved_mean), _ptr(self.saved_var), self.B, self.C, self.H, self.W,
                                             self.eps, self.momentum, 1 if training else 0, _ptr(self.ws), self.ws_bytes,
                                             _stream()), "cnn_batchnorm2d_forward")
        return y

    # ---- sync-BN: the batch is sharded over `world` data-parallel ranks; `allreduce(t)` sums a small tensor in place ----
    def forward_sync(self, x, gamma, beta, moving_mean, moving_var, y, allreduce, global_count, y_relu=None):
        """training forward over the GLOBAL batch (batchnorm2d.cpp:46-80): two tiny all-reduces of [C] sums
        (y_relu: also write relu(y), the output of the ReLU layer behind this one)"""
        import torch

        _need_gpu(x, y, gamma, beta, moving_mean, moving_var)
        L = load()
        s1 = torch.empty(self.C, dtype=torch.float32, device=x.device)
        s2 = torch.empty_like(s1)
        dims = (self.B, self.C, self.H, self.W)
        check(L.cnn_batchnorm2d_partial_sums(_ptr(x), None, 0.0, _ptr(s1), *dims, _ptr(self.ws), self.ws_bytes, _stream()), "bn sums 1")
        allreduce(s1)
        check(L.cnn_batchnorm2d_partial_sums(_ptr(x), _ptr(s1), float(global_count), _ptr(s2), *dims, _ptr(self.ws), self.ws_bytes,
                                             _stream()), "bn sums 2")
        allreduce(s2)
        if y_relu is not None:
            _need_gpu(y_relu)
            check(L.cnn_batchnorm2d_forward_from_sums_relu(_ptr(x), _ptr(y), _ptr(y_relu), _ptr(gamma), _ptr(beta), _ptr(moving_mean),
                                                           _ptr(moving_var), _ptr(self.saved_mean), _ptr(self.saved_var), _ptr(s1), _ptr(s2),
                                                           float(global_count), *dims, self.eps, self.momentum, _stream()),
                  "cnn_batchnorm2d_forward_from_sums_relu")
            return y
        check(L.cnn_batchnorm2d_forward_from_sums(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var),
                                                  _ptr(self.saved_mean), _ptr(self.saved_var), _ptr(s1), _ptr(s2), float(global_count),
                                                  *dims, self.eps, self.momentum, _stream()), "cnn_batchnorm2d_forward_from_sums")
        return y

    def backward_sync(self, x, dy, gamma, ggamma, gbeta, allreduce, global_count):
        """dy -> dx in place; ggamma / gbeta come out as the full-batch sums on every rank (one [C][4] all-reduce)"""
        import torch

        _need_gpu(x, dy, gamma, ggamma, gbeta)
        L = load()
        s4 = torch.empty(self.C * 4, dtype=torch.float32, device=x.device)
        dims = (self.B, self.C, self.H, self.W)
        check(L.cnn_batchnorm2d_backward_sums(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(self.saved_mean), _ptr(self.saved_var), _ptr(s4),
                                              *dims, self.eps, _ptr(self.ws), self.ws_bytes, _stream()), "cnn_batchnorm2d_backward_sums")
        allreduce(s4)
        check(L.cnn_batchnorm2d_backward_from_sums(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(self.saved_mean), _ptr(self.saved_var), _ptr(s4),
                                                   float(global_count), _ptr(ggamma), _ptr(gbeta), *dims, self.eps, _stream()),
              "cnn_batchnorm2d_backward_from_sums")
        return dy

    def backward(self, x, dy, gamma, ggamma, gbeta):
        """dy -> dx in place (batchnorm2d.cpp:149-155)"""
        _need_gpu(x, dy, gamma, ggamma, gbeta)
        check(load().cnn_batchnorm2d_backward(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(self.saved_mean), _ptr(self.saved_var),
                                              _ptr(ggamma), _ptr(gbeta), self.B, self.C, self.H, self.W, self.eps,
                                              _ptr(self.ws), self.ws_bytes, _stream()), "cnn_batchnorm2d_backward")
        return dy

    def forward_relu_pool(self, x, gamma, beta, moving_mean, moving_var, pooled, mask, y=None, y_relu=None, training=True):
        """BatchNorm2D -> ReLU -> MaxPool2D(2, 2) in one apply pass: pooled / mask written, y / y_relu only when given"""
        check(load().cnn_batchnorm2d_forward_relu_pool(_ptr(x), _ptr(y), _ptr(y_relu), _ptr(pooled), _ptr(mask), _ptr(gamma), _ptr(beta),
                                                       _ptr(moving_mean), _ptr(moving_var), _ptr(self.saved_mean), _ptr(self.saved_var), self.B,
                                                       self.C, self.H, self.W, self.eps, self.momentum, 1 if training else 0, _ptr(self.ws),
                                                       self.ws_bytes, _stream()), "cnn_batchnorm2d_forward_relu_pool")
        return pooled

    def backward_pooled_supported(self):
        return bool(load().cnn_batchnorm2d_backward_pooled_supported(self.B, self.C, self.H, self.W))

    def backward_pooled(self, x, dpool, mask, pooled, gamma, ggamma, gbeta, dx):
        """BatchNorm2D <- ReLU <- MaxPool2D(2, 2) backward from the pooled domain (dpool, the pool's int32 mask and output): dx written,
        ggamma / gbeta filled; bit-identical to maxpool2d_backward_relu + backward"""
        check(load().cnn_batchnorm2d_backward_pooled(_ptr(x), _ptr(dpool), _ptr(mask), _ptr(pooled), _ptr(dx), _ptr(gamma), _ptr(self.saved_mean),
                                                     _ptr(self.saved_var), _ptr(ggamma), _ptr(gbeta), self.B, self.C, self.H, self.W, self.eps,
                                                     _ptr(self.ws), self.ws_bytes, _stream()), "cnn_batchnorm2d_backward_pooled")
        return dx


def prepare_filters(convs, weights, biases, fwd_bufs, dgrad_bufs):
    """re-arrange the filters of up to 6 layers for their forward / data-gradient kernels with one or two launches"""
    n = len(convs)
    _need_gpu(*weights, *biases)
    descs = (ConvDesc * n)(*[c.desc for c in convs])
    arr = lambda ts: (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in ts])
    check(load().cnn_conv2d_prepare_filters(n, descs, arr(weights), arr(biases), arr(fwd_bufs) if fwd_bufs else None,
                                            arr(dgrad_bufs) if dgrad_bufs else None, _stream()), "cnn_conv2d_prepare_filters")


def sgd_update(params, grads, lr, grad_scale=1.0):
    _need_gpu(params, grads)
    check(load().cnn_sgd_update(_ptr(params), _ptr(grads), params.numel(), float(lr), float(grad_scale), _stream()), "cnn_sgd_update")
    return params


def sgd_momentum_update(params, grads, velocity, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, decay_ranges=(),
                        previous=None, n=None):
    """cnn_sgd_momentum_update on device tensors (or views of them); decay_ranges: [(begin, end)] relative to params, ascending.
    Tables longer than SGD_INLINE_RANGES are uploaded here (a caller that steps repeatedly would keep the device copy)."""
    import numpy as np
    import torch

    _need_gpu(params, grads, velocity, previous)
    n = params.numel() if n is None else int(n)
    opt = SgdOptions(float(lr), float(momentum), float(weight_decay), 1 if nesterov else 0)
    table = np.ascontiguousarray(np.asarray(list(decay_ranges), dtype=np.uint32).reshape(-1, 2))
    n_ranges = table.shape[0]
    dev = torch.from_numpy(table.view(np.int32).reshape(-1)).to(params.device) if n_ranges > SGD_INLINE_RANGES else None
    check(load().cnn_sgd_momentum_update(_ptr(params), _ptr(grads), _ptr(velocity), n, C.byref(opt), float(grad_scale),
                                         table.ctypes.data_as(C.c_void_p) if n_ranges else None, _ptr(dev), n_ranges, _ptr(previous), _stream()),
          "cnn_sgd_momentum_update")
    if dev is not None:
        torch.cuda.current_stream().synchronize()  # (the table must outlive the kernel that reads it)
    return params


def adam_update(params, grads, exp_avg, exp_avg_sq, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, step=1,
                grad_scale=1.0, decay_ranges=(), previous=None, n=None):
    """cnn_adam_update on device tensors (or views of them); step: the 1-based number of this step; decay_ranges as in
    sgd_momentum_update, tables longer than SGD_INLINE_RANGES are uploaded here"""
    import numpy as np
    import torch

    _need_gpu(params, grads, exp_avg, exp_avg_sq, previous)
    n = params.numel() if n is None else int(n)
    opt = AdamOptions(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), 1 if decoupled else 0, int(step))
    table = np.ascontiguousarray(np.asarray(list(decay_ranges), dtype=np.uint32).reshape(-1, 2))
    n_ranges = table.shape[0]
    dev = torch.from_numpy(table.view(np.int32).reshape(-1)).to(params.device) if n_ranges > SGD_INLINE_RANGES else None
    check(load().cnn_adam_update(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, C.byref(opt), float(grad_scale),
                                 table.ctypes.data_as(C.c_void_p) if n_ranges else None, _ptr(dev), n_ranges, _ptr(previous), _stream()),
          "cnn_adam_update")
    if dev is not None:
        torch.cuda.current_stream().synchronize()  # (the table must outlive the kernel that reads it)
    return params


def clip_grad_norm(grads, max_norm, grad_scale=1.0, n=None):
    """cnn_clip_grad_norm on a device tensor (or a view of one), in place -> the stats tensor [total norm, coefficient] on the
    device (reading it is the caller's synchronisation)"""
    import torch

    _need_gpu(grads)
    n = grads.numel() if n is None else int(n)
    lib = load()
    ws_bytes = int(lib.cnn_clip_grad_norm_workspace_bytes(n))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=grads.device)
    stats = torch.empty(2, dtype=torch.float32, device=grads.device)
    check(lib.cnn_clip_grad_norm(_ptr(grads), n, float(max_norm), float(grad_scale), _ptr(ws), ws_bytes, _ptr(stats), _stream()),
          "cnn_clip_grad_norm")
    torch.cuda.current_stream().synchronize()  # (the workspace must outlive the kernels that use it)
    return stats


def grad_accumulate(acc, grads, first, n=None):
    """cnn_grad_accumulate on device tensors (or views of them): acc = grads (first: a copy of the bits) or acc += grads"""
    _need_gpu(acc, grads)
    n = acc.numel() if n is None else int(n)
    check(load().cnn_grad_accumulate(_ptr(acc), _ptr(grads), n, 1 if first else 0, _stream()), "cnn_grad_accumulate")
    return acc


def ema_decay_at(decay, warmup, updates_done):
    """cnn_ema_decay_at: the decay of the update that follows updates_done earlier ones (host only)"""
    return float(load().cnn_ema_decay_at(float(decay), 1 if warmup else 0, int(updates_done)))


def ema_update(ema, params, decay, avg_ranges=(), n=None):
    """cnn_ema_update on device tensors (or views of them): ema = decay * ema + (1 - decay) * params inside avg_ranges ([(begin, end)]
    relative to params, ascending), a copy of the bits elsewhere and everywhere with decay 0.  Tables longer than SGD_INLINE_RANGES
    are uploaded here (a caller that updates repeatedly would keep the device copy)."""
    import numpy as np
    import torch

    _need_gpu(ema, params)
    n = ema.numel() if n is None else int(n)
    table = np.ascontiguousarray(np.asarray(list(avg_ranges), dtype=np.uint32).reshape(-1, 2))
    n_ranges = table.shape[0]
    dev = torch.from_numpy(table.view(np.int32).reshape(-1)).to(ema.device) if n_ranges > SGD_INLINE_RANGES else None
    check(load().cnn_ema_update(_ptr(ema), _ptr(params), n, float(decay), table.ctypes.data_as(C.c_void_p) if n_ranges else None, _ptr(dev),
                                n_ranges, _stream()), "cnn_ema_update")
    if dev is not None:
        torch.cuda.current_stream().synchronize()  # (the table must outlive the kernel that reads it)
    return ema


def arena_swap(a, b, n=None):
    """cnn_arena_swap on device tensors (or views of them): the bits of two disjoint buffers change places"""
    _need_gpu(a, b)
    n = a.numel() if n is None else int(n)
    check(load().cnn_arena_swap(_ptr(a), _ptr(b), n, _stream()), "cnn_arena_swap")


class Layerwise:
    """cnn_layerwise_create's handle: the flat range [0, n) cut into tensors.  bounds: n_segments + 1 ascending offsets from 0 to n;
    flags: SEG_DECAY | SEG_ADAPT per segment.  The tensors passed to the methods hold at least n floats from their data pointer."""

    def __init__(self, bounds, flags):
        import numpy as np

        self.bounds = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint32).reshape(-1))
        self.flags = np.ascontiguousarray(np.asarray(flags, dtype=np.uint32).reshape(-1))
        if self.bounds.size != self.flags.size + 1:
            raise CnnAmdError(f"Layerwise: {self.bounds.size} bounds for {self.flags.size} segments (one more is needed)")
        self.n_segments = int(self.flags.size)
        self.n = int(self.bounds[-1]) if self.bounds.size else 0
        self.h = C.c_void_p()
        check(load().cnn_layerwise_create(self.bounds.ctypes.data_as(C.c_void_p), self.flags.ctypes.data_as(C.c_void_p), self.n_segments,
                                          C.byref(self.h)), "cnn_layerwise_create")

    def close(self):
        if self.h:
            check(load().cnn_layerwise_destroy(self.h), "cnn_layerwise_destroy")
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fits(self, what, *tensors):
        _need_gpu(*tensors)
        for t in tensors:
            if t is not None and t.numel() < self.n:
                raise CnnAmdError(f"{what}: a tensor of {t.numel()} floats, the segment table ends at n={self.n}")

    def stats(self):
        """(w_norm, u_norm, ratio) of the latest update call, copied to the host (synchronises)"""
        import numpy as np
        import torch

        ptr = C.c_void_p()
        check(load().cnn_layerwise_stats(self.h, C.byref(ptr)), "cnn_layerwise_stats")
        host = torch.empty(3 * self.n_segments, dtype=torch.float32)
        check(load().cnn_memcpy_d2h(C.c_void_p(host.data_ptr()), ptr, 4 * 3 * self.n_segments, _stream()), "cnn_memcpy_d2h")
        torch.cuda.current_stream().synchronize()
        a = host.numpy().reshape(3, self.n_segments)
        return np.array(a[0]), np.array(a[1]), np.array(a[2])

    def segment_norms(self, x, out=None):
        """cnn_segment_norms -> a device tensor of n_segments floats"""
        import torch

        self._fits("segment_norms", x)
        out = torch.empty(self.n_segments, dtype=torch.float32, device=x.device) if out is None else out
        check(load().cnn_segment_norms(self.h, _ptr(x), _ptr(out), _stream()), "cnn_segment_norms")
        return out

    def lamb_update(self, params, grads, exp_avg, exp_avg_sq, update, lr, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, step=1,
                    grad_scale=1.0, previous=None):
        """cnn_lamb_update on device tensors (or views of them); update: n floats of scratch that receive r"""
        self._fits("lamb_update", params, grads, exp_avg, exp_avg_sq, update, previous)
        opt = LambOptions(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
        check(load().cnn_lamb_update(self.h, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(update), C.byref(opt),
                                     float(grad_scale), _ptr(previous), _stream()), "cnn_lamb_update")
        return params

    def lars_update(self, params, grads, velocity, lr, momentum=0.0, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8, nesterov=False,
                    grad_scale=1.0, previous=None):
        """cnn_lars_update on device tensors (or views of them); velocity may be None with momentum == 0"""
        self._fits("lars_update", params, grads, velocity, previous)
        opt = LarsOptions(float(lr), float(momentum), float(weight_decay), float(trust_coefficient), float(eps), 1 if nesterov else 0)
        check(load().cnn_lars_update(self.h, _ptr(params), _ptr(grads), _ptr(velocity), C.byref(opt), float(grad_scale), _ptr(previous),
                                     _stream()), "cnn_lars_update")
        return params


def softmax_xent(logits, labels, want_probs=True):
    import torch

    _need_gpu(logits, labels)
    B, n = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    delta = torch.empty_like(logits)
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    check(load().cnn_softmax_xent(_ptr(logits), _ptr(labels), _ptr(probs), _ptr(delta), _ptr(loss), B, n, _stream()), "cnn_softmax_xent")
    return probs, delta, loss


def softmax_xent_soft(logits, targets, want_probs=True):
    """cnn_softmax_xent_soft: cnn_softmax_xent against a dense float32 [B][classes] target tensor"""
    import torch

    _need_gpu(logits, targets)
    B, n = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    delta = torch.empty_like(logits)
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    check(load().cnn_softmax_xent_soft(_ptr(logits), _ptr(targets), _ptr(probs), _ptr(delta), _ptr(loss), B, n, _stream()), "cnn_softmax_xent_soft")
    return probs, delta, loss


def eval_state_bytes(classes):
    """cnn_eval_state_bytes: the size of the evaluation state block of `classes` classes (host only)"""
    n = int(load().cnn_eval_state_bytes(int(classes)))
    if n == 0:
        raise CnnAmdError("cnn_eval_state_bytes: " + load().cnn_amd_last_error().decode())
    return n


def eval_accumulate(logits, labels, state, k=1, pred=None):
    """cnn_eval_accumulate: one batch of float32 [B][classes] logits and int32 [B] labels (device) into the state block -- loss, top-1 /
    top-k and confusion counts, one launch, no read-back; pred: optional int32 [B] device tensor that receives the predictions"""
    _need_gpu(logits, labels, state, pred)
    B, n = logits.shape
    check(load().cnn_eval_accumulate(_ptr(logits), _ptr(labels), _ptr(pred), _ptr(state), B, n, int(k), _stream()), "cnn_eval_accumulate")
    return pred


def eval_read(state, classes, want_confusion=True):
    """cnn_eval_read: the one call that copies the state back (synchronises) -> dict of samples, top1, topk, ignored, loss_sum and, with
    want_confusion, confusion (numpy uint64 [classes][classes], row = label, column = prediction)"""
    import numpy as np

    _need_gpu(state)
    res = EvalResult()
    conf = np.zeros((classes, classes), dtype=np.uint64) if want_confusion else None
    check(load().cnn_eval_read(_ptr(state), int(classes), C.byref(res), conf.ctypes.data_as(C.c_void_p) if want_confusion else None, _stream()),
          "cnn_eval_read")
    out = {"samples": int(res.samples), "top1": int(res.top1), "topk": int(res.topk), "ignored": int(res.ignored), "loss_sum": float(res.loss_sum)}
    if want_confusion:
        out["confusion"] = conf
    return out


def soft_targets(labels, classes, smoothing=0.0, lam=1.0, pair_rule=PAIR_NONE, pair_shift=0, out=None):
    """cnn_soft_targets: labels int32 [B] (device) -> float32 [B][classes] target rows: label smoothing, and the mix lam * own +
    (1 - lam) * partner's under a pair rule (PAIR_FLIP: B - 1 - b, PAIR_ROLL: (b + pair_shift) % B)"""
    import torch

    _need_gpu(labels, out)
    B = labels.shape[0]
    if out is None:
        out = torch.empty((B, classes), dtype=torch.float32, device=labels.device)
    check(load().cnn_soft_targets(_ptr(labels), _ptr(out), B, int(classes), float(smoothing), float(lam), int(pair_rule), int(pair_shift), _stream()),
          "cnn_soft_targets")
    return out


def cutmix_lambda(H, W, y0, y1, x0, x1):
    """cnn_cutmix_lambda: the weight of the sample itself under a CutMix box (host only)"""
    return float(load().cnn_cutmix_lambda(int(H), int(W), int(y0), int(y1), int(x0), int(x1)))


def batch_mix(mix, src, dst=None):
    """cnn_batch_mix: mixup / CutMix of a float32 [B][C][H][W] device batch with its partner samples, out of place; mix: a MixDesc"""
    import torch

    _need_gpu(src, dst)
    B, Cc, H, W = src.shape
    if dst is None:
        dst = torch.empty_like(src)
    check(load().cnn_batch_mix(C.byref(mix), _ptr(src), _ptr(dst), B, Cc, H, W, _stream()), "cnn_batch_mix")
    return dst


def augment_matrix(ops, Hs, Ws, H, W):
    """cnn_augment_matrix (host only): ops, a sequence of AugmentOp or (kind, a, b, c, d) tuples (trailing values may be left out),
    applied in order to the Hs x Ws source, then the resize to H x W -> the six float32 of the output -> source map"""
    import numpy as np

    arr = (AugmentOp * max(len(ops), 1))()
    for i, op in enumerate(ops):
        arr[i] = op if isinstance(op, AugmentOp) else AugmentOp(int(op[0]), *[float(v) for v in op[1:]])
    m = np.empty(6, dtype=np.float32)
    check(load().cnn_augment_matrix(arr, len(ops), int(Hs), int(Ws), int(H), int(W), m.ctypes.data_as(C.POINTER(C.c_float))), "cnn_augment_matrix")
    return m


def colour_matrix(ops):
    """cnn_colour_matrix (host only): ops, a sequence of ColourOp or (kind, a[, b]) tuples, applied in order with no clamp between them
    -> (12,) float32: A row-major and o, the first twelve floats of a sample's photo block (BatchStager.photo(slot))"""
    import numpy as np

    arr = (ColourOp * max(len(ops), 1))()
    for i, op in enumerate(ops):
        arr[i] = op if isinstance(op, ColourOp) else ColourOp(int(op[0]), *[float(v) for v in op[1:]])
    out = np.empty(12, dtype=np.float32)
    check(load().cnn_colour_matrix(arr, len(ops), out.ctypes.data_as(C.POINTER(C.c_float))), "cnn_colour_matrix")
    return out


def augment_u8(src_u8, matrices, H, W, fill=0.0, out=None):
    """cnn_augment_u8: uint8 [B][Hs][Ws][3] and float32 [B][6] device tensors -> the float32 [B][3][H][W] batch, one launch"""
    import torch

    _need_gpu(src_u8, matrices, out)
    B, Hs, Ws, ch = src_u8.shape
    if ch != 3 or src_u8.dtype != torch.uint8 or matrices.dtype != torch.float32 or tuple(matrices.shape) != (B, 6):
        raise CnnAmdError("augment_u8: src must be uint8 [B][Hs][Ws][3] and matrices float32 [B][6]")
    if out is None:
        out = torch.empty((B, 3, int(H), int(W)), dtype=torch.float32, device=src_u8.device)
    check(load().cnn_augment_u8(_ptr(src_u8), B, Hs, Ws, _ptr(matrices), float(fill), _ptr(out), int(H), int(W), _stream()), "cnn_augment_u8")
    return out


def set_option(name, value):
    """one of the measurement switches of DESIGN.md section 10 (name with or without the CNN_AMD_ prefix); value None removes it.
    The library reads the CNN_AMD_* environment once, at first use: later changes go through here."""
    check(load().cnn_amd_set_option(name.encode(), None if value is None else str(value).encode()), "cnn_amd_set_option")


def get_option(name):
    buf = C.create_string_buffer(256)
    return buf.value.decode() if load().cnn_amd_get_option(name.encode(), buf, 256) == 0 else None


class option:
    """with capi.option("RD_SLOW", 1): ...   -- sets the switch, restores the previous state on exit"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def kernel_timing(mode, filter_key="", every=1):
    """0 = off, 1 = every kernel, 2 = only keys containing filter_key (and of those only every `every`-th launch)"""
    check(load().cnn_amd_kernel_timing_sampling(int(every)), "cnn_amd_kernel_timing_sampling")
    check(load().cnn_amd_kernel_timing_enable(int(mode), filter_key.encode()), "cnn_amd_kernel_timing_enable")


def kernel_timing_report():
    """-> {key: (launches, total_ms)} in first-launch order; clears the records"""
    lib = load()
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        need = lib.cnn_amd_kernel_timing_report(buf, cap)
        if need < 0:
            raise CnnAmdError("cnn_amd_kernel_timing_report failed")
        if need <= cap:
            break
        cap = int(need) + 64
    out = {}
    for line in buf.value.decode().splitlines():
        key, cnt, ms = line.rsplit("\t", 2)
        out[key] = (int(cnt), float(ms))
    return out


def grad_cam(feature):
    """AlexNet::grad_cam's arithmetic on a [B][C][H][W] feature map: (normalised cam [B][H][W], uint8 image [H][W] of plane 0)"""
    import torch

    _need_gpu(feature)
    B, Cc, H, W = feature.shape
    cam = torch.empty((B, H, W), dtype=torch.float32, device=feature.device)
    img = torch.empty((H, W), dtype=torch.uint8, device=feature.device)
    check(load().cnn_grad_cam(_ptr(feature), B, Cc, H, W, _ptr(cam), _ptr(img), _stream()), "cnn_grad_cam")
    return cam, img


def side_stream():
    """the library's side stream of this thread / device as a torch stream (work queued there runs behind the deferred weight gradients)"""
    import torch

    out = C.c_void_p()
    check(load().cnn_amd_side_stream_get(C.byref(out)), "cnn_amd_side_stream_get")
    return torch.cuda.ExternalStream(out.value)


def flush_reduces():
    """launch the recorded weight-gradient slab reductions on the CURRENT stream now (see cnn_amd_flush_reduces)"""
    check(load().cnn_amd_flush_reduces(_stream()), "cnn_amd_flush_reduces")


def publish_next_kernel():
    """the next library kernel on the current stream publishes its completion (see cnn_amd_publish_next_kernel)"""
    check(load().cnn_amd_publish_next_kernel(_stream()), "cnn_amd_publish_next_kernel")


def wait_published(stream=None):
    """`stream` (a torch stream; default: the current one) waits for the published kernel"""
    check(load().cnn_amd_wait_published(C.c_void_p(stream.cuda_stream) if stream is not None else _stream()), "cnn_amd_wait_published")


def side_stream_join():
    """order the library's side stream (deferred weight gradients) before the current stream"""
    check(load().cnn_amd_side_stream_join(_stream()), "cnn_amd_side_stream_join")


def dataset_max_levels(Hs, Ws):
    """cnn_dataset_max_levels: how many half-size levels an Hs x Ws image has until both dimensions are 1 (host only)"""
    n = load().cnn_dataset_max_levels(int(Hs), int(Ws))
    if n <= 0:
        raise CnnAmdError(f"cnn_dataset_max_levels: {load().cnn_amd_last_error().decode()}")
    return n


def augment_level(m, levels):
    """cnn_augment_level: -> (level, float32 (6,) map on that level) a levelled resident stager's submit() picks for the map m of a
    dataset with `levels` levels (host only)"""
    import numpy as np

    src = np.ascontiguousarray(m, dtype=np.float32).reshape(6)
    out, level = np.empty(6, np.float32), C.c_int()
    check(load().cnn_augment_level(src.ctypes.data_as(C.POINTER(C.c_float)), int(levels), C.byref(level), out.ctypes.data_as(C.POINTER(C.c_float))),
          "cnn_augment_level")
    return int(level.value), out


class ResidentDataset:
    """cnn_dataset_*: N images of Hs x Ws x 3 bytes and N int32 labels in device memory (bytes 0 and labels -1 until written); the source
    of BatchStager(u8_shape=..., resident=ds).  levels > 1: each image keeps levels - 1 prefiltered half-size copies, rebuilt by write(),
    and an attached stager gathers every sample from the level whose residual shrink is below 2 (cnn_dataset_create_u8_levels).  Close
    the stagers before the dataset."""

    def __init__(self, N, Hs, Ws, levels=1):
        self.lib = load()
        self.h = C.c_void_p()
        check(self.lib.cnn_dataset_create_u8_levels(C.byref(self.h), int(N), int(Hs), int(Ws), int(levels)), "cnn_dataset_create_u8_levels")
        self.N, self.Hs, self.Ws, self.levels = int(N), int(Hs), int(Ws), int(levels)

    def level_shape(self, level):
        """-> (H_l, W_l) of level `level` as the library holds them"""
        n, h, w = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.cnn_dataset_level_info(self.h, C.byref(n), int(level), C.byref(h), C.byref(w)), "cnn_dataset_level_info")
        return int(h.value), int(w.value)

    def read_level(self, level, first, count):
        """-> uint8 (count, H_l, W_l, 3) of samples first .. first + count - 1 at level `level`; blocks"""
        import numpy as np

        h, w = self.level_shape(level)
        count = int(count)
        images = np.empty((max(count, 0), h, w, 3), np.uint8)
        check(self.lib.cnn_dataset_read_level(self.h, int(level), int(first), count, images.ctypes.data_as(C.c_void_p)), "cnn_dataset_read_level")
        return images

    def write(self, first, images_u8=None, labels=None):
        """samples first .. first + count - 1: images_u8 uint8 (count, Hs, Ws, 3) and / or labels int32 (count,), host arrays; blocks.
        Waits first for every gather the attached stagers have submitted"""
        import numpy as np

        if images_u8 is None and labels is None:
            raise CnnAmdError("ResidentDataset.write: images_u8 and labels are both None")
        count = None
        if images_u8 is not None:
            images_u8 = np.ascontiguousarray(images_u8, dtype=np.uint8)
            if images_u8.ndim != 4 or images_u8.shape[1:] != (self.Hs, self.Ws, 3):
                raise CnnAmdError(f"ResidentDataset.write: images must be uint8 (count, {self.Hs}, {self.Ws}, 3)")
            count = images_u8.shape[0]
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
            if count is not None and labels.size != count:
                raise CnnAmdError("ResidentDataset.write: as many labels as images")
            count = labels.size
        check(self.lib.cnn_dataset_write(self.h, int(first), int(count), images_u8.ctypes.data_as(C.c_void_p) if images_u8 is not None else None,
                                         labels.ctypes.data_as(C.c_void_p) if labels is not None else None), "cnn_dataset_write")

    def read(self, first, count):
        """-> (uint8 (count, Hs, Ws, 3), int32 (count,)) of samples first .. first + count - 1; blocks"""
        import numpy as np

        count = int(count)
        images, labels = np.empty((max(count, 0), self.Hs, self.Ws, 3), np.uint8), np.empty(max(count, 0), np.int32)
        check(self.lib.cnn_dataset_read(self.h, int(first), count, images.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p)),
              "cnn_dataset_read")
        return images, labels

    def info(self):
        """-> (N, Hs, Ws) as the library holds them"""
        n, hs, ws = C.c_longlong(), C.c_int(), C.c_int()
        check(self.lib.cnn_dataset_info(self.h, C.byref(n), C.byref(hs), C.byref(ws)), "cnn_dataset_info")
        return int(n.value), int(hs.value), int(ws.value)

    def close(self):
        """cnn_dataset_destroy; raises while a stager is attached (and the dataset stays as it is)"""
        if self.h:
            check(self.lib.cnn_dataset_destroy(self.h), "cnn_dataset_destroy")
            self.h = None


class BatchStager:
    """cnn_batch_stager_*: `depth` pinned host slots + device buffers, uploads on a copy stream of its own, ordered by events"""

    def __init__(self, batch_bytes=None, depth=2, u8_shape=None, source_shape=None, augment=False, photo=False, resident=None):
        """u8_shape=(B, H, W): the slots hold interleaved BYTES [B][H][W][3] (cv::Mat CV_8UC3), submit() returns the fp32 planar batch
        the stager's conversion kernel writes (cnn_batch_stager_create_u8).  augment=True or source_shape=(Hs, Ws): the slots hold
        [B][Hs][Ws][3] bytes (Hs, Ws = H, W when source_shape is None) and per-sample maps, matrices(slot); submit() returns the
        [B][3][H][W] batch cnn_augment_u8 writes through them (cnn_batch_stager_create_u8_aug).  photo=True: an augmenting stager
        whose slots also carry (B, 20) photometric parameters, photo(slot) -- colour matrix, erase box -- and whose kernel applies them
        and set_normalize()'s mean / std behind the gather (cnn_batch_stager_create_u8_photo).  resident=ds (a ResidentDataset): a
        photo stager whose images are gathered out of ds by the slot's indices(slot); acquire() returns (None, slot), labels(slot) is
        the device pointer of the gathered labels (cnn_batch_stager_create_u8_resident)"""
        self.lib = load()
        self.h = C.c_void_p()
        self.u8 = u8_shape is not None
        self.resident = resident
        self.is_photo = bool(photo) or resident is not None
        self.aug = bool(augment) or source_shape is not None or self.is_photo
        if self.aug and not self.u8:
            raise CnnAmdError("BatchStager: augment / source_shape need u8_shape=(B, H, W)")
        if resident is not None:
            if source_shape is not None:
                raise CnnAmdError("BatchStager: a resident stager's source shape is its dataset's")
            B, H, W = (int(v) for v in u8_shape)
            self.B, self.H, self.W, self.bytes = B, H, W, 0
            check(self.lib.cnn_batch_stager_create_u8_resident(C.byref(self.h), resident.h, B, H, W, depth), "cnn_batch_stager_create_u8_resident")
        elif self.aug:
            B, H, W = (int(v) for v in u8_shape)
            Hs, Ws = (H, W) if source_shape is None else (int(v) for v in source_shape)
            self.B, self.bytes = B, B * Hs * Ws * 3
            if self.is_photo:
                check(self.lib.cnn_batch_stager_create_u8_photo(C.byref(self.h), B, Hs, Ws, H, W, depth), "cnn_batch_stager_create_u8_photo")
            else:
                check(self.lib.cnn_batch_stager_create_u8_aug(C.byref(self.h), B, Hs, Ws, H, W, depth), "cnn_batch_stager_create_u8_aug")
        elif self.u8:
            B, H, W = (int(v) for v in u8_shape)
            self.bytes = B * H * W * 3
            check(self.lib.cnn_batch_stager_create_u8(C.byref(self.h), B, H, W, depth), "cnn_batch_stager_create_u8")
        else:
            self.bytes = int(batch_bytes)
            check(self.lib.cnn_batch_stager_create(C.byref(self.h), self.bytes, depth), "cnn_batch_stager_create")

    def matrices(self, slot):
        """-> numpy (B, 6) float32 view of the slot's pinned maps (an augmenting stager; acquire() preset them to the plain resize)"""
        import numpy as np

        p = C.POINTER(C.c_float)()
        check(self.lib.cnn_batch_stager_matrices(self.h, int(slot), C.byref(p)), "cnn_batch_stager_matrices")
        return np.ctypeslib.as_array((C.c_float * (self.B * 6)).from_address(C.addressof(p.contents))).reshape(self.B, 6)

    def set_fill(self, fill):
        """the value of output pixels whose sample position lies outside the source (an augmenting stager; default 0)"""
        check(self.lib.cnn_batch_stager_set_fill(self.h, float(fill)), "cnn_batch_stager_set_fill")

    def photo(self, slot):
        """-> numpy (B, 20) float32 view of the slot's pinned photometric parameters (a photo stager; acquire() preset them to the
        identity: A = I, o = 0, no box)"""
        import numpy as np

        p = C.POINTER(C.c_float)()
        check(self.lib.cnn_batch_stager_photo(self.h, int(slot), C.byref(p)), "cnn_batch_stager_photo")
        B = getattr(self, "B", 0)
        return np.ctypeslib.as_array((C.c_float * (B * PHOTO_FLOATS)).from_address(C.addressof(p.contents))).reshape(B, PHOTO_FLOATS)

    def indices(self, slot):
        """-> numpy (B,) int32 view of the slot's pinned sample indices (a resident stager; acquire() preset them to -1: no sample)"""
        import numpy as np

        p = C.POINTER(C.c_int)()
        check(self.lib.cnn_batch_stager_indices(self.h, int(slot), C.byref(p)), "cnn_batch_stager_indices")
        B = getattr(self, "B", 0)
        return np.ctypeslib.as_array((C.c_int * B).from_address(C.addressof(p.contents)))

    def levels(self, slot):
        """-> numpy (B,) int32 copy of the levels the slot's last submit() chose (a resident stager on a dataset with levels > 1)"""
        import numpy as np

        p = C.POINTER(C.c_int)()
        check(self.lib.cnn_batch_stager_levels(self.h, int(slot), C.byref(p)), "cnn_batch_stager_levels")
        B = getattr(self, "B", 0)
        return np.ctypeslib.as_array((C.c_int * B).from_address(C.addressof(p.contents))).copy()

    def labels(self, slot):
        """-> device pointer (int) of the slot's int32 [B] labels (a resident stager): labels[idx], -1 where idx is -1; valid behind
        wait(slot) and until release(slot)"""
        p = C.POINTER(C.c_int)()
        check(self.lib.cnn_batch_stager_labels(self.h, int(slot), C.byref(p)), "cnn_batch_stager_labels")
        return C.cast(p, C.c_void_p).value

    def set_normalize(self, mean, std, clamp=True):
        """later submits write (clamp(u) - mean) / std per channel, clamp(u) = u limited to [0, 1] when clamp (a photo stager;
        default: mean 0, std 1, clamp off)"""
        m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
        check(self.lib.cnn_batch_stager_set_normalize(self.h, m, s, int(bool(clamp))), "cnn_batch_stager_set_normalize")

    def acquire(self):
        """-> (numpy view of the pinned slot to fill -- float32, or uint8 for a u8 stager --, slot index); blocks until the slot is free"""
        import numpy as np

        host, slot = C.c_void_p(), C.c_int()
        check(self.lib.cnn_batch_stager_acquire(self.h, C.byref(host), C.byref(slot)), "cnn_batch_stager_acquire")
        if self.resident is not None:  # (no pinned image block: the images are in the dataset)
            return None, slot.value
        if self.u8:
            return np.ctypeslib.as_array((C.c_ubyte * self.bytes).from_address(host.value)), slot.value
        buf = (C.c_float * (self.bytes // 4)).from_address(host.value)
        return np.ctypeslib.as_array(buf), slot.value

    def submit(self, slot):
        """enqueue the upload; -> device pointer (int) of the slot's device buffer"""
        dev = C.c_void_p()
        check(self.lib.cnn_batch_stager_submit(self.h, slot, C.byref(dev)), "cnn_batch_stager_submit")
        return dev.value

    def wait(self, slot):
        check(self.lib.cnn_batch_stager_wait(self.h, slot, _stream()), "cnn_batch_stager_wait")

    def release(self, slot):
        check(self.lib.cnn_batch_stager_release(self.h, slot, _stream()), "cnn_batch_stager_release")

    def close(self):
        if self.h:
            self.lib.cnn_batch_stager_destroy(self.h)
            self.h = None


def _dropout_counts(p, channels):
    """selected_num = int(p * C) and keep = 1 - p in the reference's FLOAT arithmetic (dropout.cpp:16: data_type p times int):
    Python doubles give a different count for some p (0.29 * 100 -> 28 here, 29 in the reference)"""
    import numpy as np

    return int(np.float32(p) * np.float32(channels)), float(np.float32(1) - np.float32(p))


def dropout_forward(x, p, training=True, y=None):
    """Dropout::forward (dropout.cpp:7-55): channels 0 .. int(p*C)-1 zeroed in training, x * (1-p) otherwise"""
    import torch

    _need_gpu(x, y)
    B, Cc, H, W = x.shape
    if y is None:
        y = torch.empty_like(x)
    dropped, keep = _dropout_counts(p, Cc)
    check(load().cnn_dropout_forward(_ptr(x), _ptr(y), B, Cc, H, W, dropped, 1 if training else 0, keep, _stream()), "cnn_dropout_forward")
    return y


def dropout_backward(dy, p):
    """in place on dy (dropout.cpp:57-69)"""
    _need_gpu(dy)
    B, Cc, H, W = dy.shape
    check(load().cnn_dropout_backward(_ptr(dy), B, Cc, H, W, _dropout_counts(p, Cc)[0], _stream()), "cnn_dropout_backward")
    return dy
