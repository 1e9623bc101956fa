"""fftconv_amd -- Python mirror of the reference's `Convolution` trait over the
MI355X C ABI (include/fftconv.h, libfftconv_amd.so).

    FFTConvolver.init(response, max_block_size, max_response_length)   src/fft_convolver.rs:105
    .update(response) / .reset() / .process(input[, out_len]) / .clone()
    TwoStageFFTConvolver.init(...)                                      src/fft_convolver.rs:340
    CrossfadeConvolver.init(...) / CrossfadeConvolver.new(conv, ...)    src/crossfade_convolver.rs:19-49

Every object is a batch of `channels` independent convolvers on one GPU
(channels=1 is exactly one reference instance).  Host arrays are
[channels][samples] (1-D for a single channel).  `process_device` takes raw
device pointers (e.g. torch tensors' data_ptr()) and a HIP stream and is
asynchronous.  Stream 0 is HIP's null stream -- torch's default stream --
as everywhere in HIP: work enqueued there after a call sees its results.

A reference panic surfaces as `ConvolutionPanic`; HIP failures as
`DeviceError`.  There is no CPU fallback: importing works anywhere, but
creating a convolver needs the HIP library and a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FFTCONV_AMD_LIB: another build of the same library (A/B of kernel revisions)
LIB_PATH = os.environ.get("FFTCONV_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "libfftconv_amd.so")

FFTCONV_OK = 0
FFTCONV_E_INVALID = -1
FFTCONV_E_UNIMPLEMENTED = -2
FFTCONV_E_UNSUPPORTED = -3
FFTCONV_E_DEVICE = -4
FFTCONV_E_NOMEM = -5

# every symbol include/fftconv.h declares: name -> (restype, argtypes)
_vp, _sz, _fp, _i = C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.c_int
_u32p = C.POINTER(C.c_uint32)
SIGNATURES = {
    "fftconv_abi_version": (_i, []),
    "fftconv_last_error": (C.c_char_p, []),
    "fftconv_device_count": (_i, []),
    "fftconv_complex_size": (_sz, [_sz]),
    "fftconv_compute_tail_block_size": (_sz, [_sz, _sz]),
    "fftconv_fft_forward": (_i, [_i, _sz, _sz, _vp, _sz, _vp, _sz, _vp]),
    "fftconv_fft_inverse": (_i, [_i, _sz, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    "fftconv_fft_forward_host": (_i, [_i, _sz, _sz, _fp, _fp]),
    "fftconv_fft_inverse_host": (_i, [_i, _sz, _sz, _fp, _fp, C.POINTER(_i)]),
    "fftconv_set_kernel_variant": (_i, [_i]),
    "fftconv_get_kernel_variant": (_i, []),
    "fftconv_set_pipeline_lag": (_i, [_i]),
    "fftconv_get_pipeline_lag": (_i, []),
    "fftconv_set_host_stage_limit": (_i, [_sz]),
    "fftconv_get_host_stage_limit": (_sz, []),
    "fftconv_uniform_init": (_vp, [_fp, _sz, _sz, _sz]),
    "fftconv_uniform_init_batch": (_vp, [_i, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_uniform_update": (_i, [_vp, _fp, _sz]),
    "fftconv_uniform_update_batch": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_uniform_update_channel": (_i, [_vp, _sz, _fp, _sz]),
    "fftconv_uniform_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_uniform_reset": (_i, [_vp]),
    "fftconv_uniform_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_uniform_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_uniform_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_uniform_clone": (_vp, [_vp]),
    "fftconv_uniform_destroy": (None, [_vp]),
    "fftconv_uniform_synchronize": (_i, [_vp]),
    "fftconv_uniform_channels": (_sz, [_vp]),
    "fftconv_uniform_lookahead_parts": (_i, [_vp]),
    "fftconv_uniform_far_windows": (_i, [_vp]),
    "fftconv_uniform_lookahead_probe": (_i, [_vp]),
    "fftconv_uniform_block_size": (_sz, [_vp]),
    "fftconv_uniform_seg_count": (_sz, [_vp]),
    "fftconv_uniform_ir_spectrum": (_i, [_vp, _sz, _sz, _fp]),
    "fftconv_uniform_channel_state": (_i, [_vp, _sz, C.POINTER(_sz)]),
    "fftconv_twostage_init": (_vp, [_fp, _sz, _sz, _sz]),
    "fftconv_twostage_init_batch": (_vp, [_i, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_twostage_update": (_i, [_vp, _fp, _sz]),
    "fftconv_twostage_reset": (_i, [_vp]),
    "fftconv_twostage_process": (_i, [_vp, _fp, _fp, _sz]),
    "fftconv_twostage_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_twostage_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_twostage_clone": (_vp, [_vp]),
    "fftconv_twostage_destroy": (None, [_vp]),
    "fftconv_twostage_synchronize": (_i, [_vp]),
    "fftconv_twostage_tail_block_size": (_sz, [_vp]),
    "fftconv_crossfade_init": (_vp, [_fp, _sz, _sz, _sz]),
    "fftconv_crossfade_init_batch": (_vp, [_i, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_crossfade_new": (_vp, [_vp, _sz, _sz, _sz]),
    "fftconv_crossfade_init_twostage": (_vp, [_fp, _sz, _sz, _sz]),
    "fftconv_crossfade_init_twostage_batch": (_vp, [_i, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_crossfade_new_twostage": (_vp, [_vp, _sz, _sz, _sz]),
    "fftconv_crossfade_update": (_i, [_vp, _fp, _sz]),
    "fftconv_crossfade_update_batch": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_crossfade_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_crossfade_reset": (_i, [_vp]),
    "fftconv_crossfade_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_crossfade_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_crossfade_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_crossfade_is_crossfading": (_i, [_vp]),
    "fftconv_crossfade_clone": (_vp, [_vp]),
    "fftconv_crossfade_destroy": (None, [_vp]),
    "fftconv_crossfade_synchronize": (_i, [_vp]),
    "fftconv_matrix_init": (_vp, [_i, _sz, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_reset": (_i, [_vp]),
    "fftconv_matrix_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_clone": (_vp, [_vp]),
    "fftconv_matrix_destroy": (None, [_vp]),
    "fftconv_matrix_synchronize": (_i, [_vp]),
    "fftconv_matrix_inputs": (_sz, [_vp]),
    "fftconv_matrix_outputs": (_sz, [_vp]),
    "fftconv_matrix_block_size": (_sz, [_vp]),
    "fftconv_matrix_seg_count": (_sz, [_vp]),
    "fftconv_matrix_mac_parts": (_i, [_vp]),
    "fftconv_matrix_state": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_lookahead_init": (_vp, [_i, _sz, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_lookahead_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_lookahead_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_reset": (_i, [_vp]),
    "fftconv_matrix_lookahead_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_lookahead_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_clone": (_vp, [_vp]),
    "fftconv_matrix_lookahead_destroy": (None, [_vp]),
    "fftconv_matrix_lookahead_synchronize": (_i, [_vp]),
    "fftconv_matrix_lookahead_inputs": (_sz, [_vp]),
    "fftconv_matrix_lookahead_outputs": (_sz, [_vp]),
    "fftconv_matrix_lookahead_block_size": (_sz, [_vp]),
    "fftconv_matrix_lookahead_seg_count": (_sz, [_vp]),
    "fftconv_matrix_lookahead_state": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_lookahead_period": (_i, []),
    "fftconv_matrix_lookahead_near_parts": (_i, [_vp]),
    "fftconv_matrix_lookahead_far_parts": (_i, [_vp]),
    "fftconv_matrix_lookahead_set_windows": (_i, [_vp, _i]),
    "fftconv_matrix_lookahead_anchors": (_i, [_vp]),
    "fftconv_matrix_sparse_init": (_vp, [_i, _sz, _sz, _sz, _u32p, _u32p, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_sparse_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_reset": (_i, [_vp]),
    "fftconv_matrix_sparse_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_sparse_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_clone": (_vp, [_vp]),
    "fftconv_matrix_sparse_destroy": (None, [_vp]),
    "fftconv_matrix_sparse_synchronize": (_i, [_vp]),
    "fftconv_matrix_sparse_inputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_outputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_pairs": (_sz, [_vp]),
    "fftconv_matrix_sparse_block_size": (_sz, [_vp]),
    "fftconv_matrix_sparse_seg_count": (_sz, [_vp]),
    "fftconv_matrix_sparse_output_parts": (_i, [_vp, _sz]),
    "fftconv_matrix_sparse_state": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_sparse_lookahead_init": (_vp, [_i, _sz, _sz, _sz, _u32p, _u32p, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_sparse_lookahead_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_lookahead_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_lookahead_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_lookahead_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_lookahead_reset": (_i, [_vp]),
    "fftconv_matrix_sparse_lookahead_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_sparse_lookahead_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_lookahead_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_lookahead_clone": (_vp, [_vp]),
    "fftconv_matrix_sparse_lookahead_destroy": (None, [_vp]),
    "fftconv_matrix_sparse_lookahead_synchronize": (_i, [_vp]),
    "fftconv_matrix_sparse_lookahead_inputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_lookahead_outputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_lookahead_pairs": (_sz, [_vp]),
    "fftconv_matrix_sparse_lookahead_block_size": (_sz, [_vp]),
    "fftconv_matrix_sparse_lookahead_seg_count": (_sz, [_vp]),
    "fftconv_matrix_sparse_lookahead_state": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_sparse_lookahead_near_parts": (_i, [_vp, _sz]),
    "fftconv_matrix_sparse_lookahead_far_parts": (_i, [_vp, _sz]),
    "fftconv_matrix_sparse_lookahead_set_windows": (_i, [_vp, _i]),
    "fftconv_matrix_sparse_lookahead_anchors": (_i, [_vp]),
    "fftconv_matrix_crossfade_init": (_vp, [_i, _sz, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_crossfade_new": (_vp, [_vp, _sz, _sz, _sz]),
    "fftconv_matrix_crossfade_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_crossfade_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_crossfade_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_crossfade_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_crossfade_diff_pairs": (_sz, [_vp]),
    "fftconv_matrix_crossfade_last_patch": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_crossfade_reset": (_i, [_vp]),
    "fftconv_matrix_crossfade_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_crossfade_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_crossfade_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_crossfade_is_crossfading": (_i, [_vp]),
    "fftconv_matrix_crossfade_clone": (_vp, [_vp]),
    "fftconv_matrix_crossfade_destroy": (None, [_vp]),
    "fftconv_matrix_crossfade_synchronize": (_i, [_vp]),
    "fftconv_matrix_crossfade_inputs": (_sz, [_vp]),
    "fftconv_matrix_crossfade_outputs": (_sz, [_vp]),
    "fftconv_matrix_crossfade_set_fused": (_i, [_vp, _i]),
    "fftconv_matrix_crossfade_path": (_i, [_vp]),
    "fftconv_matrix_sparse_crossfade_init": (_vp, [_i, _sz, _sz, _sz, _u32p, _u32p, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_sparse_crossfade_new": (_vp, [_vp, _sz, _sz, _sz]),
    "fftconv_matrix_sparse_crossfade_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_crossfade_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_crossfade_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_crossfade_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_crossfade_diff_pairs": (_sz, [_vp]),
    "fftconv_matrix_sparse_crossfade_last_patch": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_sparse_crossfade_reset": (_i, [_vp]),
    "fftconv_matrix_sparse_crossfade_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_sparse_crossfade_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_crossfade_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_crossfade_is_crossfading": (_i, [_vp]),
    "fftconv_matrix_sparse_crossfade_clone": (_vp, [_vp]),
    "fftconv_matrix_sparse_crossfade_destroy": (None, [_vp]),
    "fftconv_matrix_sparse_crossfade_synchronize": (_i, [_vp]),
    "fftconv_matrix_sparse_crossfade_inputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_crossfade_outputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_crossfade_pairs": (_sz, [_vp]),
    "fftconv_matrix_sparse_crossfade_set_fused": (_i, [_vp, _i]),
    "fftconv_matrix_sparse_crossfade_path": (_i, [_vp]),
    "fftconv_matrix_lookahead_crossfade_init": (_vp, [_i, _sz, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_lookahead_crossfade_new": (_vp, [_vp, _sz, _sz, _sz]),
    "fftconv_matrix_lookahead_crossfade_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_lookahead_crossfade_update_device": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_crossfade_update_pairs": (_i, [_vp, _sz, _u32p, _u32p, _fp, _sz, _sz]),
    "fftconv_matrix_lookahead_crossfade_update_pairs_device": (_i, [_vp, _sz, _u32p, _u32p, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_crossfade_diff_pairs": (_sz, [_vp]),
    "fftconv_matrix_lookahead_crossfade_last_patch": (_i, [_vp, C.POINTER(_sz)]),
    "fftconv_matrix_lookahead_crossfade_reset": (_i, [_vp]),
    "fftconv_matrix_lookahead_crossfade_process": (_i, [_vp, _fp, _sz, _fp, _sz]),
    "fftconv_matrix_lookahead_crossfade_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_crossfade_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_lookahead_crossfade_is_crossfading": (_i, [_vp]),
    "fftconv_matrix_lookahead_crossfade_clone": (_vp, [_vp]),
    "fftconv_matrix_lookahead_crossfade_destroy": (None, [_vp]),
    "fftconv_matrix_lookahead_crossfade_synchronize": (_i, [_vp]),
    "fftconv_matrix_lookahead_crossfade_inputs": (_sz, [_vp]),
    "fftconv_matrix_lookahead_crossfade_outputs": (_sz, [_vp]),
    "fftconv_matrix_lookahead_crossfade_set_fused": (_i, [_vp, _i]),
    "fftconv_matrix_lookahead_crossfade_path": (_i, [_vp]),
    "fftconv_matrix_lookahead_crossfade_set_windows": (_i, [_vp, _i]),
    "fftconv_matrix_lookahead_crossfade_anchors": (_i, [_vp, _i]),
    "fftconv_matrix_twostage_init": (_vp, [_i, _sz, _sz, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_twostage_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_twostage_reset": (_i, [_vp]),
    "fftconv_matrix_twostage_process": (_i, [_vp, _fp, _fp, _sz]),
    "fftconv_matrix_twostage_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_twostage_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_twostage_clone": (_vp, [_vp]),
    "fftconv_matrix_twostage_destroy": (None, [_vp]),
    "fftconv_matrix_twostage_synchronize": (_i, [_vp]),
    "fftconv_matrix_twostage_inputs": (_sz, [_vp]),
    "fftconv_matrix_twostage_outputs": (_sz, [_vp]),
    "fftconv_matrix_twostage_tail_block_size": (_sz, [_vp]),
    "fftconv_matrix_twostage_set_fused": (_i, [_vp, _i]),
    "fftconv_matrix_twostage_path": (_i, [_vp, _sz]),
    "fftconv_matrix_sparse_twostage_init": (_vp, [_i, _sz, _sz, _sz, _u32p, _u32p, _fp, _sz, _sz, _sz, _sz]),
    "fftconv_matrix_sparse_twostage_update": (_i, [_vp, _fp, _sz, _sz]),
    "fftconv_matrix_sparse_twostage_reset": (_i, [_vp]),
    "fftconv_matrix_sparse_twostage_process": (_i, [_vp, _fp, _fp, _sz]),
    "fftconv_matrix_sparse_twostage_process_device": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_twostage_process_device_steps": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp]),
    "fftconv_matrix_sparse_twostage_clone": (_vp, [_vp]),
    "fftconv_matrix_sparse_twostage_destroy": (None, [_vp]),
    "fftconv_matrix_sparse_twostage_synchronize": (_i, [_vp]),
    "fftconv_matrix_sparse_twostage_inputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_twostage_outputs": (_sz, [_vp]),
    "fftconv_matrix_sparse_twostage_pairs": (_sz, [_vp]),
    "fftconv_matrix_sparse_twostage_tail_block_size": (_sz, [_vp]),
    "fftconv_matrix_sparse_twostage_set_fused": (_i, [_vp, _i]),
    "fftconv_matrix_sparse_twostage_path": (_i, [_vp, _sz]),
}


class ConvolutionPanic(RuntimeError):
    """Where the reference panics (assert!/panic!/slice bounds)."""


class NotImplementedInReference(ConvolutionPanic):
    """Where the reference has todo!()."""


class DeviceError(RuntimeError):
    """HIP runtime failure or no usable device."""


_lib = None


def lib():
    """Load libfftconv_amd.so (fails loudly if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DeviceError(f"{LIB_PATH} not built -- run __graft_entry__.build() or make -C fft-convolution_amd")
        # One HIP runtime per process: torch's libc10_hip loads its bundled
        # libamdhip64 by the unversioned name, while this library NEEDs
        # libamdhip64.so.7.  Loading torch first makes the dynamic linker bind
        # our NEEDED entry to torch's copy (same SONAME), so device pointers and
        # hipStream_t handles from torch are valid here; loading us first would
        # put two HIP/HSA runtimes in the process and torch would see no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.fftconv_abi_version() != 1:
            raise DeviceError("ABI version mismatch")
        _lib = L
    return _lib


def last_error() -> str:
    return lib().fftconv_last_error().decode()


def _check(rc: int):
    if rc == FFTCONV_OK:
        return
    msg = last_error()
    if rc == FFTCONV_E_INVALID:
        raise ConvolutionPanic(msg)
    if rc == FFTCONV_E_UNIMPLEMENTED:
        raise NotImplementedInReference(msg)
    raise DeviceError(f"status {rc}: {msg}")


def _handle(h):
    if not h:
        msg = last_error()
        if "max_response_length" in msg or "longer" in msg or "at least one input" in msg or "pair" in msg:
            raise ConvolutionPanic(msg)
        raise DeviceError(msg or "handle creation failed")
    return h


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _p(a: np.ndarray):
    return a.ctypes.data_as(_fp)


def complex_size(n: int) -> int:
    return int(lib().fftconv_complex_size(n))


def compute_tail_block_size(head_len: int, response_len: int) -> int:
    return int(lib().fftconv_compute_tail_block_size(head_len, response_len))


def set_kernel_variant(v: int):
    _check(lib().fftconv_set_kernel_variant(v))


def get_kernel_variant() -> int:
    return int(lib().fftconv_get_kernel_variant())


def set_host_stage_limit(nbytes: int):
    """Cap (bytes, 0 = none) on the pinned host staging a handle reserves at
    creation for update(); larger updates stream through it in chunks."""
    _check(lib().fftconv_set_host_stage_limit(nbytes))


def get_host_stage_limit() -> int:
    return int(lib().fftconv_get_host_stage_limit())


def set_pipeline_lag(rows: int):
    """FDL rows the pipelined step leaves to its stream waves (-1 = automatic)."""
    _check(lib().fftconv_set_pipeline_lag(rows))


def get_pipeline_lag() -> int:
    return int(lib().fftconv_get_pipeline_lag())


def device_count() -> int:
    return int(lib().fftconv_device_count())


class Fft:
    """Fft (src/fft_convolver.rs:7-50) of length n on the GPU: realfft's
    R2C / C2R (forward unnormalised, inverse / n), batched over rows.  Any n in
    1..2^21 (Bluestein for a length that is not a power of two), or a power of
    two up to 2^23."""

    def __init__(self, length: int, device: int = 0):
        self.n = int(length)
        self.device = device

    def forward(self, x) -> np.ndarray:
        """[rows][n] (or [n]) reals -> complex64 [rows][n/2 + 1]."""
        x = _f32(x)
        flat = x.ndim == 1
        x2 = x.reshape(-1, self.n)
        out = np.zeros((x2.shape[0], 2 * (self.n // 2 + 1)), np.float32)
        _check(lib().fftconv_fft_forward_host(self.device, self.n, x2.shape[0], _p(x2), _p(out)))
        out = out.view(np.complex64)
        return out[0] if flat else out

    def inverse(self, spec):
        """complex [rows][n/2 + 1] -> ([rows][n] reals / n, per-row
        FftError::InputValues flags (non-zero DC / Nyquist imaginary part))."""
        z = np.ascontiguousarray(np.asarray(spec, np.complex64))
        flat = z.ndim == 1
        z2 = z.reshape(-1, self.n // 2 + 1)
        zf = np.ascontiguousarray(z2).view(np.float32)
        out = np.zeros((z2.shape[0], self.n), np.float32)
        st = np.zeros(z2.shape[0], np.int32)
        _check(lib().fftconv_fft_inverse_host(self.device, self.n, z2.shape[0], _p(zf), _p(out),
                                              st.ctypes.data_as(C.POINTER(_i))))
        return (out[0], bool(st[0])) if flat else (out, st.astype(bool))

    def forward_device(self, d_in: int, in_stride: int, d_out: int, out_stride: int, rows: int, stream: int = 0):
        _check(lib().fftconv_fft_forward(self.device, self.n, rows, C.c_void_p(d_in), in_stride, C.c_void_p(d_out),
                                         out_stride, C.c_void_p(stream) if stream else None))

    def inverse_device(self, d_in: int, in_stride: int, d_out: int, out_stride: int, rows: int, d_status: int = 0,
                       stream: int = 0):
        _check(lib().fftconv_fft_inverse(self.device, self.n, rows, C.c_void_p(d_in), in_stride, C.c_void_p(d_out),
                                         out_stride, C.c_void_p(d_status) if d_status else None,
                                         C.c_void_p(stream) if stream else None))


def _responses(responses, channels):
    r = _f32(responses)
    if r.ndim == 1:
        return r, r.size, 0
    if r.shape[0] != channels:
        raise ValueError("responses must be [channels][len]")
    return r, r.shape[1], r.shape[1]


class _Base:
    _prefix = ""

    def __init__(self, h, channels: int):
        self._h = h
        self.channels = channels

    def _fn(self, name):
        return getattr(lib(), f"fftconv_{self._prefix}_{name}")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            getattr(_lib, f"fftconv_{self._prefix}_destroy")(h)
            self._h = None

    def _shape_in(self, x):
        x = _f32(x)
        if self.channels == 1 and x.ndim == 1:
            return x, x.size, True
        if x.ndim != 2 or x.shape[0] != self.channels:
            raise ValueError(f"input must be [{self.channels}][n]")
        return x, x.shape[1], False

    def synchronize(self):
        _check(self._fn("synchronize")(self._h))

    def process_device(self, d_in: int, in_stride: int, d_out: int, out_stride: int, n: int, stream: int = 0):
        """process() on device buffers, enqueued on `stream` (0 = HIP's null
        stream, torch's default stream; fftconv.h "Streams"): ordered after the
        handle's previous work, and work enqueued on `stream` afterwards sees
        the output."""
        _check(self._fn("process_device")(self._h, C.c_void_p(d_in), in_stride, C.c_void_p(d_out), out_stride, n,
                                          C.c_void_p(stream) if stream else None))

    def process_device_steps(self, d_in: int, in_stride: int, in_step: int, d_out: int, out_stride: int,
                             out_step: int, n: int, steps: int, stream: int = 0):
        """`steps` consecutive process_device calls (offsets in floats); stream 0 =
        HIP's null stream, as process_device."""
        _check(self._fn("process_device_steps")(self._h, C.c_void_p(d_in), in_stride, in_step, C.c_void_p(d_out),
                                                out_stride, out_step, n, steps,
                                                C.c_void_p(stream) if stream else None))

    def __copy__(self):
        return self.clone()


class FFTConvolver(_Base):
    """FFTConvolver, src/fft_convolver.rs:86-307 (a batch of `channels`)."""

    _prefix = "uniform"

    @classmethod
    def init(cls, response, max_block_size: int, max_response_length: int, *, channels: int = 1, device: int = 0):
        r, n, stride = _responses(response, channels)
        h = lib().fftconv_uniform_init_batch(device, channels, _p(r), n, stride, max_block_size, max_response_length)
        return cls(_handle(h), channels)

    def update(self, response):
        r = _f32(response)
        if r.ndim == 2:
            _check(lib().fftconv_uniform_update_batch(self._h, _p(r), r.shape[1], r.shape[1]))
        else:
            _check(lib().fftconv_uniform_update(self._h, _p(r), r.size))

    def update_device(self, d_responses: int, response_len: int, stride: int = 0, stream: int = 0):
        """update() from device memory (channel c at d_responses + 4*c*stride;
        stride 0 = same response for all channels), stream-ordered."""
        _check(self._fn("update_device")(self._h, C.c_void_p(d_responses), response_len, stride,
                                         C.c_void_p(stream) if stream else None))

    def update_channel(self, channel: int, response):
        r = _f32(response)
        _check(lib().fftconv_uniform_update_channel(self._h, channel, _p(r), r.size))

    def reset(self):
        _check(lib().fftconv_uniform_reset(self._h))

    def process(self, inp, out_len: int | None = None) -> np.ndarray:
        x, n_in, flat = self._shape_in(inp)
        n = n_in if out_len is None else out_len
        y = np.zeros((self.channels, n), np.float32)
        _check(lib().fftconv_uniform_process(self._h, _p(x), n_in, _p(y), n))
        return y[0] if flat else y

    def clone(self):
        return FFTConvolver(_handle(lib().fftconv_uniform_clone(self._h)), self.channels)

    @property
    def block_size(self) -> int:
        return int(lib().fftconv_uniform_block_size(self._h))

    @property
    def seg_count(self) -> int:
        return int(lib().fftconv_uniform_seg_count(self._h))

    def lookahead_parts(self) -> int:
        """Anchor workgroups per channel of the lookahead step (0 = not used)."""
        return int(lib().fftconv_uniform_lookahead_parts(self._h))

    def far_windows(self) -> int:
        """Window rows per channel of the far-row windows (B >= 1024; 0 = not used)."""
        return int(lib().fftconv_uniform_far_windows(self._h))

    def lookahead_probe(self) -> int:
        """(tests) live state words the FFTCONV_LA_PROBE launches' anchors found
        already rewritten by their own launch's steps (the anchors compute from
        launch-start copies); -1 when the probe is off."""
        return int(lib().fftconv_uniform_lookahead_probe(self._h))

    def ir_spectrum(self, channel: int, segment: int) -> np.ndarray:
        """segments_ir[segment] of a channel: complex64[B + 1]."""
        out = np.zeros(2 * (self.block_size + 1), np.float32)
        _check(lib().fftconv_uniform_ir_spectrum(self._h, channel, segment, _p(out)))
        return out.view(np.complex64)

    def channel_state(self, channel: int = 0):
        """(current, active_seg_count, input_buffer_fill)."""
        out = (C.c_size_t * 3)()
        _check(lib().fftconv_uniform_channel_state(self._h, channel, out))
        return tuple(int(v) for v in out)


class TwoStageFFTConvolver(_Base):
    """TwoStageFFTConvolver, src/fft_convolver.rs:323-526."""

    _prefix = "twostage"

    @classmethod
    def init(cls, response, max_block_size: int, max_response_length: int, *, channels: int = 1, device: int = 0):
        r, n, stride = _responses(response, channels)
        h = lib().fftconv_twostage_init_batch(device, channels, _p(r), n, stride, max_block_size, max_response_length)
        return cls(_handle(h), channels)

    def update(self, response):
        r = _f32(response)
        _check(lib().fftconv_twostage_update(self._h, _p(r), r.size))

    def reset(self):
        _check(lib().fftconv_twostage_reset(self._h))

    def process(self, inp) -> np.ndarray:
        x, n, flat = self._shape_in(inp)
        y = np.zeros((self.channels, n), np.float32)
        _check(lib().fftconv_twostage_process(self._h, _p(x), _p(y), n))
        return y[0] if flat else y

    def clone(self):
        return TwoStageFFTConvolver(_handle(lib().fftconv_twostage_clone(self._h)), self.channels)

    @property
    def tail_block_size(self) -> int:
        return int(lib().fftconv_twostage_tail_block_size(self._h))


class CrossfadeConvolver(_Base):
    """CrossfadeConvolver<T>, src/crossfade_convolver.rs:3-105, for T =
    FFTConvolver (the default) or TwoStageFFTConvolver (`inner=`, or `new`
    with a TwoStageFFTConvolver).  Over a TwoStageFFTConvolver every update()
    reaches its todo!() (src/fft_convolver.rs:408-410) and raises
    NotImplementedInReference, as the reference panics."""

    _prefix = "crossfade"

    def __init__(self, h, channels: int, max_buffer_size: int, inner: type = None):
        super().__init__(h, channels)
        self.max_buffer_size = max_buffer_size
        self.inner = inner or FFTConvolver

    @classmethod
    def init(cls, response, max_block_size: int, max_response_length: int, *, channels: int = 1, device: int = 0,
             inner: type = None):
        """Convolution::init (:46-49); `inner` is the T of CrossfadeConvolver<T>."""
        r, n, stride = _responses(response, channels)
        fn = lib().fftconv_crossfade_init_twostage_batch if inner is TwoStageFFTConvolver \
            else lib().fftconv_crossfade_init_batch
        if inner not in (None, FFTConvolver, TwoStageFFTConvolver):
            raise TypeError("inner must be FFTConvolver or TwoStageFFTConvolver")
        h = fn(device, channels, _p(r), n, stride, max_block_size, max_response_length)
        return cls(_handle(h), channels, max_block_size, inner)

    @classmethod
    def new(cls, convolver, max_response_length: int, max_buffer_size: int, crossfade_samples: int):
        """CrossfadeConvolver::new (:19-43); the convolver is cloned."""
        if isinstance(convolver, TwoStageFFTConvolver):
            fn = lib().fftconv_crossfade_new_twostage
        elif isinstance(convolver, FFTConvolver):
            fn = lib().fftconv_crossfade_new
        else:
            raise TypeError("convolver must be an FFTConvolver or a TwoStageFFTConvolver")
        h = fn(convolver._h, max_response_length, max_buffer_size, crossfade_samples)
        return cls(_handle(h), convolver.channels, max_buffer_size, type(convolver))

    def update(self, response):
        r = _f32(response)
        if r.ndim == 2:
            _check(lib().fftconv_crossfade_update_batch(self._h, _p(r), r.shape[1], r.shape[1]))
        else:
            _check(lib().fftconv_crossfade_update(self._h, _p(r), r.size))

    def update_device(self, d_responses: int, response_len: int, stride: int = 0, stream: int = 0):
        """update() from device memory (channel c at d_responses + 4*c*stride;
        stride 0 = same response for all channels), stream-ordered."""
        _check(self._fn("update_device")(self._h, C.c_void_p(d_responses), response_len, stride,
                                         C.c_void_p(stream) if stream else None))

    def reset(self):
        _check(lib().fftconv_crossfade_reset(self._h))

    def process(self, inp, out_len: int | None = None) -> np.ndarray:
        x, n_in, flat = self._shape_in(inp)
        n = n_in if out_len is None else out_len
        y = np.zeros((self.channels, n), np.float32)
        _check(lib().fftconv_crossfade_process(self._h, _p(x), n_in, _p(y), n))
        return y[0] if flat else y

    def is_crossfading(self) -> bool:
        return bool(lib().fftconv_crossfade_is_crossfading(self._h))

    def clone(self):
        return CrossfadeConvolver(_handle(lib().fftconv_crossfade_clone(self._h)), self.channels,
                                  self.max_buffer_size, self.inner)


def _pair_arrays(pairs):
    """(output, input) tuples -> the two uint32 arrays of the C ABI."""
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    if pr.size and (pr.min() < 0 or pr.max() >= 1 << 32):
        raise ValueError("pair indices must fit 32 unsigned bits")
    return np.ascontiguousarray(pr[:, 0].astype(np.uint32)), np.ascontiguousarray(pr[:, 1].astype(np.uint32))


class _UpdatePairs:
    """update_pairs of the dense, sparse and crossfaded matrices (fftconv.h): update(R'),
    R' = the responses the handle holds with the listed pairs replaced."""

    def update_pairs(self, pairs, responses):
        """pairs: (output, input) tuples, strictly ascending; responses[n][len]
        is the new response of pairs[n], zero-padded to the held set's length."""
        po, pi = _pair_arrays(pairs)
        r = _f32(responses)
        if r.ndim != 2 or r.shape[0] != len(po):
            if len(po) == 0 and r.size == 0:
                r = np.zeros((0, 0), np.float32)
            else:
                raise ValueError("responses must be [pairs][len]")
        _check(self._fn("update_pairs")(self._h, len(po), po.ctypes.data_as(_u32p), pi.ctypes.data_as(_u32p), _p(r),
                                        r.shape[1], r.shape[1]))

    def update_pairs_device(self, pairs, d_responses: int, response_len: int, stride: int = 0, stream: int = 0):
        """update_pairs() from device memory (row n at d_responses + 4 * n *
        stride belongs to pairs[n]; the pair list is host data), stream-ordered."""
        po, pi = _pair_arrays(pairs)
        _check(self._fn("update_pairs_device")(self._h, len(po), po.ctypes.data_as(_u32p), pi.ctypes.data_as(_u32p),
                                               C.c_void_p(d_responses), response_len, stride,
                                               C.c_void_p(stream) if stream else None))


def _dense_responses(responses, inputs=None, outputs=None):
    r = _f32(responses)
    if r.ndim != 3 or (inputs is not None and r.shape[:2] != (outputs, inputs)):
        raise ValueError("responses must be [outputs][inputs][len]")
    return r


def _listed_responses(responses, pairs: int):
    r = _f32(responses)
    if r.ndim != 2 or r.shape[0] != pairs:
        raise ValueError("responses must be [pairs][len]")
    return r


class _MatrixBase(_Base):
    """What the matrix classes share: inputs x outputs, a whole update, reset,
    process and clone, each through the class's C prefix.  A
    dense matrix takes its responses as [O][I][len] (pair o * inputs + i); a
    class with a listed pair set (`pairs` is its size) as [pairs][len], in list
    order."""

    pairs = None

    def __init__(self, h, inputs: int, outputs: int):
        super().__init__(h, inputs)
        self.inputs = inputs
        self.outputs = outputs

    @classmethod
    def _cfn(cls, name):
        return getattr(lib(), f"fftconv_{cls._prefix}_{name}")

    def _set_pair_list(self, pair_list, pairs: int | None = None):
        self._pair_list = [(int(o), int(i)) for o, i in pair_list] if pair_list is not None else None
        self.pairs = len(self._pair_list) if pairs is None else pairs

    def _clone_args(self):
        """The constructor's arguments after the handle."""
        return self.inputs, self.outputs

    def update(self, responses):
        """update() of every pair with responses[O][I][len], or [pairs][len]
        over a listed pair set (whole matrix).  A crossfaded matrix (:51-64)
        starts the fade, or stores the responses until the fade under way has
        ended."""
        if self.pairs is None:
            r = _dense_responses(responses, self.inputs, self.outputs)
        else:
            r = _listed_responses(responses, self.pairs)
        _check(self._fn("update")(self._h, _p(r), r.shape[-1], r.shape[-1]))

    def update_device(self, d_responses: int, response_len: int, stride: int = 0, stream: int = 0):
        """update() from device memory (pair p -- o * inputs + i, or the
        position in the pair list -- at d_responses + 4 * p * stride; stride 0 =
        one response for every pair), stream-ordered."""
        _check(self._fn("update_device")(self._h, C.c_void_p(d_responses), response_len, stride,
                                         C.c_void_p(stream) if stream else None))

    def reset(self):
        _check(self._fn("reset")(self._h))

    def process(self, inp, out_len: int | None = None) -> np.ndarray:
        """x[inputs][n] -> y[outputs][out_len or n].  (A crossfaded matrix: n >=
        max_buffer_size, and the state advances by max_buffer_size samples
        whatever out_len is.)"""
        x = _f32(inp)
        if x.ndim != 2 or x.shape[0] != self.inputs:
            raise ValueError(f"input must be [{self.inputs}][n]")
        n_in = x.shape[1]
        n = n_in if out_len is None else out_len
        y = np.zeros((self.outputs, n), np.float32)
        _check(self._fn("process")(self._h, _p(x), n_in, _p(y), n))
        return y

    def clone(self):
        return type(self)(_handle(self._fn("clone")(self._h)), *self._clone_args())


class _MatrixGeometry(_MatrixBase):
    """block_size, seg_count and state() of the matrices that are one convolver
    (the C ABI has none for a crossfaded matrix)."""

    @property
    def block_size(self) -> int:
        return int(self._fn("block_size")(self._h))

    @property
    def seg_count(self) -> int:
        return int(self._fn("seg_count")(self._h))

    def state(self):
        """(current, active_seg_count, input_buffer_fill) of the whole matrix."""
        out = (C.c_size_t * 3)()
        _check(self._fn("state")(self._h, out))
        return tuple(int(v) for v in out)


class _MatrixWindows:
    """The far-row windows' controls of the two lookahead matrices."""

    @staticmethod
    def period() -> int:
        """Q: rows s >= Q are far rows, an output anchors once every Q blocks."""
        return int(lib().fftconv_matrix_lookahead_period())

    def set_windows(self, on: bool):
        """off: every output sums its far rows in full on every block (the same bits)."""
        _check(self._fn("set_windows")(self._h, 1 if on else 0))

    def anchors(self) -> int:
        """Outputs (with at least one pair) that anchor when the next block starts."""
        return int(self._fn("anchors")(self._h))


class _MatrixCrossfade(_UpdatePairs):
    """What the two crossfaded matrices share.  `_all_pairs()` lists the
    handle's (output, input) pairs in pair order."""

    def update_input(self, i: int, responses):
        """update_pairs of every pair that reads input i, in pair order: responses[those pairs][len]."""
        self.update_pairs([p for p in self._all_pairs() if p[1] == i], responses)

    def update_output(self, o: int, responses):
        """update_pairs of every pair that feeds output o, in pair order: responses[those pairs][len]."""
        self.update_pairs([p for p in self._all_pairs() if p[0] == o], responses)

    def diff_pairs(self) -> int:
        """|D|: the pairs whose spectra may differ between the two convolvers."""
        return int(self._fn("diff_pairs")(self._h))

    def last_patch(self):
        """(pairs transformed, pairs copied) by the last applied swap."""
        out = (C.c_size_t * 2)()
        _check(self._fn("last_patch")(self._h, out))
        return tuple(int(v) for v in out)

    def is_crossfading(self) -> bool:
        return bool(self._fn("is_crossfading")(self._h))

    def set_fused(self, on: bool):
        """False: every call takes the composition path (tests, A/B runs)."""
        _check(self._fn("set_fused")(self._h, 1 if on else 0))

    def path(self) -> int:
        """The path the next process() takes: 0 composition, 1 fused with both
        convolvers live, 2 fused with one convolver idle."""
        return int(self._fn("path")(self._h))


class _DenseMatrix(_MatrixGeometry):
    """init of the plain and the lookahead dense matrix."""

    @classmethod
    def init(cls, responses, max_block_size: int, max_response_length: int, device: int = 0):
        """responses[O][I][len]: h[o][i] is the response from input i to output o."""
        r = _dense_responses(responses)
        O, I, n = r.shape
        h = cls._cfn("init")(device, I, O, _p(r), n, n, max_block_size, max_response_length)
        return cls(_handle(h), I, O)


class _ListedMatrix(_UpdatePairs, _MatrixGeometry):
    """Construction of the plain and the lookahead matrix over a listed pair set."""

    def __init__(self, h, inputs: int, outputs: int, pairs: int, pair_list=None):
        super().__init__(h, inputs, outputs)
        self._set_pair_list(pair_list, pairs)

    def _clone_args(self):
        return self.inputs, self.outputs, self.pairs, self._pair_list

    @classmethod
    def init(cls, pairs, responses, inputs: int, outputs: int, max_block_size: int, max_response_length: int,
             device: int = 0):
        """pairs: (output, input) tuples, strictly ascending; responses[n] is
        the response of pairs[n]."""
        po, pi = _pair_arrays(pairs)
        r = _listed_responses(responses, len(po))
        n = r.shape[1]
        h = cls._cfn("init")(device, inputs, outputs, len(po), po.ctypes.data_as(_u32p), pi.ctypes.data_as(_u32p),
                             _p(r), n, n, max_block_size, max_response_length)
        return cls(_handle(h), inputs, outputs, len(po), list(zip(po.tolist(), pi.tolist())))


class MatrixConvolver(_UpdatePairs, _DenseMatrix):
    """Multi-input multi-output partitioned convolution (fftconv.h,
    "MatrixConvolver"): y[o] = sum_i x[i] * h[o][i], as inputs x outputs
    FFTConvolver instances in lockstep with one delay line per input."""

    _prefix = "matrix"

    @property
    def mac_parts(self) -> int:
        """Workgroups sharing one output's spectral sum, for the current active_seg_count."""
        return int(lib().fftconv_matrix_mac_parts(self._h))


class MatrixLookaheadConvolver(_MatrixWindows, _DenseMatrix):
    """The MatrixConvolver with far-row windows (fftconv.h,
    "MatrixLookaheadConvolver"): the same inputs x outputs FFTConvolver instances
    in lockstep, but an output's rows s >= period are summed once every `period`
    blocks for the next `period` blocks.  Blocks 32..512."""

    _prefix = "matrix_lookahead"

    @property
    def near_parts(self) -> int:
        """Workgroups sharing one output's near sum, for the current active_seg_count."""
        return int(lib().fftconv_matrix_lookahead_near_parts(self._h))

    @property
    def far_parts(self) -> int:
        """Workgroups sharing one output's far sum (0: no far rows, active <= Q)."""
        return int(lib().fftconv_matrix_lookahead_far_parts(self._h))


class SparseMatrixConvolver(_ListedMatrix):
    """Matrix convolution over a listed pair set (fftconv.h,
    "SparseMatrixConvolver"): one FFTConvolver instance per listed (output,
    input) pair, in lockstep; output o is the sum of the instances listed for
    it, an output without pairs is zero.  Only the listed pairs are stored,
    uploaded and streamed."""

    _prefix = "matrix_sparse"

    def output_parts(self, o: int) -> int:
        """P_o: workgroups sharing output o's spectral sum, for the current active_seg_count."""
        return int(lib().fftconv_matrix_sparse_output_parts(self._h, o))


class SparseMatrixLookaheadConvolver(_MatrixWindows, _ListedMatrix):
    """The SparseMatrixConvolver with the MatrixLookaheadConvolver's far-row
    windows (fftconv.h, "SparseMatrixLookaheadConvolver"): one FFTConvolver
    instance per listed (output, input) pair, an output's rows s >= period summed
    once every `period` blocks for the next `period` blocks.  Blocks 32..512."""

    _prefix = "matrix_sparse_lookahead"

    def near_parts(self, o: int) -> int:
        """Pn_o: workgroups sharing output o's near sum, for the current active_seg_count."""
        return int(self._fn("near_parts")(self._h, o))

    def far_parts(self, o: int) -> int:
        """Pf_o: workgroups sharing output o's far sum (0: no far rows or no pairs)."""
        return int(self._fn("far_parts")(self._h, o))


class MatrixCrossfadeConvolver(_MatrixCrossfade, _MatrixBase):
    """Crossfaded response switching for the matrix (fftconv.h,
    "MatrixCrossfadeConvolver"): inputs x outputs CrossfadeConvolver<FFTConvolver>
    instances in lockstep, one crossfader, the mix applied to the per-output sums."""

    _prefix = "matrix_crossfade"

    def __init__(self, h, inputs: int, outputs: int, max_buffer_size: int):
        super().__init__(h, inputs, outputs)
        self.max_buffer_size = max_buffer_size

    def _clone_args(self):
        return self.inputs, self.outputs, self.max_buffer_size

    def _all_pairs(self):
        return [(o, i) for o in range(self.outputs) for i in range(self.inputs)]

    @classmethod
    def init(cls, responses, max_block_size: int, max_response_length: int, device: int = 0):
        """Convolution::init (:46-49) over responses[O][I][len]: the fade takes
        len samples, the hold min(max_block_size, len)."""
        r = _dense_responses(responses)
        O, I, n = r.shape
        h = lib().fftconv_matrix_crossfade_init(device, I, O, _p(r), n, n, max_block_size, max_response_length)
        return cls(_handle(h), I, O, max_block_size)

    @classmethod
    def new(cls, convolver: MatrixConvolver, max_response_length: int, max_buffer_size: int, crossfade_samples: int):
        """CrossfadeConvolver::new (:19-43); the MatrixConvolver is cloned."""
        if not isinstance(convolver, MatrixConvolver):
            raise TypeError("convolver must be a MatrixConvolver")
        h = lib().fftconv_matrix_crossfade_new(convolver._h, max_response_length, max_buffer_size, crossfade_samples)
        return cls(_handle(h), convolver.inputs, convolver.outputs, max_buffer_size)


class SparseMatrixCrossfadeConvolver(_MatrixCrossfade, _MatrixBase):
    """Crossfaded response switching for the sparse matrix (fftconv.h,
    "SparseMatrixCrossfadeConvolver"): one CrossfadeConvolver<FFTConvolver>
    instance per listed (output, input) pair, in lockstep, one crossfader, the
    mix applied to the per-output sums; update_pairs takes listed pairs."""

    _prefix = "matrix_sparse_crossfade"

    def __init__(self, h, inputs: int, outputs: int, pair_list, max_buffer_size: int):
        super().__init__(h, inputs, outputs)
        self._set_pair_list(pair_list)
        self.max_buffer_size = max_buffer_size

    def _clone_args(self):
        return self.inputs, self.outputs, self._pair_list, self.max_buffer_size

    def _all_pairs(self):
        return self._pair_list

    @classmethod
    def init(cls, pairs, responses, inputs: int, outputs: int, max_block_size: int, max_response_length: int,
             device: int = 0):
        """Convolution::init (:46-49) over the listed pairs ((output, input)
        tuples, strictly ascending; responses[n] is the response of pairs[n]):
        the fade takes len samples, the hold min(max_block_size, len)."""
        po, pi = _pair_arrays(pairs)
        r = _listed_responses(responses, len(po))
        n = r.shape[1]
        h = lib().fftconv_matrix_sparse_crossfade_init(device, inputs, outputs, len(po), po.ctypes.data_as(_u32p),
                                                       pi.ctypes.data_as(_u32p), _p(r), n, n, max_block_size,
                                                       max_response_length)
        return cls(_handle(h), inputs, outputs, list(zip(po.tolist(), pi.tolist())), max_block_size)

    @classmethod
    def new(cls, convolver: SparseMatrixConvolver, max_response_length: int, max_buffer_size: int,
            crossfade_samples: int):
        """CrossfadeConvolver::new (:19-43); the SparseMatrixConvolver is cloned."""
        if not isinstance(convolver, SparseMatrixConvolver):
            raise TypeError("convolver must be a SparseMatrixConvolver")
        h = lib().fftconv_matrix_sparse_crossfade_new(convolver._h, max_response_length, max_buffer_size,
                                                      crossfade_samples)
        return cls(_handle(h), convolver.inputs, convolver.outputs, convolver._pair_list, max_buffer_size)


class MatrixLookaheadCrossfadeConvolver(_MatrixWindows, _MatrixCrossfade, _MatrixBase):
    """The MatrixCrossfadeConvolver over two MatrixLookaheadConvolvers (fftconv.h,
    "MatrixLookaheadCrossfadeConvolver"): the same crossfaded switching and
    update_pairs, each live convolver's far rows summed once every `period`
    blocks.  Blocks 32..512."""

    _prefix = "matrix_lookahead_crossfade"

    def __init__(self, h, inputs: int, outputs: int, max_buffer_size: int):
        super().__init__(h, inputs, outputs)
        self.max_buffer_size = max_buffer_size

    def _clone_args(self):
        return self.inputs, self.outputs, self.max_buffer_size

    def _all_pairs(self):
        return [(o, i) for o in range(self.outputs) for i in range(self.inputs)]

    def anchors(self, which: int) -> int:
        """Outputs of convolver `which` (0 = A, 1 = B) that anchor when the next
        block starts; 0 for an idle convolver."""
        return int(self._fn("anchors")(self._h, which))

    @classmethod
    def init(cls, responses, max_block_size: int, max_response_length: int, device: int = 0):
        """Convolution::init (:46-49) over responses[O][I][len], as MatrixCrossfadeConvolver.init."""
        r = _dense_responses(responses)
        O, I, n = r.shape
        h = cls._cfn("init")(device, I, O, _p(r), n, n, max_block_size, max_response_length)
        return cls(_handle(h), I, O, max_block_size)

    @classmethod
    def new(cls, convolver: MatrixLookaheadConvolver, max_response_length: int, max_buffer_size: int,
            crossfade_samples: int):
        """CrossfadeConvolver::new (:19-43); the MatrixLookaheadConvolver is cloned."""
        if not isinstance(convolver, MatrixLookaheadConvolver):
            raise TypeError("convolver must be a MatrixLookaheadConvolver")
        h = cls._cfn("new")(convolver._h, max_response_length, max_buffer_size, crossfade_samples)
        return cls(_handle(h), convolver.inputs, convolver.outputs, max_buffer_size)


class MatrixTwoStageConvolver(_Base):
    """Two-stage partitioning for the matrix (fftconv.h,
    "MatrixTwoStageConvolver"): inputs x outputs TwoStageFFTConvolver instances
    in lockstep -- a head and a first tail stage of block max_block_size, a tail
    of block tail_block_size -- with one delay line per input and stage."""

    _prefix = "matrix_twostage"

    def __init__(self, h, inputs: int, outputs: int):
        super().__init__(h, inputs)
        self.inputs = inputs
        self.outputs = outputs

    @classmethod
    def init(cls, responses, max_block_size: int, max_response_length: int, device: int = 0):
        """responses[O][I][len]: h[o][i] is the response from input i to output o."""
        r = _dense_responses(responses)
        O, I, n = r.shape
        h = lib().fftconv_matrix_twostage_init(device, I, O, _p(r), n, n, max_block_size, max_response_length)
        return cls(_handle(h), I, O)

    def update(self, responses):
        """todo!() in the reference (src/fft_convolver.rs:408-410): raises
        NotImplementedInReference, the handle is unchanged."""
        r = _dense_responses(responses, self.inputs, self.outputs)
        _check(lib().fftconv_matrix_twostage_update(self._h, _p(r), r.shape[2], r.shape[2]))

    def reset(self):
        _check(lib().fftconv_matrix_twostage_reset(self._h))

    def process(self, inp) -> np.ndarray:
        """x[inputs][n <= max_block_size] -> y[outputs][n]."""
        x = _f32(inp)
        if x.ndim != 2 or x.shape[0] != self.inputs:
            raise ValueError(f"input must be [{self.inputs}][n]")
        n = x.shape[1]
        y = np.zeros((self.outputs, n), np.float32)
        _check(lib().fftconv_matrix_twostage_process(self._h, _p(x), _p(y), n))
        return y

    def clone(self):
        return MatrixTwoStageConvolver(_handle(lib().fftconv_matrix_twostage_clone(self._h)), self.inputs,
                                       self.outputs)

    @property
    def tail_block_size(self) -> int:
        return int(lib().fftconv_matrix_twostage_tail_block_size(self._h))

    def set_fused(self, on: bool):
        """False: every call takes the composition path (tests, A/B runs)."""
        _check(lib().fftconv_matrix_twostage_set_fused(self._h, 1 if on else 0))

    def path(self, n: int) -> int:
        """The path the next process() of n samples takes: 0 composition, 1 fused."""
        return int(lib().fftconv_matrix_twostage_path(self._h, n))


class SparseMatrixTwoStageConvolver(_Base):
    """Two-stage partitioning over a listed pair set (fftconv.h,
    "SparseMatrixTwoStageConvolver"): one TwoStageFFTConvolver instance per
    listed (output, input) pair, in lockstep -- head, first tail stage and tail
    are sparse matrices over the same pattern; output o is the sum of the
    instances listed for it, an output without pairs is zero."""

    _prefix = "matrix_sparse_twostage"

    def __init__(self, h, inputs: int, outputs: int, pair_list):
        super().__init__(h, inputs)
        self.inputs = inputs
        self.outputs = outputs
        self._pair_list = [(int(o), int(i)) for o, i in pair_list]

    @classmethod
    def init(cls, pairs, responses, inputs: int, outputs: int, max_block_size: int, max_response_length: int,
             device: int = 0):
        """pairs: (output, input) tuples, strictly ascending; responses[n] is
        the response of pairs[n]."""
        po, pi = _pair_arrays(pairs)
        r = _listed_responses(responses, len(po))
        lst = list(zip(po.tolist(), pi.tolist()))
        if any(b <= a for a, b in zip(lst, lst[1:])):
            raise ValueError("the pair list must be strictly ascending in (output, input)")
        n = r.shape[1]
        h = lib().fftconv_matrix_sparse_twostage_init(device, inputs, outputs, len(po), po.ctypes.data_as(_u32p),
                                                      pi.ctypes.data_as(_u32p), _p(r), n, n, max_block_size,
                                                      max_response_length)
        return cls(_handle(h), inputs, outputs, lst)

    def update(self, responses):
        """todo!() in the reference (src/fft_convolver.rs:408-410): raises
        NotImplementedInReference, the handle is unchanged."""
        r = _listed_responses(responses, self.pairs)
        _check(self._fn("update")(self._h, _p(r), r.shape[1], r.shape[1]))

    def reset(self):
        _check(self._fn("reset")(self._h))

    def process(self, inp) -> np.ndarray:
        """x[inputs][n <= max_block_size] -> y[outputs][n]."""
        x = _f32(inp)
        if x.ndim != 2 or x.shape[0] != self.inputs:
            raise ValueError(f"input must be [{self.inputs}][n]")
        n = x.shape[1]
        y = np.zeros((self.outputs, n), np.float32)
        _check(self._fn("process")(self._h, _p(x), _p(y), n))
        return y

    def clone(self):
        return SparseMatrixTwoStageConvolver(_handle(self._fn("clone")(self._h)), self.inputs, self.outputs,
                                             self._pair_list)

    @property
    def pairs(self) -> int:
        return len(self._pair_list)

    @property
    def tail_block_size(self) -> int:
        return int(self._fn("tail_block_size")(self._h))

    def set_fused(self, on: bool):
        """False: every call takes the composition path (tests, A/B runs)."""
        _check(self._fn("set_fused")(self._h, 1 if on else 0))

    def path(self, n: int) -> int:
        """The path the next process() of n samples takes: 0 composition, 1 fused."""
        return int(self._fn("path")(self._h, n))


__all__ = [
    "Fft", "FFTConvolver", "TwoStageFFTConvolver", "CrossfadeConvolver", "MatrixConvolver",
    "MatrixLookaheadConvolver", "SparseMatrixConvolver", "SparseMatrixLookaheadConvolver",
    "MatrixCrossfadeConvolver", "SparseMatrixCrossfadeConvolver", "MatrixLookaheadCrossfadeConvolver",
    "MatrixTwoStageConvolver",
    "SparseMatrixTwoStageConvolver", "ConvolutionPanic",
    "NotImplementedInReference", "DeviceError", "complex_size", "compute_tail_block_size", "device_count",
    "lib", "LIB_PATH", "SIGNATURES",
]
