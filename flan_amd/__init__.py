"""flan_amd -- thin Python doorway to the MI355X phase-vocoder hot path (flan_amd/libflanhip.so).

The product is the HIP library behind the C ABI in include/flanhip.h and the C++ host classes in include/flan/.
This module is plumbing for tests and bench.py: it binds the C ABI with ctypes and nothing else.  There is no
CPU fallback and no import of anything under oracle/: if the library is missing, importing fails; if no GPU is
visible, every compute call raises FlanHipError(FLANHIP_ERR_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLAN_AMD_LIB") or os.path.join(_HERE, "libflanhip.so")   # FLAN_AMD_LIB: A/B a second build

OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_CANCELLED, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5


class FlanHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("flanhip error %d: %s" % (code, message))
        self.code = code


if not os.path.exists(LIB_PATH):
    raise ImportError("flan_amd/libflanhip.so is missing: build it with `python flan_amd/build.py` "
                      "(hipcc --offload-arch=gfx950); there is no fallback path")

lib = C.CDLL(LIB_PATH)

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_vp, _i64, _i32, _f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float

_SIGS = {
    "flanhip_version": (C.c_int, []),
    "flanhip_last_error": (C.c_char_p, []),
    "flanhip_device_count": (C.c_int, []),
    "flanhip_set_device": (C.c_int, [_i32]),
    "flanhip_get_device": (C.c_int, [C.POINTER(C.c_int)]),
    "flanhip_num_pv_frames": (_i64, [_i64, _i32]),
    "flanhip_hop_size": (C.c_int, [_f32, _f32]),
    "flanhip_modify_time_out_frames": (_i64, [_vp, _i64, _i32, _f32, _i32]),
    "flanhip_malloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "flanhip_free": (C.c_int, [_vp]),
    "flanhip_upload": (C.c_int, [_vp, _vp, C.c_size_t]),
    "flanhip_download": (C.c_int, [_vp, _vp, C.c_size_t]),
    "flanhip_touch_pages": (C.c_int, [_vp, C.c_size_t]),
    "flanhip_host_workers": (C.c_int, []),
    "flanhip_parallel_for": (C.c_int, [C.c_int, _vp, _vp]),
    "flanhip_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "flanhip_stream_destroy": (C.c_int, [_vp]),
    "flanhip_host_malloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "flanhip_host_free": (C.c_int, [_vp]),
    "flanhip_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "flanhip_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "flanhip_memset": (C.c_int, [_vp, _i32, C.c_size_t, _vp]),
    "flanhip_stream_synchronize": (C.c_int, [_vp]),
    "flanhip_wait_cancellable": (C.c_int, [_vp, _vp]),
    "flanhip_wait_cancellable_fn": (C.c_int, [_vp, _vp, _vp]),
    "flanhip_analyze": (C.c_int, [_vp, _i64, _i64, _f32, _i32, _i32, _i32, _vp, C.POINTER(_i64), _vp]),
    "flanhip_analyze_dev": (C.c_int, [_vp, _i64, _i64, _f32, _i32, _i32, _i32, _vp, _vp]),
    "flanhip_synthesize": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, C.POINTER(_i32), _vp]),
    "flanhip_synthesize_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _f32, _f32, _i32]),
    "flanhip_synthesize_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "flanhip_analyze_dev_fused": (C.c_int, [_vp, _i64, _i64, _f32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "flanhip_synthesize_dev_fused": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "flanhip_synthesize_dev_stages": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _i32, _i32, _vp]),
    "flanhip_debug_option": (None, [_i32, _i32]),
    "flanhip_debug_kernel_scratch_bytes": (_i32, [_i32]),
    "flanhip_modify_time": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _i64, _vp, _vp]),
    "flanhip_modify_time_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _i64, _vp, _vp]),
    "flanhip_modify_time_dev_fused": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _vp, _i64, _vp, _i32, _vp, _vp]),
    "flanhip_synthesize_dev_fused_checked": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "flanhip_stretch_map_dev": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp, _vp]),
    "flanhip_stretch_map_const_dev": (C.c_int, [_f32, _vp, _i64, _i32, _f32, _i32, _vp, _vp]),
    "flanhip_fill_dev": (C.c_int, [_vp, _i64, _f32, _vp]),
    "flanhip_modify_frequency": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _vp]),
    "flanhip_modify_frequency_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp, _vp]),
    "flanhip_modify_time_interp_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _i64, _i32, _vp, _vp]),
    "flanhip_modify_time_interp_dev_fused": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "flanhip_modify_frequency_interp_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _i32, _vp, _vp]),
    "flanhip_repitch_interp_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _i32, _vp, _vp]),
    "flanhip_repitch_map_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp]),
    "flanhip_repitch_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp]),
    "flanhip_shape_affine": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "flanhip_shape_affine_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "flanhip_shape_table_dev": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _f32, _i32, _vp, _vp]),
    "flanhip_replace_amplitudes_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _f32, _vp, _vp]),
    "flanhip_subtract_amplitudes_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _f32, _vp, _vp]),
    "flanhip_resonate_out_frames": (_i64, [_i64, _f32, _f32, _i32]),
    "flanhip_resonate_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _i64, _vp, _f32, _vp, _vp]),
    "flanhip_n_loudest_partials_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, C.c_int32, _i32, _vp, _vp]),
    "flanhip_desample_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _f32, _i32, _vp, _vp]),
    "flanhip_interp_table_create": (C.c_int, [_vp, _vp]),
    "flanhip_interp_table_destroy": (C.c_int, [_i32]),
    "flanhip_time_extrapolate_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i64, _i64, _i64, _vp, _vp, _vp]),
    "flanhip_shape_affine_dev_fused": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _i32, _vp, _vp]),
    "flanhip_shape_table_dev_fused": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _f32, _f32, _vp, _i32, _vp, _vp]),
    "flanhip_get_frame_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _vp]),
    "flanhip_select_frames_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "flanhip_freeze_plan": (_i64, [_i64, _f32, _i32, _vp, _vp, _i32, _vp]),
    "flanhip_cut_frames_range": (C.c_int, [_i64, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "flanhip_cut_frames_dev": (C.c_int, [_vp, _i64, _i64, _i32, _i64, _i64, _vp, _vp]),
    "flanhip_place_frames_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _i64, _vp]),
    "flanhip_select_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _i64, _vp, _vp]),
    "flanhip_harmonic_scale_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _i32, _i32, _vp, _vp]),
    "flanhip_modify_out_frames": (_i64, [_vp, _i64, _i32, _f32, _i32]),
    "flanhip_modify_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _vp, _i32, _i64, _vp, _vp]),
    "flanhip_stretch_spline_out_frames": (_i64, [_vp, _i64]),
    "flanhip_stretch_spline_dev": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "flanhip_smear_time_plan": (C.c_int, [_i64, _i32, _f32, _i32, _vp, _f32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "flanhip_smear_time_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _f32, _vp, _i32, _vp, _i64, _i32, _i64, _vp, _vp]),
    "flanhip_mid_side_dev": (C.c_int, [_vp, _i64, _vp, _vp]),
    "flanhip_resample_out_frames": (_i64, [_i64, _f32, _f32]),
    "flanhip_resample": (C.c_int, [_vp, _i64, _i64, _f32, _f32, _vp, _vp]),
    "flanhip_resample_dev": (C.c_int, [_vp, _i64, _i64, _f32, _f32, _vp, _vp]),
    "flanhip_synthesize_prepass_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "flanhip_synthesize_dev_carry": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "flanhip_comm_unique_id": (C.c_int, [C.c_char_p]),
    "flanhip_comm_init": (C.c_int, [C.c_char_p, _i32, _i32, C.POINTER(_vp)]),
    "flanhip_comm_destroy": (C.c_int, [_vp]),
    "flanhip_allgather_audio": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "flanhip_noise_dev": (C.c_int, [_vp, _i64, _i64, C.c_uint32, _vp]),
    "flanhip_sqdiff_dev": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "flanhip_copy_dev": (C.c_int, [_vp, _vp, _i64, _vp]),
    "flanhip_spv_analyze": (C.c_int, [_vp, _i64, _i64, _f32, _i32, _vp, _vp]),
    "flanhip_spv_analyze_dev": (C.c_int, [_vp, _i64, _i64, _f32, _i32, _vp, _vp]),
    "flanhip_spv_synthesize_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _f32]),
    "flanhip_spv_synthesize": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp]),
    "flanhip_spv_synthesize_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _vp, _vp, _vp]),
    "flanhip_spv_modify_frequency_const_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i32, _vp, _vp]),
    "flanhip_spv_twiddles": (C.c_int, [_i32, _vp]),
    "flanhip_spv_debug_chain_length": (None, [_i32]),
    "flanhip_convolve_out_frames": (_i64, [_i64, _i64]),
    "flanhip_convolve_workspace_bytes": (C.c_size_t, [_i64, _i64, _i64, _i64]),
    "flanhip_convolve": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _f32, _i32, _vp, _vp]),
    "flanhip_convolve_dev": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _f32, _i32, _vp, _vp, _vp]),
    "flanhip_convolve_debug_partition": (None, [_i32]),
    "flanhip_audio_repitch_out_frames": (_i64, [_vp, _i64, _i64]),
    "flanhip_audio_repitch_plan": (_i64, [_i64, _f32, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "flanhip_audio_repitch_runs": (_i64, [_i64, _f32, _vp, _i64, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i64)]),
    "flanhip_audio_repitch_workspace_bytes": (C.c_size_t, [_i64, _f32, _vp, _i64, _i64, _i32]),
    "flanhip_audio_repitch": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64, _i32, _vp, _vp]),
    "flanhip_audio_repitch_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "flanhip_compress_workspace_bytes": (C.c_size_t, [_i64]),
    "flanhip_compress": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64] + [_vp, _f32] * 5 + [_vp, _vp, _vp]),
    "flanhip_compress_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64] + [_vp, _f32] * 5 + [_vp, _vp, _vp, _vp]),
    "flanhip_compress_debug_run": (None, [_i32]),
    "flanhip_audio_gain_dev": (C.c_int, [_vp, _i64, _i64, _vp, _f32, _vp, _vp]),
    "flanhip_audio_set_volume_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_audio_set_volume_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _f32, _vp, _vp, _vp]),
    "flanhip_filter_1pole_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_filter_1pole": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _f32, _i32, _i32, _vp, _vp]),
    "flanhip_filter_1pole_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _f32, _i32, _i32, _vp, _vp, _vp]),
    "flanhip_filter_debug_run": (None, [_i32]),
    "flanhip_filter2_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_filter2": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 3 + [_i32, _i32, _vp, _vp]),
    "flanhip_filter2_dev": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 3 + [_i32, _i32, _vp, _vp, _vp]),
    "flanhip_filter_comb_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_filter_comb_debug_local": (None, [_i32]),
    "flanhip_filter_comb": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 3 + [_i32, _vp, _vp]),
    "flanhip_filter_comb_dev": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 3 + [_i32, _vp, _vp, _vp]),
    "flanhip_multinotch_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _i32]),
    "flanhip_multinotch_debug_run": (None, [_i32]),
    "flanhip_multinotch": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 4 + [_i32, _i32, _i32, _vp, _vp]),
    "flanhip_multinotch_dev": (C.c_int, [_vp, _i64, _i64, _f32] + [_vp, _f32] * 4 + [_i32, _i32, _i32, _vp, _vp, _vp]),
    "flanhip_halfband_poles": (None, [_vp, _vp]),
    "flanhip_halfband_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_halfband_debug_run": (None, [_i32]),
    "flanhip_hilbert": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _vp, _vp]),
    "flanhip_hilbert_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "flanhip_halfband_modulate": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _f32, _vp, _f32, _vp, _vp, _vp]),
    "flanhip_halfband_modulate_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _f32, _vp, _f32, _vp, _vp, _vp, _vp]),
    "flanhip_halfband_multiply": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64, _f32, _vp, _vp]),
    "flanhip_halfband_multiply_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _i64, _f32, _vp, _vp, _vp]),
    "flanhip_spatial_ear": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _vp, C.c_double, C.c_double, _f32, _i32, _vp, _vp]),
    "flanhip_spatial_ear_dev": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _vp, C.c_double, C.c_double, _f32, _i32, _vp, _vp]),
    "flanhip_spatial_delay_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "flanhip_spatial_itd_out_frames": (_i64, [_i64, _f32, _vp, _i64, _vp]),
    "flanhip_spatial_itd_plan": (_i64, [_i64, _f32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "flanhip_spatial_itd_workspace_bytes": (C.c_size_t, [_i64, _i64, _f32, _vp, _i64]),
    "flanhip_spatial_itd": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_spatial_itd_dev": (C.c_int, [_vp, _i64, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "flanhip_audio_pan": (C.c_int, [_vp, _i64, _i64, _vp, _f32, _vp, _vp]),
    "flanhip_audio_pan_dev": (C.c_int, [_vp, _i64, _i64, _vp, _f32, _vp, _vp]),
    "flanhip_audio_to_stereo_dev": (C.c_int, [_vp, _i64, _vp, _vp]),
    "flanhip_audio_to_mono_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "flanhip_audio_copy_rows_dev": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp]),
    "flanhip_audio_local_wavelengths_count": (_i64, [_i64] * 5),
    "flanhip_audio_local_wavelengths_workspace_bytes": (C.c_size_t, [_i64] * 5),
    "flanhip_audio_yin_dprime_dev": (C.c_int, [_vp] + [_i64] * 5 + [_vp, _vp]),
    "flanhip_audio_yin_pick_dev": (C.c_int, [_vp, _i64, _i64, _f32, _i64, _vp, _vp]),
    "flanhip_audio_local_wavelengths_dev": (C.c_int, [_vp] + [_i64] * 5 + [_f32, _i64, _vp, _vp, _vp]),
    "flanhip_audio_local_wavelength_dev": (C.c_int, [_vp, _i64, _f32, _i64, _vp, _vp]),
    "flanhip_audio_local_wavelengths": (C.c_int, [_vp, _i64, _f32] + [_i64] * 4 + [_f32, _i64, _vp, _vp]),
    "flanhip_wavelength_continuity": (C.c_int, [_vp, _i64, _f32, _i64]),
    "flanhip_average_wavelength": (C.c_int, [_vp, _i64, _f32, _f32, _vp]),
    "flanhip_grains_tile_frames": (_i64, []),
    "flanhip_grains_batch_events": (_i64, []),
    "flanhip_grains_events": (C.c_int, [_i64, _f32, _vp, _f32, _vp, _f32, C.c_uint64, _vp, _i64, _vp]),
    "flanhip_grains_cut": (C.c_int, [_i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp]),
    "flanhip_grains_cut_frames": (C.c_int, [_i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "flanhip_grains_plan": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64]),
    "flanhip_grains_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_grains_mix_dev": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _f32, _vp, _vp, _vp]),
    "flanhip_grains_mix": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _f32, _vp, _vp]),
    "flanhip_wavetable_snap": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _vp]),
    "flanhip_wavetable_starts": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i64, _vp]),
    "flanhip_wavetable_table_index": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp]),
    "flanhip_wavetable_slots": (_i64, [_vp, _i64]),
    "flanhip_wavetable_resample_workspace_bytes": (C.c_size_t, [_i64, _i64, _vp, _vp, _i32]),
    "flanhip_wavetable_resample_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "flanhip_wavetable_resample": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp]),
    "flanhip_wavetable_synth_plan": (_i64, [_i64, _f32, _i32, _i64, _vp, _i64, _i64] + [_vp] * 10),
    "flanhip_wavetable_synth_runs": (_i64, [_i64, _f32, _i32, _i64, _vp, _i64, _i64, _i64] + [_vp] * 7 + [C.POINTER(_i32), C.POINTER(_i64)]),
    "flanhip_wavetable_synth_workspace_bytes": (C.c_size_t, [_i64, _i64, _f32, _i32, _i64, _vp, _i64]),
    "flanhip_wavetable_synth_dev": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i64, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "flanhip_wavetable_synth": (C.c_int, [_vp, _i64, _i64, _i32, _f32, _i64, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    "flanhip_wavetable_edit_dev": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "flanhip_wavetable_edit": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "flanhip_spectrum_bins": (_i64, [_i32, _i32, _vp, _vp, _i64]),
    "flanhip_spectrum_num_harmonics": (_i32, [_i32]),
    "flanhip_spectrum_phases": (C.c_int, [C.c_uint32, _vp, _i64, _vp]),
    "flanhip_spectrum_jump": (_i32, [_i64, _i64, _i32]),
    "flanhip_spectrum_table_workspace_bytes": (C.c_size_t, [_i32]),
    "flanhip_spectrum_table_dev": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "flanhip_spectrum_table": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "flanhip_spectrum_synth_plan": (_i64, [_i64, C.c_double, _i64, _vp, _i64, _i64] + [_vp] * 10),
    "flanhip_spectrum_synth_workspace_bytes": (C.c_size_t, [_i32, C.c_double, _i64, _i64, _i64, _vp, _i64]),
    "flanhip_spectrum_synth_dev": (C.c_int, [_vp, _i32, C.c_double, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "flanhip_spectrum_synth": (C.c_int, [_vp, _i32, C.c_double, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_audio_synthesize_spectrum_workspace_bytes": (C.c_size_t, [_i32, _i32, _i64, _i64, _i64, _vp, _i64]),
    "flanhip_audio_synthesize_spectrum_dev": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "flanhip_audio_synthesize_spectrum": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_loud_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_loud_summary_dev": (C.c_int, [_vp, _i64, _i64, _f32, _i64, _vp, _vp, _vp]),
    "flanhip_loud_chunks_dev": (C.c_int, [_i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_loud_chunks": (C.c_int, [_vp, _i64, _i64, _f32, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_loud_debug_run": (None, [_i32]),
    "flanhip_loud_run_frames": (_i64, []),
    "flanhip_loud_block_frames": (_i64, []),
    "flanhip_loud_carry_pass_blocks": (_i64, []),
    "flanhip_audio_reverse_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "flanhip_audio_reverse": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "flanhip_loud_chunks_fades": (C.c_int, [_i64, _f32, _vp, _i64, _f32, _i32, _vp, _vp]),
    "flanhip_edge_silence_cut": (C.c_int, [_i64, _f32, _i64, _i64, _f32, _vp]),
    "flanhip_split_frames": (C.c_int, [_i64, _f32, _vp, _i64, _vp, _i64, _vp]),
    "flanhip_rearrange_order": (C.c_int, [_i64, C.c_uint64, _vp]),
    "flanhip_random_chunks_frames": (_i64, [_f32, _f32]),
    "flanhip_random_chunks_plan": (C.c_int, [_i64, _f32, _f32, _vp, _f32, _vp, _f32, C.c_uint64, _vp, _vp, _vp, _i64, _vp]),
    "flanhip_audio_ring_modulate_dev": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    "flanhip_fade_frames_plan": (C.c_int, [_i64, C.c_int32, C.c_int32, _vp]),
    "flanhip_audio_fade_dev": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "flanhip_waveform_dev": (C.c_int, [_i32, _vp, _i64, _vp, _vp]),
    "flanhip_waveform_host": (C.c_int, [_i32, _vp, _i64, _vp]),
    "flanhip_audio_moisture_dev": (C.c_int, [_vp, _i64, _i64, _f32, _i64, _f32, _vp, _f32, _vp, _f32, _vp, _f32, _i32, _vp, _vp]),
    "flanhip_audio_energy_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "flanhip_audio_energy_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "flanhip_audio_rectify_dev": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "flanhip_synthesize_waveform_frames": (_i64, [_f32, _f32, _i32, _vp, _vp]),
    "flanhip_osc_workspace_bytes": (C.c_size_t, [_i64]),
    "flanhip_osc_phase_dev": (C.c_int, [_vp, _f32, _i64, C.c_double, _vp, _vp, _i32, _vp, _vp]),
    "flanhip_osc_debug_run": (None, [_i32]),
    "flanhip_osc_run_frames": (_i64, []),
    "flanhip_osc_block_frames": (_i64, []),
    "flanhip_osc_carry_pass_blocks": (_i64, []),
    "flanhip_oneshot_resample_dev": (C.c_int, [_vp, _i64, C.c_double, C.c_double, _vp, _i64, _vp]),
    "flanhip_audio_synthesize_waveform_workspace_bytes": (C.c_size_t, [_f32, _f32, _i32]),
    "flanhip_audio_synthesize_waveform_dev": (C.c_int, [_i32, _vp, _f32, _f32, _f32, _i32, _vp, _vp, _vp]),
    "flanhip_white_noise_draw": (C.c_int, [C.c_uint64, _i64, _vp]),
}

EXPORTS = sorted(_SIGS)
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)          # AttributeError here == the library does not export what the header declares
    _fn.restype = _res
    _fn.argtypes = _args


def last_error():
    return lib.flanhip_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != OK:
        raise FlanHipError(rc, last_error())
    return rc


def _ptr(a):
    return a.ctypes.data_as(_vp)


# ---------------------------------------------------------------------------------------------------------------
# host-buffer wrappers (numpy in, numpy out) -- exactly the calls the C++ flan::Audio / flan::PV classes make
# ---------------------------------------------------------------------------------------------------------------

def analyze(audio, sample_rate, window=2048, hop=128, dft=4096):
    """Audio::convert_to_PV.  audio float32 [ch][n] -> float32 [ch][F][dft/2+1][2] (m, f)."""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    F = lib.flanhip_num_pv_frames(n, hop)
    out = np.empty((ch, F, dft // 2 + 1, 2), np.float32)
    got = _i64(0)
    check(lib.flanhip_analyze(_ptr(audio), ch, n, sample_rate, window, hop, dft, _ptr(out), C.byref(got), None))
    assert got.value == F
    return out


def synthesize(pv, sample_rate, analysis_rate, window):
    """PV::convert_to_audio.  pv float32 [ch][F][bins][2] -> (float32 [ch][F*hop], nan_flag)."""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    hop = lib.flanhip_hop_size(sample_rate, analysis_rate)
    out = np.empty((ch, F * hop), np.float32)
    flag = _i32(0)
    check(lib.flanhip_synthesize(_ptr(pv), ch, F, bins, sample_rate, analysis_rate, window, _ptr(out), C.byref(flag), None))
    return out, flag.value


def modify_time(pv, sample_rate, hop, mod_seconds):
    pv = np.ascontiguousarray(pv, np.float32)
    mod = np.ascontiguousarray(mod_seconds, np.float32)
    ch, F, bins, _ = pv.shape
    Fo = lib.flanhip_modify_time_out_frames(_ptr(mod), F, bins, sample_rate, hop)
    out = np.empty((ch, max(Fo, 0), bins, 2), np.float32)
    if Fo > 0:
        check(lib.flanhip_modify_time(_ptr(pv), ch, F, bins, sample_rate, hop, _ptr(mod), Fo, _ptr(out), None))
    return out


def modify_frequency(pv, sample_rate, mod_hz, in_modified):
    pv = np.ascontiguousarray(pv, np.float32)
    mod = np.ascontiguousarray(mod_hz, np.float32)
    inm = np.ascontiguousarray(in_modified, np.float32)
    ch, F, bins, _ = pv.shape
    out = np.empty_like(pv)
    check(lib.flanhip_modify_frequency(_ptr(pv), ch, F, bins, sample_rate, _ptr(mod), _ptr(inm), _ptr(out), None))
    return out


def resample(audio, src_rate, dst_rate):
    """Audio::resample (r8brain's single-step ratios and its block convolver + whole-stepping interpolator ratios, e.g. 44.1 <-> 48 kHz).
    audio float32 [ch][n] -> float32 [ch][n_out]"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    n_out = lib.flanhip_resample_out_frames(n, src_rate, dst_rate)
    out = np.empty((ch, n_out), np.float32)
    check(lib.flanhip_resample(_ptr(audio), ch, n, src_rate, dst_rate, _ptr(out), None))
    return out


def shape_affine(pv, sample_rate, a, b, c, d, use_shift_alignment=False):
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    out = np.empty_like(pv)
    check(lib.flanhip_shape_affine(_ptr(pv), ch, F, bins, sample_rate, a, b, c, d, int(use_shift_alignment), _ptr(out), None))
    return out


class DeviceArray:
    """A device buffer owned through the C ABI (flanhip_malloc / flanhip_free), optionally filled from a numpy array."""

    def __init__(self, nbytes=None, host=None):
        if host is not None:
            host = np.ascontiguousarray(host)
            nbytes = host.nbytes
        self.nbytes = int(nbytes)
        p = _vp()
        check(lib.flanhip_malloc(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value
        if host is not None and self.nbytes:
            check(lib.flanhip_memcpy_h2d(_vp(self.ptr), _ptr(host), self.nbytes, None))

    def data_ptr(self):
        return self.ptr

    def to_host(self, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert out.nbytes == self.nbytes, (out.nbytes, self.nbytes)
        if self.nbytes:
            check(lib.flanhip_memcpy_d2h(_ptr(out), _vp(self.ptr), self.nbytes, None))
        check(lib.flanhip_stream_synchronize(None))
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            lib.flanhip_free(_vp(self.ptr))
            self.ptr = None


def _grid_or_const(grid):
    """(device pointer or None, constant) for a sampled user function: numpy grid, or a python scalar"""
    if np.isscalar(grid):
        return None, float(grid), None
    d = DeviceArray(host=np.ascontiguousarray(grid, np.float32))
    return _vp(d.ptr), 0.0, d


def _combine_amplitudes(fn, pv, src, amount):
    pv = np.ascontiguousarray(pv, np.float32)
    src = np.ascontiguousarray(src, np.float32)
    ch, F, bins, _ = pv.shape
    sch, sF, sbins, _ = src.shape
    d_pv, d_src, d_out = DeviceArray(host=pv), DeviceArray(host=src), DeviceArray(pv.nbytes)
    a_ptr, a_const, _keep = _grid_or_const(amount)
    check(fn(_vp(d_pv.ptr), ch, F, bins, _vp(d_src.ptr), sch, sF, sbins, a_ptr, a_const, _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


def repitch(pv, sample_rate, factor_grid, interp=0):
    """PV::repitch.  factor_grid: float32 [F][bins] (the sampled factor); interp: FLANHIP_INTERP_*; returns the repitched PV"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    g = np.ascontiguousarray(factor_grid, np.float32)
    assert g.shape == (F, bins)
    d_pv, d_g, d_out = DeviceArray(host=pv), DeviceArray(host=g), DeviceArray(pv.nbytes)
    check(lib.flanhip_repitch_interp_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, _vp(d_g.ptr), interp, _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


def modify_time_interp(pv, sample_rate, hop, mod_seconds, interp):
    """PV::modify_time with a named Interpolator (FLANHIP_INTERP_*), device entry point"""
    pv = np.ascontiguousarray(pv, np.float32)
    mod = np.ascontiguousarray(mod_seconds, np.float32)
    ch, F, bins, _ = pv.shape
    Fo = lib.flanhip_modify_time_out_frames(_ptr(mod), F, bins, sample_rate, hop)
    if Fo <= 0:
        return np.empty((ch, 0, bins, 2), np.float32)
    d_pv, d_mod, d_out = DeviceArray(host=pv), DeviceArray(host=mod), DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_modify_time_interp_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, hop, _vp(d_mod.ptr), Fo, interp, _vp(d_out.ptr), None))
    return d_out.to_host((ch, Fo, bins, 2))


def modify_frequency_interp(pv, sample_rate, mod_hz, in_modified, interp):
    """PV::modify_frequency with a named Interpolator (FLANHIP_INTERP_*), device entry point"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    d_pv, d_mod, d_in = DeviceArray(host=pv), DeviceArray(host=np.ascontiguousarray(mod_hz, np.float32)), DeviceArray(host=np.ascontiguousarray(in_modified, np.float32))
    d_out = DeviceArray(pv.nbytes)
    check(lib.flanhip_modify_frequency_interp_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, _vp(d_mod.ptr), _vp(d_in.ptr), interp, _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


def replace_amplitudes(pv, src, amount):
    """PV::replace_amplitudes.  amount: float32 [F][bins] or a scalar"""
    return _combine_amplitudes(lib.flanhip_replace_amplitudes_dev, pv, src, amount)


def subtract_amplitudes(pv, src, amount):
    """PV::subtract_amplitudes"""
    return _combine_amplitudes(lib.flanhip_subtract_amplitudes_dev, pv, src, amount)


def resonate(pv, sample_rate, hop, length_seconds, decay):
    """PV::resonate.  decay: float32 [Fo][bins] over the OUTPUT's domain, or a scalar"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    Fo = int(lib.flanhip_resonate_out_frames(F, length_seconds, sample_rate, hop))
    assert Fo >= F, Fo
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(ch * Fo * bins * 8)
    d_ptr, d_const, _keep = _grid_or_const(decay)
    check(lib.flanhip_resonate_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, hop, Fo, d_ptr, d_const, _vp(d_out.ptr), None))
    return d_out.to_host((ch, Fo, bins, 2))


def n_loudest_partials(pv, n, remove=False):
    """PV::retain_n_loudest_partials / remove_n_loudest_partials.  n: int32 [F] or a scalar"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(pv.nbytes)
    if np.isscalar(n):
        n_ptr, n_const, _keep = None, int(n), None
    else:
        _keep = DeviceArray(host=np.ascontiguousarray(n, np.int32))
        n_ptr, n_const = _vp(_keep.ptr), 0
    check(lib.flanhip_n_loudest_partials_dev(_vp(d_pv.ptr), ch, F, bins, n_ptr, n_const, int(remove), _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


INTERP_TABLE_INTERVALS = 65536


class InterpTable:
    """an Interpolator built from a callable (Utility/Interpolator.h), sampled at i / 65536 and at NaN and registered with the library: use
    `.kind` wherever a FLANHIP_INTERP_* kind is taken; a context manager (the table is destroyed on exit)"""

    def __init__(self, fn):
        n = INTERP_TABLE_INTERVALS
        xs = np.arange(n + 1, dtype=np.float32) * np.float32(1.0 / n)
        samples = np.empty(n + 2, np.float32)
        samples[:n + 1] = [fn(np.float32(x)) for x in xs]
        samples[n + 1] = fn(np.float32(np.nan))
        kind = C.c_int(-1)
        check(lib.flanhip_interp_table_create(_ptr(samples), C.byref(kind)))
        self.kind = kind.value

    def close(self):
        if self.kind >= 0:
            check(lib.flanhip_interp_table_destroy(self.kind))
            self.kind = -1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def desample(pv, ratio, interp=0):
    """PV::desample.  ratio: float32 [F][bins] or a scalar; interp: FLANHIP_INTERP_*"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(pv.nbytes)
    r_ptr, r_const, _keep = _grid_or_const(ratio)
    check(lib.flanhip_desample_dev(_vp(d_pv.ptr), ch, F, bins, r_ptr, r_const, interp, _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


def time_extrapolate(pv, sample_rate, start_frame, end_frame, out_frames, interp_samples):
    """PV::time_extrapolate after its input validation.  interp_samples: float32 [out_frames - start_frame]"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    samples = np.ascontiguousarray(interp_samples, np.float32)
    assert samples.shape == (out_frames - start_frame,)
    d_pv, d_s, d_out = DeviceArray(host=pv), DeviceArray(host=samples), DeviceArray(ch * out_frames * bins * 8)
    check(lib.flanhip_time_extrapolate_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, start_frame, end_frame, out_frames,
                                           _vp(d_s.ptr), _vp(d_out.ptr), None))
    return d_out.to_host((ch, out_frames, bins, 2))


def get_frame(pv, frame_pos, interp=0):
    """PV::get_frame at the (already clamped) fractional frame position.  Returns [ch][1][bins][2]"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(ch * bins * 8)
    check(lib.flanhip_get_frame_dev(_vp(d_pv.ptr), ch, F, bins, frame_pos, interp, _vp(d_out.ptr), None))
    return d_out.to_host((ch, 1, bins, 2))


def freeze_plan(num_frames, sample_rate, hop, times, lengths):
    """PV::freeze's timing logic: int32 [out_frames], the input frame of every output frame (-1: stays zero)"""
    times = np.ascontiguousarray(times, np.float32)
    lengths = np.ascontiguousarray(lengths, np.float32)
    assert times.shape == lengths.shape and times.ndim == 1
    n = len(times)
    tp = times.ctypes.data_as(_vp) if n else None
    lp = lengths.ctypes.data_as(_vp) if n else None
    Fo = lib.flanhip_freeze_plan(num_frames, sample_rate, hop, tp, lp, n, None)
    if Fo < 0:
        raise FlanHipError(-1, "flanhip_freeze_plan: bad arguments")
    src = np.empty(Fo, np.int32)
    lib.flanhip_freeze_plan(num_frames, sample_rate, hop, tp, lp, n, src.ctypes.data_as(_vp))
    return src


def select_frames(pv, src_frames):
    """out[c][o] = pv[c][src_frames[o]], zero where src_frames[o] < 0 (the copy loops of PV::freeze)"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    src = np.ascontiguousarray(src_frames, np.int32)
    Fo = len(src)
    d_pv, d_src, d_out = DeviceArray(host=pv), DeviceArray(host=src), DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_select_frames_dev(_vp(d_pv.ptr), ch, F, bins, _vp(d_src.ptr), Fo, _vp(d_out.ptr), None))
    return d_out.to_host((ch, Fo, bins, 2))


def freeze(pv, sample_rate, hop, times, lengths):
    """PV::freeze"""
    return select_frames(pv, freeze_plan(np.shape(pv)[1], sample_rate, hop, times, lengths))


def cut_frames(pv, start, end):
    """PV::cut_frames; None for the null PV the reference returns"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    s, c = C.c_int32(0), C.c_int32(0)
    check(lib.flanhip_cut_frames_range(F, start, end, C.byref(s), C.byref(c)))
    if c.value <= 0:
        return None
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(ch * c.value * bins * 8)
    check(lib.flanhip_cut_frames_dev(_vp(d_pv.ptr), ch, F, bins, s.value, c.value, _vp(d_out.ptr), None))
    return d_out.to_host((ch, c.value, bins, 2))


def join(pvs):
    """PV::join: the format of the first input, the frames of all of them one after the other"""
    pvs = [np.ascontiguousarray(p, np.float32) for p in pvs]
    ch, _, bins, _ = pvs[0].shape
    Fo = sum(p.shape[1] for p in pvs)
    d_out = DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_memset(_vp(d_out.ptr), 0, ch * Fo * bins * 8, None))
    at = 0
    for p in pvs:
        d_in = DeviceArray(host=p)
        check(lib.flanhip_place_frames_dev(_vp(d_in.ptr), p.shape[0], p.shape[1], p.shape[2], _vp(d_out.ptr), ch, Fo, bins, at, None))
        check(lib.flanhip_stream_synchronize(None))
        at += p.shape[1]
    return d_out.to_host((ch, Fo, bins, 2))


def select(pv, sample_rate, hop, selector_tf):
    """PV::select.  selector_tf: float32 [out_frames][bins][2] = the selector sampled over the output's domain"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    sel = np.ascontiguousarray(selector_tf, np.float32)
    Fo = sel.shape[0]
    assert sel.shape == (Fo, bins, 2)
    d_pv, d_sel, d_out = DeviceArray(host=pv), DeviceArray(host=sel), DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_select_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, hop, _vp(d_sel.ptr), Fo, _vp(d_out.ptr), None))
    return d_out.to_host((ch, Fo, bins, 2))


def harmonic_scale(pv, sample_rate, series, mode):
    """PV::add_octaves (mode 0) / PV::add_harmonics (mode 1).  series: float32 [F][H]"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    series = np.ascontiguousarray(series, np.float32)
    assert series.ndim == 2 and series.shape[0] == F
    H = series.shape[1]
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(pv.nbytes)
    d_s = DeviceArray(host=series) if H else None
    check(lib.flanhip_harmonic_scale_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, _vp(d_s.ptr) if d_s else None, H, mode, _vp(d_out.ptr), None))
    return d_out.to_host(pv.shape)


def modify_out_frames(mod_tf, sample_rate, hop):
    mod = np.ascontiguousarray(mod_tf, np.float32)
    F, bins, _ = mod.shape
    return int(lib.flanhip_modify_out_frames(mod.ctypes.data_as(_vp), F, bins, sample_rate, hop))


def modify(pv, sample_rate, hop, mod_tf, in_f, interp=0, out_frames=None):
    """PV::modify.  mod_tf: float32 [F][bins][2] (seconds, Hz); in_f: float32 [ch][F][bins]"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    mod = np.ascontiguousarray(mod_tf, np.float32)
    in_f = np.ascontiguousarray(in_f, np.float32)
    assert mod.shape == (F, bins, 2) and in_f.shape == (ch, F, bins)
    Fo = modify_out_frames(mod, sample_rate, hop) if out_frames is None else out_frames
    if Fo <= 0:
        return None
    d_pv, d_mod, d_f, d_out = DeviceArray(host=pv), DeviceArray(host=mod), DeviceArray(host=in_f), DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_modify_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, hop, _vp(d_mod.ptr), _vp(d_f.ptr), interp, Fo, _vp(d_out.ptr), None))
    return d_out.to_host((ch, Fo, bins, 2))


def stretch_spline(pv, steps):
    """PV::stretch_spline.  steps: uint32 [F-1], every one >= 1"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    steps = np.ascontiguousarray(steps, np.uint32)
    assert steps.shape == (F - 1,)
    Fo = int(lib.flanhip_stretch_spline_out_frames(steps.ctypes.data_as(_vp), F))
    if Fo < 0:
        raise FlanHipError(-1, "flanhip_stretch_spline_out_frames: bad steps")
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(ch * Fo * bins * 8)
    check(lib.flanhip_stretch_spline_dev(_vp(d_pv.ptr), ch, F, bins, steps.ctypes.data_as(_vp), Fo, _vp(d_out.ptr), None))
    check(lib.flanhip_stream_synchronize(None))
    return d_out.to_host((ch, Fo, bins, 2))


def smear_time_plan(num_frames, num_bins, sample_rate, hop, smear):
    """(true_left, out_frames, dist_samples_2) of PV::smear_time for a smear grid float32 [F][bins] or a scalar"""
    left, Fo, half = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    if np.isscalar(smear):
        check(lib.flanhip_smear_time_plan(num_frames, num_bins, sample_rate, hop, None, float(smear), C.byref(left), C.byref(Fo), C.byref(half)))
    else:
        g = np.ascontiguousarray(smear, np.float32)
        assert g.shape == (num_frames, num_bins)
        check(lib.flanhip_smear_time_plan(num_frames, num_bins, sample_rate, hop, g.ctypes.data_as(_vp), 0.0, C.byref(left), C.byref(Fo), C.byref(half)))
    return left.value, Fo.value, half.value


def smear_time(pv, sample_rate, hop, smear, granularity, dist, true_left, out_frames):
    """PV::smear_time.  smear: float32 [F][bins] or scalar; granularity: int32 [F][bins] or scalar; dist: float32 [2 * dist_samples_2]"""
    pv = np.ascontiguousarray(pv, np.float32)
    ch, F, bins, _ = pv.shape
    s_ptr, s_const, _k1 = _grid_or_const(smear)
    if np.isscalar(granularity):
        g_ptr, g_const, _k2 = None, int(granularity), None
    else:
        _k2 = DeviceArray(host=np.ascontiguousarray(granularity, np.int32))
        g_ptr, g_const = _vp(_k2.ptr), 0
    dist = np.ascontiguousarray(dist, np.float32)
    d_dist = DeviceArray(host=dist) if len(dist) else None
    d_pv, d_out = DeviceArray(host=pv), DeviceArray(ch * out_frames * bins * 8)
    check(lib.flanhip_smear_time_dev(_vp(d_pv.ptr), ch, F, bins, sample_rate, hop, s_ptr, s_const, g_ptr, g_const,
                                     _vp(d_dist.ptr) if d_dist else None, len(dist), true_left, out_frames, _vp(d_out.ptr), None))
    return d_out.to_host((ch, out_frames, bins, 2))


# ---------------------------------------------------------------------------------------------------------------
# device-pointer wrappers: arguments are objects with .data_ptr() (torch tensors on the GPU) or raw ints
# ---------------------------------------------------------------------------------------------------------------

def _dp(t):
    if t is None:
        return None
    return _vp(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def analyze_dev(d_audio, ch, n, sample_rate, window, hop, dft, d_out, stream=None):
    check(lib.flanhip_analyze_dev(_dp(d_audio), ch, n, sample_rate, window, hop, dft, _dp(d_out), _vp(stream or 0)))


def analyze_dev_fused(d_audio, ch, n, sample_rate, window, hop, dft, d_out, d_ws, stream=None):
    check(lib.flanhip_analyze_dev_fused(_dp(d_audio), ch, n, sample_rate, window, hop, dft, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def synthesize_dev_fused(d_pv, ch, F, bins, sample_rate, analysis_rate, window, d_out, d_ws, d_nan=None, stream=None):
    check(lib.flanhip_synthesize_dev_fused(_dp(d_pv), ch, F, bins, sample_rate, analysis_rate, window, _dp(d_out), _dp(d_ws),
                                           _dp(d_nan), _vp(stream or 0)))


def synthesize_dev_stages(d_pv, ch, F, bins, sample_rate, analysis_rate, window, d_out, d_ws, d_nan, presummed, stages, stream=None):
    """flanhip_synthesize_dev (presummed 0) / _fused (1) / _fused_checked (2) with the kernels to launch as a per-call argument
    (1 k_phase_sums, 2 k_phase_scan, 4 k_synthesize, 8 k_ola_fixup): bench.py times one kernel at a time with it"""
    check(lib.flanhip_synthesize_dev_stages(_dp(d_pv), ch, F, bins, sample_rate, analysis_rate, window, _dp(d_out), _dp(d_ws),
                                            _dp(d_nan), presummed, stages, _vp(stream or 0)))


# flanhip_debug_option: per-thread test / A-B hooks (include/flanhip.h)
DEBUG_CHAIN_LEN, DEBUG_TARGET_CHAINS, DEBUG_FORCE_GENERIC, DEBUG_NO_FAST_DIV = 0, 1, 2, 3
DEBUG_ANA_VARIANT, DEBUG_SYN_VARIANT, DEBUG_ANA4096_OLD, DEBUG_SYN4096_OLD, DEBUG_RESAMPLE_DIRECT, DEBUG_FORCE_DIRECT, DEBUG_INLINE_FIXUP, DEBUG_WIDE_OFFSETS = 4, 5, 6, 7, 8, 9, 10, 11
_DEBUG_NAMES = {"chain_len": 0, "target_chains": 1, "force_generic": 2, "no_fast_div": 3, "ana_variant": 4, "syn_variant": 5,
                "ana4096_old": 6, "syn4096_old": 7, "resample_direct": 8, "force_direct": 9, "inline_fixup": 10, "wide_offsets": 11, "no_sub": 12}


class debug_options:
    """with fa.debug_options(chain_len=37): ...   -- the calling thread's hooks set for the block, cleared (0) afterwards"""

    def __init__(self, **kw):
        self.kw = {_DEBUG_NAMES[k]: int(v) for k, v in kw.items()}

    def __enter__(self):
        for k, v in self.kw.items():
            lib.flanhip_debug_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            lib.flanhip_debug_option(k, 0)
        return False


def synthesize_workspace_bytes(ch, F, bins, sample_rate, analysis_rate, window):
    return int(lib.flanhip_synthesize_workspace_bytes(ch, F, bins, sample_rate, analysis_rate, window))


def synthesize_dev(d_pv, ch, F, bins, sample_rate, analysis_rate, window, d_out, d_ws, d_nan=None, stream=None):
    check(lib.flanhip_synthesize_dev(_dp(d_pv), ch, F, bins, sample_rate, analysis_rate, window, _dp(d_out), _dp(d_ws),
                                     _dp(d_nan), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# the sliding-DFT vocoder (Audio::convert_to_SPV / SPV::convert_to_audio): one spectrum per input sample
# ---------------------------------------------------------------------------------------------------------------

def spv_analyze(audio, sample_rate, num_bins=1024):
    """Audio::convert_to_SPV.  audio float32 [ch][n] -> float32 [ch][n][num_bins][2] (m, f)."""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    out = np.empty((ch, n, num_bins, 2), np.float32)
    check(lib.flanhip_spv_analyze(_ptr(audio), ch, n, sample_rate, num_bins, _ptr(out), None))
    return out


def spv_synthesize(spv, sample_rate):
    """SPV::convert_to_audio.  spv float32 [ch][n][bins][2] -> float32 [ch][n]."""
    spv = np.ascontiguousarray(spv, np.float32)
    ch, n, bins, _ = spv.shape
    out = np.empty((ch, n), np.float32)
    check(lib.flanhip_spv_synthesize(_ptr(spv), ch, n, bins, sample_rate, _ptr(out), None))
    return out


def spv_twiddles(num_bins):
    """The analysis' twiddle table, float32 [2 num_bins][2] (re, im), computed on the host."""
    out = np.empty((2 * num_bins, 2), np.float32)
    check(lib.flanhip_spv_twiddles(num_bins, _ptr(out)))
    return out


def spv_analyze_dev(d_audio, ch, n, sample_rate, num_bins, d_out, stream=None):
    check(lib.flanhip_spv_analyze_dev(_dp(d_audio), ch, n, sample_rate, num_bins, _dp(d_out), _vp(stream or 0)))


def spv_synthesize_workspace_bytes(ch, n, num_bins, sample_rate):
    return int(lib.flanhip_spv_synthesize_workspace_bytes(ch, n, num_bins, sample_rate))


def spv_synthesize_dev(d_spv, ch, n, num_bins, sample_rate, d_out, d_ws, stream=None):
    check(lib.flanhip_spv_synthesize_dev(_dp(d_spv), ch, n, num_bins, sample_rate, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def spv_modify_frequency_const_dev(d_spv, ch, n, num_bins, value, multiply, d_out, stream=None):
    check(lib.flanhip_spv_modify_frequency_const_dev(_dp(d_spv), ch, n, num_bins, value, int(bool(multiply)), _dp(d_out), _vp(stream or 0)))


class spv_chain_length:
    """with fa.spv_chain_length(100): ...   -- frames per chain of this thread's SPV launches, back to the library's choice afterwards"""

    def __init__(self, frames):
        self.frames = int(frames)

    def __enter__(self):
        lib.flanhip_spv_debug_chain_length(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_spv_debug_chain_length(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# Audio::convolve: partitioned FFT convolution (the IR at the audio's sample rate)
# ---------------------------------------------------------------------------------------------------------------

def convolve_out_frames(n, m):
    return int(lib.flanhip_convolve_out_frames(n, m))


def convolve_partition(n, m):
    """The partition the library takes for an n-frame input and an m-frame IR (flanhip.h): the smallest of 512 ... 4096 with
    ceil(m / P) <= 32, else 4096.  (A forced partition, convolve_partition_forced, overrides it.)"""
    P = 512
    while P < 4096 and -(-m // P) > 32:
        P *= 2
    return P


def convolve(audio, ir, sample_rate, normalize=True):
    """Audio::convolve with both at one rate.  audio float32 [ch][n], ir float32 [ir_ch][m] -> float32 [ch][n + m]."""
    audio = np.ascontiguousarray(audio, np.float32)
    ir = np.ascontiguousarray(ir, np.float32)
    ch, n = audio.shape
    irch, m = ir.shape
    out = np.empty((ch, n + m), np.float32)
    check(lib.flanhip_convolve(_ptr(audio), ch, n, _ptr(ir), irch, m, sample_rate, int(bool(normalize)), _ptr(out), None))
    return out


def convolve_workspace_bytes(ch, n, ir_ch, m):
    return int(lib.flanhip_convolve_workspace_bytes(ch, n, ir_ch, m))


def convolve_dev(d_audio, ch, n, d_ir, ir_ch, m, sample_rate, normalize, d_out, d_ws, stream=None):
    check(lib.flanhip_convolve_dev(_dp(d_audio), ch, n, _dp(d_ir), ir_ch, m, sample_rate, int(bool(normalize)), _dp(d_out), _dp(d_ws),
                                   _vp(stream or 0)))


class convolve_partition_forced:
    """with fa.convolve_partition_forced(1024): ...   -- the partition of this thread's convolutions, back to the library's choice afterwards"""

    def __init__(self, samples):
        self.samples = int(samples)

    def __enter__(self):
        lib.flanhip_convolve_debug_partition(self.samples)
        return self

    def __exit__(self, *exc):
        lib.flanhip_convolve_debug_partition(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# Audio::repitch: variable-rate sinc resampling (inv_factors: the sampled factor already inverted and clamped)
# ---------------------------------------------------------------------------------------------------------------

REPITCH_SINC, REPITCH_LINEAR, REPITCH_UNINTERPOLATED = 0, 1, 2


def audio_repitch_out_frames(inv_factors, granularity_frames):
    inv = np.ascontiguousarray(inv_factors, np.float32)
    return int(lib.flanhip_audio_repitch_out_frames(_ptr(inv), inv.size, granularity_frames))


def _block_plan(fields, call, total_name):
    """A host plan's two calls: count the blocks, then fill one array per ( name, dtype ) of `fields`.  call( capacity, pointers, total )
    makes the C call (pointers: one per field, all None while counting; total: a reference to the int64 the plan also returns) and gives
    the number of blocks or an error code.  A dict of the arrays, and the total under `total_name`."""
    total = _i64(0)
    blocks = call(0, [None] * len(fields), C.byref(total))
    if blocks < 0:
        check(int(blocks))
    p = {name: np.empty(blocks, dtype) for name, dtype in fields}
    got = call(blocks, [_ptr(p[name]) for name, _ in fields], C.byref(total))
    assert got == blocks
    p[total_name] = int(total.value)
    return p


_PLAN_FIELDS = [("offset", np.int64), ("fracpos", np.float64), ("ratio", np.float64), ("filtpos", np.float64), ("oversize", np.int32),
                ("ideal", np.int32), ("first_out", np.int64)]


def audio_repitch_plan(num_frames, sample_rate, inv_factors, granularity_frames, quality=REPITCH_SINC):
    """The block loop on the host: a dict of per-block arrays (offset, fracpos, ratio, filtpos, oversize, ideal, first_out, wanted) and
    out_frames."""
    inv = np.ascontiguousarray(inv_factors, np.float32)
    return _block_plan(_PLAN_FIELDS + [("wanted", np.int32)], lambda capacity, pointers, total: lib.flanhip_audio_repitch_plan(
        num_frames, sample_rate, _ptr(inv), inv.size, granularity_frames, quality, capacity, *pointers, total), "out_frames")


def _run_table(fields, call):
    """A host planner's run table, in the two calls of _block_plan: call( capacity, pointers, channels_per_group, groups ) makes the C call
    and gives the number of runs or an error code.  A dict of one array per ( name, dtype ) of `fields`, channels_per_group and groups."""
    cpw, groups = _i32(0), _i64(0)
    runs = call(0, [None] * len(fields), C.byref(cpw), C.byref(groups))
    if runs < 0:
        check(int(runs))
    t = {name: np.empty(runs, dtype) for name, dtype in fields}
    got = call(runs, [_ptr(t[name]) for name, _ in fields], C.byref(cpw), C.byref(groups))
    assert got == runs
    t["channels_per_group"], t["groups"] = int(cpw.value), int(groups.value)
    return t


def audio_repitch_runs(num_frames, sample_rate, inv_factors, granularity_frames, num_channels, quality=REPITCH_SINC):
    """The runs the sinc launch cuts the plan into: a dict of per-run arrays (first_block, num_blocks, win_start, win_len; win_len 0: the
    taps come from global memory), channels_per_group and groups."""
    inv = np.ascontiguousarray(inv_factors, np.float32)
    fields = [("first_block", np.int64), ("num_blocks", np.int32), ("win_start", np.int64), ("win_len", np.int32)]
    return _run_table(fields, lambda capacity, pointers, cpw, groups: lib.flanhip_audio_repitch_runs(
        num_frames, sample_rate, _ptr(inv), inv.size, granularity_frames, quality, num_channels, capacity, *pointers, cpw, groups))


def audio_repitch_workspace_bytes(num_frames, sample_rate, inv_factors, granularity_frames, quality=REPITCH_SINC):
    inv = np.ascontiguousarray(inv_factors, np.float32)
    return int(lib.flanhip_audio_repitch_workspace_bytes(num_frames, sample_rate, _ptr(inv), inv.size, granularity_frames, quality))


def audio_repitch(audio, sample_rate, inv_factors, granularity_frames, quality=REPITCH_SINC):
    """Audio::repitch after the factor has been sampled, inverted and clamped.  audio float32 [ch][n] -> float32 [ch][out_frames]."""
    audio = np.ascontiguousarray(audio, np.float32)
    inv = np.ascontiguousarray(inv_factors, np.float32)
    ch, n = audio.shape
    out = np.empty((ch, max(audio_repitch_out_frames(inv, granularity_frames), 0)), np.float32)
    check(lib.flanhip_audio_repitch(_ptr(audio), ch, n, sample_rate, _ptr(inv), inv.size, granularity_frames, quality, _ptr(out), None))
    return out


def audio_repitch_dev(d_audio, ch, n, sample_rate, inv_factors, granularity_frames, quality, d_out, d_ws, stream=None):
    inv = np.ascontiguousarray(inv_factors, np.float32)
    check(lib.flanhip_audio_repitch_dev(_dp(d_audio), ch, n, sample_rate, _ptr(inv), inv.size, granularity_frames, quality, _dp(d_out),
                                        _dp(d_ws), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::compress / modify_volume / set_volume.  A compressor parameter is a float (the scalar) or an array of n floats (a curve)
# ---------------------------------------------------------------------------------------------------------------

COMPRESS_PARAMS = ("threshold", "ratio", "attack", "release", "knee_width")
COMPRESS_DEFAULTS = {"threshold": -20.0, "ratio": 3.0, "attack": 0.005, "release": 0.1, "knee_width": 0.0}


def compress_workspace_bytes(num_frames):
    return int(lib.flanhip_compress_workspace_bytes(num_frames))


def _compress_params(params, n, pointer):
    """the ten (curve, scalar) arguments in the header's order; curves are kept alive by the second return value"""
    unknown = set(params) - set(COMPRESS_PARAMS)
    if unknown:
        raise TypeError("unknown compressor parameters: %s" % sorted(unknown))
    args, keep = [], []
    for name in COMPRESS_PARAMS:
        v = params.get(name, COMPRESS_DEFAULTS[name])
        if isinstance(v, (int, float, np.floating)):
            args += [None, float(v)]
        else:
            if pointer is _ptr:
                v = np.ascontiguousarray(v, np.float32)
                assert v.shape == (n,), (name, v.shape)
            keep.append(v)
            args += [pointer(v), 0.0]
    return args, keep


def compress(audio, sample_rate, sidechain=None, want_gain=False, **params):
    """Audio::compress.  audio float32 [ch][n]; sidechain float32 [side_ch][side_n >= n] or None (the audio itself) -> float32 [ch][n],
    with want_gain also the gain curve float32 [n]."""
    audio = np.ascontiguousarray(audio, np.float32)
    side = audio if sidechain is None else np.ascontiguousarray(sidechain, np.float32)
    ch, n = audio.shape
    args, keep = _compress_params(params, n, _ptr)
    out = np.empty_like(audio)
    gain = np.empty(n, np.float32) if want_gain else None
    check(lib.flanhip_compress(_ptr(audio), ch, n, sample_rate, _ptr(side), side.shape[0], side.shape[1], *args, _ptr(out),
                               _ptr(gain) if want_gain else None, None))
    return (out, gain) if want_gain else out


def compress_dev(d_audio, ch, n, sample_rate, d_side, side_ch, side_n, d_out, d_gain_out, d_ws, stream=None, **params):
    """flanhip_compress_dev: parameters are floats or device arrays of n floats"""
    args, keep = _compress_params(params, n, _dp)
    check(lib.flanhip_compress_dev(_dp(d_audio), ch, n, sample_rate, _dp(d_side), side_ch, side_n, *args, _dp(d_out), _dp(d_gain_out),
                                   _dp(d_ws), _vp(stream or 0)))


class compress_run_forced:
    """with fa.compress_run_forced(3): ...   -- the frames one lane replays in this thread's compressions, back to the library's choice afterwards"""

    def __init__(self, frames):
        self.frames = frames

    def __enter__(self):
        lib.flanhip_compress_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_compress_debug_run(0)
        return False


def audio_gain_dev(d_audio, ch, n, gain, d_out, stream=None):
    """Audio::modify_volume: gain is a float or a device array of n floats"""
    scalar = isinstance(gain, (int, float, np.floating))
    check(lib.flanhip_audio_gain_dev(_dp(d_audio), ch, n, None if scalar else _dp(gain), float(gain) if scalar else 0.0, _dp(d_out),
                                     _vp(stream or 0)))


def audio_set_volume_workspace_bytes(ch, n):
    return int(lib.flanhip_audio_set_volume_workspace_bytes(ch, n))


def audio_set_volume_dev(d_audio, ch, n, sample_rate, level, d_out, d_ws, stream=None):
    """Audio::set_volume: level is a float or a device array of n floats"""
    scalar = isinstance(level, (int, float, np.floating))
    check(lib.flanhip_audio_set_volume_dev(_dp(d_audio), ch, n, sample_rate, None if scalar else _dp(level), float(level) if scalar else 0.0,
                                           _dp(d_out), _dp(d_ws), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::filter_1pole_lowpass / _highpass / _repeat_low / _repeat_high.  The cutoff is a float (the scalar) or an array of n floats (a curve)
# ---------------------------------------------------------------------------------------------------------------

FILTER_BUTTERWORTH_LOW, FILTER_BUTTERWORTH_HIGH, FILTER_REPEAT_LOW, FILTER_REPEAT_HIGH = 0, 1, 2, 3


def filter_1pole_workspace_bytes(ch, n):
    return int(lib.flanhip_filter_1pole_workspace_bytes(ch, n))


def filter_1pole(audio, sample_rate, cutoff, kind=FILTER_BUTTERWORTH_LOW, order=1):
    """Audio::filter_1pole_lowpass / _highpass (the Butterworth kinds, order N) and filter_1pole_repeat_low / _high (the repeat kinds,
    order = repeats).  audio float32 [ch][n] -> float32 [ch][n]."""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    scalar = isinstance(cutoff, (int, float, np.floating))
    curve = None if scalar else np.ascontiguousarray(cutoff, np.float32)
    assert scalar or curve.shape == (n,), curve.shape
    out = np.empty_like(audio)
    check(lib.flanhip_filter_1pole(_ptr(audio), ch, n, sample_rate, None if scalar else _ptr(curve), float(cutoff) if scalar else 0.0,
                                   kind, order, _ptr(out), None))
    return out


def filter_1pole_dev(d_audio, ch, n, sample_rate, cutoff, kind, order, d_out, d_ws, stream=None):
    """flanhip_filter_1pole_dev: cutoff is a float or a device array of n floats; d_out may be d_audio"""
    scalar = isinstance(cutoff, (int, float, np.floating))
    check(lib.flanhip_filter_1pole_dev(_dp(d_audio), ch, n, sample_rate, None if scalar else _dp(cutoff), float(cutoff) if scalar else 0.0,
                                       kind, order, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


class filter_run_forced:
    """with fa.filter_run_forced(3): ...   -- the frames one lane replays in this thread's filters, back to the library's choice afterwards"""

    def __init__(self, frames):
        self.frames = frames

    def __enter__(self):
        lib.flanhip_filter_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_filter_debug_run(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# Audio::filter_2pole_lowpass / _bandpass / _highpass / _notch, filter_2pole_lowshelf / _bandshelf / _highshelf and filter_1pole_lowshelf /
# _highshelf.  Cutoff, damping and gain are each a float (the scalar) or an array of n floats (a curve)
# ---------------------------------------------------------------------------------------------------------------

(FILTER2_1POLE_LOWSHELF, FILTER2_1POLE_HIGHSHELF, FILTER2_LOW, FILTER2_BAND, FILTER2_HIGH, FILTER2_NOTCH, FILTER2_LOWSHELF, FILTER2_BANDSHELF,
 FILTER2_HIGHSHELF) = range(9)


def filter2_workspace_bytes(ch, n):
    return int(lib.flanhip_filter2_workspace_bytes(ch, n))


def _filter2_params(values, n, pointer):
    """the six (curve, scalar) arguments in the header's order; curves are kept alive by the second return value"""
    args, keep = [], []
    for v in values:
        if isinstance(v, (int, float, np.floating)):
            args += [None, float(v)]
        else:
            if pointer is _ptr:
                v = np.ascontiguousarray(v, np.float32)
                assert v.shape == (n,), v.shape
            keep.append(v)
            args += [pointer(v), 0.0]
    return args, keep


def filter2(audio, sample_rate, cutoff, damping=1.0, gain=0.0, kind=FILTER2_LOW, order=1):
    """the nine filters of the FILTER2_* kinds.  audio float32 [ch][n] -> float32 [ch][n]."""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    args, keep = _filter2_params((cutoff, damping, gain), n, _ptr)
    out = np.empty_like(audio)
    check(lib.flanhip_filter2(_ptr(audio), ch, n, sample_rate, *args, kind, order, _ptr(out), None))
    return out


def filter2_dev(d_audio, ch, n, sample_rate, cutoff, damping, gain, kind, order, d_out, d_ws, stream=None):
    """flanhip_filter2_dev: cutoff, damping and gain are floats or device arrays of n floats; d_out may be d_audio (not for FILTER2_NOTCH)"""
    args, keep = _filter2_params((cutoff, damping, gain), n, _dp)
    check(lib.flanhip_filter2_dev(_dp(d_audio), ch, n, sample_rate, *args, kind, order, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::filter_comb.  Cutoff, feedback and wet_dry are each a float (the scalar) or an array of n floats (a curve)
# ---------------------------------------------------------------------------------------------------------------

def filter_comb_workspace_bytes(ch, n):
    return int(lib.flanhip_filter_comb_workspace_bytes(ch, n))


def filter_comb(audio, sample_rate, cutoff, feedback=0.0, wet_dry=0.5, invert=False, cancel=None):
    """Audio::filter_comb.  audio float32 [ch][n] -> float32 [ch][n].  cancel: None or a ctypes.c_int the call polls"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    args, keep = _filter2_params((cutoff, feedback, wet_dry), n, _ptr)
    out = np.empty_like(audio)
    check(lib.flanhip_filter_comb(_ptr(audio), ch, n, sample_rate, *args, int(bool(invert)), _ptr(out),
                                  None if cancel is None else C.cast(C.byref(cancel), _vp)))
    return out


class filter_comb_local_forced:
    """with fa.filter_comb_local_forced(-1): ...   -- the rounds this thread's comb calls run tile-local in LDS first (negative: none),
    back to the library's choice afterwards"""

    def __init__(self, rounds):
        self.rounds = rounds

    def __enter__(self):
        lib.flanhip_filter_comb_debug_local(self.rounds)
        return self

    def __exit__(self, *exc):
        lib.flanhip_filter_comb_debug_local(0)
        return False


def filter_comb_dev(d_audio, ch, n, sample_rate, cutoff, feedback, wet_dry, invert, d_out, d_ws, stream=None):
    """flanhip_filter_comb_dev: cutoff, feedback and wet_dry are floats or device arrays of n floats; d_out may be d_audio"""
    args, keep = _filter2_params((cutoff, feedback, wet_dry), n, _dp)
    check(lib.flanhip_filter_comb_dev(_dp(d_audio), ch, n, sample_rate, *args, int(bool(invert)), _dp(d_out), _dp(d_ws), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::filter_1pole_multinotch / filter_2pole_multinotch (use_saturator == false).  Cutoff, damping, feedback and wet_dry are each a float
# (the scalar) or an array of n floats (a curve); the 1-pole kind does not look at damping
# ---------------------------------------------------------------------------------------------------------------

MULTINOTCH_1POLE, MULTINOTCH_2POLE = range(2)


def multinotch_workspace_bytes(ch, n, kind, order):
    return int(lib.flanhip_multinotch_workspace_bytes(ch, n, kind, order))


def multinotch(audio, sample_rate, cutoff, damping=1.0, feedback=0.0, wet_dry=0.5, kind=MULTINOTCH_1POLE, order=1, invert=False, cancel=None):
    """the multinotch of a MULTINOTCH_* kind.  audio float32 [ch][n] -> float32 [ch][n].  cancel: None or a ctypes.c_int the call polls"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    args, keep = _filter2_params((cutoff, damping, feedback, wet_dry), n, _ptr)
    out = np.empty_like(audio)
    check(lib.flanhip_multinotch(_ptr(audio), ch, n, sample_rate, *args, kind, order, int(bool(invert)), _ptr(out),
                                 None if cancel is None else C.cast(C.byref(cancel), _vp)))
    return out


def multinotch_dev(d_audio, ch, n, sample_rate, cutoff, damping, feedback, wet_dry, kind, order, invert, d_out, d_ws, stream=None):
    """flanhip_multinotch_dev: the four parameters are floats or device arrays of n floats; d_out may be d_audio"""
    args, keep = _filter2_params((cutoff, damping, feedback, wet_dry), n, _dp)
    check(lib.flanhip_multinotch_dev(_dp(d_audio), ch, n, sample_rate, *args, kind, order, int(bool(invert)), _dp(d_out), _dp(d_ws), _vp(stream or 0)))


class multinotch_run_forced:
    """with fa.multinotch_run_forced(4): ...   -- the frames per team of this thread's multinotch calls, back to the library's choice afterwards"""

    def __init__(self, frames):
        self.frames = frames

    def __enter__(self):
        lib.flanhip_multinotch_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_multinotch_debug_run(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# hilbert_phase_diff_network, Audio::halfband_modulate, the modulation of Audio::shift_frequency and Audio::halfband_multiply.  The
# modulator's re and im are each a float (the scalar) or an array of n floats (a curve); a phase curve stands for both
# ---------------------------------------------------------------------------------------------------------------

def halfband_poles():
    """( first, second ): the poles of the two cascades in rad/s, float32 [10] each"""
    first, second = np.empty(10, np.float32), np.empty(10, np.float32)
    lib.flanhip_halfband_poles(_ptr(first), _ptr(second))
    return first, second


def halfband_workspace_bytes(ch, n):
    return int(lib.flanhip_halfband_workspace_bytes(ch, n))


def hilbert(audio, sample_rate):
    """hilbert_phase_diff_network.  audio float32 [ch][n] -> ( first, second ), float32 [ch][n] each"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    first, second = np.empty_like(audio), np.empty_like(audio)
    check(lib.flanhip_hilbert(_ptr(audio), ch, n, sample_rate, _ptr(first), _ptr(second), None))
    return first, second


def hilbert_dev(d_audio, ch, n, sample_rate, d_first, d_second, d_ws, stream=None):
    """flanhip_hilbert_dev: d_first or d_second may be d_audio"""
    check(lib.flanhip_hilbert_dev(_dp(d_audio), ch, n, sample_rate, _dp(d_first), _dp(d_second), _dp(d_ws), _vp(stream or 0)))


def _halfband_modulator(re, im, phase, n, pointer):
    """the five modulator arguments in the header's order; curves are kept alive by the second return value"""
    args, keep = _filter2_params((re, im), n, pointer)
    if phase is None:
        return args + [None], keep
    if pointer is _ptr:
        phase = np.ascontiguousarray(phase, np.float32)
        assert phase.shape == (n,), phase.shape
    return args + [pointer(phase)], keep + [phase]


def halfband_modulate(audio, sample_rate, re=1.0, im=0.0, phase=None):
    """Audio::halfband_modulate: first * re - second * im.  audio float32 [ch][n] -> float32 [ch][n]"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    args, keep = _halfband_modulator(re, im, phase, n, _ptr)
    out = np.empty_like(audio)
    check(lib.flanhip_halfband_modulate(_ptr(audio), ch, n, sample_rate, *args, _ptr(out), None))
    return out


def halfband_modulate_dev(d_audio, ch, n, sample_rate, re, im, phase, d_out, d_ws, stream=None):
    """flanhip_halfband_modulate_dev: re and im are floats or device arrays of n floats, phase None or a device array; d_out may be d_audio"""
    args, keep = _halfband_modulator(re, im, phase, n, _dp)
    check(lib.flanhip_halfband_modulate_dev(_dp(d_audio), ch, n, sample_rate, *args, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def halfband_multiply(a, sample_rate_a, b, sample_rate_b):
    """the network and the product of Audio::halfband_multiply.  a float32 [ch_a][n_a], b float32 [ch_b][n_b] -> float32 [min ch][min n]"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    out = np.empty((min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])), np.float32)
    check(lib.flanhip_halfband_multiply(_ptr(a), a.shape[0], a.shape[1], sample_rate_a, _ptr(b), b.shape[0], b.shape[1], sample_rate_b, _ptr(out), None))
    return out


def halfband_multiply_dev(d_a, ch_a, n_a, sample_rate_a, d_b, ch_b, n_b, sample_rate_b, d_out, d_ws, stream=None):
    """flanhip_halfband_multiply_dev: d_out float32 [min ch][min n]; the workspace is sized for the output's shape"""
    check(lib.flanhip_halfband_multiply_dev(_dp(d_a), ch_a, n_a, sample_rate_a, _dp(d_b), ch_b, n_b, sample_rate_b, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


class halfband_run_forced:
    """with fa.halfband_run_forced(4): ...   -- the frames one lane replays in this thread's halfband calls, back to the library's choice afterwards"""

    def __init__(self, frames):
        self.frames = frames

    def __enter__(self):
        lib.flanhip_halfband_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_halfband_debug_run(0)
        return False


# ---------------------------------------------------------------------------------------------------------------
# Audio::stereo_spatialize, pan, convert_to_stereo / convert_to_mono, combine_channels / split_channels
# ---------------------------------------------------------------------------------------------------------------

SPATIAL_LEFT, SPATIAL_RIGHT, SPATIAL_BOTH = 1, 2, 3
SPATIAL_GRANULARITY = 32


def _spatial_position(positions, pointer):
    """( pointer or None, x, y ): a pair is the constant position, an array [n][2] of doubles the sampled one"""
    if isinstance(positions, np.ndarray) and positions.ndim == 2 or hasattr(positions, "data_ptr"):
        return pointer(positions), 0.0, 0.0
    return None, float(positions[0]), float(positions[1])


def spatial_ear(audio, lowpassed, sample_rate, positions, head_width=0.18, ears=SPATIAL_BOTH):
    """head_ild + falloff.  audio, lowpassed float32 [n]; positions float64 [n][2] or a pair -> float32 [1 or 2][n], the left ear first"""
    audio, lowpassed = np.ascontiguousarray(audio, np.float32).reshape(-1), np.ascontiguousarray(lowpassed, np.float32).reshape(-1)
    if isinstance(positions, np.ndarray) and positions.ndim == 2:
        positions = np.ascontiguousarray(positions, np.float64)
    p, x, y = _spatial_position(positions, _ptr)
    out = np.empty((2 if ears == SPATIAL_BOTH else 1, audio.size), np.float32)
    check(lib.flanhip_spatial_ear(_ptr(audio), _ptr(lowpassed), 1, audio.size, sample_rate, p, x, y, head_width, ears, _ptr(out), None))
    return out


def spatial_ear_dev(d_audio, d_lowpassed, n, sample_rate, positions, head_width, ears, d_out, stream=None):
    p, x, y = _spatial_position(positions, _dp)
    check(lib.flanhip_spatial_ear_dev(_dp(d_audio), _dp(d_lowpassed), 1, n, sample_rate, p, x, y, head_width, ears, _dp(d_out), _vp(stream or 0)))


def spatial_delay_dev(d_audio, ears, n, delays, out_frames, out_stride, d_out, stream=None):
    delays, out_frames = np.ascontiguousarray(delays, np.float32), np.ascontiguousarray(out_frames, np.int64)
    check(lib.flanhip_spatial_delay_dev(_dp(d_audio), ears, n, _ptr(delays), _ptr(out_frames), out_stride, _dp(d_out), _vp(stream or 0)))


def spatial_itd_out_frames(num_frames, sample_rate, distances):
    """( output length, stretches ) from the distances at frames 0, 32, 64, ..."""
    d = np.ascontiguousarray(distances, np.float64)
    stretches = np.empty(d.size, np.float64)
    nout = int(lib.flanhip_spatial_itd_out_frames(num_frames, sample_rate, _ptr(d), d.size, _ptr(stretches)))
    if nout < 0:
        check(nout)
    return nout, stretches


def spatial_itd_plan(num_frames, sample_rate, stretches):
    """The block loop on the host: a dict of per-block arrays (offset, fracpos, ratio, filtpos, oversize, ideal, first_out, delivered,
    buffered) and total_out."""
    st = np.ascontiguousarray(stretches, np.float64)
    return _block_plan(_PLAN_FIELDS + [("delivered", np.int32), ("buffered", np.int32)], lambda capacity, pointers, total:
                       lib.flanhip_spatial_itd_plan(num_frames, sample_rate, _ptr(st), st.size, capacity, *pointers, total), "total_out")


def spatial_itd_workspace_bytes(num_frames, sample_rate, stretches):
    st = np.atleast_2d(np.ascontiguousarray(stretches, np.float64))
    return int(lib.flanhip_spatial_itd_workspace_bytes(st.shape[0], num_frames, sample_rate, _ptr(st), st.shape[1]))


def spatial_itd(audio, sample_rate, stretches, out_frames, out_stride=None):
    """head_itd for a moving source.  audio float32 [ears][n], stretches float64 [ears][ceil( n / 32 )], out_frames one per ear ->
    float32 [ears][out_stride] (out_stride: the longest ear unless given)"""
    audio = np.atleast_2d(np.ascontiguousarray(audio, np.float32))
    st = np.atleast_2d(np.ascontiguousarray(stretches, np.float64))
    nout = np.ascontiguousarray(np.atleast_1d(out_frames), np.int64)
    ears, n = audio.shape
    stride = int(out_stride if out_stride is not None else max(int(nout.max()), 1))
    out = np.empty((ears, stride), np.float32)
    check(lib.flanhip_spatial_itd(_ptr(audio), ears, n, sample_rate, _ptr(st), st.shape[1], _ptr(nout), stride, _ptr(out), None))
    return out


def spatial_itd_dev(d_audio, ears, n, sample_rate, stretches, out_frames, out_stride, d_out, d_ws, stream=None):
    st = np.atleast_2d(np.ascontiguousarray(stretches, np.float64))
    nout = np.ascontiguousarray(np.atleast_1d(out_frames), np.int64)
    check(lib.flanhip_spatial_itd_dev(_dp(d_audio), ears, n, sample_rate, _ptr(st), st.shape[1], _ptr(nout), out_stride, _dp(d_out), _dp(d_ws),
                                      _vp(stream or 0)))


def audio_pan(audio, pan):
    """Audio::pan_in_place.  audio float32 [2][n]; pan a float or float32 [n] -> float32 [2][n]"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    curve = None if np.isscalar(pan) else np.ascontiguousarray(pan, np.float32)
    out = np.empty_like(audio)
    check(lib.flanhip_audio_pan(_ptr(audio), ch, n, None if curve is None else _ptr(curve), 0.0 if curve is not None else float(pan), _ptr(out), None))
    return out


def audio_pan_dev(d_audio, ch, n, pan, d_out, stream=None):
    """pan: a float or a device array of n floats; d_out may be d_audio"""
    scalar = isinstance(pan, (int, float))
    check(lib.flanhip_audio_pan_dev(_dp(d_audio), ch, n, None if scalar else _dp(pan), float(pan) if scalar else 0.0, _dp(d_out), _vp(stream or 0)))


def audio_to_stereo_dev(d_audio, n, d_out, stream=None):
    check(lib.flanhip_audio_to_stereo_dev(_dp(d_audio), n, _dp(d_out), _vp(stream or 0)))


def audio_to_mono_dev(d_audio, ch, n, d_out, stream=None):
    check(lib.flanhip_audio_to_mono_dev(_dp(d_audio), ch, n, _dp(d_out), _vp(stream or 0)))


def audio_copy_rows_dev(d_src, src_stride, rows, src_frames, d_dst, dst_stride, dst_frames, stream=None):
    check(lib.flanhip_audio_copy_rows_dev(_dp(d_src), src_stride, rows, src_frames, _dp(d_dst), dst_stride, dst_frames, _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::get_local_wavelengths and its family (the YIN pitch tracker).  x is one channel row
# ---------------------------------------------------------------------------------------------------------------

def local_wavelengths_count(num_frames, start=0, end=-1, window=2048, hop=128):
    """the number of analysis windows; -1 for arguments the C ABI refuses as invalid"""
    return int(lib.flanhip_audio_local_wavelengths_count(num_frames, start, end, window, hop))


def local_wavelengths_workspace_bytes(num_frames, start=0, end=-1, window=2048, hop=128):
    return int(lib.flanhip_audio_local_wavelengths_workspace_bytes(num_frames, start, end, window, hop))


def yin_dprime_dev(d_x, num_frames, start, end, window, hop, d_dprime, stream=None):
    """d_dprime: float32 [count][window // 2] on the device"""
    check(lib.flanhip_audio_yin_dprime_dev(_dp(d_x), num_frames, start, end, window, hop, _dp(d_dprime), _vp(stream or 0)))


def yin_pick_dev(d_dprime, count, h, absolute_cutoff, minimum_wavelength, d_out, stream=None):
    check(lib.flanhip_audio_yin_pick_dev(_dp(d_dprime), count, h, absolute_cutoff, minimum_wavelength, _dp(d_out), _vp(stream or 0)))


def local_wavelengths_dev(d_x, num_frames, start, end, window, hop, absolute_cutoff, minimum_wavelength, d_out, d_ws, stream=None):
    """the raw per-window wavelengths (no continuity pass), one launch"""
    check(lib.flanhip_audio_local_wavelengths_dev(_dp(d_x), num_frames, start, end, window, hop, absolute_cutoff, minimum_wavelength,
                                                  _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def local_wavelength_dev(d_window, window, absolute_cutoff, minimum_wavelength, d_out, stream=None):
    check(lib.flanhip_audio_local_wavelength_dev(_dp(d_window), window, absolute_cutoff, minimum_wavelength, _dp(d_out), _vp(stream or 0)))


def local_wavelengths(x, sample_rate, start=0, end=-1, window=2048, hop=128, absolute_cutoff=0.2, minimum_wavelength=10, cancel=None):
    """Audio::get_local_wavelengths.  x float32 [n] -> float32 [count], continuity pass included.  cancel: None or a ctypes.c_int"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    count = local_wavelengths_count(x.size, start, end, window, hop)
    out = np.empty(max(count, 0), np.float32)
    check(lib.flanhip_audio_local_wavelengths(_ptr(x), x.size, sample_rate, start, end, window, hop, absolute_cutoff, minimum_wavelength,
                                              _ptr(out), None if cancel is None else C.cast(C.byref(cancel), _vp)))
    return out


def wavelength_continuity(w, sample_rate, hop):
    """the continuity pass of Audio::get_local_wavelengths on a copy of w"""
    out = np.array(w, np.float32).reshape(-1)
    check(lib.flanhip_wavelength_continuity(_ptr(out), out.size, sample_rate, hop))
    return out


def average_wavelength(locals_, min_active_ratio=0.0, max_length_sigma=-1.0):
    """Audio::get_average_wavelength( locals, ... )"""
    w = np.ascontiguousarray(locals_, np.float32).reshape(-1)
    out = C.c_float(0.0)
    check(lib.flanhip_average_wavelength(_ptr(w), w.size, min_active_ratio, max_length_sigma, C.cast(C.byref(out), _vp)))
    return np.float32(out.value)


# ---------------------------------------------------------------------------------------------------------------
# Audio::mix and the granular family (flan_amd/csrc/grains.hip): event tables are numpy records of GRAIN_EVENT
# ---------------------------------------------------------------------------------------------------------------

GRAIN_HANN = 1
GRAIN_EVENT = np.dtype([("src", np.uint64), ("ch_stride", np.int64), ("src_frames", np.int64), ("o", np.int64), ("gain_offset", np.int64),
                        ("s", np.int32), ("n", np.int32), ("channels", np.int32), ("sf", np.int32), ("ef", np.int32), ("flags", np.int32),
                        ("gain", np.float32), ("reserved", np.int32)], align=True)      # flanhip_grain_event, 72 bytes


def grains_tile_frames():
    return int(lib.flanhip_grains_tile_frames())


def grains_batch_events():
    return int(lib.flanhip_grains_batch_events())


def _curve(v, n):
    """( pointer or None, scalar ) of a curve of n floats or a number; the array is returned to keep it alive"""
    if np.ndim(v) == 0:
        return None, None, float(v)
    a = np.ascontiguousarray(v, np.float32).reshape(-1)
    assert a.size == n
    return a, _ptr(a), 0.0


def grains_events(length_frames, sample_rate, rate, scatter=0.0, seed=0):
    """integrate_event_rate: the event frames (int64).  rate / scatter: a number or length_frames floats"""
    _r, rp, rs = _curve(rate, length_frames)
    _s, sp, ss = _curve(scatter, length_frames)
    out = np.empty(max(int(length_frames), 0), np.int64)
    count = _i64(0)
    check(lib.flanhip_grains_events(length_frames, sample_rate, rp, rs, sp, ss, seed, _ptr(out), out.size, C.cast(C.byref(count), _vp)))
    return out[:count.value].copy()


def grains_cut(num_frames, sample_rate, start_time, end_time, start_fade, end_fade, events=None):
    """Audio::cut for a table of grains: s, n, sf, ef of the events (a fresh zeroed table unless one is given)"""
    a = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (start_time, end_time, start_fade, end_fade)]
    events = np.zeros(a[0].size, GRAIN_EVENT) if events is None else events
    check(lib.flanhip_grains_cut(num_frames, sample_rate, a[0].size, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(events)))
    return events


def grains_cut_frames(num_frames, start, end, start_fade, end_fade, events=None):
    a = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in (start, end, start_fade, end_fade)]
    events = np.zeros(a[0].size, GRAIN_EVENT) if events is None else events
    check(lib.flanhip_grains_cut_frames(num_frames, a[0].size, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(events)))
    return events


def grains_plan(events, out_frames=0):
    """( out_frames, tile_first, tile_last ) of an event table; out_frames 0: the reference's length, max( o + n )"""
    events = np.ascontiguousarray(events, GRAIN_EVENT)
    frames = _i64(out_frames)
    check(lib.flanhip_grains_plan(_ptr(events), events.size, C.cast(C.byref(frames), _vp), None, None, 0))
    tiles = -(-frames.value // grains_tile_frames())
    first, last = np.empty(tiles, np.int32), np.empty(tiles, np.int32)
    check(lib.flanhip_grains_plan(_ptr(events), events.size, C.cast(C.byref(frames), _vp), _ptr(first), _ptr(last), tiles))
    return frames.value, first, last


def grains_workspace_bytes(count, out_frames):
    return int(lib.flanhip_grains_workspace_bytes(count, out_frames))


def grains_mix_dev(events, tile_first, tile_last, d_gains, gain_floats, d_sources, sources_floats, num_channels, out_frames, sample_rate, d_out, d_ws,
                   stream=None):
    """events and the plan are host arrays; gains, sources, the output and the workspace live on the device"""
    events = np.ascontiguousarray(events, GRAIN_EVENT)
    first, last = np.ascontiguousarray(tile_first, np.int32), np.ascontiguousarray(tile_last, np.int32)
    check(lib.flanhip_grains_mix_dev(_ptr(events), events.size, _ptr(first), _ptr(last), first.size, _dp(d_gains), gain_floats, _dp(d_sources),
                                     sources_floats, num_channels, out_frames, sample_rate, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def grains_mix(events, gains, sources, num_channels, out_frames, sample_rate, cancel=None):
    """Audio::mix over host arrays: sources float32 (flat; the events' src are offsets into it) -> float32 [num_channels][out_frames]"""
    events = np.ascontiguousarray(events, GRAIN_EVENT)
    sources = np.ascontiguousarray(sources, np.float32).reshape(-1)
    gains = None if gains is None else np.ascontiguousarray(gains, np.float32).reshape(-1)
    out = np.full((num_channels, max(out_frames, 0)), np.nan, np.float32)
    check(lib.flanhip_grains_mix(_ptr(events), events.size, None if gains is None else _ptr(gains), 0 if gains is None else gains.size,
                                 _ptr(sources), sources.size, num_channels, out_frames, sample_rate, _ptr(out),
                                 None if cancel is None else C.cast(C.byref(cancel), _vp)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# flan::Wavetable: waveform starts and table index on the host, table construction, synthesis and the in-place edits on the device
# ---------------------------------------------------------------------------------------------------------------

WT_SNAP_NONE, WT_SNAP_ZERO, WT_SNAP_LEVEL = 0, 1, 2
WT_PITCH_NONE, WT_PITCH_LOCAL, WT_PITCH_GLOBAL = 0, 1, 2
WT_NORMALIZE, WT_REMOVE_DC, WT_ADD_FADES, WT_REMOVE_JUMPS = 0, 1, 2, 3


def wavetable_snap(row, frame_to_snap, snap_height, search_distance):
    row = np.ascontiguousarray(row, np.float32)
    out = _i32(0)
    check(lib.flanhip_wavetable_snap(_ptr(row), row.size, frame_to_snap, snap_height, search_distance, C.cast(C.byref(out), _vp)))
    return out.value


def wavetable_starts(row, local_wavelengths, global_wavelength, snap_mode, pitch_mode, snap_ratio, fixed_frame):
    """the walk of get_waveform_starts for one channel: int32 starts"""
    row = np.ascontiguousarray(row, np.float32)
    loc = np.ascontiguousarray([] if local_wavelengths is None else local_wavelengths, np.float32)
    count = _i64(0)
    args = (_ptr(row), row.size, _ptr(loc), loc.size, global_wavelength, snap_mode, pitch_mode, snap_ratio, fixed_frame, None)
    check(lib.flanhip_wavetable_starts(*args, None, 0, C.cast(C.byref(count), _vp)))
    out = np.empty(count.value, np.int32)
    check(lib.flanhip_wavetable_starts(*args, _ptr(out), out.size, C.cast(C.byref(count), _vp)))
    assert count.value == out.size
    return out


def wavetable_table_index(starts, num_source_frames, ratio):
    starts = np.ascontiguousarray(starts, np.int32)
    r = np.ascontiguousarray(ratio, np.float32)
    out = np.empty(r.shape, np.float32)
    check(lib.flanhip_wavetable_table_index(_ptr(starts), starts.size, num_source_frames, _ptr(r), r.size, _ptr(out)))
    return out


def _wt_starts(starts):
    """a list of per-channel start lists -> ( the int32 lists one after another, int64 counts )"""
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32).reshape(-1) for s in starts]), np.int32)
    return flat, np.array([len(s) for s in starts], np.int64)


def wavetable_slots(starts):
    _, counts = _wt_starts(starts)
    return int(lib.flanhip_wavetable_slots(_ptr(counts), counts.size))


def wavetable_resample_workspace_bytes(ch, n, starts, wavelength):
    flat, counts = _wt_starts(starts)
    return int(lib.flanhip_wavetable_resample_workspace_bytes(ch, n, _ptr(flat), _ptr(counts), wavelength))


def wavetable_resample(audio, starts, wavelength, want_rotations=True):
    """resample_waveforms.  audio float32 [ch][n], starts: one list per channel -> ( float32 [ch][slots * W], int32 [ch][slots] )"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    flat, counts = _wt_starts(starts)
    slots = int(counts.max())
    table = np.full((ch, slots * wavelength), np.nan, np.float32)
    rot = np.full((ch, slots), -1, np.int32)
    check(lib.flanhip_wavetable_resample(_ptr(audio), ch, n, _ptr(flat), _ptr(counts), wavelength, _ptr(table), _ptr(rot) if want_rotations else None, None))
    return table, rot


def wavetable_resample_dev(d_audio, ch, n, starts, wavelength, d_table, d_rot, d_ws, stream=None):
    flat, counts = _wt_starts(starts)
    check(lib.flanhip_wavetable_resample_dev(_dp(d_audio), ch, n, _ptr(flat), _ptr(counts), wavelength, _dp(d_table), _dp(d_rot), _dp(d_ws), _vp(stream or 0)))


def wavetable_synth_plan(out_frames, sample_rate, wavelength, granularity_frames, freq):
    """The resampler's block loop on the host: a dict of per-block arrays (offset, fracpos, ratio, filtpos, oversize, ideal, first_out, num_out,
    wanted, in_start)"""
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    fields = _PLAN_FIELDS + [("num_out", np.int32), ("wanted", np.int32), ("in_start", np.int64)]
    return _block_plan(fields, lambda capacity, pointers, total: lib.flanhip_wavetable_synth_plan(
        out_frames, sample_rate, wavelength, granularity_frames, _ptr(f), f.size, capacity, *pointers), "unused")


def wavetable_synth_runs(out_frames, sample_rate, wavelength, granularity_frames, freq, num_channels):
    """The runs the synthesis launch cuts the plan into: a dict of per-run arrays (first_out, num_out, first_block, num_blocks, j0, win_start,
    win_len), channels_per_group and groups."""
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    fields = [("first_out", np.int64), ("num_out", np.int32), ("first_block", np.int64), ("num_blocks", np.int32), ("j0", np.int64),
              ("win_start", np.int64), ("win_len", np.int32)]
    return _run_table(fields, lambda capacity, pointers, cpw, groups: lib.flanhip_wavetable_synth_runs(
        out_frames, sample_rate, wavelength, granularity_frames, _ptr(f), f.size, num_channels, capacity, *pointers, cpw, groups))


def wavetable_synth_workspace_bytes(ch, out_frames, sample_rate, wavelength, granularity_frames, freq):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    return int(lib.flanhip_wavetable_synth_workspace_bytes(ch, out_frames, sample_rate, wavelength, granularity_frames, _ptr(f), f.size))


def wavetable_synth(table, wavelength, sample_rate, out_frames, granularity_frames, freq, index, smooth=True):
    """Wavetable::synthesize after its Functions have been sampled.  table float32 [ch][slots * W], index float32 [ch][blocks] ->
    float32 [ch][out_frames]"""
    table = np.ascontiguousarray(table, np.float32)
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    index = np.ascontiguousarray(index, np.float32)
    ch = table.shape[0]
    slots = table.shape[1] // wavelength
    out = np.full((ch, out_frames), np.nan, np.float32)
    check(lib.flanhip_wavetable_synth(_ptr(table), ch, slots, wavelength, sample_rate, out_frames, granularity_frames, _ptr(f), f.size,
                                      _ptr(index), index.shape[-1] if index.ndim > 1 else index.size // ch, int(smooth), _ptr(out), None))
    return out


def wavetable_synth_dev(d_table, ch, slots, wavelength, sample_rate, out_frames, granularity_frames, freq, index, smooth, d_out, d_ws, stream=None):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    index = np.ascontiguousarray(index, np.float32)
    check(lib.flanhip_wavetable_synth_dev(_dp(d_table), ch, slots, wavelength, sample_rate, out_frames, granularity_frames, _ptr(f), f.size,
                                          _ptr(index), index.size // ch, int(smooth), _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def wavetable_edit(table, wavelength, mode, fade_frames=0):
    """the in-place edits on a copy: float32 [ch][slots * W] -> the edited table"""
    out = np.array(table, np.float32, order="C")
    ch = out.shape[0]
    check(lib.flanhip_wavetable_edit(_ptr(out), ch, out.shape[1] // wavelength, wavelength, mode, fade_frames, None))
    return out


def wavetable_edit_dev(d_table, ch, slots, wavelength, mode, fade_frames=0, stream=None):
    check(lib.flanhip_wavetable_edit_dev(_dp(d_table), ch, slots, wavelength, mode, fade_frames, _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio::synthesize_spectrum: bins, phases and channel jumps on the host; the table (one large inverse real FFT), the resampler loop over
# it and the whole call on the device
# ---------------------------------------------------------------------------------------------------------------

def spectrum_bins(spectrum_size_power, fundamental_power):
    """( int32 harmonic[B], float32 freq[B] ): the per-bin harmonic number and bin_to_frequency, B = 2^(p-1) + 1"""
    bins = int(lib.flanhip_spectrum_bins(spectrum_size_power, fundamental_power, None, None, 0))
    harmonic, freq = np.empty(bins, np.int32), np.empty(bins, np.float32)
    assert lib.flanhip_spectrum_bins(spectrum_size_power, fundamental_power, _ptr(harmonic), _ptr(freq), bins) == bins
    return harmonic, freq


def spectrum_num_harmonics(fundamental_power):
    return int(lib.flanhip_spectrum_num_harmonics(fundamental_power))


def spectrum_phases(seed, harmonic):
    """one mt19937( seed ) draw in [0, 2 pi) per bin with a harmonic, in ascending bin order; 0 elsewhere"""
    harmonic = np.ascontiguousarray(harmonic, np.int32)
    theta = np.empty(harmonic.size, np.float32)
    check(lib.flanhip_spectrum_phases(seed, _ptr(harmonic), harmonic.size, _ptr(theta)))
    return theta


def spectrum_jump(channel, num_channels, spectrum_size_power):
    return int(lib.flanhip_spectrum_jump(channel, num_channels, spectrum_size_power))


def spectrum_table_workspace_bytes(spectrum_size_power):
    return int(lib.flanhip_spectrum_table_workspace_bytes(spectrum_size_power))


def spectrum_table(mag, theta, spectrum_size_power):
    """float32 mag[B], theta[B] -> float32 table[2^p]: the unnormalised c2r of polar( mag, theta )"""
    mag, theta = np.ascontiguousarray(mag, np.float32), np.ascontiguousarray(theta, np.float32)
    bins = (1 << max(spectrum_size_power - 1, 0)) + 1
    if mag.size != bins or theta.size != bins:
        raise ValueError("mag and theta must hold 2^(p-1) + 1 bins")
    table = np.full(1 << spectrum_size_power, np.nan, np.float32)
    check(lib.flanhip_spectrum_table(_ptr(mag), _ptr(theta), spectrum_size_power, _ptr(table), None))
    return table


def spectrum_table_dev(d_mag, d_theta, spectrum_size_power, d_table, d_ws, stream=None):
    check(lib.flanhip_spectrum_table_dev(_dp(d_mag), _dp(d_theta), spectrum_size_power, _dp(d_table), _dp(d_ws), _vp(stream or 0)))


def spectrum_synth_plan(out_frames, rate_out, granularity_frames, freq):
    """The resampler's block loop on the host, as wavetable_synth_plan gives it"""
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    fields = _PLAN_FIELDS + [("num_out", np.int32), ("wanted", np.int32), ("in_start", np.int64)]
    return _block_plan(fields, lambda capacity, pointers, total: lib.flanhip_spectrum_synth_plan(
        out_frames, rate_out, granularity_frames, _ptr(f), f.size, capacity, *pointers), "unused")


def spectrum_synth_workspace_bytes(table_size_power, rate_out, ch, out_frames, granularity_frames, freq):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    return int(lib.flanhip_spectrum_synth_workspace_bytes(table_size_power, rate_out, ch, out_frames, granularity_frames, _ptr(f), f.size))


def spectrum_synth(table, rate_out, num_channels, out_frames, granularity_frames, freq):
    """the loop of Audio::synthesize_spectrum over one table row of 2^p frames -> float32 [num_channels][out_frames]"""
    table = np.ascontiguousarray(table, np.float32).reshape(-1)
    power = int(table.size).bit_length() - 1
    if table.size != 1 << power:
        raise ValueError("the table must hold a power of two of frames")
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    out = np.full((max(num_channels, 0), max(out_frames, 0)), np.nan, np.float32)
    check(lib.flanhip_spectrum_synth(_ptr(table), power, rate_out, num_channels, out_frames, granularity_frames, _ptr(f), f.size, _ptr(out), None))
    return out


def spectrum_synth_dev(d_table, table_size_power, rate_out, ch, out_frames, granularity_frames, freq, d_out, d_ws, stream=None):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    check(lib.flanhip_spectrum_synth_dev(_dp(d_table), table_size_power, rate_out, ch, out_frames, granularity_frames, _ptr(f), f.size, _dp(d_out),
                                         _dp(d_ws), _vp(stream or 0)))


def audio_synthesize_spectrum_workspace_bytes(spectrum_size_power, fundamental_power, ch, out_frames, granularity_frames, freq):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    return int(lib.flanhip_audio_synthesize_spectrum_workspace_bytes(spectrum_size_power, fundamental_power, ch, out_frames, granularity_frames,
                                                                     _ptr(f), f.size))


def audio_synthesize_spectrum(mag, theta, spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq):
    """Audio::synthesize_spectrum after its Functions have been sampled: table, loop, set_volume( 1 ) -> float32 [num_channels][out_frames]"""
    mag, theta = np.ascontiguousarray(mag, np.float32), np.ascontiguousarray(theta, np.float32)
    bins = (1 << max(spectrum_size_power - 1, 0)) + 1
    if mag.size != bins or theta.size != bins:
        raise ValueError("mag and theta must hold 2^(p-1) + 1 bins")
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    out = np.full((max(num_channels, 0), max(out_frames, 0)), np.nan, np.float32)
    check(lib.flanhip_audio_synthesize_spectrum(_ptr(mag), _ptr(theta), spectrum_size_power, fundamental_power, num_channels, out_frames,
                                                granularity_frames, _ptr(f), f.size, _ptr(out), None))
    return out


def audio_synthesize_spectrum_dev(d_mag, d_theta, spectrum_size_power, fundamental_power, ch, out_frames, granularity_frames, freq, d_out, d_ws,
                                  stream=None):
    f = np.ascontiguousarray(freq, np.float32).reshape(-1)
    check(lib.flanhip_audio_synthesize_spectrum_dev(_dp(d_mag), _dp(d_theta), spectrum_size_power, fundamental_power, ch, out_frames,
                                                    granularity_frames, _ptr(f), f.size, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


# ---------------------------------------------------------------------------------------------------------------
# Audio silence removal and slicing (flan_amd/csrc/temporal.hip): the loud-chunk scan, reverse and the host plans
# ---------------------------------------------------------------------------------------------------------------

def loud_workspace_bytes(ch, n):
    return int(lib.flanhip_loud_workspace_bytes(ch, n))


def loud_run_frames():
    return int(lib.flanhip_loud_run_frames())


def loud_block_frames():
    return int(lib.flanhip_loud_block_frames())


def loud_carry_pass_blocks():
    return int(lib.flanhip_loud_carry_pass_blocks())


class loud_run_forced:
    """with loud_run_forced(frames): the detection's kernels give every lane `frames` frames (1 ... 64) -- a test hook"""

    def __init__(self, frames):
        self.frames = int(frames)

    def __enter__(self):
        lib.flanhip_loud_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_loud_debug_run(0)
        return False


def loud_summary_dev(d_audio, ch, n, level, gap_frames, d_summary, d_ws, stream=None):
    check(lib.flanhip_loud_summary_dev(_dp(d_audio), ch, n, level, gap_frames, _dp(d_summary), _dp(d_ws), _vp(stream or 0)))


def loud_chunks_dev(ch, n, gap_frames, count, d_chunks, capacity, d_ws, stream=None):
    check(lib.flanhip_loud_chunks_dev(ch, n, gap_frames, count, _dp(d_chunks), capacity, _dp(d_ws), _vp(stream or 0)))


def loud_chunks(audio, level, gap_frames, cancel=None):
    """get_loud_chunks_base's chunk frames: audio float32 [ch][n] -> ( int32 [count][2], summary int64[4] )"""
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    cancel_p = None if cancel is None else C.cast(C.byref(cancel), _vp)
    summary = np.full(4, -7, np.int64)
    bound = n if gap_frames < 0 else (n - 1) // (gap_frames + 2) + 1      # one call: a table no count exceeds (chunk starts lie gap + 2 apart)
    chunks = np.full((bound, 2), -7, np.int32)
    check(lib.flanhip_loud_chunks(_ptr(audio), ch, n, level, gap_frames, _ptr(chunks), bound, _ptr(summary), cancel_p))
    assert np.all(chunks[int(summary[0]):] == -7)
    return chunks[:int(summary[0])].copy(), summary


def audio_reverse(audio, cancel=None):
    audio = np.ascontiguousarray(audio, np.float32)
    ch, n = audio.shape
    out = np.full((ch, n), np.nan, np.float32)
    check(lib.flanhip_audio_reverse(_ptr(audio), ch, n, _ptr(out), None if cancel is None else C.cast(C.byref(cancel), _vp)))
    return out


def audio_reverse_dev(d_audio, ch, n, d_out, stream=None):
    check(lib.flanhip_audio_reverse_dev(_dp(d_audio), ch, n, _dp(d_out), _vp(stream or 0)))


def loud_chunks_fades(num_frames, sample_rate, chunks, fade_in_time, join=False):
    """( events, offsets ) of get_loud_chunks_base's cuts; join: the events' o as remove_silence places them"""
    chunks = np.ascontiguousarray(chunks, np.int32).reshape(-1, 2)
    events = np.zeros(chunks.shape[0], GRAIN_EVENT)
    events["gain_offset"], events["gain"] = -1, 1.0
    offsets = np.full(chunks.shape[0] + 1, np.nan, np.float32)
    check(lib.flanhip_loud_chunks_fades(num_frames, sample_rate, _ptr(chunks), chunks.shape[0], fade_in_time, 1 if join else 0, _ptr(events), _ptr(offsets)))
    return events, offsets


def edge_silence_cut(num_frames, sample_rate, first_noisy, last_noisy, fade_time):
    out = np.zeros(4, np.int32)
    check(lib.flanhip_edge_silence_cut(num_frames, sample_rate, first_noisy, last_noisy, fade_time, _ptr(out)))
    return tuple(int(v) for v in out)


def split_frames(num_frames, sample_rate, times):
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    out = np.zeros(times.size + 2, np.int32)
    count = _i64(0)
    check(lib.flanhip_split_frames(num_frames, sample_rate, _ptr(times), times.size, _ptr(out), out.size, C.cast(C.byref(count), _vp)))
    return out[:count.value].copy()


def rearrange_order(count, seed):
    out = np.zeros(max(count, 0), np.int32)
    check(lib.flanhip_rearrange_order(count, seed, _ptr(out)))
    return out


def random_chunks_frames(sample_rate, length):
    return int(lib.flanhip_random_chunks_frames(sample_rate, length))


def random_chunks_plan(num_frames, sample_rate, length, chunk_length, fade, seed):
    """( events, chunk_starts, offsets ); chunk_length: a number or random_chunks_frames() floats, fade: a number or one float more"""
    frames = random_chunks_frames(sample_rate, length)
    _c, cp, cs = _curve(chunk_length, frames)
    _f, fp, fs = _curve(fade, frames + 1)
    count = _i64(0)
    check(lib.flanhip_random_chunks_plan(num_frames, sample_rate, length, cp, cs, fp, fs, seed, None, None, None, 0, C.cast(C.byref(count), _vp)))
    events = np.zeros(count.value, GRAIN_EVENT)
    events["gain_offset"], events["gain"] = -1, 1.0
    starts, offsets = np.zeros(count.value, np.int32), np.zeros(count.value + 1, np.float32)
    check(lib.flanhip_random_chunks_plan(num_frames, sample_rate, length, cp, cs, fp, fs, seed, _ptr(events), _ptr(starts), _ptr(offsets), count.value,
                                         C.cast(C.byref(count), _vp)))
    return events, starts, offsets


# ---------------------------------------------------------------------------------------------------------------
# Audio volume, waveforms, the oscillator and the energies (flan_amd/csrc/volume.hip).  Curves are floats or device arrays
# ---------------------------------------------------------------------------------------------------------------

WAVEFORM_SINE, WAVEFORM_SQUARE, WAVEFORM_SAW, WAVEFORM_TRIANGLE = 0, 1, 2, 3


def _dev_curve(v):
    """( device pointer or None, scalar ) of a float or a device array"""
    scalar = isinstance(v, (int, float, np.floating))
    return (None, float(v)) if scalar else (_dp(v), 0.0)


def audio_ring_modulate_dev(d_audio, ch, n, d_other, other_ch, other_n, d_out, stream=None):
    check(lib.flanhip_audio_ring_modulate_dev(_dp(d_audio), ch, n, _dp(d_other), other_ch, other_n, _dp(d_out), _vp(stream or 0)))


def fade_frames_plan(num_frames, start, end):
    """fade_frames_in_place's validation: ( start, end ) after the clamp at 0 and the proportional shrink"""
    out = np.zeros(2, np.int32)
    check(lib.flanhip_fade_frames_plan(num_frames, start, end, _ptr(out)))
    return int(out[0]), int(out[1])


def audio_fade_dev(d_audio, ch, n, d_start_gain, start, d_end_gain, end, d_out, stream=None):
    check(lib.flanhip_audio_fade_dev(_dp(d_audio), ch, n, _dp(d_start_gain), start, _dp(d_end_gain), end, _dp(d_out), _vp(stream or 0)))


def waveform_dev(kind, d_t, count, d_out, stream=None):
    check(lib.flanhip_waveform_dev(kind, _dp(d_t), count, _dp(d_out), _vp(stream or 0)))


def waveform_host(kind, t):
    t = np.ascontiguousarray(t, np.float32).reshape(-1)
    out = np.empty_like(t)
    check(lib.flanhip_waveform_host(kind, _ptr(t), t.size, _ptr(out)))
    return out


def audio_moisture_dev(d_over, ch, n_over, over_rate, n, sample_rate, amount, frequency, skew, kind, d_out, stream=None):
    """add_moisture's shaper over the oversampled block; amount, frequency, skew: floats or device arrays of n floats"""
    (ap, a), (fp, f), (kp, k) = _dev_curve(amount), _dev_curve(frequency), _dev_curve(skew)
    check(lib.flanhip_audio_moisture_dev(_dp(d_over), ch, n_over, over_rate, n, sample_rate, ap, a, fp, f, kp, k, kind, _dp(d_out), _vp(stream or 0)))


def audio_energy_workspace_bytes(ch, n):
    return int(lib.flanhip_audio_energy_workspace_bytes(ch, n))


def audio_energy_dev(d_audio, ch, n, d_energy, d_ws, stream=None):
    check(lib.flanhip_audio_energy_dev(_dp(d_audio), ch, n, _dp(d_energy), _dp(d_ws), _vp(stream or 0)))


def audio_rectify_dev(d_audio, ch, n, d_out, stream=None):
    check(lib.flanhip_audio_rectify_dev(_dp(d_audio), ch, n, _dp(d_out), _vp(stream or 0)))


def synthesize_waveform_frames(length, sample_rate, oversample):
    """( output frames, input frames, input rate ) of synthesize_waveform, or None where it returns a null Audio"""
    n_in, rate = _i64(0), C.c_double(0)
    n = int(lib.flanhip_synthesize_waveform_frames(length, sample_rate, oversample, C.cast(C.byref(n_in), _vp), C.cast(C.byref(rate), _vp)))
    return None if n < 0 else (n, int(n_in.value), float(rate.value))


def osc_workspace_bytes(n_in):
    return int(lib.flanhip_osc_workspace_bytes(n_in))


def osc_run_frames():
    return int(lib.flanhip_osc_run_frames())


def osc_block_frames():
    return int(lib.flanhip_osc_block_frames())


def osc_carry_pass_blocks():
    return int(lib.flanhip_osc_carry_pass_blocks())


class osc_run_forced:
    """with osc_run_forced(frames): the oscillator's scan gives every lane `frames` frames (1 ... 64) -- a test hook"""

    def __init__(self, frames):
        self.frames = int(frames)

    def __enter__(self):
        lib.flanhip_osc_debug_run(self.frames)
        return self

    def __exit__(self, *exc):
        lib.flanhip_osc_debug_run(0)
        return False


def osc_phase_dev(freq, n_in, in_rate, d_phases, d_wave, kind, d_ws, stream=None):
    """freq: a float or a device array of n_in floats; d_phases / d_wave: either may be None"""
    fp, f = _dev_curve(freq)
    check(lib.flanhip_osc_phase_dev(fp, f, n_in, in_rate, _dp(d_phases), _dp(d_wave), kind, _dp(d_ws), _vp(stream or 0)))


def oneshot_resample_dev(d_in, n_in, src_rate, dst_rate, d_out, n_out, stream=None):
    check(lib.flanhip_oneshot_resample_dev(_dp(d_in), n_in, src_rate, dst_rate, _dp(d_out), n_out, _vp(stream or 0)))


def audio_synthesize_waveform_workspace_bytes(length, sample_rate, oversample):
    return int(lib.flanhip_audio_synthesize_waveform_workspace_bytes(length, sample_rate, oversample))


def audio_synthesize_waveform_dev(kind, freq, length, sample_rate, oversample, d_out, d_ws, stream=None):
    fp, f = _dev_curve(freq)
    check(lib.flanhip_audio_synthesize_waveform_dev(kind, fp, f, length, sample_rate, oversample, _dp(d_out), _dp(d_ws), _vp(stream or 0)))


def white_noise_draw(seed, count):
    out = np.zeros(max(count, 0), np.float32)
    check(lib.flanhip_white_noise_draw(seed, count, _ptr(out)))
    return out
