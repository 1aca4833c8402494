"""ctypes binding of libpitchextractor_hip.so (the C ABI in include/pitchextractor_hip.h).

There is deliberately no fallback: if the library is missing or a call fails the
caller gets an exception, never a silent eager/CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("PITCHEXTRACTOR_HIP_LIB", _PKG / "libpitchextractor_hip.so"))

_lib = None


class HipLibraryError(RuntimeError):
    pass


_p = C.c_void_p
_i = C.c_int
_l = C.c_long
_f = C.c_float
_d = C.c_double
_z = C.c_size_t
_u64 = C.c_ulonglong
_pp = C.POINTER(C.c_void_p)
_ip = C.POINTER(C.c_int)

# enum pe_products: the product form, first argument of every MFMA-bound entry point
PE_PROD_NATIVE, PE_PROD_X3, PE_PROD_H2, PE_PROD_BF16, PE_PROD_F16 = range(5)
# method of pe_f0_decode_frames
PE_F0_ARGMAX, PE_F0_WEIGHTED = range(2)

# name -> (restype, argtypes).  Mirrors include/pitchextractor_hip.h one to one;
# tests/test_abi.py checks the two against each other and against the .so.
PROTOTYPES = {
    "pe_abi_version": (_i, []),
    "pe_device_count": (_i, []),
    "pe_stream_create_low_priority": (_i, [C.POINTER(_p)]),
    "pe_mel_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _f, _f]),
    "pe_mel_plan_destroy": (_i, [_p]),
    "pe_mel_num_frames": (_i, [_p, _i]),
    "pe_mel_forward": (_i, [_p, _p, _i, _i, _l, _p, _l, _l, _l, _i, _i, _f, _f, _f, _f, _p]),
    "pe_mel_forward_ragged": (_i, [_p, _p, _i, _i, _l, _p, _p, _p, _l, _l, _l, _i, _i, _f, _f, _f, _f, _p]),
    "pe_mel_chunk_fields": (_i, []),
    "pe_mel_forward_chunks": (_i, [_p, _p, _l, _p, _p, _i, _i, _p, _l, _l, _l, _i, _f, _f, _f, _f, _p]),
    "pe_mel_backward_workspace_bytes": (_z, [_p, _i, _i, _i]),
    "pe_mel_backward": (_i, [_p, _p, _i, _i, _l, _p, _l, _l, _l, _i, _i, _f, _f, _f, _p, _l, _p, _z, _p]),
    "pe_mel_backward_ragged": (_i, [_p, _p, _i, _i, _l, _p, _p, _p, _l, _l, _l, _i, _i, _f, _f, _f, _p, _l, _p, _z,
                                    _p]),
    "pe_stitch_run_fields": (_i, []),
    "pe_stitch_chunks": (_i, [_p, _l, _p, _p, _p, _i, _i, _i, _i, _p, _l, _p, _l, _p]),
    "pe_gemm_nt": (_i, [_i, _i, _p, _l, _p, _l, _p, _l, _i, _i, _i, _p, _p, _i, _p, _p, _p]),
    "pe_absmax": (_i, [_p, _l, _i, _l, _p, _p]),
    "pe_absmax_segments": (_i, [_p, _p, _p, _i, _p, _p]),
    "pe_gemm_tn_workspace_bytes": (_z, [_i, _i, _i]),
    "pe_gemm_tn": (_i, [_i, _i, _p, _l, _p, _l, _p, _l, _i, _i, _i, _i, _p, _z, _p, _p, _p]),
    "pe_transpose2d": (_i, [_p, _p, _i, _i, _p]),
    "pe_conv3x3_repack": (_i, [_p, _p, _p, _i, _i, _p]),
    "pe_conv3x3_fwd": (_i, [_i, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "pe_wfrag_bytes": (_z, [_i, _i, _i]),
    "pe_wfrag_pack": (_i, [_i, _p, _l, _i, _i, _p, _p, _p]),
    "pe_conv3x3_wf_supported": (_i, [_i, _i, _i]),
    "pe_conv3x3_fwd_wf": (_i, [_i, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "pe_conv3x3_wgrad_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
    "pe_conv3x3_wgrad": (_i, [_i, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p, _z, _p, _p, _p]),
    "pe_conv3x3_c1_stat_parts": (_i, [_i, _i, _i]),
    "pe_conv3x3_c1_fwd": (_i, [_i, _p, _l, _l, _l, _p, _p, _i, _i, _i, _p, _p]),
    "pe_conv3x3_c1_wgrad": (_i, [_i, _p, _l, _l, _l, _p, _p, _i, _i, _i, _p, _z, _p]),
    "pe_conv3x3_c1_dgrad": (_i, [_i, _p, _p, _p, _i, _i, _i, _p]),
    "pe_bn_workspace_bytes": (_z, [_i]),
    "pe_bn_train_stats": (_i, [_i, _p, _l, _i, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "pe_conv3x3_wf_stat_parts": (_i, [_i, _i, _i]),
    "pe_bn_finalize_stats": (_i, [_p, _i, _l, _i, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "pe_bn_eval_affine": (_i, [_p, _p, _p, _p, _f, _i, _p, _p, _p, _p, _p]),
    "pe_bn_act_pool_fwd": (_i, [_i, _p, _p, _p, _f, _p, _l, _i, _i, _i, _l, _i, _p, _p]),
    "pe_bn_act_pool_bwd": (_i, [_i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _l, _i, _i, _i, _l, _i, _i, _p, _z, _p,
                                _p]),
    "pe_maxpool_fwd": (_i, [_i, _p, _p, _l, _i, _i, _i, _l, _i, _p, _p]),
    "pe_maxpool_bwd_add": (_i, [_i, _p, _p, _p, _p, _l, _i, _i, _i, _l, _i, _p, _p]),
    "pe_bn_act_pool_tap_supported": (_i, [_l, _i, _i, _i, _i, _i]),
    "pe_bn_act_pool_tap_fwd": (_i, [_i, _p, _p, _p, _f, _p, _l, _i, _i, _i, _l, _i, _p, _p, _l, _i, _i, _p, _p]),
    "pe_bn_act_pool_tap_bwd": (_i, [_i, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _l, _i, _i, _i, _l, _i, _i, _p, _z, _p,
                                    _p, _l, _i, _i, _p, _p]),
    "pe_dropout_fwd": (_i, [_i, _p, _l, _p, _l, _p, _p, _l, _i, _f, _u64, _u64, _p]),
    "pe_nhwc_to_seq": (_i, [_i, _p, _l, _i, _p, _l, _i, _p]),
    "pe_seq_to_nhwc": (_i, [_i, _p, _p, _l, _i, _l, _i, _i, _p]),
    "pe_copy2d": (_i, [_i, _p, _l, _p, _l, _l, _i, _i, _p]),
    "pe_lstm_fwd": (_i, [_i, _pp, _pp, _pp, _pp, _ip, _l, _i, _i, _i, _p]),
    "pe_lstm_bwd": (_i, [_i, _pp, _pp, _pp, _pp, _pp, _ip, _l, _i, _i, _i, _p]),
    "pe_lstm_persistent_sync_bytes": (_z, [_i, _i]),
    "pe_lstm_persistent_supported": (_i, [_i, _i, _i]),
    "pe_lstm_fwd_persistent": (_i, [_i, _i, _pp, _pp, _pp, _pp, _ip, _l, _i, _i, _i, _p, _p]),
    "pe_lstm_bwd_persistent_dbias_rows": (_i, [_i, _i, _i, _i, _l]),
    "pe_lstm_configure_stamps": (_i, [_i]),
    "pe_lstm_bwd_persistent": (_i, [_i, _i, _pp, _pp, _pp, _pp, _ip, _l, _i, _i, _i, _pp, _pp, _p, _p]),
    "pe_lstm_whh_grad_workspace_bytes": (_z, [_i, _i, _i]),
    "pe_lstm_whh_grad": (_i, [_i, _p, _p, _l, _p, _i, _i, _i, _i, _p, _z, _p, _p, _p]),
    "pe_colsum_workspace_bytes": (_z, [_i]),
    "pe_colsum": (_i, [_p, _l, _i, _l, _p, _p, _p, _z, _p]),
    "pe_head_fwd": (_i, [_p, _l, _p, _p, _i, _p, _l, _i, _p]),
    "pe_head_bwd_workspace_bytes": (_z, [_i]),
    "pe_head_bwd": (_i, [_p, _l, _p, _p, _i, _p, _l, _p, _p, _l, _i, _p, _z, _p]),
    "pe_f0_sil_loss": (_i, [_p, _p, _p, _p, _f, _l, _f, _p, _p, _p, _p]),
    "pe_bgemm": (_i, [_i, _p, _l, _l, _l, _p, _l, _l, _l, _p, _l, _l, _l, _i, _i, _i, _i, _i, _f, _i, _p]),
    "pe_attn_supported": (_i, [_i, _i]),
    "pe_attn_fwd": (_i, [_i, _p, _l, _p, _l, _p, _p, _p, _i, _i, _i, _i, _f, _f, _u64, _u64, _p]),
    "pe_attn_bwd": (_i, [_i, _p, _l, _p, _p, _l, _p, _p, _p, _i, _i, _i, _i, _f, _f, _p]),
    "pe_softmax_fwd": (_i, [_p, _l, _i, _f, _p]),
    "pe_softmax_bwd": (_i, [_p, _p, _l, _i, _f, _p]),
    "pe_layernorm_fwd": (_i, [_p, _p, _p, _i, _p, _p, _f, _p, _p, _p, _p, _l, _i, _p]),
    "pe_layernorm_bwd_workspace_bytes": (_z, [_i]),
    "pe_layernorm_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p, _z, _p]),
    "pe_gelu_fwd": (_i, [_p, _p, _l, _p]),
    "pe_gelu_bwd": (_i, [_p, _p, _p, _l, _p]),
    "pe_layernorm_dropout_fwd": (_i, [_p, _p, _p, _i, _p, _p, _f, _p, _p, _p, _p, _l, _i, _p, _p, _f, _u64, _u64, _p]),
    "pe_layernorm_bwd_fused": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _l, _i, _p, _z, _p]),
    "pe_gelu_dropout_fwd": (_i, [_p, _p, _l, _p, _p, _f, _u64, _u64, _p]),
    "pe_gelu_dropout_bwd": (_i, [_p, _p, _p, _f, _p, _l, _p]),
    "pe_resample_plan_create": (_i, [C.POINTER(_p), _i, _i, _i, _f]),
    "pe_resample_plan_destroy": (_i, [_p]),
    "pe_resample_out_len": (_l, [_p, _l]),
    "pe_resample_forward": (_i, [_p, _p, _i, _i, _l, _p, _l, _i, _p]),
    "pe_resample_backward": (_i, [_p, _p, _i, _i, _l, _p, _l, _i, _p]),
    "pe_resample_ragged_backward": (_i, [_p, _p, _l, _p, _p, _p, _p, _p, _i, _p, _i, _p]),
    "pe_resample_ragged_plan_create": (_i, [C.POINTER(_p), _ip, _i, _i, _i, _f]),
    "pe_resample_ragged_plan_destroy": (_i, [_p]),
    "pe_resample_ragged_out_len": (_l, [_p, _i, _l]),
    "pe_resample_ragged_forward": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _p, _l, _i, _p]),
    "pe_pitch_shift_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _l, _i, _i, _i, _i, _p, _p, _p]),
    "pe_pitch_shift_plan_fields": (_i, []),
    "pe_pitch_shift_stft": (_i, [_p, _p, _i, _l, _p, _p]),
    "pe_pitch_shift_vocoder": (_i, [_p, _p, _p, _i, _l, _p, _p]),
    "pe_pitch_shift_istft": (_i, [_p, _p, _i, _l, _l, _p, _p, _p]),
    "pe_pitch_shift_resample": (_i, [_p, _p, _p, _p, _i, _p, _p, _i, _l, _p, _p]),
    "pe_world_plan_fields": (_i, []),
    "pe_world_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _d, _d, _i, _p, _p, _p,
                           _p]),
    "pe_world_responses": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _l, _i, _p, _p]),
    "pe_world_overlap_add": (_i, [_p, _p, _p, _p, _p, _i, _l, _i, _p, _p]),
    "pe_world_time_base_plan_fields": (_i, []),
    "pe_world_time_base_plan": (_i, [_i, _p, _p, _p, _d, _d, _p, _p]),
    "pe_world_time_base_workspace_bytes": (_z, [_l]),
    "pe_world_time_base": (_i, [_p, _p, _p, _p, _i, _d, _d, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _z, _p]),
    "pe_cheaptrick_plan_fields": (_i, []),
    "pe_cheaptrick_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _p, _d, _d, _d, _i, _p, _p]),
    "pe_cheaptrick": (_i, [_p, _p, _p, _p, _p, _i, _d, _d, _d, _d, _i, _p, _p]),
    "pe_d4c_plan_fields": (_i, []),
    "pe_d4c_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _p, _d, _d, _i, _p, _p]),
    "pe_d4c_bands": (_i, [_p, _p, _p, _p, _p, _i, _d, _d, _d, _i, _p, _p]),
    "pe_d4c_expand": (_i, [_p, _p, _p, _i, _d, _i, _p, _p]),
    "pe_world_warp_plan_fields": (_i, []),
    "pe_world_warp_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _d, _i, _p, _p]),
    "pe_world_warp": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _d, _i, _p, _p, _p]),
    "pe_f0_bins_ce_workspace_bytes": (_z, [_l]),
    "pe_f0_bins_ce_loss": (_i, [_p, _l, _i, _p, _p, _p, _f, _l, _f, _p, _p, _l, _p, _p, _z, _p]),
    "pe_nonfinite_flag": (_i, [_p, _l, _p, _p]),
    "pe_adamw_step": (_i, [_p, _p, _p, _p, _l, _f, _f, _f, _f, _f, _d, _d, _f, _p, _p]),
    "pe_f0_decode_frames": (_i, [_p, _l, _l, _i, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "pe_f0_viterbi_workspace_bytes": (_z, [_i, _i, _i]),
    "pe_f0_viterbi": (_i, [_p, _l, _l, _i, _p, _i, _i, _p, _p, _z, _p]),
    "pe_pitch_metrics": (_i, [_p, _p, _l, _d, _p, _p]),
    "pe_f0_track_plan_fields": (_i, []),
    "pe_f0_track_plan": (_i, [_i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "pe_row_stats_workspace_bytes": (_z, [_i]),
    "pe_row_stats": (_i, [_p, _p, _i, _i, _p, _p, _z, _p]),
    "pe_f0_track_frames": (_i, [_p, _p, _p, _p, _p, _p, _l, _i, _i, _i, _p, _p, _p, _p, _p]),
    "pe_f0_track_path": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _z, _p]),
    "pe_f0_dio_plan_fields": (_i, []),
    "pe_f0_dio_plan": (_i, [_i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "pe_f0_dio_bands": (_i, [_p, _p, _p, _p, _p, _l, _i, _i, _i, _p, _p, _p]),
    "pe_f0_dio_events": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _z, _p]),
    "pe_f0_dio_candidates": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "pe_f0_dio_fix": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "pe_f0_stonemask": (_i, [_p, _p, _p, _p, _p, _l, _i, _i, _i, C.c_double, _p, _p]),
    "pe_stress_plan_fields": (_i, []),
    "pe_stress_plan": (_i, [_i, _p, _p, _p, _p, _p, _p]),
    "pe_stress_rir_workspace_bytes": (_z, [_l]),
    "pe_stress_spectra": (_i, [_p, _p, _p, _i, _i, _p, _l, _p, _p]),
    "pe_stress_rir": (_i, [_p, _p, _p, _i, _p, _p, _p, _i, _p, _p, _p, _l, _p, _p, _z, _p]),
    "pe_stress_biquad": (_i, [_p, _p, _p, _i, _p, _i, _p, _p]),
    "pe_stress_clip": (_i, [_p, _p, _p, _i, _d, _i, _p, _p, _p]),
    "pe_stress_clip_rows": (_i, [_p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p]),
    "pe_stress_agc_workspace_bytes": (_z, [_l]),
    "pe_stress_agc": (_i, [_p, _p, _p, _i, _p, _i, _p, _p, _z, _p]),
    "pe_melody_metrics_fields": (_i, []),
    "pe_melody_metrics": (_i, [_p, _p, _p, _p, _p, _i, _d, _p, _p]),
    "pe_stim_plan_fields": (_i, []),
    "pe_stim_param_fields": (_i, []),
    "pe_stim_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _d, _p, _p, _p, _p]),
    "pe_stim_workspace_bytes": (_z, [_l]),
    "pe_stim_phase": (_i, [_p, _p, _p, _p, _i, _p, _p, _z, _p]),
    "pe_stim_synth": (_i, [_p, _p, _p, _p, _i, _p, _p]),
    "pe_stim_tone": (_i, [_p, _p, _p, _i, _p, _p]),
    "pe_stim_finish": (_i, [_p, _p, _p, _p, _i, _p, _p, _p, _z, _p]),
    "pe_stim_reference": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _p, _p]),
    "pe_dynamic_metrics_fields": (_i, []),
    "pe_dynamic_metrics": (_i, [_p, _p, _p, _p, _i, _p, _p]),
    "pe_noise_plan_fields": (_i, []),
    "pe_noise_param_fields": (_i, []),
    "pe_noise_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "pe_noise_workspace_bytes": (_z, [_l]),
    "pe_noise_white": (_i, [_p, _p, _i, _p, _p]),
    "pe_noise_colour": (_i, [_p, _p, _p, _p, _p, _l, _i, _p, _p, _z, _p]),
    "pe_noise_bed": (_i, [_p, _p, _p, _l, _p, _p, _i, _p, _p]),
    "pe_noise_mix": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _z, _p]),
    "pe_rir_plan_fields": (_i, []),
    "pe_rir_plan": (_i, [_i, _p, _p, _p, _p, _p, _l, _p]),
    "pe_rir_synth": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _l, _p]),
    "pe_rir_decay": (_i, [_p, _l, _p, _p, _i, _i, _d, _d, _d, _p, _p, _p]),
    "pe_augment_biquad_consts": (_i, [_p]),
    "pe_augment_biquad": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "pe_augment_gain": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p]),
    "pe_codec_plan_fields": (_i, []),
    "pe_codec_plan": (_i, [_i, _i, _p, _p, _p, _p, _p, _p]),
    "pe_codec_bands": (_i, [_i, _p, _i]),
    "pe_codec_workspace_bytes": (_z, [_i, _l]),
    "pe_codec_mdct": (_i, [_p, _p, _p, _i, _i, _p, _l, _p, _p]),
    "pe_codec_quantize": (_i, [_p, _l, _i, _i, _i, _p, _l, _p, _p, _p, _p, _p]),
    "pe_codec_imdct": (_i, [_p, _p, _p, _i, _i, _p, _l, _p, _p, _z, _p]),
    "pe_codec_apply": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _l, _p, _p, _p, _p, _z, _p]),
    "pe_codec_mulaw": (_i, [_p, _p, _p, _i, _i, _p, _p]),
    "pe_pitch_mod_consts": (_i, [_p]),
    "pe_pitch_mod_plan_fields": (_i, []),
    "pe_pitch_mod_plan": (_i, [_i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "pe_pitch_mod_wave": (_i, [_p, _p, _p, _p, _p, _i, _p, _i, _i, _p, _p]),
    "pe_pitch_mod_labels": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
}


def load():
    """Load the shared library once and attach prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python -m pitchextractor_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as /opt/rocm's, but its
    # libraries ask for it by the unversioned file name, so it is loaded even when /opt/rocm's copy already
    # is).  Loading this library first therefore left TWO runtimes in the process, and the second to open the
    # device reported hipErrorNoDevice (seen with build() followed by smoke() in one interpreter).  With torch
    # imported first, this library's DT_NEEDED libamdhip64.so.7 resolves to the copy torch already loaded.
    import torch  # noqa: F401
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status == 0:
        return
    if status < 0:
        kind = {-1: "invalid argument", -2: "unsupported shape", -3: "workspace too small"}.get(status, "error")
        raise HipLibraryError(f"{what}: {kind} ({status})")
    raise HipLibraryError(f"{what}: hipError_t {status}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


_tables = {}


def device_table(key, device, build):
    """Device copy of the float32 table that ``build()`` returns (numpy), made once per (key, device)."""
    import numpy as np
    import torch
    k = (key, str(device))
    if k not in _tables:
        _tables[k] = torch.from_numpy(np.ascontiguousarray(build(), dtype=np.float32)).to(device)
    return _tables[k]


def stream_ptr() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
