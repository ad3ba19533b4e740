"""ctypes mirror of the C ABI in include/gmr1_hip.h (libgmr1_hip.so).

This is plumbing only: every function forwards to the shared library, which runs
HIP kernels.  There is no Python or CPU implementation behind these calls --
if the library is missing or no GPU is usable they raise.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os

import numpy as np

from . import build as _build

MAX_SYNC, MAX_CHUNKS, MAX_SYNC_SYMS = 4, 8, 32
BURST_IDS = ["bcch", "dc2", "dc6", "dc12", "nt3_speech", "nt3_facch", "nt6", "nt9", "rach", "sdcch"]

# Every function include/gmr1_hip.h, include/gmr1_hip_shard.h and include/osmocom/gmr1/**.h declare:
# name -> (return type, argument types...).  Every pointer parameter is P (it takes None, an address, a c_void_p, byref()
# and ctypes arrays alike); an enum is I.  tests/test_capi.py compares each row with the header's declaration.
I, U8, U32, U64, F, D, P, Z, SZ = (C.c_int, C.c_uint8, C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_void_p,
                                   C.c_char_p, C.c_size_t)
SIGNATURES = {
    # include/gmr1_hip.h
    "gmr1_hip_init": (I, I),
    "gmr1_hip_last_error": (Z,),
    "gmr1_hip_version": (Z,),
    "gmr1_hip_burst_info": (I, I, P),
    "gmr1_hip_clock_probe_dev": (I, P, I, P, P),
    "gmr1_hip_set_conv_decoder": (I, I),
    "gmr1_hip_get_conv_decoder": (I,),
    "gmr1_hip_demod_batch_dev": (I, P, I, I, I, I, P, P, P, P, I, P, P, P, P, P),
    "gmr1_hip_demod_batch": (I, I, I, I, I, P, U64, P, P, P, I, P, P, P, P, P),
    "gmr1_hip_demod_taps": (I, I, I, I, P, F, P, P, P, P, P, P, P, P, P, P),
    "gmr1_hip_detect_batch_dev": (I, P, I, P, I, I, I, P, P, P, P, P, P, P, P),
    "gmr1_hip_detect_batch": (I, I, P, I, I, I, P, U64, P, P, P, P, P, P, P),
    "gmr1_hip_mod_order_batch_dev": (I, P, I, I, I, P, P, P, P),
    "gmr1_hip_mod_order_batch": (I, I, I, I, P, U64, P, P, P),
    "gmr1_hip_bcch_decode_batch_dev": (I, P, I, P, P, P, P),
    "gmr1_hip_ccch_decode_batch_dev": (I, P, I, P, P, P, P),
    "gmr1_hip_bcch_decode_batch": (I, I, P, P, P, P),
    "gmr1_hip_ccch_decode_batch": (I, I, P, P, P, P),
    "gmr1_hip_rx_bcch_ccch_batch_dev": (I, P, I, I, P, P, P, P, P, P, P, P, P, P, P, P),
    "gmr1_hip_rx_bcch_ccch_batch": (I, I, I, P, U64, P, P, P, P, P, P, P, P, P, P, P),
    "gmr1_hip_rx_bcch_ccch_batch_planar_dev": (I, P, I, I, P, U64, P, P, P, P, P, P, P, P, P, P, P),
    "gmr1_hip_iq_to_planar_dev": (I, P, I, U64, P, P, U64),
    "gmr1_hip_facch3_decode_batch_dev": (I, P, I, P, P, P, P, P, P),
    "gmr1_hip_facch3_decode_batch": (I, I, P, P, P, P, P, P),
    "gmr1_hip_tch3_decode_batch_dev": (I, P, I, I, P, P, P, P, P),
    "gmr1_hip_tch3_decode_batch": (I, I, I, P, P, P, P, P),
    "gmr1_hip_tch3_rx_batch_dev": (I, P, I, I, I, P, P, P, I, P, P, P, P, P, P, P, P),
    "gmr1_hip_tch3_rx_batch": (I, I, I, I, P, U64, P, P, I, P, P, P, P, P, P, P, P),
    "gmr1_hip_dkab_demod_batch_dev": (I, P, I, I, I, P, P, P, P, P, P, P),
    "gmr1_hip_dkab_demod_batch": (I, I, I, I, P, U64, P, P, P, P, P, P),
    "gmr1_hip_a5_batch_dev": (I, P, I, I, I, P, P, P, P),
    "gmr1_hip_a5_batch": (I, I, I, I, P, P, P, P),
    "gmr1_hip_facch9_decode_batch_dev": (I, P, I, P, P, P, P, P, P, P),
    "gmr1_hip_facch9_decode_batch": (I, I, P, P, P, P, P, P, P),
    "gmr1_hip_tch9_decode_batch_dev": (I, P, I, I, I, P, P, P, P, P, P),
    "gmr1_hip_tch9_decode_batch": (I, I, I, I, P, P, P, P, P, P),
    "gmr1_hip_xch_dc12_decode_batch_dev": (I, P, I, P, P, P, P),
    "gmr1_hip_xch_dc12_decode_batch": (I, I, P, P, P, P),
    "gmr1_hip_rach_decode_batch_dev": (I, P, I, P, P, P, P, P, P),
    "gmr1_hip_rach_decode_batch": (I, I, P, P, P, P, P, P),
    "gmr1_hip_bcch_encode_batch_dev": (I, P, I, P, P),
    "gmr1_hip_bcch_encode_batch": (I, I, P, P),
    "gmr1_hip_ccch_encode_batch_dev": (I, P, I, P, P),
    "gmr1_hip_ccch_encode_batch": (I, I, P, P),
    "gmr1_hip_xch_dc12_encode_batch_dev": (I, P, I, P, P),
    "gmr1_hip_xch_dc12_encode_batch": (I, I, P, P),
    "gmr1_hip_facch3_encode_batch_dev": (I, P, I, P, P, P, P),
    "gmr1_hip_facch3_encode_batch": (I, I, P, P, P, P),
    "gmr1_hip_tch3_encode_batch_dev": (I, P, I, I, P, P, P, P),
    "gmr1_hip_tch3_encode_batch": (I, I, I, P, P, P, P),
    "gmr1_hip_facch9_encode_batch_dev": (I, P, I, P, P, P, P, P),
    "gmr1_hip_facch9_encode_batch": (I, I, P, P, P, P, P),
    "gmr1_hip_tch9_encode_batch_dev": (I, P, I, I, I, P, P, P, P, P),
    "gmr1_hip_tch9_encode_batch": (I, I, I, I, P, P, P, P, P),
    "gmr1_hip_rach_encode_batch_dev": (I, P, I, P, P, P),
    "gmr1_hip_rach_encode_batch": (I, I, P, P, P),
    "gmr1_hip_mod_batch_dev": (I, P, I, I, I, P, P),
    "gmr1_hip_mod_batch": (I, I, I, I, P, P),
    "gmr1_hip_shape_batch_dev": (I, P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, U64),
    "gmr1_hip_shape_batch": (I, I, I, I, I, I, I, P, P, P, P, P, P, P, P, U64),
    "gmr1_hip_mod_shaped_batch_dev": (I, P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, U64),
    "gmr1_hip_mod_shaped_batch": (I, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, U64),
    "gmr1_hip_fcch_chirp_batch_dev": (I, P, I, I, I, I, P, P, P, P, P, P, P, U64),
    "gmr1_hip_fcch_chirp_batch": (I, I, I, I, I, P, P, P, P, P, P, P, U64),
    "gmr1_hip_carrier_mix_dev": (I, P, I, P, P, P, P, P, U32, P, P, U64, P, P, P, P, U64, P),
    "gmr1_hip_carrier_mix": (I, I, P, U64, I, P, P, P, P, U32, P, P, U64, P, P, P, P, U64, P, U64),
    "gmr1_hip_encoder_plan": (I, I, P, I),
    "gmr1_hip_fcch_rough_batch_dev": (I, P, I, I, I, I, P, P, P, P, P),
    "gmr1_hip_fcch_rough_batch": (I, I, I, I, I, P, U64, P, P, P, P),
    "gmr1_hip_fcch_rough_multi_batch_dev": (I, P, I, I, I, I, P, P, P, P, I, P),
    "gmr1_hip_fcch_rough_multi_batch": (I, I, I, I, I, P, U64, P, P, P, I, P),
    "gmr1_hip_fcch_fine_batch_dev": (I, P, I, I, I, P, P, P, P, P),
    "gmr1_hip_fcch_fine_batch": (I, I, I, I, P, U64, P, P, P, P),
    "gmr1_hip_fcch_snr_batch_dev": (I, P, I, I, I, P, P, P, P),
    "gmr1_hip_fcch_snr_batch": (I, I, I, I, P, U64, P, P, P),
    "gmr1_hip_fcch_acquire_batch_dev": (I, P, I, I, I, P, P, P, P, P),
    "gmr1_hip_fcch_acquire_batch": (I, I, I, I, P, U64, P, P, P, P),
    "gmr1_hip_ddc_plan": (I, D, I, U64, P, P, P, P),
    "gmr1_hip_ddc_dev": (I, P, D, I, P, U64, I, P, P, U64, P),
    "gmr1_hip_ddc": (I, D, I, P, U64, I, P, P, U64, P),
    "gmr1_hip_channelize_plan": (I, D, I, U64, P, P, P),
    "gmr1_hip_channelize_dev": (I, P, D, I, P, U64, F, I, P, P, U64, P),
    "gmr1_hip_channelize": (I, D, I, P, U64, F, I, P, P, U64, P),
    "gmr1_hip_channelize_planar_dev": (I, P, D, I, P, U64, F, I, P, P, U64, U64, P),
    "gmr1_hip_channelize_stream_create": (I, D, I, F, I, P, P),
    "gmr1_hip_ddc_stream_create": (I, D, I, I, P, P),
    "gmr1_hip_chan_stream_out_len": (I, P, U64, P),
    "gmr1_hip_chan_stream_push_dev": (I, P, P, P, U64, P, U64, P),
    "gmr1_hip_chan_stream_push": (I, P, P, U64, P, U64, P),
    "gmr1_hip_chan_stream_destroy": (I, P),
    "gmr1_hip_iq_sample_bytes": (I, I),
    "gmr1_hip_channelize_iq_dev": (I, P, D, I, I, P, U64, F, I, P, P, U64, P),
    "gmr1_hip_channelize_iq": (I, D, I, I, P, U64, F, I, P, P, U64, P),
    "gmr1_hip_channelize_planar_iq_dev": (I, P, D, I, I, P, U64, F, I, P, P, U64, U64, P),
    "gmr1_hip_ddc_iq_dev": (I, P, D, I, I, P, U64, I, P, P, U64, P),
    "gmr1_hip_ddc_iq": (I, D, I, I, P, U64, I, P, P, U64, P),
    "gmr1_hip_channelize_stream_create_iq": (I, D, I, I, F, I, P, P),
    "gmr1_hip_ddc_stream_create_iq": (I, D, I, I, I, P, P),
    "gmr1_hip_chan_stream_push_iq_dev": (I, P, P, P, U64, P, U64, P),
    "gmr1_hip_chan_stream_push_iq": (I, P, P, U64, P, U64, P),
    "gmr1_hip_rx_run_dev": (I, P, I, I, P, P, P, P, P, I, P, P, P),
    "gmr1_hip_rx_run": (I, I, I, P, U64, P, P, P, P, I, P, P, P),
    "gmr1_hip_rx_stream_create": (I, I, I, P, P),
    "gmr1_hip_rx_stream_max_records": (I, P, U64, P),
    "gmr1_hip_rx_stream_push_dev": (I, P, P, P, U64, U64, I, P, I, P),
    "gmr1_hip_rx_stream_push": (I, P, P, U64, U64, I, P, I, P),
    "gmr1_hip_rx_stream_status": (I, P, P, P, P),
    "gmr1_hip_rx_stream_destroy": (I, P),
    "gmr1_hip_rx_stream_create_tch": (I, I, I, P, P, P),
    "gmr1_hip_rx_stream_push_tch_dev": (I, P, P, P, P, U64, U64, I, P, I, P),
    "gmr1_hip_rx_stream_push_tch": (I, P, P, P, U64, U64, I, P, I, P),
    "gmr1_hip_rx_stream_create_full": (I, I, I, P, P, P),
    "gmr1_hip_rx_stream_max_big": (I, P, U64, P),
    "gmr1_hip_rx_stream_push_full_dev": (I, P, P, P, P, P, U64, U64, I, P, I, P, P, I, P),
    "gmr1_hip_rx_stream_push_full": (I, P, P, P, P, U64, U64, I, P, I, P, P, I, P),
    "gmr1_hip_rx_stream_create_voice": (I, I, I, P, P, P),
    "gmr1_hip_rx_stream_max_audio": (I, P, U64, P),
    "gmr1_hip_rx_stream_push_voice_dev": (I, P, P, P, P, U64, U64, I, P, I, P, P, I, P),
    "gmr1_hip_rx_stream_push_voice": (I, P, P, P, U64, U64, I, P, I, P, P, I, P),
    "gmr1_hip_rx_run_voice_dev": (I, P, I, I, P, P, P, P, P, P, P, I, P, P, P, P, I, P),
    "gmr1_hip_rx_run_voice": (I, I, I, P, P, U64, P, P, P, P, P, I, P, P, P, P, I, P),
    "gmr1_hip_rx_run_tch_dev": (I, P, I, I, P, P, P, P, P, P, P, I, P, P, P),
    "gmr1_hip_rx_run_tch": (I, I, I, P, P, U64, P, P, P, P, P, I, P, P, P),
    "gmr1_hip_rx_run_last_timing": (I, P),
    "gmr1_hip_tch3_state_assign": (I, P, I, F),
    "gmr1_hip_tch3_state_assign_batch_dev": (I, P, I, P, P, P, P),
    "gmr1_hip_tch3_follow_batch_dev": (I, P, I, I, I, P, P, I, P, P, P, P, P),
    "gmr1_hip_tch3_follow_batch": (I, I, I, I, P, U64, P, I, P, P, P, P, P),
    "gmr1_hip_tch3_frames_to_pcm_dev": (I, P, I, P, I, P, P, P, P),
    "gmr1_hip_tch3_frames_to_pcm": (I, I, P, I, P, P, I, P, P),
    "gmr1_hip_tch3_frames_to_audio_dev": (I, P, I, P, I, P, P, P, P, P, I, P),
    "gmr1_hip_tch3_voice_batch_dev": (I, P, I, I, I, P, P, I, P, P, P, P, P, P, P, P),
    "gmr1_hip_tch3_voice_batch": (I, I, I, I, P, U64, P, I, P, P, P, P, P, P, I, P, P),
    "gmr1_hip_tch9_state_assign": (I, P),
    "gmr1_hip_tch9_state_assign_batch_dev": (I, P, I, P, P),
    "gmr1_hip_tch9_follow_bits_batch_dev": (I, P, I, I, P, I, P, P, P, P, P, P),
    "gmr1_hip_tch9_follow_bits_batch": (I, I, I, P, I, P, P, P, P, P, P),
    "gmr1_hip_tch9_follow_batch_dev": (I, P, I, I, I, I, P, P, I, P, P, P, P, P),
    "gmr1_hip_tch9_follow_batch": (I, I, I, I, I, P, U64, P, I, P, P, P, P, P),
    "gmr1_hip_tch9_frames_to_records_dev": (I, P, I, P, I, P, P, P, I, P),
    "gmr1_hip_rx_run_full_dev": (I, P, I, I, P, P, P, P, P, P, P, P, I, P, P, I, P, P, P),
    "gmr1_hip_rx_run_full": (I, I, I, P, P, P, U64, P, P, P, P, P, I, P, P, I, P, P, P),
    "gmr1_hip_codec_state_bytes": (SZ,),
    "gmr1_hip_codec_init_dev": (I, P, I, P, I),
    "gmr1_hip_codec_init_list_dev": (I, P, I, P, P, I),
    "gmr1_hip_codec_decode_batch_dev": (I, P, I, I, P, P, P, P),
    "gmr1_hip_codec_decode_batch": (I, I, I, P, P, P, P, I),
    "gmr1_hip_codec_host_tables": (I, P, P),
    "gmr1_hip_codec_libm_check": (I, I, I, P, P),
    "gmr1_hip_gsmtap_pack": (I, P, I, P, I),
    "gmr1_hip_gsmtap_pack_big": (I, P, I, P, I),
    # include/gmr1_hip_shard.h
    "gmr1_hip_shard_unique_id": (I, P),
    "gmr1_hip_shard_create": (I, P, P, I, I),
    "gmr1_hip_shard_adopt": (I, P, P, I, I),
    "gmr1_hip_shard_destroy": (None, P),
    "gmr1_hip_rx_run_sharded": (I, P, P, I, I, I, P, P, P, P, P, I, P, P, P, P),
    "gmr1_hip_rx_run_sharded_resident": (I, P, P, I, I, I, P, P, P, P, P, I, P, P, P, P),
    # include/osmocom/gmr1/codec/codec.h
    "gmr1_codec_alloc": (P,),
    "gmr1_codec_release": (None, P),
    "gmr1_codec_decode_frame": (I, P, P, I, P, I),
    "gmr1_codec_decode_dtx": (I, P, P, I),
    # include/osmocom/gmr1/l1/*.h
    "gmr1_a5": (None, I, P, U32, I, P, P),
    "gmr1_a5_1": (None, P, U32, I, P, P),
    "gmr1_bcch_decode": (I, P, P, P),
    "gmr1_bcch_encode": (None, P, P),
    "gmr1_ccch_decode": (I, P, P, P),
    "gmr1_ccch_encode": (None, P, P),
    "gmr1_facch3_decode": (I, P, P, P, P, P),
    "gmr1_facch3_encode": (None, P, P, P, P),
    "gmr1_facch9_decode": (I, P, P, P, P, P, P),
    "gmr1_facch9_encode": (None, P, P, P, P, P),
    "gmr1_interleave_intra": (None, P, P, I),
    "gmr1_deinterleave_intra": (None, P, P, I),
    "gmr1_interleave_inter": (None, P, P, P),
    "gmr1_deinterleave_inter": (None, P, P, P),
    "gmr1_interleaver_init": (I, P, I, I),
    "gmr1_interleaver_fini": (None, P),
    "gmr1_puncturer_generate": (I, P, P, P, P, I),
    "gmr1_rach_decode": (I, P, P, U8, P, P),
    "gmr1_rach_encode": (None, P, P, U8),
    "gmr1_scramble_sbit": (None, P, P, I),
    "gmr1_scramble_ubit": (None, P, P, I),
    "gmr1_tch3_decode": (None, P, P, P, P, P, I, P, P),
    "gmr1_tch3_encode": (None, P, P, P, P, P, I),
    "gmr1_tch9_decode": (None, P, P, P, P, I, P, P, P),
    "gmr1_tch9_encode": (None, P, P, I, P, P, P, P),
    "gmr1_xch_dc12_decode": (I, P, P, P),
    "gmr1_xch_dc12_encode": (I, P, P),
    # include/osmocom/gmr1/sdr/*.h
    "gmr1_dkab_demod": (I, P, I, F, I, P, P),
    "gmr1_fcch_rough": (I, P, P, I, F, P),
    "gmr1_fcch_rough_multi": (I, P, P, I, F, P, I),
    "gmr1_fcch_fine": (I, P, P, I, F, P, P),
    "gmr1_fcch_snr": (I, P, P, I, F, P),
    "gmr1_pi4cxpsk_demod": (I, P, P, I, F, P, P, P, P),
    "gmr1_pi4cxpsk_detect": (I, P, F, P, I, F, P, P, P),
    "gmr1_pi4cxpsk_mod_order": (I, P, I, F),
    "gmr1_pi4cxpsk_mod": (I, P, P, I, P),
}
EXPORTED_FUNCTIONS = list(SIGNATURES)
EXPORTED_DATA = [
    "gmr1_pi2cbpsk", "gmr1_pi4cbpsk", "gmr1_pi4cqpsk",
    "gmr1_bcch_burst", "gmr1_dc2_burst", "gmr1_dc6_burst", "gmr1_dc12_burst",
    "gmr1_nt3_speech_burst", "gmr1_nt3_facch_burst", "gmr1_nt6_burst", "gmr1_nt9_burst",
    "gmr1_rach_burst", "gmr1_sdcch_burst",
    "gmr1_fcch_burst", "gmr1_fcch3_lband_burst", "gmr1_fcch3_sband_burst",
    # code descriptions for libosmocore's own codec (l1/conv.h, l1/crc.h, l1/punct.h): host data, not used by the kernels
    "gmr1_conv_k5_12", "gmr1_conv_k5_13", "gmr1_conv_k5_14", "gmr1_conv_k5_15", "gmr1_conv_k6_14", "gmr1_conv_k9_12",
    "gmr1_conv_k9_13", "gmr1_conv_k9_14", "gmr1_conv_tch3", "gmr1_crc8", "gmr1_crc12", "gmr1_crc16",
] + ["gmr1_punct_" + _n for _n in """
    k5_12_P23 k5_12_P25 k5_12_Ps25 k5_12_P311 k5_12_P412 k5_12_Ps412 k5_12_P12 k5_12_Ps12 k5_12_A k5_12_B
    k5_12_C k5_12_D k5_12_E k5_12_P38 k5_12_P26 k5_12_P37 k5_13_P16 k5_13_P25 k5_13_P15 k5_13_Ps15 k5_13_P78
    k5_15_P23 k5_15_P53 k5_15_Ps53 k7_12_P23 k7_12_P410 k7_12_P512 k7_12_P116 k7_12_P148 k7_12_P184
    k7_12_P1152 k7_12_P45 k7_12_P245 k9_12_P13 k9_12_P47 k9_12_P34 k9_12_P17 k9_12_P19 k9_12_P26 k9_12_P110
    k9_12_P14 k9_12_P45 k9_12_P234 k6_14_P45 k9_14_P148 k9_14_P65 k9_13_P12 k9_13_P1213 k9_13_P44 k9_13_P33
    k9_13_P65
""".split()]


class Chunk(C.Structure):
    _fields_ = [("pos", C.c_int32), ("len", C.c_int32), ("syms", C.c_uint8 * MAX_SYNC_SYMS)]


class BurstFlat(C.Structure):
    _fields_ = [
        ("name", C.c_char * 16), ("rotation", C.c_float), ("nbits", C.c_int32),
        ("guard_pre", C.c_int32), ("guard_post", C.c_int32), ("len", C.c_int32), ("ebits", C.c_int32),
        ("n_sync", C.c_int32), ("n_sync_chunks", C.c_int32 * MAX_SYNC),
        ("sync", (Chunk * MAX_CHUNKS) * MAX_SYNC),
        ("n_data", C.c_int32), ("data", Chunk * MAX_CHUNKS),
    ]


class CxVec(C.Structure):
    """struct osmo_cxvec (include/osmocom/gmr1/compat.h)."""
    _fields_ = [("len", C.c_int), ("max_len", C.c_int), ("flags", C.c_int), ("data", C.c_void_p)]


class Gmr1HipError(RuntimeError):
    pass


_lib = None
_fns = {}


def lib_path() -> str:
    # tools/ (never the tests, never bench.py's default run) may point at the profiling build: build.py --profile
    return os.environ.get("GMR1_HIP_LIBRARY") or _build.LIB


def load(build_if_missing: bool = False):
    """dlopen libgmr1_hip.so (fails loudly if it has not been built).  The handle stays untyped but for the two string
    returns: raw callers (bench.py, tests, tools) wrap their own arguments."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        if build_if_missing:
            _build.build()
        else:
            raise Gmr1HipError(
                f"{path} is missing: the HIP extension has not been built "
                "(run __graft_entry__.build()); there is no CPU fallback")
    _lib = C.CDLL(path)
    _lib.gmr1_hip_last_error.restype = C.c_char_p
    _lib.gmr1_hip_version.restype = C.c_char_p
    return _lib


def _fn(name):
    """The typed prototype of SIGNATURES[name]: a function object of its own, not the shared handle's attribute."""
    f = _fns.get(name)
    if f is None:
        f = _fns[name] = C.CFUNCTYPE(*SIGNATURES[name])((name, load()))
    return f


def _last_error() -> str:
    return _fn("gmr1_hip_last_error")().decode(errors="replace")


def _check(rc: int, what: str):
    if rc != 0:
        raise Gmr1HipError(f"{what} failed with {rc}: {_last_error()}")


def _call(name, *args):
    """A function that returns 0 or a negative errno: raise on the latter."""
    rc = (_fns.get(name) or _fn(name))(*args)
    if rc:
        _check(rc, name)


def _arr(a, dtype, shape=None):
    """Input array: contiguous, of `dtype`, optionally reshaped; None (an optional buffer left out) stays None.
    The caller holds the result in a local for as long as the library reads it."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype)
    return a if shape is None else a.reshape(shape)


def _p(a):
    """Address of an array, or None for a buffer left out."""
    return None if a is None else a.ctypes.data


def _window(iq, offset, freq_shift, broadcast=False):
    """The batch calls' window arguments -> (flat complex64 iq, uint64 offset, n, float32 freq_shift or None)"""
    iq = _arr(iq, np.complex64, -1)
    offset = _arr(offset, np.uint64)
    if broadcast and freq_shift is not None:
        freq_shift = np.broadcast_to(np.asarray(freq_shift, np.float32), (offset.size,))
    return iq, offset, offset.size, _arr(freq_shift, np.float32)


def _cxvec(iq):
    """-> (complex64 samples, the struct osmo_cxvec over them)"""
    iq = _arr(iq, np.complex64)
    return iq, CxVec(iq.size, iq.size, 0, iq.ctypes.data)


def _burst_id(burst):
    return BURST_IDS.index(burst) if isinstance(burst, str) else int(burst)


class _Handle:
    """close / with / del of an object that owns something inside the library; a subclass states _destroy()."""

    def close(self):
        self._destroy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def burst_info(name_or_id) -> BurstFlat:
    out = BurstFlat()
    _call("gmr1_hip_burst_info", _burst_id(name_or_id), C.byref(out))
    return out


def burst_format(name_or_id):
    """Product burst table -> synth.BurstFormat."""
    from . import synth
    b = burst_info(name_or_id)
    sync = []
    for s in range(b.n_sync):
        sync.append([(b.sync[s][c].pos, [int(b.sync[s][c].syms[k]) for k in range(b.sync[s][c].len)])
                     for c in range(b.n_sync_chunks[s])])
    data = [(b.data[c].pos, b.data[c].len) for c in range(b.n_data)]
    return synth.BurstFormat(b.name.decode(), float(b.rotation), b.nbits, b.len, b.ebits, sync, data)


CONV_GENERIC, CONV_ACC = 0, 1


def set_conv_decoder(decoder: int):
    """gmr1_hip_set_conv_decoder: which libosmocore Viterbi decoder the layer-1 chains reproduce (process-wide)."""
    _call("gmr1_hip_set_conv_decoder", int(decoder))


def get_conv_decoder() -> int:
    return _fn("gmr1_hip_get_conv_decoder")()


class conv_decoder:
    """with api.conv_decoder(api.CONV_ACC): ...  -- switch the decoder for a block (tests, bench)."""

    def __init__(self, decoder):
        self.decoder = int(decoder)

    def __enter__(self):
        self.prev = get_conv_decoder()
        set_conv_decoder(self.decoder)
        return self

    def __exit__(self, *exc):
        set_conv_decoder(self.prev)
        return False


def init(device: int = 0):
    _call("gmr1_hip_init", device)


def clock_probe_dev(stream, micros=200):
    """(shader clock held right now in MHz, wall counter rate in MHz), measured on the device behind what `stream` holds."""
    core, wall = C.c_double(), C.c_double()
    _call("gmr1_hip_clock_probe_dev", stream, micros, C.byref(core), C.byref(wall))
    return core.value, wall.value


# ---------------------------------------------------------------------------
# host-pointer batch calls (numpy in, numpy out)
# ---------------------------------------------------------------------------
def demod_batch(burst, iq, offset, in_len, sps=4, freq_shift=None, want_ssyms=True):
    bid = _burst_id(burst)
    info = burst_info(bid)
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    eb = np.zeros((n, info.ebits), np.int8)
    sid = np.zeros(n, np.int32)
    toa = np.zeros(n, np.float32)
    fe = np.zeros(n, np.float32)
    ss = np.zeros((n, info.len), np.float32) if want_ssyms else None
    rv = np.zeros(n, np.int32)
    _call("gmr1_hip_demod_batch", bid, n, sps, in_len, _p(iq), iq.size, _p(offset), _p(fs),
          _p(eb), info.ebits, _p(sid), _p(toa), _p(fe), _p(ss), _p(rv))
    return dict(rv=rv, ebits=eb, sync_id=sid, toa=toa, freq_err=fe, ssyms=ss)


def demod_taps(burst, iq, sps=4, freq_shift=0.0):
    """One burst through gmr1_hip_demod_taps: the batch entry's outputs plus the four vectors the reference dumps under
    ENABLE_DEBUG_SIGNAL (sdr/defs.h:35-39): corr (pi4cxpsk.c:251), burst (:545), align (:345), final (:582)."""
    bid = _burst_id(burst)
    info = burst_info(bid)
    iq = _arr(iq, np.complex64, -1)
    in_len = iq.size
    w = in_len - info.len * sps + 1
    out = dict(corr=np.zeros(max(w, 0), np.float32), burst=np.zeros(in_len, np.complex64),
               align=np.zeros(info.len, np.complex64), final=np.zeros(info.len, np.complex64),
               ebits=np.zeros(info.ebits, np.int8), sync_id=np.zeros(1, np.int32), toa=np.zeros(1, np.float32),
               freq_err=np.zeros(1, np.float32), ssyms=np.zeros(info.len, np.float32), rv=np.zeros(1, np.int32))
    _call("gmr1_hip_demod_taps", bid, sps, in_len, _p(iq), freq_shift, *[_p(a) for a in out.values()])
    for k in ("sync_id", "toa", "freq_err", "rv"):
        out[k] = out[k][0]
    return out


def _l1_batch(fn, ebits, neb):
    ebits = _arr(ebits, np.int8, (-1, neb))
    n = ebits.shape[0]
    l2 = np.zeros((n, 24), np.uint8)
    crc = np.zeros(n, np.int32)
    conv = np.zeros(n, np.int32)
    _call(fn, n, _p(ebits), _p(l2), _p(crc), _p(conv))
    return l2, crc, conv


def bcch_decode_batch(ebits):
    return _l1_batch("gmr1_hip_bcch_decode_batch", ebits, 424)


def ccch_decode_batch(ebits):
    return _l1_batch("gmr1_hip_ccch_decode_batch", ebits, 432)


def rx_bcch_ccch_batch(iq, offset, kind, sps=4, freq_shift=None, want_ebits=True, want_ssyms=True):
    iq, offset, _, fs = _window(iq, offset, freq_shift)
    kind = _arr(kind, np.uint8)
    n = kind.size
    out = dict(l2=np.zeros((n, 24), np.uint8), crc=np.zeros(n, np.int32), conv=np.zeros(n, np.int32),
               toa=np.zeros(n, np.float32), freq_err=np.zeros(n, np.float32), rv=np.zeros(n, np.int32))
    eb = np.zeros((n, 432), np.int8) if want_ebits else None
    ss = np.zeros((n, 234), np.float32) if want_ssyms else None
    _call("gmr1_hip_rx_bcch_ccch_batch", n, sps, _p(iq), iq.size, _p(offset), _p(kind), _p(fs),
          _p(out["l2"]), _p(out["crc"]), _p(out["conv"]), _p(out["toa"]), _p(out["freq_err"]), _p(eb), _p(ss),
          _p(out["rv"]))
    out["ebits"], out["ssyms"] = eb, ss
    return out


# ---------------------------------------------------------------------------
# reference-style single-burst calls (the legacy C API, through ctypes)
# ---------------------------------------------------------------------------
def _burst_addr(burst):
    """what goes where C callers write &gmr1_<name>_burst: the exported struct's address, or a CallerBurst's"""
    if isinstance(burst, CallerBurst):
        return burst.address
    return C.addressof(C.c_void_p.in_dll(load(), f"gmr1_{burst}_burst"))


def pi4cxpsk_demod(burst_name, iq, sps=4, freq_shift=0.0):
    """gmr1_pi4cxpsk_demod(&gmr1_<name>_burst, cxvec, ...) exactly as C callers use it; burst_name may also be a
    CallerBurst (the caller's own description of a format)."""
    bt_addr = _burst_addr(burst_name)
    n_eb = int(burst_name.burst.ebits) if isinstance(burst_name, CallerBurst) else burst_info(burst_name).ebits
    iq, vec = _cxvec(iq)
    eb = np.zeros(n_eb, np.int8)
    sid, toa, fe = C.c_int(-1), C.c_float(), C.c_float()
    rv = _fn("gmr1_pi4cxpsk_demod")(bt_addr, C.byref(vec), sps, freq_shift, _p(eb), C.byref(sid), C.byref(toa),
                                    C.byref(fe))
    return dict(rv=rv, ebits=eb, sync_id=sid.value, toa=toa.value, freq_err=fe.value)


def _decode1(fn, ebits):
    ebits = _arr(ebits, np.int8)
    l2 = np.zeros(24, np.uint8)
    cv = C.c_int()
    rv = _fn(fn)(_p(l2), _p(ebits), C.byref(cv))
    return l2, rv, cv.value


def bcch_decode(ebits):
    return _decode1("gmr1_bcch_decode", ebits)


def ccch_decode(ebits):
    return _decode1("gmr1_ccch_decode", ebits)


# ---------------------------------------------------------------------------
# device-pointer calls (torch tensors as plumbing for HBM + streams)
# ---------------------------------------------------------------------------
def rx_bcch_ccch_batch_dev(stream, n, sps, iq, offset, kind, freq_shift, l2, crc, conv, toa, freq_err,
                           ebits, ssyms, rv):
    """All tensor arguments are device pointers (ints) or None."""
    _call("gmr1_hip_rx_bcch_ccch_batch_dev", stream, n, sps, iq, offset, kind, freq_shift, l2, crc, conv, toa,
          freq_err, ebits, ssyms, rv)


def rx_bcch_ccch_batch_planar_dev(stream, n, sps, iq_planes, plane_stride, offset, kind, freq_shift, l2, crc, conv, toa,
                                  freq_err, ebits, ssyms, rv):
    """The same call on a polyphase-planar sample array (include/gmr1_hip.h); device pointers (ints) or None."""
    _call("gmr1_hip_rx_bcch_ccch_batch_planar_dev", stream, n, sps, iq_planes, plane_stride, offset, kind, freq_shift,
          l2, crc, conv, toa, freq_err, ebits, ssyms, rv)


def iq_to_planar_dev(stream, sps, n_samples, iq, iq_planes, plane_stride):
    """Interleaved device sample array -> polyphase-planar (sample s to iq_planes[(s % sps) * plane_stride + s // sps])."""
    _call("gmr1_hip_iq_to_planar_dev", stream, sps, n_samples, iq, iq_planes, plane_stride)


# ---------------------------------------------------------------------------
# FCCH acquisition
# ---------------------------------------------------------------------------
FCCH_TYPES = ["fcch", "fcch3_lband", "fcch3_sband"]
FCCH_LEN = [117, 468, 468]


class FcchBurst(C.Structure):
    """struct gmr1_fcch_burst (include/osmocom/gmr1/sdr/fcch.h)."""
    _fields_ = [("freq", C.c_float), ("len", C.c_int)]


def _fcch_id(t):
    return FCCH_TYPES.index(t) if isinstance(t, str) else int(t)


def fcch_rough_batch(iq, offset, length, sps=4, freq_shift=None, fcch_type="fcch"):
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    toa = np.zeros(n, np.int32)
    rv = np.zeros(n, np.int32)
    _call("gmr1_hip_fcch_rough_batch", _fcch_id(fcch_type), n, sps, length, _p(iq), iq.size, _p(offset), _p(fs),
          _p(toa), _p(rv))
    return toa, rv


def fcch_fine_batch(iq, offset, sps=4, freq_shift=None, fcch_type="fcch"):
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    toa = np.zeros(n, np.int32)
    fe = np.zeros(n, np.float32)
    _call("gmr1_hip_fcch_fine_batch", _fcch_id(fcch_type), n, sps, _p(iq), iq.size, _p(offset), _p(fs), _p(toa), _p(fe))
    return toa, fe


def fcch_snr_batch(iq, offset, sps=4, freq_shift=None, fcch_type="fcch"):
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    snr = np.zeros(n, np.float32)
    _call("gmr1_hip_fcch_snr_batch", _fcch_id(fcch_type), n, sps, _p(iq), iq.size, _p(offset), _p(fs), _p(snr))
    return snr


def _fcch_struct(fcch_type):
    name = {"fcch": "gmr1_fcch_burst", "fcch3_lband": "gmr1_fcch3_lband_burst",
            "fcch3_sband": "gmr1_fcch3_sband_burst"}[fcch_type]
    return C.byref(FcchBurst.in_dll(load(), name))


def fcch_rough(iq, sps=4, freq_shift=0.0, fcch_type="fcch"):
    """gmr1_fcch_rough(&gmr1_fcch_burst, cxvec, sps, freq_shift, &toa): the reference's own call."""
    iq, vec = _cxvec(iq)
    toa = C.c_int()
    rv = _fn("gmr1_fcch_rough")(_fcch_struct(fcch_type), C.byref(vec), sps, freq_shift, C.byref(toa))
    return rv, toa.value


def fcch_fine(iq, sps=4, freq_shift=0.0, fcch_type="fcch"):
    iq, vec = _cxvec(iq)
    toa, fe = C.c_int(), C.c_float()
    rv = _fn("gmr1_fcch_fine")(_fcch_struct(fcch_type), C.byref(vec), sps, freq_shift, C.byref(toa), C.byref(fe))
    return rv, toa.value, fe.value


def fcch_snr(iq, sps=4, freq_shift=0.0, fcch_type="fcch"):
    iq, vec = _cxvec(iq)
    snr = C.c_float()
    rv = _fn("gmr1_fcch_snr")(_fcch_struct(fcch_type), C.byref(vec), sps, freq_shift, C.byref(snr))
    return rv, snr.value


def fcch_rough_batch_dev(stream, fcch_type, n, sps, length, iq, offset, freq_shift, toa, rv):
    _call("gmr1_hip_fcch_rough_batch_dev", stream, _fcch_id(fcch_type), n, sps, length, iq, offset, freq_shift, toa, rv)


ACQ_MAX_CHAINS = 16


class FcchAcq(C.Structure):
    """struct gmr1_hip_fcch_acq (include/gmr1_hip.h)."""
    _fields_ = [("status", C.c_int32), ("n_chains", C.c_int32), ("align", C.c_int32), ("base_align", C.c_int32),
                ("freq_err", C.c_float), ("n_cand", C.c_int32), ("chain_align", C.c_int32 * ACQ_MAX_CHAINS),
                ("chain_freq_err", C.c_float * ACQ_MAX_CHAINS), ("chain_snr", C.c_float * ACQ_MAX_CHAINS)]


# the same layout for arrays of them (FCCH_ACQ.itemsize == ctypes.sizeof(FcchAcq))
FCCH_ACQ = np.dtype([("status", "<i4"), ("n_chains", "<i4"), ("align", "<i4"), ("base_align", "<i4"), ("freq_err", "<f4"),
                     ("n_cand", "<i4"), ("chain_align", "<i4", (ACQ_MAX_CHAINS,)), ("chain_freq_err", "<f4", (ACQ_MAX_CHAINS,)),
                     ("chain_snr", "<f4", (ACQ_MAX_CHAINS,))])


def fcch_acquire(iq, offset, length, sps=4, start=None, fcch_type="fcch"):
    """gmr1_rx's acquisition (fcch_single_init, fcch_multi_process up to its survivor list) of the streams
    iq[offset[i] : offset[i] + length[i]] -> one FCCH_ACQ record each.  start: where each stream's 330 ms window begins
    (None: 8000 everywhere)."""
    iq = _arr(iq, np.complex64, -1)
    offset, length, start = _arr(offset, np.uint64), _arr(length, np.uint64), _arr(start, np.int32)
    out = np.zeros(offset.size, FCCH_ACQ)
    _call("gmr1_hip_fcch_acquire_batch", _fcch_id(fcch_type), offset.size, sps, _p(iq), iq.size, _p(offset), _p(length),
          _p(start), _p(out))
    return out


def fcch_acquire_dev(stream, n, iq, offset, length, out, sps=4, start=None, fcch_type="fcch"):
    """The same on device memory (addresses): enqueues on `stream` and returns; out: n records of FCCH_ACQ.itemsize bytes."""
    _call("gmr1_hip_fcch_acquire_batch_dev", stream, _fcch_id(fcch_type), n, sps, iq, offset, length, start, out)


# ---------------------------------------------------------------------------
# following a voice call (rx_tch3)
# ---------------------------------------------------------------------------
TCH3_OFF, TCH3_DKAB, TCH3_DKAB_MISSING, TCH3_FACCH, TCH3_SPEECH, TCH3_ERR = range(6)


class Tch3State(C.Structure):
    """struct gmr1_hip_tch3_state (include/gmr1_hip.h)."""
    _fields_ = [("active", C.c_int32), ("p", C.c_int32), ("ciph", C.c_int32), ("weak_cnt", C.c_int32),
                ("sync_id", C.c_int32), ("burst_cnt", C.c_int32), ("energy_dkab", C.c_float), ("energy_burst", C.c_float),
                ("bi_fn", C.c_uint32 * 4), ("ebits", C.c_int8 * 416), ("kc", C.c_uint8 * 8)]


class Tch3Frame(C.Structure):
    """struct gmr1_hip_tch3_frame (include/gmr1_hip.h)."""
    _fields_ = [("cls", C.c_uint8), ("type", C.c_uint8), ("len", C.c_uint8), ("ciph", C.c_uint8), ("fn", C.c_uint32),
                ("conv", C.c_int32), ("energy", C.c_float), ("l2", C.c_uint8 * 20), ("pad", C.c_uint8 * 4)]


# the same layouts for arrays of them
TCH3_STATE = np.dtype([("active", "<i4"), ("p", "<i4"), ("ciph", "<i4"), ("weak_cnt", "<i4"), ("sync_id", "<i4"),
                       ("burst_cnt", "<i4"), ("energy_dkab", "<f4"), ("energy_burst", "<f4"), ("bi_fn", "<u4", (4,)),
                       ("ebits", "i1", (416,)), ("kc", "u1", (8,))])
TCH3_FRAME = np.dtype([("cls", "u1"), ("type", "u1"), ("len", "u1"), ("ciph", "u1"), ("fn", "<u4"), ("conv", "<i4"),
                       ("energy", "<f4"), ("l2", "u1", (20,)), ("pad", "u1", (4,))])


def tch3_in_len(sps):
    """The window rx_tch3 cuts for a frame (gmr1_rx.c:549-551): an NT3 burst and sps + sps/2 samples of search room."""
    return 117 * sps + sps + sps // 2


def tch3_state_assign(state, p, ref_energy, index=0):
    """rx_tch3_init on state[index] of a TCH3_STATE array (in place; host arithmetic, needs no device) -> state."""
    assert state.dtype == TCH3_STATE and state.flags.c_contiguous and state.flags.writeable
    _call("gmr1_hip_tch3_state_assign", state.ctypes.data + index * TCH3_STATE.itemsize, p, ref_energy)
    return state


def tch3_state_assign_batch_dev(stream, n, call, p, ref_energy, state):
    """rx_tch3_init on device-resident states (addresses): entry j < n assigns state[call[j]] with p[j], ref_energy[j], in
    the order of j; enqueues on `stream` and returns."""
    _call("gmr1_hip_tch3_state_assign_batch_dev", stream, n, call, p, ref_energy, state)


def tch3_follow(iq, first, offset, freq_shift, fn, state, sps=4, in_len=None):
    """rx_tch3 over the frames of len(first) - 1 calls: call c owns frames first[c] .. first[c+1], frame k's window is
    iq[offset[k] : offset[k] + in_len].  -> (TCH3_FRAME record per frame, the calls' TCH3_STATE after them); `state` itself
    is left as it is."""
    iq = _arr(iq, np.complex64, -1)
    first, offset = _arr(first, np.int32), _arr(offset, np.uint64)
    freq_shift, fn = _arr(freq_shift, np.float32), _arr(fn, np.uint32)
    state = np.array(state, TCH3_STATE, ndmin=1)
    out = np.zeros(offset.size, TCH3_FRAME)
    _call("gmr1_hip_tch3_follow_batch", first.size - 1, sps, tch3_in_len(sps) if in_len is None else in_len, _p(iq), iq.size,
          _p(first), offset.size, _p(offset), _p(freq_shift), _p(fn), _p(state), _p(out))
    return out, state


def tch3_follow_dev(stream, n_calls, n_frames, iq, first, offset, freq_shift, fn, state, out, sps=4, in_len=None):
    """The same on device memory (addresses): enqueues on `stream` and returns; state: n_calls x TCH3_STATE.itemsize bytes,
    updated in place; out: n_frames x TCH3_FRAME.itemsize bytes."""
    _call("gmr1_hip_tch3_follow_batch_dev", stream, n_calls, sps, tch3_in_len(sps) if in_len is None else in_len, iq, first,
          n_frames, offset, freq_shift, fn, state, out)


# ---------------------------------------------------------------------------
# following a circuit-switched data call (rx_tch9)
# ---------------------------------------------------------------------------
TCH9_OFF, TCH9_FACCH9, TCH9_TCH9, TCH9_ERR = range(4)


# struct gmr1_hip_tch9_state and struct gmr1_hip_tch9_frame (include/gmr1_hip.h) for arrays of them
TCH9_STATE = np.dtype([("active", "<i4"), ("n_held", "<i4"), ("kc", "u1", (8,)), ("held", "i1", (1324,))])
TCH9_FRAME = np.dtype([("cls", "u1"), ("type", "u1"), ("len", "u1"), ("crc", "u1"), ("fn", "<u4"), ("conv", "<i4"),
                       ("l2", "u1", (64,)), ("pad", "u1", (4,))])


def tch9_in_len(sps):
    """The window rx_tch9 cuts for a frame (gmr1_rx.c:290-291): an NT9 burst and sps + sps/2 samples of search room."""
    return 351 * sps + sps + sps // 2


def tch9_state_assign(state, index=0):
    """rx_tch9_init on state[index] of a TCH9_STATE array (in place; host arithmetic, needs no device) -> state."""
    assert state.dtype == TCH9_STATE and state.flags.c_contiguous and state.flags.writeable
    _call("gmr1_hip_tch9_state_assign", state.ctypes.data + index * TCH9_STATE.itemsize)
    return state


def tch9_state_assign_batch_dev(stream, n, call, state):
    """rx_tch9_init on device-resident states (addresses): entry j < n assigns state[call[j]]; enqueues on `stream`."""
    _call("gmr1_hip_tch9_state_assign_batch_dev", stream, n, call, state)


def tch9_follow_bits(first, ebits, sync_id, fn, state, rv=None, mode=2):
    """rx_tch9 behind the demodulator over the frames of len(first) - 1 calls: frame k is ebits[k] (662 soft bits),
    sync_id[k], rv[k] (None: all 0), fn[k].  -> (TCH9_FRAME record per frame, the calls' TCH9_STATE after them); `state`
    itself is left as it is."""
    first, ebits = _arr(first, np.int32), _arr(ebits, np.int8, (-1, 662))
    sync_id, rv, fn = _arr(sync_id, np.int32), _arr(rv, np.int32), _arr(fn, np.uint32)
    state = np.array(state, TCH9_STATE, ndmin=1)
    out = np.zeros(ebits.shape[0], TCH9_FRAME)
    _call("gmr1_hip_tch9_follow_bits_batch", first.size - 1, mode, _p(first), ebits.shape[0], _p(ebits), _p(sync_id), _p(rv),
          _p(fn), _p(state), _p(out))
    return out, state


def tch9_follow_bits_dev(stream, n_calls, n_frames, first, ebits, sync_id, rv, fn, state, out, mode=2):
    """The same on device memory (addresses; rv may be None): enqueues on `stream` and returns; state: n_calls x
    TCH9_STATE.itemsize bytes, updated in place; out: n_frames x TCH9_FRAME.itemsize bytes."""
    _call("gmr1_hip_tch9_follow_bits_batch_dev", stream, n_calls, mode, first, n_frames, ebits, sync_id, rv, fn, state, out)


def tch9_follow(iq, first, offset, freq_shift, fn, state, sps=4, in_len=None, mode=2):
    """rx_tch9 from samples: frame k's window is iq[offset[k] : offset[k] + in_len], demodulated as an NT9 burst with
    freq_shift[k].  -> (TCH9_FRAME record per frame, the calls' TCH9_STATE after them)."""
    iq = _arr(iq, np.complex64, -1)
    first, offset = _arr(first, np.int32), _arr(offset, np.uint64)
    freq_shift, fn = _arr(freq_shift, np.float32), _arr(fn, np.uint32)
    state = np.array(state, TCH9_STATE, ndmin=1)
    out = np.zeros(offset.size, TCH9_FRAME)
    _call("gmr1_hip_tch9_follow_batch", first.size - 1, sps, tch9_in_len(sps) if in_len is None else in_len, mode, _p(iq),
          iq.size, _p(first), offset.size, _p(offset), _p(freq_shift), _p(fn), _p(state), _p(out))
    return out, state


def tch9_follow_dev(stream, n_calls, n_frames, iq, first, offset, freq_shift, fn, state, out, sps=4, in_len=None, mode=2):
    """The same on device memory (addresses): enqueues on `stream` and returns."""
    _call("gmr1_hip_tch9_follow_batch_dev", stream, n_calls, sps, tch9_in_len(sps) if in_len is None else in_len, mode, iq,
          first, n_frames, offset, freq_shift, fn, state, out)


# ---------------------------------------------------------------------------
# traffic-channel layer 1
# ---------------------------------------------------------------------------
def facch3_decode_batch(ebits, ciph=None):
    """ebits (n, 4, 104) or (n, 416) int8 -> l2 (n,10), bits_s (n,32), crc, conv."""
    ebits = _arr(ebits, np.int8, (-1, 416))
    n = ebits.shape[0]
    ciph = _arr(ciph, np.uint8)
    l2 = np.zeros((n, 10), np.uint8)
    s = np.zeros((n, 32), np.uint8)
    crc = np.zeros(n, np.int32)
    conv = np.zeros(n, np.int32)
    _call("gmr1_hip_facch3_decode_batch", n, _p(ebits), _p(ciph), _p(l2), _p(s), _p(crc), _p(conv))
    return l2, s, crc, conv


def tch3_decode_batch(ebits, m=0, ciph=None):
    """ebits (n, 212) int8 -> frame0 (n,10), frame1 (n,10), bits_s (n,4), conv0, conv1."""
    ebits = _arr(ebits, np.int8, (-1, 212))
    n = ebits.shape[0]
    ciph = _arr(ciph, np.uint8)
    fr = np.zeros((n, 2, 10), np.uint8)
    s = np.zeros((n, 4), np.uint8)
    conv = np.zeros((n, 2), np.int32)
    _call("gmr1_hip_tch3_decode_batch", n, m, _p(ebits), _p(ciph), _p(fr), _p(s), _p(conv))
    return fr[:, 0], fr[:, 1], s, conv[:, 0], conv[:, 1]


def tch3_rx_batch(iq, offset, in_len, sps=4, freq_shift=None, m=0, ciph=None, want_ebits=True):
    """NT3 speech bursts from samples to speech frames (rx_tch3's demodulate-then-decode, one call):
    dict(rv, sync_id, toa, ebits (n, 212), frame0, frame1, bits_s, conv0, conv1)."""
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    ciph = _arr(ciph, np.uint8)
    eb = np.zeros((n, 212), np.int8) if want_ebits else None
    sid = np.zeros(n, np.int32)
    toa = np.zeros(n, np.float32)
    rv = np.zeros(n, np.int32)
    fr = np.zeros((n, 2, 10), np.uint8)
    st = np.zeros((n, 4), np.uint8)
    conv = np.zeros((n, 2), np.int32)
    _call("gmr1_hip_tch3_rx_batch", n, sps, in_len, _p(iq), iq.size, _p(offset), _p(fs), m, _p(ciph),
          _p(eb), _p(sid), _p(toa), _p(rv), _p(fr), _p(st), _p(conv))
    return dict(rv=rv, sync_id=sid, toa=toa, ebits=eb, frame0=fr[:, 0], frame1=fr[:, 1], bits_s=st, conv0=conv[:, 0],
                conv1=conv[:, 1])


def facch3_decode(ebits):
    """gmr1_facch3_decode(l2, bits_s, bits_e, NULL, &conv): the reference's own call."""
    ebits = _arr(ebits, np.int8, 416)
    l2 = np.zeros(10, np.uint8)
    s = np.zeros(32, np.uint8)
    cv = C.c_int()
    rv = _fn("gmr1_facch3_decode")(_p(l2), _p(s), _p(ebits), None, C.byref(cv))
    return l2, s, rv, cv.value


def tch3_decode(ebits, m=0):
    ebits = _arr(ebits, np.int8, 212)
    f0 = np.zeros(10, np.uint8)
    f1 = np.zeros(10, np.uint8)
    s = np.zeros(4, np.uint8)
    c0, c1 = C.c_int(), C.c_int()
    _fn("gmr1_tch3_decode")(_p(f0), _p(f1), _p(s), _p(ebits), None, m, C.byref(c0), C.byref(c1))
    return f0, f1, s, c0.value, c1.value


# ---------------------------------------------------------------------------
# burst type detection / modulation order
# ---------------------------------------------------------------------------
def detect_batch(bursts, iq, offset, in_len, sps=4, freq_shift=None, e_toa=None):
    ids = np.array([_burst_id(b) for b in bursts], np.int32)
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    et = None if e_toa is None else _arr(np.broadcast_to(np.asarray(e_toa, np.float32), (n,)), np.float32)
    bt = np.zeros(n, np.int32)
    sid = np.zeros(n, np.int32)
    toa = np.zeros(n, np.float32)
    rv = np.zeros(n, np.int32)
    _call("gmr1_hip_detect_batch", ids.size, _p(ids), n, sps, in_len, _p(iq), iq.size, _p(offset), _p(fs), _p(et),
          _p(bt), _p(sid), _p(toa), _p(rv))
    return dict(rv=rv, bt_id=bt, sync_id=sid, toa=toa)


def mod_order_batch(iq, offset, in_len, sps=4, freq_shift=None):
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    order = np.zeros(n, np.int32)
    _call("gmr1_hip_mod_order_batch", n, sps, in_len, _p(iq), iq.size, _p(offset), _p(fs), _p(order))
    return order


class _RefMod(C.Structure):       # struct gmr1_pi4cxpsk_modulation (sdr/pi4cxpsk.h)
    _fields_ = [("rotation", C.c_float), ("nbits", C.c_int), ("syms", C.c_void_p), ("bits", C.c_void_p)]


class _RefSync(C.Structure):      # struct gmr1_pi4cxpsk_sync
    _fields_ = [("pos", C.c_int), ("len", C.c_int), ("syms", C.c_uint8 * 32), ("_ref", C.c_void_p)]


class _RefData(C.Structure):      # struct gmr1_pi4cxpsk_data
    _fields_ = [("pos", C.c_int), ("len", C.c_int)]


class _RefBurst(C.Structure):     # struct gmr1_pi4cxpsk_burst
    _fields_ = [("mod", C.POINTER(_RefMod)), ("guard_pre", C.c_int), ("guard_post", C.c_int),
                ("len", C.c_int), ("ebits", C.c_int), ("sync", C.POINTER(_RefSync) * 4),
                ("data", C.POINTER(_RefData))]


class CallerBurst:
    """A caller-defined `struct gmr1_pi4cxpsk_burst` (the reference lets applications describe their own burst formats
    and pass them to gmr1_pi4cxpsk_demod / _detect): a deep copy of an exported one in memory of our own, optionally
    edited.  `.address` is what goes where `&gmr1_xyz_burst` would."""

    def __init__(self, like: str):
        src = _RefBurst.in_dll(load(), f"gmr1_{like}_burst")
        self.burst = _RefBurst()
        self.burst.mod = src.mod                       # the modulation objects are the library's (as in the reference)
        self.burst.guard_pre, self.burst.guard_post = src.guard_pre, src.guard_post
        self.burst.len, self.burst.ebits = src.len, src.ebits
        self._keep = []
        for k in range(4):
            if not src.sync[k]:
                break
            n = 0
            while src.sync[k][n].pos >= 0:
                n += 1
            arr = (_RefSync * (n + 1))()
            for i in range(n):
                arr[i].pos, arr[i].len = src.sync[k][i].pos, src.sync[k][i].len
                C.memmove(arr[i].syms, src.sync[k][i].syms, 32)
            arr[n].pos = -1
            self._keep.append(arr)
            self.burst.sync[k] = C.cast(arr, C.POINTER(_RefSync))
        n = 0
        while src.data[n].pos >= 0:
            n += 1
        d = (_RefData * (n + 1))()
        for i in range(n):
            d[i].pos, d[i].len = src.data[i].pos, src.data[i].len
        d[n].pos = -1
        self._keep.append(d)
        self.burst.data = C.cast(d, C.POINTER(_RefData))

    @property
    def address(self):
        return C.addressof(self.burst)


def pi4cxpsk_detect(burst_names, e_toa, iq, sps=4, freq_shift=0.0):
    """gmr1_pi4cxpsk_detect({&gmr1_a_burst, &gmr1_b_burst, NULL}, e_toa, cxvec, ...) as C callers use it; an entry
    may also be a CallerBurst (a description of the caller's own)."""
    arr = (C.c_void_p * (len(burst_names) + 1))(*[_burst_addr(nm) for nm in burst_names], None)
    iq, vec = _cxvec(iq)
    bt, sid, toa = C.c_int(-1), C.c_int(-1), C.c_float()
    rv = _fn("gmr1_pi4cxpsk_detect")(arr, e_toa, C.byref(vec), sps, freq_shift, C.byref(bt), C.byref(sid), C.byref(toa))
    return dict(rv=rv, bt_id=bt.value, sync_id=sid.value, toa=toa.value)


def pi4cxpsk_mod_order(iq, sps=4, freq_shift=0.0):
    iq, vec = _cxvec(iq)
    return _fn("gmr1_pi4cxpsk_mod_order")(C.byref(vec), sps, freq_shift)


def fcch_rough_multi_batch(iq, offset, length, sps=4, freq_shift=None, N=16, fcch_type="fcch"):
    iq, offset, n, fs = _window(iq, offset, freq_shift)
    toa = np.zeros((n, N), np.int32)
    cnt = np.zeros(n, np.int32)
    _call("gmr1_hip_fcch_rough_multi_batch", _fcch_id(fcch_type), n, sps, length, _p(iq), iq.size, _p(offset), _p(fs),
          _p(toa), N, _p(cnt))
    return cnt, toa


def fcch_rough_multi(iq, sps=4, freq_shift=0.0, N=16, fcch_type="fcch"):
    iq, vec = _cxvec(iq)
    toa = np.zeros(N, np.int32)
    rv = _fn("gmr1_fcch_rough_multi")(_fcch_struct(fcch_type), C.byref(vec), sps, freq_shift, _p(toa), N)
    return rv, toa[:max(rv, 0)].copy()


# ---------------------------------------------------------------------------
# gmr1_rx receive loop over many BCCH carriers (reference src/gmr1_rx.c:605-895)
# ---------------------------------------------------------------------------
RX_RECORD = np.dtype([("arfcn", "<u2"), ("chain", "u1"), ("type", "u1"), ("fn", "<u4"),
                      ("tn", "u1"), ("crc", "u1"), ("len", "u1"), ("pad", "u1"),
                      ("conv", "<i4"), ("l2", "u1", (24,))])
assert RX_RECORD.itemsize == 40


def _records(out, max_records, dtype=RX_RECORD):
    """The record buffer of a receive-loop call: the caller's own array (checked) or a fresh one -> (array, its capacity)"""
    if out is None:
        return np.empty(max(max_records, 1), dtype), max_records   # only the records written are handed back
    if out.dtype != dtype or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous RX_RECORD array")
    return out, out.size


_NO_KC = object()


def _rx_loop(fname, head, offset, length, arfcn, out_ptr, max_records, kc=_NO_KC, big=(), tail=()):
    """The one marshalling of every receive-loop entry (gmr1_hip_rx_run*).  `head` is what the entry takes before offset /
    length / arfcn, `kc` the (n, 8) keys or None where it takes them, `big` and `tail` what follows the record count and
    the n_chains array.  Everything is converted here, once -> (run, n_rec, status[n], n_chains[n]): run() is the bare
    C call and returns its code, n_rec.value is then the number of records found."""
    n = len(offset)
    offset, length, arfcn = _arr(offset, np.uint64), _arr(length, np.uint64), _arr(arfcn, np.uint16)
    if kc is not _NO_KC:
        kc = None if kc is None else _arr(np.broadcast_to(np.asarray(kc, np.uint8).reshape(-1, 8), (n, 8)), np.uint8)
    n_rec = C.c_int(0)
    status = np.zeros(max(n, 1), np.int32)
    chains = np.zeros(max(n, 1), np.int32)
    f = _fn(fname)
    args = (*head, _p(offset), _p(length), _p(arfcn), *(() if kc is _NO_KC else (_p(kc),)), out_ptr, max_records,
            C.addressof(n_rec), *big, _p(status), _p(chains), *tail)
    run = functools.partial(f, *(t(a) for t, a in zip(f.argtypes, args, strict=True)))
    run.keep = (offset, length, arfcn, kc)      # the arrays the pointers point into
    return run, n_rec, status[:n], chains[:n]


def rx_run(iq, offset, length, sps=4, arfcn=None, max_records=1 << 16):
    """gmr1_hip_rx_run: iq is one host complex64 buffer holding every carrier; carrier i is
    iq[offset[i] : offset[i] + length[i]].  Returns (records RX_RECORD[], status[n], n_chains[n], n_found)."""
    iq = _arr(iq, np.complex64, -1)
    out, cap = _records(None, max_records)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run", (len(offset), sps, _p(iq), iq.size), offset, length, arfcn,
                                          _p(out), cap)
    _check(run(), "gmr1_hip_rx_run")
    return out[:min(n_rec.value, cap)].copy(), status, chains, n_rec.value


def rx_run_dev(stream, iq_ptr, offset, length, sps=4, arfcn=None, max_records=1 << 16, out=None):
    """gmr1_hip_rx_run_dev: as rx_run with the capture already in HBM (iq_ptr = device address).
    out: optional preallocated RX_RECORD array the records are written into (a view of it is returned)."""
    reuse = out is not None
    out, cap = _records(out, max_records)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_dev", (stream, len(offset), sps, iq_ptr), offset, length,
                                          arfcn, _p(out), cap)
    _check(run(), "gmr1_hip_rx_run_dev")
    got = out[:min(n_rec.value, cap)]
    return (got if reuse else got.copy()), status, chains, n_rec.value


def rx_run_dev_prepared(stream, iq_ptr, offset, length, out, sps=4, arfcn=None):
    """gmr1_hip_rx_run_dev with every argument marshalled ONCE: returns call() -> (records view, status, n_chains, n_found).
    What a C host pays per call is the call itself; a Python caller that repeats the same call (bench.py) should not time
    its own argument conversion either."""
    out, cap = _records(out, 0)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_dev", (stream, len(offset), sps, iq_ptr), offset, length,
                                          arfcn, _p(out), cap)

    def call():
        rc = run()
        if rc:
            _check(rc, "gmr1_hip_rx_run_dev")
        return out[:min(n_rec.value, cap)], status, chains, n_rec.value
    call.keep = run.keep
    return call


def rx_run_last_timing():
    """Phases of this thread's last rx_run* call in ms: acquisition, frame loop (kernels), records hand-back, host work around
    the loop, traffic-channel passes."""
    us = (C.c_double * 5)()
    _call("gmr1_hip_rx_run_last_timing", us)
    return dict(zip(("acquisition_ms", "chain_ms", "handback_ms", "host_ms", "traffic_passes_ms"), [v / 1e3 for v in us]))


def rx_run_dev_raw(stream, iq_ptr, offset, length, out_ptr, max_records, sps=4, arfcn=None):
    """gmr1_hip_rx_run_dev with the record buffer given as an address -- device memory or pinned host memory, which the
    library copies into directly.  Returns (n_found, status[n], n_chains[n])."""
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_dev", (stream, len(offset), sps, iq_ptr), offset, length,
                                          arfcn, out_ptr, max_records)
    _check(run(), "gmr1_hip_rx_run_dev")
    return n_rec.value, status, chains


def _gsmtap(fname, record, dtype, with_arfcn, size):
    rec = _arr(record, dtype, 1)
    buf = (C.c_uint8 * size)()
    n = _fn(fname)(_p(rec), 1 if with_arfcn else 0, buf, size)
    if n < 0:
        _check(n, fname)
    return bytes(buf[:n])


def gsmtap_pack(record, with_arfcn=False) -> bytes:
    """gmr1_hip_gsmtap_pack: the GSMTAP packet the reference would send for one RX_RECORD (src/gsmtap.c:43-71)."""
    return _gsmtap("gmr1_hip_gsmtap_pack", record, RX_RECORD, with_arfcn, 64)


# ---------------------------------------------------------------------------
# TCH3 follow-up pieces: DKAB demodulator, A5 keystream
# ---------------------------------------------------------------------------
def dkab_demod_batch(iq, offset, in_len, p, sps=4, freq_shift=None):
    """gmr1_hip_dkab_demod_batch -> (rv[n], ebits[n, 8], toa[n])"""
    iq, offset, n, fs = _window(iq, offset, freq_shift, broadcast=True)
    p = _arr(np.broadcast_to(np.asarray(p, np.int32), (n,)), np.int32)
    eb = np.zeros((n, 8), np.int8)
    toa = np.zeros(n, np.float32)
    rv = np.zeros(n, np.int32)
    _call("gmr1_hip_dkab_demod_batch", n, sps, in_len, _p(iq), iq.size, _p(offset), _p(fs), _p(p), _p(eb), _p(toa),
          _p(rv))
    return rv, eb, toa


def dkab_demod(iq, sps=4, freq_shift=0.0, p=0):
    """gmr1_dkab_demod, the reference's own call -> (rv, ebits[8], toa)"""
    iq, vec = _cxvec(iq)
    eb = np.zeros(8, np.int8)
    toa = C.c_float(0.0)
    rv = _fn("gmr1_dkab_demod")(C.byref(vec), sps, freq_shift, p, _p(eb), C.byref(toa))
    if rv < 0:
        _check(rv, "gmr1_dkab_demod")
    return rv, eb, toa.value


def a5_batch(alg, keys, fn, nbits, want_ul=False):
    """gmr1_hip_a5_batch: keys (n, 8) or (8,), fn (n,) -> dl (n, nbits) [, ul]"""
    fn = _arr(np.atleast_1d(fn), np.uint32)
    n = fn.size
    keys = _arr(np.broadcast_to(np.asarray(keys, np.uint8).reshape(-1, 8), (n, 8)), np.uint8)
    dl = np.zeros((n, nbits), np.uint8)
    ul = np.zeros((n, nbits), np.uint8) if want_ul else None
    _call("gmr1_hip_a5_batch", n, alg, nbits, _p(keys), _p(fn), _p(dl), _p(ul))
    return (dl, ul) if want_ul else dl


def a5(n, key, fn, nbits):
    """gmr1_a5, the reference's own call -> (dl, ul)"""
    key = _arr(key, np.uint8)
    dl = np.full(nbits, 0xEE, np.uint8)
    ul = np.full(nbits, 0xEE, np.uint8)
    _fn("gmr1_a5")(n, _p(key), int(fn), nbits, _p(dl), _p(ul))
    return dl, ul


def _same_size(x, iq):
    """an optional carrier set laid out like iq"""
    x = _arr(x, np.complex64, -1)
    assert x is None or x.size == iq.size
    return x


def rx_run_tch(iq, tch, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16):
    """gmr1_hip_rx_run_tch: rx_run with the traffic carriers `tch` (same layout as iq) and keys kc (n, 8)."""
    iq = _arr(iq, np.complex64, -1)
    tch = _same_size(tch, iq)
    out, cap = _records(None, max_records)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_tch", (len(offset), sps, _p(iq), _p(tch), iq.size), offset,
                                          length, arfcn, _p(out), cap, kc=kc)
    _check(run(), "gmr1_hip_rx_run_tch")
    return out[:min(n_rec.value, cap)].copy(), status, chains, n_rec.value


def rx_run_tch_dev(stream, iq_ptr, tch_ptr, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16):
    """gmr1_hip_rx_run_tch_dev: rx_run_tch with both captures already in HBM (device addresses, same layout)."""
    out, cap = _records(None, max_records)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_tch_dev", (stream, len(offset), sps, iq_ptr, tch_ptr), offset,
                                          length, arfcn, _p(out), cap, kc=kc)
    _check(run(), "gmr1_hip_rx_run_tch_dev")
    return out[:min(n_rec.value, cap)].copy(), status, chains, n_rec.value


# struct gmr1_hip_rx_audio: 40 ms of a followed call's audio, one block per frame the follower walked with the call running
RX_AUDIO = np.dtype([("arfcn", "<u2"), ("chain", "u1"), ("cls", "u1"), ("fn", "<u4"), ("tn", "u1"), ("call", "u1"),
                     ("rv", "<i2", (2,)), ("pad", "u1", (2,)), ("pcm", "<i2", (320,))])
assert RX_AUDIO.itemsize == 656 and RX_AUDIO.fields["pcm"][1] == 16


def rx_run_voice(iq, tch, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16, max_audio=1 << 12):
    """gmr1_hip_rx_run_voice: rx_run_tch with the followed calls decoded to audio
    -> (records, audio RX_AUDIO[], status, n_chains, n_records found, n_audio found)"""
    iq = _arr(iq, np.complex64, -1)
    tch = _same_size(tch, iq)
    out, cap = _records(None, max_records)
    audio, cap_audio = _records(None, max_audio, RX_AUDIO)
    n_audio = C.c_int(0)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_voice", (len(offset), sps, _p(iq), _p(tch), iq.size), offset,
                                          length, arfcn, _p(out), cap, kc=kc, tail=(_p(audio), cap_audio, C.addressof(n_audio)))
    _check(run(), "gmr1_hip_rx_run_voice")
    return (out[:min(n_rec.value, cap)].copy(), audio[:min(n_audio.value, cap_audio)].copy(), status, chains, n_rec.value,
            n_audio.value)


def rx_run_voice_dev(stream, iq_ptr, tch_ptr, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16, max_audio=1 << 12):
    """gmr1_hip_rx_run_voice_dev: rx_run_voice with both captures already in HBM (device addresses, same layout)."""
    out, cap = _records(None, max_records)
    audio, cap_audio = _records(None, max_audio, RX_AUDIO)
    n_audio = C.c_int(0)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_voice_dev", (stream, len(offset), sps, iq_ptr, tch_ptr), offset,
                                          length, arfcn, _p(out), cap, kc=kc, tail=(_p(audio), cap_audio, C.addressof(n_audio)))
    _check(run(), "gmr1_hip_rx_run_voice_dev")
    return (out[:min(n_rec.value, cap)].copy(), audio[:min(n_audio.value, cap_audio)].copy(), status, chains, n_rec.value,
            n_audio.value)


# ---------------------------------------------------------------------------
# wideband -> per-ARFCN channelizer (reference utils/gmr1_rx_sdr.py:391-602)
# ---------------------------------------------------------------------------
def channelize_plan(samp_rate, sps, n_in):
    """-> (n_chans, samples per 2x oversampled channel stream, output samples per channel)"""
    nch, nm, no = C.c_int32(), C.c_uint64(), C.c_uint64()
    _call("gmr1_hip_channelize_plan", samp_rate, sps, n_in, C.byref(nch), C.byref(nm), C.byref(no))
    return nch.value, nm.value, no.value


def channelize(wide, samp_rate, channels, sps=4, rotation=0.0):
    """gmr1_hip_channelize: host wideband complex64 -> (len(channels), n_out) complex64"""
    wide = _arr(wide, np.complex64, -1)
    ch = _arr(channels, np.int32)
    _, _, n_out = channelize_plan(samp_rate, sps, wide.size)
    out = np.zeros((ch.size, n_out), np.complex64)
    no = C.c_uint64()
    _call("gmr1_hip_channelize", samp_rate, sps, _p(wide), wide.size, rotation, ch.size, _p(ch), _p(out), n_out,
          C.byref(no))
    return out


def ddc_plan(samp_rate, sps, n_in):
    """gmr1_hip_ddc_plan -> (decim1, decim2, resamp, n_out) of the recorder script's direct mode."""
    d1, d2, rs, n_out = C.c_int32(), C.c_int32(), C.c_double(), C.c_uint64()
    _call("gmr1_hip_ddc_plan", samp_rate, sps, n_in, C.byref(d1), C.byref(d2), C.byref(rs), C.byref(n_out))
    return d1.value, d2.value, rs.value, n_out.value


def ddc(wide, samp_rate, freqs_hz, sps=4):
    """gmr1_hip_ddc: wide (complex64, host) -> array (len(freqs_hz), n_out) complex64."""
    wide = _arr(wide, np.complex64, -1)
    freqs = _arr(freqs_hz, np.float64)
    _, _, _, n_out = ddc_plan(samp_rate, sps, wide.size)
    out = np.zeros((freqs.size, max(n_out, 1)), np.complex64)
    got = C.c_uint64()
    _call("gmr1_hip_ddc", samp_rate, sps, _p(wide), wide.size, freqs.size, _p(freqs), _p(out), out.shape[1],
          C.byref(got))
    return out[:, :got.value]


def ddc_dev(stream, wide_ptr, n_in, samp_rate, freqs_hz, out_ptr, out_stride, sps=4):
    freqs = _arr(freqs_hz, np.float64)
    got = C.c_uint64()
    _call("gmr1_hip_ddc_dev", stream, samp_rate, sps, wide_ptr, n_in, freqs.size, _p(freqs), out_ptr, out_stride,
          C.byref(got))
    return got.value


def channelize_dev(stream, wide_ptr, n_in, samp_rate, channels, out_ptr, out_stride, sps=4, rotation=0.0):
    ch = _arr(channels, np.int32)
    no = C.c_uint64()
    _call("gmr1_hip_channelize_dev", stream, samp_rate, sps, wide_ptr, n_in, rotation, ch.size, _p(ch), out_ptr,
          out_stride, C.byref(no))
    return no.value


def channelize_planar_dev(stream, wide_ptr, n_in, samp_rate, channels, out_ptr, out_stride, plane_stride, sps=4, rotation=0.0):
    """gmr1_hip_channelize_planar_dev: the streams written polyphase-planar (sample m of stream i at flat index
    g = i * out_stride + m -> out[(g % sps) * plane_stride + g // sps])."""
    ch = _arr(channels, np.int32)
    no = C.c_uint64()
    _call("gmr1_hip_channelize_planar_dev", stream, samp_rate, sps, wide_ptr, n_in, rotation, ch.size, _p(ch), out_ptr,
          out_stride, plane_stride, C.byref(no))
    return no.value


# the same on captures as radios and archives hold them (gmr1_hip.h: GMR1_HIP_IQ_*)
IQ_F32, IQ_S16, IQ_S8 = 0, 1, 2
_IQ_DTYPES = {IQ_S16: np.int16, IQ_S8: np.int8}


def iq_sample_bytes(fmt):
    """gmr1_hip_iq_sample_bytes: bytes per complex sample of a format (no device needed)"""
    n = _fn("gmr1_hip_iq_sample_bytes")(fmt)
    if n < 0:
        raise Gmr1HipError(f"gmr1_hip_iq_sample_bytes failed with {n}: fmt={fmt}")
    return n


def _iq(wide, fmt=None):
    """a host capture and its format: (n, 2) int16 / int8 arrays are S16 / S8 (the format is the dtype's), anything else
    complex64; fmt given: the array must be of that format -> (array, fmt, complex samples)"""
    a = np.asarray(wide)
    got = next((f for f, dt in _IQ_DTYPES.items() if a.dtype == dt), IQ_F32)
    if fmt is not None and fmt != got:
        raise TypeError("a format %d capture, not dtype %s" % (fmt, a.dtype))
    if got == IQ_F32:
        a = _arr(a, np.complex64, -1)
        return a, got, a.size
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("an integer capture is an (n, 2) array of I, Q, not shape %s" % (a.shape,))
    a = np.ascontiguousarray(a)
    return a, got, a.shape[0]


def channelize_iq(wide, samp_rate, channels, sps=4, rotation=0.0):
    """gmr1_hip_channelize_iq: host capture, (n, 2) int16 / int8 or complex64 -> (len(channels), n_out) complex64"""
    wide, fmt, n = _iq(wide)
    ch = _arr(channels, np.int32)
    _, _, n_out = channelize_plan(samp_rate, sps, n)
    out = np.zeros((ch.size, n_out), np.complex64)
    no = C.c_uint64()
    _call("gmr1_hip_channelize_iq", samp_rate, sps, fmt, _p(wide), n, rotation, ch.size, _p(ch), _p(out), n_out, C.byref(no))
    return out


def ddc_iq(wide, samp_rate, freqs_hz, sps=4):
    """gmr1_hip_ddc_iq: host capture, (n, 2) int16 / int8 or complex64 -> (len(freqs_hz), n_out) complex64"""
    wide, fmt, n = _iq(wide)
    freqs = _arr(freqs_hz, np.float64)
    _, _, _, n_out = ddc_plan(samp_rate, sps, n)
    out = np.zeros((freqs.size, max(n_out, 1)), np.complex64)
    got = C.c_uint64()
    _call("gmr1_hip_ddc_iq", samp_rate, sps, fmt, _p(wide), n, freqs.size, _p(freqs), _p(out), out.shape[1], C.byref(got))
    return out[:, :got.value]


def channelize_iq_dev(stream, fmt, wide_ptr, n_in, samp_rate, channels, out_ptr, out_stride, sps=4, rotation=0.0):
    ch = _arr(channels, np.int32)
    no = C.c_uint64()
    _call("gmr1_hip_channelize_iq_dev", stream, samp_rate, sps, fmt, wide_ptr, n_in, rotation, ch.size, _p(ch), out_ptr,
          out_stride, C.byref(no))
    return no.value


def channelize_planar_iq_dev(stream, fmt, wide_ptr, n_in, samp_rate, channels, out_ptr, out_stride, plane_stride, sps=4,
                             rotation=0.0):
    ch = _arr(channels, np.int32)
    no = C.c_uint64()
    _call("gmr1_hip_channelize_planar_iq_dev", stream, samp_rate, sps, fmt, wide_ptr, n_in, rotation, ch.size, _p(ch), out_ptr,
          out_stride, plane_stride, C.byref(no))
    return no.value


def ddc_iq_dev(stream, fmt, wide_ptr, n_in, samp_rate, freqs_hz, out_ptr, out_stride, sps=4):
    freqs = _arr(freqs_hz, np.float64)
    got = C.c_uint64()
    _call("gmr1_hip_ddc_iq_dev", stream, samp_rate, sps, fmt, wide_ptr, n_in, freqs.size, _p(freqs), out_ptr, out_stride,
          C.byref(got))
    return got.value


class _LibHandle(_Handle):
    """an opaque handle the library made (self._h), given back to `_destroy_fn` once"""

    def _destroy(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            _call(self._destroy_fn, h)


class ChanStream(_LibHandle):
    """gmr1_hip_chan_stream_*: the channelizer (or, from ChanStream.direct, the direct mode) over a capture pushed piece
    by piece.  Each push returns the outputs that have become computable; all pushes' outputs, concatenated per stream, are
    identical to one channelize() / ddc() call on the samples pushed so far.  fmt: what the pushes hold (IQ_F32, IQ_S16,
    IQ_S8), for the handle's life."""
    _destroy_fn = "gmr1_hip_chan_stream_destroy"

    def __init__(self, samp_rate, channels, sps=4, rotation=0.0, _handle=None, _n_sel=None, fmt=IQ_F32):
        self._h = C.c_void_p()
        self.fmt = fmt
        if _handle is not None:
            self._h, self.n_sel = _handle, _n_sel
            return
        ch = _arr(channels, np.int32)
        _call("gmr1_hip_channelize_stream_create_iq", samp_rate, sps, fmt, rotation, ch.size, _p(ch), C.byref(self._h))
        self.n_sel = ch.size

    @classmethod
    def direct(cls, samp_rate, freqs_hz, sps=4, fmt=IQ_F32):
        """gmr1_hip_ddc_stream_create_iq: the recorder script's direct mode, carriers at freqs_hz from the centre."""
        freqs = _arr(freqs_hz, np.float64)
        h = C.c_void_p()
        _call("gmr1_hip_ddc_stream_create_iq", samp_rate, sps, fmt, freqs.size, _p(freqs), C.byref(h))
        return cls(None, None, _handle=h, _n_sel=freqs.size, fmt=fmt)

    def out_len(self, n_in):
        """outputs per stream the next push of n_in samples will give"""
        n = C.c_uint64()
        _call("gmr1_hip_chan_stream_out_len", self._h, n_in, C.byref(n))
        return n.value

    def push(self, wide):
        """host samples in the handle's format (complex64, or (n, 2) int16 / int8) -> (n_sel, n_new) complex64"""
        wide, _, n = _iq(wide, self.fmt)
        n_new = self.out_len(n)
        out = np.zeros((self.n_sel, max(n_new, 1)), np.complex64)
        got = C.c_uint64()
        _call("gmr1_hip_chan_stream_push_iq", self._h, _p(wide), n, _p(out), out.shape[1], C.byref(got))
        return out[:, :got.value]

    def push_dev(self, stream, wide_ptr, n_in, out_ptr, out_stride):
        """device pointers (wide in the handle's format), enqueued on `stream` (not waited for) -> outputs written per stream"""
        got = C.c_uint64()
        _call("gmr1_hip_chan_stream_push_iq_dev", stream, self._h, wide_ptr, n_in, out_ptr, out_stride, C.byref(got))
        return got.value


class RxStream(_LibHandle):
    """gmr1_hip_rx_stream_*: the receive loop (rx_run) over a capture pushed piece by piece.  Each push returns the records
    that became final in it; all pushes' records up to the `last` one, stable-sorted by (carrier, chain), are identical to
    one rx_run() call on the whole capture.  tch=True: the loop also follows TCH3 calls (rx_run_tch with the same kc) --
    every push then takes the traffic carriers' samples as well.  full=True: it follows TCH3 and TCH9 calls (rx_run_full
    with the same kc) -- every push takes the traffic and the CSD carriers' samples and returns (records, big records).
    voice=True: it follows TCH3 calls and decodes them (rx_run_voice with the same kc) -- every push takes the traffic
    carriers' samples and returns (records, audio blocks (RX_AUDIO[])).  What was asked for is `kind` ("plain", "tch",
    "full", "voice"); everything below asks _RX_STREAM_KINDS[kind] (beside RX_BIG_RECORD, whose dtype it holds)."""
    _destroy_fn = "gmr1_hip_rx_stream_destroy"

    def __init__(self, n_arfcn, sps=4, arfcn=None, tch=False, kc=None, full=False, voice=False):
        self._h = C.c_void_p()
        self.n = int(n_arfcn)
        if full and voice:
            raise ValueError("a handle is made with full=True or with voice=True, not both")
        self.kind = "full" if full else "voice" if voice else "tch" if tch else "plain"
        self._k = _RX_STREAM_KINDS[self.kind]
        self._arfcn = _arr(arfcn, np.uint16)
        if not self.tch and kc is not None:
            raise ValueError("kc belongs to a handle that follows TCH3 calls (tch=True)")
        kc = _arr(kc, np.uint8, (self.n, 8))        # (held here until the create entry has copied the keys)
        _call(self._k.create, self.n, sps, _p(self._arfcn), *((_p(kc),) if self.tch else ()), C.byref(self._h))

    tch = property(lambda self: self._k.planes > 1, doc="follows TCH3 calls: a tch, full or voice handle")
    full = property(lambda self: self.kind == "full")
    voice = property(lambda self: self.kind == "voice")

    def _max(self, fname, n):
        m = C.c_int()
        _call(fname, self._h, n, C.byref(m))
        return m.value

    def max_records(self, n):
        """the most records the next push of n samples per carrier can return"""
        return self._max("gmr1_hip_rx_stream_max_records", n)

    def max_big(self, n):
        """the most big records the next push of n samples per carrier can return (0 unless full=True)"""
        return self._max("gmr1_hip_rx_stream_max_big", n)

    def max_audio(self, n):
        """the most audio blocks the next push of n samples per carrier can return (0 unless voice=True)"""
        return self._max("gmr1_hip_rx_stream_max_audio", n)

    def _out(self, n, out):
        return _records(out, self.max_records(n))[0]

    def _extra(self, n, given):
        """the second array a push of n fills, the caller's own (checked) or a fresh one; None for a kind that has none"""
        if self._k.extra is None:
            return None
        return _records(given, self._max(self._k.max_extra, n), self._k.extra)[0]

    def _kind(self, tch, csd=None):
        if self.tch and tch is None:
            raise ValueError("a handle that follows TCH3 calls takes the traffic carriers' samples with every push (tch=)")
        if not self.tch and tch is not None:
            raise ValueError("tch= belongs to a handle made with tch=True")
        if self.full and csd is None:
            raise ValueError("a handle that follows TCH9 calls takes the CSD carriers' samples with every push (csd=)")
        if not self.full and csd is not None:
            raise ValueError("csd= belongs to a handle made with full=True")

    def _push(self, fname, head, chunks, stride, n, last, out_ptr, max_records, extra=None):
        """The one marshalling of every push entry: `head` is what the entry takes before the handle, `chunks` the addresses
        of iq, tch and csd (as many as the entry takes), `extra` its second array or None -> (records, extra entries) written"""
        got, got_extra = C.c_int(), C.c_int()
        tail = () if extra is None else (extra.ctypes.data, extra.size, C.byref(got_extra))
        _call(fname, *head, self._h, *chunks, stride, n, 1 if last else 0, out_ptr, max_records, C.byref(got), *tail)
        return got.value, got_extra.value

    def push(self, iq, last=False, out=None, tch=None, csd=None):
        """host (n_arfcn, n) complex64 (and, on a tch handle, tch of the same shape; on a full handle csd as well) -> the
        records that became final (RX_RECORD[]); on a full handle (records, big records (RX_BIG_RECORD[])); on a voice handle
        (records, audio blocks (RX_AUDIO[]))"""
        self._kind(tch, csd)
        iq = _arr(iq, np.complex64, (self.n, -1))
        n = iq.shape[1]
        out = self._out(n, out)
        chunks = [iq] + [_arr(x, np.complex64, (self.n, n)) for x in (tch, csd)[:self._k.planes - 1]]
        extra = self._extra(n, None)
        got, got_extra = self._push(self._k.push, (), [_p(x) for x in chunks], n, n, last, _p(out), out.size, extra)
        return out[:got] if extra is None else (out[:got], extra[:got_extra])

    def push_dev(self, stream, iq_ptr, iq_stride, n, last=False, out=None, tch_ptr=None, csd_ptr=None, big=None, audio=None):
        """device samples (carrier i at iq_ptr + 8 * i * iq_stride; on a tch handle its traffic samples at tch_ptr + 8 * i *
        iq_stride, on a full handle its CSD samples at csd_ptr + 8 * i * iq_stride), read on `stream` -> the records
        (synchronous); on a full handle (records, big records), on a voice handle (records, audio blocks).
        out, big, audio: host RX_RECORD / RX_BIG_RECORD / RX_AUDIO arrays, or None; out_ptr (device / pinned) goes through
        push_dev_raw.  (csd_ptr, big and audio are looked at only on a handle that takes them.)"""
        out = self._out(n, out)
        self._kind(tch_ptr, csd_ptr if self.full else None)
        extra = self._extra(n, {"big": big, "audio": audio}.get(self._k.extra_arg))
        got, got_extra = self._push(self._k.push_dev, (stream,), (iq_ptr, tch_ptr, csd_ptr)[:self._k.planes], iq_stride, n, last,
                                    out.ctypes.data, out.size, extra)
        return out[:got] if extra is None else (out[:got], extra[:got_extra])

    def push_dev_raw(self, stream, iq_ptr, iq_stride, n, last, out_ptr, max_records, tch_ptr=None):
        """gmr1_hip_rx_stream_push_dev with a caller's record buffer (any memory rx_run_dev takes) -> records written; on a
        tch handle gmr1_hip_rx_stream_push_tch_dev, whose record buffer is host memory.  (A full or a voice handle has no raw
        form: the tch entry refuses it.)"""
        self._kind(tch_ptr)
        k = self._k if self._k.extra is None else _RX_STREAM_KINDS["tch"]
        return self._push(k.push_dev, (stream,), (iq_ptr, tch_ptr)[:k.planes], iq_stride, n, last, out_ptr, max_records)[0]

    def status(self):
        """(status[n], n_chains[n], retained[n]) per carrier"""
        st = np.zeros(self.n, np.int32)
        nc = np.zeros(self.n, np.int32)
        ret = np.zeros(self.n, np.uint64)
        _call("gmr1_hip_rx_stream_status", self._h, _p(st), _p(nc), _p(ret))
        return st, nc, ret


# ---------------------------------------------------------------------------
# NT9 bursts: FACCH9, TCH9
# ---------------------------------------------------------------------------
TCH9_BYTES = (18, 30, 60)


def facch9_decode_batch(ebits, ciph=None):
    """(n, 662) soft bits -> (l2 (n, 38), sacch (n, 10), status (n, 4), crc (n,), conv (n,))"""
    eb = _arr(ebits, np.int8)
    n = eb.shape[0]
    ciph = _arr(ciph, np.uint8)
    l2 = np.zeros((n, 38), np.uint8)
    sa = np.zeros((n, 10), np.int8)
    stt = np.zeros((n, 4), np.int8)
    crc = np.zeros(n, np.int32)
    conv = np.zeros(n, np.int32)
    _call("gmr1_hip_facch9_decode_batch", n, _p(eb), _p(ciph), _p(l2), _p(sa), _p(stt), _p(crc), _p(conv))
    return l2, sa, stt, crc, conv


def facch9_decode(ebits, ciph=None):
    """gmr1_facch9_decode, the reference's own call -> (l2, sacch, status, crc, conv)"""
    eb = _arr(ebits, np.int8)
    ciph = _arr(ciph, np.uint8)
    l2 = np.zeros(38, np.uint8)
    sa = np.zeros(10, np.int8)
    stt = np.zeros(4, np.int8)
    conv = C.c_int(0)
    crc = _fn("gmr1_facch9_decode")(_p(l2), _p(sa), _p(stt), _p(eb), _p(ciph), C.byref(conv))
    if crc < 0:
        _check(crc, "gmr1_facch9_decode")
    return l2, sa, stt, crc, conv.value


class Interleaver(C.Structure):
    """struct gmr1_interleaver (include/osmocom/gmr1/l1/interleave.h)"""
    _fields_ = [("N", C.c_int), ("K", C.c_int), ("n", C.c_int), ("bits_cpp", C.c_void_p)]


class _InterleaverHandle(_Handle):
    """gmr1_interleaver_init(&self.il, N, K) now, gmr1_interleaver_fini(&self.il) at close"""

    def __init__(self, N=3, K=648):
        self.il = Interleaver()
        _call("gmr1_interleaver_init", C.byref(self.il), N, K)

    def _destroy(self):
        if self.il.bits_cpp:
            _fn("gmr1_interleaver_fini")(C.byref(self.il))
            self.il.bits_cpp = None


class Tch9Channel(_InterleaverHandle):
    """One TCH9 channel decoded burst by burst with the reference's own stateful calls:
    gmr1_interleaver_init(&il, 3, 648) once, then gmr1_tch9_decode(...) per burst (gmr1_rx.c:273, :333)."""

    def __init__(self, mode: int, N: int = 3, K: int = 648):
        self.mode = mode
        super().__init__(N, K)

    def decode(self, ebits, ciph=None):
        """-> (l2, sacch (10,), status (4,), conv)"""
        eb = _arr(ebits, np.int8)
        if eb.size != 662:
            raise ValueError("tch9: a burst has 662 soft bits")
        ciph = _arr(ciph, np.uint8)
        l2 = np.zeros((18, 30, 60)[self.mode], np.uint8)
        sa = np.zeros(10, np.int8)
        stt = np.zeros(4, np.int8)
        conv = C.c_int(0)
        _fn("gmr1_tch9_decode")(_p(l2), _p(sa), _p(stt), _p(eb), self.mode, _p(ciph), C.byref(self.il), C.byref(conv))
        return l2, sa, stt, conv.value


def xch_dc12_decode_batch(ebits):
    """(n, 432) soft bits of DC12 bursts -> (l2 (n, 24), crc (n,), conv (n,))"""
    eb = _arr(ebits, np.int8)
    n = eb.shape[0]
    if eb.ndim != 2 or eb.shape[1] != 432:
        raise ValueError("xch_dc12: ebits must be (n, 432)")
    l2 = np.zeros((n, 24), np.uint8)
    crc = np.zeros(n, np.int32)
    conv = np.zeros(n, np.int32)
    _call("gmr1_hip_xch_dc12_decode_batch", n, _p(eb), _p(l2), _p(crc), _p(conv))
    return l2, crc, conv


def xch_dc12_decode(ebits):
    """gmr1_xch_dc12_decode, the reference's own call -> (l2, crc, conv)"""
    eb = _arr(ebits, np.int8)
    l2 = np.zeros(24, np.uint8)
    conv = C.c_int(0)
    crc = _fn("gmr1_xch_dc12_decode")(_p(l2), _p(eb), C.byref(conv))
    if crc < 0:
        _check(crc, "gmr1_xch_dc12_decode")
    return l2, crc, conv.value


def rach_decode_batch(ebits, sb_mask):
    """(n, 494) soft bits of RACH bursts, sb_mask scalar or (n,) -> (rach (n, 18), rv (n,), conv (n,), crc (n, 2))"""
    eb = _arr(ebits, np.int8)
    n = eb.shape[0]
    if eb.ndim != 2 or eb.shape[1] != 494:
        raise ValueError("rach: ebits must be (n, 494)")
    m = _arr(np.broadcast_to(np.asarray(sb_mask, np.uint8), (n,)), np.uint8)
    rach = np.zeros((n, 18), np.uint8)
    rv = np.zeros(n, np.int32)
    conv = np.zeros(n, np.int32)
    crc = np.zeros((n, 2), np.int32)
    _call("gmr1_hip_rach_decode_batch", n, _p(eb), _p(m), _p(rach), _p(rv), _p(conv), _p(crc))
    return rach, rv, conv, crc


def rach_decode(ebits, sb_mask):
    """gmr1_rach_decode, the reference's own call -> (rach, rv, conv, (crc8, crc12))"""
    eb = _arr(ebits, np.int8)
    rach = np.zeros(18, np.uint8)
    conv = C.c_int(0)
    crc = (C.c_int * 2)()
    rv = _fn("gmr1_rach_decode")(_p(rach), _p(eb), int(sb_mask), C.byref(conv), crc)
    if rv < 0:
        _check(rv, "gmr1_rach_decode")
    return rach, rv, conv.value, (crc[0], crc[1])


def tch9_decode_batch(ebits, mode, seq_len, ciph=None):
    """(n_chan * seq_len, 662) soft bits, channel after channel -> (l2 (n, bytes), sacch, status, conv)"""
    eb = _arr(ebits, np.int8)
    n = eb.shape[0]
    assert n % seq_len == 0
    ciph = _arr(ciph, np.uint8)
    l2 = np.zeros((n, TCH9_BYTES[mode]), np.uint8)
    sa = np.zeros((n, 10), np.int8)
    stt = np.zeros((n, 4), np.int8)
    conv = np.zeros(n, np.int32)
    _call("gmr1_hip_tch9_decode_batch", n // seq_len, seq_len, mode, _p(eb), _p(ciph), _p(l2), _p(sa), _p(stt), _p(conv))
    return l2, sa, stt, conv


RX_BIG_RECORD = np.dtype([("arfcn", "<u2"), ("chain", "u1"), ("type", "u1"), ("fn", "<u4"),
                          ("tn", "u1"), ("crc", "u1"), ("len", "u1"), ("pad", "u1"),
                          ("conv", "<i4"), ("l2", "u1", (64,))])
assert RX_BIG_RECORD.itemsize == 80


# What RxStream needs to know of a kind of handle, once: its create and push entries, the carriers a push brings, and --
# for a kind whose push returns a second array -- that array's dtype, the entry that bounds it and the push_dev keyword
# that takes a caller's own.  (It stands here, below the class, because the dtypes do.)
_RxStreamKind = collections.namedtuple("_RxStreamKind", ["create", "push", "push_dev", "planes", "extra", "max_extra", "extra_arg"],
                                       defaults=[None, None, None])      # (no second array)
_RX_STREAM_KINDS = {
    "plain": _RxStreamKind("gmr1_hip_rx_stream_create", "gmr1_hip_rx_stream_push", "gmr1_hip_rx_stream_push_dev", 1),
    "tch": _RxStreamKind("gmr1_hip_rx_stream_create_tch", "gmr1_hip_rx_stream_push_tch", "gmr1_hip_rx_stream_push_tch_dev", 2),
    "full": _RxStreamKind("gmr1_hip_rx_stream_create_full", "gmr1_hip_rx_stream_push_full", "gmr1_hip_rx_stream_push_full_dev", 3,
                          RX_BIG_RECORD, "gmr1_hip_rx_stream_max_big", "big"),
    "voice": _RxStreamKind("gmr1_hip_rx_stream_create_voice", "gmr1_hip_rx_stream_push_voice", "gmr1_hip_rx_stream_push_voice_dev", 2,
                           RX_AUDIO, "gmr1_hip_rx_stream_max_audio", "audio"),
}


def rx_run_full(iq, tch, csd, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16, max_big=1 << 14):
    """gmr1_hip_rx_run_full: rx_run_tch plus the CSD carriers -> (records, big records, status, n_chains)"""
    iq = _arr(iq, np.complex64, -1)
    tch, csd = _same_size(tch, iq), _same_size(csd, iq)
    out, cap = _records(None, max_records)
    big, cap_big = _records(None, max_big, RX_BIG_RECORD)
    n_big = C.c_int(0)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_full", (len(offset), sps, _p(iq), _p(tch), _p(csd), iq.size),
                                          offset, length, arfcn, _p(out), cap, kc=kc,
                                          big=(_p(big), cap_big, C.addressof(n_big)))
    _check(run(), "gmr1_hip_rx_run_full")
    return out[:min(n_rec.value, cap)].copy(), big[:min(n_big.value, cap_big)].copy(), status, chains


def rx_run_full_dev(stream, iq_ptr, tch_ptr, csd_ptr, offset, length, sps=4, arfcn=None, kc=None, max_records=1 << 16,
                    max_big=1 << 14):
    """gmr1_hip_rx_run_full_dev: rx_run_full with the three captures already in HBM (device addresses, same layout)."""
    out, cap = _records(None, max_records)
    big, cap_big = _records(None, max_big, RX_BIG_RECORD)
    n_big = C.c_int(0)
    run, n_rec, status, chains = _rx_loop("gmr1_hip_rx_run_full_dev", (stream, len(offset), sps, iq_ptr, tch_ptr, csd_ptr), offset,
                                          length, arfcn, _p(out), cap, kc=kc, big=(_p(big), cap_big, C.addressof(n_big)))
    _check(run(), "gmr1_hip_rx_run_full_dev")
    return out[:min(n_rec.value, cap)].copy(), big[:min(n_big.value, cap_big)].copy(), status, chains


def tch9_frames_to_records_dev(stream, n_calls, first, n_frames, frames, label, out, max_out, n_out):
    """gmr1_hip_tch9_frames_to_records_dev: device pointers throughout; enqueues on `stream` and returns."""
    _call("gmr1_hip_tch9_frames_to_records_dev", stream, n_calls, first, n_frames, frames, label, out, max_out, n_out)


def gsmtap_pack_big(record, with_arfcn=False) -> bytes:
    """gmr1_hip_gsmtap_pack_big: the GSMTAP packet of one RX_BIG_RECORD (FACCH9 / TCH9 payloads)."""
    return _gsmtap("gmr1_hip_gsmtap_pack_big", record, RX_BIG_RECORD, with_arfcn, 96)


# ---- transmit direction: channel encoders and modulator (csrc/capi_encode.cpp, capi_mod.cpp, capi_tx_ref.cpp, tx_kernels.hip) ----------------
ENC_CHAINS = ("bcch", "ccch", "facch3", "tch3_m0", "tch3_m1", "facch9", "tch9_2k4", "tch9_4k8", "tch9_9k6", "rach",
              "xch_dc12")


def encoder_plan(chain):
    """The position map of one encoder chain (struct EncPlan of csrc/enc_plan.h) as a dict of numpy arrays.
    Host-only: works without a GPU."""
    cid = ENC_CHAINS.index(chain) if isinstance(chain, str) else int(chain)
    f = _fn("gmr1_hip_encoder_plan")
    size = f(cid, None, 0)
    if size < 0:
        _check(size, "gmr1_hip_encoder_plan")
    buf = np.zeros(size, np.uint8)
    rc = f(cid, _p(buf), size)
    if rc < 0:
        _check(rc, "gmr1_hip_encoder_plan")
    head = buf[:32].view(np.int32)
    o = 32
    poly = buf[o:o + 32].view(np.uint32); o += 32
    n_tab = 64 * 8
    crc_tab = buf[o:o + 2 * n_tab].view(np.uint16); o += 2 * n_tab
    crc_tab2 = buf[o:o + 2 * n_tab].view(np.uint16); o += 2 * n_tab
    ext_src = buf[o:o + 2 * 512].view(np.uint16); o += 2 * 512
    out = buf[o:o + 4 * 672].view(np.uint32); o += 4 * 672
    assert o == size, (o, size)
    names = ("n_in0", "n_in1", "n_ext", "n_out", "n_aux0", "n_aux1", "n_ciph", "depth")
    d = {k: int(v) for k, v in zip(names, head)}
    d.update(poly=poly.copy(), crc_tab=crc_tab.copy(), crc_tab2=crc_tab2.copy(), ext_src=ext_src[:d["n_ext"]].copy(),
             out=out[:d["n_out"]].copy())
    return d


def _encode_batch(fname, n_out, n, head, arrays):
    """arrays: list of (array or None); -> (n, n_out) uint8"""
    arrays = [_arr(a, np.uint8) for a in arrays]
    e = np.zeros((n, n_out), np.uint8)
    _call(fname, *head, *map(_p, arrays), _p(e))
    return e


def bcch_encode_batch(l2):
    l2 = _arr(l2, np.uint8, (-1, 24))
    return _encode_batch("gmr1_hip_bcch_encode_batch", 424, l2.shape[0], [l2.shape[0]], [l2])


def ccch_encode_batch(l2):
    l2 = _arr(l2, np.uint8, (-1, 24))
    return _encode_batch("gmr1_hip_ccch_encode_batch", 432, l2.shape[0], [l2.shape[0]], [l2])


def xch_dc12_encode_batch(l2):
    l2 = _arr(l2, np.uint8, (-1, 24))
    return _encode_batch("gmr1_hip_xch_dc12_encode_batch", 432, l2.shape[0], [l2.shape[0]], [l2])


def facch3_encode_batch(l2, bits_s, ciph=None):
    """l2 (n, 10), bits_s (n, 32), ciph (n, 384) optional -> (n, 4, 104)"""
    l2 = _arr(l2, np.uint8, (-1, 10))
    n = l2.shape[0]
    return _encode_batch("gmr1_hip_facch3_encode_batch", 416, n, [n], [l2, bits_s, ciph]).reshape(n, 4, 104)


def tch3_encode_batch(frames, bits_s, m=0, ciph=None):
    """frames (n, 2, 10), bits_s (n, 4), ciph (n, 208) optional -> (n, 212)"""
    frames = _arr(frames, np.uint8, (-1, 20))
    n = frames.shape[0]
    return _encode_batch("gmr1_hip_tch3_encode_batch", 212, n, [n, m], [frames, bits_s, ciph])


def facch9_encode_batch(l2, sacch, status, ciph=None):
    l2 = _arr(l2, np.uint8, (-1, 38))
    n = l2.shape[0]
    return _encode_batch("gmr1_hip_facch9_encode_batch", 662, n, [n], [l2, sacch, status, ciph])


def tch9_encode_batch(l2, mode, seq_len, sacch, status, ciph=None):
    """l2 (n, 18 | 30 | 60): whole runs of seq_len consecutive bursts of one channel each -> (n, 662)"""
    l2 = _arr(l2, np.uint8)
    l2 = l2.reshape(-1, (18, 30, 60)[mode] if 0 <= mode < 3 else l2.shape[-1])
    n = l2.shape[0]
    return _encode_batch("gmr1_hip_tch9_encode_batch", 662, n, [mode, n, seq_len], [l2, sacch, status, ciph])


def rach_encode_batch(rach, sb_mask):
    rach = _arr(rach, np.uint8, (-1, 18))
    n = rach.shape[0]
    return _encode_batch("gmr1_hip_rach_encode_batch", 494, n, [n], [rach, np.asarray(sb_mask, np.uint8).reshape(n)])


def mod_batch(burst, ebits, sync_id=0):
    """ebits (n, burst.ebits) ubits -> (n, burst.len) complex64 symbols at one sample per symbol"""
    bid = _burst_id(burst)
    b = burst_info(bid)
    eb = _arr(ebits, np.uint8, (-1, b.ebits))
    out = np.zeros((eb.shape[0], b.len), np.complex64)
    _call("gmr1_hip_mod_batch", bid, sync_id, eb.shape[0], _p(eb), _p(out))
    return out


PULSE_RC, PULSE_RRC = 0, 1
PULSES = {"rc": PULSE_RC, "rrc": PULSE_RRC}


def _shape_windows(n, in_len, offset, out, impair):
    """The shaping calls' window arguments -> (uint64 offset, complex64 out, what to return, the five per-burst arrays):
    offset None = windows back to back; out None = a fresh array that exactly holds them (returned as (n, in_len)), else
    the caller's flat complex64 array, written in place (what lies between the windows stays) and returned as it is."""
    offset = np.arange(n, dtype=np.uint64) * np.uint64(max(in_len, 0)) if offset is None else _arr(offset, np.uint64)
    if out is None:
        out = np.zeros(int(offset.max()) + in_len if n else 0, np.complex64)
        ret = out.reshape(n, in_len) if out.size == n * in_len else out
    else:
        if not (isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.flags.c_contiguous):
            raise TypeError("out: a contiguous complex64 array, written in place")
        ret = out
    types = (np.int32, np.float32, np.float32, np.float32, np.float32)
    per = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, t), (n,))) for a, t in zip(impair, types)]
    return offset, out, ret, per


def shape_batch(symbols, sps, in_len, *, pulse="rc", span=5, offset=None, start=None, frac=None, cfo=None, phase0=None,
                gain=None, out=None):
    """gmr1_hip_shape_batch: symbols (n, len) complex64 at one sample per symbol -> (n, in_len) complex64 windows at sps
    samples per symbol (offset = arange(n) * in_len unless given: then the flat buffer the windows lie in).  Per burst, a
    scalar or (n,), None = 0 / 0 / 0 / 0 / 1: start (window sample of symbol 0), frac (samples), cfo (rad / sample), phase0
    (rad), gain.  pulse: "rc" | "rrc" (roll-off 0.35), cut at +-span symbols."""
    sym = _arr(symbols, np.complex64)
    sym = sym.reshape(-1, sym.shape[-1] if sym.ndim else 1)
    n, length = sym.shape
    offset, out, ret, per = _shape_windows(n, in_len, offset, out, (start, frac, cfo, phase0, gain))
    _call("gmr1_hip_shape_batch", n, length, sps, PULSES.get(pulse, pulse), span, in_len, _p(sym), _p(offset),
          *[_p(a) for a in per], _p(out), out.size)
    return ret


def mod_shaped_batch(burst, ebits, sps, in_len, *, sync_id=None, pulse="rc", span=5, offset=None, start=None, frac=None,
                     cfo=None, phase0=None, gain=None, out=None):
    """gmr1_hip_mod_shaped_batch: ebits (n, burst.ebits) ubits -> windows as shape_batch(mod_batch(burst, ebits), ...) gives
    them, float for float, in one launch; sync_id: a scalar or (n,), the training sequence of each burst (None: 0)."""
    bid = _burst_id(burst)
    b = burst_info(bid)
    eb = _arr(ebits, np.uint8, (-1, b.ebits))
    n = eb.shape[0]
    sid = None if sync_id is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sync_id, np.int32), (n,)))
    offset, out, ret, per = _shape_windows(n, in_len, offset, out, (start, frac, cfo, phase0, gain))
    _call("gmr1_hip_mod_shaped_batch", bid, n, sps, PULSES.get(pulse, pulse), span, in_len, _p(eb), _p(sid), _p(offset),
          *[_p(a) for a in per], _p(out), out.size)
    return ret


def shape_batch_dev(stream, n, length, sps, pulse, span, in_len, symbols, offset, start, frac, cfo, phase0, gain, out, out_len):
    """gmr1_hip_shape_batch_dev on device memory (addresses, None for an array left out): enqueues on `stream` and returns"""
    _call("gmr1_hip_shape_batch_dev", stream, n, length, sps, pulse, span, in_len, symbols, offset, start, frac, cfo, phase0,
          gain, out, out_len)


def mod_shaped_batch_dev(stream, burst, n, sps, pulse, span, in_len, ebits, sync_id, offset, start, frac, cfo, phase0, gain,
                         out, out_len):
    """gmr1_hip_mod_shaped_batch_dev on device memory (addresses, None for an array left out): enqueues and returns"""
    _call("gmr1_hip_mod_shaped_batch_dev", stream, _burst_id(burst), n, sps, pulse, span, in_len, ebits, sync_id, offset, start,
          frac, cfo, phase0, gain, out, out_len)


def fcch_chirp_batch(n, sps, in_len, *, fcch_type="fcch", offset=None, start=None, frac=None, cfo=None, phase0=None, gain=None,
                     out=None):
    """gmr1_hip_fcch_chirp_batch: n windows of in_len complex64 samples, each holding one FCCH dual chirp at sps samples per
    symbol, under shape_batch's window arguments (offset, out, and per window start / frac / cfo / phase0 / gain)."""
    offset, out, ret, per = _shape_windows(n, in_len, offset, out, (start, frac, cfo, phase0, gain))
    _call("gmr1_hip_fcch_chirp_batch", _fcch_id(fcch_type), n, sps, in_len, _p(offset), *[_p(a) for a in per], _p(out), out.size)
    return ret


def fcch_chirp_batch_dev(stream, fcch_type, n, sps, in_len, offset, start, frac, cfo, phase0, gain, out, out_len):
    """gmr1_hip_fcch_chirp_batch_dev on device memory (addresses, None for an array left out): enqueues and returns"""
    _call("gmr1_hip_fcch_chirp_batch_dev", stream, _fcch_id(fcch_type), n, sps, in_len, offset, start, frac, cfo, phase0, gain,
          out, out_len)


CARRIER_MIX_TILE = 1024       # GMR1_HIP_CARRIER_MIX_TILE


def carrier_mix(seg_iq, seg_first, seg_src, seg_pos, seg_len, length, *, out_offset=None, first=None, sigma=None, cfo=None,
                noise_id=None, seed=0, max_seg_len=None, max_length=None, out=None):
    """gmr1_hip_carrier_mix: the windows in seg_iq (flat complex64: what shape_batch / mod_shaped_batch / fcch_chirp_batch
    wrote) to carriers.  Carrier c owns segments seg_first[c] .. seg_first[c + 1] (seg_first None: no segments), segment s is
    seg_iq[seg_src[s] : seg_src[s] + seg_len[s]] landing on absolute sample seg_pos[s] (sorted per carrier); carrier c has
    length[c] samples from absolute sample first[c] (None: 0) and gets the noise sigma[c] (None: 0) of stream noise_id[c]
    (None: c) under `seed`, and the carrier offset cfo[c] in radians per sample (None: 0).  out_offset None: carriers back to
    back; out None: a fresh array that exactly holds them, else the caller's flat complex64 array, written in place.
    Returns the array; with out None and one carrier or equal lengths, shaped (n_carriers, length)."""
    length = _arr(length, np.uint64, -1)
    n = length.size
    seg_iq = _arr(seg_iq, np.complex64, -1)
    seg_first, seg_src = _arr(seg_first, np.int32), _arr(seg_src, np.uint64)
    seg_pos, seg_len = _arr(seg_pos, np.int64), _arr(seg_len, np.uint32)
    n_seg = 0 if seg_first is None or seg_src is None else seg_src.size
    if max_seg_len is None:
        max_seg_len = int(seg_len.max()) if n_seg else 0
    if max_length is None:
        max_length = int(length.max()) if n else 0
    if out_offset is None:
        out_offset = (np.cumsum(length) - length).astype(np.uint64)
    out_offset = _arr(out_offset, np.uint64, -1)
    if out is None:
        out = np.zeros(int((out_offset + length).max()) if n else 0, np.complex64)
        ret = out.reshape(n, -1) if n and out.size == n * int(length[0]) and (length == length[0]).all() else out
    else:
        if not (isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.flags.c_contiguous):
            raise TypeError("out: a contiguous complex64 array, written in place")
        ret = out
    per = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, t), (n,)))
           for a, t in ((first, np.int64), (sigma, np.float32), (cfo, np.float64), (noise_id, np.uint32))]
    _call("gmr1_hip_carrier_mix", n, _p(seg_iq), 0 if seg_iq is None else seg_iq.size, n_seg, _p(seg_first), _p(seg_src),
          _p(seg_pos), _p(seg_len), max_seg_len, _p(out_offset), _p(length), max_length, *[_p(a) for a in per], seed, _p(out),
          out.size)
    return ret


def carrier_mix_dev(stream, n_carriers, seg_iq, seg_first, seg_src, seg_pos, seg_len, max_seg_len, out_offset, length, max_length,
                    first, sigma, cfo, noise_id, seed, out):
    """gmr1_hip_carrier_mix_dev on device memory (addresses, None for an array left out): enqueues on `stream` and returns"""
    _call("gmr1_hip_carrier_mix_dev", stream, n_carriers, seg_iq, seg_first, seg_src, seg_pos, seg_len, max_seg_len, out_offset,
          length, max_length, first, sigma, cfo, noise_id, seed, out)


def encode_single(chain, *args):
    """The reference's own single calls gmr1_<chain>_encode (void unless xch_dc12): returns the burst bits.
    bcch / ccch / xch_dc12: (l2); facch3: (l2, bits_s, ciph | None); tch3: (frame0, frame1, bits_s, ciph | None, m);
    facch9: (l2, sacch, status, ciph | None); rach: (rach, sb_mask)."""
    n_out = {"bcch": 424, "ccch": 432, "xch_dc12": 432, "facch3": 416, "tch3": 212, "facch9": 662, "rach": 494}[chain]
    e = np.full(n_out, 255, np.uint8)
    # a scalar goes as it is (the prototype knows its type), anything else as a uint8 array
    args = [int(a) if isinstance(a, (int, np.integer)) else _arr(a, np.uint8) for a in args]
    rc = _fn("gmr1_%s_encode" % chain)(_p(e), *[a if isinstance(a, int) else _p(a) for a in args])
    if chain == "xch_dc12":
        _check(rc, "gmr1_xch_dc12_encode")
    if (e == 255).any():
        raise Gmr1HipError("gmr1_%s_encode: %s" % (chain, _last_error()))
    return e


class Tch9Encoder(_InterleaverHandle):
    """One TCH9 channel encoded burst by burst with the reference's stateful calls (tch9.h:47-49)."""

    def __init__(self, mode: int):
        self.mode = mode
        super().__init__()

    def encode(self, l2, sacch, status, ciph=None):
        l2, sa, stt, ciph = (_arr(a, np.uint8) for a in (l2, sacch, status, ciph))
        e = np.full(662, 255, np.uint8)
        _fn("gmr1_tch9_encode")(_p(e), _p(l2), self.mode, _p(sa), _p(stt), _p(ciph), C.byref(self.il))
        if (e == 255).any():
            raise Gmr1HipError("gmr1_tch9_encode: %s" % _last_error())
        return e


def pi4cxpsk_mod(burst_name: str, ebits, sync_id=0, max_len=None):
    """The reference's gmr1_pi4cxpsk_mod on one of the exported burst objects -> (rc, symbols)"""
    n = burst_info(burst_name).len if max_len is None else max_len
    data = np.zeros(max(n, 1), np.complex64)
    v = CxVec(0, n, 0, data.ctypes.data)
    eb = _arr(ebits, np.uint8)
    rc = _fn("gmr1_pi4cxpsk_mod")(_burst_addr(burst_name), _p(eb), sync_id, C.byref(v))
    return rc, data[:v.len].copy()


# ---- stand-alone layer-1 primitives (reference scramb.h / interleave.h), each one blocking GPU call ----------
def _prim(fname, x, dtype, *size):
    x = _arr(x, dtype)
    out = np.full(x.shape, 77, dtype)
    _fn(fname)(_p(out), _p(x), *size)
    return out


def scramble_sbit(x):
    return _prim("gmr1_scramble_sbit", x, np.int8, np.size(x))


def scramble_ubit(x):
    return _prim("gmr1_scramble_ubit", x, np.uint8, np.size(x))


def interleave_intra(x, N, inverse=False):
    x = _arr(x, np.uint8, -1)
    assert x.size == 8 * N
    return _prim("gmr1_deinterleave_intra" if inverse else "gmr1_interleave_intra", x, np.uint8, N)


class InterBurstInterleaver(_InterleaverHandle):
    """gmr1_interleaver_init(il, 3, 648) + gmr1_interleave_inter / gmr1_deinterleave_inter on that object."""

    def _call(self, fname, x):
        x = _arr(x, np.uint8)
        assert x.size == 648
        out = np.full(648, 77, np.uint8)
        _fn(fname)(C.byref(self.il), _p(out), _p(x))
        return out

    def interleave(self, bits_ep):
        return self._call("gmr1_interleave_inter", bits_ep)

    def deinterleave(self, bits_epp):
        return self._call("gmr1_deinterleave_inter", bits_epp)


# ---- gmr1_hip_shard.h: the receive loop over the ranks of a node, RCCL exchanges inside the library ------------------
class Shard(_Handle):
    """One rank's end of the node-wide communicator (gmr1_hip_shard_create).  `id_bytes`: the 128-byte id made by
    Shard.unique_id() on one rank and handed to the others by the host program (here: torch.distributed)."""

    def __init__(self, id_bytes: bytes, rank: int, world: int):
        self._h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(id_bytes)
        _call("gmr1_hip_shard_create", C.byref(self._h), buf, rank, world)
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _call("gmr1_hip_shard_unique_id", buf)
        return bytes(buf)

    def rx_run(self, stream, iq_ptr, offset, length, sps=4, arfcn=None, root=0, max_records=1 << 17, resident=False):
        """gmr1_hip_rx_run_sharded (resident: gmr1_hip_rx_run_sharded_resident -- iq_ptr is this rank's own memory holding
        the carriers it owns, nothing is scattered).  Returns (records, status, n_chains, timing_ms) on root,
        (None, None, None, timing_ms) elsewhere."""
        is_root = self.rank == root
        out = _records(None, max_records)[0] if is_root else None
        timing = np.zeros(3, np.float32)
        fname = "gmr1_hip_rx_run_sharded_resident" if resident else "gmr1_hip_rx_run_sharded"
        run, n_rec, status, chains = _rx_loop(fname, (self._h.value, stream, root, len(offset), sps, iq_ptr), offset,
                                              length, arfcn, _p(out), max_records, tail=(_p(timing),))
        _check(run(), fname)
        if not is_root:
            return None, None, None, timing
        return out[:min(n_rec.value, max_records)].copy(), status, chains, timing

    def _destroy(self):
        if self._h:
            _fn("gmr1_hip_shard_destroy")(self._h)
            self._h = C.c_void_p()


# ---------------------------------------------------------------------------
# AMBE speech decoder (include/osmocom/gmr1/codec/codec.h, gmr1_hip_codec_*)
# ---------------------------------------------------------------------------
CODEC_CLEARED, CODEC_FRESH = 1, 2


def codec_state_bytes() -> int:
    return _fn("gmr1_hip_codec_state_bytes")()


def codec_decode_batch(frames, state=None, flags=0):
    """frames (n_ch, n_frames, 10) uint8 -> (pcm (n_ch, n_frames, 160) int16, rv (n_ch, n_frames) int32, state).
    state: None = fresh decoders, or the uint8 array a previous call returned (continues those channels)."""
    frames = _arr(frames, np.uint8)
    assert frames.ndim == 3 and frames.shape[2] == 10
    n_ch, n_fr = frames.shape[:2]
    pcm = np.zeros((n_ch, n_fr, 160), np.int16)
    rv = np.zeros((n_ch, n_fr), np.int32)
    if state is None:
        state = np.zeros((n_ch, codec_state_bytes()), np.uint8)
        flags |= CODEC_FRESH
    else:
        state = _arr(state, np.uint8).copy()
        assert state.shape == (n_ch, codec_state_bytes())
    _call("gmr1_hip_codec_decode_batch", n_ch, n_fr, _p(frames), _p(pcm), _p(rv), _p(state), flags)
    return pcm, rv, state


def codec_init_dev(stream, n_ch, state_ptr, flags=0):
    _call("gmr1_hip_codec_init_dev", stream, n_ch, state_ptr, flags)


def codec_init_list_dev(stream, n, call_ptr, state_ptr, flags=0):
    """gmr1_hip_codec_init_list_dev: fresh decoders for state[call[j]], j < n (device pointers; call[j] < 0 is skipped)."""
    _call("gmr1_hip_codec_init_list_dev", stream, n, call_ptr, state_ptr, flags)


def codec_decode_batch_dev(stream, n_ch, n_frames, frames_ptr, pcm_ptr, rv_ptr, state_ptr):
    _call("gmr1_hip_codec_decode_batch_dev", stream, n_ch, n_frames, frames_ptr, pcm_ptr, rv_ptr, state_ptr)


# ---------------------------------------------------------------------------
# a followed voice call to audio (gmr1_hip_tch3_frames_to_pcm*, gmr1_hip_tch3_voice_batch*)
# ---------------------------------------------------------------------------
def _codec_state(state, n_calls, flags):
    """-> (a 16-byte aligned (n_calls, codec_state_bytes()) uint8 array: a copy of `state`, or zeros for fresh decoders;
    flags with CODEC_FRESH set in the latter case)"""
    nb = codec_state_bytes()
    raw = np.zeros(n_calls * nb + 16, np.uint8)
    at = -raw.ctypes.data % 16
    own = raw[at:at + n_calls * nb].reshape(n_calls, nb)
    if state is None:
        return own, flags | CODEC_FRESH
    state = _arr(state, np.uint8)
    assert state.shape == (n_calls, nb)
    own[:] = state
    return own, flags


def tch3_frames_to_pcm(frames, first, state=None, flags=0):
    """The TCH3 follower's records (TCH3_FRAME array) of len(first) - 1 calls, call c owning records first[c] .. first[c+1]
    -> (pcm (n_frames, 320) int16, rv (n_frames, 2) int32, state): a speech record (type 0x10) is its two frames decoded, any
    other record 320 zeros that leave the decoder alone.  state: None = fresh decoders, or the uint8 array a previous call
    (or codec_decode_batch) returned: continues those calls."""
    frames = np.ascontiguousarray(frames, TCH3_FRAME).reshape(-1)
    first = _arr(first, np.int32)
    n_calls, n_fr = first.size - 1, frames.size
    pcm = np.zeros((n_fr, 320), np.int16)
    rv = np.zeros((n_fr, 2), np.int32)
    state, flags = _codec_state(state, n_calls, flags)
    _call("gmr1_hip_tch3_frames_to_pcm", n_calls, _p(first), n_fr, _p(frames), _p(state), flags, _p(pcm), _p(rv))
    return pcm, rv, state


def tch3_frames_to_pcm_dev(stream, n_calls, n_frames, first, frames, state, pcm, rv=None):
    """The same on device memory (addresses): enqueues on `stream` and returns; state: n_calls x codec_state_bytes() bytes
    (codec_init_dev makes fresh ones), updated in place; pcm: n_frames x 320 int16; rv: n_frames x 2 int32 or None."""
    _call("gmr1_hip_tch3_frames_to_pcm_dev", stream, n_calls, first, n_frames, frames, state, pcm, rv)


def tch3_frames_to_audio_dev(stream, n_calls, n_frames, first, frames, fn, label, state, out, max_out, n_out):
    """gmr1_hip_tch3_frames_to_audio_dev: device pointers throughout; enqueues on `stream` and returns.  fn: n_frames uint32;
    label: n_calls uint64 (tch3_audio_label); out: max_out RX_AUDIO blocks on a 16-byte boundary; n_out: one int32."""
    _call("gmr1_hip_tch3_frames_to_audio_dev", stream, n_calls, first, n_frames, frames, fn, label, state, out, max_out, n_out)


def tch3_audio_label(arfcn, chain, tn, call):
    """a call's label for tch3_frames_to_audio_dev: arfcn | chain << 16 | tn << 24 | call << 32"""
    return (int(arfcn) & 0xffff) | (int(chain) & 0xff) << 16 | (int(tn) & 0xff) << 24 | (int(call) & 0xff) << 32


def tch3_voice(iq, first, offset, freq_shift, fn, state, codec_state=None, flags=0, sps=4, in_len=None):
    """tch3_follow and tch3_frames_to_pcm in one call, the records staying on the device in between
    -> (TCH3_FRAME record per frame, the calls' TCH3_STATE, pcm (n_frames, 320), rv (n_frames, 2), the calls' decoder state)."""
    iq = _arr(iq, np.complex64, -1)
    first, offset = _arr(first, np.int32), _arr(offset, np.uint64)
    freq_shift, fn = _arr(freq_shift, np.float32), _arr(fn, np.uint32)
    state = np.array(state, TCH3_STATE, ndmin=1)
    n_calls, n_fr = first.size - 1, offset.size
    out = np.zeros(n_fr, TCH3_FRAME)
    pcm = np.zeros((n_fr, 320), np.int16)
    rv = np.zeros((n_fr, 2), np.int32)
    codec_state, flags = _codec_state(codec_state, n_calls, flags)
    _call("gmr1_hip_tch3_voice_batch", n_calls, sps, tch3_in_len(sps) if in_len is None else in_len, _p(iq), iq.size,
          _p(first), n_fr, _p(offset), _p(freq_shift), _p(fn), _p(state), _p(out), _p(codec_state), flags, _p(pcm), _p(rv))
    return out, state, pcm, rv, codec_state


def tch3_voice_dev(stream, n_calls, n_frames, iq, first, offset, freq_shift, fn, state, out, codec_state, pcm, rv=None, sps=4,
                   in_len=None):
    """The same on device memory (addresses): enqueues on `stream` and returns; state, out as for tch3_follow_dev, codec_state,
    pcm, rv as for tch3_frames_to_pcm_dev."""
    _call("gmr1_hip_tch3_voice_batch_dev", stream, n_calls, sps, tch3_in_len(sps) if in_len is None else in_len, iq, first,
          n_frames, offset, freq_shift, fn, state, out, codec_state, pcm, rv)


class Codec(_Handle):
    """The reference's one-channel object: gmr1_codec_alloc / decode_frame / decode_dtx / release."""

    def __init__(self):
        self.h = _fn("gmr1_codec_alloc")()
        if not self.h:
            raise Gmr1HipError("gmr1_codec_alloc returned NULL: " + _last_error())

    def decode_frame(self, frame, N=160, bad=0):
        frame = _arr(frame, np.uint8)
        audio = np.zeros(max(N, 160), np.int16)
        rc = _fn("gmr1_codec_decode_frame")(self.h, _p(audio), N, _p(frame), bad)
        return audio, rc

    def decode_dtx(self, N=160):
        audio = np.ones(N, np.int16)
        rc = _fn("gmr1_codec_decode_dtx")(self.h, _p(audio), N)
        return audio, rc

    def _destroy(self):
        if self.h:
            _fn("gmr1_codec_release")(self.h)
            self.h = None

    release = _Handle.close


# layout of the host table image (csrc/ambe_dev.h: struct AmbeTab), for the tests that check it without a GPU
CODEC_TAB_DTYPE = np.dtype([
    ("cosv", "<f4", 1024), ("win", "<f4", 128), ("f0_sf1", "<f4", 128), ("log2_L", "<f4", 64), ("tone_ampl", "<i4", 256),
    ("lcg_mul", "<u4", 128), ("lcg_add", "<u4", 128), ("gain", "<f4", 512), ("prba12", "<f4", 256), ("prba34", "<f4", 128),
    ("prba57", "<f4", 384), ("hoc", "<f4", (4, 512)), ("interp", "<f4", 4), ("perr14", "<f4", 256), ("perr58", "<f4", 128),
    ("rho", "<f4", 56), ("vuv", "<u2", 64), ("hpg", "u1", 192), ("f0_sf0", "<f4", (129, 128, 4)),
])


def codec_host_tables():
    img, n = C.c_void_p(), C.c_size_t()
    _call("gmr1_hip_codec_host_tables", C.byref(img), C.byref(n))
    assert n.value == CODEC_TAB_DTYPE.itemsize, (n.value, CODEC_TAB_DTYPE.itemsize)
    raw = C.string_at(img.value, n.value)
    return np.frombuffer(raw, CODEC_TAB_DTYPE)[0]


def codec_libm_check(which, x):
    x = _arr(x, np.float32)
    out = np.zeros(x.size, np.float32)
    _call("gmr1_hip_codec_libm_check", which, x.size, _p(x), _p(out))
    return out
