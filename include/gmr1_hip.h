/*
 * gmr1_hip.h -- C ABI of the MI355X-native GMR-1 receive hot path.
 *
 * Two families of entry points live in libgmr1_hip.so:
 *
 *  1. The reference's own per-burst C API (declared in include/osmocom/gmr1/
 *     {sdr,l1}/.h of this repo, same names / argument meaning / return values
 *     as osmocom/osmo-gmr) -- each call is blocking: H2D, one kernel, D2H.  (The BCCH / DC6 demodulation call at
 *     4 samples per symbol is answered by a resident one-wave kernel fed from a mailbox in pinned memory instead of
 *     a launch per call; it ends by itself 200 us after the last call.  GMR1_HIP_ONE_BURST_SERVER=0 in the
 *     environment keeps the launch per call.  INTEGRATION.md, "What the unchanged application costs".)
 *
 *  2. The batched entry points below, which are what a high-rate caller binds.
 *     "_dev" variants take DEVICE pointers (inputs already resident in HBM) and
 *     a hipStream_t passed as void*; they only enqueue work.  The variants
 *     without "_dev" take HOST pointers and stage through HBM themselves.
 *
 * Every function returns 0 on success or a negative errno; the per-burst
 * status (the reference's own return value) is written to rv[].  There is NO
 * CPU fallback: without a usable HIP device every call fails with -ENODEV.
 *
 * Reference interfaces replaced (osmocom/osmo-gmr, paths relative to the
 * reference tree):
 *   gmr1_hip_demod_batch*        -> gmr1_pi4cxpsk_demod   include/osmocom/gmr1/sdr/pi4cxpsk.h:101-105
 *   gmr1_hip_detect_batch*       -> gmr1_pi4cxpsk_detect  include/osmocom/gmr1/sdr/pi4cxpsk.h:107-110
 *   gmr1_hip_mod_order_batch*    -> gmr1_pi4cxpsk_mod_order include/osmocom/gmr1/sdr/pi4cxpsk.h:112-113
 *   gmr1_hip_bcch_decode_batch*  -> gmr1_bcch_decode      include/osmocom/gmr1/l1/bcch.h:38
 *   gmr1_hip_ccch_decode_batch*  -> gmr1_ccch_decode      include/osmocom/gmr1/l1/ccch.h:38
 *   gmr1_hip_facch3_decode_batch*-> gmr1_facch3_decode    include/osmocom/gmr1/l1/facch3.h:39-40
 *   gmr1_hip_tch3_decode_batch*  -> gmr1_tch3_decode      include/osmocom/gmr1/l1/tch3.h:40-42
 *   gmr1_hip_rx_bcch_ccch_batch* -> rx_bcch / rx_ccch     src/gmr1_rx.c:746-850 (demod + decode of one burst)
 *   gmr1_hip_fcch_rough_batch*   -> gmr1_fcch_rough       include/osmocom/gmr1/sdr/fcch.h:47-49
 *   gmr1_hip_fcch_rough_multi_batch* -> gmr1_fcch_rough_multi include/osmocom/gmr1/sdr/fcch.h:51-53
 *   gmr1_hip_fcch_fine_batch*    -> gmr1_fcch_fine        include/osmocom/gmr1/sdr/fcch.h:55-57
 *   gmr1_hip_fcch_snr_batch*     -> gmr1_fcch_snr         include/osmocom/gmr1/sdr/fcch.h:59-61
 *   gmr1_hip_fcch_acquire_batch* -> fcch_single_init / fcch_multi_process  src/gmr1_rx.c:605-733 (up to the survivor list)
 *   gmr1_hip_tch3_follow_batch*  -> rx_tch3, src/gmr1_rx.c:355-600
 *   gmr1_hip_tch9_follow*_batch* -> rx_tch9, src/gmr1_rx.c:262-353
 *   gmr1_hip_tch3_frames_to_pcm* -> gmr1_codec_decode_frame / _decode_dtx over a call's bursts  include/osmocom/gmr1/codec/codec.h:41-45
 *   gmr1_hip_tch3_voice_batch*   -> rx_tch3 and the above: samples in, audio out (gmr1_rx and gmr1_ambe_decode in one call)
 *   gmr1_hip_rx_run_voice*, gmr1_hip_rx_stream_*voice* -> main() of src/gmr1_rx.c with the calls it follows decoded as
 *                                   gmr1_ambe_decode decodes them (src/gmr1_ambe_decode.c:122-150), one-shot and streaming
 */
#ifndef GMR1_HIP_H
#define GMR1_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMR1_HIP_MAX_SYNC       4
#define GMR1_HIP_MAX_CHUNKS     8
#define GMR1_HIP_MAX_SYNC_SYMS  32
#define GMR1_HIP_MAX_WINDOW     256   /* lags the demod kernels keep room for by default; wider search windows size their own */
#define GMR1_HIP_MAX_IN_LEN     4096  /* max samples per burst window (BCCH at 16 samples per symbol: 4 064) */

/* burst type ids (order of include/osmocom/gmr1/sdr/nb.h:37-46) */
enum gmr1_hip_burst_id {
	GMR1_HIP_BCCH = 0, GMR1_HIP_DC2, GMR1_HIP_DC6, GMR1_HIP_DC12,
	GMR1_HIP_NT3_SPEECH, GMR1_HIP_NT3_FACCH, GMR1_HIP_NT6, GMR1_HIP_NT9,
	GMR1_HIP_RACH, GMR1_HIP_SDCCH, GMR1_HIP_N_BURSTS
};

/* flat, pointer-free copy of a struct gmr1_pi4cxpsk_burst */
struct gmr1_hip_chunk {
	int32_t pos, len;
	uint8_t syms[GMR1_HIP_MAX_SYNC_SYMS];
};

struct gmr1_hip_burst_flat {
	char    name[16];
	float   rotation;
	int32_t nbits, guard_pre, guard_post, len, ebits;
	int32_t n_sync;
	int32_t n_sync_chunks[GMR1_HIP_MAX_SYNC];
	struct gmr1_hip_chunk sync[GMR1_HIP_MAX_SYNC][GMR1_HIP_MAX_CHUNKS];
	int32_t n_data;
	struct gmr1_hip_chunk data[GMR1_HIP_MAX_CHUNKS];
};

/* ---- library / device ----------------------------------------------------
 * Threads: gmr1_hip_last_error() is per thread; the burst-level _batch / _batch_dev calls keep no state
 * between calls and may run from several threads on different streams.  The calls that use the library's
 * grow-only per-device workspace -- gmr1_hip_fcch_rough*_batch*, gmr1_hip_fcch_acquire_batch*, gmr1_hip_channelize*, gmr1_hip_ddc*,
 * gmr1_hip_rx_run*, gmr1_hip_tch3_follow_batch*, gmr1_hip_tch3_voice_batch*, gmr1_hip_tch9_follow*_batch*, gmr1_hip_detect_batch* with more than four candidates, and gmr1_hip_tch3_rx_batch* where it
 * runs as two launches without a caller's soft-bit buffer -- may ALSO be called from several threads and streams:
 * they take turns.  The host part of such a call runs under a per-device lock (a second thread waits), and a call
 * on another stream first makes its stream wait, on the device, for the previous user's kernels; nothing is
 * refused and no result depends on the interleaving (tests/test_gpu_threads.py).  They do not run in PARALLEL
 * with each other on one device: one receiver per GPU, as in the reference (one process per capture).  The streaming
 * channelizer (gmr1_hip_chan_stream_*) does not use the workspace: its handles own their memory and run concurrently. */
int         gmr1_hip_init(int device);          /* optional; selects the HIP device     */
const char *gmr1_hip_last_error(void);
const char *gmr1_hip_version(void);
int         gmr1_hip_burst_info(int burst_id, struct gmr1_hip_burst_flat *out);
/* Measurement aid (no counterpart in the reference): the shader clock the device holds right now, in MHz -- one wave on
 * `stream` compares the shader-clock counter with the constant-rate wall counter over `micros` microseconds (blocking).
 * Launched behind a timed region it tells what clock that region ran at.  wall_mhz (optional): the wall counter's rate. */
int         gmr1_hip_clock_probe_dev(void *stream, int micros, double *core_mhz, double *wall_mhz);

/* ---- which Viterbi decoder of libosmocore the layer-1 chains reproduce ------
 * The reference hands every channel to osmo_conv_decode() (src/l1/bcch.c:94, ccch.c:98, facch3.c:160, tch3.c:174,
 * facch9.c:134, tch9.c:170, rach.c:167, xch_dc12.c:97).  Which arithmetic that is depends on the libosmocore the
 * integrator links: its generic decoder (every version; src/conv.c), or -- since 2017, for codes with K in {5, 7} and
 * N in {2, 3, 4}: every chain above except xCH (K = 9) and TCH9 2k4 (N = 5) -- osmo_conv_decode_acc (src/conv_acc.c).
 * The two differ in metric quantisation, start states, flush steps and the tail-biting end state, so near the decoding
 * threshold they return different frames, and the accelerated one returns 0 where the generic one returns the path
 * metric (`conv_rv`).  Pick the one the replaced build used.  Process-wide; takes effect with the next call.  The
 * DEFAULT is GMR1_HIP_CONV_ACC -- what a build against any libosmocore released since 2017 ran (configure.ac:23 only
 * asks for >= 0.4.1, but no distribution has shipped anything older than 1.x for years) -- unless the environment says
 * GMR1_HIP_CONV_DECODER=generic when the library is first used; gmr1_hip_version() names the decoder in force. */
enum gmr1_hip_conv_decoder {
	GMR1_HIP_CONV_GENERIC = 0,   /* osmo_conv_decode's generic path for every code */
	GMR1_HIP_CONV_ACC     = 1,   /* osmo_conv_decode_acc where libosmocore >= 0.10 dispatches to it, generic elsewhere */
};
int gmr1_hip_set_conv_decoder(int decoder);     /* 0, or -EINVAL */
int gmr1_hip_get_conv_decoder(void);

/* ---- normal-burst demodulation (any burst type, one type per call) ------- */
/* iq: interleaved float32 I/Q; burst i occupies iq[offset[i] .. offset[i]+in_len) (complex samples).
 * Optional outputs may be NULL.  ebits is n rows of bt.ebits int8, ebits_stride (>= bt.ebits) bytes apart: what lies
 * between two rows is left as it was.  ssyms is n x bt.len float. */
int gmr1_hip_demod_batch_dev(void *stream, int burst_id, int n, int sps, int in_len,
                             const float *iq, const uint64_t *offset, const float *freq_shift,
                             int8_t *ebits, int ebits_stride, int32_t *sync_id,
                             float *toa, float *freq_err, float *ssyms, int32_t *rv);
int gmr1_hip_demod_batch(int burst_id, int n, int sps, int in_len,
                         const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                         int8_t *ebits, int ebits_stride, int32_t *sync_id,
                         float *toa, float *freq_err, float *ssyms, int32_t *rv);
/* Debugging aid (the reference's ENABLE_DEBUG_SIGNAL dumps, include/osmocom/gmr1/sdr/defs.h:35-39): ONE burst,
 * demodulated as above (host pointers, blocking), plus the four intermediate vectors of gmr1_pi4cxpsk_demod --
 *   corr   [in_len - symbols*sps + 1] float    "pi4cxpsk_corr"  (pi4cxpsk.c:251)  sync correlation magnitude per lag
 *                                              (formats with several training sequences: summed over them)
 *   burst  [in_len]  complex                   "pi4cxpsk_burst" (pi4cxpsk.c:545)  normalised, de-rotated window
 *   align  [symbols] complex                   "pi4cxpsk_align" (pi4cxpsk.c:345)  one sample per symbol at the found timing
 *   final  [symbols] complex                   "pi4cxpsk_final" (pi4cxpsk.c:582)  after fine-frequency + carrier correction
 * Any output but rv may be NULL.  The production kernels work on phases and never form three of these; this entry
 * rebuilds them from the same demodulation (rx_debug_kernels.inc), so ssyms / ebits / toa here ARE the batch entry's. */
int gmr1_hip_demod_taps(int burst_id, int sps, int in_len, const float *iq, float freq_shift,
                        float *corr, float *burst, float *align, float *final_,
                        int8_t *ebits, int32_t *sync_id, float *toa, float *freq_err, float *ssyms, int32_t *rv);

/* ---- burst type detection / modulation order -------------------------------
 * burst_ids: any number of candidate types (same length / modulation family; more than four run as several launches
 * that hand the best so far on); e_toa optional. */
int gmr1_hip_detect_batch_dev(void *stream, int n_types, const int *burst_ids, int n, int sps, int in_len,
                              const float *iq, const uint64_t *offset, const float *freq_shift,
                              const float *e_toa, int32_t *bt_id, int32_t *sync_id, float *toa, int32_t *rv);
int gmr1_hip_detect_batch(int n_types, const int *burst_ids, int n, int sps, int in_len,
                          const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                          const float *e_toa, int32_t *bt_id, int32_t *sync_id, float *toa, int32_t *rv);
int gmr1_hip_mod_order_batch_dev(void *stream, int n, int sps, int in_len,
                                 const float *iq, const uint64_t *offset, const float *freq_shift, int32_t *order);
int gmr1_hip_mod_order_batch(int n, int sps, int in_len, const float *iq, uint64_t iq_len,
                             const uint64_t *offset, const float *freq_shift, int32_t *order);

/* ---- layer-1 channel decoding (soft bits in, L2 out) --------------------- */
int gmr1_hip_bcch_decode_batch_dev(void *stream, int n, const int8_t *ebits /* n x 424 */,
                                   uint8_t *l2 /* n x 24 */, int32_t *crc, int32_t *conv);
int gmr1_hip_ccch_decode_batch_dev(void *stream, int n, const int8_t *ebits /* n x 432 */,
                                   uint8_t *l2 /* n x 24 */, int32_t *crc, int32_t *conv);
int gmr1_hip_bcch_decode_batch(int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv);
int gmr1_hip_ccch_decode_batch(int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv);

/* ---- fused BCCH / CCCH receive: demod + descramble + deinterleave + Viterbi + CRC
 * kind[i]: 0 = BCCH burst (window 234*sps + 20*sps), 1 = CCCH on a DC6 burst
 * (window 234*sps + 10*sps), the windows gmr1_rx.c:759,809 cut.
 * crc[i]: 0 pass, 1 fail, -1 when the demodulator found no sync (rv[i] != 0). */
int gmr1_hip_rx_bcch_ccch_batch_dev(void *stream, int n, int sps,
                                    const float *iq, const uint64_t *offset, const uint8_t *kind,
                                    const float *freq_shift,
                                    uint8_t *l2 /* n x 24 */, int32_t *crc, int32_t *conv,
                                    float *toa, float *freq_err,
                                    int8_t *ebits /* n x 432, optional */,
                                    float *ssyms /* n x 234, optional */, int32_t *rv);
int gmr1_hip_rx_bcch_ccch_batch(int n, int sps,
                                const float *iq, uint64_t iq_len, const uint64_t *offset, const uint8_t *kind,
                                const float *freq_shift,
                                uint8_t *l2, int32_t *crc, int32_t *conv,
                                float *toa, float *freq_err,
                                int8_t *ebits, float *ssyms, int32_t *rv);

/* The same call on a POLYPHASE-PLANAR sample array (opt-in, 4 samples per symbol only): sample s of the flat array the
 * offsets count in is stored at iq_planes[(s % sps) * plane_stride + s / sps] (complex samples; plane_stride >=
 * ceil(total samples / sps)).  Nothing but addresses changes -- every output is bit-identical to the interleaved call's
 * on the same samples -- but the samples gmr1_pi4cxpsk_demod keeps after timing recovery (one per symbol from sample
 * round(toa) on, src/sdr/pi4cxpsk.c:292-295) are then 234 CONSECUTIVE samples of one plane instead of every fourth
 * sample of the whole window, which cuts the second read of a burst from every 128-byte line of its window to 15 of
 * them.  gmr1_hip_iq_to_planar_dev converts an interleaved array (any sps 1..16); the channelizer writes the layout
 * directly when asked (gmr1_hip_channelize_planar_dev). */
int gmr1_hip_rx_bcch_ccch_batch_planar_dev(void *stream, int n, int sps,
                                           const float *iq_planes, uint64_t plane_stride,
                                           const uint64_t *offset, const uint8_t *kind,
                                           const float *freq_shift,
                                           uint8_t *l2 /* n x 24 */, int32_t *crc, int32_t *conv,
                                           float *toa, float *freq_err,
                                           int8_t *ebits /* n x 432, optional */,
                                           float *ssyms /* n x 234, optional */, int32_t *rv);
int gmr1_hip_iq_to_planar_dev(void *stream, int sps, uint64_t n_samples, const float *iq /* interleaved, device */,
                              float *iq_planes /* device, sps x plane_stride complex samples */, uint64_t plane_stride);

/* ---- traffic channel layer 1 -------------------------------------------------
 * FACCH3: n frames, each 4 bursts x 104 soft bits (n x 416) -> l2 n x 10, optional
 * bits_s n x 32, crc / conv per frame; ciph optional n x 384 keystream bits.
 * TCH3: n speech bursts x 212 soft bits -> frames n x 2 x 10 (frame0 then frame1),
 * optional bits_s n x 4, conv n x 2; ciph optional n x 208; m = multiplexing mode. */
int gmr1_hip_facch3_decode_batch_dev(void *stream, int n, const int8_t *ebits, const uint8_t *ciph,
                                     uint8_t *l2, uint8_t *bits_s, int32_t *crc, int32_t *conv);
int gmr1_hip_facch3_decode_batch(int n, const int8_t *ebits, const uint8_t *ciph,
                                 uint8_t *l2, uint8_t *bits_s, int32_t *crc, int32_t *conv);
int gmr1_hip_tch3_decode_batch_dev(void *stream, int n, int m, const int8_t *ebits, const uint8_t *ciph,
                                   uint8_t *frames, uint8_t *bits_s, int32_t *conv);
int gmr1_hip_tch3_decode_batch(int n, int m, const int8_t *ebits, const uint8_t *ciph,
                               uint8_t *frames, uint8_t *bits_s, int32_t *conv);
/* What rx_tch3 does with a speech burst (src/gmr1_rx.c:551-587): gmr1_pi4cxpsk_demod of the NT3 speech format
 * (include/osmocom/gmr1/sdr/pi4cxpsk.h:101-105, src/sdr/nb.c gmr1_nt3_speech_burst), then gmr1_tch3_decode
 * (include/osmocom/gmr1/l1/tch3.h:35-37) of its 212 soft bits -- n bursts from samples to 2 x 10-byte speech frames.  The
 * outputs are those of gmr1_hip_demod_batch* (ebits n x 212, sync_id, toa, rv: optional except rv) followed by those of
 * gmr1_hip_tch3_decode_batch* (frames n x 20, bits_s n x 4, conv n x 2) and identical to calling the two in sequence; large
 * batches at 4 samples per symbol run as ONE launch with the soft bits kept on chip. */
int gmr1_hip_tch3_rx_batch_dev(void *stream, int n, int sps, int in_len,
                               const float *iq, const uint64_t *offset, const float *freq_shift,
                               int m, const uint8_t *ciph,
                               int8_t *ebits, int32_t *sync_id, float *toa, int32_t *rv,
                               uint8_t *frames, uint8_t *bits_s, int32_t *conv);
int gmr1_hip_tch3_rx_batch(int n, int sps, int in_len,
                           const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                           int m, const uint8_t *ciph,
                           int8_t *ebits, int32_t *sync_id, float *toa, int32_t *rv,
                           uint8_t *frames, uint8_t *bits_s, int32_t *conv);

/* ---- TCH3 follow-up pieces --------------------------------------------------
 * DKAB demodulation (gmr1_dkab_demod, include/osmocom/gmr1/sdr/dkab.h:39-41): n windows of in_len
 * samples (117 * sps + search window), p[i] = DKAB position; rv[i] = 0 found / 1 not found;
 * ebits n x 8 (zero where not found), toa in samples.
 * A5 keystream (gmr1_a5, include/osmocom/gmr1/l1/a5.h:37-41): one (key, frame number) per item,
 * keys n x 8 bytes, dl / ul n x nbits ubits (either may be NULL); alg 0 = zeros, 1 = A5/1. */
int gmr1_hip_dkab_demod_batch_dev(void *stream, int n, int sps, int in_len,
                                  const float *iq, const uint64_t *offset, const float *freq_shift,
                                  const int32_t *p, int8_t *ebits, float *toa, int32_t *rv);
int gmr1_hip_dkab_demod_batch(int n, int sps, int in_len,
                              const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                              const int32_t *p, int8_t *ebits, float *toa, int32_t *rv);
int gmr1_hip_a5_batch_dev(void *stream, int n, int alg, int nbits,
                          const uint8_t *keys, const uint32_t *fn, uint8_t *dl, uint8_t *ul);
int gmr1_hip_a5_batch(int n, int alg, int nbits, const uint8_t *keys, const uint32_t *fn, uint8_t *dl, uint8_t *ul);

/* ---- NT9 bursts (662 soft bits): FACCH9 and TCH9 ---------------------------------
 * FACCH9 (gmr1_facch9_decode, include/osmocom/gmr1/l1/facch9.h:39-41): n bursts -> l2 n x 38, sacch n x 10 and
 * status n x 4 soft bits (optional), crc (0 = pass), conv.  ciph: optional n x 658 keystream bits.
 * TCH9 (gmr1_tch9_decode, include/osmocom/gmr1/l1/tch9.h:40-53): mode 0 2k4 / 1 4k8 / 2 9k6
 * (enum gmr1_tch9_mode) -> l2 of 18 / 30 / 60 bytes per burst.  The bursts are n_chan sequences of seq_len
 * consecutive bursts each (channel after channel): the depth-3 inter-burst de-interleaver
 * (gmr1_deinterleave_inter, l1/interleave.h:52-56) runs along every sequence from an all-zero state, so
 * burst i of a sequence yields the block sent two bursts earlier.  No CRC (the reference has none). */
int gmr1_hip_facch9_decode_batch_dev(void *stream, int n, const int8_t *ebits, const uint8_t *ciph,
                                     uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv);
int gmr1_hip_facch9_decode_batch(int n, const int8_t *ebits, const uint8_t *ciph,
                                 uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv);
int gmr1_hip_tch9_decode_batch_dev(void *stream, int n_chan, int seq_len, int mode, const int8_t *ebits,
                                   const uint8_t *ciph, uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *conv);
int gmr1_hip_tch9_decode_batch(int n_chan, int seq_len, int mode, const int8_t *ebits, const uint8_t *ciph,
                               uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *conv);

/* ---- the two layer-1 decoders gmr1_rx does not call ----------------------------------------------------
 * xCH over DC12 (gmr1_xch_dc12_decode, include/osmocom/gmr1/l1/xch_dc12.h:38): ebits n x 432 -> l2 n x 24,
 * crc[n] (0 = pass), conv[n] (optional).  K = 9 rate 1/3 tail-biting, 256 states.
 * RACH (gmr1_rach_decode, include/osmocom/gmr1/l1/rach.h:38-39): ebits n x 494, sb_mask[n] -> rach n x 18,
 * rv[n] (0 = both CRCs pass), conv[n] and crc[n x 2] = {CRC8, CRC12} (both optional).
 * _dev: device pointers (ebits 4-byte, l2 2-byte aligned), asynchronous on `stream`. */
int gmr1_hip_xch_dc12_decode_batch_dev(void *stream, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc,
                                       int32_t *conv);
int gmr1_hip_xch_dc12_decode_batch(int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv);
int gmr1_hip_rach_decode_batch_dev(void *stream, int n, const int8_t *ebits, const uint8_t *sb_mask,
                                   uint8_t *rach, int32_t *rv, int32_t *conv, int32_t *crc);
int gmr1_hip_rach_decode_batch(int n, const int8_t *ebits, const uint8_t *sb_mask, uint8_t *rach, int32_t *rv,
                               int32_t *conv, int32_t *crc);

/* ---- transmit direction: channel encoders and modulator -------------------------------------------------
 * Batch forms of gmr1_{bcch,ccch,xch_dc12,facch3,tch3,facch9,tch9,rach}_encode (the headers under include/osmocom/gmr1/l1) and
 * of gmr1_pi4cxpsk_mod (sdr/pi4cxpsk.h:115-117).  Payloads are packed bytes, everything else one ubit per byte:
 *   bcch / xch_dc12: l2 n x 24 -> ebits n x 424 / 432;  ccch: l2 n x 24 -> n x 432
 *   facch3: l2 n x 10, bits_s n x 32, ciph n x 384 (optional) -> ebits n x 416 (four bursts of 104)
 *   tch3:   frames n x 2 x 10, bits_s n x 4, ciph n x 208 (optional), m -> ebits n x 212
 *   facch9: l2 n x 38, sacch n x 10, status n x 4, ciph n x 658 (optional) -> ebits n x 662
 *   tch9:   l2 n x 18 / 30 / 60 by mode; n = whole runs of seq_len consecutive bursts of one channel, the
 *           inter-burst interleaver starts empty at every run (as after gmr1_interleaver_init)
 *   rach:   rach n x 18, sb_mask n -> ebits n x 494
 *   mod:    ebits n x (ebits of the burst format) -> out n x len complex float32 symbols, sync sequence sync_id
 * _dev: device pointers, asynchronous on `stream` (mod_dev returns after its launch has finished). */
int gmr1_hip_bcch_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_bcch_encode_batch(int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_ccch_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_ccch_encode_batch(int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_xch_dc12_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_xch_dc12_encode_batch(int n, const uint8_t *l2, uint8_t *ebits);
int gmr1_hip_facch3_encode_batch_dev(void *stream, int n, const uint8_t *l2, const uint8_t *bits_s, const uint8_t *ciph,
                                     uint8_t *ebits);
int gmr1_hip_facch3_encode_batch(int n, const uint8_t *l2, const uint8_t *bits_s, const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_tch3_encode_batch_dev(void *stream, int n, int m, const uint8_t *frames, const uint8_t *bits_s,
                                   const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_tch3_encode_batch(int n, int m, const uint8_t *frames, const uint8_t *bits_s, const uint8_t *ciph,
                               uint8_t *ebits);
int gmr1_hip_facch9_encode_batch_dev(void *stream, int n, const uint8_t *l2, const uint8_t *sacch, const uint8_t *status,
                                     const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_facch9_encode_batch(int n, const uint8_t *l2, const uint8_t *sacch, const uint8_t *status,
                                 const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_tch9_encode_batch_dev(void *stream, int mode, int n, int seq_len, const uint8_t *l2, const uint8_t *sacch,
                                   const uint8_t *status, const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_tch9_encode_batch(int mode, int n, int seq_len, const uint8_t *l2, const uint8_t *sacch,
                               const uint8_t *status, const uint8_t *ciph, uint8_t *ebits);
int gmr1_hip_rach_encode_batch_dev(void *stream, int n, const uint8_t *rach, const uint8_t *sb_mask, uint8_t *ebits);
int gmr1_hip_rach_encode_batch(int n, const uint8_t *rach, const uint8_t *sb_mask, uint8_t *ebits);
int gmr1_hip_mod_batch_dev(void *stream, int burst_id, int sync_id, int n, const uint8_t *ebits, float *out);
int gmr1_hip_mod_batch(int burst_id, int sync_id, int n, const uint8_t *ebits, float *out);
/* The shaped modulator: symbols at one sample per symbol to demodulator-ready windows at sps samples per symbol, on the
 * device -- the pulse (raised cosine: what a demodulator behind a channelizer sees; root raised cosine: what a transmitter
 * sends; roll-off 0.35, cut at +-span symbols), a fraction of a sample of delay, a carrier offset, a phase and a level.
 * No framing, no overlapping bursts, no noise: a caller who wants noise adds it to the windows, or hands the windows to
 * gmr1_hip_carrier_mix* below, which places them on a carrier, overlapping where they must, over a noise floor.
 *   shape:      symbols n x len complex float32 (gmr1_hip_mod_batch's output, DKAB symbols, anything)
 *   mod_shaped: ebits n x (ebits of the burst format), sync_id per burst (NULL: sequence 0): the modulator and the shaper
 *               in one launch, float for float what shape gives on gmr1_hip_mod_batch's symbols
 * offset and in_len are those of gmr1_hip_demod_batch*: burst b's window is out[2*offset[b] .. 2*(offset[b] + in_len)), and
 * the same offset array and buffer go straight into the demodulator on the same stream.  Windows must not overlap.
 * Per burst, each array optional (NULL: 0, 0, 0, 0, 1): start, the window sample symbol 0 lands on (it may be negative or
 * past the window: the body is clipped at both ends); frac, a further delay in samples (the true arrival time is
 * start + frac); cfo in radians per sample; phase0 in radians; gain, linear.  With s[j] = 0 outside 0..len, window sample
 * k = 0..in_len is, for q = k - (start - span*sps), i = q div sps, p = q mod sps:
 *   x[k] = gain e^{j(phase0 + cfo k)} sum_{m=-span..span} s[i - span - m] g(m + (p - frac) / sps)
 * where 0 <= q < (len + 2 span) sps, and 0 elsewhere: every window is written in full.  The coefficients are evaluated in
 * double and rounded to float once; the phase is formed and the sum is taken in float.
 * -EINVAL, before anything is written: sps outside 1..16, span outside 1..8, an unknown pulse or burst_id, len outside
 * 1..2048, in_len < 1, n < 0, a NULL symbols / ebits / offset / out; the host forms also refuse a window that leaves the
 * out_len samples of out, windows that overlap and a sync_id outside the format's sequences (the _dev forms cannot see the
 * arrays: there a burst with such a sync_id has no symbols, and the rest is the caller's).  n == 0 returns 0.
 * _dev: device pointers, asynchronous on `stream`. */
enum gmr1_hip_pulse { GMR1_HIP_PULSE_RC = 0, GMR1_HIP_PULSE_RRC = 1 };   /* roll-off 0.35 both */
int gmr1_hip_shape_batch_dev(void *stream, int n, int len, int sps, int pulse, int span, int in_len,
                             const float *symbols, const uint64_t *offset, const int32_t *start,
                             const float *frac, const float *cfo, const float *phase0, const float *gain,
                             float *out, uint64_t out_len);
int gmr1_hip_shape_batch(int n, int len, int sps, int pulse, int span, int in_len,
                         const float *symbols, const uint64_t *offset, const int32_t *start,
                         const float *frac, const float *cfo, const float *phase0, const float *gain,
                         float *out, uint64_t out_len);
int gmr1_hip_mod_shaped_batch_dev(void *stream, int burst_id, int n, int sps, int pulse, int span, int in_len,
                                  const uint8_t *ebits, const int32_t *sync_id,
                                  const uint64_t *offset, const int32_t *start,
                                  const float *frac, const float *cfo, const float *phase0, const float *gain,
                                  float *out, uint64_t out_len);
int gmr1_hip_mod_shaped_batch(int burst_id, int n, int sps, int pulse, int span, int in_len,
                              const uint8_t *ebits, const int32_t *sync_id,
                              const uint64_t *offset, const int32_t *start,
                              const float *frac, const float *cfo, const float *phase0, const float *gain,
                              float *out, uint64_t out_len);
/* FCCH chirp windows: the one window kind the shaper cannot make.  A window writer under exactly the window contract of
 * gmr1_hip_shape_batch*: offset, in_len, start, frac, cfo, phase0, gain, out and out_len mean what they mean there, every
 * window is written in full, windows must not overlap, the NULL defaults are the same (0, 0, 0, 0, 1).  fcch_type: 0, 1, 2
 * as in the FCCH entries below; freq and len are those of gmr1_fcch_burst, gmr1_fcch3_lband_burst, gmr1_fcch3_sband_burst.
 * For q = k - start, 0 <= q < len sps:
 *   t = (q - frac) / sps - len / 2,   x[k] = gain e^{j(phase0 + cfo k)} sqrt(2) cos(freq 2 pi / len t^2)
 * and 0 elsewhere.  The chirp value is evaluated in double and rounded to float once, as the pulse coefficients are; the
 * rotation is the shaper's (phase formed in float), so a chirp and a burst given the same cfo / phase0 rotate alike.
 * -EINVAL, before anything is written: fcch_type outside 0..2, sps outside 1..16, in_len < 1, n < 0, a NULL offset / out;
 * the host form also refuses a window that leaves out_len and windows that overlap.  n == 0 returns 0.
 * _dev: device pointers, asynchronous on `stream`. */
int gmr1_hip_fcch_chirp_batch_dev(void *stream, int fcch_type, int n, int sps, int in_len,
                                  const uint64_t *offset, const int32_t *start,
                                  const float *frac, const float *cfo, const float *phase0, const float *gain,
                                  float *out, uint64_t out_len);
int gmr1_hip_fcch_chirp_batch(int fcch_type, int n, int sps, int in_len,
                              const uint64_t *offset, const int32_t *start,
                              const float *frac, const float *cfo, const float *phase0, const float *gain,
                              float *out, uint64_t out_len);
/* The carrier mixer: windows (the outputs of shape / mod_shaped / fcch_chirp, any layout, complex float32 in seg_iq) to
 * CARRIERS -- continuous streams with the windows overlap-added at absolute sample positions, a carrier offset and a noise
 * floor: what the FCCH acquisition, gmr1_hip_rx_run*, the streaming handles and the call followers read.  Which burst goes
 * where (the frame schedule) is the caller's.
 * Carrier c owns segments seg_first[c] .. seg_first[c + 1]; segment s is seg_iq[seg_src[s] .. seg_src[s] + seg_len[s]) and
 * its first sample lands on absolute sample seg_pos[s].  Carrier c is out[out_offset[c] .. out_offset[c] + length[c])
 * (gmr1_hip_rx_run*'s arrays) and its sample k has the absolute index n = first[c] + k (first NULL: 0).  Its value:
 *   1. acc = 0; for the carrier's segments IN LIST ORDER, each one with pos <= n < pos + len adds seg_iq[src + (n - pos)],
 *      one float add per component.  List order is the summation order: the result is reproducible bit for bit.
 *   2. if cfo[c] != 0 (radians per sample, double; NULL: 0): theta = cfo n formed in double, reduced to [-pi, pi] in double,
 *      rounded to float, through the accurate sincosf; acc = acc e^{j theta} in float.  (n passes 2^23 within 90 s at four
 *      samples per symbol: a float phase is not an option.)  cfo == 0 skips the step.
 *   3. if sigma[c] != 0 (deviation per component, so the noise power is 2 sigma^2; NULL: 0): acc += sigma z(seed, id, n), id =
 *      noise_id[c] (NULL: c).  z: Philox4x32-10 with key = (seed low, seed high) and counter = (j low, j high, id, 0),
 *      j = n >> 1; words w0, w1 belong to sample 2 j and w2, w3 to sample 2 j + 1; with (wa, wb) the sample's words,
 *      u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrtf(-2 logf(u1)), z = r (cospi(2 u2) + j sinpi(2 u2)).
 *      The noise is not rotated (it is circular).  sigma == 0 skips the step.
 *   4. every sample of every carrier is written, zeros where nothing lands; nothing else in out is touched.
 * z depends on the absolute index alone, and segments are clipped to the carrier (pos may be negative or past its end): a
 * carrier made in pieces (first = 0, a, b, ...) is sample for sample the carrier made in one call, so a stream of any
 * length needs bounded memory and can feed the streaming handles push by push.
 * Required of the caller, each carrier: segments sorted by pos, non-decreasing, and seg_len <= max_seg_len (the kernel finds
 * a sample's segments by a search over pos).  seg_first NULL (host form: n_seg == 0): no segments, noise and zeros only.
 * -EINVAL, before anything is written: n_carriers < 0, a NULL out_offset / length / out, segments present with a NULL
 * seg_iq / seg_src / seg_pos / seg_len or max_seg_len == 0; the host form, which sees the arrays, also: segments not sorted
 * or longer than max_seg_len, a segment that leaves seg_iq_len, seg_first not non-decreasing from 0 to n_seg, carriers that
 * overlap in out or leave out_len, length[c] > max_length, a negative or non-finite sigma.  n_carriers == 0 returns 0.
 * _dev: device pointers, asynchronous on `stream`, no scratch.  The host form copies seg_iq and the arrays in and the
 * carriers out (what lies between them in out stays). */
#define GMR1_HIP_CARRIER_MIX_TILE 1024      /* samples a work-group of the mixer owns (for tests of its edges) */
int gmr1_hip_carrier_mix_dev(void *stream, int n_carriers, const float *seg_iq, const int32_t *seg_first,
                             const uint64_t *seg_src, const int64_t *seg_pos, const uint32_t *seg_len, uint32_t max_seg_len,
                             const uint64_t *out_offset, const uint64_t *length, uint64_t max_length, const int64_t *first,
                             const float *sigma, const double *cfo, const uint32_t *noise_id, uint64_t seed, float *out);
int gmr1_hip_carrier_mix(int n_carriers, const float *seg_iq, uint64_t seg_iq_len, int n_seg, const int32_t *seg_first,
                         const uint64_t *seg_src, const int64_t *seg_pos, const uint32_t *seg_len, uint32_t max_seg_len,
                         const uint64_t *out_offset, const uint64_t *length, uint64_t max_length, const int64_t *first,
                         const float *sigma, const double *cfo, const uint32_t *noise_id, uint64_t seed,
                         float *out, uint64_t out_len);
/* The position map (payload bits -> burst bits) the encoder kernel evaluates for one chain, copied into buf as
 * struct EncPlan of osmo-gmr_amd/csrc/enc_plan.h; returns its size (buf may be NULL) or -EINVAL.  Host-only,
 * works without a GPU: tests/test_tx_plan.py evaluates it bit by bit against the CPU oracle. */
enum gmr1_hip_enc_chain {
	GMR1_HIP_ENC_BCCH = 0, GMR1_HIP_ENC_CCCH, GMR1_HIP_ENC_FACCH3, GMR1_HIP_ENC_TCH3_M0, GMR1_HIP_ENC_TCH3_M1,
	GMR1_HIP_ENC_FACCH9, GMR1_HIP_ENC_TCH9_2K4, GMR1_HIP_ENC_TCH9_4K8, GMR1_HIP_ENC_TCH9_9K6, GMR1_HIP_ENC_RACH,
	GMR1_HIP_ENC_XCH_DC12, GMR1_HIP_ENC__COUNT
};
int gmr1_hip_encoder_plan(int chain, void *buf, int buf_len);

/* ---- FCCH acquisition ------------------------------------------------------
 * fcch_type: 0 gmr1_fcch_burst, 1 gmr1_fcch3_lband_burst, 2 gmr1_fcch3_sband_burst.
 * rough: n search windows of `len` samples each -> toa[i] (samples), rv[i] (0 / -errno).
 * fine / snr: n bursts of exactly burst_len*sps samples each.
 * The rough sweep keeps a grow-only device scratch per GPU (decimated streams +
 * partials, about len/sps*8 bytes per stream). */
int gmr1_hip_fcch_rough_batch_dev(void *stream, int fcch_type, int n, int sps, int len,
                                  const float *iq, const uint64_t *offset, const float *freq_shift,
                                  int32_t *toa, int32_t *rv);
int gmr1_hip_fcch_rough_batch(int fcch_type, int n, int sps, int len,
                              const float *iq, uint64_t iq_len, const uint64_t *offset,
                              const float *freq_shift, int32_t *toa, int32_t *rv);
/* rough_multi: peaks_toa is n x N, count[i] = peaks found or -EINVAL (fcch.c:425-427) */
int gmr1_hip_fcch_rough_multi_batch_dev(void *stream, int fcch_type, int n, int sps, int len,
                                        const float *iq, const uint64_t *offset, const float *freq_shift,
                                        int32_t *peaks_toa, int N, int32_t *count);
int gmr1_hip_fcch_rough_multi_batch(int fcch_type, int n, int sps, int len,
                                    const float *iq, uint64_t iq_len, const uint64_t *offset,
                                    const float *freq_shift, int32_t *peaks_toa, int N, int32_t *count);
int gmr1_hip_fcch_fine_batch_dev(void *stream, int fcch_type, int n, int sps,
                                 const float *iq, const uint64_t *offset, const float *freq_shift,
                                 int32_t *toa, float *freq_error);
int gmr1_hip_fcch_fine_batch(int fcch_type, int n, int sps,
                             const float *iq, uint64_t iq_len, const uint64_t *offset,
                             const float *freq_shift, int32_t *toa, float *freq_error);
int gmr1_hip_fcch_snr_batch_dev(void *stream, int fcch_type, int n, int sps,
                                const float *iq, const uint64_t *offset, const float *freq_shift,
                                float *snr);
int gmr1_hip_fcch_snr_batch(int fcch_type, int n, int sps,
                            const float *iq, uint64_t iq_len, const uint64_t *offset,
                            const float *freq_shift, float *snr);
/* The whole acquisition gmr1_rx runs on a capture before it follows a carrier (main() -> fcch_single_init and
 * fcch_multi_process up to its survivor list, gmr1_rx.c:605-733) over n streams at once: rough over 330 ms from start[i],
 * fine, rough_multi over 650 ms, then fine and snr of every candidate, and the decisions between and behind them -- all on
 * the device, one record per stream.  It is what gmr1_hip_rx_run* does first; this call stops there and reports what that
 * one only uses.  Stream i is iq[offset[i] .. offset[i] + length[i]) (complex64; the layout a gmr1_hip_channelize* call
 * leaves its outputs in), length[i] at most 2^31 - 1; start may be NULL: 8000 everywhere, the samples gmr1_rx discards
 * (gmr1_rx.c:52).  The window lengths are the reference's whatever the fcch_type, the burst length is the type's.
 * _dev: iq, offset, length, start and out are device memory; the call enqueues on `stream` and returns -- no copy to the
 * host, no synchronisation (but for a scratch buffer that has to grow).  The host form copies iq (iq_len complex samples)
 * and the arrays in and the records out.  n == 0 does nothing.  -EINVAL: fcch_type outside 0..2, sps outside 1..16, n < 0,
 * a NULL array, iq not aligned to 8 bytes; host form also: a stream that leaves iq or is too long, a negative start (on
 * the device these two end that stream alone, status -EINVAL). */
#define GMR1_HIP_ACQ_MAX_CHAINS 16          /* the candidates rough_multi is asked for (mtoa[16], gmr1_rx.c:647) */
struct gmr1_hip_fcch_acq {
	int32_t status;        /* 0, or what gmr1_rx's main() would have exited with for this stream: -1 (not enough
	                          samples, at any of the reference's win_map checks, or a candidate outside the stream),
	                          rough's rv, rough_multi's negative count.  Not 0: every field below is 0 */
	int32_t n_chains;      /* survivors of fcch_multi_process: the chains gmr1_hip_rx_run* would follow */
	int32_t align;         /* start + rough toa + fine toa (fcch_single_init) */
	int32_t base_align;    /* max(0, align - burst_len*sps): where the 650 ms window begins */
	float   freq_err;      /* fcch_single_init's, as gmr1_fcch_fine returns it (Hz = 23400 x freq_err / 2 pi) */
	int32_t n_cand;        /* peaks rough_multi reported */
	/* the survivors, in candidate order (the first one is the strongest peak); slots at and past n_chains are 0 */
	int32_t chain_align[GMR1_HIP_ACQ_MAX_CHAINS];     /* base_align + peak + fine toa: first sample of the chain's FCCH */
	float   chain_freq_err[GMR1_HIP_ACQ_MAX_CHAINS];  /* the candidate's residual (fine with -freq_err applied) */
	float   chain_snr[GMR1_HIP_ACQ_MAX_CHAINS];       /* gmr1_fcch_snr with -(freq_err + residual) applied, linear */
};
int gmr1_hip_fcch_acquire_batch_dev(void *stream, int fcch_type, int n, int sps, const float *iq,
                                    const uint64_t *offset, const uint64_t *length, const int32_t *start,
                                    struct gmr1_hip_fcch_acq *out);
int gmr1_hip_fcch_acquire_batch(int fcch_type, int n, int sps, const float *iq, uint64_t iq_len,
                                const uint64_t *offset, const uint64_t *length, const int32_t *start,
                                struct gmr1_hip_fcch_acq *out);

/* Direct mode of the recorder script (utils/gmr1_rx_sdr.py:605-807, DirectOutputParameters / DirectOutputBranch): a few
 * carriers straight from the wideband stream, no filterbank.  Per carrier at freq_hz[i] from the centre:
 * filter.freq_xlating_fir_filter_ccc(decim1, low_pass(1, 1, .3 / decim1, .3 / decim1), f, fs), filter.fir_filter_ccc(decim2,
 * low_pass(1, 1, .45 / decim2, .1 / decim2)), pfb.arb_resampler_ccf(resamp, root_raised_cosine(32, ..., 0.35), 32) -- the
 * split chosen as the script's _select_decim does (2.0 Msps: 7, 6, 1.9656).  out: n_sel streams of *n_out complex64 at
 * 23400 x sps, out_stride complex samples apart.  -EINVAL for rates the reference itself cannot run (an exact multiple
 * of 23400 x sps), whose resampler has more than 96 taps per phase, or whose 64 output phases of a wave span more input
 * than the kernel's window for that bank holds (1.0 and 1.5 Msps at sps 1: 636 and 602 samples against 512) -- from the
 * plan, the one-shot calls and gmr1_hip_ddc_stream_create alike, before anything is launched. */
int gmr1_hip_ddc_plan(double samp_rate, int sps, uint64_t n_in, int32_t *decim1, int32_t *decim2, double *resamp,
                      uint64_t *n_out);
int gmr1_hip_ddc_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in, int n_sel,
                     const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_ddc(double samp_rate, int sps, const float *wide, uint64_t n_in, int n_sel, const double *freq_hz,
                 float *out, uint64_t out_stride, uint64_t *n_out);

/* ------------------------------------------------------------------------
 * Wideband capture -> per-ARFCN streams at sym_rate x sps (reference utils/gmr1_rx_sdr.py:391-602:
 * PFBBase = 2x oversampled polyphase channelizer over n_chans = (ceil(fs / 31.25 kHz) + 1) & ~1 channels
 * with firdes.low_pass(1, fs, 15.625 k, 7.8125 k); PFBOutputBranch = per-channel arbitrary resampler to
 * 23.4 k x sps with a 32-phase root-raised-cosine bank, alpha 0.35, 11 symbols).
 * Channel k is the carrier k x 31.25 kHz above the centre (k >= n_chans / 2: below, freq2index :478-485).
 * rotation: optional pre-rotation in rad / sample (:444-448).  chan_idx: n_sel channel numbers (host);
 * out: n_sel streams, out_stride complex samples apart; *n_out = samples written per stream.
 * n_chans even and <= 256 (64 channels / 2.0 Msps is the fast path).  A sample rate (whole Hz) that is not
 * n_chans x 31.25 kHz is first resampled to that rate by a 32-phase arbitrary resampler (:413-417, :453-461:
 * pfb.arb_resampler_ccf(rate, taps=None, flt_size=32)) -- a branch that cannot run in the reference as written
 * (it reads self.samp_rate before anything sets it); built to its evident intent, with the library's own
 * prototype for the resampler (GNU Radio's default design is not restatable: csrc/chan_plan.h,
 * design_pre_resampler).  The multi-ARFCN synthesizer (:567-576) is not built.
 * gmr1_hip_channelize_plan reports sizes: n_mid = 2x oversampled samples per channel.
 * gmr1_hip_channelize_planar_dev writes the n_sel streams POLYPHASE-PLANAR, the layout
 * gmr1_hip_rx_bcch_ccch_batch_planar_dev reads: sample m of stream i is flat sample g = i x out_stride + m and
 * goes to out_planes[(g % sps) * plane_stride + g / sps]  (plane_stride >= ceil(n_sel x out_stride / sps)). */
int gmr1_hip_channelize_plan(double samp_rate, int sps, uint64_t n_in,
                             int32_t *n_chans, uint64_t *n_mid, uint64_t *n_out);
int gmr1_hip_channelize_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in,
                            float rotation, int n_sel, const int32_t *chan_idx,
                            float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_channelize(double samp_rate, int sps, const float *wide, uint64_t n_in, float rotation,
                        int n_sel, const int32_t *chan_idx, float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_channelize_planar_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in,
                                   float rotation, int n_sel, const int32_t *chan_idx,
                                   float *out_planes, uint64_t out_stride, uint64_t plane_stride, uint64_t *n_out);

/* Streaming form of the two front ends above, for a capture that arrives in pieces (an SDR read loop, a file read block by
 * block): a handle, created once per (mode, sample rate, sps, selection) on the current device, carries the filters'
 * history, the resamplers' phases and the direct mode's decimation and mixer phases from one push to the next.  A push of
 * the next n_in wideband samples writes, per selected stream, exactly the outputs that have become computable:
 * n_out(N + n_in) - n_out(N), N = samples pushed before, n_out() the one-shot count (gmr1_hip_channelize_plan /
 * gmr1_hip_ddc_plan).  The outputs of any sequence of pushes, concatenated, are IDENTICAL to one gmr1_hip_channelize /
 * gmr1_hip_ddc call on the same samples (any chunk sizes, 0 included; no flush is needed: every output is causal).
 * Creation refuses what the one-shot calls refuse (-EINVAL).  gmr1_hip_chan_stream_out_len: the count the next push of
 * n_in samples will write (host arithmetic).  _push_dev enqueues on `stream` and returns (wide, out: device memory the
 * caller keeps alive until the stream has run); pushes on one handle are ordered, from any thread and any stream (a push
 * on another stream than the previous one waits for it); a refused push (-EINVAL) leaves the handle as it was.  The handle
 * owns its device memory (the input's tail, grow-only intermediate streams): after the first push of a size, pushes
 * allocate nothing.  _push: host arrays, synchronous.  _destroy waits for the handle's last push. */
struct gmr1_hip_chan_stream;
int gmr1_hip_channelize_stream_create(double samp_rate, int sps, float rotation, int n_sel, const int32_t *chan_idx,
                                      struct gmr1_hip_chan_stream **h);
int gmr1_hip_ddc_stream_create(double samp_rate, int sps, int n_sel, const double *freq_hz,
                               struct gmr1_hip_chan_stream **h);
int gmr1_hip_chan_stream_out_len(const struct gmr1_hip_chan_stream *h, uint64_t n_in, uint64_t *n_out);
int gmr1_hip_chan_stream_push_dev(void *stream, struct gmr1_hip_chan_stream *h, const float *wide, uint64_t n_in,
                                  float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_chan_stream_push(struct gmr1_hip_chan_stream *h, const float *wide, uint64_t n_in,
                              float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_chan_stream_destroy(struct gmr1_hip_chan_stream *h);

/* The same front ends on captures as radios and archives hold them: `wide` is interleaved I, Q of the format named by fmt --
 * GMR1_HIP_IQ_F32 (float, 8 bytes per complex sample), _S16 (int16_t, 4 bytes: a USRP's sc16) or _S8 (int8_t, 2 bytes) -- and
 * a sample's value is its integer x 2^-15 (S16) or x 2^-7 (S8), so -32768 and -128 are -1.0.  The integers are read by the
 * first kernel of the chain itself (a quarter or a half of the float's bytes, uploaded by the host forms and read on the
 * device); only a sample rate off the n_chans x 31.25 kHz grid converts to float first, in front of its pre-resampler.
 * The conversion is exact, so every output of an _iq call or push sequence is BIT-IDENTICAL to the float entry's on
 * (float)v x 2^-k, and a streamed integer capture equals the one-shot integer call.  Everything else -- outputs, counts,
 * strides, refusals, threading, stream ordering, -ENODEV without a device -- is the float entry's, and with GMR1_HIP_IQ_F32 an
 * _iq entry IS the float entry.  Any other fmt: -EINVAL, before anything is allocated.  `wide` needs the alignment of one
 * complex sample only (4 bytes S16, 2 bytes S8): a _dev pointer may lie any number of samples into an allocation.
 * A stream handle has one format for life: _create_iq sets it (the plain _create calls make F32 handles), _push_iq* read
 * `wide` in it; the float _push* on a handle of another format are refused (-EINVAL, the handle stays as it was).
 * gmr1_hip_iq_sample_bytes: 8 / 4 / 2 bytes per complex sample, -EINVAL for any other fmt; host arithmetic, no device
 * needed.  Unsigned (offset-binary) 8-bit samples are not a format: their centre is a convention of the source. */
enum { GMR1_HIP_IQ_F32 = 0, GMR1_HIP_IQ_S16 = 1, GMR1_HIP_IQ_S8 = 2 };
int gmr1_hip_iq_sample_bytes(int fmt);
int gmr1_hip_channelize_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in,
                               float rotation, int n_sel, const int32_t *chan_idx,
                               float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_channelize_iq(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, float rotation,
                           int n_sel, const int32_t *chan_idx, float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_channelize_planar_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in,
                                      float rotation, int n_sel, const int32_t *chan_idx,
                                      float *out_planes, uint64_t out_stride, uint64_t plane_stride, uint64_t *n_out);
int gmr1_hip_ddc_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel,
                        const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_ddc_iq(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel,
                    const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_channelize_stream_create_iq(double samp_rate, int sps, int fmt, float rotation, int n_sel,
                                         const int32_t *chan_idx, struct gmr1_hip_chan_stream **h);
int gmr1_hip_ddc_stream_create_iq(double samp_rate, int sps, int fmt, int n_sel, const double *freq_hz,
                                  struct gmr1_hip_chan_stream **h);
int gmr1_hip_chan_stream_push_iq_dev(void *stream, struct gmr1_hip_chan_stream *h, const void *wide, uint64_t n_in,
                                     float *out, uint64_t out_stride, uint64_t *n_out);
int gmr1_hip_chan_stream_push_iq(struct gmr1_hip_chan_stream *h, const void *wide, uint64_t n_in,
                                 float *out, uint64_t out_stride, uint64_t *n_out);

/* ------------------------------------------------------------------------
 * The gmr1_rx receive loop over many BCCH carriers (reference src/gmr1_rx.c:605-895 and
 * main() :897-975, one process per capture file there).
 *
 * Carrier i is the complex64 stream iq[offset[i] .. offset[i]+length[i]) at sps samples per
 * symbol (offset / length / arfcn / out / status / n_chains are HOST arrays; iq is a device
 * pointer for _dev, a host pointer otherwise).  For every carrier: FCCH acquisition
 * (fcch_single_init), multi-FCCH survivor selection (fcch_multi_process), then per chain the
 * BCCH / CCCH frame loop with its time / frequency / SI1 TDMA feedback (process_bcch, rx_bcch,
 * rx_ccch, bcch_tdma_align).  Every frame whose CRC passed comes back as one record -- what the
 * reference hands to gsmtap_sendmsg (gmr1_rx.c:793-795, 845-847) -- ordered by carrier, chain,
 * time.  n_records = records found (only the first max_records are stored).
 * status[i] = 0 or the negative value main() would have exited with for that carrier;
 * n_chains[i] = FCCH chains followed.  TCH follow-up after IMM.ASS is not performed.
 * arfcn may be NULL (records then carry the carrier index).
 * `out` of gmr1_hip_rx_run_dev may be pageable host memory, pinned / registered host memory (hipHostMalloc,
 * hipHostRegister) or DEVICE memory: the records are closed up on the device in the order above and copied once,
 * exactly as many as there are -- straight into a pinned or device buffer (no staging copy; a device buffer is what
 * gmr1_hip_rx_run_sharded sends from), through the library's pinned block for pageable memory. */
struct gmr1_hip_rx_record {
	uint16_t arfcn;
	uint8_t  chain;      /* FCCH chain within the carrier          */
	uint8_t  type;       /* 1 = GSMTAP_GMR1_BCCH, 2 = GSMTAP_GMR1_CCCH */
	uint32_t fn;
	uint8_t  tn;
	uint8_t  crc;        /* always 0: only frames whose CRC passed */
	uint8_t  len;        /* 24                                     */
	uint8_t  pad;
	int32_t  conv;       /* Viterbi path metric, as logged by the reference */
	uint8_t  l2[24];
};

int gmr1_hip_rx_run_dev(void *stream, int n_arfcn, int sps, const float *iq,
                        const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                        struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                        int32_t *status, int32_t *n_chains);
int gmr1_hip_rx_run(int n_arfcn, int sps, const float *iq, uint64_t iq_len,
                    const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                    struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                    int32_t *status, int32_t *n_chains);

/* The receive loop over a capture pushed piece by piece: gmr1_hip_rx_run for a live receiver, with bounded memory and no
 * capture-length limit.  Carrier i's next n complex64 samples are iq[2*(i*iq_stride + k)], k < n -- the layout of a
 * gmr1_hip_chan_stream push's `out`, which can go straight in on the same HIP stream.  last != 0: these are the capture's
 * final samples (n may be 0).  arfcn may be NULL (records carry the carrier index); sps 1..16 as for gmr1_hip_rx_run.
 *  - Each push returns exactly the records that became final in it, ordered by carrier, chain, time.  The records of any
 *    sequence of pushes ending with `last`, concatenated and stable-sorted by (carrier, chain), are byte-identical to one
 *    gmr1_hip_rx_run call on the whole capture (every field, conv included), for any push sizes (0 included) and in both
 *    Viterbi decoder modes; after the last push _status's status / n_chains equal that call's.
 *  - The FCCH acquisition runs once 8000 + 330 ms + 650 ms + 3 FCCH bursts of samples are in (earlier on `last`); before
 *    that a carrier keeps everything, after it what its chains can still reach: from 2 frames before the earliest chain,
 *    a carrier whose acquisition failed nothing.  _status reports, per carrier, status (0 while undecided or fine),
 *    chains followed and the samples the handle retains.
 *  - A push with max_records below gmr1_hip_rx_stream_max_records(h, n) (host arithmetic) is refused with -EINVAL, as
 *    are bad arguments and a push after `last`; a refused push leaves the handle as it was.  -EIO: the handle failed and
 *    takes no further pushes.
 *  - `out` takes what gmr1_hip_rx_run_dev's does.  A push is synchronous: it returns when its records are in `out`.
 *    _push_dev: iq is device memory, read on `stream`; _push: host memory.  Pushes on one handle are ordered, from any
 *    thread or stream; independent handles may be pushed concurrently (they take turns on the device's workspace).  A
 *    handle belongs to the device current when it was created: a push from a thread whose current device is another
 *    one is refused (-EINVAL).
 *  - A chain whose walk outgrows the loop's buffers stops for good and its carrier's status becomes -EIO, as in
 *    gmr1_hip_rx_run; the carrier's other chains go on.
 *  - A handle made by _create follows no traffic channel; one made by _create_tch (below) follows TCH3 calls, one made
 *    by _create_full (below that) TCH3 and TCH9 calls.  Without a GPU every entry point returns -ENODEV. */
struct gmr1_hip_rx_stream;
int gmr1_hip_rx_stream_create(int n_arfcn, int sps, const uint16_t *arfcn, struct gmr1_hip_rx_stream **h);
int gmr1_hip_rx_stream_max_records(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_records);
int gmr1_hip_rx_stream_push_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride,
                                uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records);
int gmr1_hip_rx_stream_push(struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n,
                            int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records);
int gmr1_hip_rx_stream_status(const struct gmr1_hip_rx_stream *h, int32_t *status, int32_t *n_chains,
                              uint64_t *retained);
int gmr1_hip_rx_stream_destroy(struct gmr1_hip_rx_stream *h);

/* The streaming loop with the TCH3 follow-up: gmr1_hip_rx_run_tch over a capture pushed piece by piece.  kc = n_arfcn x 8
 * key bytes (NULL: the all-zero key).  `tch` has the layout, stride and timing of `iq`: carrier i's traffic samples of a
 * push are tch[2*(i*iq_stride + k)], k < n (a channelizer-stream push with twice the channels feeds both).
 *  - A handle made by _create_tch takes only _push_tch*, one made by _create only _push*: the wrong pairing is refused
 *    (-EINVAL) and leaves the handle as it was, as does tch == NULL with n > 0.  _max_records, _status and _destroy serve
 *    both kinds; for a tch handle _max_records adds one record per frame a chain's walk can log (a frame gives at most
 *    one TCH3 record).
 *  - The records of any sequence of pushes ending with `last`, stable-sorted by (carrier, chain), are byte-identical to
 *    one gmr1_hip_rx_run_tch call on the whole capture with the same kc: every field, conv included, in both Viterbi
 *    decoder modes, for any push sizes (0 included).  Within a push they come by carrier, chain, frame; a frame's BCCH /
 *    CCCH records before its TCH3 record.  An IMMEDIATE ASSIGNMENT is followed from its own frame on, so the call's
 *    records start in the push that returns the assignment.
 *  - The traffic samples are retained exactly as the BCCH carrier's are (_status's `retained` holds for both); every
 *    chain's struct gmr1_hip_tch3_state stays in device memory between pushes.
 *  - `out` is host memory.  Everything else is as for gmr1_hip_rx_stream_push*.
 *  - -EIO (the handle takes no further pushes) also when a frame the walk admitted does not hold its traffic window: an
 *    SI1 that moves a chain's timeslot label down by more than 13 slots inside the newest frame of a push that is not
 *    the last.  gmr1_hip_rx_run_tch has no such limit. */
int gmr1_hip_rx_stream_create_tch(int n_arfcn, int sps, const uint16_t *arfcn,
                                  const uint8_t *kc /* n_arfcn x 8, or NULL */, struct gmr1_hip_rx_stream **h);
int gmr1_hip_rx_stream_push_tch_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                    uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out,
                                    int max_records, int *n_records);
int gmr1_hip_rx_stream_push_tch(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride,
                                uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records);

/* The streaming loop with the followed calls decoded to audio: gmr1_hip_rx_run_voice (below) over a capture pushed piece
 * by piece.  kc, tch and the records are the tch handle's; audio_out (host memory) takes struct gmr1_hip_rx_audio blocks.
 *  - A handle made by _create_voice takes only _push_voice*, and _push_voice* takes no other handle: the wrong pairing is
 *    refused (-EINVAL) and leaves the handle as it was, as do max_audio below gmr1_hip_rx_stream_max_audio(h, n), a NULL
 *    n_audio and audio_out == NULL with max_audio > 0; n_records and n_audio are then 0.  _max_records is the tch
 *    handle's; _max_audio (host arithmetic; 0 for the other kinds) is one block per frame a chain's walk can log, times
 *    the chains -- what _max_big counts.  _status and _destroy serve all kinds.
 *  - The handle keeps one AMBE decoder state per chain in device memory beside the chain's struct gmr1_hip_tch3_state,
 *    and each chain's count of assignments on the host: a call's audio goes on in the next push where this one left it.
 *  - The audio of any sequence of pushes ending with `last`, stable-sorted by (carrier, chain), is byte-identical to the
 *    audio_out of one gmr1_hip_rx_run_voice call on the whole capture with the same kc, and the records to its `out`, for
 *    any push sizes (0 included) and in both Viterbi decoder modes.  Within a push both come by carrier, chain, frame; a
 *    call's first blocks come out of the push that returns its IMMEDIATE ASSIGNMENT.
 *  - Everything else, -EIO included, is as for gmr1_hip_rx_stream_push_tch*.  Audio on a _create_full handle is not
 *    provided. */
struct gmr1_hip_rx_audio;            /* defined with gmr1_hip_tch3_frames_to_audio_dev below */
int gmr1_hip_rx_stream_create_voice(int n_arfcn, int sps, const uint16_t *arfcn,
                                    const uint8_t *kc /* n_arfcn x 8, or NULL */, struct gmr1_hip_rx_stream **h);
int gmr1_hip_rx_stream_max_audio(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_audio);
int gmr1_hip_rx_stream_push_voice_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                      uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out,
                                      int max_records, int *n_records,
                                      struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio);
int gmr1_hip_rx_stream_push_voice(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride,
                                  uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                  struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio);

/* The streaming loop with both follow-ups: gmr1_hip_rx_run_full (below) over a capture pushed piece by piece.  kc as for
 * _create_tch.  `csd` has the layout, stride and timing of `iq` and `tch`: carrier i's CSD samples of a push are
 * csd[2*(i*iq_stride + k)], k < n.
 *  - A handle made by _create_full takes only _push_full*, and _push_full* takes no other handle: the wrong pairing is
 *    refused (-EINVAL) and leaves the handle as it was, as do tch == NULL or csd == NULL with n > 0, max_big below
 *    gmr1_hip_rx_stream_max_big(h, n) and big_out == NULL with max_big > 0; n_records and n_big are then 0.
 *    _max_records for a full handle is the tch handle's; _max_big (host arithmetic; 0 for the other kinds) is one big
 *    record per frame a chain's walk can log, times the chains.  _status and _destroy serve all kinds, and the plain and
 *    tch handles are what they were.
 *  - The ordinary records of any sequence of pushes ending with `last`, stable-sorted by (carrier, chain), are
 *    byte-identical to the `out` of one gmr1_hip_rx_run_full call on the whole capture with the same kc, and the big
 *    records, sorted the same way, to its `big_out`: every field, conv included, in both Viterbi decoder modes, for any
 *    push sizes (0 included).  Within a push both arrays come by carrier, chain, frame.  An ASSIGNMENT COMMAND 1 is
 *    followed from its own frame on, so the call's first big records come out of the push that returns the FACCH3 record
 *    carrying the command.
 *  - The CSD samples are retained exactly as the other two carriers' are; every chain's struct gmr1_hip_tch9_state stays
 *    in device memory between pushes, and a push runs the TCH9 call follower once, however many commands it holds.
 *  - `out` and `big_out` are host memory.  Everything else is as for gmr1_hip_rx_stream_push_tch*, its -EIO included: a
 *    frame the walk admitted holds its NT9 window (351 sps + sps + sps/2 samples) unless an SI1 moves the chain's timeslot
 *    label down by more than 7 slots (a call on timeslot 31; 23 slots up to timeslot 15) inside the newest frame of a
 *    push that is not the last.
 *  - The NT9 window passes GMR1_HIP_MAX_IN_LEN from sps 12 on: _create_full refuses sps > 11 (-EINVAL) when it is called,
 *    before anything is allocated.  gmr1_hip_rx_run_full takes such a capture and fails only once it meets an NT9 frame. */
struct gmr1_hip_rx_big_record;       /* defined with gmr1_hip_rx_run_full below */
int gmr1_hip_rx_stream_create_full(int n_arfcn, int sps, const uint16_t *arfcn,
                                   const uint8_t *kc /* n_arfcn x 8, or NULL */, struct gmr1_hip_rx_stream **h);
int gmr1_hip_rx_stream_max_big(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_big);
int gmr1_hip_rx_stream_push_full_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                     const float *csd, uint64_t iq_stride, uint64_t n, int last,
                                     struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                     struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big);
int gmr1_hip_rx_stream_push_full(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, const float *csd,
                                 uint64_t iq_stride, uint64_t n, int last,
                                 struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                 struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big);

/* The same with the TCH3 follow-up (gmr1_rx's optional tch.cfile and key arguments, gmr1_rx.c:355-600,
 * 897-975): tch holds, for every carrier, the traffic carrier an IMMEDIATE ASSIGNMENT on its CCCH points
 * to -- same offset[] / length[] layout and timing as iq; kc = n_arfcn x 8 key bytes (NULL: the all-zero
 * key the reference starts with).  After an assignment every frame's burst on the assigned timeslot is
 * classified (energy -> DKAB | burst; burst -> FACCH3 | speech by sync detection), FACCH3 bursts are
 * grouped by sync sequence and decoded (type 0x12 = GSMTAP_GMR1_TCH3 | GSMTAP_GMR1_FACCH, 10 bytes,
 * fn = fn of the flush - 3), with A5/1 deciphering once a message only decodes ciphered.  Speech bursts
 * come back as type 0x10 records of 20 bytes (two 10-byte frames; conv = conv0 | conv1 << 16) -- the
 * reference decodes them but only logs them.  tch = NULL is gmr1_hip_rx_run*. */
int gmr1_hip_rx_run_tch_dev(void *stream, int n_arfcn, int sps, const float *iq, const float *tch,
                            const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                            const uint8_t *kc,
                            struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                            int32_t *status, int32_t *n_chains);
int gmr1_hip_rx_run_tch(int n_arfcn, int sps, const float *iq, const float *tch, uint64_t iq_len,
                        const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                        struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                        int32_t *status, int32_t *n_chains);

/* The same with the followed calls decoded to audio: gmr1_hip_rx_run_tch* plus struct gmr1_hip_rx_audio blocks (defined
 * with gmr1_hip_tch3_frames_to_audio_dev below; audio_out is host memory).  The records, status and n_chains are
 * byte-identical to gmr1_hip_rx_run_tch* on the same inputs.  Every chain with an assignment owns one AMBE decoder, made
 * fresh (gmr1_hip_codec_init_dev, flags 0: what gmr1_ambe_decode computes) by every IMMEDIATE ASSIGNMENT the chain
 * follows; every frame the follower walks with the call running gives one block -- a speech frame its 320 samples and two
 * verdicts, every other frame 320 zeros -- with `call` counting the chain's assignments from 1.  The decoder runs behind
 * the follower on the frames where they lie in device memory; no frame and no decoder state visits the host for it.
 * Blocks come ordered by carrier, chain, frame.  Only the first max_audio blocks are stored; *n_audio is the number found.
 * tch == NULL gives no audio and gmr1_hip_rx_run*'s records.  -EINVAL also for a NULL n_audio, a negative max_audio, and
 * a NULL audio_out with max_audio > 0. */
struct gmr1_hip_rx_audio;
int gmr1_hip_rx_run_voice_dev(void *stream, int n_arfcn, int sps, const float *iq, const float *tch,
                              const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                              const uint8_t *kc,
                              struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                              int32_t *status, int32_t *n_chains,
                              struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio);
int gmr1_hip_rx_run_voice(int n_arfcn, int sps, const float *iq, const float *tch, uint64_t iq_len,
                          const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                          struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                          int32_t *status, int32_t *n_chains,
                          struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio);

/* ---- following a voice call: rx_tch3 over many calls at once (gmr1_rx.c:355-600) ------------------------
 * What gmr1_rx does per frame once an IMMEDIATE ASSIGNMENT has named a timeslot -- burst energy against the running
 * DKAB / burst averages, DKAB search or burst type detection, FACCH3 bursts grouped by sync sequence and decoded every
 * four bursts or at a sync change, speech bursts decoded, A5/1 deciphering switched on by the first message that only
 * decodes ciphered -- for n_calls calls in one invocation, every decision taken on the device.  The state of a call is
 * the caller's: struct gmr1_hip_tch3_state goes in and comes back, so a call is continued by the next invocation with
 * the frames that follow (as the speech decoder's state is, gmr1_hip_codec_*).  The caller finds the call: timeslot,
 * DKAB position and key come from its own control plane (or from a type-2 record of gmr1_hip_rx_run*), and it cuts
 * the windows as burst_map does (gmr1_rx.c:149-170).
 *
 * Call c owns frames first[c] .. first[c+1]-1 in time order; first[0] = 0, first[n_calls] = n_frames, non-decreasing.
 * Frame k's window is iq[offset[k] .. offset[k] + in_len) (complex64), offset = carrier start + align + sps*tn*39 - e_toa
 * with in_len = 117*sps + sps + sps/2 and e_toa = (in_len - 117*sps) >> 1 (gmr1_rx.c:549-551; the entry derives e_toa from
 * in_len the same way); a frame whose window does not fit is not handed in (burst_map fails: rx_tch3 returns before it
 * touches anything).  freq_shift[k] = -freq_err of the frame (rad/symbol), fn[k] its frame number.
 * One record per frame handed in comes back at out[k]; a frame yields at most one payload (a speech burst: its two
 * frames; a FACCH3 burst: at most one flush -- at a sync change or as the fourth burst, never both).  In both Viterbi
 * decoder modes (gmr1_hip_set_conv_decoder) payloads and conv follow the selected mode.
 *
 * _dev: every pointer is device memory; the call enqueues on `stream` and returns -- no copy to the host and no
 * synchronisation (but for the workspace that has to grow).  The host form copies iq (iq_len complex samples) and the
 * arrays in, state and out back.  n_calls == 0 or n_frames == 0 does nothing; a call without frames keeps its state
 * untouched.  -EINVAL: sps outside 1..16, in_len below 117*sps or above GMR1_HIP_MAX_IN_LEN, a negative count, a NULL
 * array, iq not aligned to 8 bytes; host form also: first not as described, a window that leaves iq (on the device the
 * entries of first are clamped to 0..n_frames).  -ENODEV without a device.  Nothing is written on either. */
struct gmr1_hip_tch3_state {        /* struct tch3_state of gmr1_rx.c:59-78 plus the key; all-zero = no call */
	int32_t  active;            /* 0: every frame is GMR1_HIP_TCH3_OFF and nothing changes */
	int32_t  p;                 /* DKAB position (IMMEDIATE ASSIGNMENT) */
	int32_t  ciph;              /* A5/1 deciphering is on (set by the first FACCH3 message that only decodes ciphered) */
	int32_t  weak_cnt;          /* consecutive frames without DKAB or burst; the tenth ends the call */
	int32_t  sync_id;           /* sync sequence of the FACCH3 message being collected */
	int32_t  burst_cnt;         /* its bursts so far */
	float    energy_dkab, energy_burst;   /* running averages; threshold = (energy_dkab + energy_burst) / 4 */
	uint32_t bi_fn[4];          /* frame number of each stored burst (A5/1 runs per burst), 0xffffffff: none */
	int8_t   ebits[4 * 104];    /* the stored bursts' soft bits, burst fn & 3 at 104 * (fn & 3) */
	uint8_t  kc[8];             /* the call's key */
};                                  /* 472 bytes */

enum { GMR1_HIP_TCH3_OFF = 0, GMR1_HIP_TCH3_DKAB, GMR1_HIP_TCH3_DKAB_MISSING, GMR1_HIP_TCH3_FACCH,
       GMR1_HIP_TCH3_SPEECH, GMR1_HIP_TCH3_ERR };

struct gmr1_hip_tch3_frame {        /* one per frame handed in, in the order handed in; 40 bytes */
	uint8_t  cls;       /* what rx_tch3 did with the frame (enum above); OFF: the call was not active; ERR: the DKAB
	                       search, the detector or the demodulator refused the window (rx_tch3 returns rv < 0) */
	uint8_t  type;      /* 0 nothing to report | 0x10 two speech frames | 0x12 a FACCH3 message whose CRC passed */
	uint8_t  len;       /* 0 | 20 | 10 */
	uint8_t  ciph;      /* the payload was deciphered */
	uint32_t fn;        /* speech: the frame's fn; FACCH3: fn of the flush - 3 (gmr1_rx.c:432-436) */
	int32_t  conv;      /* as gmr1_hip_rx_run_tch reports it (speech: conv0 & 0xffff | conv1 << 16) */
	float    energy;    /* burst_energy of the window (of every frame handed in, whatever its class) */
	uint8_t  l2[20];    /* type 0 / len 10: the rest is 0 */
	uint8_t  pad[4];    /* 0 */
};

/* rx_tch3_init (gmr1_rx.c:358-378) on a caller-held state: host arithmetic, needs no device.  Sets active, p, the two
 * energies from ref_energy (gmr1_rx takes burst_energy of the CCCH burst that carried the assignment), weak_cnt, sync_id,
 * clears ebits -- and, like the reference, leaves ciph, burst_cnt, bi_fn (and kc) as they are.  -EINVAL: s is NULL. */
int gmr1_hip_tch3_state_assign(struct gmr1_hip_tch3_state *s, int p, float ref_energy);
/* The same on states in device memory, between two invocations of gmr1_hip_tch3_follow_batch_dev, so that a call's state
 * never visits the host: for j < n what gmr1_hip_tch3_state_assign(&state[call[j]], p[j], ref_energy[j]) does, in the order
 * of j (a call named twice gets both; call[j] < 0 is skipped).  call, p, ref_energy and state are device memory; the entry
 * enqueues on `stream` and returns.  -EINVAL: n < 0 or a NULL array; -ENODEV without a device. */
int gmr1_hip_tch3_state_assign_batch_dev(void *stream, int n, const int32_t *call, const int32_t *p,
                                         const float *ref_energy, struct gmr1_hip_tch3_state *state);

int gmr1_hip_tch3_follow_batch_dev(void *stream, int n_calls, int sps, int in_len, const float *iq,
                                   const int32_t *first /* n_calls + 1 */, int n_frames,
                                   const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                                   struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out);
int gmr1_hip_tch3_follow_batch(int n_calls, int sps, int in_len, const float *iq, uint64_t iq_len,
                               const int32_t *first, int n_frames,
                               const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                               struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out);

/* ---- a followed voice call to audio: the follower's records through the AMBE decoder, on the device ------------
 * gmr1_rx logs the speech bursts it decodes and gmr1_ambe_decode reads a file of frames (src/gmr1_rx.c:551-600,
 * src/gmr1_ambe_decode.c:122-150); here the records of n_calls calls of any lengths go to 8 kHz PCM in one launch, one
 * wavefront per call.  Call c owns records first[c] .. first[c+1]-1 of `frames`, as in the follower.  Record k gives
 * pcm[320 k .. 320 k + 320) and, where rv is given, rv[2 k], rv[2 k + 1]:
 *   type 0x10    l2[0..10) is decoded into samples 0..159 and l2[10..20) into samples 160..319, exactly as
 *                gmr1_hip_codec_decode_batch* decodes two consecutive frames (tone and silence frames included); rv gets
 *                the two verdicts (0, or -EINVAL for a tone frame with an unassigned code).
 *   any other    (type 0, 0x12; class OFF, DKAB, DKAB_MISSING, FACCH, ERR) 320 zero samples, rv 0, 0, and the decoder is
 *                not touched: two gmr1_codec_decode_dtx calls (src/codec/ambe.c:130-141).  Only `type` is looked at;
 *                l2 of such a record is ignored whatever it holds.
 * codec_state: gmr1_hip_codec_state_bytes() per call, 16-byte aligned: the opaque state of gmr1_hip_codec_decode_batch*,
 * so a call can move between that entry and these, and travels with the call's gmr1_hip_tch3_state: both go in and come
 * back, and a call cut into any pieces gives the samples and the states of one invocation.  A call without records
 * keeps its codec_state byte for byte.
 *
 * gmr1_hip_tch3_voice_batch* is gmr1_hip_tch3_follow_batch* and gmr1_hip_tch3_frames_to_pcm* back to back on the stream:
 * the follower's record array `out` is the decoder's input; arguments up to `out` are the follower's.
 *
 * _dev: every pointer is device memory; the call enqueues on `stream` and returns -- no copy to the host and no
 * synchronisation (but for the first use on a device, which builds the decoder's tables, and a workspace that has to
 * grow); gmr1_hip_codec_init_dev makes fresh decoders; the entries of first are clamped to 0..n_frames.  Host forms: flags
 * and codec_state == NULL as for gmr1_hip_codec_decode_batch (GMR1_HIP_CODEC_FRESH, GMR1_HIP_CODEC_CLEARED; NULL: fresh
 * decoders, nothing written back); first is checked as the follower's host form checks it.
 * n_calls == 0 or n_frames == 0 does nothing.  -EINVAL: a negative count, a NULL required array (rv is optional;
 * codec_state in the _dev forms is not), pcm not 2-byte or codec_state not 16-byte aligned, unknown flag bits, and for the
 * samples forms everything the follower refuses.  -ENODEV without a device.  Nothing is written on either: the arguments are
 * checked before the device is asked for. */
int gmr1_hip_tch3_frames_to_pcm_dev(void *stream, int n_calls, const int32_t *first /* n_calls + 1 */, int n_frames,
                                    const struct gmr1_hip_tch3_frame *frames, void *codec_state,
                                    int16_t *pcm /* n_frames x 320 */, int32_t *rv /* n_frames x 2, or NULL */);
int gmr1_hip_tch3_frames_to_pcm(int n_calls, const int32_t *first, int n_frames,
                                const struct gmr1_hip_tch3_frame *frames, void *codec_state, int flags,
                                int16_t *pcm, int32_t *rv);
int gmr1_hip_tch3_voice_batch_dev(void *stream, int n_calls, int sps, int in_len, const float *iq,
                                  const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                                  const uint32_t *fn, struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out,
                                  void *codec_state, int16_t *pcm, int32_t *rv);
int gmr1_hip_tch3_voice_batch(int n_calls, int sps, int in_len, const float *iq, uint64_t iq_len, const int32_t *first,
                              int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                              struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out,
                              void *codec_state, int flags, int16_t *pcm, int32_t *rv);

/* The frames of running calls closed up into audio blocks on the device: what gmr1_hip_rx_run_voice* reports, and what a
 * caller that follows calls with gmr1_hip_tch3_follow_batch_dev can hand to a sound device.  Call c owns
 * frames[first[c] .. first[c+1]) as in the follower, fn[k] is frame k's own fn as handed to the follower, label[c] =
 * arfcn | chain << 16 | tn << 24 | call << 32.
 *   cls != GMR1_HIP_TCH3_OFF   one block: arfcn, chain, tn and call from the call's label, cls from the frame, fn = fn[k]
 *                              (also for a FACCH3 message, whose record carries fn - 3), pad 0.  type == 0x10: pcm and rv
 *                              are what gmr1_hip_tch3_frames_to_pcm* gives for the record (rv as int16_t).  Any other
 *                              type: 320 zero samples, rv 0, 0, and the decoder is not touched.
 *   cls == GMR1_HIP_TCH3_OFF   nothing, and the decoder is not touched.
 * Blocks come in call order, then frame order.  Only the first max_out blocks are stored; *n_out is the number found.
 * The decoders step over every speech frame whether its block is stored or not: codec_state afterwards does not depend
 * on max_out, and equals gmr1_hip_tch3_frames_to_pcm_dev's on the same frames.  A call cut into any pieces gives the
 * blocks and the states of one invocation.
 * Every pointer is device memory; the call enqueues two kernels on `stream` and returns (no synchronisation but for the
 * first use on a device, which builds the decoder's tables, and a workspace that has to grow).  The entries of first are
 * clamped to 0..n_frames.  n_calls == 0 writes *n_out = 0.  -EINVAL, before the device is asked for and with nothing
 * written: everything gmr1_hip_tch3_frames_to_pcm_dev refuses (out taking the place of pcm; it may be NULL when max_out
 * == 0), a negative max_out, a NULL fn, label or n_out, an out that is not on a 16-byte boundary.  -ENODEV without a
 * device. */
struct gmr1_hip_rx_audio {          /* 656 bytes, pcm at offset 16 */
	uint16_t arfcn;
	uint8_t  chain;
	uint8_t  cls;       /* the follower's class of the frame (GMR1_HIP_TCH3_*, never OFF) */
	uint32_t fn;        /* the frame's own fn, as handed to the follower */
	uint8_t  tn;
	uint8_t  call;      /* IMMEDIATE ASSIGNMENTs this chain has followed so far, mod 256 (>= 1) */
	int16_t  rv[2];     /* the decoder's two verdicts: 0, or -EINVAL for a tone frame with an unassigned code */
	uint8_t  pad[2];    /* 0 */
	int16_t  pcm[320];  /* 40 ms of 8 kHz audio */
};
int gmr1_hip_tch3_frames_to_audio_dev(void *stream, int n_calls, const int32_t *first /* n_calls + 1 */, int n_frames,
                                      const struct gmr1_hip_tch3_frame *frames, const uint32_t *fn /* n_frames */,
                                      const uint64_t *label /* n_calls */, void *codec_state,
                                      struct gmr1_hip_rx_audio *out, int max_out, int32_t *n_out /* device */);

/* ---- following a circuit-switched data call: rx_tch9 over many calls at once (gmr1_rx.c:262-353) -------------
 * What gmr1_rx does per frame once an ASSIGNMENT COMMAND 1 has named a timeslot on the CSD carrier: demodulate the NT9
 * burst, sync sequence 0 -> FACCH9, any other -> TCH9, decipher with A5/1 of the frame number (always) and decode; a TCH9
 * block is decoded against the call's two previous TCH9 bursts (the depth-3 inter-burst de-interleaver, which only
 * advances on TCH9 bursts).  The state of a call is the caller's, as for the TCH3 follower above: it goes in and comes
 * back, and a call cut into any pieces gives byte for byte what one invocation gives.  Calls and frames are laid out as
 * there (first[0] = 0, first[n_calls] = n_frames, non-decreasing); one record per frame handed in comes back at out[k].
 *
 * The bits form IS the follower: frame k is ebits[662 k ..] (the demodulator's soft bits), sync_id[k], rv[k] (the
 * demodulator's return value; NULL: all 0) and fn[k].  The from-samples form demodulates frame k's window
 * iq[offset[k] .. offset[k] + in_len) as an NT9 burst (in_len >= 351*sps, <= GMR1_HIP_MAX_IN_LEN; gmr1_rx cuts
 * 351*sps + sps + sps/2, which fits up to sps 11) with freq_shift[k] into scratch and runs the bits form on it.  Both are
 * entries because the reference's sync search keeps its correlation sums from one sync sequence to the next
 * (pi4cxpsk.c:207-253), so an NT9 burst sent with sequence 0 is reported as 1: through the demodulator the FACCH9 route is
 * practically unreachable, and a caller with a demodulator of its own wants the bits form anyway.
 * mode: enum gmr1_tch9_mode (0 2k4, 1 4k8, 2 9k6; gmr1_rx hard-codes 9k6), one per invocation; the state does not depend
 * on it.  In both Viterbi decoder modes (gmr1_hip_set_conv_decoder) payloads and conv follow the selected mode.
 *
 * _dev: every pointer is device memory; the call enqueues on `stream` and returns -- no copy to the host and no
 * synchronisation (but for the workspace that has to grow); the entries of first are clamped to 0..n_frames.  The host
 * forms copy the arrays in, state and out back, and also check first and the windows.  n_calls == 0 or n_frames == 0 does
 * nothing; a call without frames keeps its state byte for byte.  -EINVAL, before anything is written and before the device
 * is asked for: a negative count, a NULL array (rv excepted), mode outside 0..2, sps outside 1..16, in_len out of range,
 * iq not aligned to 8 bytes.  -ENODEV without a device. */
struct gmr1_hip_tch9_state {        /* struct tch9_state of gmr1_rx.c:82-91 plus the key; all-zero = no call; 1340 bytes */
	int32_t active;             /* 0: every frame is GMR1_HIP_TCH9_OFF and nothing changes */
	int32_t n_held;             /* TCH9 bursts the de-interleaver still needs: 0, 1 or 2 (saturates at 2) */
	uint8_t kc[8];              /* the call's key (A5/1 is always applied, gmr1_rx.c:310, 326) */
	int8_t  held[2 * 662];      /* [0..661] the previous TCH9 burst, [662..1323] the one before it: soft bits in
	                               bits_e order AFTER deciphering (what tch9.c:152-160 leaves, status bits in place);
	                               slots >= n_held are 0.  A key changed between invocations does not touch them */
};

enum { GMR1_HIP_TCH9_OFF = 0, GMR1_HIP_TCH9_FACCH9, GMR1_HIP_TCH9_TCH9, GMR1_HIP_TCH9_ERR };

struct gmr1_hip_tch9_frame {        /* one per frame handed in, in the order handed in; 80 bytes */
	uint8_t  cls;               /* enum above; ERR: the demodulation refused the window (rv != 0): no burst, the
	                               de-interleaver does not advance (decision D8) */
	uint8_t  type;              /* 0 nothing to report | 0x1a FACCH9 whose CRC passed | 0x18 a TCH9 block (always) */
	uint8_t  len;               /* 0 | 38 | 18 / 30 / 60 by mode */
	uint8_t  crc;               /* FACCH9: 0 pass, 1 fail; otherwise 0 */
	uint32_t fn;                /* the frame's fn (every frame) */
	int32_t  conv;              /* the decoder's value for every FACCH9 / TCH9 frame, CRC passed or not; else 0 */
	uint8_t  l2[64];            /* beyond len: 0; a FACCH9 whose CRC failed: all 0 */
	uint8_t  pad[4];            /* 0 */
};

/* rx_tch9_init (gmr1_rx.c:263-274) on a caller-held state: active = 1, n_held = 0, held cleared; kc stays.  Host
 * arithmetic, needs no device.  -EINVAL: s is NULL. */
int gmr1_hip_tch9_state_assign(struct gmr1_hip_tch9_state *s);
/* The same on states in device memory: for j < n what gmr1_hip_tch9_state_assign(&state[call[j]]) does (call[j] < 0 is
 * skipped, a call may be named twice).  call and state are device memory; enqueues on `stream` and returns.  -EINVAL:
 * n < 0 or a NULL array; -ENODEV without a device. */
int gmr1_hip_tch9_state_assign_batch_dev(void *stream, int n, const int32_t *call, struct gmr1_hip_tch9_state *state);

int gmr1_hip_tch9_follow_bits_batch_dev(void *stream, int n_calls, int mode, const int32_t *first /* n_calls + 1 */,
                                        int n_frames, const int8_t *ebits /* n_frames x 662 */, const int32_t *sync_id,
                                        const int32_t *rv /* or NULL: all 0 */, const uint32_t *fn,
                                        struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out);
int gmr1_hip_tch9_follow_bits_batch(int n_calls, int mode, const int32_t *first, int n_frames, const int8_t *ebits,
                                    const int32_t *sync_id, const int32_t *rv, const uint32_t *fn,
                                    struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out);
int gmr1_hip_tch9_follow_batch_dev(void *stream, int n_calls, int sps, int in_len, int mode, const float *iq,
                                   const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                                   const uint32_t *fn, struct gmr1_hip_tch9_state *state,
                                   struct gmr1_hip_tch9_frame *out);
int gmr1_hip_tch9_follow_batch(int n_calls, int sps, int in_len, int mode, const float *iq, uint64_t iq_len,
                               const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                               const uint32_t *fn, struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out);

/* The whole application: gmr1_rx with all its optional arguments (tch.cfile, key, tch_csd.cfile; gmr1_rx.c:897-975).
 * csd holds, per carrier, the carrier of the TCH9 (circuit switched data) channel an ASSIGNMENT COMMAND 1
 * on the FACCH3 points to -- same layout and timing as iq / tch.  From that message on every frame's NT9 burst
 * on the assigned timeslot is demodulated, deciphered (A5/1, always) and decoded: sync sequence 0 -> FACCH9
 * (type 0x1a = GSMTAP_GMR1_TCH9 | GSMTAP_GMR1_FACCH, 38 bytes, reported when the CRC passes), sync sequence 1 ->
 * TCH9 9k6 (type 0x18, 60 bytes, always reported -- no CRC; gmr1_rx.c:262-353).  Their payloads do not fit
 * the 40-byte record, so they come back as big records, ordered like the others. */
struct gmr1_hip_rx_big_record {
	uint16_t arfcn;
	uint8_t  chain, type;
	uint32_t fn;
	uint8_t  tn, crc, len, pad;
	int32_t  conv;
	uint8_t  l2[64];
};
/* The TCH9 follower's frames as gmr1_hip_rx_run_full reports them, closed up on the device: call c owns
 * frames[first[c] .. first[c+1]) as in gmr1_hip_tch9_follow*_batch*, label[c] = arfcn | chain << 16 | tn << 24.  A frame
 * with type == 0 gives nothing, every other one a big record -- arfcn, chain and tn from its call's label; fn, type, len,
 * conv and l2[0..len) from the frame; crc, pad and the rest of l2 0 -- in call order, then frame order.  Only the first
 * max_out records are stored; *n_out is the number found.  Every pointer is device memory (out on a 16-byte boundary); the
 * call enqueues one kernel on `stream` and returns.  The entries of first are clamped to 0..n_frames.  -EINVAL, before the
 * device is asked for: a negative count, a NULL array (out may be NULL when max_out == 0), a misaligned out.  -ENODEV
 * without a device.  n_calls == 0 writes *n_out = 0. */
int gmr1_hip_tch9_frames_to_records_dev(void *stream, int n_calls, const int32_t *first /* n_calls + 1 */, int n_frames,
                                        const struct gmr1_hip_tch9_frame *frames,
                                        const uint32_t *label /* n_calls */, struct gmr1_hip_rx_big_record *out,
                                        int max_out, int32_t *n_out /* device */);

/* Measurement aid: wall time, in microseconds, of the phases of the calling thread's last gmr1_hip_rx_run* call --
 * [0] FCCH acquisition (main() -> fcch_single_init / fcch_multi_process, gmr1_rx.c:605-744) incl. the chains set up from its result,
 * [1] the frame loop (process_bcch, :852-895) from its first launch until its kernels are through, [2] the records to the
 * caller's buffer, [3] host work around the loop, [4] the traffic-channel passes. */
int gmr1_hip_rx_run_last_timing(double *us5);

int gmr1_hip_rx_run_full_dev(void *stream, int n_arfcn, int sps, const float *iq, const float *tch,
                             const float *csd, const uint64_t *offset, const uint64_t *length,
                             const uint16_t *arfcn, const uint8_t *kc,
                             struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                             struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                             int32_t *status, int32_t *n_chains);
int gmr1_hip_rx_run_full(int n_arfcn, int sps, const float *iq, const float *tch, const float *csd, uint64_t iq_len,
                         const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                         struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                         struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                         int32_t *status, int32_t *n_chains);

/* ---- AMBE speech decoder over many voice channels (reference: one `struct gmr1_codec` per channel, frames one call
 * at a time: include/osmocom/gmr1/codec/codec.h:37-45, src/codec) ----
 * frames [n_ch][n_frames][10] bytes, pcm [n_ch][n_frames][160] samples, rv (optional) [n_ch][n_frames]: 0, or -EINVAL
 * for a tone frame with an unassigned code.  One wavefront per channel walks that channel's frames in order.
 * `state`: gmr1_hip_codec_state_bytes() per channel, 16-byte aligned, opaque, carried between calls so a channel can
 * be decoded piecewise; gmr1_hip_codec_init_dev makes fresh decoders (the reference's gmr1_codec_alloc).
 * GMR1_HIP_CODEC_CLEARED: per-harmonic voicing above the harmonic count reads 0 instead of what the same subframe of
 * an earlier frame left there (DESIGN.md decision D9: the reference leaves it to its stack; the default is what its
 * own program gmr1_ambe_decode computes).
 * The host form copies frames in and samples out; state == NULL or GMR1_HIP_CODEC_FRESH: fresh decoders; otherwise
 * `state` (host memory) is read before and written after. */
#define GMR1_HIP_CODEC_CLEARED 1
#define GMR1_HIP_CODEC_FRESH   2
size_t gmr1_hip_codec_state_bytes(void);
int gmr1_hip_codec_init_dev(void *stream, int n_ch, void *state, int flags);
/* Fresh decoders for a list of channels, between two invocations, so that a decoder's state never visits the host: for
 * j < n what gmr1_hip_codec_init_dev(stream, 1, state + call[j], flags) does (call[j] < 0 is skipped, a channel may be named
 * twice); every other state keeps its bytes.  It is the codec-state counterpart of gmr1_hip_tch3_state_assign_batch_dev.
 * call and state are device memory; enqueues on `stream` and returns.  -EINVAL: n < 0, a NULL array, state not 16-byte
 * aligned, unknown flag bits; -ENODEV without a device. */
int gmr1_hip_codec_init_list_dev(void *stream, int n, const int32_t *call, void *state, int flags);
int gmr1_hip_codec_decode_batch_dev(void *stream, int n_ch, int n_frames, const uint8_t *frames, int16_t *pcm,
                                    int32_t *rv, void *state);
int gmr1_hip_codec_decode_batch(int n_ch, int n_frames, const uint8_t *frames, int16_t *pcm, int32_t *rv, void *state,
                                int flags);
/* The tables the library computes with the host's libm when it loads (cosine table, 2^f0log per pitch history, ...):
 * for tests; works without a GPU. */
int gmr1_hip_codec_host_tables(const void **image, size_t *bytes);
/* The kernel's restatement of glibc's powf and cosf, evaluated on the host (for tests; works without a GPU): which = 0:
 * out[i] = powf(2, x[i]); 1: powf(x[i], 0.25f) (NaN where the kernel would fall back to double precision); 2: cosf(x[i]). */
int gmr1_hip_codec_libm_check(int which, int n, const float *x, float *out);

/* The GSMTAP packet gmr1_gsmtap_makemsg (reference src/gsmtap.c:43-71, include/osmocom/gmr1/gsmtap.h:35-37)
 * builds for one record: 16-byte gsmtap_hdr + L2.  Returns the packet length (16 + rec->len) or
 * -EINVAL.  Host-only; works without a GPU.  with_arfcn = 0 leaves the arfcn field 0 as the reference does. */
int gmr1_hip_gsmtap_pack(const struct gmr1_hip_rx_record *rec, int with_arfcn, uint8_t *buf, int buf_len);
int gmr1_hip_gsmtap_pack_big(const struct gmr1_hip_rx_big_record *rec, int with_arfcn, uint8_t *buf, int buf_len);

#ifdef __cplusplus
}
#endif

#endif /* GMR1_HIP_H */
