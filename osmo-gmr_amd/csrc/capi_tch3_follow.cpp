// capi_tch3_follow.cpp -- C ABI of the batched TCH3 call follower (reference src/gmr1_rx.c:355-600: rx_tch3_init, rx_tch3
// and its helpers).  The state of a call is the caller's; every decision between the frames is taken on the device
// (tch3_follow_kernels.hip, tch3_follow.h).  gmr1_hip_tch3_voice_batch* puts the speech decoder behind it (capi_ambe.cpp:
// tch3_pcm_*).
#include "capi_common.h"
#include "tch3_follow.h"

#include <cstddef>

#include "../../include/gmr1_hip.h"

using namespace gmr1;

namespace {

int follow_check(int n_calls, int sps, int in_len, const float *iq, const int32_t *first, int n_frames,
                 const uint64_t *offset, const float *freq_shift, const uint32_t *fn, const void *state, const void *out)
{
	if (n_calls < 0 || n_frames < 0)
		return fail(-EINVAL, "tch3_follow: negative count");
	if (!iq || !first || !offset || !freq_shift || !fn || !state || !out)
		return fail(-EINVAL, "tch3_follow: NULL argument");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "tch3_follow: sps=%d out of range (1..16)", sps);
	if (in_len < 117 * sps || in_len > kMaxInLen)
		return fail(-EINVAL, "tch3_follow: window of %d samples (%d..%d at sps=%d)", in_len, 117 * sps, kMaxInLen, sps);
	if ((uintptr_t)iq & 7)
		return fail(-EINVAL, "tch3_follow: iq is not aligned to a complex sample");
	return 0;
}

}  // namespace

namespace gmr1 {

// The whole chain, enqueued on `st`; every pointer is device memory.  The caller has checked the arguments and holds a
// WsLease; `scratch` is tch3_follow_scratch_bytes(n_frames) of device memory on a 128-byte boundary that is the chain's
// alone until its last kernel is through.
int tch3_follow_enqueue(hipStream_t st, void *scratch, int n_calls, int sps, int in_len, const float *iq, const int32_t *first,
                        int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                        struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out)
{
	const FollowScratch o(scratch, (size_t)n_frames);

	Tch3FollowArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n_calls = n_calls; a.n_frames = n_frames;
	a.e_toa = (in_len - 117 * sps) >> 1;           // burst_map's e_toa for a window of 117 sps + win (gmr1_rx.c:157-167)
	a.first = first; a.fn = fn; a.state = state; a.out = out;
	a.call_of = o.call; a.p = o.p; a.et = o.et;
	a.energy = o.en; a.dkab_rv = o.krv; a.det_rv = o.drv; a.btid = o.bt;
	a.facch_rv = o.frv; a.facch_sid = o.fsid; a.speech_rv = o.srv;
	a.facch_eb = o.feb;
	a.cls = o.cls; a.need = o.need; a.job_eb = o.jeb; a.job_fn = o.jfn;
	a.ks_speech = o.kss; a.ks_facch = o.ksf;
	for (int v = 0; v < 2; v++) {
		a.sp_frames[v] = o.sfr[v]; a.sp_conv[v] = o.scv[v];
		a.fa_l2[v] = o.fl[v]; a.fa_crc[v] = o.fcrc[v]; a.fa_conv[v] = o.fcv[v];
	}

	HIP_TRY(launch_tch3f_prep(a, st));

	// A. speculative per-frame work: the state machine picks from it
	int r = demod_dev_energy(st, GMR1_HIP_NT3_FACCH, n_frames, sps, in_len, iq, offset, freq_shift, o.feb, 104, o.fsid, o.ftoa, o.en,
	                         o.frv);
	if (r) return r;
	r = demod_dev_energy(st, GMR1_HIP_NT3_SPEECH, n_frames, sps, in_len, iq, offset, freq_shift, o.seb, 212, nullptr, nullptr, nullptr,
	                     o.srv);
	if (r) return r;
	{
		const int ids[2] = {GMR1_HIP_NT3_FACCH, GMR1_HIP_NT3_SPEECH};     // gmr1_rx.c:534-538
		r = gmr1_hip_detect_batch_dev(st, 2, ids, n_frames, sps, in_len, iq, offset, freq_shift, a.et, o.bt, o.dsid, o.dtoa, o.drv);
		if (r) return r;
	}
	r = gmr1_hip_dkab_demod_batch_dev(st, n_frames, sps, in_len, iq, offset, freq_shift, a.p, nullptr, nullptr, o.krv);
	if (r) return r;

	// B. the state machine, call by call
	HIP_TRY(launch_tch3f_walk(a, st));

	// C. keystreams and decodes, plain and deciphered, over the frames that ask for one
	HIP_TRY(launch_a5_tch3f(a, st));
	for (int v = 0; v < 2; v++) {
		Tch3Args t;
		t.n = n_frames; t.m = 0; t.conv_acc = conv_acc();
		t.ebits = o.seb; t.ciph = v ? a.ks_speech : nullptr;
		t.frames = o.sfr[v]; t.bits_s = nullptr; t.conv = o.scv[v];
		HIP_TRY(launch_tch3_jobs(t, a.need, st));
		Facch3Args f;
		f.n = n_frames; f.conv_acc = conv_acc();
		f.ebits = a.job_eb; f.ciph = v ? a.ks_facch : nullptr;
		f.l2 = o.fl[v]; f.bits_s = nullptr; f.crc = o.fcrc[v]; f.conv = o.fcv[v];
		HIP_TRY(launch_facch3_jobs(f, a.need, st));
	}

	// D. ciphering state and records, in frame order
	HIP_TRY(launch_tch3f_emit(a, st));
	return 0;
}

}  // namespace gmr1

extern "C" {

int gmr1_hip_tch3_state_assign(struct gmr1_hip_tch3_state *s, int p, float ref_energy)
{
	if (!s)
		return fail(-EINVAL, "tch3_state_assign: NULL state");
	// rx_tch3_init, gmr1_rx.c:358-376: ciph, burst_cnt and bi_fn keep what they hold (tch3_follow_assign, which
	// k_tch3f_assign runs on device-resident states)
	static_assert(offsetof(gmr1_hip_tch3_state, ebits) == sizeof(Tch3Walk), "Tch3Walk is the state up to its soft bits");
	Tch3Walk w;
	std::memcpy(&w, s, sizeof(w));
	tch3_follow_assign(w, p, ref_energy);
	std::memcpy(s, &w, sizeof(w));
	std::memset(s->ebits, 0, sizeof(s->ebits));
	return 0;
}

int gmr1_hip_tch3_state_assign_batch_dev(void *stream, int n, const int32_t *call, const int32_t *p, const float *ref_energy,
                                         struct gmr1_hip_tch3_state *state)
{
	if (n < 0)
		return fail(-EINVAL, "tch3_state_assign_batch: negative count");
	if (!call || !p || !ref_energy || !state)
		return fail(-EINVAL, "tch3_state_assign_batch: NULL argument");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	HIP_TRY(launch_tch3f_assign(n, call, p, ref_energy, state, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_tch3_follow_batch_dev(void *stream, int n_calls, int sps, int in_len, const float *iq,
                                   const int32_t *first, int n_frames,
                                   const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                                   struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out)
{
	int r = follow_check(n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	return with_scratch(s, st, tch3_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch3_follow_enqueue(st, ws, n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	});
}

int gmr1_hip_tch3_follow_batch(int n_calls, int sps, int in_len, const float *iq, uint64_t iq_len,
                               const int32_t *first, int n_frames,
                               const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                               struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out)
{
	int r = follow_check(n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	if ((r = tch3_pcm_first_check("tch3_follow", n_calls, first, n_frames))) return r;
	if ((r = bursts_fit(n_frames, offset, in_len, iq_len))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	Stage sg;
	const auto d = stage_follow(sg, n_calls, iq, iq_len, first, n_frames, offset, freq_shift, fn, state, out);
	if ((r = sg.err())) return r;
	r = with_scratch(s, nullptr, tch3_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch3_follow_enqueue(nullptr, ws, n_calls, sps, in_len, d.iq, d.first, n_frames, d.off, d.fs, d.fn, d.state, d.out);
	});
	if (r) return r;
	return sg.fetch();
}

// ---- samples to records and audio: the follower, then the speech decoder over its records (ambe_kernels.hip: k_ambe_calls),
// back to back on the stream.  No kernel of their own: `out` is the decoder's input. ----

int gmr1_hip_tch3_voice_batch_dev(void *stream, int n_calls, int sps, int in_len, const float *iq,
                                  const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                                  const uint32_t *fn, struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out,
                                  void *codec_state, int16_t *pcm, int32_t *rv)
{
	int r = follow_check(n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	if ((r = tch3_pcm_check("tch3_voice", n_calls, first, n_frames, out, codec_state, true, 0, 0, pcm))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	if ((r = tch3_pcm_prepare())) return r;            // nothing is enqueued unless both halves can be
	hipStream_t st = (hipStream_t)stream;
	r = with_scratch(s, st, tch3_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch3_follow_enqueue(st, ws, n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	});
	if (r) return r;
	return tch3_pcm_enqueue(st, n_calls, first, n_frames, out, codec_state, pcm, rv);
}

int gmr1_hip_tch3_voice_batch(int n_calls, int sps, int in_len, const float *iq, uint64_t iq_len, const int32_t *first,
                              int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                              struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out,
                              void *codec_state, int flags, int16_t *pcm, int32_t *rv)
{
	int r = follow_check(n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	if ((r = tch3_pcm_check("tch3_voice", n_calls, first, n_frames, out, codec_state, false, flags,
	                        GMR1_HIP_CODEC_CLEARED | GMR1_HIP_CODEC_FRESH, pcm)))
		return r;
	if ((r = tch3_pcm_first_check("tch3_voice", n_calls, first, n_frames))) return r;
	if ((r = bursts_fit(n_frames, offset, in_len, iq_len))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	if ((r = tch3_pcm_prepare())) return r;
	Stage sg;
	const bool carry = codec_state && !(flags & GMR1_HIP_CODEC_FRESH);
	const size_t cs_bytes = (size_t)n_calls * gmr1_hip_codec_state_bytes();
	const auto d = stage_follow(sg, n_calls, iq, iq_len, first, n_frames, offset, freq_shift, fn, state, out);
	unsigned char *h_cs = static_cast<unsigned char *>(codec_state);
	unsigned char *d_cs = carry ? sg.inout(h_cs, cs_bytes) : sg.out_always(h_cs, cs_bytes);
	int16_t *d_pcm = sg.out(pcm, (size_t)n_frames * 320);
	int32_t *d_rv = sg.out(rv, (size_t)n_frames * 2);
	if ((r = sg.err())) return r;
	if (!carry && (r = tch3_pcm_fresh(nullptr, n_calls, d_cs, flags))) return r;
	r = with_scratch(s, nullptr, tch3_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch3_follow_enqueue(nullptr, ws, n_calls, sps, in_len, d.iq, d.first, n_frames, d.off, d.fs, d.fn, d.state, d.out);
	});
	if (r) return r;
	if ((r = tch3_pcm_enqueue(nullptr, n_calls, d.first, n_frames, d.out, d_cs, d_pcm, d_rv))) return r;
	return sg.fetch();
}

}  // extern "C"
