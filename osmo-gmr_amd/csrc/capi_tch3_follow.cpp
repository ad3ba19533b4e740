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

size_t up128(size_t x) { return (x + 127) & ~(size_t)127; }

// where the follower's scratch of n frames lies, from a 128-byte boundary: per-frame results, job slots, keystreams, decodes
struct FollowScratch {
	size_t call, p, et, en, krv, drv, bt, dsid, dtoa, frv, fsid, ftoa, srv, feb, seb, cls, need, jeb, jfn, kss, ksf, sfr[2],
	       scv[2], fl[2], fcrc[2], fcv[2], bytes;
	explicit FollowScratch(size_t n)
	{
		size_t o = 0;
		auto take = [&](size_t b) { const size_t at = o; o += up128(b); return at; };
		call = take(n * 4); p = take(n * 4); et = take(n * 4); en = take(n * 4); krv = take(n * 4); drv = take(n * 4);
		bt = take(n * 4); dsid = take(n * 4); dtoa = take(n * 4); frv = take(n * 4); fsid = take(n * 4); ftoa = take(n * 4);
		srv = take(n * 4); feb = take(n * 104); seb = take(n * 212); cls = take(n); need = take(n); jeb = take(n * 416);
		jfn = take(n * 16); kss = take(n * 208); ksf = take(n * 384);
		for (int v = 0; v < 2; v++) sfr[v] = take(n * 20);
		for (int v = 0; v < 2; v++) scv[v] = take(n * 8);
		for (int v = 0; v < 2; v++) fl[v] = take(n * 10);
		for (int v = 0; v < 2; v++) fcrc[v] = take(n * 4);
		for (int v = 0; v < 2; v++) fcv[v] = take(n * 4);
		bytes = o;
	}
};

}  // namespace

namespace gmr1 {

size_t tch3_follow_scratch_bytes(int n_frames) { return FollowScratch((size_t)n_frames).bytes; }

// The whole chain, enqueued on `st`; every pointer is device memory.  The caller has checked the arguments and holds a
// WsLease; `scratch` is tch3_follow_scratch_bytes(n_frames) of device memory on a 128-byte boundary that is the chain's
// alone until its last kernel is through.
int tch3_follow_enqueue(hipStream_t st, void *scratch, int n_calls, int sps, int in_len, const float *iq, const int32_t *first,
                        int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                        struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out)
{
	const FollowScratch o((size_t)n_frames);
	unsigned char *d = static_cast<unsigned char *>(scratch);
	auto I32 = [&](size_t at) { return reinterpret_cast<int32_t *>(d + at); };
	auto F32 = [&](size_t at) { return reinterpret_cast<float *>(d + at); };
	auto U8 = [&](size_t at) { return reinterpret_cast<uint8_t *>(d + at); };
	auto I8 = [&](size_t at) { return reinterpret_cast<int8_t *>(d + at); };

	Tch3FollowArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n_calls = n_calls; a.n_frames = n_frames;
	a.e_toa = (in_len - 117 * sps) >> 1;           // burst_map's e_toa for a window of 117 sps + win (gmr1_rx.c:157-167)
	a.first = first; a.fn = fn; a.state = state; a.out = out;
	a.call_of = I32(o.call); a.p = I32(o.p); a.et = F32(o.et);
	a.energy = F32(o.en); a.dkab_rv = I32(o.krv); a.det_rv = I32(o.drv); a.btid = I32(o.bt);
	a.facch_rv = I32(o.frv); a.facch_sid = I32(o.fsid); a.speech_rv = I32(o.srv);
	a.facch_eb = I8(o.feb);
	a.cls = U8(o.cls); a.need = U8(o.need); a.job_eb = I8(o.jeb); a.job_fn = reinterpret_cast<uint32_t *>(d + o.jfn);
	a.ks_speech = U8(o.kss); a.ks_facch = U8(o.ksf);
	a.sp_frames[0] = U8(o.sfr[0]); a.sp_frames[1] = U8(o.sfr[1]);
	a.sp_conv[0] = I32(o.scv[0]); a.sp_conv[1] = I32(o.scv[1]);
	a.fa_l2[0] = U8(o.fl[0]); a.fa_l2[1] = U8(o.fl[1]);
	a.fa_crc[0] = I32(o.fcrc[0]); a.fa_crc[1] = I32(o.fcrc[1]);
	a.fa_conv[0] = I32(o.fcv[0]); a.fa_conv[1] = I32(o.fcv[1]);

	HIP_TRY(launch_tch3f_prep(a, st));

	// A. speculative per-frame work: the state machine picks from it
	int r = demod_dev_energy(st, GMR1_HIP_NT3_FACCH, n_frames, sps, in_len, iq, offset, freq_shift, I8(o.feb), 104, I32(o.fsid),
	                         F32(o.ftoa), F32(o.en), I32(o.frv));
	if (r) return r;
	r = demod_dev_energy(st, GMR1_HIP_NT3_SPEECH, n_frames, sps, in_len, iq, offset, freq_shift, I8(o.seb), 212, nullptr, nullptr,
	                     nullptr, I32(o.srv));
	if (r) return r;
	{
		const int ids[2] = {GMR1_HIP_NT3_FACCH, GMR1_HIP_NT3_SPEECH};     // gmr1_rx.c:534-538
		r = gmr1_hip_detect_batch_dev(st, 2, ids, n_frames, sps, in_len, iq, offset, freq_shift, a.et, I32(o.bt), I32(o.dsid),
		                              F32(o.dtoa), I32(o.drv));
		if (r) return r;
	}
	r = gmr1_hip_dkab_demod_batch_dev(st, n_frames, sps, in_len, iq, offset, freq_shift, a.p, nullptr, nullptr, I32(o.krv));
	if (r) return r;

	// B. the state machine, call by call
	HIP_TRY(launch_tch3f_walk(a, st));

	// C. keystreams and decodes, plain and deciphered, over the frames that ask for one
	HIP_TRY(launch_a5_tch3f(a, st));
	for (int v = 0; v < 2; v++) {
		Tch3Args t;
		t.n = n_frames; t.m = 0; t.conv_acc = conv_acc();
		t.ebits = I8(o.seb); t.ciph = v ? a.ks_speech : nullptr;
		t.frames = U8(o.sfr[v]); t.bits_s = nullptr; t.conv = I32(o.scv[v]);
		HIP_TRY(launch_tch3_jobs(t, a.need, st));
		Facch3Args f;
		f.n = n_frames; f.conv_acc = conv_acc();
		f.ebits = a.job_eb; f.ciph = v ? a.ks_facch : nullptr;
		f.l2 = U8(o.fl[v]); f.bits_s = nullptr; f.crc = I32(o.fcrc[v]); f.conv = I32(o.fcv[v]);
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
	WsLease lease;
	if ((r = lease.acquire(s, (hipStream_t)stream))) return r;
	Arena ws;                                      // the start of the device's workspace
	if ((r = ws.init(tch3_follow_scratch_bytes(n_frames)))) return r;
	return tch3_follow_enqueue((hipStream_t)stream, ws.base, n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state,
	                           out);
}

int gmr1_hip_tch3_follow_batch(int n_calls, int sps, int in_len, const float *iq, uint64_t iq_len,
                               const int32_t *first, int n_frames,
                               const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                               struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out)
{
	int r = follow_check(n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	if (first[0] != 0 || first[n_calls] != n_frames)
		return fail(-EINVAL, "tch3_follow: first[] must run from 0 to n_frames");
	for (int c = 0; c < n_calls; c++)
		if (first[c + 1] < first[c])
			return fail(-EINVAL, "tch3_follow: first[%d] decreases", c + 1);
	if ((r = bursts_fit(n_frames, offset, in_len, iq_len))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const int32_t *d_first = sg.in(first, (size_t)n_calls + 1);
	const uint64_t *d_off = sg.in(offset, (size_t)n_frames);
	const float *d_fs = sg.in(freq_shift, (size_t)n_frames);
	const uint32_t *d_fn = sg.in(fn, (size_t)n_frames);
	struct gmr1_hip_tch3_state *d_state = sg.inout(state, (size_t)n_calls);
	struct gmr1_hip_tch3_frame *d_out = sg.out(out, (size_t)n_frames);
	if ((r = sg.err())) return r;
	{
		WsLease lease;
		if ((r = lease.acquire(s, nullptr))) return r;
		Arena ws;
		if ((r = ws.init(tch3_follow_scratch_bytes(n_frames)))) return r;
		if ((r = tch3_follow_enqueue(nullptr, ws.base, n_calls, sps, in_len, d_iq, d_first, n_frames, d_off, d_fs, d_fn, d_state,
		                             d_out)))
			return r;
	}
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
	{
		WsLease lease;
		if ((r = lease.acquire(s, st))) return r;
		Arena ws;
		if ((r = ws.init(tch3_follow_scratch_bytes(n_frames)))) return r;
		if ((r = tch3_follow_enqueue(st, ws.base, n_calls, sps, in_len, iq, first, n_frames, offset, freq_shift, fn, state, out)))
			return r;
	}
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
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const int32_t *d_first = sg.in(first, (size_t)n_calls + 1);
	const uint64_t *d_off = sg.in(offset, (size_t)n_frames);
	const float *d_fs = sg.in(freq_shift, (size_t)n_frames);
	const uint32_t *d_fn = sg.in(fn, (size_t)n_frames);
	struct gmr1_hip_tch3_state *d_state = sg.inout(state, (size_t)n_calls);
	struct gmr1_hip_tch3_frame *d_out = sg.out(out, (size_t)n_frames);
	unsigned char *h_cs = static_cast<unsigned char *>(codec_state);
	unsigned char *d_cs = carry ? sg.inout(h_cs, cs_bytes) : sg.out_always(h_cs, cs_bytes);
	int16_t *d_pcm = sg.out(pcm, (size_t)n_frames * 320);
	int32_t *d_rv = sg.out(rv, (size_t)n_frames * 2);
	if ((r = sg.err())) return r;
	if (!carry && (r = tch3_pcm_fresh(nullptr, n_calls, d_cs, flags))) return r;
	{
		WsLease lease;
		if ((r = lease.acquire(s, nullptr))) return r;
		Arena ws;
		if ((r = ws.init(tch3_follow_scratch_bytes(n_frames)))) return r;
		if ((r = tch3_follow_enqueue(nullptr, ws.base, n_calls, sps, in_len, d_iq, d_first, n_frames, d_off, d_fs, d_fn, d_state,
		                             d_out)))
			return r;
	}
	if ((r = tch3_pcm_enqueue(nullptr, n_calls, d_first, n_frames, d_out, d_cs, d_pcm, d_rv))) return r;
	return sg.fetch();
}

}  // extern "C"
