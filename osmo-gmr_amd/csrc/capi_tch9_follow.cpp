// capi_tch9_follow.cpp -- C ABI of the batched TCH9 call follower (reference src/gmr1_rx.c:262-353: rx_tch9_init, rx_tch9).
// The state of a call is the caller's; every decision between the frames is taken on the device (tch9_follow_kernels.hip,
// tch9_follow.h).  The bits form is the follower; the from-samples form is the NT9 demodulator into scratch in front of it.
// tch9_follow_enqueue is the from-samples form for the library's own callers (the streaming receive loop), and
// gmr1_hip_tch9_frames_to_records_dev closes a follower's frames up into the receive loop's big records (k_tch9f_big).
#include "capi_common.h"
#include "tch9_follow.h"

#include <cstddef>

#include "../../include/gmr1_hip.h"

using namespace gmr1;

namespace {

int bits_check(int n_calls, int mode, const int32_t *first, int n_frames, const void *ebits, const void *sync_id, const uint32_t *fn,
               const void *state, const void *out)
{
	if (n_calls < 0 || n_frames < 0)
		return fail(-EINVAL, "tch9_follow: negative count");
	if (!first || !ebits || !sync_id || !fn || !state || !out)
		return fail(-EINVAL, "tch9_follow: NULL argument");
	if (mode < 0 || mode > 2)
		return fail(-EINVAL, "tch9_follow: mode %d unknown (0 2k4, 1 4k8, 2 9k6)", mode);
	return 0;
}

int samples_check(int n_calls, int sps, int in_len, int mode, const float *iq, const int32_t *first, int n_frames,
                  const uint64_t *offset, const float *freq_shift, const uint32_t *fn, const void *state, const void *out)
{
	// (the demodulator's outputs stand in for the bits form's arrays: they are scratch)
	int r = bits_check(n_calls, mode, first, n_frames, iq, offset, fn, state, out);
	if (r) return r;
	if (!freq_shift)
		return fail(-EINVAL, "tch9_follow: NULL argument");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "tch9_follow: sps=%d out of range (1..16)", sps);
	if (in_len < 351 * sps || in_len > kMaxInLen)
		return fail(-EINVAL, "tch9_follow: window of %d samples (%d..%d at sps=%d)", in_len, 351 * sps, kMaxInLen, sps);
	if ((uintptr_t)iq & 7)
		return fail(-EINVAL, "tch9_follow: iq is not aligned to a complex sample");
	return 0;
}

// The follower, enqueued on `st`; every pointer is device memory.  The caller has checked the arguments and holds a WsLease;
// `o` names tch9_follow_scratch_bytes(n_frames) of device memory on a 128-byte boundary.
int bits_enqueue(hipStream_t st, const Follow9Scratch &o, int n_calls, int mode, const int32_t *first, int n_frames,
                 const int8_t *ebits, const int32_t *sync_id, const int32_t *rv, const uint32_t *fn,
                 struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	Nt9Args f, t;
	std::memset(&f, 0, sizeof(f));
	std::memset(&t, 0, sizeof(t));
	int r = nt9_kind_args(3, &f);
	if (r) return r;
	if ((r = nt9_kind_args(mode, &t))) return r;

	Tch9FollowArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n_calls = n_calls; a.n_frames = n_frames; a.l2_bytes = t.l2_bytes;
	a.first = first; a.ebits = ebits; a.sync_id = sync_id; a.rv = rv; a.fn = fn; a.state = state; a.out = out;
	a.cls = o.cls; a.need = o.need; a.src = o.src; a.call_of = o.call;
	a.ks = o.ks; a.fa_l2 = o.fl2; a.t_l2 = o.tl2;
	a.fa_crc = o.fcrc; a.fa_conv = o.fcv; a.t_conv = o.tcv;

	// A. classes and sources, call by call (a frame no call owns -- first[] is the caller's device memory -- asks for nothing)
	HIP_TRY(hipMemsetAsync(a.need, 0, (size_t)n_frames, st));
	HIP_TRY(launch_tch9f_plan(a, st));

	// B. keystreams and the two decodes over the frame slots
	HIP_TRY(launch_a5_tch9f(a, st));
	f.n = t.n = n_frames;
	f.ebits = t.ebits = ebits; f.ciph = t.ciph = a.ks;
	f.need = t.need = a.need; f.src = t.src = a.src; f.src_call = t.src_call = a.call_of;
	f.held = t.held = reinterpret_cast<const int8_t *>(state) + offsetof(gmr1_hip_tch9_state, held);
	f.held_stride = t.held_stride = sizeof(gmr1_hip_tch9_state);
	f.want = kT9NeedFacch; f.l2 = o.fl2; f.crc = o.fcrc; f.conv = o.fcv;
	t.want = kT9NeedTch; t.l2 = o.tl2; t.conv = o.tcv;
	HIP_TRY(launch_nt9_jobs(f, st));
	HIP_TRY(launch_nt9_jobs(t, st));

	// C. records in frame order, and the calls' last two TCH9 bursts into their states
	HIP_TRY(launch_tch9f_emit(a, st));
	return 0;
}

}  // namespace

namespace gmr1 {

// the NT9 demodulator into the scratch's own slots, then the follower on them
int tch9_follow_enqueue(hipStream_t st, void *scratch, int n_calls, int sps, int in_len, int mode, const float *iq, const int32_t *first,
                        int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                        struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	const Follow9Scratch o(scratch, (size_t)n_frames);
	int r = demod_dev_energy(st, GMR1_HIP_NT9, n_frames, sps, in_len, iq, offset, freq_shift, o.eb, 662, o.sid, nullptr, nullptr, o.rv);
	if (r) return r;
	return bits_enqueue(st, o, n_calls, mode, first, n_frames, o.eb, o.sid, o.rv, fn, state, out);
}

}  // namespace gmr1

extern "C" {

int gmr1_hip_tch9_state_assign(struct gmr1_hip_tch9_state *s)
{
	if (!s)
		return fail(-EINVAL, "tch9_state_assign: NULL state");
	// rx_tch9_init, gmr1_rx.c:263-274: a fresh interleaver (k_tch9f_assign does the same on device-resident states)
	s->active = 1;
	s->n_held = 0;
	std::memset(s->held, 0, sizeof(s->held));
	return 0;
}

int gmr1_hip_tch9_state_assign_batch_dev(void *stream, int n, const int32_t *call, struct gmr1_hip_tch9_state *state)
{
	if (n < 0)
		return fail(-EINVAL, "tch9_state_assign_batch: negative count");
	if (!call || !state)
		return fail(-EINVAL, "tch9_state_assign_batch: NULL argument");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	HIP_TRY(launch_tch9f_assign(n, call, state, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_tch9_follow_bits_batch_dev(void *stream, int n_calls, int mode, const int32_t *first, int n_frames,
                                        const int8_t *ebits, const int32_t *sync_id, const int32_t *rv, const uint32_t *fn,
                                        struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	int r = bits_check(n_calls, mode, first, n_frames, ebits, sync_id, fn, state, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	return with_scratch(s, st, tch9_follow_scratch_bytes(n_frames), [&](void *ws) {
		return bits_enqueue(st, Follow9Scratch(ws, (size_t)n_frames), n_calls, mode, first, n_frames, ebits, sync_id, rv, fn, state, out);
	});
}

int gmr1_hip_tch9_follow_bits_batch(int n_calls, int mode, const int32_t *first, int n_frames, const int8_t *ebits,
                                    const int32_t *sync_id, const int32_t *rv, const uint32_t *fn,
                                    struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	int r = bits_check(n_calls, mode, first, n_frames, ebits, sync_id, fn, state, out);
	if (r) return r;
	if ((r = tch3_pcm_first_check("tch9_follow", n_calls, first, n_frames))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	Stage sg;
	const auto d = stage_follow(sg, n_calls, nullptr, 0, first, n_frames, nullptr, nullptr, fn, state, out);
	const int8_t *d_eb = sg.in(ebits, (size_t)n_frames * 662);
	const int32_t *d_sid = sg.in(sync_id, (size_t)n_frames);
	const int32_t *d_rv = sg.in(rv, (size_t)n_frames);
	if ((r = sg.err())) return r;
	r = with_scratch(s, nullptr, tch9_follow_scratch_bytes(n_frames), [&](void *ws) {
		return bits_enqueue(nullptr, Follow9Scratch(ws, (size_t)n_frames), n_calls, mode, d.first, n_frames, d_eb, d_sid, d_rv, d.fn,
		                    d.state, d.out);
	});
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_tch9_follow_batch_dev(void *stream, int n_calls, int sps, int in_len, int mode, const float *iq,
                                   const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                                   const uint32_t *fn, struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	int r = samples_check(n_calls, sps, in_len, mode, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	hipStream_t st = (hipStream_t)stream;
	return with_scratch(s, st, tch9_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch9_follow_enqueue(st, ws, n_calls, sps, in_len, mode, iq, first, n_frames, offset, freq_shift, fn, state, out);
	});
}

int gmr1_hip_tch9_follow_batch(int n_calls, int sps, int in_len, int mode, const float *iq, uint64_t iq_len,
                               const int32_t *first, int n_frames, const uint64_t *offset, const float *freq_shift,
                               const uint32_t *fn, struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out)
{
	int r = samples_check(n_calls, sps, in_len, mode, iq, first, n_frames, offset, freq_shift, fn, state, out);
	if (r) return r;
	if ((r = tch3_pcm_first_check("tch9_follow", n_calls, first, n_frames))) return r;
	if ((r = bursts_fit(n_frames, offset, in_len, iq_len))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_calls == 0 || n_frames == 0) return 0;
	Stage sg;
	const auto d = stage_follow(sg, n_calls, iq, iq_len, first, n_frames, offset, freq_shift, fn, state, out);
	if ((r = sg.err())) return r;
	r = with_scratch(s, nullptr, tch9_follow_scratch_bytes(n_frames), [&](void *ws) {
		return tch9_follow_enqueue(nullptr, ws, n_calls, sps, in_len, mode, d.iq, d.first, n_frames, d.off, d.fs, d.fn, d.state, d.out);
	});
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_tch9_frames_to_records_dev(void *stream, int n_calls, const int32_t *first, int n_frames,
                                        const struct gmr1_hip_tch9_frame *frames, const uint32_t *label,
                                        struct gmr1_hip_rx_big_record *out, int max_out, int32_t *n_out)
{
	if (n_calls < 0 || n_frames < 0 || max_out < 0)
		return fail(-EINVAL, "tch9_frames_to_records: negative count");
	if (!first || !frames || !label || !n_out || (max_out > 0 && !out))
		return fail(-EINVAL, "tch9_frames_to_records: NULL argument");
	if (((uintptr_t)out & 15) || ((uintptr_t)frames & 3))
		return fail(-EINVAL, "tch9_frames_to_records: out is not on a 16-byte boundary, or frames not on a 4-byte one");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n_calls == 0) {
		HIP_TRY(hipMemsetAsync(n_out, 0, 4, (hipStream_t)stream));
		return 0;
	}
	Tch9BigArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n_calls = n_calls; a.n_frames = n_frames; a.max_out = max_out;
	a.first = first; a.frames = frames; a.label = label; a.out = out; a.n_out = n_out;
	HIP_TRY(launch_tch9f_big(a, (hipStream_t)stream));
	return 0;
}

}  // extern "C"
