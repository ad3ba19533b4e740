// tch3_follow_kernels.hip -- the device side of gmr1_hip_tch3_follow_batch* that is not a demodulator or a decoder (gfx950).
//
// The entry (capi_tch3_follow.cpp) runs, on one stream and without the host in between:
//   k_tch3f_prep   one thread per frame: which call it belongs to, that call's DKAB position, the detector's e_toa
//   step A         the existing kernels over every frame, speculatively: FACCH3 demodulation with burst energy, speech
//                  demodulation, burst type detection, DKAB search
//   k_tch3f_walk   one wavefront per call: rx_tch3's state machine (tch3_follow.h) over the call's frames in order
//   k_a5_tch3f     (tch_kernels.hip) keystreams of the frames that ask for a decode
//   k_tch3_jobs, k_facch3_jobs   (l1_kernels.hip) the decodes, plain and deciphered
//   k_tch3f_emit   one lane per call: the ciphering state picks the variant, the caller's records are written
// and, between two invocations, k_tch3f_assign (gmr1_hip_tch3_state_assign_batch_dev): rx_tch3_init on the states where they lie.
//
// k_tch3f_walk is a latency chain.  The per-frame results of 64 frames are fetched by the 64 lanes at once and handed to
// the step one frame at a time by readlane, so the chain never waits for a load that depends on the step before; the
// state's scalars are wave-uniform (every lane computes the same step), the four-burst store of 416 soft bits lives in LDS
// (104 words per wave) and is moved by all lanes.  The only per-frame global reads left are the 104 soft bits of a frame
// that turns out to be a FACCH3 burst, and they do not depend on the state.
#include <cstddef>

#include "gmr1_dev.h"
#include "tch3_audio.h"
#include "tch3_follow.h"
#include "wave_ops.h"

namespace gmr1 {

static_assert(sizeof(gmr1_hip_tch3_state) == 472 && sizeof(gmr1_hip_tch3_frame) == 40, "public layout");
static_assert(offsetof(gmr1_hip_tch3_state, ebits) == sizeof(Tch3Walk) && offsetof(gmr1_hip_tch3_state, ebits) % 4 == 0,
              "Tch3Walk is the state up to its soft bits");
static_assert(kT3Off == GMR1_HIP_TCH3_OFF && kT3Dkab == GMR1_HIP_TCH3_DKAB && kT3DkabMissing == GMR1_HIP_TCH3_DKAB_MISSING &&
              kT3Facch == GMR1_HIP_TCH3_FACCH && kT3Speech == GMR1_HIP_TCH3_SPEECH && kT3Err == GMR1_HIP_TCH3_ERR, "classes");

constexpr int kWalkWaves = 4;              // calls per work-group of k_tch3f_walk

// first[] of the _dev entry is the caller's device memory: whatever it holds, no frame index leaves 0..n_frames
__device__ __forceinline__ int clamp_frame(int v, int lo, int n_frames)
{
	return v < lo ? lo : v > n_frames ? n_frames : v;
}

__global__ __launch_bounds__(256) void k_tch3f_prep(Tch3FollowArgs a)
{
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= a.n_frames)
		return;
	// the last call whose first frame is not behind k (calls without frames share their first[] with the next one)
	int lo = 0, hi = a.n_calls;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (a.first[mid] <= k)
			lo = mid;
		else
			hi = mid;
	}
	a.call_of[k] = lo;
	a.p[k] = a.state[lo].active ? a.state[lo].p : 0;
	a.et[k] = (float)a.e_toa;
}

__global__ __launch_bounds__(64 * kWalkWaves) void k_tch3f_walk(Tch3FollowArgs a)
{
	__shared__ __align__(16) uint32_t s_bursts[kWalkWaves][104];
	const int lane = threadIdx.x & 63;
	const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int c = blockIdx.x * kWalkWaves + wv;
	if (c >= a.n_calls)
		return;
	const int k0 = clamp_frame(a.first[c], 0, a.n_frames), k1 = clamp_frame(a.first[c + 1], k0, a.n_frames);
	if (k1 <= k0)
		return;                                    // a call without frames keeps its state untouched
	gmr1_hip_tch3_state *st = a.state + c;
	uint32_t *store = s_bursts[wv];
	uint32_t *st_eb = reinterpret_cast<uint32_t *>(st->ebits);
	for (int i = lane; i < 104; i += 64)
		store[i] = st_eb[i];
	Tch3Walk s;
	s.active = st->active; s.p = st->p; s.ciph = st->ciph; s.weak_cnt = st->weak_cnt;
	s.sync_id = st->sync_id; s.burst_cnt = st->burst_cnt;
	s.energy_dkab = st->energy_dkab; s.energy_burst = st->energy_burst;
#pragma unroll
	for (int i = 0; i < 4; i++)
		s.bi_fn[i] = st->bi_fn[i];
	WSYNC();

	// the stored bursts and their frame numbers go to frame k's job slot; the store starts over
	auto flush_to = [&](int k, const Tch3Act &act) {
		uint32_t *job = reinterpret_cast<uint32_t *>(a.job_eb + (size_t)k * 416);
		for (int i = lane; i < 104; i += 64) {
			job[i] = store[i];
			store[i] = 0;
		}
		if (lane < 4)
			a.job_fn[(size_t)k * 4 + lane] = lane == 0 ? act.job_fn[0] : lane == 1 ? act.job_fn[1] : lane == 2 ? act.job_fn[2] : act.job_fn[3];
		WSYNC();
	};

	for (int kb = k0; kb < k1; kb += 64) {
		const int cnt = k1 - kb < 64 ? k1 - kb : 64;
		// lane j holds frame kb + j
		float m_en = 0.f;
		int m_krv = 0, m_drv = 0, m_bt = 0, m_frv = 0, m_fsid = 0, m_srv = 0, m_fn = 0;
		if (lane < cnt) {
			const int k = kb + lane;
			m_en = a.energy[k]; m_krv = a.dkab_rv[k]; m_drv = a.det_rv[k]; m_bt = a.btid[k];
			m_frv = a.facch_rv[k]; m_fsid = a.facch_sid[k]; m_srv = a.speech_rv[k]; m_fn = (int)a.fn[k];
		}
		for (int j = 0; j < cnt; j++) {
			const int k = kb + j;
			Tch3FrameIn f;
			f.energy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m_en), j));
			f.dkab_rv = __builtin_amdgcn_readlane(m_krv, j);
			f.det_rv = __builtin_amdgcn_readlane(m_drv, j);
			f.btid = __builtin_amdgcn_readlane(m_bt, j);
			f.facch_rv = __builtin_amdgcn_readlane(m_frv, j);
			f.facch_sid = __builtin_amdgcn_readlane(m_fsid, j);
			f.speech_rv = __builtin_amdgcn_readlane(m_srv, j);
			f.fn = (uint32_t)__builtin_amdgcn_readlane(m_fn, j);
			const Tch3Act act = tch3_follow_step(s, f);
			if (act.flush == 1)
				flush_to(k, act);
			if (act.store) {
				if (lane < 26)
					store[26 * act.bi + lane] = reinterpret_cast<const uint32_t *>(a.facch_eb + (size_t)k * 104)[lane];
				WSYNC();
			}
			if (act.flush == 2)
				flush_to(k, act);
			if (lane == 0) {
				a.cls[k] = (uint8_t)act.cls;
				a.need[k] = (uint8_t)act.need;
			}
		}
	}

	// the state goes back, but for ciph: that is k_tch3f_emit's, which knows how the flushes decoded
	for (int i = lane; i < 104; i += 64)
		st_eb[i] = store[i];
	if (lane == 0) {
		st->active = s.active; st->p = s.p; st->weak_cnt = s.weak_cnt;
		st->sync_id = s.sync_id; st->burst_cnt = s.burst_cnt;
		st->energy_dkab = s.energy_dkab; st->energy_burst = s.energy_burst;
#pragma unroll
		for (int i = 0; i < 4; i++)
			st->bi_fn[i] = s.bi_fn[i];
	}
}

__global__ __launch_bounds__(64) void k_tch3f_emit(Tch3FollowArgs a)
{
	const int c = blockIdx.x * 64 + threadIdx.x;
	if (c >= a.n_calls)
		return;
	const int k0 = clamp_frame(a.first[c], 0, a.n_frames), k1 = clamp_frame(a.first[c + 1], k0, a.n_frames);
	if (k1 <= k0)
		return;
	int ciph = a.state[c].ciph ? 1 : 0;
	for (int k = k0; k < k1; k++) {
		gmr1_hip_tch3_frame r;
		r.cls = a.cls[k];
		r.type = 0; r.len = 0; r.ciph = 0;
		r.fn = 0; r.conv = 0;
		r.energy = a.energy[k];
#pragma unroll
		for (int i = 0; i < 20; i++)
			r.l2[i] = 0;
#pragma unroll
		for (int i = 0; i < 4; i++)
			r.pad[i] = 0;
		const int need = a.need[k];
		if (need == kT3NeedSpeech) {
			// _rx_tch3_speech, gmr1_rx.c:517-520: the keystream of the frame where ciphering is on, zeros where it is not
			const int v = ciph;
			const uint8_t *fr = (v ? a.sp_frames[1] : a.sp_frames[0]) + (size_t)k * 20;
			const int32_t *cv = (v ? a.sp_conv[1] : a.sp_conv[0]) + (size_t)k * 2;
			r.type = 0x10; r.len = 20; r.ciph = (uint8_t)v;
			r.fn = a.fn[k];
			r.conv = (cv[0] & 0xffff) | (cv[1] << 16);
#pragma unroll
			for (int i = 0; i < 20; i++)
				r.l2[i] = fr[i];
		} else if (need == kT3NeedFlush) {
			int v = ciph;
			int crc = ciph ? a.fa_crc[1][k] : a.fa_crc[0][k];
			if (!ciph && crc) {                    // retry with ciphering (gmr1_rx.c:416-428)
				v = 1;
				crc = a.fa_crc[1][k];
				if (!crc)
					ciph = 1;
			}
			if (!crc) {
				const uint8_t *m = (v ? a.fa_l2[1] : a.fa_l2[0]) + (size_t)k * 10;
				r.type = 0x12; r.len = 10; r.ciph = (uint8_t)v;
				r.fn = a.fn[k] - 3u;
				r.conv = v ? a.fa_conv[1][k] : a.fa_conv[0][k];
#pragma unroll
				for (int i = 0; i < 10; i++)
					r.l2[i] = m[i];
			}
		}
		a.out[k] = r;
	}
	a.state[c].ciph = ciph;
}

// rx_tch3_init on device-resident states: entry j assigns state[call[j]].  One wavefront per entry; the wave of the FIRST
// entry that names a call takes all of that call's entries, in order, so a call named twice gets both and no two waves
// write one state.  The scalars are wave-uniform and written by one lane, the 416 soft bits are cleared by all lanes.
__global__ __launch_bounds__(64 * kWalkWaves) void k_tch3f_assign(int n, const int32_t *__restrict__ call, const int32_t *__restrict__ p,
                                                                  const float *__restrict__ ref_energy, gmr1_hip_tch3_state *state)
{
	const int lane = threadIdx.x & 63;
	const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWalkWaves + (threadIdx.x >> 6)));
	if (w >= n)
		return;
	const int c = call[w];
	if (c < 0)
		return;
	for (int j0 = 0; j0 < w; j0 += 64) {           // an earlier entry names this call: its wave applies this one too
		const int j = j0 + lane;
		if (__ballot(j < w && call[j] == c))
			return;
	}
	gmr1_hip_tch3_state *st = state + c;
	Tch3Walk s;
	s.active = st->active; s.p = st->p; s.ciph = st->ciph; s.weak_cnt = st->weak_cnt;
	s.sync_id = st->sync_id; s.burst_cnt = st->burst_cnt;
	s.energy_dkab = st->energy_dkab; s.energy_burst = st->energy_burst;
#pragma unroll
	for (int i = 0; i < 4; i++)
		s.bi_fn[i] = st->bi_fn[i];
	for (int j0 = w; j0 < n; j0 += 64) {
		const int j = j0 + lane;
		unsigned long long m = __ballot(j < n && call[j] == c);
		while (m) {
			const int k = j0 + __builtin_ctzll(m);
			m &= m - 1;
			tch3_follow_assign(s, p[k], ref_energy[k]);
		}
	}
	uint32_t *st_eb = reinterpret_cast<uint32_t *>(st->ebits);
	for (int i = lane; i < 104; i += 64)
		st_eb[i] = 0;
	if (lane == 0) {
		st->active = s.active; st->p = s.p; st->weak_cnt = s.weak_cnt; st->sync_id = s.sync_id;
		st->energy_dkab = s.energy_dkab; st->energy_burst = s.energy_burst;
	}
}

// The follower's frames closed up into audio blocks (tch3_audio.h): one wavefront per call.  A frame reports when its
// class is not OFF; its slot is the number of reporting frames in front of it, over all calls -- frames are contiguous
// over calls, so a wave counts the frames below its call's first one with the same ballot and popcount it then uses on its
// own, 64 frames a step (as k_tch9f_big does).  Lane j of a step writes frame j's slot into a.slot for the decoder that
// follows on the stream (k_ambe_audio), and the block's 16-byte header where the slot is below max_out.  The wave of the
// last call writes the count.  first[] is the caller's device memory: clamped as in the follower.
__global__ __launch_bounds__(64 * kWalkWaves) void k_tch3f_audio(Tch3AudioArgs a)
{
	const int lane = threadIdx.x & 63;
	const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWalkWaves + (threadIdx.x >> 6)));
	if (c >= a.n_calls)
		return;
	const int kf = ambe_calls_span(a.first, 0, a.n_frames).lo;
	const AmbeSpan sp = ambe_calls_span(a.first, c, a.n_frames);
	const uint8_t *rec = reinterpret_cast<const uint8_t *>(a.frames);
	int base = 0;
	for (int kb = kf; kb < sp.lo; kb += 64) {
		const int k = kb + lane;
		base += __popcll(__ballot(k < sp.lo && tch3_audio_reports(rec[(size_t)k * kAmbeRecBytes + kAudioRecCls])));
	}
	if (a.call_base && lane == 0)
		a.call_base[c] = base;
	const uint64_t lab = a.label[c];
	for (int kb = sp.lo; kb < sp.hi; kb += 64) {
		const int k = kb + lane;
		const unsigned cls = k < sp.hi ? rec[(size_t)k * kAmbeRecBytes + kAudioRecCls] : (unsigned)kAudioClsOff;
		const bool mine = k < sp.hi && tch3_audio_reports(cls);
		const unsigned long long rep = __ballot(mine);
		const int slot = tch3_audio_slot(base, rep, lane);
		if (k < sp.hi)
			a.slot[k] = mine ? slot : kAudioNoSlot;
		if (mine && slot < a.max_out) {
			const AudioHead h = tch3_audio_head(lab, cls, a.fn[k]);
			*reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(a.out) + (size_t)slot * kAudioBytes) =
			    make_uint4(h.w[0], h.w[1], h.w[2], h.w[3]);
		}
		base += __popcll(rep);
	}
	if (c == a.n_calls - 1 && lane == 0)
		*a.n_out = base;
}

hipError_t launch_tch3f_audio(const Tch3AudioArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch3f_audio, dim3((a.n_calls + kWalkWaves - 1) / kWalkWaves), dim3(64 * kWalkWaves), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_tch3f_assign(int n, const int32_t *call, const int32_t *p, const float *ref_energy,
                               struct gmr1_hip_tch3_state *state, hipStream_t stream)
{
	if (n <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch3f_assign, dim3((n + kWalkWaves - 1) / kWalkWaves), dim3(64 * kWalkWaves), 0, stream, n, call, p,
	                   ref_energy, state);
	return hipGetLastError();
}

hipError_t launch_tch3f_prep(const Tch3FollowArgs &a, hipStream_t stream)
{
	if (a.n_frames <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch3f_prep, dim3((a.n_frames + 255) / 256), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_tch3f_walk(const Tch3FollowArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch3f_walk, dim3((a.n_calls + kWalkWaves - 1) / kWalkWaves), dim3(64 * kWalkWaves), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_tch3f_emit(const Tch3FollowArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch3f_emit, dim3((a.n_calls + 63) / 64), dim3(64), 0, stream, a);
	return hipGetLastError();
}

}  // namespace gmr1
