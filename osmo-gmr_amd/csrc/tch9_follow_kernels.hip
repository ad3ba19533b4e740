// tch9_follow_kernels.hip -- the device side of gmr1_hip_tch9_follow* that is not a demodulator or a decoder (gfx950).
//
// The entry (capi_tch9_follow.cpp) runs, on one stream and without the host in between:
//   k_tch9f_plan   one wavefront per call: every frame's class, the decode it asks for and, for a TCH9 frame, where the two
//                  bursts in front of it in the inter-burst de-interleaver come from (tch9_follow.h)
//   k_a5_tch9f     (tch_kernels.hip) keystreams of the frames that ask for a decode
//   k_nt9 <JOBS>   (nt9_kernels.hip) twice over the frame slots: the FACCH9 frames, the TCH9 frames
//   k_tch9f_emit   one wavefront per call: the caller's records, and the call's last two TCH9 bursts, deciphered, into its state
// and, between two invocations, k_tch9f_assign (gmr1_hip_tch9_state_assign_batch_dev): rx_tch9_init on the states where they lie.
// For the receive loop's callers: k_tch9f_big (gmr1_hip_tch9_frames_to_records_dev) closes the reporting frames up into big
// records, and k_tch9f_move copies whole states between two device arrays (the streaming push gathers its calls' states
// and adopts the last one of every chain).
//
// Nothing here is a chain: a frame's class depends on nothing before it, and its sources are the nearest two TCH9 frames
// below it -- one ballot of "is TCH9" per 64 frames and two highest-set-bit searches below the lane, the last two TCH9
// frames carried from step to step and seeded from what the state holds.
#include <cstddef>

#include "gmr1_dev.h"
#include "tch9_follow.h"
#include "wave_ops.h"

namespace gmr1 {

static_assert(sizeof(gmr1_hip_tch9_state) == 1340 && sizeof(gmr1_hip_tch9_frame) == 80, "public layout");
static_assert(offsetof(gmr1_hip_tch9_state, held) == 16 && offsetof(gmr1_hip_tch9_frame, l2) == 12, "public layout");
static_assert(sizeof(gmr1_hip_rx_big_record) == 80 && offsetof(gmr1_hip_rx_big_record, l2) == 16 &&
              offsetof(gmr1_hip_rx_big_record, tn) == 8 && offsetof(gmr1_hip_rx_big_record, conv) == 12, "public layout");
static_assert(offsetof(gmr1_hip_tch9_frame, type) == 1 && offsetof(gmr1_hip_tch9_frame, fn) == 4 &&
              offsetof(gmr1_hip_tch9_frame, conv) == 8 && sizeof(gmr1_hip_tch9_state) % 4 == 0, "public layout");
static_assert(kT9Off == GMR1_HIP_TCH9_OFF && kT9Facch == GMR1_HIP_TCH9_FACCH9 && kT9Tch == GMR1_HIP_TCH9_TCH9 &&
              kT9Err == GMR1_HIP_TCH9_ERR, "classes");

constexpr int kT9Waves = 4;                // calls per work-group

// first[] of the _dev entry is the caller's device memory: whatever it holds, no frame index leaves 0..n_frames
__device__ __forceinline__ int clamp_frame9(int v, int lo, int n_frames)
{
	return v < lo ? lo : v > n_frames ? n_frames : v;
}

__global__ __launch_bounds__(64 * kT9Waves) void k_tch9f_plan(Tch9FollowArgs a)
{
	const int lane = threadIdx.x & 63;
	const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kT9Waves + (threadIdx.x >> 6)));
	if (c >= a.n_calls)
		return;
	const int k0 = clamp_frame9(a.first[c], 0, a.n_frames), k1 = clamp_frame9(a.first[c + 1], k0, a.n_frames);
	if (k1 <= k0)
		return;
	const int active = a.state[c].active;
	Tch9Carry carry = tch9f_seed(a.state[c].n_held);
	for (int kb = k0; kb < k1; kb += 64) {
		const int k = kb + lane;
		const bool in = k < k1;
		const int cls = in ? tch9f_class(active, a.rv ? a.rv[k] : 0, a.sync_id[k]) : kT9Off;
		const unsigned long long tch = __ballot(in && cls == kT9Tch);
		if (in) {
			const Tch9Carry s = tch9f_sources(tch, lane, kb, carry);
			a.cls[k] = (uint8_t)cls;
			a.need[k] = (uint8_t)tch9f_need(cls);
			a.src[3 * (size_t)k] = k;
			a.src[3 * (size_t)k + 1] = s.s1;
			a.src[3 * (size_t)k + 2] = s.s2;
			a.call_of[k] = c;
		}
		carry = tch9f_sources(tch, 64, kb, carry);
	}
}

__global__ __launch_bounds__(64 * kT9Waves) void k_tch9f_emit(Tch9FollowArgs a)
{
	const int lane = threadIdx.x & 63;
	const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kT9Waves + (threadIdx.x >> 6)));
	if (c >= a.n_calls)
		return;
	const int k0 = clamp_frame9(a.first[c], 0, a.n_frames), k1 = clamp_frame9(a.first[c + 1], k0, a.n_frames);
	if (k1 <= k0)
		return;                                    // a call without frames keeps its state untouched

	// ---- the records, 20 words each, a word per lane
	uint32_t *out = reinterpret_cast<uint32_t *>(a.out);
	const int n_words = (k1 - k0) * 20;
	for (int w = lane; w < n_words; w += 64) {
		const int k = k0 + w / 20, j = w % 20;
		const int need = a.need[k];
		const bool fa = need == kT9NeedFacch, tc = need == kT9NeedTch;
		const int crc = fa && a.fa_crc[k] ? 1 : 0;
		// a TCH9 block has no CRC to check (gmr1_rx.c:336-339); a FACCH9 message is reported when its CRC passes (:317)
		const int type = tc ? 0x18 : fa && !crc ? 0x1a : 0;
		const int len = tc ? a.l2_bytes : fa && !crc ? 38 : 0;
		uint32_t v = 0;
		if (j == 0) {
			v = (uint32_t)a.cls[k] | ((uint32_t)type << 8) | ((uint32_t)len << 16) | ((uint32_t)crc << 24);
		} else if (j == 1) {
			v = a.fn[k];
		} else if (j == 2) {
			v = (uint32_t)(fa ? a.fa_conv[k] : tc ? a.t_conv[k] : 0);
		} else if (j < 19) {
			const int b = 4 * (j - 3);
			if (b < len) {
				v = reinterpret_cast<const uint32_t *>((tc ? a.t_l2 : a.fa_l2) + (size_t)k * 64)[j - 3];
				if (len - b < 4)
					v &= (1u << (8 * (len - b))) - 1u;
			}
		}
		out[(size_t)k * 20 + j] = v;
	}

	// ---- the state: the call's last two TCH9 bursts, from this invocation's frames or from what it held
	Tch9Carry carry = tch9f_seed(a.state[c].n_held);
	for (int kb = k0; kb < k1; kb += 64) {
		const int k = kb + lane;
		const unsigned long long tch = __ballot(k < k1 && a.need[k] == kT9NeedTch);
		carry = tch9f_sources(tch, 64, kb, carry);
	}
	if (carry.s1 < 0)
		return;                                    // no TCH9 frame: nothing moves
	// a frame's soft bits with the keystream's sign flips applied, in bits_e order (tch9.c:152-160)
	auto taken_in = [&](int f, int i) -> int8_t {
		int v = a.ebits[(size_t)f * 662 + i];
		const int my = tch9f_e2my(i);
		if (my >= 0 && a.ks[(size_t)f * 658 + my])
			v = -v;
		return (int8_t)v;
	};
	int8_t *held = a.state[c].held;
	// slot 1 first: it may take what slot 0 holds (a lane moves the bytes it then overwrites itself)
	for (int i = lane; i < 662; i += 64)
		held[662 + i] = carry.s2 >= 0 ? taken_in(carry.s2, i) : carry.s2 == kT9SrcHeld0 ? held[i] : (int8_t)0;
	for (int i = lane; i < 662; i += 64)
		held[i] = taken_in(carry.s1, i);
	if (lane == 0)
		a.state[c].n_held = tch9f_n_held(carry);
}

// rx_tch9_init on device-resident states: entry j assigns state[call[j]].  One wavefront per entry; the wave of the FIRST
// entry that names a call does it (the assignment does not depend on how often it is made), so no two waves write one state.
__global__ __launch_bounds__(64 * kT9Waves) void k_tch9f_assign(int n, const int32_t *__restrict__ call, gmr1_hip_tch9_state *state)
{
	const int lane = threadIdx.x & 63;
	const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kT9Waves + (threadIdx.x >> 6)));
	if (w >= n)
		return;
	const int c = call[w];
	if (c < 0)
		return;
	for (int j0 = 0; j0 < w; j0 += 64) {
		const int j = j0 + lane;
		if (__ballot(j < w && call[j] == c))
			return;
	}
	gmr1_hip_tch9_state *st = state + c;
	for (int i = lane; i < 2 * 662; i += 64)
		st->held[i] = 0;
	if (lane == 0) {
		st->active = 1;
		st->n_held = 0;
	}
}

// The follower's frames as gmr1_hip_rx_run_full reports them: one wavefront per call.  A frame reports when its type is
// not 0; its slot in `out` is the number of reporting frames in front of it, over all calls -- frames are contiguous over
// calls, so a wave counts the frames below its call's first one with the same ballot and popcount it then uses on its
// own, 64 frames a step, and nobody waits for anybody.  A record is five 16-byte stores: lane w of a step writes part
// w % 5 of the step's frame w / 5, whose slot it takes from that frame's lane.  Only slots below max_out are stored; the
// wave of the last call writes the count.  first[] is the caller's device memory: clamped as in the follower.
__global__ __launch_bounds__(64 * kT9Waves) void k_tch9f_big(Tch9BigArgs a)
{
	const int lane = threadIdx.x & 63;
	const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kT9Waves + (threadIdx.x >> 6)));
	if (c >= a.n_calls)
		return;
	const int kf = clamp_frame9(a.first[0], 0, a.n_frames);
	const int k0 = clamp_frame9(a.first[c], 0, a.n_frames), k1 = clamp_frame9(a.first[c + 1], k0, a.n_frames);
	int base = 0;
	for (int kb = kf; kb < k0; kb += 64) {
		const int k = kb + lane;
		base += __popcll(__ballot(k < k0 && a.frames[k].type != 0));
	}
	const uint32_t lab = a.label[c];
	for (int kb = k0; kb < k1; kb += 64) {
		const int k = kb + lane;
		const unsigned long long rep = __ballot(k < k1 && a.frames[k].type != 0);
		const int slot = base + __popcll(rep & ((1ull << lane) - 1ull));
		for (int w = lane; w < 64 * 5; w += 64) {
			const int i = w / 5, j = w % 5;
			const int s = __shfl(slot, i);
			if (!((rep >> i) & 1ull) || s >= a.max_out)
				continue;
			const uint32_t *f = reinterpret_cast<const uint32_t *>(a.frames + kb + i);
			const uint32_t w0 = f[0];
			const uint32_t type = (w0 >> 8) & 0xffu, len = (w0 >> 16) & 0xffu;
			uint4 v;
			if (j == 0) {
				v.x = (lab & 0x00ffffffu) | (type << 24);        // arfcn, chain, type
				v.y = f[1];                                      // fn
				v.z = (lab >> 24) | (len << 16);                 // tn, crc 0, len, pad 0
				v.w = f[2];                                      // conv
			} else {
				uint32_t q[4];
				for (int t = 0; t < 4; t++) {
					const int b = 16 * (j - 1) + 4 * t;          // first byte of the word in l2
					const int left = (int)len - b;
					q[t] = left <= 0 ? 0u : f[3 + b / 4] & (left >= 4 ? 0xffffffffu : (1u << (8 * left)) - 1u);
				}
				v = make_uint4(q[0], q[1], q[2], q[3]);
			}
			reinterpret_cast<uint4 *>(a.out + s)[j] = v;
		}
		base += __popcll(rep);
	}
	if (c == a.n_calls - 1 && lane == 0)
		*a.n_out = base;
}

// whole states from one device array to another: pair j copies src[src_at[j]] to dst[dst_at[j]], one wavefront per pair
// (no two pairs of a launch name one destination)
__global__ __launch_bounds__(64 * kT9Waves) void k_tch9f_move(int n, gmr1_hip_tch9_state *dst, const int32_t *__restrict__ dst_at,
                                                                const gmr1_hip_tch9_state *src, const int32_t *__restrict__ src_at)
{
	const int lane = threadIdx.x & 63;
	const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kT9Waves + (threadIdx.x >> 6)));
	if (w >= n)
		return;
	const uint32_t *s = reinterpret_cast<const uint32_t *>(src + src_at[w]);
	uint32_t *d = reinterpret_cast<uint32_t *>(dst + dst_at[w]);
	for (int i = lane; i < (int)(sizeof(gmr1_hip_tch9_state) / 4); i += 64)
		d[i] = s[i];
}

hipError_t launch_tch9f_big(const Tch9BigArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch9f_big, dim3((a.n_calls + kT9Waves - 1) / kT9Waves), dim3(64 * kT9Waves), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_tch9f_move(int n, struct gmr1_hip_tch9_state *dst, const int32_t *dst_at, const struct gmr1_hip_tch9_state *src,
                             const int32_t *src_at, hipStream_t stream)
{
	if (n <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch9f_move, dim3((n + kT9Waves - 1) / kT9Waves), dim3(64 * kT9Waves), 0, stream, n, dst, dst_at, src, src_at);
	return hipGetLastError();
}

hipError_t launch_tch9f_assign(int n, const int32_t *call, struct gmr1_hip_tch9_state *state, hipStream_t stream)
{
	if (n <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch9f_assign, dim3((n + kT9Waves - 1) / kT9Waves), dim3(64 * kT9Waves), 0, stream, n, call, state);
	return hipGetLastError();
}

hipError_t launch_tch9f_plan(const Tch9FollowArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch9f_plan, dim3((a.n_calls + kT9Waves - 1) / kT9Waves), dim3(64 * kT9Waves), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_tch9f_emit(const Tch9FollowArgs &a, hipStream_t stream)
{
	if (a.n_calls <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_tch9f_emit, dim3((a.n_calls + kT9Waves - 1) / kT9Waves), dim3(64 * kT9Waves), 0, stream, a);
	return hipGetLastError();
}

}  // namespace gmr1
