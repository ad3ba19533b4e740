// rx_stream_kernels.hip -- the staging step of the streaming receive loop (gmr1_hip_rx_stream_push*, capi_rx_stream.cpp).
//
// k_rx_stage, one launch per push: per carrier (blockIdx.y) the samples it keeps from the handle's current buffer and the
// caller's strided chunk go, back to back, into the other buffer of the handle's ping-pong pair, two complex samples per
// thread and step (16-byte stores; 16-byte loads where the source pair is aligned, else two 8-byte loads), grid-stride.
// The work-groups of column 0 also rebase the carrier's chain states onto the new buffer: align moves back by the samples
// dropped, len / base describe the new buffer, and a stopped or unstarted chain is released when the frame it waits at
// now passes rx_loop_advance's check (rx_stream.h).  The receive loop's own kernels then walk the states unchanged.
//
// k_rx_stage_copy, one more launch per push of a handle that follows TCH3 calls: the same copy with the same per-carrier
// parameters for the traffic carrier's buffer pair.  It touches no state and no error word -- the chains' walk is the
// BCCH carrier's alone -- and it is a kernel of its own so that k_rx_stage stays what it is.
#include "capi_common.h"
#include "rx_stream.h"

namespace gmr1 {

__global__ __launch_bounds__(256) void k_rx_stage(RxStageArgs a)
{
	const RxStageCarrier c = a.car[blockIdx.y];
	const long long total = (long long)c.kept + c.n_new;
	const long long pairs = (total + 1) >> 1;
	const float2 *src = a.src + c.src;
	const float2 *chunk = a.iq + c.iq;
	float2 *dst = a.dst + c.dst;                   // c.dst is a multiple of kRxKeepAlign: pair p is 16-byte aligned
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += (long long)gridDim.x * blockDim.x) {
		const long long j = 2 * p;
		const bool two = j + 1 < total;
		float2 v0, v1 = make_float2(0.f, 0.f);
		const float2 *s0 = j < c.kept ? src + j : chunk + (j - c.kept);
		const bool same = !two || (j < c.kept) == (j + 1 < c.kept);
		if (two && same && ((uintptr_t)s0 & 15) == 0) {
			const float4 q = *reinterpret_cast<const float4 *>(s0);
			v0 = make_float2(q.x, q.y);
			v1 = make_float2(q.z, q.w);
		} else {
			v0 = *s0;
			if (two)
				v1 = j + 1 < c.kept ? src[j + 1] : chunk[j + 1 - c.kept];
		}
		if (two)
			*reinterpret_cast<float4 *>(dst + j) = make_float4(v0.x, v0.y, v1.x, v1.y);
		else
			dst[j] = v0;
	}
	if (blockIdx.x != 0)
		return;
	const int reach = rx_stream_reach_back(a.sps);
	for (int k = c.c0 + (int)threadIdx.x; k < c.c1; k += blockDim.x) {
		RxLoopState s = a.state[k];
		s.base = c.dst;
		s.align -= c.shift;
		s.len = (int)total;
		s.done = rx_stream_next_done(s.done, s.align, s.len, a.sps, a.last);
		// Every window of this push's walk starts at most `reach` samples before the align the walk starts from (the
		// bound of rx_stream_reach_back holds over any stretch of frames, not only the first), so a chain whose align is
		// at least `reach` from the front of its carrier's kept samples cannot meet a window before them anywhere in the
		// walk.  The check is made here, where the walk's starting point is known, so that the loop's kernels stay the
		// one-shot ones: in a carrier that has dropped samples, a chain closer to the front fails the push (-EIO) instead
		// of having burst_map refuse a window the one-shot call reads.
		if (s.done == 0 && c.rebased && s.align < reach)
			atomicOr(a.err, 1);
		a.state[k] = s;
	}
}

__global__ __launch_bounds__(256) void k_rx_stage_copy(RxStageArgs a)
{
	// k_rx_stage's copy, restated: shared through an inline function it compiles to other instructions in k_rx_stage
	const RxStageCarrier c = a.car[blockIdx.y];
	const long long total = (long long)c.kept + c.n_new;
	const long long pairs = (total + 1) >> 1;
	const float2 *src = a.src + c.src;
	const float2 *chunk = a.iq + c.iq;
	float2 *dst = a.dst + c.dst;                   // c.dst is a multiple of kRxKeepAlign: pair p is 16-byte aligned
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += (long long)gridDim.x * blockDim.x) {
		const long long j = 2 * p;
		const bool two = j + 1 < total;
		float2 v0, v1 = make_float2(0.f, 0.f);
		const float2 *s0 = j < c.kept ? src + j : chunk + (j - c.kept);
		const bool same = !two || (j < c.kept) == (j + 1 < c.kept);
		if (two && same && ((uintptr_t)s0 & 15) == 0) {
			const float4 q = *reinterpret_cast<const float4 *>(s0);
			v0 = make_float2(q.x, q.y);
			v1 = make_float2(q.z, q.w);
		} else {
			v0 = *s0;
			if (two)
				v1 = j + 1 < c.kept ? src[j + 1] : chunk[j + 1 - c.kept];
		}
		if (two)
			*reinterpret_cast<float4 *>(dst + j) = make_float4(v0.x, v0.y, v1.x, v1.y);
		else
			dst[j] = v0;
	}
}

// a few work-groups per carrier are plenty to stream its samples
static unsigned rx_stage_columns(int max_pairs)
{
	int gx = (max_pairs + 255) / 256;
	if (gx > 64) gx = 64;
	if (gx < 1) gx = 1;
	return (unsigned)gx;
}

hipError_t launch_rx_stage_copy(const RxStageArgs &a, hipStream_t stream)
{
	if (a.n_carriers <= 0)
		return hipSuccess;
	if (a.n_carriers > 65535 || a.max_pairs < 0 || !a.car || !a.dst)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_rx_stage_copy, dim3(rx_stage_columns(a.max_pairs), (unsigned)a.n_carriers), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_rx_stage(const RxStageArgs &a, hipStream_t stream)
{
	if (a.n_carriers <= 0)
		return hipSuccess;
	if (a.n_carriers > 65535 || a.max_pairs < 0 || !a.car || !a.err || !a.dst)
		return hipErrorInvalidValue;
	// column 0 also takes the chain states
	hipLaunchKernelGGL(k_rx_stage, dim3(rx_stage_columns(a.max_pairs), (unsigned)a.n_carriers), dim3(256), 0, stream, a);
	return hipGetLastError();
}

}  // namespace gmr1
