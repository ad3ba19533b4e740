// k_one_server -- the fused BCCH / DC6 burst body (rx4_body, exactly what k_rx4 runs for one burst) as a resident one-wave
// kernel that answers requests from a mailbox in pinned host memory.
// (part of rx_kernels.hip's translation unit, included by it after rx_debug_kernels.inc, inside namespace gmr1)
//
// An unchanged gmr1_rx.c calls gmr1_pi4cxpsk_demod once per burst and waits for the answer: a launch and a stream
// synchronisation per call cost about twice what the burst itself does (29 us a call; the kernel's share is 10).  With the
// server the call is: write the window and the request number into the block, spin on the answer's number.
//   * The wave polls the request number with system-scope loads (they bypass the caches), sleeps ~0.5 us between polls.
//   * Before it reads a request it invalidates the vector L1 / L2 lines and the scalar cache: the window and the
//     parameters sit at the SAME host addresses for every request, and a resident kernel sees no launch boundary that
//     would do it for it.
//   * It ends by itself: after idle_us without a request, after life_us in any case, or when the host has started a newer
//     generation -- nothing here can spin for ever, and a process that dies leaves nothing behind for longer than idle_us.
//     It leaves its generation number in `ended`; the host starts the next generation when the current one has ended
//     (capi_one.cpp), on the servers' one stream, so a new one starts when the last has gone.

}  // namespace gmr1 (left for the header, which opens it itself)
#include "rx_server.h"
namespace gmr1 {

__device__ __forceinline__ uint32_t one_ld_sys(const uint32_t *p)
{
	return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void one_st_sys(uint32_t *p, uint32_t v)
{
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool ACC>
__global__ __launch_bounds__(64) void k_one_server(RxArgs a, OneMail *mb, uint32_t gen, int stage_samples, int cw,
                                                   unsigned long long idle_ticks, unsigned long long life_ticks)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int lane = (int)threadIdx.x;
	const RxIo io = {
#ifdef GMR1_HIP_PROFILE
	                 nullptr,
#endif
	                 a.offset, a.kind, a.freq_shift, a.l2, a.crc, a.conv, a.rv, a.sync_id, a.toa, a.freq_err, a.energy,
	                 a.ebits, a.ssyms};
	uint32_t last = one_ld_sys(&mb->done);
	const unsigned long long t_start = wall_clock64();
	unsigned long long t_idle = t_start;
	for (;;) {
		const uint32_t r = one_ld_sys(&mb->req);
		const uint32_t g = one_ld_sys(&mb->gen);
		const unsigned long long now = wall_clock64();
		if (g != gen)
			break;                                   // superseded
		if (r != last) {
			// what the host wrote before it changed the number: not from this wave's caches
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
			asm volatile("s_dcache_inv\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
			rx4_body<CfgBatch<16, 4, ACC, false>>(a, io, stage_samples, cw, 0, 1, lds_raw, lane);
			WSYNC();
			__threadfence_system();                  // the answer is in host memory before its number is
			last = r;
			if (lane == 0)
				one_st_sys(&mb->done, r);
			t_idle = wall_clock64();
			if (t_idle - t_start > life_ticks)
				break;
			continue;
		}
		if (now - t_idle > idle_ticks || now - t_start > life_ticks)
			break;
		__builtin_amdgcn_s_sleep(8);
	}
	if (lane == 0)
		one_st_sys(&mb->ended, gen);
}

hipError_t launch_one_server(const RxArgs &a, OneMail *mail_dev, uint32_t gen, unsigned idle_us, unsigned life_us, hipStream_t stream)
{
	if (a.n != 1 || a.sps != 4 || !mail_dev || a.plane_stride || a.energy || a.seg_count)
		return hipErrorInvalidValue;
	// (the launch parameters of launch_rx_t for this shape: lags of the longer window, the fused layout with the decoded words
	// over the branch metrics)
	const int max_len = 20 * a.sps + 1;
	const int cw = (max_len + 15) & ~15;
	size_t off4[4];
	const size_t lds4 = lds4_layout(a.stage_samples, cw, off4, false, true);
	// ticks of the device's constant-rate wall counter (wall_clock64): its rate from the driver, once per device; 100 MHz only
	// if the driver does not say
	static int khz_of[64];
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
		return hipErrorInvalidDevice;
	if (khz_of[dev] == 0) {
		int khz = 0;
		if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
			khz = 100000;
		khz_of[dev] = khz;
	}
	const unsigned long long per_us_x1000 = (unsigned long long)khz_of[dev];
	const unsigned long long idle_ticks = (unsigned long long)idle_us * per_us_x1000 / 1000ull, life_ticks = (unsigned long long)life_us * per_us_x1000 / 1000ull;
	if (a.conv_acc)
		hipLaunchKernelGGL((k_one_server<true>), dim3(1), dim3(64), lds4, stream, a, mail_dev, gen, a.stage_samples, cw, idle_ticks, life_ticks);
	else
		hipLaunchKernelGGL((k_one_server<false>), dim3(1), dim3(64), lds4, stream, a, mail_dev, gen, a.stage_samples, cw, idle_ticks, life_ticks);
	return hipGetLastError();
}
