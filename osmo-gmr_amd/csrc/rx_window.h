// rx_window.h -- a burst's window of samples: the one-burst LDS carve-up, HBM -> registers -> LDS, DC / power
// statistics, burst energy.
#pragma once
#include "conv_k5_12.h"
#include "rx_touch.h"

namespace gmr1 {

static constexpr int kEbRow = 448;                // LDS bytes per soft-bit row (>= 432, /16)
static constexpr int kEbitsLds = 704;             // single-burst soft-bit buffer (>= 662)

// ---------------------------------------------------------------------------
// LDS carve-up of one wavefront
//   [x | aux | eb]   aux = corr + coef during the sync search, y afterwards
//   after the 4 demods of a fused wave, bm and surv overlay x
// ---------------------------------------------------------------------------
struct Lds {
	float2 *x;        // normalised input window           [max_in_len]
	float *corr;      // accumulated sync correlation      [kMaxWindow]      (aux)
	float2 *coef;     // rotated sync reference            [kMaxCoef]        (aux + 1 KiB)
	float2 *y;        // decimated symbols                 [max_len]         (aux)
	int8_t *eb;       // soft bits: 4 rows (fused) or one buffer
	uint32_t *bm;     // branch metrics 4 x 212            (overlays x)
	uint64_t *surv;   // 13 x 64 halfwords of window decisions (overlays x, after bm)
	uint32_t *ubits;  // decoded bits, 4 rows x 8 words    (overlays x, after surv)
};

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

__host__ __device__ inline size_t lds_corr_bytes(int max_len, bool decode)
{
	if (decode)
		return align16((size_t)max_len * 4);
	return align16((size_t)(max_len > kMaxWindow ? max_len : kMaxWindow) * 4);
}

__host__ __device__ inline size_t lds_layout(int max_in_len, int max_len, bool decode, size_t *off)
{
	size_t o = 0;
	size_t xbytes = align16((size_t)max_in_len * 8);
	const size_t dec_bytes = 4 * kSteps12 * 4 + kSteps12 * 8 + 4 * 8 * 4;
	if (decode && xbytes < dec_bytes)
		xbytes = align16(dec_bytes);
	off[0] = o; o += xbytes;
	// aux = correlation accumulator + rotated sync reference.  The fused BCCH / CCCH path knows
	// its formats (<= max_len lags, 17 sync symbols), which keeps 15 wavefronts per CU resident
	// (demodulation only: the caller's lag count when it passes the 256 the layout has always had room for)
	const size_t corr_bytes = lds_corr_bytes(max_len, decode);
	const size_t coef_bytes = decode ? 32 * 8 : (size_t)kMaxCoef * 8;
	off[1] = o; o += corr_bytes + coef_bytes;
	off[2] = o; o += decode ? 4 * kEbRow : kEbitsLds;
	return align16(o);
}

__device__ __forceinline__ Lds lds_carve(unsigned char *raw, int max_in_len, int max_len, bool decode)
{
	size_t off[3];
	lds_layout(max_in_len, max_len, decode, off);
	Lds L;
	L.x = reinterpret_cast<float2 *>(raw + off[0]);
	L.corr = reinterpret_cast<float *>(raw + off[1]);
	L.coef = reinterpret_cast<float2 *>(raw + off[1] + lds_corr_bytes(max_len, decode));
	L.y = reinterpret_cast<float2 *>(raw + off[1]);
	L.eb = reinterpret_cast<int8_t *>(raw + off[2]);
	L.bm = reinterpret_cast<uint32_t *>(raw + off[0]);
	L.surv = reinterpret_cast<uint64_t *>(raw + off[0] + 4 * kSteps12 * 4);
	L.ubits = reinterpret_cast<uint32_t *>(raw + off[0] + 4 * kSteps12 * 4 + kSteps12 * 8);
	return L;
}

// ---------------------------------------------------------------------------
// building blocks of the demodulator, one burst per wavefront
// ---------------------------------------------------------------------------

// window HBM -> registers -> LDS, DC and power normalised
template <int NPL>
__device__ __forceinline__ void load_normalise_stats(const float2 *__restrict__ in, int in_len, const Lds &L, int lane,
                                                     float &avr_o, float &avi_o, float &inv_o)
{
	// ---- load + normalise (osmo_cxvec_sig_normalize, decim 1) ------------------
	// rows k < nfull are whole (no lane test); row nfull is the ragged tail
	float2 v[NPL];
	float sr = 0.f, si = 0.f;
	const int nfull = in_len >> 6;
	const bool tail = (lane + 64 * nfull) < in_len;
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		if (k < nfull)
			v[k] = in[lane + 64 * k];
		else if (k == nfull && tail)
			v[k] = in[lane + 64 * k];
		else
			v[k] = make_float2(0.f, 0.f);
		sr += v[k].x;
		si += v[k].y;
	}
	sr = wave_sum(sr);
	si = wave_sum(si);
	// mean / sigma only fix the DC offset and an overall scale that nothing downstream depends
	// on, so reciprocals (1 ulp) stand in for the reference's divisions and square root
	const float inv_n = __builtin_amdgcn_rcpf((float)in_len);
	// (the mean keeps the true division: a constant window must normalise to exactly zero)
	const float avr = sr / (float)in_len, avi = si / (float)in_len;
	float acc = 0.f;
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		if (k < nfull || (k == nfull && tail)) {
			v[k].x -= avr;
			v[k].y -= avi;
			acc = fmaf(v[k].x, v[k].x, fmaf(v[k].y, v[k].y, acc));
		}
	}
	float sigma = wave_sum(acc) * inv_n;
	float stddev = __builtin_amdgcn_sqrtf(sigma);
	if (stddev == 0.0f)
		stddev = 1.0f;
	const float inv = __builtin_amdgcn_rcpf(stddev);
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		if (k < nfull || (k == nfull && tail))
			L.x[lane + 64 * k] = make_float2(v[k].x * inv, v[k].y * inv);
	}
	avr_o = avr;
	avi_o = avi;
	inv_o = inv;
}

// window statistics only (mean, 1/sigma); the samples stay in registers and are dropped
// NFULL >= 0: the caller knows in_len >> 6 at compile time (the fused sps = 4 path: 1016 and 976
// samples both have 15 whole rows), which removes the per-row branches
// RS = 64: `in` is the window, lane l takes samples l + 64 k.  RS = 16 (polyphase-planar array at 4 samples per symbol,
// rx4_body's PL): `in` is already this lane's first sample in its plane, sample l + 64 k is 16 k places further on.
template <int NPL, int NFULL = -1, int RS = 64>
__device__ __forceinline__ void window_fetch(const float2 *__restrict__ in, int in_len, int lane, float2 (&v)[NPL])
{
	const int nfull = NFULL >= 0 ? NFULL : (in_len >> 6);
	const bool tail = (lane + 64 * nfull) < in_len;
	const int l0 = RS == 64 ? lane : 0;
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		if (k < nfull)
			v[k] = in[l0 + RS * k];
		else if (k == nfull && tail)
			v[k] = in[l0 + RS * k];
		else
			v[k] = make_float2(0.f, 0.f);
	}
}

// perm_src >= 0 (rx4_body's PL): this lane holds the samples of ANOTHER lane of the usual assignment (`lane` names that
// one); the per-lane partial sums -- formed over the same samples in the same order -- are first moved to the lane that
// usually forms them (every lane fetches from lane perm_src), so the cross-lane sums add the same numbers in the same
// order and the statistics come out bit-identical.
template <int NPL, int NFULL = -1>
__device__ __forceinline__ void window_stats(const float2 (&v)[NPL], int in_len, int lane,
                                             float &avr_o, float &avi_o, float &inv_o, int perm_src = -1, int odd_src = 1)
{
	auto home = [&](float x) {
		return perm_src < 0 ? x : __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(perm_src << 2, __builtin_bit_cast(int, x)));
	};
	// (re, im) pairs through the packed FP32 pipe: one v_pk_add_f32 per sample for the sums, one v_pk_add_f32 and
	// one v_pk_fma_f32 for the variance (re and im are summed in separate chains, as they are in the mean)
	v2f s2 = {0.f, 0.f};
	const int nfull = NFULL >= 0 ? NFULL : (in_len >> 6);
	const bool tail = (lane + 64 * nfull) < in_len;
#pragma unroll
	for (int k = 0; k < NPL; k++)
		s2 += (v2f){v[k].x, v[k].y};
	const float sr = wave_sum(home(s2.x));
	const float si = wave_sum(home(s2.y));
	const float inv_n = __builtin_amdgcn_rcpf((float)in_len);
	// true division, see load_normalise -- ONE division sequence for the two wave-uniform sums: lanes with an even `lane`
	// divide the real sum, those with an odd one (wave lane odd_src is one) the imaginary sum
	const float quot = ((lane & 1) ? si : sr) / (float)in_len;
	const float avr = lane_val(quot, 0), avi = lane_val(quot, odd_src);
	const v2f av = {avr, avi};
	v2f acc2 = {0.f, 0.f};
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		if (k < nfull || (k == nfull && tail)) {
			const v2f d = (v2f){v[k].x, v[k].y} - av;
			acc2 = __builtin_elementwise_fma(d, d, acc2);
		}
	}
	float stddev = __builtin_amdgcn_sqrtf(wave_sum(home(acc2.x + acc2.y)) * inv_n);
	if (stddev == 0.0f)
		stddev = 1.0f;
	avr_o = avr;
	avi_o = avi;
	inv_o = __builtin_amdgcn_rcpf(stddev);
}

template <int NPL, int NFULL = -1>
__device__ __forceinline__ void load_stats(const float2 *__restrict__ in, int in_len, int lane,
                                           float &avr_o, float &avi_o, float &inv_o)
{
	float2 v[NPL];
	window_fetch<NPL, NFULL>(in, in_len, lane, v);
	window_stats<NPL, NFULL>(v, in_len, lane, avr_o, avi_o, inv_o);
}

// ---- the QUAD layout of a window in registers (rx4_body's QL: the fused batch kernel at 4 samples per symbol) ----
// Lane l holds window samples 256 b + 4 l + c as v[4 b + c] (b = 0..3, c = 0..3): four CONSECUTIVE samples of each quarter
// of the window, fetched as two 16-byte loads a quarter (a wave instruction covers 1 KB, every line asked for whole).
// What it buys: the samples pass 2 keeps -- d, d + 4, d + 8, ... (pi4cxpsk.c:292-295) -- are sub-slot c = d & 3 of EVERY lane
// of every quarter, one per lane and quarter, in lane order: kept sample i sits in lane (i + (d >> 2)) & 63 of quarter
// (i + (d >> 2)) >> 6.  A lane ROTATION by d >> 2 (ds_bpermute, no LDS memory) puts kept sample l + 64 r into lane l --
// pass 2's own assignment -- while the window is still in registers: no second trip to memory for it (rx4_body, QX).
// With the samples stored polyphase-planar the same assignment is lane l <- place l + 64 b of plane c: a coalesced 512-byte
// load, and the per-lane partial sums below are formed over the same samples in the same order, so the planar call's
// statistics equal the interleaved call's bit for bit.
typedef float v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));
// ONE: every register pair of the ragged last quarter is the destination of ONE load.  With the two alternative loads of the
// plain form (sixteen bytes where both samples lie inside the window, eight where only the first does) the second is held
// back until the first has arrived -- the same registers -- and with it everything asked for behind it: a burst's window
// came in three round trips in a row instead of one.  A lane whose second sample lies outside takes its sixteen bytes one
// sample EARLIER (inside the window: the last quarter starts at sample 768) and keeps the upper half: the same values.
// That lane's registers are put right by window_fix_q, which the caller runs once everything else has been asked for (a
// select on the spot would wait for the load on the spot).
template <bool ONE = false>
__device__ __forceinline__ void window_fetch_q(const float2 *__restrict__ in, int in_len, int lane, float2 (&v)[16])
{
	const v4f_a8 *__restrict__ p = reinterpret_cast<const v4f_a8 *>(in + 4 * lane);
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const int s0 = 256 * b + 4 * lane;
#pragma unroll
		for (int h = 0; h < 2; h++) {
			float2 lo = make_float2(0.f, 0.f), hi = make_float2(0.f, 0.f);
			if (ONE && b == 3) {
				const bool full = s0 + 2 * h + 1 < in_len, part = !full && s0 + 2 * h < in_len;
				if (full || part) {
					const v4f_a8 u = *reinterpret_cast<const v4f_a8 *>(in + s0 + 2 * h - (part ? 1 : 0));
					lo = make_float2(u.x, u.y);
					hi = make_float2(u.z, u.w);
				}
			} else
			if (b < 3 || s0 + 2 * h + 1 < in_len) {        // (in_len >= 960: the first three quarters are whole)
				const v4f_a8 u = p[128 * b + h];
				lo = make_float2(u.x, u.y);
				hi = make_float2(u.z, u.w);
			} else if (s0 + 2 * h < in_len) {
				lo = in[s0 + 2 * h];
			}
			v[4 * b + 2 * h] = lo;
			v[4 * b + 2 * h + 1] = hi;
		}
	}
}

__device__ __forceinline__ void window_fix_q(int in_len, int lane, float2 (&v)[16])
{
	const int s0 = 256 * 3 + 4 * lane;
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const bool part = s0 + 2 * h + 1 >= in_len && s0 + 2 * h < in_len;
		v[12 + 2 * h] = part ? v[12 + 2 * h + 1] : v[12 + 2 * h];
		v[12 + 2 * h + 1] = part ? make_float2(0.f, 0.f) : v[12 + 2 * h + 1];
	}
}

// The wave's look-ahead as lines in the XCD's L2: every 128-byte line the NEXT burst's window overlaps is asked for with one
// dword load a lane (a second window in registers costs the sixth wave, see Rx4Switches::PREFETCH_NEXT).  The addresses
// are window_touch_offset's (rx_touch.h), all inside the window's own bytes.  Plain loads: a volatile one is a flat load
// at system scope with a full wait right behind it.  What keeps them alive is the caller handing the returned word to
// window_touch_done() -- an empty asm that names the register -- at a point where waiting costs nothing; the wait counts
// stay the compiler's own.
struct Touched { uint32_t a, b; };
__device__ __forceinline__ Touched window_touch_q(const float2 *__restrict__ next, int in_len, int lane)
{
	const char *base = reinterpret_cast<const char *>(next);
	const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(next) & (uintptr_t)(kTouchLine - 1));
	const int o = window_touch_offset(mis, in_len, lane);
	Touched t = {0, 0};                                         // (two words, never combined: combining them would wait for both)
	if (o >= 0)
		t.a = *reinterpret_cast<const uint32_t *>(base + o);
	const int o64 = window_touch_offset(mis, in_len, 64);       // (wave-uniform: the 65th line of a window that starts inside a line)
	if (o64 >= 0 && lane == 0)
		t.b = *reinterpret_cast<const uint32_t *>(base + o64);
	return t;
}
__device__ __forceinline__ void window_touch_done(const Touched &t)
{
	asm volatile("" : : "v"(t.a), "v"(t.b));
}

// the same assignment out of a polyphase-planar array: `pl` = the array, o = the window's first sample (flat count)
__device__ __forceinline__ void window_fetch_q_planar(const float2 *__restrict__ pl, long long plane_stride, uint64_t o, int in_len,
                                                      int lane, float2 (&v)[16])
{
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const uint64_t oc = o + (uint64_t)c;
		const float2 *__restrict__ src = pl + (long long)(oc & 3) * plane_stride + (long long)(oc >> 2) + lane;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int sidx = 256 * b + 4 * lane + c;
			v[4 * b + c] = (b < 3 || sidx < in_len) ? src[64 * b] : make_float2(0.f, 0.f);
		}
	}
}

// mean and 1 / sigma of a window in the quad layout (osmo_cxvec_sig_normalize's statistics), ONE sweep: sum x and sum |x|^2
// together -- sum |x - m|^2 = sum |x|^2 - n |m|^2, never below zero -- as the small formats' pass 1 has always had it: sigma only
// sets a scale nothing downstream depends on (every consumer takes an angle, a ratio of energies or the place of a peak), and a
// second sweep over sixteen register pairs for the variance about the mean is a third of the statistics' instructions.  Packed
// sums, ONE true division sequence for the two means (a constant window must normalise to exactly zero), reciprocals elsewhere.
__device__ __forceinline__ void window_stats_q(const float2 (&v)[16], int in_len, int lane, float &avr_o, float &avi_o, float &inv_o)
{
	v2f s2 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll
	for (int k = 0; k < 16; k++) {
		const v2f x = {v[k].x, v[k].y};                     // (samples beyond the window are zeros)
		s2 += x;
		q2 = __builtin_elementwise_fma(x, x, q2);
	}
	const float sr = wave_sum(s2.x);
	const float si = wave_sum(s2.y);
	const float sq = wave_sum(q2.x + q2.y);
	const float inv_n = __builtin_amdgcn_rcpf((float)in_len);
	const float quot = ((lane & 1) ? si : sr) / (float)in_len;
	const float avr = lane_val(quot, 0), avi = lane_val(quot, 1);
	const float var = fmaxf(fmaf(-(float)in_len, fmaf(avr, avr, avi * avi), sq), 0.0f) * inv_n;
	float stddev = __builtin_amdgcn_sqrtf(var);
	if (stddev == 0.0f)
		stddev = 1.0f;
	avr_o = avr;
	avi_o = avi;
	inv_o = __builtin_amdgcn_rcpf(stddev);
}

// The window's mean as the reference forms it (osmo_cxvec_sig_normalize): ONE fp32 sum in sample order, then a true division.
// Under a constant offset of the burst's own amplitude that sum ends about 1e-6 from the exact mean, the wave's tree sums
// within 1e-7 of it -- and a sample that all but vanishes once the mean is out (a guard symbol's noise, 1e-3 of the burst)
// turns the difference into 1e-4 ... 5e-4 of a soft-symbol step.  Soft SYMBOLS are held to the reference's to 1e-4, so the
// callers that write them out form them about this mean; nothing else uses it (soft bits come from symbols that carry
// energy), and a call without the soft-symbol output never runs it.  Every lane walks the same addresses.
__device__ __forceinline__ float2 window_mean_serial(const float2 *__restrict__ in, int in_len)
{
	float sr = 0.f, si = 0.f;
	for (int i = 0; i < in_len; i++) {
		const float2 v = in[i];
		sr += v.x;
		si += v.y;
	}
	return make_float2(sr / (float)in_len, si / (float)in_len);
}

// burst_energy() of the caller (gmr1_rx.c:172-182): sum |x|^2 over [len>>5, len - len>>5) of the RAW
// window, divided by len.  Only the receive driver asks for it (RxArgs::energy); the window was
// read a moment ago, so this second read is served by L1 / L2.
template <int NPL>
__device__ __noinline__ float window_energy(const float2 *__restrict__ in, int in_len, int lane)
{
	const int bd = in_len >> 5;
	float e = 0.f;
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		const int idx = lane + 64 * k;
		if (idx >= bd && idx < in_len - bd) {
			const float2 v = in[idx];
			e = fmaf(v.x, v.x, fmaf(v.y, v.y, e));
		}
	}
	return wave_sum(e) / (float)in_len;
}

// the same sum over a window that is still in registers (window_fetch layout): identical operations in
// identical order, without the second read
template <int NPL>
__device__ __forceinline__ float window_energy_regs(const float2 (&v)[NPL], int in_len, int lane)
{
	const int bd = in_len >> 5;
	float e = 0.f;
#pragma unroll
	for (int k = 0; k < NPL; k++) {
		const int idx = lane + 64 * k;
		if (idx >= bd && idx < in_len - bd)
			e = fmaf(v[k].x, v[k].x, fmaf(v[k].y, v[k].y, e));
	}
	return wave_sum(e) / (float)in_len;
}

template <int NPL>
__device__ __forceinline__ void load_normalise(const float2 *__restrict__ in, int in_len, const Lds &L, int lane)
{
	float a, b, c;
	load_normalise_stats<NPL>(in, in_len, L, lane, a, b, c);
}

}  // namespace gmr1
