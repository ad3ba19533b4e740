// rx_kernels.hip -- the receive translation unit for gfx950 (MI355X).  This file holds the headline's own text: the fused
// BCCH / CCCH burst body rx4_body, the kernels around it (k_rx4, k_rx4g, k_rx4g_tch3) and their launchers.  The rest of the
// translation unit lives in files of its own, included below in the order of their definitions:
//
//   wave_ops.h           WSYNC, DPP moves and row / wave reductions, readlane, the LDS flags of the loop's hand-shakes
//   fast_math.h          sincos_fast, atan2_fast / _turns, cmul, pk_cmac, conj_ref_mul
//   conv_k5_12.h         the layer-1 chain: constant tables (trellis steps, costs, CRC syndromes, soft-bit tables), branch
//                        metrics, decode4_k5_12 / decode1_k5_12_lat, survivor walk + CRC16, store_l2
//                        (reference src/l1/bcch.c:83-103, src/l1/ccch.c:87-107 and libosmocore's osmo_conv_decode)
//   rx4_operands.h       (through conv_k5_12.h; no HIP in it) the trellis-step table's maker and the packed per-lane tables
//                        k_rx4 asks for in batches behind pass 1 (g_ord4, g_steps4), with the checks the host runs on them
//   rx_window.h          the one-burst LDS carve-up; window HBM -> registers -> LDS, statistics, burst energy
//   rx_one.h             sync_search, demod_one and k_rx: pi/4-CxPSK demodulation, one burst per wavefront; with DECODE four
//                        bursts back to back and the layer-1 chain behind them
//                        (reference src/sdr/pi4cxpsk.c:520-602 gmr1_pi4cxpsk_demod)
//   (here)               c_types, k_coef0; corr_fixed, the Lds4 carve-up, Fmt, LatPre and the loop's helpers;
//                        rx4_body: the same arithmetic as k_rx with the serial phases (timing bisection, sync-symbol terms)
//                        done once for the four bursts of a wave, one burst per 16-lane row;
//                        k_rx4 (the default fused BCCH / CCCH kernel), k_rx4g (demodulation only, four bursts per wave),
//                        k_rx4g_tch3 (with the TCH3 decoder behind it, tch3_body.h)
//   rx_small_kernels.h   k_detect, k_mod_order (gmr1_pi4cxpsk_detect / _mod_order, pi4cxpsk.c:617-729), k_l1 / k_l1_acc (the
//                        layer-1 chain alone on soft bits read from HBM), k_to_planar, with their launchers
//   (here)               launch_rx, launch_rx_tch3, the profiling build's accessors
//   rx_loop_kernels.inc  k_rx_chain_pipe, k_rx_chain, k_rx_merge, k_rx_pack: the frame loop of gmr1_rx (process_bcch,
//                        src/gmr1_rx.c:852-895): the chain kernel walks the BCCH feedback chain of one chain per work-group --
//                        rx4_body in its latency shape, cut into pipeline stages (PART) that run rounds apart on the
//                        work-group's waves -- and lists the CCCH bursts, k_rx4 takes those as one batch, k_rx_merge writes
//                        the records
//   rx_debug_kernels.inc the intermediate signals of one burst, for parity debugging
//   rx_server_kernels.inc  k_one_server: rx4_body behind a mailbox in pinned host memory
//
// Design notes (DESIGN.md has the long form):
//   * Work-groups are single 64-lane wavefronts: every hand-off goes through the
//     wave's own LDS slice and needs no s_barrier (the loop's chain kernels: several waves, one barrier per round).
//   * Samples are loaded once from HBM with coalesced 8-byte-per-lane loads, DC /
//     power normalised in registers and parked in LDS; everything else reads LDS.
//   * Burst formats live in __constant__ memory and are read with scalar loads.
//   * The sync search never derotates the window: |sum conj(ref_n) x[.] e^{j th n}|
//     is evaluated with per-burst rotated coefficients, which drops ~1000
//     sincos per burst.  Only the 234 decimated symbols are derotated.
//   * The sinc interpolation of the early/late timing loop needs one sine per
//     point: sin(pi (k - f)) = -(-1)^k sin(pi f) for integer tap offsets k.
//   * The Viterbi butterfly is in place: the two predecessors of a state sit in two lanes
//     of the row that differ by an xor mask (8, 7, 2, 1 over the four phases: one DPP control
//     each), so the partner's candidate arrives folded into the min and no metric ever moves.  A
//     state's 32-bit word is [metric:16 | decisions of the current 16-step window:16]; each lane
//     forms both candidates it sends on (two v_add3_u32: word + cost + tie-break bit) and v_min_u32
//     with DPP does compare, select, tie-break and decision recording at once -- three VALU per
//     trellis step (see decode4_k5_12).
#include <mutex>
#include <type_traits>

#include "gmr1_dev.h"
#include "tch3_body.h"
#include "wave_ops.h"
#include "fast_math.h"

namespace gmr1 {
// the burst formats (upload_types below fills them).  Defined ahead of conv_k5_12.h's tables, where they always stood:
// the order of the constant objects in the code object stays what it was
__constant__ DevBurst c_types[kNumTypes];
}  // namespace gmr1

#include "conv_k5_12.h"
#include "rx_window.h"

namespace gmr1 {

// where the soft bits of a lane's four symbols go, BCCH and DC6 (rx4_operands.h; upload_rx4_operands fills it from the
// host's burst tables, next to c_types)
__device__ Rx4Ord4 g_ord4;

#include "rx_one.h"

// ---------------------------------------------------------------------------
// k_rx4 -- fused BCCH / CCCH receive, four bursts per wavefront, with the serial phases
// (timing bisection, sync-symbol arithmetic) done ONCE for the four bursts, one burst per
// 16-lane row, instead of once per burst with most lanes idle:
//
//   pass 1, per burst : load -> statistics in registers, sync-chunk windows -> LDS (normalised),
//                       sync correlation                              -> corr[q][.]
//   rows              : peak window argmax, early/late bisection (21 taps, early point on lanes
//                       0-7 and late point on lanes 8-15 of the row), interpolated peak power
//                                                                     -> toa, rv per row
//   rows              : sync symbols re-read from L2 / Infinity Cache, chunk sums,
//                       fine frequency error, carrier phase           -> ffe, psi per row
//   pass 2, per burst : 234 symbols re-read (stride sps), soft symbols from the phase in turns,
//                       soft bits by Gray-boundary arithmetic
//   rows              : branch metrics (table words, batched fetches), Viterbi, survivor walk,
//                       CRC (decode4_k5_12)
//
// The second read of a burst happens a few microseconds after the first and is served by the
// L2 / Infinity Cache; it buys back ~650 VALU instructions per burst.
// Single-sequence burst formats only (BCCH, DC6), which is all the fused path handles.
// ---------------------------------------------------------------------------
// rotated reference value of sync symbol n of a format's first training sequence: conj(ref_n) e^{j fs (n' sps)},
// n' = position of the symbol inside its chunk (pi4cxpsk.c:125-171 + the derotation of :539 folded in)
__device__ __forceinline__ float2 sync_coef0(const DevBurst &bt, int n, int sps, float fs)
{
	const int nch = bt.n_chunks[0];
	int ch = 0, base = 0, cum = 0;
	for (int c = 0; c < nch - 1; c++) {
		cum += bt.sync[0][c].len;
		if (n >= cum) { base = cum; ch = c + 1; }
	}
	const int nn = n - base;
	float s, c;
	sincos_fast(fs * (float)(nn * sps), s, c);
	return conj_ref_mul(bt.nbits, bt.sync[0][ch].syms[nn], make_float2(c, s));
}

// the same for symbol n of training sequence sq of a format whose sequences have ONE chunk each (NT3 FACCH)
__device__ __forceinline__ float2 sync_coef_seq1(const DevBurst &bt, int sq, int n, int sps, float fs)
{
	float s, c;
	sincos_fast(fs * (float)(n * sps), s, c);
	return conj_ref_mul(bt.nbits, bt.sync[sq][0].syms[n], make_float2(c, s));
}

// the same for freq_shift = 0, every burst format, sps 1..16: [sps][type][n < 32]
constexpr int kCoef0MaxSps = 16;
__device__ float2 g_coef0[kCoef0MaxSps + 1][kNumTypes][32];
// ... and a copy in the constant address space (made on the device after every k_coef0 run), which a wave-uniform index
// reads with scalar loads -- from the writable array above the compiler issues one vector load per value
__constant__ float2 c_coef0[kCoef0MaxSps + 1][kNumTypes][32];

__global__ __launch_bounds__(64) void k_coef0(int first, int count)
{
	const int type = first + (int)blockIdx.x, sps = (int)blockIdx.y + 1, n = (int)threadIdx.x;
	if (type >= first + count || n >= 32)
		return;
	const DevBurst &bt = c_types[type];
	float2 v = make_float2(0.f, 0.f);
	if (bt.n_sync > 0 && n < bt.sync_tl[0]) {
		const float fs = (0.0f - bt.rotation) / (float)sps;               // pi4cxpsk.c:539 with freq_shift = 0
		v = sync_coef0(bt, n, sps, fs);
	}
	g_coef0[sps][type][n] = v;
}

hipError_t upload_types(const DevBurst *host, int first, int count, hipStream_t stream)
{
	hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_types), host, sizeof(DevBurst) * (size_t)count,
	                                      sizeof(DevBurst) * (size_t)first, hipMemcpyHostToDevice, stream);
	if (e != hipSuccess)
		return e;
	// the zero-shift sync references of the uploaded formats (same stream: ordered before any burst kernel)
	hipLaunchKernelGGL(k_coef0, dim3((unsigned)count, kCoef0MaxSps), dim3(64), 0, stream, first, count);
	e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	void *src = nullptr;
	e = hipGetSymbolAddress(&src, HIP_SYMBOL(g_coef0));
	if (e != hipSuccess)
		return e;
	return hipMemcpyToSymbolAsync(HIP_SYMBOL(c_coef0), src, sizeof(g_coef0), 0, hipMemcpyDeviceToDevice, stream);
}

hipError_t upload_rx4_operands(const Rx4Ord4 *host, hipStream_t stream)
{
	return hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ord4), host, sizeof(Rx4Ord4), 0, hipMemcpyHostToDevice, stream);
}

// Sync correlation of the fused path's two formats with everything static: chunks of T0, T1, T2 training symbols
// (BCCH 11 + 3 + 3, DC6 7 + 3 + 3; nb.c:36-41, 94-99).  The rotated reference values sit in scalar registers, one pair
// (re, im) per tap -- read straight from the table with scalar loads when no frequency shift was given (`ctab`), else
// out of lane n of `cfl` (v_readlane) -- and feed the packed FMAs as scalar operands, so a tap costs one LDS read and two
// v_pk_fma_f32, all reads of a lag issued back to back.  xs: the staged chunk windows, window c = samples
// [pos_c sps, pos_c sps + T_c sps + w - 1).  corr[j] = sum over chunks of |sum_n c_n x[j + n sps]|.  (pk_cmac: fast_math.h)
// (lags [j_begin, j_end) of the w there are; j_end < 0: all)
// (best / best_j, optional: the largest magnitude among this lane's lags and its lag -- rx4_body's QX speculates on it)
template <int SPS, int T0, int T1, int T2>
__device__ __forceinline__ void corr_fixed(const float2 *__restrict__ xs, int sps_rt, int w, int lane,
                                           const float2 *__restrict__ ctab, float2 cfl, float *__restrict__ corr,
                                           int j_begin = 0, int j_end = -1, uint32_t *best = nullptr, int *best_j = nullptr)
{
	constexpr int T[3] = {T0, T1, T2};
	constexpr int NT = T0 + T1 + T2;
	const int sps = SPS ? SPS : sps_rt;
	unsigned long long cf[NT];
	if (ctab) {
		const unsigned long long *__restrict__ ct = reinterpret_cast<const unsigned long long *>(ctab);
#pragma unroll
		for (int n = 0; n < NT; n++)
			cf[n] = ct[n];
	} else {
#pragma unroll
		for (int n = 0; n < NT; n++)
			cf[n] = (unsigned long long)__builtin_bit_cast(uint32_t, lane_val(cfl.x, n)) |
			        ((unsigned long long)__builtin_bit_cast(uint32_t, lane_val(cfl.y, n)) << 32);
	}
	const int j_stop = j_end < 0 ? w : j_end;
	for (int j = j_begin + lane; j < j_stop; j += 64) {
		float cj = 0.f;
		int wb = 0, base = 0;
#pragma unroll
		for (int ch = 0; ch < 3; ch++) {
			const float2 *xp = xs + wb + j;
			v2f acc = {0.f, 0.f};
#pragma unroll
			for (int n = 0; n < T[ch]; n++) {
				const float2 x = xp[n * sps];
				pk_cmac(acc, cf[base + n], (v2f){x.x, x.y});
			}
			base += T[ch];
			wb += T[ch] * sps + w - 1;
			cj += __builtin_amdgcn_sqrtf(fmaf(acc.x, acc.x, acc.y * acc.y));
		}
		corr[j] = cj;
		if (best) {
			// (a sum of square roots is not negative: its bits order like its value)
			const uint32_t cb = __builtin_bit_cast(uint32_t, cj);
			if (cb > *best) { *best = cb; *best_j = j; }
		}
	}
}

struct Lds4 {
	float2 *x;        // normalised sync-chunk windows of the burst being correlated [stage_samples]
	float *corr;      // 4 x cw correlation magnitudes
	float2 *coef;     // 32 rotated sync reference values
	int8_t *eb;       // 4 soft-bit rows
	uint32_t *bm;     // overlays x after pass 1
	uint64_t *surv;
	uint32_t *ubits;
};

// (ebrow, gen only: bytes between the four soft-bit rows -- rx4_body's EBROW)
__host__ __device__ inline size_t lds4_layout(int stage_samples, int cw, size_t *off, bool gen = false, bool ub_over = false,
                                              int ebrow = 432)
{
	// pass 1 keeps only the sync-chunk windows of the burst in LDS (everything else it needs is in
	// registers; pass 2 takes its kept samples out of the window registers -- the fused sps-4 kernel -- or re-reads them).
	// Decode-time data overlays all of it:
	//   [stage | corr 4 x cw | coef]   during pass 1 and the timing rows
	//   [bm | ubits | 4 soft-bit rows / window decisions]   from pass 2 on; during pass 2 itself the soft-bit
	//   table (2 KB, g_sb_lut) sits where the branch metrics will go
	// (the 13 x 64 halfwords of window decisions overlay the soft-bit rows, which are dead once the
	// branch metrics exist)
	// (ub_over, the batch kernel: the decoded words go where the branch metrics were -- all of them are consumed by the time
	// the survivor walk writes -- which brings the headline shape to 5 120 B, the LDS of eight waves per SIMD)
	const size_t dec_bytes = 4 * kSteps12 * 4 + (ub_over ? 0 : 4 * 8 * 4);
	const size_t stage_bytes = align16((size_t)stage_samples * 8);
	const size_t corr_bytes = align16((size_t)4 * cw * 4);
	off[0] = 0;
	off[1] = stage_bytes;
	off[2] = stage_bytes + corr_bytes;
	off[3] = dec_bytes;            // soft-bit rows
	if (gen) {
		// demodulation only (k_rx4g): no layer-1 data; the soft-bit rows overlay the pass-1 data, which is dead by then
		off[3] = 0;
		const size_t p1 = stage_bytes + corr_bytes + 18 * 8;
		const size_t p2 = 4 * (size_t)ebrow + kSbLutBytes;      // pass 2: soft-bit rows, then the soft-bit table
		// the small formats' pass 1 (one burst per row): 4 x 64 staged samples, 4 x <= 128 correlation values, 4 x 16 coefficients
		const size_t p3 = 4 * 64 * 8 + 4 * 128 * 4 + 4 * 16 * 8;
		const size_t m = p1 > p2 ? p1 : p2;
		return align16(m > p3 ? m : p3);
	}
	size_t total = stage_bytes + corr_bytes + 18 * 8;
	if (total < dec_bytes + 4 * 432)
		total = dec_bytes + 4 * 432;
	return align16(total);
}

// samples of the sync-chunk windows a burst type needs staged: sum over chunks of len*sps + w - 1
__host__ __device__ inline int stage_samples_of(const DevBurst &bt, int sps, int in_len)
{
	const int w = in_len - bt.len * sps + 1;
	int n = 0;
	for (int c = 0; c < bt.n_chunks[0]; c++)
		n += bt.sync[0][c].len * sps + w - 1;
	return n;
}

// The body works on bursts g0 .. n_end-1 (at most four) of `a` with one wavefront and its own LDS slice;
// k_rx4 is the batch kernel around it, k_rx_chain (below) the receive loop's feedback chain that calls it round after round.
// per-burst arrays of a launch: the batch kernel takes them from its arguments, the receive loop points them
// at the current round's log blocks (by value: they stay in scalar registers)
#ifdef GMR1_HIP_PROFILE
// cycle stamps of ONE burst of the receive loop (chain 0, the BCCH burst of round kStampRound): tools/loop_stamps.py
__device__ unsigned long long g_stamp[32];
__device__ int g_prof_flag;              // experiments of the profiling build (gmr1_hip_prof_flag)
__device__ int g_prof_miss;              // bursts of k_rx4's QX path whose speculated pick did not hold (gmr1_hip_prof_miss)
constexpr int kStampRound = 55;    // (late in a time slice: its first rounds share the CU with the previous slice's CCCH batch)
#define GMR1_STAMP(k)                                                        \
	do {                                                                    \
		if (LAT && io.stamp && lane == 0)                                   \
			io.stamp[k] = __builtin_readcyclecounter();                     \
	} while (0)
#else
#define GMR1_STAMP(k) do { } while (0)
#endif

struct RxIo {
#ifdef GMR1_HIP_PROFILE
	unsigned long long *stamp;
#endif
	const uint64_t *offset;
	const uint8_t *kind;
	const float *freq_shift;
	uint8_t *l2;
	int32_t *crc, *conv, *rv, *sync_id;
	float *toa, *freq_err, *energy;
	int8_t *ebits;
	float *ssyms;
};

// Burst-format parameters as the body reads them.  GEN (any one format per launch): the descriptor table.  The fused BCCH /
// DC6 path: the two formats' numbers themselves (nb.c:36-62, 94-120) -- one sync chunk of 11 / 7 symbols at 28, two of 3
// at 119 and 197, 234 pi/4-CQPSK symbols --, so that no phase waits for a table entry (a per-row descriptor lookup is a
// vector load from constant memory: three dependent ones sat in front of the sync-symbol terms); the host refuses to start
// the fused kernels unless the tables say exactly this (fused_formats_match, rx_select.h).
constexpr unsigned long long kFusedSymsBcch =      // [0 2 2 0 0 0 2 0 2 2 2 | 2 2 0 | 2 2 0], two bits each, first symbol lowest
	0ull | 2ull << 2 | 2ull << 4 | 0ull << 6 | 0ull << 8 | 0ull << 10 | 2ull << 12 | 0ull << 14 | 2ull << 16 | 2ull << 18 | 2ull << 20 |
	2ull << 22 | 2ull << 24 | 0ull << 26 | 2ull << 28 | 2ull << 30 | 0ull << 32;
constexpr unsigned long long kFusedSymsDc6 =       // [0 0 0 2 2 0 2 | 0 3 0 | 3 1 1]
	0ull | 0ull << 2 | 0ull << 4 | 2ull << 6 | 2ull << 8 | 0ull << 10 | 2ull << 12 |
	0ull << 14 | 3ull << 16 | 0ull << 18 | 3ull << 20 | 1ull << 22 | 1ull << 24;
template <bool GEN>
struct Fmt {
	static __device__ __forceinline__ int len(const DevBurst &b) { return GEN ? b.len : 234; }
	static __device__ __forceinline__ int nbits(const DevBurst &b) { return GEN ? b.nbits : 2; }
	static __device__ __forceinline__ float rotation(const DevBurst &b) { return GEN ? b.rotation : kPif / 4.0f; }
	static __device__ __forceinline__ int tl(const DevBurst &b, int kind) { return GEN ? b.sync_tl[0] : (kind ? 13 : 17); }
	static __device__ __forceinline__ int nch(const DevBurst &b) { return GEN ? b.n_chunks[0] : 3; }
	static __device__ __forceinline__ int clen(const DevBurst &b, int kind, int c) { return GEN ? b.sync[0][c].len : (c == 0 ? (kind ? 7 : 11) : 3); }
	static __device__ __forceinline__ int cpos(const DevBurst &b, int c) { return GEN ? b.sync[0][c].pos : (c == 0 ? 28 : (c == 1 ? 119 : 197)); }
	// training symbol n (counted through the chunks) of the first sequence; GEN: symbol nn of chunk ch of sequence sq
	static __device__ __forceinline__ int sym(const DevBurst &b, int kind, int sq, int ch, int nn, int n)
	{
		if constexpr (GEN)
			return b.sync[sq][ch].syms[nn];
		else
			return (int)(((kind ? kFusedSymsDc6 : kFusedSymsBcch) >> (2 * n)) & 3ull);
	}
};

// What the receive loop hands its burst body (LAT).
// (1) What depends only on WHERE the burst sits -- the window's mean and deviation, its energy, the normalised samples under
// the sync chunks -- prepared a round ahead by the chain's second wave (lat_prepare, on another SIMD) for the place the
// chain's schedule puts the next BCCH burst, eight frames on; a burst that turns out to sit elsewhere (the feedback moved
// the chain) is prepared by the body itself, as every burst of the batch kernels is.
// (2) What every burst reads from constant tables, kept where a wave of the loop gets at it in an LDS access instead of a
// trip to the L2 (each of these sat at the head of a phase of every burst of every round): the soft-bit table, the
// trellis-step descriptors and the cost words of the branch metrics (work-group copies), the decoder's per-lane
// constants and CRC syndrome words (registers).
struct LoopCo {                    // front wave <-> helper wave, within a tick (flags carry the tick's job id)
	int job;                       // F -> S, before the tick's barrier: id (> 0) of the job, 0: none
	float fsh;                     // the burst: frequency shift ...
	uint64_t off;                  // ... and first sample (S helps only if that is the window prepared)
	int p_id, p;                   // F -> S: the coarse peak (p < 0: never mind)
	int p_pred;                    // F -> S with the job: where the peak is expected (e_toa) -- S works that case out ahead
	int c_id;                      // S -> F: the correlation's tail is in place
	int s_id;                      // S -> F: ffe / psi of the three candidates are in place
	float ffe[3], psi[3];
	float tail[64];                // the correlation of the last partial round of lags (F copies it in: a front that was
	                               // squashed meanwhile never looks at it)
};

template <int NPL, int SPS>
struct LatPre {
	const uint64_t *h_off = nullptr;       // LDS: first sample of the window prepared (~0: none)
	const int *h_kind = nullptr;
	const float *h_stat = nullptr;         // LDS: mean re, mean im, 1 / deviation, burst energy
	const float2 *h_x = nullptr;           // LDS: the staged sync-chunk windows
	const unsigned char *lut = nullptr;
	const uint32_t *steps = nullptr;       // [2][kSteps12]
	const uint32_t *cost_a = nullptr, *cost_b = nullptr;   // [512] each
	uint32_t *vtab = nullptr;              // LDS: the decoder's per-step operand table (decode1_k5_12_lat), kLatTabBytes
	uint32_t dc = 0;
	uint4 sy0, sy1;
	// (3) The pipelined loop (k_rx_chain_pipe, PART): the burst is cut where its feedback exists -- after the sync-symbol
	// terms (pi4cxpsk.c:547-575: toa, freq_err) --, the FRONT on one wave, the rest (soft bits, layer 1) on others, rounds
	// later.  What crosses the cut: `cut`; the burst's raw window stays in LDS for the kept samples of pass 2.
	struct Cut { int found, d, sid; float toa, ffe, psi, avr, avi; };
	Cut *cut = nullptr;                    // LDS
	Cut out;                               // front: the same in (scalar) registers, for the walk
	float out_energy = 0.f;                // front: burst_energy() of the window
	// (4) The front's helper wave (k_rx_chain_pipe's S): for a burst whose window was prepared it correlates the last
	// partial round of lags while the front wave does the whole rounds, and, once the front has posted the coarse peak p,
	// forms the sync-symbol terms for the three values round(toa) can take (p - 1, p, p + 1: the bisection starts at p - 1
	// and moves less than one lag) while the front wave bisects.
	LoopCo *co = nullptr;                  // LDS; null: the front works alone
	int co_id = 0;
	// (5) PART 1 / 2: the one burst's operands in registers of the caller (a BCCH burst) -- not through the arrays of `io`,
	// whose every read would be an LDS round trip in front of the phase that needs it
	uint64_t b_off = 0;
	float b_fsh = 0.f;
	float2 *win_w = nullptr;               // LDS, front half: where the window goes if the front had to fetch it itself
	const float2 *win_r = nullptr;         // LDS, back half: the burst's raw window (lane l's samples l + 64 k as fetched)
};

// rotated reference of a fused format's training sequence under a caller-supplied frequency shift: value n in lane n
__device__ __forceinline__ float2 lat_coef(int kind, int lane, float fs, int sps)
{
	float2 cfl = make_float2(0.f, 0.f);
	if (lane < (kind ? 13 : 17)) {
		const int l0 = kind ? 7 : 11;
		const int nn = lane < l0 ? lane : (lane < l0 + 3 ? lane - l0 : lane - l0 - 3);
		float sn, cs;
		sincos_fast(fs * (float)(nn * sps), sn, cs);
		cfl = conj_ref_mul(2, (int)(((kind ? kFusedSymsDc6 : kFusedSymsBcch) >> (2 * lane)) & 3ull), make_float2(cs, sn));
	}
	return cfl;
}

// The sync-symbol terms of a fused-format burst whose sync-chunk windows are staged in LDS (the receive loop's bursts): fine
// frequency from the chunk sums, then the carrier phase (pi4cxpsk.c:381-433, 574-575) -- one burst, or one candidate
// timing d of a burst, per 16-lane row; lane col holds sync symbols n = col and n = col + 16.  The window scale 1 / sigma
// is irrelevant to every angle.
__device__ __forceinline__ void lat_sync_terms(const float2 *__restrict__ xst, int kind, int d, bool live, float fs, int sps, int w,
                                               int in_len, int col, float &ffe_o, float &psi_o)
{
	typedef Fmt<false> F;
	const DevBurst &bt = c_types[GMR1_HIP_BCCH];      // (Fmt<false> carries the numbers itself)
	const int tl = F::tl(bt, kind);
	float2 t0[2], xr[2];
	int chn[2], spos[2], idxv[2];
#pragma unroll
	for (int h = 0; h < 2; h++) {
		const int n = col + 16 * h;
		t0[h] = xr[h] = make_float2(0.f, 0.f);
		chn[h] = -1;
		spos[h] = idxv[h] = 0;
		if (n < tl && live) {
			int ch = 0, base = 0, cum = 0, wb = 0;
			for (int c = 0; c < 2; c++) {
				cum += F::clen(bt, kind, c);
				if (n >= cum) { base = cum; ch = c + 1; wb += F::clen(bt, kind, c) * sps + w - 1; }
			}
			const int nn = n - base;
			const int sp = F::cpos(bt, ch) + nn;
			const int idx = sp * sps + d;
			if (idx >= 0 && idx < in_len)
				xr[h] = xst[wb + nn * sps + d];
			chn[h] = ch;
			spos[h] = sp;
			idxv[h] = idx;
		}
	}
#pragma unroll
	for (int h = 0; h < 2; h++) {
		if (chn[h] >= 0) {
			float sn, cs;
			sincos_fast(fs * (float)idxv[h], sn, cs);
			const float2 x = cmul(xr[h], make_float2(cs, sn));
			t0[h] = conj_ref_mul(2, F::sym(bt, kind, 0, 0, 0, col + 16 * h), x);
		}
	}
	float ffe = 0.f;
	{
		float sumr[3], sumi[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const float pr = (chn[0] == c ? t0[0].x : 0.f) + (chn[1] == c ? t0[1].x : 0.f);
			const float pi = (chn[0] == c ? t0[0].y : 0.f) + (chn[1] == c ? t0[1].y : 0.f);
			sumr[c] = row_sum(pr);
			sumi[c] = row_sum(pi);
		}
		float f = 0.f;
#pragma unroll
		for (int i = 1; i < 3; i++) {
			const float ppos = (float)F::cpos(bt, i - 1) + (float)F::clen(bt, kind, i - 1) / 2.0f;
			const float cpos = (float)F::cpos(bt, i) + (float)F::clen(bt, kind, i) / 2.0f;
			const float re = sumr[i] * sumr[i - 1] - sumi[i] * (-sumi[i - 1]);
			const float im = sumr[i] * (-sumi[i - 1]) + sumi[i] * sumr[i - 1];
			f += atan2_fast(im, re) / (cpos - ppos);
		}
		ffe = f / (float)(3 - 1);
	}
	float tr = 0.f, ti = 0.f;
#pragma unroll
	for (int h = 0; h < 2; h++) {
		float2 tt = t0[h];
		if (ffe != 0.0f) {
			float sn, cs;
			sincos_fast(-ffe * (float)spos[h], sn, cs);
			tt = cmul(tt, make_float2(cs, sn));
		}
		tr += tt.x;
		ti += tt.y;
	}
	ffe_o = ffe;
	psi_o = atan2_fast(row_sum(ti), row_sum(tr));
}

// What the front's helper wave does for one BCCH burst of the loop whose window was prepared (LatPre (4)).
template <int SPS>
__device__ __forceinline__ void loop_front_helper_corr(const RxArgs &a, LoopCo *co, int id, const float2 *__restrict__ xst, int lane)
{
	const int sps = SPS ? SPS : a.sps;
	const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[0]);
	const int w = in_len - 234 * sps + 1;
	const float fs = (co->fsh - kPif / 4.0f) / (float)sps;              // as rx4_body: (shift - rotation) / sps
	const float2 cfl = lat_coef(0, lane, fs, sps);
	const int j0 = ((w - 1) >> 6) << 6;                                 // the last, partial round of lags
	corr_fixed<SPS, 11, 3, 3>(xst, sps, w, lane, nullptr, cfl, co->tail - j0, j0, w);
	WSYNC();
	if (lane == 0)
		lds_post(&co->c_id, id);
}
// the sync-symbol terms of the three timing candidates p - 1, p, p + 1 -> co->ffe / psi
template <int SPS>
__device__ __forceinline__ void loop_front_helper_sync(const RxArgs &a, LoopCo *co, const float2 *__restrict__ xst, int lane, int p)
{
	const int sps = SPS ? SPS : a.sps;
	const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[0]);
	const int w = in_len - 234 * sps + 1;
	const float fs = (co->fsh - kPif / 4.0f) / (float)sps;
	const int row = lane >> 4, col = lane & 15;
	float ffe, psi;
	lat_sync_terms(xst, 0, p - 1 + row, row < 3, fs, sps, w, in_len, col, ffe, psi);
	if (col == 0 && row < 3) {
		co->ffe[row] = ffe;
		co->psi[row] = psi;
	}
	WSYNC();
}

// The position-only part of a fused-format burst's pass 1 (rx4_body does the same, operation for operation): window,
// statistics, burst energy, normalised sync-chunk windows.
template <int NPL, int SPS>
__device__ __forceinline__ void lat_prepare(const RxArgs &a, uint64_t off, int kind, int lane, float2 *__restrict__ hx,
                                            float *__restrict__ hs, float2 *__restrict__ win = nullptr)
{
	const int sps = SPS ? SPS : a.sps;
	const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[kind]);
	typedef Fmt<false> F;
	const DevBurst &bt = c_types[kind ? GMR1_HIP_DC6 : GMR1_HIP_BCCH];
	const int w = in_len - 234 * sps + 1;
	const float2 *__restrict__ in = a.iq + off;
	constexpr int NFULL = (SPS == 4 && NPL == 16) ? 15 : -1;
	constexpr int SIT = SPS == 4 ? 2 : 4;
	float2 wv[NPL];
	float2 sv[3][SIT];
	window_fetch<NPL, NFULL>(in, in_len, lane, wv);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const int wl = F::clen(bt, kind, c) * sps + w - 1;
		const float2 *__restrict__ src = in + F::cpos(bt, c) * sps;
#pragma unroll
		for (int h = 0; h < SIT; h++) {
			const int sidx = lane + 64 * h;
			sv[c][h] = sidx < wl ? src[sidx] : make_float2(0.f, 0.f);
		}
	}
	if (win) {
		// the whole raw window, as fetched (lane l's samples l + 64 k): the back half of the burst takes its kept samples here
#pragma unroll
		for (int k = 0; k < NPL; k++)
			win[lane + 64 * k] = wv[k];
	}
	float avr, avi, inv;
	window_stats<NPL, NFULL>(wv, in_len, lane, avr, avi, inv);
	const float e = window_energy_regs<NPL>(wv, in_len, lane);
	int wb = 0;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const int wl = F::clen(bt, kind, c) * sps + w - 1;
#pragma unroll
		for (int h = 0; h < SIT; h++) {
			const int sidx = lane + 64 * h;
			if (sidx < wl) {
				const v2f nv = ((v2f){sv[c][h].x, sv[c][h].y} - (v2f){avr, avi}) * (v2f){inv, inv};
				hx[wb + sidx] = make_float2(nv.x, nv.y);
			}
		}
		wb += wl;
	}
	if (lane == 0) {
		hs[0] = avr;
		hs[1] = avi;
		hs[2] = inv;
		hs[3] = e;
	}
}

// The burst body's configuration: a type with these members; the kernels name theirs below, Rx4Cfg holds the defaults.
// LAT: the caller cares about the latency of ONE burst (the receive loop), not about throughput
// GEN: demodulation only, every burst of the one format a.fixed_type (one training sequence, QPSK, <= 3 sync chunks,
// <= 18 sync symbols, <= 256 symbols: NT3 speech, DC2, BCCH, DC6) -- the batch form of gmr1_pi4cxpsk_demod for large n
// FAC (with GEN, NPL = 8): a format with TWO training sequences of one chunk each at the same place, BPSK - NT3 FACCH.
// Both sequences are correlated over the one staged window; the second is ranked and timed on the SUM of both
// correlations, as the reference's uncleared accumulator has it (pi4cxpsk.c:207-237); the timing rows run once per
// sequence; `cw` holds both correlation arrays of a burst (first cw / 2 lags: sequence 0, then the sum).
// EN (fused batch kernel only): the caller wants burst_energy() of every window (RxArgs::energy; the receive loop's CCCH batch).
// A template parameter because keeping the window registers alive for it costs the headline instantiation its sixth wave
// (80 VGPRs with 2 spilled against 78 with none: 0.257 -> 0.265 ms per 100 k bursts, and the spill stores tripled the kernel's
// write traffic -- which is how it was found).
// PL (fused batch kernel at 4 samples per symbol only): the sample array is stored POLYPHASE-PLANAR -- sample s of the flat
// array sits at iq[(s & 3) * plane_stride + (s >> 2)] (include/gmr1_hip.h, gmr1_hip_rx_bcch_ccch_batch_planar_dev).  Only
// addresses change: the window sits in registers in the same QUAD layout as the interleaved call's (lane l holds samples
// 256 b + 4 l + c: place l + 64 b of plane c, a coalesced 512-byte load), so every sum is formed over the same samples in the
// same order and every result is bit-identical; pass 2's 234 samples at stride 4 from sample d (pi4cxpsk.c:292-295) are 234
// CONSECUTIVE samples of plane (offset + d) & 3 -- 15 lines of 128 bytes instead of every line of the window.
// EBROW (GEN only): bytes between the four bursts' soft-bit rows in LDS.  432 holds any format; the kernel that decodes NT3
// speech bursts right behind the demodulator (k_rx4g_tch3) packs its 212-byte rows at 216 to leave the decoder its tables.
// PART (LAT only): 0 the whole burst; 1 its front -- pass 1, timing, sync-symbol terms; rv / toa / freq_err / energy to
// `io`, the rest of what the middle needs to pre->cut --; 2 its middle -- pass 2 out of pre->win_r, then the decoder's
// operand table into pre->vtab; the decoder itself is the caller's third stage (see LatPre (3))
struct Rx4Cfg {
	static constexpr int NPL = 16, SPS = 4;            // window samples per lane / 64; samples per symbol (0: a.sps at run time)
	static constexpr bool LAT = false, GEN = false, FAC = false, ACC = false, EN = true, PL = false;
	static constexpr int EBROW = 432, PART = 0;
	static constexpr bool EARLY = false;               // the batch kernel asks early for what its bursts need (Rx4Switches)
};
// the fused batch kernel (k_rx4; k_one_server runs the same body on one burst)
template <int NPL_, int SPS_, bool ACC_, bool EN_, bool PL_ = false, bool EARLY_ = false>
struct CfgBatch : Rx4Cfg {
	static constexpr int NPL = NPL_, SPS = SPS_;
	static constexpr bool ACC = ACC_, EN = EN_, PL = PL_, EARLY = EARLY_;
};
// demodulation only (k_rx4g): generic, small (NPL 8) and two-sequence (FAC) forms
template <int NPL_, int SPS_, bool FAC_>
struct CfgDemod : Rx4Cfg {
	static constexpr int NPL = NPL_, SPS = SPS_;
	static constexpr bool GEN = true, FAC = FAC_;
};
// the small demodulator in front of the TCH3 decoder (k_rx4g_tch3): soft-bit rows packed at 216 bytes
struct CfgTch3Front : Rx4Cfg {
	static constexpr int NPL = 8, SPS = 4, EBROW = 216;
	static constexpr bool GEN = true;
};
// the receive loop's BCCH burst: whole (PART 0, k_rx_chain) or one pipeline stage of it (k_rx_chain_pipe)
template <int NPL_, int SPS_, bool ACC_, int PART_ = 0>
struct CfgLoop : Rx4Cfg {
	static constexpr int NPL = NPL_, SPS = SPS_, PART = PART_;
	static constexpr bool LAT = true, ACC = ACC_;
};

// experiment on the headline instantiation (build.py --variant): GMR1_EXP_RX4_TOUCH 1 / 2 -- a wave touches its next burst's
// window (window_touch_q) right behind this burst's requests / behind its statistics.  Measured: 4 % and 3 % SLOWER than
// without (profiles/r07a_ab_rx4_waits.txt), so the product is built without (0).
#ifndef GMR1_EXP_RX4_TOUCH
#define GMR1_EXP_RX4_TOUCH 0
#endif

// what follows from a configuration P
template <class P>
struct Rx4Switches : P {
	// the small generic variant (NPL = 8; the host launches it for formats of <= 128 symbols with one sync chunk of
	// <= 16 symbols whose window is <= 64 samples: NT3 speech, DC2) drops the unrolled work the long bursts need
	static constexpr bool SMALL = P::GEN && P::NPL == 8;
	static_assert(!P::FAC || SMALL, "the two-sequence variant builds on the small generic one");
	static_assert(!P::PL || (P::SPS == 4 && !P::GEN && !P::LAT && !P::EN), "the planar layout exists for the fused batch kernel at sps 4");
	static_assert(P::PART == 0 || P::LAT, "only the receive loop's burst is cut in two");
	// The next burst's window in flight during this burst's correlation costs 32 registers at the body's peak.  The fused
	// kernel does without: 78 instead of 87 VGPRs is the step from five to six waves per SIMD, and the sixth wave hides more
	// latency than the prefetch did (0.288 -> 0.274 ms per 100 k bursts).  The other instantiations keep it.
	static constexpr bool PREFETCH_NEXT = P::GEN || P::LAT;
	static constexpr int NSYM = SMALL ? 2 : 4;               // 64-symbol pieces of a burst
	static constexpr int NCHK = SMALL ? 1 : 3;               // sync chunks
	static constexpr int NSH = SMALL ? 1 : 2;                // 16-symbol pieces of the sync sequence
	static constexpr bool UB_OVER = !P::LAT && !P::GEN;         // the decoded words go where the branch metrics were (lds4_layout)
	// QL (the fused batch kernel at 4 samples per symbol, both sample layouts): the window sits in registers in the QUAD layout
	// (window_fetch_q).  QX (interleaved samples): pass 2's kept samples never make a second trip to memory.  Right behind a
	// burst's correlation its pick d = round(toa) is SPECULATED as the lag of the largest correlation magnitude (the timing
	// rows below start their early / late walk on the strongest lag p of the best three-lag window and end within a lag of it,
	// pi4cxpsk.c:240, so round(toa) is p - 1, p or p + 1, and p is the largest magnitude itself whenever the peak is clean);
	// the 234 kept samples d + 4 i are then one sub-slot of every lane of the window registers, a lane rotation away from
	// pass 2's assignment, and what pass 2 takes from a kept sample -- its phase -- is formed on the spot: four registers a
	// burst instead of a window.  The timing rows then compute the pick as ever; a burst whose pick is NOT the speculated one
	// (a few per cent: noise decides where toa lies half-way between two samples) takes the old route -- kept samples and sync
	// symbols re-read from memory, the same operations on the same numbers -- so no output depends on the speculation.
	static constexpr bool QL = !P::GEN && !P::LAT && !P::EN && P::SPS == 4 && P::NPL == 16;
	static constexpr bool QX = QL && !P::PL;
	static_assert(!P::PL || QL, "the planar layout exists for the fused batch kernel");
	// EARLY (the batch kernel, interleaved samples): what a wave's bursts need from memory before their windows can be asked
	// for is asked for once, ahead of the first window (AHEAD); the rows behind pass 1 take their burst's kind / offset /
	// frequency shift from those scalars (H_ROW); and a window's ragged last quarter no longer holds its loads back (ONE_LOAD)
	static constexpr bool AHEAD = P::EARLY && QX;
	static constexpr int TOUCH = AHEAD ? GMR1_EXP_RX4_TOUCH : 0;
	static constexpr bool H_ROW = AHEAD, ONE_LOAD = AHEAD;
	// OPS_AHEAD (with AHEAD, whose scalars name each burst's kind): what pass 2, the branch metrics and the decoder read per
	// lane that is fixed for the launch goes out in batches, ahead of the waits it used to stand behind.  Where the lane's
	// four symbols' soft bits go (g_ord4, one 8-byte load a burst) is asked for with the soft-bit table's two loads, right
	// behind the sync rows: one memory trip where pass 2 made one per burst.  The lane's step descriptors (g_steps4, one
	// 16-byte load a chain) go out inside the pass-2 loop (kRx4StepsAt), the decoder's constants in front of the branch
	// metrics' gathers.  The other instantiations read c_types' ord_of_sym, c_steps and the constants where they always did
	// (profiles/r14a_rx4_waits_behind_pass1.txt has both lists of waits).
	static constexpr bool OPS_AHEAD = AHEAD;
};

// OPS_AHEAD: the pass-2 iteration (bursts run 3, 2, 1, 0) at whose head the step descriptors are asked for
constexpr int kRx4StepsAt = 1;

template <class Cfg>
__device__ __forceinline__ void rx4_body(const RxArgs &a, const RxIo io, int stage_samples, int cw, int g0, int n_end,
                                         unsigned char *__restrict__ lds_raw, int lane, LatPre<Cfg::NPL, Cfg::SPS> *pre = nullptr)
{
	typedef Rx4Switches<Cfg> C;
	constexpr int NPL = C::NPL, SPS = C::SPS, EBROW = C::EBROW, PART = C::PART;
	constexpr bool LAT = C::LAT, GEN = C::GEN, FAC = C::FAC, ACC = C::ACC, EN = C::EN, PL = C::PL;
	constexpr bool SMALL = C::SMALL, QL = C::QL, QX = C::QX, PREFETCH_NEXT = C::PREFETCH_NEXT, UB_OVER = C::UB_OVER;
	constexpr int NSYM = C::NSYM, NCHK = C::NCHK, NSH = C::NSH;
	constexpr int TOUCH = C::TOUCH;
	constexpr bool AHEAD = C::AHEAD, H_ROW = C::H_ROW, OPS_AHEAD = C::OPS_AHEAD;
	const int row = lane >> 4, col = lane & 15;
	const int sps = SPS ? SPS : a.sps;
	const int cwh = FAC ? cw / 2 : cw;                // lags per correlation array
	size_t off[4];
	lds4_layout(stage_samples, cw, off, GEN, UB_OVER, EBROW);
	Lds4 L;
	L.x = reinterpret_cast<float2 *>(lds_raw + off[0]);
	L.corr = reinterpret_cast<float *>(lds_raw + off[1]);
	L.coef = reinterpret_cast<float2 *>(lds_raw + off[2]);
	L.eb = reinterpret_cast<int8_t *>(lds_raw + off[3]);
	L.bm = reinterpret_cast<uint32_t *>(lds_raw + off[0]);
	L.surv = reinterpret_cast<uint64_t *>(lds_raw + off[3]);
	L.ubits = reinterpret_cast<uint32_t *>(lds_raw + off[0] + (UB_OVER ? 0 : 4 * kSteps12 * 4));

	const int g_row = g0 + row;                       // this row's burst
	const bool row_live = g_row < n_end;

	float avr_r = 0.f, avi_r = 0.f;                    // window mean of this row's burst
	const float2 *xst_lat = L.x;                       // LAT: where the one burst's sync-chunk windows are staged

	float th_q[QX ? 4 : 1][4];                         // QX: phase (turns) of kept sample lane + 64 r of burst q
	uint32_t zm_q = 0xff000000u;                       // bit 4 q + r: that sample counts as 0 + 0j (outside the window, or zero);
	                                                   // bits 24-31 (row q's lanes): burst q's speculated pick (0 ... 80; 255: none)
	float2 xs_q[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};   // row q: normalised samples of sync symbols col, col + 16 at the speculated pick
	float inv_r = 1.0f;                                // row q: 1 / sigma of burst q's window
	// a burst's operands: the arrays of `io`, or (the loop's pipeline stages) the caller's registers (LatPre (5))
	auto op_kind = [&](int g) -> int {
		if constexpr (LAT && PART != 0) return 0; else return io.kind[g] ? 1 : 0;
	};
	auto op_fsh = [&](int g) -> float {
		if constexpr (LAT && PART != 0) return pre->b_fsh; else return io.freq_shift ? io.freq_shift[g] : 0.0f;
	};
	auto op_off = [&](int g) -> uint64_t {
		if constexpr (LAT && PART != 0) return pre->b_off; else return io.offset[g];
	};
	// AHEAD: the four bursts' kind, offset and frequency shift, asked for together before the first window (one trip to
	// the L2 a wave instead of three in a row a burst) and kept in scalars; a burst the wave does not have shadows its first
	int kind_s[4] = {0, 0, 0, 0};
	uint64_t off_s[4] = {0, 0, 0, 0};
	float fsh_s[4] = {0.f, 0.f, 0.f, 0.f};
	if constexpr (AHEAD) {
		if (g0 < n_end) {
			int kv[4];
			uint64_t ov[4];
			float fv[4];
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const int gq = g0 + q < n_end ? g0 + q : g0;
				kv[q] = op_kind(gq);
				ov[q] = op_off(gq);
				fv[q] = op_fsh(gq);
			}
#pragma unroll
			for (int q = 0; q < 4; q++) {
				kind_s[q] = __builtin_amdgcn_readfirstlane(kv[q]);
				off_s[q] = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ov[q]) |
				           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ov[q] >> 32)) << 32);
				fsh_s[q] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fv[q])));
			}
		}
	}
	float2 wv_own[NPL];
	bool co_on = false;                                // (LAT, PART 1) the helper wave shares this burst's front (LatPre (4))
	int co_p = 0;
	if constexpr (PART == 2)
		GMR1_STAMP(14);
	else
		GMR1_STAMP(0);
	// =========================== pass 1: correlation magnitudes ===========================
	if constexpr (PART != 2) {
	if constexpr (SMALL) {
		// The short formats (<= 512 samples, one sync chunk of <= 16 symbols, <= 64 lags) take pass 1 with ONE BURST PER ROW
		// as well: lane `col` of a row reads samples col, col + 16, ... of the row's burst (16 lanes x 8 B = one 128-byte
		// line per row and load), so window sums, the division, the rotated reference, the staged sync window and the
		// correlation are formed once per wave for its four bursts instead of once per burst with the other rows' lanes
		// idle or duplicating.
		const DevBurst &bt = c_types[a.fixed_type];
		const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[0]);
		const int w = in_len - bt.len * sps + 1;
		const int tl = bt.sync_tl[0];
		const int len0 = bt.sync[0][0].len;
		const int wl = len0 * sps + w - 1;                 // samples under the sync chunk for every lag (<= 64)
		const int gq = row_live ? g_row : g0;              // a dead row shadows the wave's first burst
		const float2 *__restrict__ in = a.iq + io.offset[gq];
		const float fsh = io.freq_shift ? io.freq_shift[gq] : 0.0f;
		const float fs = (fsh - bt.rotation) / (float)sps;
		float2 *xs = reinterpret_cast<float2 *>(lds_raw) + row * 64;
		L.corr = reinterpret_cast<float *>(lds_raw + 2048);
		float2 *coef = reinterpret_cast<float2 *>(lds_raw + 4096) + row * 16;
		// what needs memory is asked for first: the samples under the sync chunk ...
		float2 sv[4];
		{
			const float2 *__restrict__ src = in + bt.sync[0][0].pos * sps;
#pragma unroll
			for (int h = 0; h < 4; h++) {
				const int sidx = col + 16 * h;
				sv[h] = sidx < wl ? src[sidx] : make_float2(0.f, 0.f);
			}
		}
		// ... and the whole window, ONE sweep: sum x and sum |x|^2 (a second sweep for the variance about the mean would
		// be a third trip through the memory system for a kernel whose two -- this one and pass 2's -- already load it
		// fully; sigma only sets a scale nothing downstream depends on)
		const int nit = in_len >> 4, rem = in_len & 15;
		const bool want_en = io.energy != nullptr;
		v2f s2 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll 8
		for (int t = 0; t < nit; t++) {
			const float2 x = in[col + 16 * t];
			s2 += (v2f){x.x, x.y};
			q2 = __builtin_elementwise_fma((v2f){x.x, x.y}, (v2f){x.x, x.y}, q2);
		}
		if (col < rem) {
			const float2 x = in[col + 16 * nit];
			s2 += (v2f){x.x, x.y};
			q2 = __builtin_elementwise_fma((v2f){x.x, x.y}, (v2f){x.x, x.y}, q2);
		}
		float en = 0.f;
		if (want_en) {
			// burst_energy() (gmr1_rx.c:172-182): the inner 30 / 32 of the raw window, served by the caches
			const int bd = in_len >> 5;
			for (int idx = col; idx < in_len; idx += 16)
				if (idx >= bd && idx < in_len - bd) {
					const float2 x = in[idx];
					en = fmaf(x.x, x.x, fmaf(x.y, x.y, en));
				}
		}
		// rotated reference of the training sequence(s), one value per lane of the row, while the samples travel
		if constexpr (FAC) {
			if (col < 2 * tl)
				coef[col] = sync_coef_seq1(bt, col >= tl ? 1 : 0, col >= tl ? col - tl : col, sps, fs);
		} else {
			float2 cfl = make_float2(0.f, 0.f);
			if (io.freq_shift == nullptr)
				cfl = g_coef0[sps][a.fixed_type][col];
			else if (col < tl)
				cfl = sync_coef0(bt, col, sps, fs);
			coef[col] = cfl;
		}
		const float inv_n = __builtin_amdgcn_rcpf((float)in_len);
		const float avr = row_sum(s2.x) / (float)in_len, avi = row_sum(s2.y) / (float)in_len;     // true division, see load_normalise
		const v2f av = {avr, avi};
		// sum |x - m|^2 = sum |x|^2 - n |m|^2 (never below zero)
		const float var = fmaxf(fmaf(-(float)in_len, fmaf(avr, avr, avi * avi), row_sum(q2.x + q2.y)), 0.0f) * inv_n;
		float stddev = __builtin_amdgcn_sqrtf(var);
		if (stddev == 0.0f)
			stddev = 1.0f;
		const float inv = __builtin_amdgcn_rcpf(stddev);
		avr_r = avr;
		avi_r = avi;
		if (want_en) {
			const float e = row_sum(en) / (float)in_len;
			if (col == 0 && row_live)
				io.energy[g_row] = e;
		}
#pragma unroll
		for (int h = 0; h < 4; h++) {
			const int sidx = col + 16 * h;
			if (sidx < wl) {
				const v2f nv = ((v2f){sv[h].x, sv[h].y} - av) * (v2f){inv, inv};
				xs[sidx] = make_float2(nv.x, nv.y);
			}
		}
		WSYNC();
		float *corr = L.corr + row * cw;
		for (int j = col; j < w; j += 16) {
			const float2 *xp = xs + j;
			v2f acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
			for (int n = 0; n < len0; n++) {
				const float2 x = xp[n * sps];
				const float2 c0 = coef[n];
				acc0 = __builtin_elementwise_fma((v2f){-c0.y, c0.y}, (v2f){x.y, x.x}, acc0);
				acc0 = __builtin_elementwise_fma((v2f){c0.x, c0.x}, (v2f){x.x, x.y}, acc0);
				if constexpr (FAC) {
					const float2 c1 = coef[tl + n];
					acc1 = __builtin_elementwise_fma((v2f){-c1.y, c1.y}, (v2f){x.y, x.x}, acc1);
					acc1 = __builtin_elementwise_fma((v2f){c1.x, c1.x}, (v2f){x.x, x.y}, acc1);
				}
			}
			float cj = 0.f;
			cj += sqrtf(fmaf(acc0.x, acc0.x, acc0.y * acc0.y));
			corr[j] = cj;                                   // FAC: sequence 0
			if constexpr (FAC) {
				cj += sqrtf(fmaf(acc1.x, acc1.x, acc1.y * acc1.y));
				corr[cwh + j] = cj;                         // what sequence 1 is ranked and timed on
			}
		}
	} else {
	float2 (&wv)[NPL] = wv_own;
	const int lane_outer = lane;
	// QX: where, in the staged sync-chunk windows of a BCCH / of a DC6 burst, the sample under sync symbol `col` lies for pick 0
	// (chunk c's window starts at staged sample wb_c; symbol nn of it, at pick d, is staged sample wb_c + 4 nn + d); -1: none
	int xsp_bc = 0xffff;                               // (the two places in one register, a byte each; 255: none)
	if constexpr (QX) {
		auto place = [&](int kind) -> int {
			const int w = a.in_len[kind] - 234 * 4 + 1;
			const int c0 = kind ? 7 : 11;
			const int n = col;
			const int ch = n < c0 ? 0 : (n < c0 + 3 ? 1 : 2);
			const int nn = n - (ch == 0 ? 0 : (ch == 1 ? c0 : c0 + 3));
			const int wb = ch == 0 ? 0 : (ch == 1 ? c0 * 4 + w - 1 : c0 * 4 + w - 1 + 3 * 4 + w - 1);
			return n < c0 + 6 ? wb + nn * 4 : -1;
		};
		xsp_bc = (place(0) & 0xff) | ((place(1) & 0xff) << 8);      // (places are below 240)
	}
	// (QX: unrolled, the bursts' phase registers th_q[q] are picked at compile time and come to life one burst at a time)
#pragma clang loop unroll_count(QX ? 4 : 1)
	for (int q = 0; q < 4; q++) {
		const int g = g0 + q;
		if (g >= n_end)
			break;
		// (QX: the lane number is made opaque once per iteration, so that nothing derived from it -- addresses, staging
		// predicates, tap places -- is hoisted out of the loop to sit in registers beside the bursts' kept phases)
		int lane_l = lane_outer;
		if constexpr (QX)
			asm volatile("" : "+v"(lane_l));
		const int lane = lane_l;
		const int row = lane >> 4, col = lane & 15;
		const bool has_nx = TOUCH != 0 && window_touch_wanted(q, g, n_end);
		int kind_l;
		if constexpr (AHEAD)
			kind_l = kind_s[q];
		else
			kind_l = GEN ? 0 : __builtin_amdgcn_readfirstlane(op_kind(g));
		const int kind = kind_l;
		const int type = GEN ? a.fixed_type : (kind ? GMR1_HIP_DC6 : GMR1_HIP_BCCH);
		const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[kind]);
		const DevBurst &bt = c_types[type];
		typedef Fmt<GEN> F;
		const int w = in_len - F::len(bt) * sps + 1;
		float fsh_l;
		if constexpr (AHEAD)
			fsh_l = fsh_s[q];
		else
			fsh_l = op_fsh(g);
		const float fsh = fsh_l;
		const float fs = (fsh - F::rotation(bt)) / (float)sps;

		const float2 *__restrict__ in = a.iq + (AHEAD ? off_s[q] : op_off(g));
		Touched touched = {0, 0};
		auto touch_next = [&]() {
			if (has_nx)
				touched = window_touch_q(a.iq + off_s[(q + 1) & 3], __builtin_amdgcn_readfirstlane(a.in_len[kind_s[(q + 1) & 3]]), lane);
		};
		const int sl = lane;
		const int tl = F::tl(bt, kind);
		const int nch = F::nch(bt);
		constexpr int NFULL = (!GEN && SPS == 4 && NPL == 16) ? 15 : -1;
		// everything that needs memory is asked for first -- the whole window (statistics) and, again,
		// the ~300 samples under the sync chunks (they go to LDS; the second request hits the lines the
		// first one is fetching) -- and what needs no data (the rotated reference) is computed while it
		// travels
		constexpr int SIT = SMALL ? 1 : (SPS == 4 ? 2 : 4);   // 64-sample pieces per chunk window
		float2 sv_own[NCHK][SIT];
		float2 (&sv)[NCHK][SIT] = sv_own;
		auto fetch_window = [&](const float2 *__restrict__ from) {
			window_fetch<NPL, NFULL>(from, in_len, lane, wv);
#pragma unroll
			for (int c = 0; c < NCHK; c++) {
				const int wl = c < nch ? F::clen(bt, kind, c) * sps + w - 1 : 0;
				const float2 *__restrict__ src = from + (c < nch ? F::cpos(bt, c) * sps : 0);
#pragma unroll
				for (int h = 0; h < SIT; h++) {
					const int sidx = lane + 64 * h;
					sv[c][h] = sidx < wl ? src[sidx] : make_float2(0.f, 0.f);
				}
			}
		};
		// LAT: prepared a round ago by the chain's helper wave, if the burst sits where it was expected (LatPre)
		bool prepared = false;
		const float2 *__restrict__ xst = L.x;
		if constexpr (LAT) {
			prepared = *pre->h_off == op_off(g) && *pre->h_kind == kind;
			if (prepared)
				xst = xst_lat = pre->h_x;
			if constexpr (PART == 1)
				co_on = prepared && pre->co != nullptr && kind == 0;
		}
		if (LAT) {
			if (!prepared)
				fetch_window(in);
		} else {
			if constexpr (PL) {
				window_fetch_q_planar(a.iq, a.plane_stride, io.offset[g], in_len, lane, wv);
			} else {
			if constexpr (QL)
				window_fetch_q<C::ONE_LOAD>(in, in_len, lane, wv);
			else if (q == 0 || !PREFETCH_NEXT)
				window_fetch<NPL, NFULL>(in, in_len, lane, wv);
#pragma unroll
			for (int c = 0; c < NCHK; c++) {
				const int wl = c < nch ? F::clen(bt, kind, c) * sps + w - 1 : 0;
				const float2 *__restrict__ src = in + (c < nch ? F::cpos(bt, c) * sps : 0);
#pragma unroll
				for (int h = 0; h < SIT; h++) {
					const int sidx = lane + 64 * h;
					sv[c][h] = sidx < wl ? src[sidx] : make_float2(0.f, 0.f);
				}
			}
			// (the youngest load: the wait for this burst's data leaves it in flight)
			if constexpr (TOUCH == 1)
				touch_next();
			if constexpr (C::ONE_LOAD)
				window_fix_q(in_len, lane, wv);
			}
		}
		// rotated reference of the (single) sync sequence: without a caller-supplied frequency shift it only depends on
		// the burst format and sps -- a table built once with this same arithmetic (g_coef0)
		// (lane n keeps value n: tl <= 32 for every format this body is launched for)
		float2 cfl = make_float2(0.f, 0.f);
		// (!GEN: the table row itself, read by scalar loads in corr_fixed -- a wave-uniform pointer, so set outside the
		// lane-dependent branches below)
		const float2 *__restrict__ ctab = (!GEN && io.freq_shift == nullptr) ? c_coef0[sps][type] : nullptr;
		if (io.freq_shift == nullptr) {
			if (GEN && lane < 32)
				cfl = g_coef0[sps][type][lane];
		} else if (lane < tl) {
			if constexpr (GEN) {
				cfl = sync_coef0(bt, lane, sps, fs);
			} else {
				// the same with the fused formats' numbers (Fmt<false>): no table walk
				cfl = lat_coef(kind, lane, fs, sps);
			}
		}
		WSYNC();
		if constexpr (FAC) {
			if (lane < 2 * tl)
				L.coef[lane] = sync_coef_seq1(bt, lane >= tl ? 1 : 0, lane >= tl ? lane - tl : lane, sps, fs);
		} else if (GEN && lane < tl)
			L.coef[lane] = cfl;
		float avr, avi, inv;
		if (prepared) {
			avr = pre->h_stat[0];
			avi = pre->h_stat[1];
			inv = pre->h_stat[2];
			if constexpr (PART == 1)
				pre->out_energy = pre->h_stat[3];
			if (io.energy && lane == 0)
				io.energy[g] = pre->h_stat[3];
		} else {
		if constexpr (QL)
			window_stats_q(wv, in_len, lane, avr, avi, inv);
		else
			window_stats<NPL, NFULL>(wv, in_len, sl, avr, avi, inv, -1, 1);
		if constexpr (LAT && PART == 1) {
			if (pre->win_w) {
#pragma unroll
				for (int k = 0; k < NPL; k++)
					pre->win_w[lane + 64 * k] = wv[k];
			}
		}
		if constexpr (LAT && PART == 1) {
			const float e = window_energy_regs<NPL>(wv, in_len, lane);
			pre->out_energy = e;
			if (io.energy && lane == 0)
				io.energy[g] = e;
		} else if ((LAT || !PREFETCH_NEXT) && EN && io.energy) {
			// burst_energy() while the window is still in registers
			const float e = window_energy_regs<NPL>(wv, in_len, lane);
			if (lane == 0)
				io.energy[g] = e;
		}
		}
		GMR1_STAMP(1);
		if (row == q) { avr_r = avr; avi_r = avi; inv_r = inv; }
		if constexpr (TOUCH == 2)
			touch_next();
		if (PREFETCH_NEXT && !LAT && q + 1 < 4 && g + 1 < n_end) {
			// the next burst's window travels during this burst's correlation
			const int kind1 = GEN ? 0 : __builtin_amdgcn_readfirstlane(io.kind[g + 1] ? 1 : 0);
			window_fetch<NPL, NFULL>(a.iq + io.offset[g + 1], __builtin_amdgcn_readfirstlane(a.in_len[kind1]), lane, wv);
		}
		if (!LAT && PREFETCH_NEXT && EN && io.energy) {
			// second read (L2): the registers already hold the next burst's window
			const float e = window_energy<NPL>(in, in_len, lane);
			if (lane == 0)
				io.energy[g] = e;
		}
		// stage the sync-chunk windows, normalised: window c = samples [pos_c sps, pos_c sps + len_c sps + w - 1)
		if constexpr (PL) {
			// The quad layout stages out of the window registers (the planar call; the interleaved one asks for the samples under
			// the sync chunks a second time, as the other instantiations do -- staging out of registers that have to last through
			// the correlation for the kept samples costs it more registers than it has): a lane's four consecutive samples 256 b + 4 l .. + 3 lie wholly
			// inside a chunk window or wholly outside it (the windows start on a symbol, 4 | pos sps, and are len sps + w - 1
			// samples long with w - 1 = 80 or 40), so a lane whose quad is inside writes it with two 16-byte stores.  Chunk 0
			// ([112, 236) at most) lies in quarter 0, chunk 1 ([476, 568)) in quarters 1 and 2, chunk 2 ([788, 880)) in quarter 3.
			const int wl0 = F::clen(bt, kind, 0) * 4 + w - 1, wl1 = 3 * 4 + w - 1;
			const v2f av = {avr, avi}, iv = {inv, inv};
			auto stage_quad = [&](int b, int start, int wl, int wb) {
				const int rel = 256 * b + 4 * lane - start;
				if (rel >= 0 && rel < wl) {
					v2f n0 = ((v2f){wv[4 * b].x, wv[4 * b].y} - av) * iv, n1 = ((v2f){wv[4 * b + 1].x, wv[4 * b + 1].y} - av) * iv;
					v2f n2 = ((v2f){wv[4 * b + 2].x, wv[4 * b + 2].y} - av) * iv, n3 = ((v2f){wv[4 * b + 3].x, wv[4 * b + 3].y} - av) * iv;
					float4 *dst = reinterpret_cast<float4 *>(L.x + wb + rel);
					dst[0] = make_float4(n0.x, n0.y, n1.x, n1.y);
					dst[1] = make_float4(n2.x, n2.y, n3.x, n3.y);
				}
			};
			stage_quad(0, 28 * 4, wl0, 0);
			stage_quad(1, 119 * 4, wl1, wl0);
			stage_quad(2, 119 * 4, wl1, wl0);
			stage_quad(3, 197 * 4, wl1, wl0 + wl1);
		} else
		if (!prepared) {
			int wb = 0;
#pragma unroll
			for (int c = 0; c < NCHK; c++) {
				const int wl = c < nch ? F::clen(bt, kind, c) * sps + w - 1 : 0;
#pragma unroll
				for (int h = 0; h < SIT; h++) {
					const int sidx = sl + 64 * h;
					if (sidx < wl) {
						const v2f nv = ((v2f){sv[c][h].x, sv[c][h].y} - (v2f){avr, avi}) * (v2f){inv, inv};
						L.x[wb + sidx] = make_float2(nv.x, nv.y);
					}
				}
				wb += wl;
			}
		}
		// (TOUCH 1: the touch was asked for right behind the samples staged above, so it is here by now)
		if constexpr (TOUCH == 1)
			window_touch_done(touched);
		WSYNC();
		float *corr = L.corr + q * cw;
		if constexpr (!GEN) {
			// BCCH / DC6: static tap structure (the host refuses to start this kernel if the tables say otherwise)
			if (LAT && PART == 1 && co_on) {
				// the whole rounds of lags here, the last partial one on the helper wave
				const int j0 = ((w - 1) >> 6) << 6;
				corr_fixed<SPS, 11, 3, 3>(xst, sps, w, lane, ctab, cfl, corr, 0, j0);
				if (lds_wait_eq(&pre->co->c_id, pre->co_id)) {
					if (lane < w - j0)
						corr[j0 + lane] = pre->co->tail[lane];
				} else
					corr_fixed<SPS, 11, 3, 3>(xst, sps, w, lane, ctab, cfl, corr, j0, w);
			} else if constexpr (QX) {
				uint32_t cbest = 0;
				int cbj = 0;
				if (kind == 0)
					corr_fixed<SPS, 11, 3, 3>(xst, sps, w, lane, ctab, cfl, corr, 0, -1, &cbest, &cbj);
				else
					corr_fixed<SPS, 7, 3, 3>(xst, sps, w, lane, ctab, cfl, corr, 0, -1, &cbest, &cbj);
				// the lag of the largest magnitude (any lane that holds it): the speculated pick
				uint32_t mx = cbest, o;
				o = dpp<0xB1>(mx); mx = o > mx ? o : mx;
				o = dpp<0x4E>(mx); mx = o > mx ? o : mx;
				o = dpp<0x141>(mx); mx = o > mx ? o : mx;
				o = dpp<0x140>(mx); mx = o > mx ? o : mx;
				const uint32_t m01 = max((uint32_t)__builtin_amdgcn_readlane((int)mx, 0), (uint32_t)__builtin_amdgcn_readlane((int)mx, 16));
				const uint32_t m23 = max((uint32_t)__builtin_amdgcn_readlane((int)mx, 32), (uint32_t)__builtin_amdgcn_readlane((int)mx, 48));
				const uint32_t M = max(m01, m23);
				const unsigned long long holders = __ballot(cbest == M);
				const int d = __builtin_amdgcn_readlane(cbj, holders ? __builtin_ctzll(holders) : 0);     // 0 <= d < w <= 81
				// row q keeps what the rows below need of this burst at that pick: the normalised samples under its sync symbols
				// (still staged) ...
				if (row == q) {
					zm_q = (zm_q & 0x00ffffffu) | ((uint32_t)d << 24);
					const int pl = (xsp_bc >> (kind ? 8 : 0)) & 0xff;
					if (pl != 0xff)
						xs_q[0] = xst[pl + d];
					// (the one symbol beyond the sixteenth: BCCH's n = 16, symbol 2 of the third chunk, on the row's first lane)
					if (kind == 0 && col == 0)
						xs_q[1] = xst[11 * 4 + w - 1 + 3 * 4 + w - 1 + 2 * 4 + d];
				}
				// ... and every lane the phases of its four kept samples i = lane + 64 r: sample 4 i + d is sub-slot d & 3 of lane
				// (i + (d >> 2)) & 63 in quarter (i + (d >> 2)) >> 6 of the window registers
				{
					const int srcl = lane + (d >> 2);
					const int addr = (srcl & 63) << 2;
					const bool up = srcl >= 64;
					float2 rot[4];
					auto pull = [&](const float2 &v) {
						return make_float2(__builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v.x))),
						                   __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v.y))));
					};
					switch (d & 3) {                                  // (wave-uniform)
					case 0: rot[0] = pull(wv[0]); rot[1] = pull(wv[4]); rot[2] = pull(wv[8]); rot[3] = pull(wv[12]); break;
					case 1: rot[0] = pull(wv[1]); rot[1] = pull(wv[5]); rot[2] = pull(wv[9]); rot[3] = pull(wv[13]); break;
					case 2: rot[0] = pull(wv[2]); rot[1] = pull(wv[6]); rot[2] = pull(wv[10]); rot[3] = pull(wv[14]); break;
					default: rot[0] = pull(wv[3]); rot[1] = pull(wv[7]); rot[2] = pull(wv[11]); rot[3] = pull(wv[15]); break;
					}
#pragma unroll
					for (int r = 0; r < 4; r++) {
						const int i = lane + 64 * r;
						float2 x = up ? (r < 3 ? rot[r < 3 ? r + 1 : 3] : make_float2(0.f, 0.f)) : rot[r];
						// (kept samples 0 .. 191 lie inside any window this kernel is started for: 4 * 191 + 80 < 960 <= in_len)
						const bool ok = r < 3 || (i < 234 && 4 * i + d < in_len);
						// (as pass 2 does it: the mean is subtracted whether or not the lane has a sample; the zero test knows)
						x.x -= avr;
						x.y -= avi;
						th_q[q][r] = atan2_turns(x.y, x.x);
						if (!ok || (x.x == 0.0f && x.y == 0.0f))
							zm_q |= 1u << (4 * q + r);
					}
				}
			} else if (kind == 0)
				corr_fixed<SPS, 11, 3, 3>(xst, sps, w, lane, ctab, cfl, corr);
			else
				corr_fixed<SPS, 7, 3, 3>(xst, sps, w, lane, ctab, cfl, corr);
		} else if constexpr (FAC) {
			const int len = bt.sync[0][0].len;
			for (int j = lane; j < w; j += 64) {
				const float2 *xp = L.x + j;
				v2f acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
				for (int n = 0; n < len; n++) {
					const float2 x = xp[n * sps];
					const float2 c0 = L.coef[n], c1 = L.coef[tl + n];
					acc0 = __builtin_elementwise_fma((v2f){-c0.y, c0.y}, (v2f){x.y, x.x}, acc0);
					acc0 = __builtin_elementwise_fma((v2f){c0.x, c0.x}, (v2f){x.x, x.y}, acc0);
					acc1 = __builtin_elementwise_fma((v2f){-c1.y, c1.y}, (v2f){x.y, x.x}, acc1);
					acc1 = __builtin_elementwise_fma((v2f){c1.x, c1.x}, (v2f){x.x, x.y}, acc1);
				}
				float cj = 0.f;
				cj += sqrtf(fmaf(acc0.x, acc0.x, acc0.y * acc0.y));
				corr[j] = cj;                               // sequence 0
				cj += sqrtf(fmaf(acc1.x, acc1.x, acc1.y * acc1.y));
				corr[cwh + j] = cj;                         // what sequence 1 is ranked and timed on
			}
		} else
		for (int j = lane; j < w; j += 64) {
			float cj = 0.f;
			int base = 0, wb = 0;
			for (int ch = 0; ch < nch; ch++) {
				const int len = F::clen(bt, kind, ch);
				const float2 *xp = L.x + wb + j;          // staged window of this chunk
				const float2 *cp = L.coef + base;
				// (ar, ai) += c x as two packed FMAs: (-c.im x.im, c.im x.re) first, then c.re (x.re, x.im) -- the order the
				// scalar chains ar = fma(c.re, x.re, fma(-c.im, x.im, ar)), ai = fma(c.re, x.im, fma(c.im, x.re, ai)) had
				v2f acc = {0.f, 0.f};
				for (int n = 0; n < len; n++) {
					const float2 x = xp[n * sps];
					const float2 cf = cp[n];
					acc = __builtin_elementwise_fma((v2f){-cf.y, cf.y}, (v2f){x.y, x.x}, acc);
					acc = __builtin_elementwise_fma((v2f){cf.x, cf.x}, (v2f){x.x, x.y}, acc);
				}
				const float ar = acc.x, ai = acc.y;
				base += len;
				wb += len * sps + w - 1;
				cj += sqrtf(fmaf(ar, ar, ai * ai));
			}
			corr[j] = cj;
		}
		if constexpr (TOUCH == 2)
			window_touch_done(touched);
	}
	}
	WSYNC();
	GMR1_STAMP(2);
	if (a.dbg_stop == 2) return;
	}


	// per-row (lane-resident) burst parameters: looked up here, not before pass 1, which has no register to spare for them
	// (H_ROW: out of the scalars pass 1 read them into -- no trip to memory)
	int kind_row = 0;
	uint64_t off_row = 0;
	float fsh_row = 0.f;
	if constexpr (H_ROW) {
		// (the row number is made opaque here, so that the selects below are not formed burst by burst inside pass 1)
		int row_o = row;
		asm volatile("" : "+v"(row_o));
		kind_row = row_o == 0 ? kind_s[0] : (row_o == 1 ? kind_s[1] : (row_o == 2 ? kind_s[2] : kind_s[3]));
		off_row = row_o == 0 ? off_s[0] : (row_o == 1 ? off_s[1] : (row_o == 2 ? off_s[2] : off_s[3]));
		fsh_row = row_o == 0 ? fsh_s[0] : (row_o == 1 ? fsh_s[1] : (row_o == 2 ? fsh_s[2] : fsh_s[3]));
		if (!row_live) {
			kind_row = 0;
			off_row = 0;
			fsh_row = 0.f;
		}
	}
	int kind_r_l;
	if constexpr (H_ROW)
		kind_r_l = kind_row;
	else
		kind_r_l = (!GEN && row_live) ? op_kind(g_row) : 0;
	const int kind_r = kind_r_l;
	const int type_r = GEN ? a.fixed_type : (kind_r ? GMR1_HIP_DC6 : GMR1_HIP_BCCH);
	typedef Fmt<GEN> F;
	const int in_len_r = kind_r ? a.in_len[1] : a.in_len[0];
	float fsh_r_l;
	if constexpr (H_ROW)
		fsh_r_l = fsh_row;
	else
		fsh_r_l = row_live ? op_fsh(g_row) : 0.0f;
	const float fsh_r = fsh_r_l;
	const DevBurst &bt_r = c_types[type_r];
	const float fs_r = (fsh_r - F::rotation(bt_r)) / (float)sps;     // pi4cxpsk.c:539
	const int w_r = in_len_r - F::len(bt_r) * sps + 1;
	const float2 *__restrict__ in_r = a.iq + (H_ROW ? off_row : (row_live ? op_off(g_row) : 0));

	// =========================== rows: peak + early/late timing ===========================
	// osmo_cxvec_peak_energy_find(corr, 3, PEAK_EARLY_LATE, &peak), pi4cxpsk.c:240
	// LAT: the one burst is row 0's; the other rows work on ITS correlation (speculative bisection below)
	const float *cr = L.corr + (LAT ? 0 : row) * cw;          // FAC: moved to the second array for the second sequence
	const int w_p = LAT ? __builtin_amdgcn_readlane(w_r, 0) : w_r;
	const int tl_p = LAT ? F::tl(c_types[__builtin_amdgcn_readlane(type_r, 0)], __builtin_amdgcn_readlane(kind_r, 0)) : F::tl(bt_r, kind_r);
	// (LAT: the loop's windows have 10 * sps + 1 or 20 * sps + 1 lags -- a constant lets the two little loops below unroll)
	const int win = LAT ? 3 : (w_p < 3 ? w_p : 3);
	const bool w3 = !LAT && __ballot(win != 3) == 0;   // (wave-uniform) every row's energy window is three lags
	float toa_r = 0.f, p_pwr = 0.f;                    // pi4cxpsk.c:227-237: the best sequence so far
	int sid_r = -1;
	if constexpr (PART == 2) {
		toa_r = pre->cut->toa;
		sid_r = pre->cut->sid;
		avr_r = pre->cut->avr;
		avi_r = pre->cut->avi;
	}
	for (int sq = 0; sq < (PART == 2 ? 0 : (FAC ? 2 : 1)); sq++) {
		if (FAC)
			cr = L.corr + row * cw + sq * cwh;
		GMR1_STAMP(10);
		int mi;
		if constexpr (LAT) {
			// the one burst's <= 128 lags, two per lane: the largest window energy as a 32-bit maximum (a non-negative float's
			// bits order like its value) by four DPP steps and four v_readlane, then the LOWEST lag that has it from two ballots
			// -- what the 64-bit (energy, ~index) keys of the batch form decide, in a quarter of the instructions
			constexpr int NH = SPS == 4 ? 2 : 3;              // 81 lags at sps 4, <= 161 at sps 8
			uint32_t eb2[NH];
			bool ok2[NH];
			uint32_t mx = 0;
#pragma unroll
			for (int h = 0; h < NH; h++) {
				const int m = lane + 64 * h;
				ok2[h] = m + win <= w_p;
				float e = 0.f;
				for (int k = 0; k < win; k++) {
					const float c = cr[ok2[h] ? m + k : 0];
					e += c * c;
				}
				eb2[h] = ok2[h] ? __builtin_bit_cast(uint32_t, e) : 0u;
				mx = eb2[h] > mx ? eb2[h] : mx;
			}
			uint32_t o;
			o = dpp<0xB1>(mx); mx = o > mx ? o : mx;
			o = dpp<0x4E>(mx); mx = o > mx ? o : mx;
			o = dpp<0x141>(mx); mx = o > mx ? o : mx;
			o = dpp<0x140>(mx); mx = o > mx ? o : mx;
			const uint32_t m01 = max((uint32_t)__builtin_amdgcn_readlane((int)mx, 0), (uint32_t)__builtin_amdgcn_readlane((int)mx, 16));
			const uint32_t m23 = max((uint32_t)__builtin_amdgcn_readlane((int)mx, 32), (uint32_t)__builtin_amdgcn_readlane((int)mx, 48));
			const uint32_t M = max(m01, m23);
			mi = 0;
#pragma unroll
			for (int h = NH - 1; h >= 0; h--) {
				const unsigned long long bh = __ballot(ok2[h] && eb2[h] == M);
				if (bh)
					mi = 64 * h + __builtin_ctzll(bh);
			}
		} else {
		if (w3) {
			// every row's window energy is over three lags (any search window of >= 3 lags): per lane the best of its lags
			// m = col, col + 16, ... in ascending order (a later one must be strictly larger), then over the row the largest
			// energy as a 32-bit maximum (a non-negative float's bits order like its value) and the LOWEST lag that has it --
			// what the 64-bit (energy, ~lag) keys below decide, in a third of the instructions
			uint32_t be = 0;
			int bl = 0x7fffffff;
			for (int m = col; m + 3 <= w_p; m += 16) {
				const float c0 = cr[m], c1 = cr[m + 1], c2 = cr[m + 2];
				float e = c0 * c0;                           // (0 + c0^2 is c0^2)
				e += c1 * c1;
				e += c2 * c2;
				const uint32_t eb = __builtin_bit_cast(uint32_t, e);
				const bool better = bl == 0x7fffffff || eb > be;
				be = better ? eb : be;
				bl = better ? m : bl;
			}
			uint32_t mx = be, o;
			o = dpp<0xB1>(mx); mx = o > mx ? o : mx;
			o = dpp<0x4E>(mx); mx = o > mx ? o : mx;
			o = dpp<0x141>(mx); mx = o > mx ? o : mx;
			o = dpp<0x140>(mx); mx = o > mx ? o : mx;
			uint32_t lo = (bl != 0x7fffffff && be == mx) ? (uint32_t)bl : 0x7fffffffu;
			o = dpp<0xB1>(lo); lo = o < lo ? o : lo;
			o = dpp<0x4E>(lo); lo = o < lo ? o : lo;
			o = dpp<0x141>(lo); lo = o < lo ? o : lo;
			o = dpp<0x140>(lo); lo = o < lo ? o : lo;
			mi = lo == 0x7fffffffu ? -1 : (int)lo;
		} else {
		unsigned long long key = 0;
		for (int m = col; m + win <= w_p; m += 16) {
			float e = 0.f;
			for (int k = 0; k < win; k++) {
				const float c = cr[m + k];
				e += c * c;
			}
			const unsigned long long kk = ((unsigned long long)__builtin_bit_cast(uint32_t, e) << 32) | (uint32_t)(~m);
			key = kk > key ? kk : key;
		}
		key = row_max_u64<1>(key);
		key = row_max_u64<2>(key);
		key = row_max_u64<4>(key);
		key = row_max_u64<8>(key);
		mi = (int)(~(uint32_t)key);
		}
		}
		if (mi < 0 || mi + win > w_p)
			mi = 0;
		GMR1_STAMP(11);
		int p = mi;
		if (w3 || LAT) {
			float pe = -1.f;
#pragma unroll
			for (int k = 0; k < 3; k++) {
				const float c = cr[mi + k];
				const float e = c * c;
				const bool up = e > pe;
				pe = up ? e : pe;
				p = up ? mi + k : p;
			}
		} else {
			float pe = -1.f;
			for (int k = 0; k < win; k++) {
				const float c = cr[mi + k];
				const float e = c * c;
				if (e > pe) { pe = e; p = mi + k; }
			}
		}
		GMR1_STAMP(8);
		if constexpr (LAT && PART == 1) {
			if (co_on) {
				// the helper wave starts on the sync-symbol terms of round(toa) = p - 1, p, p + 1
				co_p = __builtin_amdgcn_readfirstlane(p);
				if (lane == 0) {
					pre->co->p = co_p;
					lds_post(&pre->co->p_id, pre->co_id);
				}
			}
		}
		// interpolated correlation at `pos` (lanes 0-7 of the row) and at `pos + 2` (lanes 8-15): same
		// fractional part, so the same 21 weights; lane sub = col & 7 holds taps k = 3 sub - 10 + {0,1,2}
		const int ipt = col >> 3, isub = col & 7;
		// what the evaluations below share: the lane's first tap, as an index offset and as the float the weight needs, the
		// sign bit sin(pi (k - f)) = -(-1)^k sin(pi f) sets for an even first tap, whether the lane has taps at all (sub 7
		// would hold k = 11, 12, 13) and the one bound an array index has to be checked against: i = ib + k with |k| <= 10
		// lies in [max(ib - 10, 0), min(ib + 11, w - 1)) exactly if 0 <= i < w - 1
		const int k0 = 3 * isub - 10;
		const float kf0 = (float)k0, kf1 = (float)(k0 + 1), kf2 = (float)(k0 + 2);
		const uint32_t sgn0 = (isub & 1) ? 0u : 0x80000000u;
		const bool has_taps = isub != 7;
		const uint32_t wlim = (uint32_t)(w_p - 1);
		// -> acc: the lane's own half-row sum (at `pos` in lanes 0-7, at `pos + 2` in lanes 8-15), oth: the other half's
		// (guard: the weight 1 within 0.01 of a whole tap, osmo_sinc's small-argument case.  The walk's levels stand on odd
		// multiples of 1/2 ... 1/256, at least pi / 256 = 0.0123 from every tap: only the evaluation at the point reached --
		// a multiple of 1/512 -- can come that close, so the eight evaluations of the walk go without the two compares and the
		// select per tap)
		auto interp2 = [&](float pos, float &acc_o, float &oth_o, auto guard_tag) {
			constexpr bool GUARD = decltype(guard_tag)::value;
			const float fl = floorf(pos);
			const int ib = (int)fl + 2 * ipt;
			const float f = pos - fl;
			const float S = __builtin_amdgcn_sinf(0.5f * f);       // sin(pi f)
			float acc = 0.f;
			if (SMALL && w_p <= 8) {
				// A search window of at most eight lags (NT3: seven) has at most seven correlation values to interpolate
				// over: lane sub takes the ONE value cr[sub] with the weight of tap k = sub - ib, instead of three of the
				// 21 tap places of which most lie outside the array (a third of the instructions of the timing rows).
				int b = ib - 10, e = ib + 11;
				if (b < 0) b = 0;
				if (e >= w_p) e = w_p - 1;
				const int k = isub - ib;
				const float sg = (k & 1) ? S : -S;
				const float xx = kPif * ((float)k - f);
				const float wgt = (!GUARD || xx >= 0.01f || xx <= -0.01f) ? sg * __builtin_amdgcn_rcpf(xx) : 1.0f;
				const bool valid = isub >= b && isub < e;          // (|k| <= 10 follows from b and e)
				const float c = cr[isub];
				acc = valid ? c * wgt : 0.0f;
			} else {
				// (the three values are read whether or not they lie in the array -- an LDS address outside it is harmless --
				// and dropped by the select)
				const int i0 = ib + k0;
				const float *cp = cr + i0;
				const float c0 = cp[0], c1 = cp[1], c2 = cp[2];
				const float S0 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, S) ^ sgn0);
				const float x0 = kPif * (kf0 - f), x1 = kPif * (kf1 - f), x2 = kPif * (kf2 - f);
				const float w0 = (!GUARD || x0 >= 0.01f || x0 <= -0.01f) ? S0 * __builtin_amdgcn_rcpf(x0) : 1.0f;
				const float w1 = (!GUARD || x1 >= 0.01f || x1 <= -0.01f) ? -S0 * __builtin_amdgcn_rcpf(x1) : 1.0f;
				const float w2 = (!GUARD || x2 >= 0.01f || x2 <= -0.01f) ? S0 * __builtin_amdgcn_rcpf(x2) : 1.0f;
				const bool v0 = has_taps && (uint32_t)i0 < wlim;
				const bool v1 = has_taps && (uint32_t)(i0 + 1) < wlim;
				const bool v2 = has_taps && (uint32_t)(i0 + 2) < wlim;
				acc += v0 ? c0 * w0 : 0.0f;
				acc += v1 ? c1 * w1 : 0.0f;
				acc += v2 ? c2 * w2 : 0.0f;
			}
			acc += row_xorf<1>(acc);
			acc += row_xorf<2>(acc);
			acc += row_xorf<4>(acc);
			acc_o = acc;
			oth_o = row_xorf<8>(acc);
		};
		float early = (float)p - 1.0f, incr = 0.5f;
		bool active = true;
		float toa_s, pk_s;
		if constexpr (LAT) {
			// THREE levels of the bisection per evaluation (the eight groups of 8 lanes each interpolate the correlation at one
			// candidate position and two samples later -- same fractional part, same 21 weights, lane sub holding taps
			// k = 3 sub - 10 + {0,1,2}): group 0 at the current point, groups 1 / 2 where the search goes if the early / the
			// late side wins, groups 3..6 one level further down.  The candidates are formed by the float operations the
			// level-by-level walk performs and summed in its order, so the decisions are its decisions; the walk itself is
			// scalar work on two ballots.  Nine levels = three evaluations, then the peak value at the point reached.
			const int grp = lane >> 3, isub8 = lane & 7;
			// (index checks and tap signs as in interp2 above: 0 <= i < w - 1 is the whole bound, one XOR sets the sign)
			const int k08 = 3 * isub8 - 10;
			const float kg0 = (float)k08, kg1 = (float)(k08 + 1), kg2 = (float)(k08 + 2);
			const uint32_t sgn8 = (isub8 & 1) ? 0u : 0x80000000u;
			const bool taps8 = isub8 != 7;
			auto interp_pair = [&](float pos, float &se, float &sl) {
				const float fl = floorf(pos);
				const int ib = (int)fl;
				const float f = pos - fl;
				const float S = __builtin_amdgcn_sinf(0.5f * f);       // sin(pi f); sin(pi (k - f)) = -(-1)^k sin(pi f)
				const int i0 = ib + k08;
				const float *cp = cr + i0;
				// early sum over i0 + {0, 1, 2}, late sum two lags further up: five values, whether or not they lie in the array
				const float c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4];
				const float S0 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, S) ^ sgn8);
				const float x0 = kPif * (kg0 - f), x1 = kPif * (kg1 - f), x2 = kPif * (kg2 - f);
				const float w0 = (x0 >= 0.01f || x0 <= -0.01f) ? S0 * __builtin_amdgcn_rcpf(x0) : 1.0f;
				const float w1 = (x1 >= 0.01f || x1 <= -0.01f) ? -S0 * __builtin_amdgcn_rcpf(x1) : 1.0f;
				const float w2 = (x2 >= 0.01f || x2 <= -0.01f) ? S0 * __builtin_amdgcn_rcpf(x2) : 1.0f;
				float ae = 0.f, al = 0.f;
				ae += (taps8 && (uint32_t)i0 < wlim) ? c0 * w0 : 0.0f;
				al += (taps8 && (uint32_t)(i0 + 2) < wlim) ? c2 * w0 : 0.0f;
				ae += (taps8 && (uint32_t)(i0 + 1) < wlim) ? c1 * w1 : 0.0f;
				al += (taps8 && (uint32_t)(i0 + 3) < wlim) ? c3 * w1 : 0.0f;
				ae += (taps8 && (uint32_t)(i0 + 2) < wlim) ? c2 * w2 : 0.0f;
				al += (taps8 && (uint32_t)(i0 + 4) < wlim) ? c4 * w2 : 0.0f;
				ae += row_xorf<1>(ae);
				ae += row_xorf<2>(ae);
				ae += row_xorf<4>(ae);
				al += row_xorf<1>(al);
				al += row_xorf<2>(al);
				al += row_xorf<4>(al);
				se = ae;
				sl = al;
			};
			// The loop's front (PART 1) stops after the FIRST evaluation.  Everything it hands on depends on the timing through
			// the pick round(toa) alone (pi4cxpsk.c:292-295; the feedback is align += round(toa) - e_toa, gmr1_rx.c:782; no
			// record carries toa), and round(toa) is settled by the first two levels: the walk starts on the whole lag p - 1
			// and steps by 1/2, 1/4, ... 1/512, so after two levels toa = early + 1 is p -+ 1/4 or p -+ 3/4 and the seven levels
			// left move it by less than 1/4 in all -- never across p -+ 1/2; a level that ties ends the walk in both forms.
			constexpr int kEvals = PART == 1 ? 1 : 3;
	#pragma unroll 1
			for (int it = 0; it < kEvals; it++) {
				const float half = incr * 0.5f, quarter = incr * 0.25f;
				float pos = early;
				if (grp == 1) {
					pos = early - incr;
				} else if (grp == 2) {
					pos = early + incr;
				} else if (grp >= 3 && grp <= 6) {
					const float a1 = grp < 5 ? early - incr : early + incr;
					pos = (grp & 1) ? a1 - half : a1 + half;           // 3: - -, 4: - +, 5: + -, 6: + +
				}
				float se, sl;
				interp_pair(pos, se, sl);
				const float ee = se * se, le = sl * sl;
				const unsigned long long m_neg = __ballot(ee > le), m_pos = __ballot(ee < le);
				auto dec = [&](int gq) -> int { return ((m_neg >> (8 * gq)) & 1ull) ? -1 : (((m_pos >> (8 * gq)) & 1ull) ? 1 : 0); };
				const int d0 = dec(0);
				if (d0 == 0) break;
				early = d0 < 0 ? early - incr : early + incr;
				const int d1 = dec(d0 < 0 ? 1 : 2);
				if (d1 == 0) break;
				early = d1 < 0 ? early - half : early + half;
				const int d2 = dec(3 + (d0 > 0 ? 2 : 0) + (d1 > 0 ? 1 : 0));
				if (d2 == 0) break;
				early = d2 < 0 ? early - quarter : early + quarter;
				incr *= 0.125f;
			}
			toa_s = early + 1.0f;
			GMR1_STAMP(9);
			float pa, po;
			interp2(toa_s, pa, po, std::true_type{});
			pk_s = ipt ? po : pa;
		} else {
			// early energy ee > late energy le: early -= incr, ee < le: early += incr.  Lanes 8-15 hold the late sum as their
			// own, so they see the two energies swapped and step by -incr instead: the same decisions without the selects
			float sincr = ipt ? -incr : incr;
			{
				// the first level sits on a whole lag (early = p - 1): sin(pi f) = 0, so tap 0 has the weight 1 and the twenty
				// others (+-)0 -- the two sums ARE cr[p - 1] and cr[p + 1] (0 outside the array), no interpolation to run
				const int io = p - 1 + 2 * ipt;
				const float c = cr[io];
				const float sa = (uint32_t)io < wlim ? c : 0.0f;
				const float so = row_xorf<8>(sa);
				const float ea = sa * sa, eo = so * so;
				if (ea > eo) early -= sincr;
				else if (ea < eo) early += sincr;
				else active = false;
				sincr *= 0.5f;
			}
	#pragma unroll 1
			for (int it = 1; it < 9; it++) {              // incr = 0.25 ... 1/512 (> 1/1024)
				float sa, so;
				interp2(early, sa, so, std::false_type{});
				const float ea = sa * sa, eo = so * so;
				if (active) {
					if (ea > eo) early -= sincr;
					else if (ea < eo) early += sincr;
					else active = false;
				}
				sincr *= 0.5f;
			}
			toa_s = early + 1.0f;
			float pa, po;
			interp2(toa_s, pa, po, std::true_type{});
			pk_s = ipt ? po : pa;
		}
		pk_s = pk_s * __builtin_amdgcn_rcpf((float)tl_p);
		if (pk_s * pk_s > p_pwr) {                      // needs strictly more than what is there (0 at first)
			p_pwr = pk_s * pk_s;
			toa_r = toa_s;
			sid_r = sq;
		}
	}
	const bool found_r = sid_r >= 0;
	if constexpr (PART != 2) {
		GMR1_STAMP(3);
		if (a.dbg_stop == 3) return;
	}
	const int d_r = (int)roundf(toa_r);

	// QX: whose speculated pick held (per row; a burst that was not found has no pass 2 at all)
	const bool hit_r = QX && found_r && d_r == (int)(zm_q >> 24) && a.dbg_stop != 101;      // (101: experiment, every burst takes the old route)
#ifdef GMR1_HIP_PROFILE
	if constexpr (QX) {
		// (counted only when asked for, GMR1_HIP_DBG_STOP=105: fifteen thousand atomic adds to one word per launch cost the profiling
		// build a tenth of the kernel's time -- and made an experiment that switched them off with the mis-speculation look like
		// a 10 % gain)
		if (a.dbg_stop == 105 && col == 0 && row_live && found_r && !hit_r)
			atomicAdd(&g_prof_miss, 1);
	}
#endif

	// pass-2 operands of a burst (its 234 symbols at stride sps from sample d, re-read from
	// L2 / Infinity Cache): fetched two bursts ahead of their use
	struct Sym4 { float2 x[NSYM]; int ok; };
	auto fetch = [&](int q, Sym4 &o) {
		const int g = g0 + q;
		o.ok = 0;
#pragma unroll
		for (int r = 0; r < NSYM; r++) o.x[r] = make_float2(0.f, 0.f);
		if (q < 0 || q >= 4 || g >= n_end || a.dbg_stop == 100)     // 100: timing experiment, pass 2 without its re-read
			return;
		const int src = 16 * q;
		const int kind = __builtin_amdgcn_readlane(kind_r, src);
		const DevBurst &bt = c_types[GEN ? a.fixed_type : (kind ? GMR1_HIP_DC6 : GMR1_HIP_BCCH)];
		const int in_len = __builtin_amdgcn_readlane(in_len_r, src);
		const int d = __builtin_amdgcn_readlane(d_r, src);
		const float2 *__restrict__ in = a.iq + op_off(g);
		const int blen = F::len(bt);
		if constexpr (PL) {
			// the kept samples d, d + 4, ... are consecutive in plane (offset + d) & 3
			const long long sr = (long long)io.offset[g] + d;
			in = a.iq + (sr & 3) * a.plane_stride + (sr >> 2);
		}
#pragma unroll
		for (int r = 0; r < NSYM; r++) {
			const int i = lane + 64 * r;
			const int j = i * sps + d;
			if (i < blen && j >= 0 && j < in_len) {
				if (LAT && PART == 2)
					o.x[r] = pre->win_r[j];
				else
					o.x[r] = PL ? in[i] : in[j];
				o.ok |= 1 << r;
			}
		}
	};
	// pass 2 takes the bursts last-read first: burst 3's window was streamed in a few microseconds ago and may still be
	// in this XCD's L2, burst 0's is long gone from it
	// (two bursts ahead of their use: asking for all four at once was measured and is no faster)
	Sym4 first, second;
	int first_q = -1;                                  // QX: the mis-speculated burst whose samples `first` holds

	// =========================== rows: sync symbols, frequency, phase ===========================
	const int nbits_r = F::nbits(bt_r);
	const int nch_r = F::nch(bt_r);
	const int tl_r = F::tl(bt_r, kind_r);
	float ffe_r = 0.f, psi_r = 0.f;
	if constexpr (PART == 2) {
		ffe_r = pre->cut->ffe;
		psi_r = pre->cut->psi;
		fetch(0, first);
	} else if constexpr (LAT) {
		if constexpr (PART == 0)
			fetch(0, first);            // the one burst's kept samples travel during the whole sync-term phase
		bool have = false;
		if constexpr (PART == 1) {
			if (co_on) {
				// what the helper wave made of the candidate that round(toa) turned out to be
				const int k = __builtin_amdgcn_readfirstlane(d_r) - (co_p - 1);
				if ((unsigned)k < 3u && lds_wait_eq(&pre->co->s_id, pre->co_id)) {
					ffe_r = pre->co->ffe[k];
					psi_r = pre->co->psi[k];
					have = true;
				}
			}
		}
		if (!have)
			lat_sync_terms(xst_lat, kind_r, d_r, row_live, fs_r, sps, w_r, in_len_r, col, ffe_r, psi_r);
	} else {
		// lane col holds sync symbols n = col and n = col + 16 (< tl <= 32); their samples are asked for first (loads
		// come back in order), then pass 2's
		float2 t0[NSH], xr[NSH];
		int chn[NSH], spos[NSH], idxv[NSH], nnv[NSH];
#pragma unroll
		for (int h = 0; h < NSH; h++) {
			const int n = col + 16 * h;
			t0[h] = xr[h] = make_float2(0.f, 0.f);
			chn[h] = -1;
			spos[h] = idxv[h] = nnv[h] = 0;
			if (n < tl_r && row_live) {
				int ch = 0, base = 0, cum = 0, wb = 0;
				for (int c = 0; c < nch_r - 1; c++) {
					cum += F::clen(bt_r, kind_r, c);
					if (n >= cum) { base = cum; ch = c + 1; wb += F::clen(bt_r, kind_r, c) * sps + w_r - 1; }
				}
				const int nn = n - base;
				const int sp = F::cpos(bt_r, ch) + nn;
				const int idx = sp * sps + d_r;
				if (idx >= 0 && idx < in_len_r) {
					// LAT, the wave's one burst: its sync-chunk windows are still staged (normalised, which no angle
					// below notices) -- no second trip to L2
					if constexpr (PL) {
						// sample sp sps + d of the window = place sp of the plane the kept samples lie in
						const long long sr = (long long)(row_live ? io.offset[g_row] : 0) + d_r;
						xr[h] = (a.iq + (sr & 3) * a.plane_stride + (sr >> 2))[sp];
					} else if (QX && hit_r) {
						xr[h] = xs_q[h];            // taken from the staged windows when the pick was speculated (normalised)
					} else
					xr[h] = LAT ? xst_lat[wb + nn * sps + d_r] : in_r[idx];
				}
				chn[h] = ch;
				spos[h] = sp;
				idxv[h] = idx;
				nnv[h] = nn;
			}
		}
		if constexpr (LAT) {
			if constexpr (PART == 0)
				fetch(0, first);        // the one burst's kept samples travel during the whole sync-term phase
		} else if constexpr (QX) {
			// the (rare) burst whose pick is not the speculated one: its kept samples travel during the rest of this phase (the last
			// such burst of the wave; a second one in the same wave waits for its samples in pass 2)
			const unsigned long long mb = __ballot(found_r && !hit_r && row_live);       // (row-uniform: bit 16 q speaks for burst q)
			const unsigned missm = (unsigned)((mb & 1ull) | ((mb >> 15) & 2ull) | ((mb >> 30) & 4ull) | ((mb >> 45) & 8ull));
			first_q = missm ? 31 - __builtin_clz(missm) : -1;
			if (first_q >= 0)
				fetch(first_q, first);
		} else {
			fetch(3, first);
			fetch(2, second);
		}
#pragma unroll
		for (int h = 0; h < NSH; h++) {
			if (chn[h] >= 0) {
				const int idx = idxv[h], ch = chn[h], nn = nnv[h], sp = spos[h];
				float2 x = xr[h];
				if (!LAT && idx >= 0 && idx < in_len_r && !(QX && hit_r)) {
					x.x -= avr_r;
					x.y -= avi_r;
					if constexpr (QL) {
						// as the staged windows are normalised (a scale no angle below notices; the same numbers whichever
						// way the sample came)
						x.x *= inv_r;
						x.y *= inv_r;
					}
				}
				float s, c;
				sincos_fast(fs_r * (float)idx, s, c);
				x = cmul(x, make_float2(c, s));
				t0[h] = conj_ref_mul(nbits_r, F::sym(bt_r, kind_r, FAC ? (sid_r > 0 ? 1 : 0) : 0, ch, nn, col + 16 * h), x);
				chn[h] = ch;
				spos[h] = sp;
			}
		}
		// chunk sums (pi4cxpsk.c:381-389); the window scale 1/sigma is irrelevant to every angle
		constexpr int NCS = GEN ? 4 : 3;                // chunks a format can have (the fused formats: three)
		if constexpr (!SMALL) if (nch_r > 1) {
			float sumr[NCS], sumi[NCS];
#pragma unroll
			for (int c = 0; c < NCS; c++) {
				const float pr = (chn[0] == c ? t0[0].x : 0.f) + (chn[1] == c ? t0[1].x : 0.f);
				const float pi = (chn[0] == c ? t0[0].y : 0.f) + (chn[1] == c ? t0[1].y : 0.f);
				sumr[c] = row_sum(pr);
				sumi[c] = row_sum(pi);
			}
			float f = 0.f;
#pragma unroll
			for (int i = 1; i < NCS; i++) {
				if (i < nch_r) {
					const float ppos = (float)F::cpos(bt_r, i - 1) + (float)F::clen(bt_r, kind_r, i - 1) / 2.0f;
					const float cpos = (float)F::cpos(bt_r, i) + (float)F::clen(bt_r, kind_r, i) / 2.0f;
					const float re = sumr[i] * sumr[i - 1] - sumi[i] * (-sumi[i - 1]);
					const float im = sumr[i] * (-sumi[i - 1]) + sumi[i] * sumr[i - 1];
					f += atan2_fast(im, re) / (cpos - ppos);
				}
			}
			ffe_r = f / (float)(nch_r - 1);
		}
		// carrier phase of the frequency-corrected sync symbols (pi4cxpsk.c:415-433,574-575)
		float tr = 0.f, ti = 0.f;
#pragma unroll
		for (int h = 0; h < NSH; h++) {
			float2 tt = t0[h];
			if (ffe_r != 0.0f) {
				float s, c;
				sincos_fast(-ffe_r * (float)spos[h], s, c);
				tt = cmul(tt, make_float2(c, s));
			}
			tr += tt.x;
			ti += tt.y;
		}
		psi_r = atan2_fast(row_sum(ti), row_sum(tr));
	}
	if constexpr (PART != 2) {
	GMR1_STAMP(4);
	if (a.dbg_stop == 5) return;

	// per-burst results
	if (col == 0 && row_live && (PART != 1 || io.rv)) {
		const int rv = found_r ? 0 : -1;
		io.rv[g_row] = rv;
		if (io.sync_id) io.sync_id[g_row] = found_r ? sid_r : -1;
		if (io.toa) io.toa[g_row] = found_r ? toa_r : 0.f;
		if (io.freq_err) io.freq_err[g_row] = found_r ? ffe_r : 0.f;
	}
	}
	if constexpr (PART == 1) {
		// (row 0 holds the burst: lane 0's values, for every lane)
		auto first_f = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
		pre->out = {__builtin_amdgcn_readfirstlane(found_r ? 1 : 0), __builtin_amdgcn_readfirstlane(d_r), __builtin_amdgcn_readfirstlane(sid_r),
		            first_f(found_r ? toa_r : 0.f), first_f(found_r ? ffe_r : 0.f), first_f(psi_r), first_f(avr_r), first_f(avi_r)};
		if (lane == 0)
			*pre->cut = {found_r ? 1 : 0, d_r, sid_r, toa_r, ffe_r, psi_r, avr_r, avi_r};
		return;
	}

	// =========================== pass 2: soft symbols / soft bits ===========================
	// the soft-bit table overlays the pass-1 data (fused: where the branch metrics go after pass 2; demodulation
	// only: behind the soft-bit rows, which themselves overlay the correlation the rows above were reading)
	const unsigned char *lut = lds_raw + (GEN ? 4 * EBROW : 0);
	uint2 ord4_q[4] = {};                              // OPS_AHEAD: burst q's g_ord4 entry of this lane
	uint4 st4[2] = {};                                 // OPS_AHEAD: this lane's g_steps4 entries, both chains
	if constexpr (LAT) {
		lut = pre->lut;                             // the work-group's resident copy
		WSYNC();
	} else {
		// the soft-bit table (2 KB, L2-resident) goes to LDS now that the rows are done with the pass-1 data it overlays
		unsigned char *const lutw = lds_raw + (GEN ? 4 * EBROW : 0);
		const uint4 *__restrict__ lut_src = reinterpret_cast<const uint4 *>(FAC ? g_sb_lut1.v : g_sb_lut.v);
		const uint4 lut_a = lut_src[lane], lut_b = lut_src[lane + 64];
		if constexpr (OPS_AHEAD) {
			// (behind the table's loads, which are needed first: loads come back in order)
			const uint2 *__restrict__ ord_src = reinterpret_cast<const uint2 *>(g_ord4.v);
#pragma unroll
			for (int q = 0; q < 4; q++)
				ord4_q[q] = ord_src[(uint32_t)((kind_s[q] ? 64 : 0) + lane)];      // (kind_s: scalars, 0 / 1)
		}
		WSYNC();
		reinterpret_cast<uint4 *>(lutw)[lane] = lut_a;
		reinterpret_cast<uint4 *>(lutw)[lane + 64] = lut_b;
		WSYNC();
	}

	int row_ok = 0, row_chain = 0;
	Sym4 nxt1, nxt2;
	if constexpr (!QX) { nxt1 = first; nxt2 = second; }
#pragma unroll
	for (int q = 3; q >= 0; q--) {
		const int g = g0 + q;
		if constexpr (OPS_AHEAD) {
			// the step descriptors, for the branch metrics behind this loop: eight registers that do not fit beside the
			// four bursts' kept phases in front of it (spills), and do once two bursts' phases are used up
			if (q == kRx4StepsAt) {
				const uint4 *__restrict__ st_src = reinterpret_cast<const uint4 *>(g_steps4.w);
#pragma unroll
				for (int c = 0; c < 2; c++)
					st4[c] = st_src[(uint32_t)(64 * c + lane)];
			}
		}
		Sym4 cur;
		if constexpr (LAT) {
			if (q != 0)
				continue;
			cur = first;
		} else if constexpr (QX) {
			cur.ok = 0;
#pragma unroll
			for (int r = 0; r < NSYM; r++) cur.x[r] = make_float2(0.f, 0.f);
		} else {
			cur = nxt1;
			nxt1 = nxt2;
			fetch(q - 2, nxt2);         // the samples of burst q - 2 travel while q and q - 1 are worked on
		}
		if (g >= n_end)
			continue;
		const int src = 16 * q;
		const bool hit = QX && __builtin_amdgcn_readlane((int)hit_r, src) != 0;
		if constexpr (QX) {
			if (!hit && __builtin_amdgcn_readlane((int)found_r, src) != 0) {
				// the pick is not the speculated one: this burst's kept samples come from memory
				if (q == first_q)
					cur = first;
				else
					fetch(q, cur);
			}
		}
		const bool found = __builtin_amdgcn_readlane((int)found_r, src) != 0;
		const int kind = __builtin_amdgcn_readlane(kind_r, src);
		const int type = GEN ? a.fixed_type : (kind ? GMR1_HIP_DC6 : GMR1_HIP_BCCH);
		const DevBurst &bt = c_types[type];
		const int d = __builtin_amdgcn_readlane(d_r, src);
		const float fs = lane_val(fs_r, src);
		const float rps = -lane_val(ffe_r, src);
		const float psi = lane_val(psi_r, src);
		const float avr = lane_val(avr_r, src), avi = lane_val(avi_r, src);
		const int blen = F::len(bt), nbits = F::nbits(bt);
		float *gss = io.ssyms ? io.ssyms + (size_t)g * a.ssyms_stride : nullptr;
		int8_t *eb = L.eb + q * (GEN ? EBROW : 432);
		row_chain |= kind << q;
		if (!found) {
			// (demodulation only: a row's soft bits and nothing behind them, which is the caller's where the rows lie
			// further apart; the fused path's rows of 432 are zero beyond the format's soft bits)
			if (io.ebits)
				for (int i = lane; i < a.ebits_stride; i += 64)
					if (!GEN || i < bt.ebits)
						io.ebits[(size_t)g * a.ebits_stride + i] = 0;
			if constexpr (GEN)                                  // (a fused decoder reads the LDS row)
				for (int i = lane; i < EBROW / 4; i += 64)
					reinterpret_cast<uint32_t *>(eb)[i] = 0;
			if (gss)
				for (int i = lane; i < blen; i += 64)
					gss[i] = 0.f;
			continue;
		}
		row_ok |= 1 << q;
		// where the soft bits of symbol i go (position of the symbol's bits among the e-bits, -1: sync / guard)
		int ordv[NSYM];
#pragma unroll
		for (int r = 0; r < NSYM; r++) {
			const int i = lane + 64 * r;
			if constexpr (OPS_AHEAD) {
				const uint32_t pair = r < 2 ? ord4_q[q].x : ord4_q[q].y;       // int16 r of the entry, sign-extended
				ordv[r] = (r & 1) ? (int)pair >> 16 : (int)(pair << 16) >> 16;
			} else {
				ordv[r] = i < blen ? bt.ord_of_sym[i] : -1;
			}
		}
		// phase of symbol i in TURNS: arg(x_i) + fs (i sps + d) + rps i - psi  =  arg(x_i) + A i + B
		// (pi4cxpsk.c:351-371 derotation, :574-588 frequency / phase correction, folded into one fma), carried
		// scaled by 2048 (exact): floor(2048 th) & 2046 is the byte offset of the phase's cell in the soft-bit table
		const float kInv2Pi = 0.159154943091895336f;
		const float At = (fs * (float)sps + rps) * kInv2Pi;
		float Bt = (fs * (float)d - psi) * kInv2Pi;
		Bt -= rintf(Bt);
		const float A2 = At * 2048.0f, B2 = Bt * 2048.0f;
		const float scale = (float)(1 << nbits);
		// demodulation only: the soft symbols that go out are formed about the reference's mean (window_mean_serial)
		float2 mref = make_float2(avr, avi);
		if constexpr (GEN) {
			if (gss)
				mref = window_mean_serial(a.iq + io.offset[g], a.in_len[0]);
		}
#pragma unroll
		for (int r = 0; r < NSYM; r++) {
			const int i = lane + 64 * r;
			if (i >= blen)
				continue;
			// (a sample outside the window counts as 0 + 0j, not as minus the mean: the subtraction runs for every lane
			// and the zero test knows which lanes had a sample)
			float2 x = cur.x[r];
			x.x -= avr;
			x.y -= avi;
			float at;
			bool zero;
			if (QX && hit) {
				at = th_q[QX ? q : 0][r];
				zero = ((zm_q >> (4 * q + r)) & 1u) != 0;
			} else {
				at = atan2_turns(x.y, x.x);
				zero = !(cur.ok & (1 << r)) || (x.x == 0.0f && x.y == 0.0f);   // cargf(0) = 0
			}
			const float th2 = fmaf(A2, (float)i, fmaf(at, 2048.0f, B2));
			if (gss) {
				float th = th2 * (1.0f / 2048.0f);
				bool zero_ss = zero;
				if constexpr (GEN) {
					const float xr = cur.x[r].x - mref.x, xi = cur.x[r].y - mref.y;
					th = fmaf(A2, (float)i, fmaf(atan2_turns(xi, xr), 2048.0f, B2)) * (1.0f / 2048.0f);
					zero_ss = !(cur.ok & (1 << r)) || (xr == 0.0f && xi == 0.0f);
				}
				th -= rintf(th);
				gss[i] = zero_ss ? 0.0f : th * scale;
			}
			const int ord = ordv[r];
			if (ord >= 0) {
				int cell;
				asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(cell) : "v"(th2));
				cell = zero ? 0 : (cell & 2046);
				if constexpr (FAC)
					eb[ord] = (int8_t)lut[cell];                   // one soft bit per symbol
				else
					*reinterpret_cast<uint16_t *>(eb + 2 * ord) = *reinterpret_cast<const uint16_t *>(lut + cell);
			}
		}
		if (io.ebits) {
			WSYNC();
			const int neb = bt.ebits;
			int8_t *ge = io.ebits + (size_t)g * a.ebits_stride;
			for (int i = lane; i < a.ebits_stride; i += 64)
				if (!GEN || i < neb)
					ge[i] = i < neb ? eb[i] : (int8_t)0;
		}
	}
	if (GEN || (a.dbg_stop && a.dbg_stop < 7))
		return;
	GMR1_STAMP(5);

	// =========================== rows: layer 1 ===========================
	WSYNC();     // the window is dead: bm / surv / ubits overlay it
	DecPre dpre;
	if constexpr (LAT) {
		// one burst (row 0; what the other rows decode is never looked at), tables from the work-group's LDS copies
		const int chain = row_chain & 1;
		const bool ok = (row_ok & 1) != 0;
#pragma unroll
		for (int it = 0; it < 4; it++) {
			const int k = lane + 64 * it;
			if (k < kSteps12) {
				const uint32_t stw = pre->steps[chain * kSteps12 + k];
				const uint32_t ia = (uint32_t)(uint8_t)L.eb[stw & 0x3ffu] | ((stw >> 2) & 0x100u);
				const uint32_t ib = (uint32_t)(uint8_t)L.eb[(stw >> 16) & 0x3ffu] | ((stw >> 18) & 0x100u);
				lat_expand_step(pre->vtab, k, ok ? pre->cost_a[ia] + pre->cost_b[ib] : 0u);
			}
		}
		dpre.dc = pre->dc; dpre.sy0 = pre->sy0; dpre.sy1 = pre->sy1;
#ifdef GMR1_HIP_PROFILE
		dpre.stamp = io.stamp;
#endif
	} else if constexpr (OPS_AHEAD) {
		// the decoder's per-lane constants are asked for in front of the branch metrics' gathers, not behind them
		dpre.dc = c_dec.v[col];
		dpre.sy0 = *reinterpret_cast<const uint4 *>(&c_syn_rows.w[col][0]);
		dpre.sy1 = *reinterpret_cast<const uint4 *>(&c_syn_rows.w[col][4]);
		branch_metrics4_k5_12<ACC>(L.eb, 432, row_ok, row_chain, L.bm, lane, st4[0], st4[1]);
	} else {
		branch_metrics4_k5_12<ACC>(L.eb, 432, row_ok, row_chain, L.bm, lane);
	}
	WSYNC();
	GMR1_STAMP(6);
	if (a.dbg_stop == 7)
		return;
	if constexpr (PART == 2)
		return;                                     // (the decoder runs on another wave, a round later: k_rx_chain_pipe)
	uint32_t syn, fae;
	if constexpr (LAT)
		decode1_k5_12_lat<ACC>(pre->vtab, L.surv, L.ubits, lane, syn, fae, &dpre);
	else
		decode4_k5_12<ACC>(L.bm, L.surv, L.ubits, lane, syn, fae, OPS_AHEAD ? &dpre : nullptr);
	GMR1_STAMP(7);
	if (col == 0 && row_live) {
		if ((row_ok >> row) & 1) {
			store_l2(io.l2 + (size_t)g_row * 24, L.ubits + row * 8);
			io.crc[g_row] = syn ? 1 : 0;
			io.conv[g_row] = (int32_t)fae;
		} else {
			uint32_t *l2w = reinterpret_cast<uint32_t *>(io.l2 + (size_t)g_row * 24);
#pragma unroll
			for (int i = 0; i < 6; i++)
				l2w[i] = 0;
			io.crc[g_row] = -1;
			io.conv[g_row] = 0;
		}
	}
}

// resident waves per SIMD each instantiation is compiled for: the headline one (windows <= 1024 samples at sps 4) fits six
// without spilling, the run-time-sps one five; the long windows (sps 8: 32 samples per lane) need the registers of three
// (the receive loop's instantiation, EN, keeps the window registers for the burst energy: five)
#ifndef GMR1_EXP_RX4_WAVES
#define GMR1_EXP_RX4_WAVES 6
#endif
template <int NPL, int SPS, bool EN = false>
constexpr int kRx4Waves = NPL > 16 ? 3 : ((SPS == 4 && !EN) ? GMR1_EXP_RX4_WAVES : 5);   // (seven: 72 VGPRs; measured again in round 4 with the LDS of seven -- no gain interleaved, spills and 4 % slower planar)

template <int NPL, int SPS, bool ACC = false, bool EN = false, bool PL = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kRx4Waves<NPL, SPS, EN>, kRx4Waves<NPL, SPS, EN>)))
void k_rx4(RxArgs a, int stage_samples, int cw, int bpw)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	// bpw bursts per wavefront: 4 for throughput; 1 when the batch is too small to fill the machine anyway,
	// which shortens the critical path of a wave to a quarter
	int g0 = blockIdx.x * bpw;
	int n_end = min(a.n, g0 + bpw);
	if (EN && a.seg_count) {
		// bursts listed in segments with unused slots at each segment's end (the receive loop's CCCH lists); with seg_first a
		// launch takes one time slice of every list: block -> (segment, group of four behind the slice's first slot)
		int sg = g0 / a.seg_stride;
		int lo = 0;
		if (a.seg_first) {
			if (a.seg_groups > 0) {
				sg = (int)blockIdx.x / a.seg_groups;
				lo = (a.seg_first[sg] + 3) & ~3;
				g0 = sg * a.seg_stride + lo + ((int)blockIdx.x % a.seg_groups) * bpw;
			} else {
				lo = (a.seg_first[sg] + 3) & ~3;
			}
		}
		const int base = sg * a.seg_stride;
		n_end = min(min(a.n, g0 + bpw), base + min(a.seg_count[sg], a.seg_stride));
		if (g0 >= n_end || g0 < base + lo)
			return;
	}
	const RxIo io = {
#ifdef GMR1_HIP_PROFILE
	                 nullptr,
#endif
	                 a.offset, a.kind, a.freq_shift, a.l2, a.crc, a.conv, a.rv, a.sync_id, a.toa, a.freq_err, a.energy,
	                 a.ebits, a.ssyms};
	rx4_body<CfgBatch<NPL, SPS, ACC, EN, PL, true>>(a, io, stage_samples, cw, g0, n_end, lds_raw, (int)threadIdx.x);
}

// demodulation only, one burst format per launch, four bursts per wavefront (rx4_body<..., GEN>)
template <int NPL, int SPS, bool FAC = false>
__global__ __launch_bounds__(64) void k_rx4g(RxArgs a, int stage_samples, int cw)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int g0 = blockIdx.x * 4;
	const RxIo io = {
#ifdef GMR1_HIP_PROFILE
	                 nullptr,
#endif
	                 a.offset, nullptr, a.freq_shift, nullptr, nullptr, nullptr, a.rv, a.sync_id, a.toa, a.freq_err, a.energy,
	                 a.ebits, a.ssyms};
	rx4_body<CfgDemod<NPL, SPS, FAC>>(a, io, stage_samples, cw, g0, min(a.n, g0 + 4), lds_raw, (int)threadIdx.x);
}

// NT3 speech bursts from samples to speech frames in one launch (what rx_tch3 does with a burst, gmr1_rx.c:551-587:
// gmr1_pi4cxpsk_demod, then gmr1_tch3_decode): the small-format demodulator of four bursts per wavefront, then the TCH3
// decoder (tch3_body.h) on each of the four while their soft bits are still in the wave's LDS rows -- no 212-byte trip to
// HBM and back per burst, one launch, and a compute unit always holds wavefronts in the traffic-bound half next to
// wavefronts in the issue-bound half.
// (resident waves per SIMD: the accelerated decoder's instantiation fits seven -- 72 VGPRs, 5 024 B of LDS -- and gains 2.4 %
// over six; the generic one needs the registers of six)
template <bool ACC>
constexpr int kRx4gTch3Waves = 7;
template <bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kRx4gTch3Waves<ACC>, kRx4gTch3Waves<ACC>))) void k_rx4g_tch3(RxArgs a, Tch3Args t, int stage_samples, int cw)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int g0 = blockIdx.x * 4;
	const int lane = (int)threadIdx.x;
	const int n_end = min(a.n, g0 + 4);
	const RxIo io = {
#ifdef GMR1_HIP_PROFILE
	                 nullptr,
#endif
	                 a.offset, nullptr, a.freq_shift, nullptr, nullptr, nullptr, a.rv, a.sync_id, a.toa, a.freq_err, a.energy,
	                 a.ebits, a.ssyms};
	constexpr int kRow = 216;                    // 212 soft bits + the zero a punctured position reads
	static_assert(CfgTch3Front::EBROW == kRow, "the body's soft-bit rows are the decoder's");
	rx4_body<CfgTch3Front>(a, io, stage_samples, cw, g0, n_end, lds_raw, lane);
	// soft-bit rows of the four bursts at the front of the wave's LDS (kRow bytes apart), the decoder's tables behind them
	t3::Tch3Lds *S = reinterpret_cast<t3::Tch3Lds *>(lds_raw + 4 * kRow);
	WSYNC();
	t3::tch3_fill_locof(S, lane);
	if (lane < 4)
		*reinterpret_cast<uint32_t *>(lds_raw + lane * kRow + 212) = 0;      // byte 212: what a punctured position reads
	t3::Tch3Lane lc;
	t3::tch3_lane(lc, S, lane);
	WSYNC();
	for (int q = 0; q < 4 && g0 + q < n_end; q++) {
		t3::tch3_burst<ACC>(t, g0 + q, lane, reinterpret_cast<const int8_t *>(lds_raw + q * kRow), S, lc);
		WSYNC();
	}
}

#include "rx_small_kernels.h"

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int NPL, int SPS>
static hipError_t launch_rx_t(const RxArgs &a, bool decode, int max_in_len, int max_len, hipStream_t stream)
{
	size_t off[3];
	const size_t lds = lds_layout(max_in_len, max_len, decode, off);
	if (decode) {
		const bool sliced = a.seg_first && a.seg_groups > 0 && a.seg_stride > 0;       // the receive loop's lists, one time slice
		const int grid = sliced ? (a.n / a.seg_stride) * a.seg_groups : (a.n + 3) / 4;
		// (windows beyond 2048 samples -- more than 8 samples per symbol -- exist only in the one-burst-at-a-time body)
		if (a.impl == 1 || NPL > 32) {
			if (a.conv_acc)
				hipLaunchKernelGGL((k_rx<NPL, SPS, true, true>), dim3(grid), dim3(64), lds, stream, a, max_in_len, max_len);
			else
				hipLaunchKernelGGL((k_rx<NPL, SPS, true>), dim3(grid), dim3(64), lds, stream, a, max_in_len, max_len);
		} else if constexpr (NPL <= 32) {
			const int cw = (max_len + 15) & ~15;
			size_t off4[4];
			const size_t lds4 = lds4_layout(a.stage_samples, cw, off4, false, true);
			static size_t pad = (size_t)-1;     // profiling only: extra LDS per wave to cap the occupancy
			if (pad == (size_t)-1) {
				const char *e = profile_env("GMR1_HIP_LDS_PAD");
				pad = e ? (size_t)atoi(e) : 0;
			}
			// small batches (the receive loop's rounds): one burst per wave, four times the waves
			static int bpw_force = -1;          // profiling only: GMR1_HIP_RX_BPW = 1 | 4
			if (bpw_force < 0) {
				const char *e = profile_env("GMR1_HIP_RX_BPW");
				bpw_force = e ? atoi(e) : 0;
			}
			const int bpw = sliced ? 4 : (bpw_force == 1 || bpw_force == 4 ? bpw_force : (a.n <= 4096 ? 1 : 4));
			const int grid4 = sliced ? (a.n / a.seg_stride) * a.seg_groups : (a.n + bpw - 1) / bpw;
			// (the instantiation with the burst energy and the segment bound is the receive loop's: see rx4_body's EN)
			const bool en = a.energy != nullptr || a.seg_count != nullptr;
			if (a.plane_stride) {
				// polyphase-planar sample array: the fused batch kernel at 4 samples per symbol (the host refuses anything else)
				if constexpr (NPL == 16 && SPS == 4) {
					if (en)
						return hipErrorInvalidValue;
					if (a.conv_acc)
						hipLaunchKernelGGL((k_rx4<16, 4, true, false, true>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
					else
						hipLaunchKernelGGL((k_rx4<16, 4, false, false, true>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
				} else
					return hipErrorInvalidValue;
			} else
			if (a.conv_acc) {
				if (en)
					hipLaunchKernelGGL((k_rx4<NPL, SPS, true, true>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
				else
					hipLaunchKernelGGL((k_rx4<NPL, SPS, true, false>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
			} else {
				if (en)
					hipLaunchKernelGGL((k_rx4<NPL, SPS, false, true>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
				else
					hipLaunchKernelGGL((k_rx4<NPL, SPS, false, false>), dim3(grid4), dim3(64), lds4 + pad, stream, a, a.stage_samples, cw, bpw);
			}
		}
	} else {
		hipLaunchKernelGGL((k_rx<NPL, SPS, false>), dim3(a.n), dim3(64), lds, stream, a, max_in_len, max_len);
	}
	return hipGetLastError();
}

hipError_t launch_rx(const RxArgs &a, bool decode, int max_in_len, hipStream_t stream)
{
	if (a.n <= 0)
		return hipSuccess;
	if (max_in_len > kMaxInLen)
		return hipErrorInvalidValue;
	// symbols per burst: fused path is BCCH/DC6 (234); generic path sizes for the longest format
	// third kernel argument: lags the correlation accumulator must hold (fused path: 20*sps + 1)
	// (demodulation only: the lags of this launch's one format, in_len - symbols * sps + 1; ssyms_stride = symbols per burst)
	const int w_demod = a.in_len[0] - a.ssyms_stride * a.sps + 1;
	const int max_len = decode ? (20 * a.sps + 1) : (w_demod > kMaxWindow ? w_demod : kMaxWindow);
	if (!decode && (a.impl == 2 || a.impl == 3 || a.impl == 4) && a.sps == 4 && max_in_len <= 1024) {
		// large batch of one simple burst format (the host checked what rx4_body<GEN> assumes; impl 3: also what its
		// small variant assumes; impl 4: the small variant for two training sequences and BPSK): four bursts per wave
		const int cw1 = (a.in_len[0] - a.ssyms_stride * 4 + 1 + 15) & ~15;      // lags (ssyms_stride = symbols per burst)
		const int cw = a.impl == 4 ? 2 * cw1 : cw1;                            // impl 4: two correlation arrays per burst
		size_t off4[4];
		const size_t lds4 = lds4_layout(a.stage_samples, cw, off4, true);
		const int grid4 = (a.n + 3) / 4;
		if (a.impl == 4)
			hipLaunchKernelGGL((k_rx4g<8, 4, true>), dim3(grid4), dim3(64), lds4, stream, a, a.stage_samples, cw);
		else if (a.impl == 3)
			hipLaunchKernelGGL((k_rx4g<8, 4>), dim3(grid4), dim3(64), lds4, stream, a, a.stage_samples, cw);
		else
			hipLaunchKernelGGL((k_rx4g<16, 4>), dim3(grid4), dim3(64), lds4, stream, a, a.stage_samples, cw);
		return hipGetLastError();
	}
	if (max_in_len <= 1024) {
		if (a.sps == 4)
			return launch_rx_t<16, 4>(a, decode, max_in_len, max_len, stream);
		return launch_rx_t<16, 0>(a, decode, max_in_len, max_len, stream);
	}
	if (max_in_len <= 2048) {
		if (a.sps == 4)
			return launch_rx_t<32, 4>(a, decode, max_in_len, max_len, stream);
		return launch_rx_t<32, 0>(a, decode, max_in_len, max_len, stream);
	}
	return launch_rx_t<64, 0>(a, decode, max_in_len, max_len, stream);
}

#ifdef GMR1_HIP_PROFILE
extern "C" int gmr1_hip_prof_stamps(unsigned long long *out16)
{
	return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamp), sizeof(g_stamp)) == hipSuccess ? 0 : -5;
}
// reads (and clears) the count of mis-speculated picks
extern "C" int gmr1_hip_prof_miss(void)
{
	int v = 0, z = 0;
	if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_prof_miss), sizeof(v)) != hipSuccess)
		return -5;
	hipMemcpyToSymbol(HIP_SYMBOL(g_prof_miss), &z, sizeof(z));
	return v;
}

extern "C" int gmr1_hip_prof_flag(int v)
{
	return hipMemcpyToSymbol(HIP_SYMBOL(g_prof_flag), &v, sizeof(v)) == hipSuccess ? 0 : -5;
}
#endif

hipError_t launch_rx_tch3(const RxArgs &a, const Tch3Args &t, hipStream_t stream)
{
	if (a.n <= 0)
		return hipSuccess;
	if (a.impl != 3 || a.sps != 4 || a.in_len[0] > 512 || a.ebits_stride != 212 || a.n != t.n)
		return hipErrorInvalidValue;
	const int cw = (a.in_len[0] - a.ssyms_stride * 4 + 1 + 15) & ~15;          // lags (ssyms_stride = symbols per burst)
	size_t off4[4];
	// the demodulator's phases as rx4_body<CfgTch3Front> carves them (pass 1: staged windows, correlation,
	// coefficients; pass 2: four 216-byte soft-bit rows and the soft-bit table) -- the same function sizes them here --
	// and, after them, the rows + the decoder's tables
	size_t lds = lds4_layout(a.stage_samples, cw, off4, true, false, 216);
	const size_t need = 4 * 216 + sizeof(t3::Tch3Lds);
	if (lds < need)
		lds = need;
	{
		static size_t pad = (size_t)-1;     // profiling only: extra LDS per wave to cap the occupancy
		if (pad == (size_t)-1) {
			const char *e = profile_env("GMR1_HIP_LDS_PAD");
			pad = e ? (size_t)atoi(e) : 0;
		}
		lds += pad;
	}
	const int grid4 = (a.n + 3) / 4;
	if (t.conv_acc)
		hipLaunchKernelGGL(k_rx4g_tch3<true>, dim3(grid4), dim3(64), lds, stream, a, t, a.stage_samples, cw);
	else
		hipLaunchKernelGGL(k_rx4g_tch3<false>, dim3(grid4), dim3(64), lds, stream, a, t, a.stage_samples, cw);
	return hipGetLastError();
}

#include "rx_loop_kernels.inc"
#include "rx_debug_kernels.inc"
#include "rx_server_kernels.inc"

}  // namespace gmr1
