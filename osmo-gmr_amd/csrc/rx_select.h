// rx_select.h -- which kernel a demodulation batch gets, and what the fused BCCH / DC6 path asks of the burst tables: the
// host's rules as functions of their inputs.  No HIP call and nothing global, so tests/c/rx_select_host.cpp runs them
// against the built-in tables without a GPU.
#pragma once

#include <cmath>

#include "gmr1_dev.h"
#include "rx4_operands.h"

namespace gmr1 {

inline int window_len(int burst_len, int sps, int win) { return burst_len * sps + win; }

// the window rx_bcch (kind 0) / rx_ccch (kind 1) cut out for a burst (gmr1_rx.c:759, 809)
inline int fused_window_len(int kind, int sps) { return window_len(234, sps, (kind ? 10 : 20) * sps); }

// RxArgs::impl of a demodulation batch of n bursts of format `ht`: 0 = k_rx (one burst per wave), 2 / 3 / 4 = k_rx4g, its
// small-format variant, its two-training-sequence variant, with *stage_samples what that kernel stages of the sync windows
inline int demod_kernel_choice(const DevBurst &ht, int n, int sps, int in_len, int dbg_stop, int *stage_samples)
{
	const int w = in_len - ht.len * sps + 1;
	int impl = 0;
	*stage_samples = 0;
	// Large batches of a simple format (one training sequence, QPSK, <= 3 sync chunks of <= 128 window samples,
	// <= 18 sync symbols, <= 256 symbols; sps 4: NT3 speech, DC2, BCCH, DC6) take the four-bursts-per-wave kernel, where the
	// serial phases of four bursts share their instructions (k_rx4g); everything else, and small batches, one burst per wave.
	if (n > 4096 && sps == 4 && ht.n_sync == 1 && ht.nbits == 2 && ht.n_chunks[0] >= 1 &&
	    ht.n_chunks[0] <= 3 && ht.sync_tl[0] <= 18 && ht.len <= 256 && in_len <= 1024 && w <= 128 && ht.ebits <= 432) {
		bool fits = true;
		int stage = 0;
		for (int c = 0; c < ht.n_chunks[0]; c++) {
			const int wl = ht.sync[0][c].len * sps + w - 1;
			fits &= wl <= 128;
			stage += wl;
		}
		if (fits) {
			// short formats with a single sync chunk (NT3 speech, DC2) have their own instantiation
			const bool small = in_len <= 512 && ht.len <= 128 && ht.n_chunks[0] == 1 && ht.sync_tl[0] <= 16 && stage <= 64;
			impl = small ? 3 : 2;
			*stage_samples = stage;
		}
	}
	// The same kernel's variant for two training sequences of one chunk each at the same place, one bit per symbol (NT3 FACCH)
	if (impl == 0 && n > 4096 && sps == 4 && dbg_stop == 0 && ht.n_sync == 2 && ht.nbits == 1 &&
	    ht.n_chunks[0] == 1 && ht.n_chunks[1] == 1 && ht.sync[0][0].pos == ht.sync[1][0].pos &&
	    ht.sync[0][0].len == ht.sync[1][0].len && ht.sync_tl[0] <= 8 && ht.sync_tl[0] == ht.sync_tl[1] && in_len <= 512 &&
	    ht.len <= 128 && w <= 64 && ht.ebits <= 432) {
		const int stage = ht.sync[0][0].len * sps + w - 1;
		if (stage <= 64) {
			impl = 4;
			*stage_samples = stage;
		}
	}
	return impl;
}

// the two formats of the fused path, by kind
constexpr int kFusedType[2] = {GMR1_HIP_BCCH, GMR1_HIP_DC6};
static_assert(kFusedType[0] == kRx4Type[0] && kFusedType[1] == kRx4Type[1], "the packed operand tables are made for the fused path's formats");

// The fused kernels unroll the sync correlation for these two formats (corr_fixed, rx_kernels.hip) and carry both formats'
// geometry and training symbols as constants (Fmt<false>, rx_kernels.hip; nb.c:36-62, 94-120): is `bt` what they hold for `kind`?
inline bool fused_format_matches(const DevBurst &bt, int kind)
{
	static const int kTaps[2][3] = {{11, 3, 3}, {7, 3, 3}};
	static const int kPos[3] = {28, 119, 197};
	static const uint8_t kSyms[2][17] = {{0, 2, 2, 0, 0, 0, 2, 0, 2, 2, 2, 2, 2, 0, 2, 2, 0}, {0, 0, 0, 2, 2, 0, 2, 0, 3, 0, 3, 1, 1}};
	bool ok = bt.n_sync == 1 && bt.n_chunks[0] == 3 && bt.len == 234 && bt.nbits == 2 && bt.rotation == (float)M_PI / 4.0f &&
	          bt.sync_tl[0] == kTaps[kind][0] + 6;
	for (int c = 0, n = 0; ok && c < 3; c++) {
		ok = bt.sync[0][c].len == kTaps[kind][c] && bt.sync[0][c].pos == kPos[c];
		for (int j = 0; ok && j < kTaps[kind][c]; j++, n++)
			ok = bt.sync[0][c].syms[j] == kSyms[kind][n];
	}
	return ok;
}

inline bool fused_formats_match(const DevBurst types[kNumTypes])
{
	return fused_format_matches(types[kFusedType[0]], 0) && fused_format_matches(types[kFusedType[1]], 1);
}

// The batch kernel reads where a lane's soft bits go and its trellis-step descriptors from packed per-lane copies (g_ord4,
// g_steps4: rx4_operands.h) instead of c_types' ord_of_sym and c_steps: do the copies say what the originals say?
// kHostSteps4 is the host's rendering of the table the kernels are compiled with.
constexpr StepTable kHostSteps = make_steps();
constexpr Rx4Steps4 kHostSteps4 = make_steps4(kHostSteps);
inline bool fused_operands_match(const DevBurst types[kNumTypes], const Rx4Ord4 &ord4, const Rx4Steps4 &steps4)
{
	return rx4_ord4_matches(types, ord4) && rx4_steps4_matches(kHostSteps, steps4);
}

// LDS samples of the sync-chunk windows, sum over chunks of len*sps + w - 1: the larger of the two formats'
inline int fused_stage_samples(const DevBurst types[kNumTypes], int sps)
{
	int stage = 0;
	for (int k = 0; k < 2; k++) {
		const DevBurst &bt = types[kFusedType[k]];
		const int w = fused_window_len(k, sps) - bt.len * sps + 1;
		int tot = 0;
		for (int c = 0; c < bt.n_chunks[0]; c++)
			tot += bt.sync[0][c].len * sps + w - 1;
		if (tot > stage) stage = tot;
	}
	return stage;
}

// RxArgs::impl of a fused launch; env_impl is the profiling switch GMR1_HIP_RX_IMPL (0 in the product build)
inline int fused_impl(int sps, long long plane_stride, int env_impl)
{
	// below four samples per symbol the reference delays the burst by a fraction of a sample with a 21-tap sinc
	// (pi4cxpsk.c:298-343) instead of picking samples: the one-burst-at-a-time body has that branch, the row-batched one not
	if (sps < 4)
		return 1;
	// (the polyphase-planar layout exists in the row-batched kernel only, and at 4 samples per symbol only)
	if (plane_stride)
		return 0;
	return env_impl;
}

}  // namespace gmr1
