// Intermediate signals of one burst's demodulation, for parity debugging on someone else's capture.
// (part of rx_kernels.hip's translation unit, included by it after rx_loop_kernels.inc, inside namespace gmr1)
//
// The reference dumps four vectors per gmr1_pi4cxpsk_demod call when it is built with ENABLE_DEBUG_SIGNAL
// (include/osmocom/gmr1/sdr/defs.h:35-39): "pi4cxpsk_corr" (pi4cxpsk.c:251), "pi4cxpsk_align" (:345),
// "pi4cxpsk_burst" (:545) and "pi4cxpsk_final" (:582).  The production kernels never form three of them -- after
// the sync search they work on phases (see demod_one) -- so this kernel runs the very same demod_one on one burst and
// then REBUILDS the four vectors from what demod_one left in LDS and from its outputs:
//   burst[n] = x[n] e^{j fs n}                 x = the normalised window, fs = (freq_shift - rotation) / sps
//   corr[m]  = the sync search's accumulator   (one training sequence: |correlation| at lag m; several: their sum, as
//                                               after the LAST sequence -- the reference's file holds the state at the
//                                               last sequence that took the lead)
//   align[i] = burst[i sps + round(toa)]       (below 4 samples per symbol: after the 21-tap fractional delay)
//   final[i] = |align[i]| e^{j 2 pi ssym[i] / 2^nbits}     i.e. align after the fine-frequency and carrier rotations
// One wave, one burst, no claim to speed.

}  // namespace gmr1 (left for the header, which opens it itself)
#include "rx_debug.h"
namespace gmr1 {

template <int NPL, int SPS>
__global__ __launch_bounds__(64) void k_rx_taps(RxArgs a, RxTapsOut o, int max_in_len, int max_len)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int lane = threadIdx.x;
	const Lds L = lds_carve(lds_raw, max_in_len, max_len, false);
	const int type = __builtin_amdgcn_readfirstlane(a.fixed_type);
	const int in_len = __builtin_amdgcn_readfirstlane(a.in_len[0]);
	const DevBurst &bt = c_types[type];
	const int sps = a.sps, blen = bt.len, nbits = bt.nbits;
	const int w = in_len - blen * sps + 1;
	const float fsh = a.freq_shift ? a.freq_shift[0] : 0.0f;
	int sid = -1;
	float toa = 0.f, fe = 0.f;

	const int rv = demod_one<NPL, SPS>(type, a.iq + a.offset[0], in_len, sps, fsh, L, L.eb, lane, 0, sid, toa, fe, a.ssyms);
	WSYNC();
	if (lane == 0) {
		a.rv[0] = rv;
		if (a.sync_id) a.sync_id[0] = sid;
		if (a.toa) a.toa[0] = rv ? 0.f : toa;
		if (a.freq_err) a.freq_err[0] = rv ? 0.f : fe;
	}
	if (a.ebits)
		for (int i = lane; i < a.ebits_stride; i += 64)
			a.ebits[i] = (rv == 0 && i < bt.ebits) ? L.eb[i] : (int8_t)0;

	const float fs = (fsh - bt.rotation) / (float)sps;
	auto rot = [&](float2 x, int n) -> float2 {
		float s, c;
		sincosf(fs * (float)n, &s, &c);
		return make_float2(x.x * c - x.y * s, x.x * s + x.y * c);
	};
	for (int n = lane; n < in_len; n += 64)
		o.burst[n] = rot(L.x[n], n);
	for (int m = lane; m < w; m += 64)
		o.corr[m] = L.corr[m];
	if (rv) {
		// no training sequence had power: the reference returns before it aligns anything
		for (int i = lane; i < blen; i += 64) {
			o.align[i] = o.final_[i] = make_float2(0.f, 0.f);
			if (a.ssyms) a.ssyms[i] = 0.f;
		}
		return;
	}
	const int d = (int)roundf(toa);
	const float frac = toa - (float)d;
	const bool frac_on = (sps < 4) && (fabsf(frac) > 0.1f);     // demod_one left its 21 rotated taps in L.coef
	const float step = 2.0f * kPif / (float)(1 << nbits);
	for (int i = lane; i < blen; i += 64) {
		const int j = i * sps + d;
		float2 x = make_float2(0.f, 0.f);
		if (j >= 0 && j < in_len) {
			x = frac_on ? delayed_sample(L, fs, j, in_len) : L.x[j];
		}
		const float2 al = rot(x, j);
		o.align[i] = al;
		const float mag = sqrtf(al.x * al.x + al.y * al.y);
		float s, c;
		sincosf(a.ssyms[i] * step, &s, &c);
		o.final_[i] = make_float2(mag * c, mag * s);
	}
}

// (a.n == 1, a.ssyms required; `o` device pointers)
hipError_t launch_rx_taps(const RxArgs &a, const RxTapsOut &o, hipStream_t stream)
{
	const int in_len = a.in_len[0];
	if (a.n != 1 || !a.ssyms || !a.rv || in_len > kMaxInLen)
		return hipErrorInvalidValue;
	const int w = in_len - a.ssyms_stride * a.sps + 1;
	const int max_len = w > kMaxWindow ? w : kMaxWindow;
	size_t off[3];
	const size_t lds = lds_layout(in_len, max_len, false, off);
	// (the instantiations launch_rx picks for the same window, so that the ordinary outputs are the batch entry's to the bit)
#define GMR1_TAPS(NPL, SPS) hipLaunchKernelGGL((k_rx_taps<NPL, SPS>), dim3(1), dim3(64), lds, stream, a, o, in_len, max_len)
	if (in_len <= 1024) {
		if (a.sps == 4) GMR1_TAPS(16, 4); else GMR1_TAPS(16, 0);
	} else if (in_len <= 2048) {
		if (a.sps == 4) GMR1_TAPS(32, 4); else GMR1_TAPS(32, 0);
	} else {
		GMR1_TAPS(64, 0);
	}
#undef GMR1_TAPS
	return hipGetLastError();
}
