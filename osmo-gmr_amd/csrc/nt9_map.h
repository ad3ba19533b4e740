// nt9_map.h -- the gather maps of the NT9 burst decoders (TCH9 2k4 / 4k8 / 9k6, FACCH9), host code without HIP: for
// every coded bit of every trellis step, where its soft bit sits in the burst -- puncturing, intra- and inter-burst
// de-interleaving, descrambling and demultiplexing folded together from l1_codes.h.  capi_nt9.cpp uploads them,
// tests/test_l1_codes_host.py checks them entry by entry.
#pragma once
#include <vector>

#include "l1_codes.h"

namespace gmr1 {

struct Nt9Kind { int N, len, l2_bytes, intra, x_off, inter; };
constexpr Nt9Kind kNt9Kinds[4] = {
	{5, 144, 18, 81, 0, 1},     // TCH9 2k4: k5_15, tch9.c:56-62
	{3, 240, 30, 81, 0, 1},     // TCH9 4k8: k5_13, tch9.c:64-70
	{2, 480, 60, 81, 0, 1},     // TCH9 9k6: k5_12, tch9.c:72-78
	{2, 316, 38, 80, 4, 0},     // FACCH9:   k5_12 len 316, facch9.c:42-48, 4 + 4 pad bits
};

// One of the two private slots behind gmr1_interleaver::bits_cpp (gmr1_interleaver_init, capi_nt9.cpp), which the stateful
// single-burst TCH9 calls keep their history of two bursts in.  gmr1_tch9_decode: a burst as received, 662 soft bits then
// the 658 key stream bits.  gmr1_tch9_encode (capi_tx_ref.cpp): a burst's payload, the first l2_bytes of the slot.
constexpr int kNt9IlSlot = 662 + 658;

// per unpunctured coded bit of the kind's (len + 4) * N: 1 = not sent (FACCH9 punctures nothing)
inline std::vector<uint8_t> nt9_punctured(int kind)
{
	using namespace l1c;
	const int cl = (kNt9Kinds[kind].len + 4) * kNt9Kinds[kind].N;
	std::vector<uint8_t> p(cl, 0);
	if (kind == 0) punctured_bits(p.data(), cl, scheme(k5_15_P53), scheme(k5_15_P23), scheme(k5_15_Ps53), 41);
	if (kind == 1) punctured_bits(p.data(), cl, scheme(k5_13_P15), scheme(k5_13_P25), scheme(k5_13_Ps15), 41);
	if (kind == 2) punctured_bits(p.data(), cl, scheme(k5_12_P25), scheme(k5_12_P23), scheme(k5_12_Ps25), 158);
	return p;
}

// map entry of a coded bit: bit 31 punctured; else bits 0-9 index into the 662 e-bits, bit 10 the scrambler flips it,
// bits 11-20 index into the 658 bits the key stream covers, bits 21-22 how many bursts back the bit was sent
inline std::vector<uint32_t> nt9_build_map(int kind)
{
	const Nt9Kind &kd = kNt9Kinds[kind];
	const std::vector<uint8_t> punct = nt9_punctured(kind);
	const int cl = (int)punct.size();
	const auto scr = l1c::scramble_seq<648>();   // over the 648 positions of bits_epp_x
	std::vector<uint32_t> map(cl);
	int q = 0;                                   // index into bits_c (the sent coded bits)
	for (int ii = 0; ii < cl; ii++) {
		if (punct[ii]) {
			map[ii] = 0x80000000u;
			continue;
		}
		// bits_c[q] = ep[intra_pos(intra, q)]   (gmr1_deinterleave_intra, interleave.c:73-87)
		const int xi = l1c::intra_pos(kd.intra, q) + kd.x_off;
		const int back = kd.inter ? 2 - (xi % 3) : 0;      // gmr1_deinterleave_inter, N = 3 (interleave.c:163-186)
		const int mi = xi < 52 ? xi : xi + 10;             // bits_my: 52 | sacch 10 | 596
		const int ei = mi < 52 ? mi : mi + 4;              // bits_e:  52 | status 4 | 606
		map[ii] = (uint32_t)ei | (scr.bit[xi] ? 0x400u : 0u) | ((uint32_t)mi << 11) | ((uint32_t)back << 21);
		q++;
	}
	return map;
}

}  // namespace gmr1
