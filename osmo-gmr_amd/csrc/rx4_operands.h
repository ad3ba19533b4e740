// rx4_operands.h -- what a lane of the fused batch kernel (k_rx4) needs behind pass 1 that is fixed for the launch and known
// from the burst's kind and the lane alone, packed so that one load fetches what four or more did: where the soft bits of
// the lane's four symbols go (ord4) and the lane's four trellis-step descriptors (steps4).  Plain C++17 without a HIP call:
// the kernels' table makers, the host's upload and tests/c/rx4_operands_host.cpp read this one description.
#pragma once
#include <stdint.h>

#include "gmr1_dev.h"
#include "l1_codes.h"

namespace gmr1 {

static constexpr int kSteps12 = 212;              // 208 data + 4 flush steps (BCCH/CCCH)

// Per trellis step of the BCCH / CCCH chain: where the two soft bits of the step
// sit in the burst's e-bit order and whether the scrambler flips them
//   bits  0..9  index of c[2k]   bit 10 its scrambling bit
//   bits 16..25 index of c[2k+1] bit 26 its scrambling bit
// (interleave.c:73-87 with N=53, scramb.c:39-73; CCCH: 4 leading pad bits, ccch.c:95-96)
struct StepTable { uint32_t w[2][kSteps12]; };
static constexpr StepTable make_steps()
{
	StepTable t{};
	const auto scr = l1c::scramble_seq<448>();        // scrambling sequence over the e-bit positions
	for (int chain = 0; chain < 2; chain++) {
		const int off = chain ? 4 : 0;
		for (int k = 0; k < kSteps12; k++) {
			uint32_t w = 0;
			for (int j = 0; j < 2; j++) {
				const int kc = 2 * k + j;
				const int ei = l1c::intra_pos(53, kc) + off;
				w |= ((uint32_t)ei | (scr.bit[ei] ? 0x400u : 0u)) << (16 * j);
			}
			t.w[chain][k] = w;
		}
	}
	return t;
}

// the fused path's two formats by kind (0: BCCH, 1: CCCH on a DC6 burst); their chains are 0 and 1 as well
constexpr int kRx4Type[2] = {GMR1_HIP_BCCH, GMR1_HIP_DC6};

// steps4.w[chain][lane][it] = c_steps.w[chain][lane + 64 it], 0 where lane + 64 it >= kSteps12: a lane's four step
// descriptors of a chain in one 16-byte load
struct alignas(16) Rx4Steps4 { uint32_t w[2][64][4]; };
static constexpr Rx4Steps4 make_steps4(const StepTable &st)
{
	Rx4Steps4 t{};
	for (int chain = 0; chain < 2; chain++)
		for (int lane = 0; lane < 64; lane++)
			for (int it = 0; it < 4; it++) {
				const int k = lane + 64 * it;
				t.w[chain][lane][it] = k < kSteps12 ? st.w[chain][k] : 0u;
			}
	return t;
}

// ord4.v[kind][lane][r] = ord_of_sym[lane + 64 r] of the kind's format, -1 where lane + 64 r >= its len: the places of a
// lane's four symbols among the data symbols in one 8-byte load (the formats come from the host's burst tables, so this
// one is made at run time, with them)
struct alignas(8) Rx4Ord4 { int16_t v[2][64][4]; };
inline void make_ord4(const DevBurst types[kNumTypes], Rx4Ord4 *out)
{
	for (int kind = 0; kind < 2; kind++) {
		const DevBurst &bt = types[kRx4Type[kind]];
		for (int lane = 0; lane < 64; lane++)
			for (int r = 0; r < 4; r++) {
				const int i = lane + 64 * r;
				out->v[kind][lane][r] = (i < bt.len && i < kMaxLen) ? bt.ord_of_sym[i] : (int16_t)-1;
			}
	}
}

// do the packed tables say what the tables they pack say?  (the fused path does not start otherwise: rx_select.h)
inline bool rx4_ord4_matches(const DevBurst types[kNumTypes], const Rx4Ord4 &o)
{
	for (int kind = 0; kind < 2; kind++) {
		const DevBurst &bt = types[kRx4Type[kind]];
		if (bt.len > 256)                              // four symbols a lane
			return false;
		for (int lane = 0; lane < 64; lane++)
			for (int r = 0; r < 4; r++) {
				const int i = lane + 64 * r;
				if (o.v[kind][lane][r] != (i < bt.len ? bt.ord_of_sym[i] : (int16_t)-1))
					return false;
			}
	}
	return true;
}
inline bool rx4_steps4_matches(const StepTable &st, const Rx4Steps4 &s)
{
	for (int chain = 0; chain < 2; chain++)
		for (int lane = 0; lane < 64; lane++)
			for (int it = 0; it < 4; it++) {
				const int k = lane + 64 * it;
				if (s.w[chain][lane][it] != (k < kSteps12 ? st.w[chain][k] : 0u))
					return false;
			}
	return true;
}

}  // namespace gmr1
