// tch9_follow.h -- the routing of rx_tch9 (reference src/gmr1_rx.c:276-353) over the frames of one call: what each frame
// is, and for a TCH9 frame which two earlier bursts the depth-3 inter-burst de-interleaver (gmr1_deinterleave_inter,
// interleave.c:163-186) reads with it.  A frame's class depends on nothing before it, and the de-interleaver only
// advances on TCH9 bursts, so the sources are a scan over "is TCH9": the nearest and the second nearest TCH9 frame below,
// and past the start of the invocation what the call's state holds.  The device runs it 64 frames a step with one ballot
// (k_tch9f_plan, k_tch9f_emit: tch9_follow_kernels.hip); it is host-callable too (tests).  Integer arithmetic only.
#pragma once

#include <stdint.h>

#include "rx_loop.h"

namespace gmr1 {

// what rx_tch9 did with a frame: the values of GMR1_HIP_TCH9_* (gmr1_hip.h)
constexpr int kT9Off = 0, kT9Facch = 1, kT9Tch = 2, kT9Err = 3;
// the decode a frame asks for
constexpr int kT9NeedNone = 0, kT9NeedFacch = 1, kT9NeedTch = 2;
// a source of the de-interleaver: a frame index of this invocation (>= 0), or
constexpr int32_t kT9SrcZeros = -1, kT9SrcHeld0 = -2, kT9SrcHeld1 = -3;      // held slot s is -2 - s

// A failed demodulation is no burst (decision D8, as tch9_plan_jobs); sync sequence 0 is a FACCH9, any other a TCH9
GMR1_HD int tch9f_class(int active, int rv, int sync_id)
{
	return !active ? kT9Off : rv ? kT9Err : sync_id == 0 ? kT9Facch : kT9Tch;
}
GMR1_HD int tch9f_need(int cls)
{
	return cls == kT9Facch ? kT9NeedFacch : cls == kT9Tch ? kT9NeedTch : kT9NeedNone;
}

// the last two TCH9 bursts in front of a step: s1 the previous one, s2 the one before it
struct Tch9Carry { int32_t s1, s2; };

// in front of the invocation's first frame: what the state holds (n_held is the caller's memory: anything counts as 0..2)
GMR1_HD Tch9Carry tch9f_seed(int n_held)
{
	Tch9Carry c;
	c.s1 = n_held >= 1 ? kT9SrcHeld0 : kT9SrcZeros;
	c.s2 = n_held >= 2 ? kT9SrcHeld1 : kT9SrcZeros;
	return c;
}

GMR1_HD int tch9f_top_bit(unsigned long long m) { return 63 - __builtin_clzll(m); }      // m != 0

// Lane `lane` of a step over the frames base .. base + 63, `tch` = the lanes that are TCH9 frames: the burst one back and
// two back of that lane.  lane 64 is the frame behind the step: what the next step is carried.
GMR1_HD Tch9Carry tch9f_sources(unsigned long long tch, int lane, int base, Tch9Carry c)
{
	unsigned long long below = lane >= 64 ? tch : tch & ((1ull << lane) - 1ull);
	if (!below)
		return c;
	Tch9Carry r;
	const int h = tch9f_top_bit(below);
	r.s1 = base + h;
	below &= ~(1ull << h);
	r.s2 = below ? base + tch9f_top_bit(below) : c.s1;
	return r;
}

// n_held after the invocation, from the carry behind its last frame
GMR1_HD int tch9f_n_held(Tch9Carry c)
{
	return (c.s1 != kT9SrcZeros) + (c.s2 != kT9SrcZeros);
}

// where bit i of bits_e sits in the 658-bit cipher stream (tch9.c:152-160), -1: a status bit, not ciphered
GMR1_HD int tch9f_e2my(int i)
{
	return i < 52 ? i : i < 56 ? -1 : i - 4;
}

}  // namespace gmr1
