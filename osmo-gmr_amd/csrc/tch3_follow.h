// tch3_follow.h -- the per-frame state machine of rx_tch3 (reference src/gmr1_rx.c:531-600) with its helpers
// _rx_tch3_facch (:454-494) and the bookkeeping half of _rx_tch3_facch_flush (:444-448), over results that were computed
// for the frame beforehand: burst energy, DKAB search, burst type detection, the two demodulators' return values and the
// FACCH3 sync sequence.  The device runs it inside k_tch3f_walk (tch3_follow_kernels.hip; one wavefront walks one call
// through all of its frames); it is host-callable too (tests).  The 104 soft bits of a FACCH3 burst are moved by the
// caller as Tch3Act says.  No signal arithmetic here: the two running averages are the only floating point.
#pragma once

#include <stdint.h>

#include "rx_loop.h"

namespace gmr1 {

// what rx_tch3 did with a frame: the values of GMR1_HIP_TCH3_* (gmr1_hip.h)
constexpr int kT3Off = 0, kT3Dkab = 1, kT3DkabMissing = 2, kT3Facch = 3, kT3Speech = 4, kT3Err = 5;
// the decode a frame asks for
constexpr int kT3NeedNone = 0, kT3NeedSpeech = 1, kT3NeedFlush = 2;

struct Tch3Walk {                          // struct gmr1_hip_tch3_state up to its soft bits, field by field
	int32_t active, p, ciph, weak_cnt, sync_id, burst_cnt;
	float energy_dkab, energy_burst;
	uint32_t bi_fn[4];
};

struct Tch3FrameIn {                       // one frame's speculative results
	float energy;                          // burst_energy of the window
	int32_t dkab_rv;                       // gmr1_dkab_demod at the call's p
	int32_t det_rv, btid;                  // gmr1_pi4cxpsk_detect over {NT3 FACCH, NT3 speech}
	int32_t facch_rv, facch_sid;           // gmr1_pi4cxpsk_demod as an NT3 FACCH burst
	int32_t speech_rv;                     // ... as an NT3 speech burst
	uint32_t fn;
};

struct Tch3Act {
	int cls;                               // kT3Off ..
	int need;                              // kT3NeedNone ..
	int flush;                             // 0 no; 1 the stored bursts go out BEFORE this one is stored (its sync sequence
	                                       // differs); 2 AFTER it (it is the fourth)
	int store;                             // this burst's soft bits go to ebits[104 * bi ..]
	int bi;
	uint32_t job_fn[4];                    // bi_fn as the flush finds it
};

// rx_tch3_init (gmr1_rx.c:358-376) on the state's scalars: ciph, burst_cnt and bi_fn keep what they hold.  The caller clears
// the 416 soft bits (the host entry with a memset, k_tch3f_assign with all lanes).
GMR1_HD void tch3_follow_assign(Tch3Walk &s, int p, float ref_energy)
{
	s.active = 1;
	s.p = p;
	s.energy_burst = ref_energy * 0.75f;
	s.energy_dkab = s.energy_burst / 8.0f;
	s.weak_cnt = 0;
	s.sync_id = 0;
}

GMR1_HD void tch3_follow_flush(Tch3Walk &s, Tch3Act &a, int when)
{
	a.need = kT3NeedFlush;
	a.flush = when;
	for (int i = 0; i < 4; i++) {
		a.job_fn[i] = s.bi_fn[i];
		s.bi_fn[i] = 0xffffffffu;
	}
	s.sync_id ^= 1;
	s.burst_cnt = 0;
}

GMR1_HD Tch3Act tch3_follow_step(Tch3Walk &s, const Tch3FrameIn &f)
{
	Tch3Act a = {kT3Off, kT3NeedNone, 0, 0, 0, {0, 0, 0, 0}};
	if (!s.active)
		return a;
	const float be = f.energy;
	const float det = (s.energy_dkab + s.energy_burst) / 4.0f;
	if (be < det) {
		a.cls = f.dkab_rv < 0 ? kT3Err : f.dkab_rv == 1 ? kT3DkabMissing : kT3Dkab;
		if (f.dkab_rv < 0)
			return a;
		if (f.dkab_rv == 1) {
			if (s.weak_cnt++ > 8)
				s.active = 0;
		} else
			s.energy_dkab = (0.1f * be) + (0.9f * s.energy_dkab);
		return a;
	}
	s.weak_cnt = 0;
	s.energy_burst = (0.1f * be) + (0.9f * s.energy_burst);
	a.cls = kT3Err;
	if (f.det_rv < 0)
		return a;
	if (f.btid == 0) {
		if (f.facch_rv < 0)
			return a;
		a.cls = kT3Facch;
		a.bi = (int)(f.fn & 3u);
		if (f.facch_sid != s.sync_id)
			tch3_follow_flush(s, a, 1);
		a.store = 1;
		s.sync_id = f.facch_sid;
		for (int i = 0; i < 4; i++)            // (not bi_fn[bi]: a register array is never indexed at run time)
			s.bi_fn[i] = i == a.bi ? f.fn : s.bi_fn[i];
		s.burst_cnt += 1;
		if (s.burst_cnt == 4)
			tch3_follow_flush(s, a, 2);
	} else {
		if (f.speech_rv < 0)
			return a;
		a.cls = kT3Speech;
		a.need = kT3NeedSpeech;
	}
	return a;
}

}  // namespace gmr1
