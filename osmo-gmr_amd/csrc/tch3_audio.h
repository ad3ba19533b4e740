// tch3_audio.h -- the close-up of a running call's frames into audio blocks (struct gmr1_hip_rx_audio, gmr1_hip.h): which
// record of the TCH3 call follower gives a block, what a call's label packs, which slot a reporting record takes, and the
// block's 16-byte header.  The device uses it in k_tch3f_audio (tch3_follow_kernels.hip: slots and headers) and in the
// audio instantiation of the decoder (k_ambe_audio, ambe_kernels.hip: where the samples go); the receive loop packs the
// labels with it (capi_rx_follow.cpp); it is host-callable too (tests walk tch3_audio_closeup).  Integer arithmetic only.
#pragma once

#include <stdint.h>

#include "ambe_calls.h"

namespace gmr1 {

// struct gmr1_hip_rx_audio as the kernels see it (capi_ambe.cpp asserts the offsets against the public struct)
constexpr int kAudioBytes = 656;               // blocks lie back to back, each on a 16-byte boundary
constexpr int kAudioRv = 10;                   // int16_t rv[2]
constexpr int kAudioPcm = 16;                  // int16_t pcm[320]
constexpr int kAudioRecCls = 0;                // uint8_t cls of struct gmr1_hip_tch3_frame
constexpr int kAudioClsOff = 0;                // GMR1_HIP_TCH3_OFF
constexpr int32_t kAudioNoSlot = -1;           // the slot of a record that gives no block

// Every frame the follower walked with a call running gives a block, whatever became of it: audio keeps the call's time.
GMR1_HD bool tch3_audio_reports(unsigned cls)
{
	return cls != (unsigned)kAudioClsOff;
}

// a call's label: arfcn | chain << 16 | tn << 24 | call << 32
GMR1_HD uint64_t tch3_audio_label(unsigned arfcn, unsigned chain, unsigned tn, unsigned call)
{
	return (uint64_t)(arfcn & 0xffffu) | ((uint64_t)(chain & 0xffu) << 16) | ((uint64_t)(tn & 0xffu) << 24) |
	       ((uint64_t)(call & 0xffu) << 32);
}

// The slot of the record at position `pos` (0..63) of a step of 64 records: `base` blocks lie in front of the step, `rep`
// has bit j set where the step's record j reports.
GMR1_HD int tch3_audio_slot(int base, uint64_t rep, int pos)
{
	const uint64_t below = rep & ((1ull << pos) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
	return base + __popcll(below);
#else
	return base + __builtin_popcountll(below);
#endif
}

// the header, bytes 0..15 of a block, as four words: arfcn, chain, cls | fn | tn, call, rv[0] = 0 | rv[1] = 0, pad = 0
struct AudioHead { uint32_t w[4]; };
GMR1_HD AudioHead tch3_audio_head(uint64_t label, unsigned cls, uint32_t fn)
{
	AudioHead h;
	h.w[0] = (uint32_t)(label & 0x00ffffffu) | ((cls & 0xffu) << 24);
	h.w[1] = fn;
	h.w[2] = (uint32_t)((label >> 24) & 0xffu) | ((uint32_t)((label >> 32) & 0xffu) << 8);
	h.w[3] = 0;
	return h;
}

// The whole close-up the way the device runs it -- call by call, 64 records a step -- over the records' classes alone:
// slot[k] for every record (kAudioNoSlot where it gives none, and for records no call owns), call_base[c] = blocks in
// front of call c (n_calls + 1 entries, the last one the number found).  first[] is clamped as in the follower.
inline void tch3_audio_closeup(int n_calls, const int32_t *first, int n_frames, const uint8_t *cls, int32_t *slot, int32_t *call_base)
{
	for (int k = 0; k < n_frames; k++)
		slot[k] = kAudioNoSlot;
	int base = 0;
	call_base[0] = 0;
	if (n_calls <= 0)
		return;
	// the blocks in front of a call are those of the records from the first call's first record on (k_tch3f_audio counts them
	// the same way: records are contiguous over calls)
	const int kf = ambe_calls_span(first, 0, n_frames).lo;
	for (int c = 0; c < n_calls; c++) {
		const AmbeSpan s = ambe_calls_span(first, c, n_frames);
		base = 0;
		for (int kb = kf; kb < s.lo; kb += 64) {
			uint64_t rep = 0;
			for (int j = 0; j < 64; j++)
				if (kb + j < s.lo && tch3_audio_reports(cls[kb + j]))
					rep |= 1ull << j;
			base += __builtin_popcountll(rep);
		}
		call_base[c] = base;
		for (int kb = s.lo; kb < s.hi; kb += 64) {
			uint64_t rep = 0;
			for (int j = 0; j < 64; j++)
				if (kb + j < s.hi && tch3_audio_reports(cls[kb + j]))
					rep |= 1ull << j;
			for (int j = 0; j < 64; j++)
				if ((rep >> j) & 1ull)
					slot[kb + j] = tch3_audio_slot(base, rep, j);
			base += __builtin_popcountll(rep);
		}
	}
	call_base[n_calls] = base;
}

}  // namespace gmr1
