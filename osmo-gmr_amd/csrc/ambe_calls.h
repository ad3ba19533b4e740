// ambe_calls.h -- what the speech decoder needs to walk the records of the TCH3 call follower (struct gmr1_hip_tch3_frame,
// gmr1_hip.h) instead of a dense block of frames: which records a call owns, and which of them carry speech.  A record
// that does not is what the reference's gmr1_codec_decode_dtx is for (src/codec/ambe.c:130-141): zeros out, the decoder as
// it was.  The device uses it in the calls instantiation of the decoder (k_ambe_calls, ambe_kernels.hip), the C ABI for the
// host form's checks (capi_ambe.cpp); it is host-callable too (tests).  Integer arithmetic only.
#pragma once

#include <stdint.h>

#include "rx_loop.h"

namespace gmr1 {

// struct gmr1_hip_tch3_frame as the decoder sees it (capi_ambe.cpp asserts the offsets against the public struct)
constexpr int kAmbeRecBytes = 40;              // records lie back to back
constexpr int kAmbeRecType = 1;                // uint8_t type
constexpr int kAmbeRecL2 = 16;                 // uint8_t l2[20]: two 10-byte speech frames
constexpr int kAmbeRecFrames = 2;              // speech frames, and verdicts, per record
constexpr int kAmbeRecSpeech = 0x10;           // the type of a record that holds them

struct AmbeSpan { int32_t lo, hi; };           // records lo .. hi - 1; lo == hi: none

// Call c owns first[c] .. first[c + 1] - 1.  first[] of the _dev entries is the caller's device memory: whatever it holds,
// no record index leaves 0..n_frames and hi is never below lo (the follower's rule, tch3_follow_kernels.hip: clamp_frame).
GMR1_HD AmbeSpan ambe_calls_span(const int32_t *first, int c, int n_frames)
{
	const int32_t a = first[c], b = first[c + 1];
	AmbeSpan s;
	s.lo = a < 0 ? 0 : a > n_frames ? n_frames : a;
	s.hi = b < s.lo ? s.lo : b > n_frames ? n_frames : b;
	return s;
}

// The decision reads `type` only: whatever else a record holds (class, length, l2), 0x10 is two speech frames and
// everything else is 320 samples of silence.
GMR1_HD bool ambe_calls_is_speech(unsigned type)
{
	return type == (unsigned)kAmbeRecSpeech;
}

}  // namespace gmr1
