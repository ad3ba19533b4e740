// rx_stream.h -- the integer arithmetic of the streaming receive loop (gmr1_hip_rx_stream_*, capi_rx_stream.cpp): when the
// acquisition may run, what a carrier keeps between pushes, how the chain states move with it.  Host-callable (tests,
// sizing) and used by the staging kernel (rx_stream_kernels.hip).  No signal arithmetic here.
#pragma once

#include <stdint.h>

#include "rx_loop.h"

namespace gmr1 {

constexpr int kRxStartDiscard = 8000;      // gmr1_rx.c:52
constexpr int kRxKeepAlign = 64;           // a carrier drops whole multiples of this many samples

// chain states between pushes (RxLoopState::done): 0 walking, 1 stopped by rx_loop_advance's check against the samples
// available (provisional until the last push), 2 acquired but not yet started, 3 stopped for good (outgrew its buffers)
constexpr int kRxDoneStopped = 1, kRxDoneUnstarted = 2, kRxDoneFinal = 3;

GMR1_HD int rx_stream_frame_len(int sps) { return sps * 24 * 39; }

// Samples a carrier needs before its FCCH acquisition (RxRun::acquire) decides as it would on any longer capture.
// Every bound check there compares an end position with the carrier's length, and every sweep reads inside a window a
// check admitted.  With wl1 = 330 ms, wl3 = 650 ms, flen = 117 sps, toa1 <= wl1 - flen (the rough sweep's last lag),
// |ftoa|, |ctoa| < flen (the fine stage's chirp offset: at most 58 bins / 2 over the chirp rate, 91 sps) and rough-multi
// peaks <= wl3 - flen, the largest end any check compares is
//   kStartDiscard + toa1 + ftoa - flen + peak + ctoa + flen  <=  kStartDiscard + wl1 + wl3 - flen + flen
// and H_acq adds three FCCH lengths of margin on top of that.
GMR1_HD long long rx_stream_acq_need(int sps)
{
	const long long wl1 = (330LL * 23400 * sps) / 1000, wl3 = (650LL * 23400 * sps) / 1000, flen = 117LL * sps;
	return kRxStartDiscard + wl1 + wl3 + 3 * flen;
}

// How far back of a chain's align a window of the walk can start: a window begins at most 10 sps before align
// (burst_map's etoa), and over any stretch of frames bcch_tdma_align's shifts (stn_old - stn_new) * 39 * sps telescope to
// at most 31 * 39 * sps (stn is a 5-bit field) while every frame adds frame_len and a BCCH correction takes at most 10 sps
// of it back.  The handle keeps 2 * frame_len > (31 * 39 + 10) * sps before the earliest align.
GMR1_HD int rx_stream_reach_back(int sps) { return (31 * 39 + 10) * sps; }

// First sample a carrier keeps, given the smallest align of its chains (its own coordinates)
GMR1_HD long long rx_stream_keep_from(long long min_align, int sps)
{
	long long k = min_align - 2LL * rx_stream_frame_len(sps);
	if (k < 0) k = 0;
	return k - k % kRxKeepAlign;
}

// What the loop may do with a chain once its carrier holds `len` samples: a chain that has not started walks only when
// its first frame passes rx_loop_advance's check (or on the last push, as gmr1_rx processes the first frame unchecked);
// a stopped one resumes only when the frame it stopped at passes it.
GMR1_HD int rx_stream_next_done(int done, int align, int len, int sps, int last)
{
	const bool fits = (long long)align + 2LL * rx_stream_frame_len(sps) <= (long long)len;
	if (done == kRxDoneUnstarted && (last || fits)) return 0;
	if (done == kRxDoneStopped && fits) return 0;
	return done;
}

// Frames a walk over `len` samples can log per chain: the per-chain frame log of RxRun::frame_loop
GMR1_HD long long rx_stream_frames_per_chain(long long len, int sps) { return len / rx_stream_frame_len(sps) + 2; }

// Records a walk over `len` samples can hand back per chain: the per-chain record buffer of RxRun::frame_loop
GMR1_HD long long rx_stream_rec_per_chain(long long len, int sps)
{
	return (rx_stream_frames_per_chain(len, sps) / 7 + 8) * kLoopPerRound;
}

// The window rx_tch3 cuts on the traffic carrier for a frame at `align` (burst_map of an NT3 burst with sps + sps / 2
// samples of search room, gmr1_rx.c:149-170, 549-551): [begin, begin + in_len).  rx_tch3 returns before it touches
// anything when begin < 0 or begin + in_len > len.  One rule for the one-shot pass and the streaming push.
GMR1_HD int rx_tch3_in_len(int sps) { return 117 * sps + sps + sps / 2; }
GMR1_HD long long rx_tch3_begin(int align, int sps, int tn) { return (long long)align + sps * tn * 39 - ((sps + sps / 2) >> 1); }

// A tch handle hands back, on top of the BCCH / CCCH records, at most one TCH3 record per frame a chain's walk logs
GMR1_HD long long rx_stream_tch_rec_per_chain(long long len, int sps)
{
	return rx_stream_rec_per_chain(len, sps) + rx_stream_frames_per_chain(len, sps);
}

// ---- what a handle follows ----
// plain: BCCH / CCCH only; tch: TCH3 calls as well; full: TCH3 and TCH9 calls; voice: TCH3 calls, decoded to audio
constexpr int kRxStreamPlain = 0, kRxStreamTch = 1, kRxStreamFull = 2, kRxStreamVoice = 3;
constexpr int kRxStreamKinds = 4;
constexpr int kRxStreamMaxPlanes = 3;

// A kind, described once: the handle, its entries and their messages ask this and nothing else (host only)
struct RxStreamKind {
	int planes;                  // carriers a push brings: the BCCH carrier, the traffic carrier, the CSD carrier
	bool tch3, tch9, audio;      // follows TCH3 calls; follows TCH9 calls; decodes the TCH3 calls it follows
	const char *maker, *entry;   // who makes such a handle and who pushes to it
};
inline constexpr RxStreamKind kRxStreamKind[kRxStreamKinds] = {
	{1, false, false, false, "gmr1_hip_rx_stream_create", "gmr1_hip_rx_stream_push*"},
	{2, true, false, false, "gmr1_hip_rx_stream_create_tch", "gmr1_hip_rx_stream_push_tch*"},
	{3, true, true, false, "gmr1_hip_rx_stream_create_full", "gmr1_hip_rx_stream_push_full*"},
	{2, true, false, true, "gmr1_hip_rx_stream_create_voice", "gmr1_hip_rx_stream_push_voice*"},
};
inline const RxStreamKind &rx_stream_kind(int kind) { return kRxStreamKind[kind]; }

// The window rx_tch9 cuts on the CSD carrier is 351 * sps + sps + sps / 2 samples (rx_tch9_in_len, rx_follow.h), and the
// demodulator takes windows up to kMaxInLen: the largest sps a full handle can be made for
GMR1_HD int rx_stream_full_max_sps() { return 11; }

// Beside its records a handle hands back at most one more thing per frame a chain's walk can log: a full handle a big
// record (FACCH9 / TCH9), a voice handle an audio block
GMR1_HD long long rx_stream_max_big(long long chains, long long len, int sps)
{
	return chains > 0 ? chains * rx_stream_frames_per_chain(len, sps) : 0;
}
GMR1_HD long long rx_stream_max_audio(long long chains, long long len, int sps) { return rx_stream_max_big(chains, len, sps); }

}  // namespace gmr1
