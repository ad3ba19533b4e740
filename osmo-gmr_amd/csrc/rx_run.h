// rx_run.h -- what the translation units of the receive loop share (capi_rx.cpp: the one-shot run; capi_rx_follow.cpp:
// the traffic follow-ups; capi_rx_stream.cpp: the streaming handle).  Host only.
#pragma once

#include "capi_common.h"
#include "rx_follow.h"

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/gmr1_hip.h"

namespace gmr1 {

constexpr int kMaxPeaks = 16;         // gmr1_rx.c:650

// What a chain is: the integers the reference keeps in struct chan_desc.  The streaming handle keeps these across pushes.
struct RxChain {
	int a;                // carrier index
	int chain;            // chain index within the carrier
	uint64_t base;        // first sample of the carrier in iq
	int len;              // samples of the carrier
	int align;
	float freq_err;
	int fn, delay, stn;
	float bcch_energy;
	bool done;
	bool outgrew = false;                // its walk outgrew the loop's buffers (the carrier's status is -EIO)
};

// What one frame_loop plus its follow-ups produce for a chain (walks[i] belongs to chains[i]); it dies with its RxRun
struct RxWalk {
	std::vector<gmr1_hip_rx_record> rec;
	int n_rec = 0;                       // records of the chain when they went straight to the caller (RxRun::direct)
	std::vector<int> rec_frame;          // frame (index into log) each record belongs to
	std::vector<FrameCtx> log;           // one entry per loop iteration of process_bcch (only with a traffic carrier)
	std::vector<AssEvt> events;          // IMMEDIATE ASSIGNMENT taken from the CCCH
	std::vector<AssEvt> events9;         // ASSIGNMENT COMMAND 1 taken from a FACCH3 (frame, tn)
	std::vector<gmr1_hip_rx_big_record> big;
};

// What a chain's TCH3 follow-up carries from one run of tch3_follow_chains to the next: a push of the streaming loop
// continues the call the pushes before it found (the one-shot pass starts from nothing)
struct TchCarry {
	int tn = 0;               // the timeslot of the last assignment
	bool assigned = false;    // there was one
};

// The audio of one run of tch3_follow_chains (gmr1_hip_rx_run_voice*, a push of a voice handle): behind every invocation
// of the call follower its frames are closed up into audio blocks and decoded where they lie (tch3_audio_enqueue,
// capi_ambe.cpp), one AMBE decoder per call, made fresh where the follower's state is assigned.
struct RxVoice {
	void *d_codec = nullptr;             // one decoder state per call in device memory; NULL: the run's own, which die with it
	int *count = nullptr;                // per call: IMMEDIATE ASSIGNMENTs followed before this run, brought up to date by it; NULL: none
	gmr1_hip_rx_audio *out = nullptr;    // host memory: the first max_out blocks, by call, then frame
	int max_out = 0;
	int found = 0;
};

// One call of gmr1_hip_rx_run*, or one push of the streaming loop: what the phases share.  The phases run in the order
// the reference's main() runs them (gmr1_rx.c:897-975).  Which follow-ups run behind the walk is said by what is handed
// in: a one-shot entry's arguments arrive under their names as an RxRunCall (capi_rx.cpp) and a carrier that is there is
// followed; a push's arrive as an RxStreamPush on a handle whose kind (RxStreamKind, rx_stream.h) says it.
struct RxRun {
	hipStream_t st;
	int sps;
	const float *iq, *tch, *csd;
	int A;                                   // carriers
	const uint64_t *offset, *length;
	const uint16_t *arfcn;
	const uint8_t *kc;
	// hand-back of a plain BCCH / CCCH run (no traffic follow-up): the records are closed up on the device in the order
	// they are returned in (k_rx_pack) and copied ONCE, as many as there are -- straight into the caller's buffer when
	// that is device memory or pinned host memory, else through the library's pinned block
	gmr1_hip_rx_record *out;
	int max_records;
	int r = 0;
	std::vector<int32_t> stat, nch;          // per carrier: status, chains followed
	std::vector<RxChain> chains;
	std::vector<RxWalk> walks;
	double t_loop_gpu_us = 0;                // launch to log-on-host
	double t_chain_us = 0;                   // ... of which: launches until the loop's kernels are through (counters on the host)
	bool direct = false;
	int direct_total = 0;
	// the streaming loop (gmr1_hip_rx_stream_*): the chains' states live in this device array across pushes -- the walk
	// starts from and writes back to it, nothing is uploaded
	RxLoopState *loop_state = nullptr;
	RxVoice *voice = nullptr;                // gmr1_hip_rx_run_voice*: the TCH3 pass decodes the calls it follows

	RxRun(hipStream_t st_, int sps_, const float *iq_, const float *tch_, const float *csd_, int A_, const uint64_t *offset_,
	      const uint64_t *length_, const uint16_t *arfcn_, const uint8_t *kc_, gmr1_hip_rx_record *out_, int max_records_)
	    : st(st_), sps(sps_), iq(iq_), tch(tch_), csd(csd_), A(A_), offset(offset_), length(length_), arfcn(arfcn_), kc(kc_),
	      out(out_), max_records(max_records_), stat((size_t)A_, 0), nch((size_t)A_, 0) {}

	int acquire();        // fcch_single_init + fcch_multi_process (capi_rx.cpp)
	int frame_loop();     // process_bcch: BCCH / CCCH, in rounds (capi_rx.cpp)
	int tch3_pass();      // rx_tch3 and its helpers (capi_rx_follow.cpp)
};

// the traffic follow-ups over chains and their walks (capi_rx_follow.cpp)
int tch3_follow_chains(hipStream_t st, int sps, const float *tch, const uint16_t *arfcn, bool want9, bool horizon,
                       const std::vector<RxChain> &chains, std::vector<RxWalk> &walks, const std::vector<int> &calls,
                       const gmr1_hip_tch3_state *h_state0, gmr1_hip_tch3_state *d_state, TchCarry *carry, RxVoice *voice = nullptr);
int tch9_follow_chains(hipStream_t st, int sps, const float *csd, const uint16_t *arfcn, const uint8_t *kc,
                       const std::vector<RxChain> &chains, std::vector<RxWalk> &walks);

// the TCH9 follow-up of one push of the streaming loop: d_state holds one state per chain, carry one entry per chain;
// big_out is host memory
int tch9_follow_push(hipStream_t st, int sps, const float *csd, const uint16_t *arfcn, bool horizon, const std::vector<RxChain> &chains,
                     const std::vector<RxWalk> &walks, gmr1_hip_tch9_state *d_state, Tch9CallCarry *carry,
                     gmr1_hip_rx_big_record *big_out, int max_big, int *n_big);

// what a carrier's records carry: its ARFCN, or its index
inline uint16_t rx_label(const uint16_t *arfcn, int a) { return arfcn ? arfcn[a] : (uint16_t)a; }

// a chain's first state on the device
inline RxLoopState rx_first_state(const RxChain &c, uint16_t label, int done)
{
	return {c.base, c.len, c.align, c.freq_err, c.fn, c.delay, c.stn, done, c.bcch_energy, label, (uint16_t)c.chain};
}

// the calls' first states: no call, not ciphered, the carrier's key (ciphering outlives a re-assignment, gmr1_rx.c:358-376)
inline std::vector<gmr1_hip_tch3_state> tch3_first_states(const std::vector<RxChain> &chains, const std::vector<int> &calls,
                                                          const uint8_t *kc)
{
	std::vector<gmr1_hip_tch3_state> state(calls.size());
	std::memset(state.data(), 0, state.size() * sizeof(gmr1_hip_tch3_state));
	for (size_t q = 0; kc && q < calls.size(); q++)
		std::memcpy(state[q].kc, kc + (size_t)chains[calls[q]].a * 8, 8);
	return state;
}

// records to the caller chain by chain (chains were created carrier by carrier), as many as fit; returns how many there are
inline int rx_hand_back(const std::vector<RxWalk> &walks, gmr1_hip_rx_record *out, int max_records)
{
	int total = 0;
	for (const RxWalk &w : walks) {
		const int cnt = (int)w.rec.size();
		const int fit = std::max(0, std::min(cnt, max_records - total));
		if (fit)
			std::memcpy(out + total, w.rec.data(), (size_t)fit * sizeof(gmr1_hip_rx_record));
		total += cnt;
	}
	return total;
}

// host-side stamps, microseconds
using RxClock = std::chrono::steady_clock;
inline double us_between(RxClock::time_point a, RxClock::time_point b)
{
	return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3;
}
inline double us_since(RxClock::time_point a) { return us_between(a, RxClock::now()); }

}  // namespace gmr1
