// The reference's TCH9 follow-up, restated frame by frame as gmr1_rx walks it (gmr1_rx.c:248-258, 262-353), for the host
// tests of the receive loops' TCH9 planner (rx_follow_host.cpp, rx_stream_full_host.cpp): ASSIGNMENT COMMAND 1 on the
// FACCH3 activates the follow-up, sets the timeslot and re-initialises the interleaver (rx_tch9_init), then rx_tch9 runs in
// that very frame; burst_map refuses a window that leaves the carrier; sync sequence 0 is a FACCH9, anything else a TCH9
// burst, and gmr1_deinterleave_inter only advances on TCH9 bursts.  Nothing of the library's planner is used here.
#pragma once

#include <stdint.h>

#include <vector>

#include "rx_follow.h"

namespace ref9 {

using gmr1::AssEvt;
using gmr1::FrameCtx;

// burst_map (gmr1_rx.c:149-170) of a burst of `syms` symbols with sps + sps / 2 samples of search room: the window or nothing
inline bool burst_window(int align, int sps, int tn, int syms, int len, long long *begin, bool *past_end)
{
	const int win = sps + sps / 2, etoa = win >> 1;
	*begin = (long long)align + (long long)sps * tn * 39 - etoa;
	const long long in_len = (long long)syms * sps + win;
	*past_end = *begin + in_len > len;
	return *begin >= 0 && !*past_end;
}

struct Chain {
	const std::vector<FrameCtx> *log;
	const std::vector<AssEvt> *events9;  // frames counted in the log
	int len;                             // samples of the carrier
};
// a frame in which rx_tch9 maps a burst; run: the command in force (index into the chain's events9), one interleaver life
struct Frame { int chain, frame, tn, run; long long begin; };

// gmr1_rx's frame loop over the chains: the frames rx_tch9 maps, chain by chain
inline std::vector<Frame> frames(const std::vector<Chain> &chains, int sps)
{
	std::vector<Frame> out;
	for (size_t ci = 0; ci < chains.size(); ci++) {
		const Chain &c = chains[ci];
		bool active = false;
		int tn = 0, run = -1;
		for (int f = 0; f < (int)c.log->size(); f++) {
			for (size_t e = 0; e < c.events9->size(); e++)
				if ((*c.events9)[e].frame == f) {         // rx_tch3 -> rx_tch9_init: activate, timeslot, gmr1_interleaver_init
					active = true;
					tn = (*c.events9)[e].tn;
					run = (int)e;
				}
			if (!active)
				continue;
			long long begin;
			bool pe;
			if (!burst_window((*c.log)[f].align, sps, tn, 351, c.len, &begin, &pe))
				continue;
			out.push_back({(int)ci, f, tn, run, begin});
		}
	}
	return out;
}

struct Jobs {
	std::vector<int> facch, tch;         // indices into the mapped frames: FACCH9 bursts, TCH9 bursts
	std::vector<int> pos;                // per TCH9 burst: how many TCH9 bursts its interleaver has taken before it
};

// what rx_tch9 does with every mapped frame, given its demodulation: a failed one is no burst
inline Jobs jobs(const std::vector<Frame> &fr, const std::vector<int32_t> &sync_id, const std::vector<int32_t> &rv)
{
	Jobs j;
	int il = 0;
	for (size_t k = 0; k < fr.size(); k++) {
		if (!k || fr[k].chain != fr[k - 1].chain || fr[k].run != fr[k - 1].run)
			il = 0;                                       // gmr1_interleaver_init at the command
		if (rv[k])
			continue;
		if (sync_id[k] == 0) {
			j.facch.push_back((int)k);
		} else {
			j.tch.push_back((int)k);
			j.pos.push_back(il++);                        // gmr1_deinterleave_inter advances on TCH9 bursts only
		}
	}
	return j;
}

}  // namespace ref9
