// rx_follow.h -- the integer rules of the receive loop's traffic follow-ups (capi_rx_follow.cpp): which frames of which
// chain belong to which assignment, which invocation of the call follower takes them, what a push carries in, and how the
// NT9 bursts of a chain split into FACCH9 jobs and TCH9 interleaver runs.  Host-only, no HIP: the tests walk it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rx_stream.h"

namespace gmr1 {

struct FrameCtx { int align; float freq_err; int fn; };       // what rx_tch3 sees in a frame
struct AssEvt { int frame; int tn, p; float ref_energy; };     // an assignment: IMMEDIATE ASSIGNMENT (CCCH) or ASSIGNMENT COMMAND 1 (FACCH3)

// ---- TCH3 (rx_tch3, gmr1_rx.c:355-600) ----
struct Tch3Call {                      // one chain's walk, as the TCH3 follow-up sees it
	const std::vector<FrameCtx> *log;
	const std::vector<AssEvt> *events;  // in the order the CCCH gave them
	bool assigned;                      // a call carried in from the push before ...
	int tn;                             // ... and its timeslot
	int len;                            // samples of the carrier
};
struct Tch3Item {                      // one frame of a call in which rx_tch3 maps a burst
	int call, frame;
	int tn, gen;                        // the assignment it belongs to: its timeslot; 1 + its index in the events, 0: carried in
};
struct Tch3Plan {
	std::vector<Tch3Item> items;        // call by call, frame by frame
	std::vector<size_t> start;          // per call: its first item (n_calls + 1 entries)
	size_t n_gen = 0;                   // invocations: one per assignment any call sees, and one before them
	bool any_event = false;
};

// IMM.ASS on the CCCH starts the follow-up in that very frame (gmr1_rx.c:235-246, 836-841): invocation g takes, of every
// call, the frames from its g-th assignment up to the next one, invocation 0 those of the call carried in.  A frame whose
// window (rx_tch3_begin, rx_tch3_in_len) does not lie in the carrier is dropped as burst_map drops it -- unless `horizon`
// says the walk admitted every logged frame against samples that more will follow: then a window past the end is an
// error, and the plan says so by returning false.
inline bool tch3_plan(const std::vector<Tch3Call> &calls, int sps, bool horizon, Tch3Plan *out)
{
	const int in_len = rx_tch3_in_len(sps);
	*out = Tch3Plan();
	for (size_t q = 0; q < calls.size(); q++) {
		const Tch3Call &c = calls[q];
		const std::vector<AssEvt> &events = *c.events;
		out->start.push_back(out->items.size());
		out->any_event |= !events.empty();
		int tn = c.assigned ? c.tn : 0;
		if (!c.assigned && events.empty())
			continue;
		out->n_gen = std::max(out->n_gen, events.size() + 1);
		size_t ev = 0;
		for (int f = c.assigned ? 0 : events[0].frame; f < (int)c.log->size(); f++) {
			while (ev < events.size() && events[ev].frame <= f)
				tn = events[ev++].tn;
			const long long begin = rx_tch3_begin((*c.log)[f].align, sps, tn);
			if (begin + in_len > c.len && horizon)
				return false;
			if (begin < 0 || begin + in_len > c.len)
				continue;                     // burst_map fails: rx_tch3 returns before touching anything
			out->items.push_back({(int)q, f, tn, (int)ev});
		}
	}
	out->start.push_back(out->items.size());
	return true;
}

// ---- the audio of the followed calls (gmr1_hip_rx_run_voice*, a voice handle's pushes) ----
// A block's `call` counts the IMMEDIATE ASSIGNMENTs its chain has followed: invocation `gen` of a run (Tch3Item::gen) comes
// behind `gen` of the run's own assignments, on top of the `carried` ones of the pushes before (0 in the one-shot pass).
// The next push is carried what this one was, plus its events: cut anywhere, the counts are the one-shot pass's.
inline int tch3_voice_call(int carried, int gen) { return carried + gen; }
inline int tch3_voice_carry(int carried, size_t n_events) { return carried + (int)n_events; }

// Where a run's blocks go.  Every invocation hands its blocks back call by call, so a run in which one invocation has
// frames -- a chain assigned once, the usual case, and almost every push -- has them in the caller's order already, and
// they are copied from the device straight to the caller.  Otherwise they are kept per invocation and handed back
// call by call, invocation by invocation.
inline size_t tch3_voice_invocations(const Tch3Plan &plan)
{
	std::vector<char> seen(plan.n_gen + 1, 0);
	size_t n = 0;
	for (const Tch3Item &it : plan.items)
		if (!seen[(size_t)it.gen]) {
			seen[(size_t)it.gen] = 1;
			n++;
		}
	return n;
}

// ---- TCH9 (rx_tch9, gmr1_rx.c:262-353) ----
struct Nt9Item { int chain, frame, tn, ass; };     // ass: the ASSIGNMENT COMMAND 1 in force (index into the chain's events)

// the NT9 window of a frame at `align`: burst_map with sps + sps / 2 samples of search room (gmr1_rx.c:290-291)
GMR1_HD int rx_tch9_in_len(int sps) { return 351 * sps + sps + sps / 2; }
GMR1_HD long long rx_tch9_begin(int align, int sps, int tn) { return (long long)align + sps * tn * 39 - ((sps + sps / 2) >> 1); }

// From the frame of a chain's first ASSIGNMENT COMMAND 1 on, every frame whose NT9 window on the assigned timeslot fits
inline void tch9_plan_items(int chain, const std::vector<FrameCtx> &log, const std::vector<AssEvt> &events9, int len, int sps,
                            std::vector<Nt9Item> *items)
{
	if (events9.empty())
		return;
	size_t ev = 0;
	for (int f = events9[0].frame; f < (int)log.size(); f++) {
		while (ev + 1 < events9.size() && events9[ev + 1].frame <= f)
			ev++;
		const int tn = events9[ev].tn;
		const long long begin = rx_tch9_begin(log[f].align, sps, tn);
		if (begin < 0 || begin + rx_tch9_in_len(sps) > len)
			continue;
		items->push_back({chain, f, tn, (int)ev});
	}
}

// ---- TCH9 over a push of the streaming loop (tch9_follow_push, capi_rx_follow.cpp) ----
// What a chain's TCH9 follow-up carries from one push to the next, beside its state on the device
struct Tch9CallCarry {
	int tn = 0;               // the timeslot of the last ASSIGNMENT COMMAND 1
	bool assigned = false;    // there was one
};
struct Tch9PushCall {                  // one chain's walk of this push, as the TCH9 follow-up sees it
	const std::vector<FrameCtx> *log;
	const std::vector<AssEvt> *events9; // this push's commands, frames counted in this push's log
	Tch9CallCarry carry;                   // the call carried in
	int len;                            // samples the carrier holds
};
struct Tch9Seg {                       // one call of the follower's invocation: a stretch of a chain's frames under one command
	int chain;
	int ev;                             // the command: 1 + its index in events9; 0: the call carried in (the chain's own state)
	int tn;
	size_t first;                       // its first item
};
struct Tch9PushPlan {
	std::vector<Nt9Item> items;         // chain by chain, frame by frame; ass: the segment (index into segs)
	std::vector<Tch9Seg> segs;          // chain by chain, in the order of the commands: items are contiguous over them
	std::vector<int> last_seg;          // per chain: the segment whose state the chain keeps, -1: none ran
	std::vector<Tch9CallCarry> carry;      // per chain: what the next push is carried
};

// tch9_plan_items over a capture cut into pushes.  rx_tch9_init leaves a state that depends on nothing before it, so
// every command of the push starts a segment with a fresh state and all segments go into ONE invocation of the follower;
// the frames in front of the push's first command belong to the call carried in (segment 0, only if there is one).  A
// frame moves to the next segment by tch9_plan_items' own rule, events9[ev + 1].frame <= f.  A window that begins before
// the samples is dropped as burst_map drops it; one that ends past them too -- unless `horizon` says more samples follow:
// the walk admitted the frame against them, so that is an error, and the plan returns false.
inline bool tch9_plan_push(const std::vector<Tch9PushCall> &calls, int sps, bool horizon, Tch9PushPlan *out)
{
	const int in_len = rx_tch9_in_len(sps);
	*out = Tch9PushPlan();
	for (size_t q = 0; q < calls.size(); q++) {
		const Tch9PushCall &c = calls[q];
		const std::vector<AssEvt> &ev9 = *c.events9;
		out->carry.push_back(ev9.empty() ? c.carry : Tch9CallCarry{ev9.back().tn, true});
		out->last_seg.push_back(-1);
		if (!c.carry.assigned && ev9.empty())
			continue;
		const size_t seg0 = out->segs.size();
		if (c.carry.assigned)
			out->segs.push_back({(int)q, 0, c.carry.tn, out->items.size()});
		size_t ev = 0;                    // commands applied so far
		for (int f = c.carry.assigned ? 0 : ev9[0].frame; f < (int)c.log->size(); f++) {
			while (ev < ev9.size() && ev9[ev].frame <= f) {
				out->segs.push_back({(int)q, (int)ev + 1, ev9[ev].tn, out->items.size()});
				ev++;
			}
			const int tn = out->segs.back().tn;
			const long long begin = rx_tch9_begin((*c.log)[f].align, sps, tn);
			if (begin + in_len > c.len && horizon)
				return false;
			if (begin < 0 || begin + in_len > c.len)
				continue;
			out->items.push_back({(int)q, f, tn, (int)out->segs.size() - 1});
		}
		// (a command behind the log's last frame cannot be: it came out of a frame of the log; it would still start a segment)
		for (; ev < ev9.size(); ev++)
			out->segs.push_back({(int)q, (int)ev + 1, ev9[ev].tn, out->items.size()});
		if (out->segs.size() > seg0)
			out->last_seg.back() = (int)out->segs.size() - 1;
	}
	return true;
}

struct Tch9Jobs {
	std::vector<int> facch, tch;        // item indices: FACCH9 jobs, TCH9 jobs (run-major: one run per interleaver life)
	std::vector<int32_t> pos;           // per TCH9 job: its position in its run
};

// Sync sequence 0 is a FACCH9, 1 a TCH9; a failed demodulation is no burst (decision D8).  A (re-)assignment at or before
// a frame restarts the interleaver (rx_tch9_init), and gmr1_deinterleave_inter only advances on TCH9 bursts.
inline Tch9Jobs tch9_plan_jobs(const std::vector<Nt9Item> &items, const int32_t *sync_id, const int32_t *rv)
{
	Tch9Jobs j;
	int cur = 0;
	for (size_t k = 0; k < items.size(); k++) {
		if (!k || items[k].chain != items[k - 1].chain || items[k].ass != items[k - 1].ass)
			cur = 0;
		if (rv[k])
			continue;
		if (sync_id[k] == 0) {
			j.facch.push_back((int)k);
		} else {
			j.tch.push_back((int)k);
			j.pos.push_back(cur++);
		}
	}
	return j;
}

}  // namespace gmr1
