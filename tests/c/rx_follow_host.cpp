// Host-side check of the traffic follow-ups' integer rules (osmo-gmr_amd/csrc/rx_follow.h) against the reference's own
// rule, restated here frame by frame as gmr1_rx walks it:
//   TCH3 (gmr1_rx.c:836-841, 881): in each frame the CCCH's IMMEDIATE ASSIGNMENT re-initialises the call first, then rx_tch3
//   runs if a call is active, on the current timeslot; burst_map refuses a window that leaves the carrier.
//   TCH9 (gmr1_rx.c:248-258, 262-353): ASSIGNMENT COMMAND 1 on the FACCH3 activates and re-initialises the interleaver, then
//   rx_tch9 runs in that very frame; sync sequence 0 is a FACCH9, anything else a TCH9 burst that advances the interleaver
//   (restated in rx_tch9_ref.h, which the streaming planner's test shares).  Held against it: the one-shot call's planner,
//   and tch9_plan_push with nothing carried in followed by the call follower's routing (tch9_follow.h) over every segment.
// tests/test_rx_follow_host.py builds and runs it (once more under the address and undefined-behaviour sanitizers).
#include <cstdio>
#include <vector>

#include "rx_follow.h"
#include "rx_tch9_ref.h"
#include "tch9_follow.h"

using namespace gmr1;

#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d, sps %d: %s\n", __LINE__, sps, #x); return 1; } } while (0)

namespace {

struct Call {
	std::vector<FrameCtx> log;
	std::vector<AssEvt> events;
	bool assigned = false;
	int tn = 0;
	int len = 0;
};

// a log of n frames from align a0 on, one frame apart, with a small BCCH correction now and then
std::vector<FrameCtx> make_log(int n, int a0, int sps)
{
	std::vector<FrameCtx> log;
	for (int f = 0; f < n; f++)
		log.push_back({a0 + f * sps * 24 * 39 + (f % 8 == 2 ? 3 : 0), 0.f, 1000 + f});
	return log;
}

using ref9::burst_window;

// gmr1_rx's frame loop over one call: the items, and whether a window ran past the end of the carrier
std::vector<Tch3Item> ref_tch3(int q, const Call &c, int sps, bool *past)
{
	std::vector<Tch3Item> items;
	bool active = c.assigned;
	int tn = c.tn, gen = 0;
	for (int f = 0; f < (int)c.log.size(); f++) {
		for (size_t e = 0; e < c.events.size(); e++)
			if (c.events[e].frame == f) {             // rx_ccch: rx_tch3_init
				active = true;
				tn = c.events[e].tn;
				gen = (int)e + 1;
			}
		if (!active)                                  // rx_tch3: "Is TCH active at all ?"
			continue;
		long long begin;
		bool pe;
		if (burst_window(c.log[f].align, sps, tn, 117, c.len, &begin, &pe))
			items.push_back({q, f, tn, gen});
		*past |= pe;
	}
	return items;
}

bool same(const Tch3Item &a, const Tch3Item &b) { return a.call == b.call && a.frame == b.frame && a.tn == b.tn && a.gen == b.gen; }

// the plan of `calls` against the reference's walk; *out: the plan (valid when 0 is returned and no horizon error is expected)
int check_tch3(const std::vector<Call> &calls, int sps, bool horizon, bool expect_error, Tch3Plan *out)
{
	std::vector<Tch3Call> pc;
	for (const Call &c : calls)
		pc.push_back({&c.log, &c.events, c.assigned, c.tn, c.len});
	const bool ok = tch3_plan(pc, sps, horizon, out);
	std::vector<Tch3Item> want;
	std::vector<size_t> start;
	size_t n_gen = 0;
	bool past = false, any_event = false;
	for (size_t q = 0; q < calls.size(); q++) {
		start.push_back(want.size());
		for (const Tch3Item &t : ref_tch3((int)q, calls[q], sps, &past))
			want.push_back(t);
		any_event |= !calls[q].events.empty();
		if (calls[q].assigned || !calls[q].events.empty())
			n_gen = std::max(n_gen, calls[q].events.size() + 1);
	}
	start.push_back(want.size());
	CHECK(expect_error == (horizon && past));
	CHECK(ok == !expect_error);
	if (!ok)
		return 0;
	CHECK(out->items.size() == want.size());
	for (size_t k = 0; k < want.size(); k++)
		CHECK(same(out->items[k], want[k]));
	CHECK(out->start == start);
	CHECK(out->n_gen == n_gen);
	CHECK(out->any_event == any_event);
	// invocation g holds exactly the g-th assignment's frames of every call: [its frame, the next one's frame), carried-in
	// frames in invocation 0, every one whose window fits and no other
	for (size_t q = 0; q < calls.size(); q++) {
		const Call &c = calls[q];
		for (size_t g = 0; g <= c.events.size(); g++) {
			const int lo = g ? c.events[g - 1].frame : 0;
			int hi = (int)c.log.size();
			for (size_t e = g; e < c.events.size(); e++)        // the next assignment in a LATER OR EQUAL frame ends it
				hi = std::min(hi, c.events[e].frame);
			std::vector<int> frames;
			for (size_t k = out->start[q]; k < out->start[q + 1]; k++)
				if (out->items[k].gen == (int)g)
					frames.push_back(out->items[k].frame);
			for (int f : frames)
				CHECK(f >= lo && f < hi && (g || c.assigned));
			long long begin;
			bool pe;
			int fit = 0;
			for (int f = lo; f < hi; f++)
				fit += (g || c.assigned) && burst_window(c.log[f].align, sps, g ? c.events[g - 1].tn : c.tn, 117, c.len, &begin, &pe);
			CHECK((int)frames.size() == fit);
		}
	}
	return 0;
}

int tch3_cases(int sps)
{
	const int fl = sps * 24 * 39, n = 30, a0 = 5000 * sps;
	const int roomy = a0 + (n + 3) * fl;
	Tch3Plan p;
	Call c;
	c.log = make_log(n, a0, sps);
	c.len = roomy;
	// no event and no carry: nothing
	if (check_tch3({c}, sps, false, false, &p)) return 1;
	CHECK(p.items.empty() && p.n_gen == 0 && !p.any_event);
	// carry only: frames from 0, generation 0
	Call carried = c;
	carried.assigned = true;
	carried.tn = 7;
	if (check_tch3({carried}, sps, true, false, &p)) return 1;
	CHECK((int)p.items.size() == n && p.n_gen == 1 && p.items[0].frame == 0 && p.items[0].gen == 0 && p.items[0].tn == 7);
	// one event
	Call one = c;
	one.events = {{11, 5, 33, 2.f}};
	if (check_tch3({one}, sps, true, false, &p)) return 1;
	CHECK((int)p.items.size() == n - 11 && p.n_gen == 2 && p.items[0].frame == 11 && p.items[0].gen == 1 && p.items[0].tn == 5);
	// ... on top of a call carried in
	Call both = carried;
	both.events = one.events;
	if (check_tch3({both}, sps, true, false, &p)) return 1;
	CHECK((int)p.items.size() == n && p.items[10].gen == 0 && p.items[10].tn == 7 && p.items[11].gen == 1 && p.items[11].tn == 5);
	// an event in frame 0
	Call zero = carried;
	zero.events = {{0, 9, 1, 1.f}};
	if (check_tch3({zero}, sps, true, false, &p)) return 1;
	CHECK((int)p.items.size() == n && p.n_gen == 2 && p.items[0].gen == 1 && p.items[0].tn == 9);
	// two events in the same frame: both applied in order, the first with no frames
	Call twin = c;
	twin.events = {{6, 3, 1, 1.f}, {6, 12, 2, 1.f}, {20, 4, 3, 1.f}};
	if (check_tch3({twin}, sps, true, false, &p)) return 1;
	CHECK(p.n_gen == 4 && p.items[0].frame == 6 && p.items[0].gen == 2 && p.items[0].tn == 12);
	for (const Tch3Item &t : p.items)
		CHECK(t.gen != 1);
	// an assignment whose every window falls off the end of the carrier, then another that fits: both applied, in order
	Call off = c;
	off.len = c.log[n - 1].align + 200 * sps;                       // timeslot 31 of the last frames does not fit, 0 does
	off.events = {{n - 2, 31, 1, 1.f}, {n - 1, 0, 2, 1.f}};
	if (check_tch3({off}, sps, false, false, &p)) return 1;
	CHECK(p.n_gen == 3 && p.items.size() == 1 && p.items[0].gen == 2 && p.items[0].frame == n - 1);
	// ... which is an error when the walk admitted every frame against samples to come
	if (check_tch3({off}, sps, true, true, &p)) return 1;
	// windows with begin < 0 dropped (horizon on or off: only the end is the walk's promise), past the end dropped or an error
	Call early = carried;
	early.tn = 0;
	early.log[0].align = -3 * sps;
	early.log[1].align = -1;
	if (check_tch3({early}, sps, false, false, &p)) return 1;
	CHECK((int)p.items.size() == n - 2 && p.items[0].frame == 2);
	if (check_tch3({early}, sps, true, false, &p)) return 1;
	CHECK((int)p.items.size() == n - 2);
	Call late = carried;
	late.len = c.log[n - 3].align + fl;
	if (check_tch3({late}, sps, false, false, &p)) return 1;
	CHECK(!p.items.empty() && p.items.back().frame < n - 1);
	if (check_tch3({late}, sps, true, true, &p)) return 1;
	// three calls of unequal event counts together (and one without any between them)
	Call three = c;
	three.events = {{2, 1, 1, 1.f}, {9, 2, 2, 1.f}, {17, 30, 3, 1.f}};
	if (check_tch3({one, c, three, both, twin}, sps, false, false, &p)) return 1;
	CHECK(p.n_gen == 4 && p.start[1] == p.start[2]);
	// a pseudo-random mix
	unsigned s = 12345u + (unsigned)sps;
	auto rnd = [&](int m) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)m); };
	for (int round = 0; round < 200; round++) {
		std::vector<Call> calls((size_t)(1 + rnd(4)));
		for (Call &x : calls) {
			const int nf = rnd(40);
			x.log = make_log(nf, rnd(3) ? a0 : rnd(50), sps);
			x.len = rnd(4) ? roomy : a0 + rnd(n + 2) * fl;
			x.assigned = rnd(2) != 0;
			x.tn = rnd(32);
			int f = 0;
			for (int e = rnd(5); e > 0 && nf > 0; e--) {
				f = std::min(nf - 1, f + rnd(8));
				x.events.push_back({f, rnd(32), rnd(64), 1.f});
			}
		}
		bool past = false;
		for (size_t q = 0; q < calls.size(); q++)
			(void)ref_tch3((int)q, calls[q], sps, &past);
		if (check_tch3(calls, sps, false, false, &p)) return 1;
		if (check_tch3(calls, sps, true, past, &p)) return 1;
	}
	return 0;
}

struct Chain9 {
	std::vector<FrameCtx> log;
	std::vector<AssEvt> events9;
	int len = 0;
};

// Both ways the library has of following a whole capture's TCH9 calls against the reference's frame loop (rx_tch9_ref.h):
// what the one-shot call runs, tch9_plan_items / tch9_plan_jobs; and what a push runs, here over the whole log --
// tch9_plan_push with nothing carried in and no horizon, then the follower's routing (tch9_follow.h) over every segment
// from a fresh state, 64 frames a step as the device walks it.  sid / rv of every mapped frame are drawn from sid_in /
// rv_in.  *items_out: the items; *jobs_out: the FACCH9 frames, the TCH9 frames and their positions -- the same from the
// one-shot planner and from the routing (a TCH9 frame's position there: one more than its s1's, 0 where s1 is zeros).
int check_tch9(const std::vector<Chain9> &chains, int sps, const std::vector<int> &sid_in, const std::vector<int> &rv_in,
               std::vector<Nt9Item> *items_out, ref9::Jobs *jobs_out)
{
	std::vector<ref9::Chain> rc;
	std::vector<Tch9PushCall> pc;
	for (const Chain9 &c : chains) {
		rc.push_back({&c.log, &c.events9, c.len});
		pc.push_back({&c.log, &c.events9, Tch9CallCarry(), c.len});
	}
	const std::vector<ref9::Frame> want = ref9::frames(rc, sps);
	Tch9PushPlan plan;
	CHECK(tch9_plan_push(pc, sps, false, &plan));
	// the items are the reference's mapped frames, in order, each in the segment of the command in force
	const std::vector<Nt9Item> &items = plan.items;
	CHECK(items.size() == want.size());
	for (size_t k = 0; k < want.size(); k++) {
		const Chain9 &c = chains[(size_t)want[k].chain];
		CHECK(items[k].chain == want[k].chain && items[k].frame == want[k].frame && items[k].tn == want[k].tn);
		CHECK(want[k].begin == rx_tch9_begin(c.log[(size_t)want[k].frame].align, sps, want[k].tn) &&
		      want[k].begin + rx_tch9_in_len(sps) <= c.len);
		CHECK(items[k].ass >= 0 && items[k].ass < (int)plan.segs.size());
		const Tch9Seg &sg = plan.segs[(size_t)items[k].ass];
		CHECK(sg.chain == want[k].chain && sg.ev == want[k].run + 1 && sg.tn == want[k].tn);
		CHECK(sg.first <= k && (items[k].ass + 1 == (int)plan.segs.size() || k < plan.segs[(size_t)items[k].ass + 1].first));
	}
	// no call is carried in, a segment per command, chain by chain
	size_t n_cmd = 0;
	for (size_t ci = 0; ci < chains.size(); ci++) {
		n_cmd += chains[ci].events9.size();
		CHECK(plan.carry[ci].assigned == !chains[ci].events9.empty());
	}
	CHECK(plan.segs.size() == n_cmd);
	std::vector<int32_t> sid(items.size()), rv(items.size());
	for (size_t k = 0; k < items.size(); k++) {
		sid[k] = sid_in.empty() ? 0 : sid_in[k % sid_in.size()];
		rv[k] = rv_in.empty() ? 0 : rv_in[k % rv_in.size()];
	}
	const ref9::Jobs ref = ref9::jobs(want, sid, rv);
	// the one-shot planner: the same frames, each under the command in force, and the reference's jobs and positions
	{
		std::vector<Nt9Item> one;
		for (size_t ci = 0; ci < chains.size(); ci++)
			tch9_plan_items((int)ci, chains[ci].log, chains[ci].events9, chains[ci].len, sps, &one);
		CHECK(one.size() == want.size());
		for (size_t k = 0; k < want.size(); k++)
			CHECK(one[k].chain == want[k].chain && one[k].frame == want[k].frame && one[k].tn == want[k].tn && one[k].ass == want[k].run);
		const Tch9Jobs jobs = tch9_plan_jobs(one, sid.data(), rv.data());
		CHECK(jobs.facch == ref.facch && jobs.tch == ref.tch);
		CHECK(jobs.pos.size() == ref.pos.size());
		for (size_t i = 0; i < ref.pos.size(); i++)
			CHECK(jobs.pos[i] == ref.pos[i]);
		// the two lists merge back into frame order by item index: every burst once, ascending
		size_t a = 0, b = 0;
		int prev = -1;
		while (a < jobs.facch.size() || b < jobs.tch.size()) {
			const bool take_f = b >= jobs.tch.size() || (a < jobs.facch.size() && jobs.facch[a] < jobs.tch[b]);
			const int i = take_f ? jobs.facch[a++] : jobs.tch[b++];
			CHECK(i > prev && !rv[(size_t)i] && (sid[(size_t)i] == 0) == take_f);
			prev = i;
		}
	}
	// the follower over each segment: rx_tch9_init's state (active, nothing held), then k_tch9f_plan's steps
	std::vector<int> cls(items.size(), -1), s1(items.size(), 0), s2(items.size(), 0);
	for (size_t q = 0; q < plan.segs.size(); q++) {
		const int k0 = (int)plan.segs[q].first, k1 = q + 1 < plan.segs.size() ? (int)plan.segs[q + 1].first : (int)items.size();
		Tch9Carry carry = tch9f_seed(0);
		for (int kb = k0; kb < k1; kb += 64) {
			unsigned long long tch = 0;
			for (int lane = 0; lane < 64 && kb + lane < k1; lane++) {
				cls[(size_t)(kb + lane)] = tch9f_class(1, rv[(size_t)(kb + lane)], sid[(size_t)(kb + lane)]);
				if (cls[(size_t)(kb + lane)] == kT9Tch)
					tch |= 1ull << lane;
			}
			for (int lane = 0; lane < 64 && kb + lane < k1; lane++) {
				const Tch9Carry s = tch9f_sources(tch, lane, kb, carry);
				s1[(size_t)(kb + lane)] = s.s1;
				s2[(size_t)(kb + lane)] = s.s2;
			}
			carry = tch9f_sources(tch, 64, kb, carry);
		}
	}
	// a frame's class is FACCH9, TCH9 or error exactly where the reference says, and it asks for that decode
	ref9::Jobs got;
	size_t a = 0, b = 0;
	std::vector<int> pos_of(items.size(), -1);
	std::vector<int> seg_tch;                                // the TCH9 frames of the segment so far
	for (size_t k = 0; k < items.size(); k++) {
		if (!k || items[k].ass != items[k - 1].ass)
			seg_tch.clear();
		const bool is_f = a < ref.facch.size() && ref.facch[a] == (int)k, is_t = b < ref.tch.size() && ref.tch[b] == (int)k;
		CHECK(cls[k] == (is_f ? kT9Facch : is_t ? kT9Tch : kT9Err));
		CHECK((cls[k] == kT9Err) == (rv[k] != 0));
		CHECK(tch9f_need(cls[k]) == (is_f ? kT9NeedFacch : is_t ? kT9NeedTch : kT9NeedNone));
		if (is_f) {
			got.facch.push_back((int)k);
			a++;
		}
		if (!is_t)
			continue;
		// at reference position pos: the previous two TCH9 frames of the same segment, zeros in front of the run's first
		const int pos = ref.pos[b++];
		CHECK(pos == (int)seg_tch.size());
		CHECK(s1[k] == (pos < 1 ? kT9SrcZeros : seg_tch[(size_t)pos - 1]));
		CHECK(s2[k] == (pos < 2 ? kT9SrcZeros : seg_tch[(size_t)pos - 2]));
		pos_of[k] = s1[k] == kT9SrcZeros ? 0 : pos_of[(size_t)s1[k]] + 1;
		got.tch.push_back((int)k);
		got.pos.push_back(pos_of[k]);
		seg_tch.push_back((int)k);
	}
	CHECK(a == ref.facch.size() && b == ref.tch.size());
	CHECK(got.facch == ref.facch && got.tch == ref.tch && got.pos == ref.pos);
	// the big records come out in item order: chain by chain, and within a chain frame by frame
	for (size_t k = 1; k < items.size(); k++)
		CHECK(items[k].chain > items[k - 1].chain || (items[k].chain == items[k - 1].chain && items[k].frame > items[k - 1].frame));
	if (items_out) *items_out = items;
	if (jobs_out) *jobs_out = got;
	return 0;
}

int tch9_cases(int sps)
{
	const int fl = sps * 24 * 39, n = 24, a0 = 5000 * sps;
	std::vector<Nt9Item> items;
	ref9::Jobs jobs;
	Chain9 c;
	c.log = make_log(n, a0, sps);
	c.len = a0 + (n + 3) * fl;
	// no assignment: nothing
	if (check_tch9({c}, sps, {1}, {0}, &items, &jobs)) return 1;
	CHECK(items.empty() && jobs.facch.empty() && jobs.tch.empty());
	// a re-assignment mid-run restarts positions at 0
	Chain9 re = c;
	re.events9 = {{4, 2, 0, 0.f}, {10, 6, 0, 0.f}};
	if (check_tch9({re}, sps, {1}, {0}, &items, &jobs)) return 1;
	CHECK((int)items.size() == n - 4 && (int)jobs.tch.size() == n - 4 && jobs.facch.empty());
	CHECK(jobs.pos[0] == 0 && jobs.pos[5] == 5 && jobs.pos[6] == 0 && jobs.pos[7] == 1 && items[6].frame == 10 && items[6].tn == 6);
	// a failed demodulation takes no position
	if (check_tch9({re}, sps, {1}, {0, 0, 1, 0, 0}, &items, &jobs)) return 1;
	CHECK(jobs.tch[2] == 3 && jobs.pos[2] == 2 && jobs.tch.size() < items.size());
	// FACCH9 and TCH9 bursts interleaved in frame order: a FACCH9 takes no position either
	if (check_tch9({re}, sps, {1, 0, 1, 1, 0, 0, 1}, {0}, &items, &jobs)) return 1;
	CHECK(jobs.facch[0] == 1 && jobs.tch[1] == 2 && jobs.pos[1] == 1 && jobs.facch.size() + jobs.tch.size() == items.size());
	// several chains, one without an assignment, one whose last windows leave the carrier, two assignments in one frame
	Chain9 cut = re;
	cut.len = c.log[n - 4].align + fl;
	cut.events9 = {{3, 31, 0, 0.f}, {3, 1, 0, 0.f}, {15, 30, 0, 0.f}};
	if (check_tch9({re, c, cut, re}, sps, {1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1}, {0, 0, 0, 0, 0, 0, 1}, &items, &jobs)) return 1;
	CHECK(!items.empty() && items.back().chain == 3);
	unsigned s = 99u + (unsigned)sps;
	auto rnd = [&](int m) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (unsigned)m); };
	for (int round = 0; round < 200; round++) {
		std::vector<Chain9> chains((size_t)(1 + rnd(4)));
		for (Chain9 &x : chains) {
			const int nf = rnd(30);
			x.log = make_log(nf, rnd(3) ? a0 : rnd(50), sps);
			x.len = rnd(3) ? c.len : a0 + rnd(n + 2) * fl;
			int f = 0;
			for (int e = rnd(4); e > 0 && nf > 0; e--) {
				f = std::min(nf - 1, f + rnd(9));
				x.events9.push_back({f, rnd(32), 0, 0.f});
			}
		}
		std::vector<int> sid, rv;
		for (int i = 0; i < 37; i++) {
			sid.push_back(rnd(3) ? 1 : 0);
			rv.push_back(rnd(6) ? 0 : -1);
		}
		if (check_tch9(chains, sps, sid, rv, nullptr, nullptr)) return 1;
	}
	return 0;
}

}  // namespace

int main()
{
	for (int sps : {1, 4, 16})
		if (tch3_cases(sps) || tch9_cases(sps))
			return 1;
	std::printf("ok\n");
	return 0;
}
