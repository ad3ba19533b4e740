// Host-side check of what lets the streaming receive loop follow TCH9 data calls (osmo-gmr_amd/csrc/rx_follow.h,
// rx_stream.h): tch9_plan_push over a frame log cut into pushes gives, concatenated, the frames the
// reference's own frame loop maps on the whole log (restated in rx_tch9_ref.h), with a new segment exactly where the
// command in force changes and interleaver positions that are the reference's; the NT9 window of a frame the walk admitted lies inside the samples held; the big-record bound, the audio bound that is the same one, and the one description of the four kinds of handle.
// tests/test_rx_stream_full_host.py builds and runs it, plain and under the address / undefined-behaviour sanitizers.
#include <cstdio>
#include <random>

#include "rx_follow.h"
#include "rx_tch9_ref.h"

using namespace gmr1;

static int g_sps = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d, sps %d: %s\n", __LINE__, g_sps, #x); return 1; } } while (0)

namespace {

struct Capture {
	std::vector<FrameCtx> log;
	std::vector<AssEvt> ev9;       // frames counted in the whole log
	int len = 0;
	int n_adm = 0;                 // frames a push that is not the last can hold: align + 2 frame_len <= len
};

Capture make_capture(std::mt19937 &rng, int sps, int n_frames, const std::vector<int> &cmd_frames)
{
	const int fl = rx_stream_frame_len(sps);
	Capture c;
	int align = (int)(rng() % (unsigned)(3 * sps + 1));           // (the first windows may begin before the samples)
	for (int f = 0; f < n_frames; f++) {
		c.log.push_back({align, 0.f, 1000 + f});
		align += fl + (int)(rng() % (unsigned)(2 * sps + 1)) - sps;
	}
	// the capture ends inside the last frames' reach: on timeslots high enough their windows pass the end
	c.len = c.log.back().align + fl / 2 + (int)(rng() % (unsigned)fl);
	for (int f : cmd_frames)
		c.ev9.push_back({f, (int)(rng() % 32u), 0, 0.f});
	for (const FrameCtx &x : c.log)
		if ((long long)x.align + 2LL * fl <= c.len)
			c.n_adm++;
	return c;
}

// the log cut at `cuts` (ascending frame indices, all <= n_adm) and planned push by push: every item must be the
// reference's, in order, and its run (the command in force, counted over the whole capture) the reference's
int streamed_is_one_shot(const Capture &c, int sps, const std::vector<int> &cuts, const std::vector<ref9::Frame> &want,
                         const ref9::Jobs &want_jobs, const std::vector<int32_t> &sync_id, const std::vector<int32_t> &rv)
{
	const int fl = rx_stream_frame_len(sps);
	const int n = (int)c.log.size();
	Tch9CallCarry carry;
	size_t at = 0, ev_done = 0, job = 0;
	int run_in = -1;                       // the run the carried call belongs to
	int pos_run = -1, pos = 0;             // what a call's state carries: TCH9 bursts of its run so far
	std::vector<int> bounds(cuts);
	bounds.push_back(n);
	int a = 0;
	for (size_t p = 0; p < bounds.size(); p++) {
		const int b = bounds[p];
		const bool last = p + 1 == bounds.size();
		const std::vector<FrameCtx> log(c.log.begin() + a, c.log.begin() + b);
		std::vector<AssEvt> ev9;
		const size_t ev_first = ev_done;
		for (; ev_done < c.ev9.size() && c.ev9[ev_done].frame < b; ev_done++) {
			AssEvt e = c.ev9[ev_done];
			e.frame -= a;
			ev9.push_back(e);
		}
		// a push that is not the last holds what its newest frame was admitted against
		const int len = last ? c.len : (b > a ? c.log[b - 1].align + 2 * fl : c.log[a ? a - 1 : 0].align + 2 * fl);
		CHECK(last || len <= c.len);
		Tch9PushPlan plan;
		CHECK(tch9_plan_push({{&log, &ev9, carry, len}}, sps, !last, &plan));
		CHECK(plan.carry.size() == 1 && plan.last_seg.size() == 1);
		// the carry: assigned once any command has come, its timeslot the last command's
		CHECK(plan.carry[0].assigned == (ev_done > 0));
		CHECK(!ev_done || plan.carry[0].tn == c.ev9[ev_done - 1].tn);
		// the segments: one for the call carried in, one per command, in order; the last one is what the chain keeps
		CHECK(plan.segs.size() == (carry.assigned ? 1u : 0u) + ev9.size());
		CHECK(plan.last_seg[0] == (int)plan.segs.size() - 1);
		for (size_t s = 0; s < plan.segs.size(); s++) {
			const Tch9Seg &sg = plan.segs[s];
			CHECK(sg.chain == 0 && sg.ev == (int)s + (carry.assigned ? 0 : 1));
			CHECK(sg.tn == (sg.ev ? ev9[sg.ev - 1].tn : carry.tn));
			CHECK(sg.first <= plan.items.size() && (!s || plan.segs[s - 1].first <= sg.first));
		}
		for (size_t k = 0; k < plan.items.size(); k++, at++) {
			const Nt9Item &it = plan.items[k];
			CHECK(at < want.size());
			CHECK(it.chain == 0 && it.frame + a == want[at].frame && it.tn == want[at].tn);
			const Tch9Seg &sg = plan.segs[it.ass];
			CHECK(sg.first <= k && (it.ass + 1 == (int)plan.segs.size() || k < plan.segs[it.ass + 1].first));
			CHECK(it.tn == sg.tn);
			const int run = sg.ev ? (int)ev_first + sg.ev - 1 : run_in;
			CHECK(run == want[at].run);
			// a fresh state where the run changes, the carried one otherwise
			if (run != pos_run) {
				pos_run = run;
				pos = 0;
			}
			if (!rv[at] && sync_id[at] != 0) {
				CHECK(job < want_jobs.tch.size() && want_jobs.tch[job] == (int)at && want_jobs.pos[job] == pos);
				job++;
				pos++;
			}
		}
		carry = plan.carry[0];
		if (ev_done)
			run_in = (int)ev_done - 1;
		a = b;
	}
	CHECK(at == want.size() && job == want_jobs.tch.size());
	return 0;
}

int planner(int sps)
{
	std::mt19937 rng(1234u + (unsigned)sps);
	for (int round = 0; round < 40; round++) {
		const int n = 6 + (int)(rng() % 30u);
		std::vector<int> cmds;
		if (round % 4 == 0) {
			cmds = {3, 4, n - 1};                            // two commands in consecutive frames, one in the last frame
		} else if (round % 4 == 1) {
			cmds = {0, n / 2, n / 2 + 1};                    // one in the capture's first frame
		} else if (round % 4 != 3) {
			for (int f = 0; f < n; f++)
				if (rng() % 5u == 0)
					cmds.push_back(f);
		}                                                    // (round % 4 == 3: no command at all)
		const Capture c = make_capture(rng, sps, n, cmds);
		CHECK(c.n_adm >= n - 2 && c.n_adm >= 4);
		const std::vector<ref9::Frame> want = ref9::frames({{&c.log, &c.ev9, c.len}}, sps);
		CHECK(!cmds.empty() || want.empty());
		std::vector<int32_t> sync_id(want.size()), rv(want.size());
		for (size_t k = 0; k < want.size(); k++) {
			sync_id[k] = (int32_t)(rng() % 3u);
			rv[k] = rng() % 7u == 0 ? -1 : 0;
		}
		const ref9::Jobs jobs = ref9::jobs(want, sync_id, rv);
		// every window the reference maps lies in the capture, and one past the end was dropped
		for (const ref9::Frame &it : want)
			CHECK(rx_tch9_begin(c.log[it.frame].align, sps, it.tn) >= 0 &&
			      rx_tch9_begin(c.log[it.frame].align, sps, it.tn) + rx_tch9_in_len(sps) <= c.len);
		if (streamed_is_one_shot(c, sps, {}, want, jobs, sync_id, rv)) return 1;
		// one cut at every position: a command lands in a push's first frame and in its last frame
		for (int cut = 0; cut <= c.n_adm; cut++)
			if (streamed_is_one_shot(c, sps, {cut}, want, jobs, sync_id, rv)) return 1;
		// a push per frame, empty pushes between them
		std::vector<int> every;
		for (int f = 0; f <= c.n_adm; f++) {
			every.push_back(f);
			if (f % 3 == 0) every.push_back(f);
		}
		if (streamed_is_one_shot(c, sps, every, want, jobs, sync_id, rv)) return 1;
		// random cuts
		for (int t = 0; t < 8; t++) {
			std::vector<int> cuts;
			for (int f = 0; f <= c.n_adm; f++)
				if (rng() % 4u == 0)
					cuts.push_back(f);
			if (streamed_is_one_shot(c, sps, cuts, want, jobs, sync_id, rv)) return 1;
		}
	}
	// two chains in one plan: the segments stand chain by chain and the items are contiguous over them; a chain without a
	// call has none
	{
		const Capture c0 = make_capture(rng, sps, 12, {2, 7}), c1 = make_capture(rng, sps, 9, {}), c2 = make_capture(rng, sps, 10, {5});
		Tch9CallCarry in1;
		in1.assigned = true;
		in1.tn = 9;
		Tch9PushPlan plan;
		CHECK(tch9_plan_push({{&c0.log, &c0.ev9, Tch9CallCarry(), c0.len}, {&c1.log, &c1.ev9, Tch9CallCarry(), c1.len},
		                      {&c2.log, &c2.ev9, in1, c2.len}}, sps, false, &plan));
		CHECK(plan.segs.size() == 4 && plan.last_seg[0] == 1 && plan.last_seg[1] == -1 && plan.last_seg[2] == 3);
		CHECK(plan.segs[2].chain == 2 && plan.segs[2].ev == 0 && plan.segs[2].tn == 9 && plan.segs[3].ev == 1);
		CHECK(!plan.carry[1].assigned && plan.carry[2].assigned && plan.carry[2].tn == c2.ev9[0].tn);
		for (size_t k = 0; k < plan.items.size(); k++) {
			CHECK(plan.items[k].chain == plan.segs[plan.items[k].ass].chain);
			CHECK(!k || plan.items[k - 1].ass <= plan.items[k].ass);
		}
	}
	// the horizon: a window past the samples held is dropped on the last push and an error on any other
	{
		const int fl = rx_stream_frame_len(sps);
		const std::vector<FrameCtx> log = {{fl, 0.f, 1}, {2 * fl, 0.f, 2}};
		const std::vector<AssEvt> ev9 = {{0, 31, 0, 0.f}};
		const int len = 2 * fl + (39 * 31 + 100) * sps;                       // the second frame's window passes it
		Tch9PushPlan plan;
		CHECK(tch9_plan_push({{&log, &ev9, Tch9CallCarry(), len}}, sps, false, &plan) && plan.items.size() == 1);
		CHECK(!tch9_plan_push({{&log, &ev9, Tch9CallCarry(), len}}, sps, true, &plan));
	}
	return 0;
}

int windows(int sps)
{
	const long long fl = rx_stream_frame_len(sps);
	const int in_len = rx_tch9_in_len(sps), win = sps + sps / 2;
	CHECK(in_len == 351 * sps + win && in_len <= 4096 /* GMR1_HIP_MAX_IN_LEN */);
	for (int tn = 0; tn < 32; tn++) {
		// burst_map of an NT9 burst with `win` samples of search room (rx_loop.h), restated by rx_tch9_begin
		RxLoopState c{};
		c.align = 100000;
		c.len = 1 << 30;
		int begin = 0;
		CHECK(rx_loop_burst_map(c, sps, 351, tn, win, &begin) == win >> 1);
		CHECK(begin == rx_tch9_begin(c.align, sps, tn));
		// the window ends below align + (39 tn + 352.5) sps ...
		CHECK(2 * (rx_tch9_begin(0, sps, tn) + in_len) <= (2 * (39 * tn + 352) + 1) * (long long)sps + 1);
		// ... which leaves, of the 2 frame_len the frame was admitted with, the timing correction (10 sps) and an SI1 that
		// relabels the timeslot `down` slots downwards: 7 at timeslot 31, 23 up to timeslot 15
		const long long slack2 = 2 * 2 * fl - (2 * (39 * tn + 352) + 1) * (long long)sps;     // twice the slack
		CHECK(tn != 31 || slack2 == 621LL * sps);                                            // 310.5 sps
		CHECK(tn != 15 || slack2 == 1869LL * sps);                                           // 934.5 sps
		const int down = (int)((slack2 - 20LL * sps) / (78LL * sps));
		CHECK(tn != 31 || down == 7);
		CHECK(tn > 15 || down >= 23);
		const long long a = 7 * fl + 13;
		for (long long d = -(31 * 39 + 10) * sps; d <= (down * 39 + 10) * sps; d += (d < 0 ? 97 : 1))
			CHECK(rx_tch9_begin((int)(a + d), sps, tn) + in_len <= a + 2 * fl);
		if (tn == 31 || tn == 15)      // one slot further the window passes the end
			CHECK(rx_tch9_begin((int)(a + ((down + 1) * 39 + 10) * sps), sps, tn) + in_len > a + 2 * fl);
		// it begins no earlier than align - e_toa, inside the walk's own reach: once a carrier has dropped samples begin < 0
		// cannot happen in rebased coordinates
		CHECK(rx_tch9_begin(100000, sps, tn) >= 100000 - (win >> 1));
		CHECK(rx_tch9_begin(0, sps, tn) >= -(long long)rx_stream_reach_back(sps));
		CHECK(rx_tch9_begin(rx_stream_reach_back(sps), sps, tn) >= 0);
	}
	return 0;
}

}  // namespace

int main()
{
	for (int sps = 1; sps <= 11; sps++) {
		g_sps = sps;
		if (windows(sps)) return 1;
	}
	for (int sps : {1, 4, 11}) {
		g_sps = sps;
		if (planner(sps)) return 1;
	}
	g_sps = 0;
	// a full handle is made for sps 1..11: from 12 on the NT9 window passes the demodulator's
	CHECK(rx_stream_full_max_sps() == 11 && rx_tch9_in_len(11) <= 4096 && rx_tch9_in_len(12) > 4096);
	CHECK(kRxStreamPlain == 0 && kRxStreamTch == 1 && kRxStreamFull == 2);
	// the kinds, described once: carriers a push brings, what is followed, and a handle decodes audio or follows TCH9, never both
	CHECK(kRxStreamVoice == 3 && kRxStreamKinds == 4);
	const int planes[kRxStreamKinds] = {1, 2, 3, 2};
	for (int kind = 0; kind < kRxStreamKinds; kind++) {
		const RxStreamKind &k = rx_stream_kind(kind);
		CHECK(k.planes == planes[kind] && k.planes <= kRxStreamMaxPlanes);
		CHECK(k.tch3 == (kind != kRxStreamPlain) && k.tch9 == (kind == kRxStreamFull) && k.audio == (kind == kRxStreamVoice));
		CHECK(!(k.tch9 && k.audio) && (k.tch3 || !(k.tch9 || k.audio)));
		CHECK(k.planes == 1 + (k.tch3 ? 1 : 0) + (k.tch9 ? 1 : 0));
		CHECK(k.maker && k.entry);
	}
	// the big-record bound: one per frame a chain's walk can log, times the chains; the audio bound is the same one; and a
	// tch handle's records are the plain ones plus one per frame
	for (int sps = 1; sps <= 16; sps++) {
		g_sps = sps;
		const long long fl = rx_stream_frame_len(sps);
		for (long long len = 0; len <= 50 * fl; len += 1013)
			for (long long c = 0; c <= 65; c++) {
				const long long chains = c < 65 ? c : 1024;       // 0..64, and 1024
				CHECK(rx_stream_max_big(chains, len, sps) == chains * (len / fl + 2));
				CHECK(rx_stream_max_big(chains, len, sps) == chains * rx_stream_frames_per_chain(len, sps));
				CHECK(rx_stream_max_audio(chains, len, sps) == rx_stream_max_big(chains, len, sps));
				CHECK(rx_stream_tch_rec_per_chain(len, sps) == rx_stream_rec_per_chain(len, sps) + rx_stream_frames_per_chain(len, sps));
			}
	}
	std::printf("ok\n");
	return 0;
}
