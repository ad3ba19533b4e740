// Host-side exercise of the audio close-up's rule (osmo-gmr_amd/csrc/tch3_audio.h: which record of the TCH3 follower gives a
// block, its slot, the label and the header; the device runs it in k_tch3f_audio and k_ambe_audio) and of the receive
// loop's carry rule for a chain's assignment count (rx_follow.h: tch3_voice_call, tch3_voice_carry, over tch3_plan).
// tests/test_rx_voice_host.py builds it, once more under the address and undefined-behaviour sanitizers, and compares the
// close-up with a numpy restatement.
//   first line printed: tch3_audio_reports(cls) for cls = 0 .. 255, then the block layout the header states
//   second line: "carry ok", or what failed, of the self-check below
//   then per line of stdin "n_frames n_calls first[0] .. first[n_calls] cls[0] .. cls[n_frames - 1] label fn":
//   the slot of every record, call_base[0 .. n_calls], and the header words of (label, cls[0] or 0, fn), on one line
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "rx_follow.h"
#include "tch3_audio.h"

using namespace gmr1;

namespace {

// A chain of n frames with assignments at `at`, cut into pushes at `cuts` (frame indices): the `call` every frame's block
// carries in the pushes, through tch3_plan and the carry, against the one-shot pass's
bool carry_holds(int n, const std::vector<int> &at, const std::vector<int> &cuts, int sps)
{
	const int fl = sps * 24 * 39, a0 = 5000 * sps, len = a0 + (n + 3) * fl;
	auto log_of = [&](int lo, int hi) {
		std::vector<FrameCtx> log;
		for (int f = lo; f < hi; f++)
			log.push_back({a0 + (f - lo) * fl, 0.f, 1000 + f});
		return log;
	};
	auto events_of = [&](int lo, int hi) {
		std::vector<AssEvt> ev;
		for (size_t e = 0; e < at.size(); e++)
			if (at[e] >= lo && at[e] < hi)
				ev.push_back({at[e] - lo, 3 + (int)e, 7, 1.f});
		return ev;
	};
	// one shot: frame -> call
	std::vector<int> want((size_t)n, 0);
	{
		const std::vector<FrameCtx> log = log_of(0, n);
		const std::vector<AssEvt> ev = events_of(0, n);
		Tch3Plan p;
		if (!tch3_plan({{&log, &ev, false, 0, len}}, sps, false, &p))
			return false;
		for (const Tch3Item &it : p.items)
			want[(size_t)it.frame] = tch3_voice_call(0, it.gen);
		if (tch3_voice_carry(0, ev.size()) != (int)at.size())
			return false;
	}
	// pushes
	std::vector<int> got((size_t)n, 0);
	int carried = 0, tn = 0, lo = 0;
	bool assigned = false;
	std::vector<int> edges = cuts;
	edges.push_back(n);
	for (int hi : edges) {
		const std::vector<FrameCtx> log = log_of(lo, hi);
		const std::vector<AssEvt> ev = events_of(lo, hi);
		Tch3Plan p;
		if (!tch3_plan({{&log, &ev, assigned, tn, len}}, sps, false, &p))
			return false;
		for (const Tch3Item &it : p.items)
			got[(size_t)(lo + it.frame)] = tch3_voice_call(carried, it.gen);
		// a push in which one invocation has frames hands its blocks straight back
		size_t gens = 0;
		for (size_t g = 0; g <= ev.size(); g++) {
			bool any = false;
			for (const Tch3Item &it : p.items)
				any |= it.gen == (int)g;
			gens += any;
		}
		if (tch3_voice_invocations(p) != gens)
			return false;
		carried = tch3_voice_carry(carried, ev.size());
		if (!ev.empty()) {
			assigned = true;
			tn = ev.back().tn;
		}
		lo = hi;
	}
	return got == want && carried == (int)at.size();
}

const char *carry_check()
{
	const int n = 40;
	const std::vector<std::vector<int>> ats = {{}, {0}, {5}, {5, 6}, {5, 20, 39}, {3, 3, 17}};
	for (const std::vector<int> &at : ats) {
		if (!carry_holds(n, at, {}, 4))
			return "one push";
		for (int a = 0; a <= n; a++)
			for (int b = a; b <= n; b += 3)
				if (!carry_holds(n, at, {a, b}, 4))
					return "two cuts";
		std::vector<int> every;
		for (int f = 1; f < n; f++)
			every.push_back(f);
		if (!carry_holds(n, at, every, 1) || !carry_holds(n, at, every, 16))
			return "a push per frame";
	}
	return "carry ok";
}

}  // namespace

int main()
{
	for (unsigned cls = 0; cls < 256; cls++)
		printf("%d ", tch3_audio_reports(cls) ? 1 : 0);
	printf("%d %d %d %d %d %d\n", kAudioBytes, kAudioRv, kAudioPcm, kAudioRecCls, kAudioClsOff, (int)kAudioNoSlot);
	printf("%s\n", carry_check());
	int n_frames, n_calls;
	while (scanf("%d %d", &n_frames, &n_calls) == 2) {
		if (n_calls < 0 || n_frames < 0)
			return 2;
		// exactly as long as the rule reads and writes: ASan sees one past
		std::vector<int32_t> first((size_t)n_calls + 1), slot((size_t)n_frames), base((size_t)n_calls + 1);
		std::vector<uint8_t> cls((size_t)n_frames);
		for (int c = 0; c <= n_calls; c++)
			if (scanf("%" SCNd32, &first[(size_t)c]) != 1)
				return 3;
		for (int k = 0; k < n_frames; k++) {
			unsigned v;
			if (scanf("%u", &v) != 1)
				return 4;
			cls[(size_t)k] = (uint8_t)v;
		}
		uint64_t label;
		uint32_t fn;
		if (scanf("%" SCNu64 " %" SCNu32, &label, &fn) != 2)
			return 5;
		tch3_audio_closeup(n_calls, first.data(), n_frames, cls.data(), slot.data(), base.data());
		for (int k = 0; k < n_frames; k++)
			printf("%d ", slot[(size_t)k]);
		for (int c = 0; c <= n_calls; c++)
			printf("%d ", base[(size_t)c]);
		const AudioHead h = tch3_audio_head(label, n_frames ? cls[0] : 0u, fn);
		printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", h.w[0], h.w[1], h.w[2], h.w[3]);
	}
	return 0;
}
