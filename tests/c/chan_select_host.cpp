// Host-side check of the resampler's launch rule (osmo-gmr_amd/csrc/chan_select.h).  A wrong choice among the forms that all
// compute the same sums leaves every output correct on a GPU and only moves a time; a wrong refusal shows only at a plan nobody
// runs.  So the program is a table: it reads lines of
//     num den tpf T n_out ext stream o0 one_only shared_ring wg1 n_slots
// from its standard input and prints, per line, what the rule answers:
//     form P Q span span_r taps win per_lane wg nch gx gy gz runs
// (ext 2: polyphase-planar output; runs = resamp_plan_runs).  tests/test_chan_select_host.py derives what it expects with Python's
// fractions, not with this rule, and compares.  With the argument "search" it instead walks the direct mode's plans over the
// sample rates that are multiples of 10 kHz from 0.5 to 8 Msps x sps 1 .. 16 -- the test feeds it each plan's step and bank as
//     rate sps num den tpf
// and it prints the accepted plan with the largest span_r <= 128, the accepted plan with the largest span <= 512 on the
// 96-tap bank and the refused plan nearest above each window.  Built once more under the address and undefined-behaviour
// sanitizers (a stand-alone program: nothing is preloaded).
#include <cstdio>
#include <cstring>

#include "chan_select.h"

using namespace gmr1;

namespace {

int table()
{
	long long num, den, T, n_out, o0;
	int tpf, ext, stream, one_only, shared_ring, wg1, n_slots;
	while (std::scanf("%lld %lld %d %lld %lld %d %d %lld %d %d %d %d", &num, &den, &tpf, &T, &n_out, &ext, &stream, &o0, &one_only,
	                  &shared_ring, &wg1, &n_slots) == 12) {
		ResampQuery q;
		q.num = num; q.den = den; q.nfilt = 32; q.tpf = tpf; q.T = T; q.n_out = n_out; q.n_slots = n_slots;
		q.ext = ext != 0; q.planar = ext == 2; q.stream = stream != 0; q.o0 = o0;
		q.one_only = one_only != 0; q.shared_ring = shared_ring != 0; q.wg1 = wg1 != 0;
		const ResampChoice c = resamp_choice(q);
		int span = 0;
		const bool runs = resamp_plan_runs(num, den, 32, tpf, &span);
		std::printf("%d %lld %lld %d %d %d %d %d %d %d %u %u %u %d\n", (int)c.form, c.P, c.Q, c.span, c.span_r, c.taps, c.win,
		            c.per_lane, c.wg, c.nch, c.gx, c.gy, c.gz, runs ? 1 : 0);
	}
	return 0;
}

struct Found {
	long long rate = 0;
	int sps = 0, val = -1;
};

void show(const char *what, const Found &f)
{
	std::printf("%s %lld %d %d\n", what, f.rate, f.sps, f.val);
}

int search()
{
	long long rate, num, den;
	int sps, tpf;
	Found two_widest, long_widest, short_refused, long_refused;
	while (std::scanf("%lld %d %lld %lld %d", &rate, &sps, &num, &den, &tpf) == 5) {
		if (tpf != kRsTapsShort && tpf != kRsTapsLong)
			continue;
		int span = 0;
		const bool runs = resamp_plan_runs(num, den, 32, tpf, &span);
		ResampQuery q;
		q.num = num; q.den = den; q.nfilt = 32; q.tpf = tpf; q.T = 1 << 20; q.n_out = 1 << 20; q.n_slots = 1;
		const ResampChoice c = resamp_choice(q);
		if (runs != (c.form != kRsFormRefused)) {
			std::printf("FAIL: %lld sps %d: plan and launch disagree\n", rate, sps);
			return 1;
		}
		// (the first of equal values: rates ascend, then sps)
		if (runs && c.form == kRsFormTwo && c.span_r > two_widest.val)
			two_widest = Found{rate, sps, c.span_r};
		if (runs && tpf == kRsTapsLong && span > long_widest.val)
			long_widest = Found{rate, sps, span};
		if (!runs && tpf == kRsTapsShort && (short_refused.val < 0 || span < short_refused.val))
			short_refused = Found{rate, sps, span};
		if (!runs && tpf == kRsTapsLong && (long_refused.val < 0 || span < long_refused.val))
			long_refused = Found{rate, sps, span};
	}
	show("two_widest", two_widest);
	show("long_widest", long_widest);
	show("short_refused", short_refused);
	show("long_refused", long_refused);
	return 0;
}

}  // namespace

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "search"))
		return search();
	return table();
}
