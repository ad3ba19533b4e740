// chan_select.h -- which form of the arbitrary resampler a launch gets (chan_kernels.hip: k_resamp, k_resamp2, k_resamp2w) and
// whether the kernels can run the plan at all: the launchers' rule as a function of its inputs.  No HIP call and nothing
// global, so tests/c/chan_select_host.cpp runs it without a GPU; chan_plan.h asks it when it makes a plan, so that a plan the
// kernels cannot run is refused there (-EINVAL) and not at its first launch.
#pragma once

namespace gmr1 {

// taps per filter: 30 for the 941-tap / 32-phase bank of every plan that raises the rate; the direct mode at 1.0 Msps
// resamples DOWN (rate 0.468) and its root-raised cosine is 95 taps per phase long -- a second instantiation
static constexpr int kRsTapsShort = 30, kRsTapsLong = 96;
static constexpr int kRsPeriods = 32;        // periods one wave walks
static constexpr int kRsPeriodsStream = 4;   // ... in a streamed push (a small grid: the walk is the push's time)
static constexpr int kRsWinTight = 128, kRsWinShort = 256, kRsWinLong = 512;     // LDS window (samples) per wave, >= span
static constexpr int kRsWg = 8;              // waves of a k_resamp2w work-group

enum ResampForm {
	kRsFormNone = 0,       // nothing to launch (no output, no stream)
	kRsFormRefused,        // the kernels cannot run this
	kRsFormOne,            // k_resamp<taps, win, ext, stream>: one output per lane
	kRsFormTwo,            // k_resamp2<128, ring, wg>: two outputs per lane, a window ring per wave
	kRsFormTwoShared,      // k_resamp2w: ... a ring per work-group (profiling build, on request)
};

struct ResampQuery {
	long long num = 0, den = 1;        // phase step num / den in 1 / nfilt input samples, reduced
	int nfilt = 32;
	int tpf = 0;                       // row length of the bank: kRsTapsShort or kRsTapsLong
	long long T = 0, n_out = 0;        // input samples and outputs per stream (streamed: the global counts after the push)
	int n_slots = 0;
	bool ext = false;                  // a rotation of the input or polyphase-planar output
	bool planar = false;               // (polyphase-planar output: one-shot only)
	bool stream = false;               // a streamed push: the outputs [o0, n_out)
	long long o0 = 0;
	// the profiling build's switches (false in the product): GMR1_HIP_RESAMP_R=1, GMR1_HIP_RESAMP_WG, GMR1_HIP_RESAMP_WG1
	bool one_only = false, shared_ring = false, wg1 = false;
};

struct ResampChoice {
	ResampForm form = kRsFormNone;
	long long P = 0, Q = 0;            // the (filter, fraction) pair repeats every P outputs = Q inputs
	int span = 0, span_r = 0;          // inputs the 64 / 128 phases of a wave can touch
	int taps = 0, win = 0;             // tap bank (30 / 96) and LDS window (128 / 256 / 512) of the form
	int per_lane = 0;                  // outputs per lane
	int wg = 0;                        // waves per work-group
	int nch = 0;                       // kRsFormTwoShared: 128-sample chunks of the work-group's window
	unsigned gx = 0, gy = 0, gz = 0;   // the grid
};

// P, Q and the spans of a step num / den with a bank of `taps` taps (what a plan needs to know before any launch)
inline void resamp_period(long long num, long long den, int nfilt, int taps, long long *P, long long *Q, int *span, int *span_r)
{
	long long g = num, b = den * nfilt;
	while (b) { const long long t = g % b; g = b; b = t; }
	*P = den * nfilt / g;
	*Q = num / g;
	*span = (int)((63 * num) / (den * nfilt)) + taps + 2;
	*span_r = (int)((127 * num) / (den * nfilt)) + taps + 2;
}

// can the kernels run a plan of this step on a bank of tpf taps?  (the span of a wave's 64 phases must fit the window its
// tap bank gets: 256 samples with 30 taps, 512 with 96)
inline bool resamp_plan_runs(long long num, long long den, int nfilt, int tpf, int *span_out)
{
	if (tpf != kRsTapsShort && tpf != kRsTapsLong)
		return false;
	long long P, Q;
	int span, span_r;
	resamp_period(num, den, nfilt, tpf, &P, &Q, &span, &span_r);
	if (span_out) *span_out = span;
	return span <= (tpf == kRsTapsLong ? kRsWinLong : kRsWinShort);
}

inline ResampChoice resamp_choice(const ResampQuery &q)
{
	ResampChoice c;
	const long long lo = q.stream ? q.o0 : 0;
	if (q.n_out <= lo || q.n_slots <= 0)
		return c;
	const bool lng = q.tpf == kRsTapsLong;
	c.form = kRsFormRefused;
	if (q.tpf != kRsTapsShort && !lng)
		return c;
	if (q.stream && (q.o0 < 0 || q.planar))
		return c;
	c.taps = lng ? kRsTapsLong : kRsTapsShort;
	c.win = lng ? kRsWinLong : kRsWinShort;
	resamp_period(q.num, q.den, q.nfilt, c.taps, &c.P, &c.Q, &c.span, &c.span_r);
	if (c.span > c.win)
		return c;
	if (lng && q.ext)
		return c;                                // (the long bank is the direct mode's: neither option reaches it)
	const long long P = c.P;
	const int per = q.stream ? kRsPeriodsStream : kRsPeriods;
	const long long periods = (q.n_out + P - 1) / P - (q.stream ? q.o0 / P : 0);
	c.gx = (unsigned)((P + 63) / 64);
	c.gy = (unsigned)q.n_slots;
	c.gz = (unsigned)((periods + per - 1) / per);
	c.per_lane = 1;
	c.wg = 1;
	// two consecutive outputs per lane where the rate goes up (their windows then start at most one sample apart) and the
	// 128 phases of a wave still fit the tight window; a streamed push keeps one output per lane
	const bool two = !q.stream && !lng && !q.ext && !q.one_only && q.num < q.den * q.nfilt && c.span_r <= kRsWinTight &&
	                 P >= 2 && q.T >= 2;
	if (!two) {
		c.form = kRsFormOne;
		if (!lng && c.span <= kRsWinTight)
			c.win = kRsWinTight;
		return c;
	}
	c.per_lane = 2;
	c.win = kRsWinTight;
	// one window ring per work-group of kRsWg waves where the union of their windows is fewer chunks than they are and
	// the period has at least that many output groups (k_resamp2w); else a ring per wave
	const long long gx2 = (P + 127) / 128;
	const int span_w = (int)(((long long)(kRsWg * 128 - 1) * q.num) / (q.den * q.nfilt)) + c.taps + 2;
	const int nch = (span_w + 127) / 128;
	if (q.shared_ring && nch < kRsWg && gx2 >= kRsWg) {
		c.form = kRsFormTwoShared;
		c.wg = kRsWg;
		c.nch = nch;
		c.gx = (unsigned)((gx2 + kRsWg - 1) / kRsWg);
		return c;
	}
	// the largest of 8, 4, 2 output groups per work-group that divides the period's groups: a work-group's LDS is its waves'
	// rings whether or not they have an output group, so a part-filled one would cost residency
	c.form = kRsFormTwo;
	c.wg = q.wg1 ? 1 : (gx2 % 8 == 0 ? 8 : (gx2 % 4 == 0 ? 4 : (gx2 % 2 == 0 ? 2 : 1)));
	c.gx = (unsigned)(gx2 / c.wg);
	return c;
}

}  // namespace gmr1
