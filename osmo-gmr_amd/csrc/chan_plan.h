// chan_plan.h -- what the channelizer and the direct mode work out for a (sample rate, sps) before anything touches the device
// (reference utils/gmr1_rx_sdr.py:391-602 PFBBase / PFBOutputParameters, :605-749 DirectOutputParameters): the three filter
// designs in double precision, the decimation search, the resamplers' reduced phase steps, the polyphase banks as they are
// uploaded, and the refusals with their texts.  No HIP call and nothing global, so tests/c/chan_plan_host.cpp runs it without a
// GPU; capi_chan.cpp adds the device copies and the cache (chan_chain.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "chan_select.h"

#pragma GCC visibility push(hidden)        // inside the library all of this is internal: it exports its C ABI
namespace gmr1 {

constexpr double kChanWidth = 31250.0;     // GMR-1 carrier raster (gmr1_rx_sdr.py)
constexpr int kSymRate = 23400;
constexpr int kNfilt = 32;
// what the kernels hold (gmr1_dev.h: kPfbMaxChans, kPfbMaxBlocks, kDdcMaxTaps; chan_chain.h asserts that they are the same)
constexpr int kPlanMaxChans = 256, kPlanMaxBlocks = 11, kPlanMaxFirTaps = 256;

// two floats laid out as HIP's float2: a bank's (tap, next - tap), a complex tap's (re, im)
struct F2 {
	float x, y;
};

// the text of a refusal; the caller hands it to fail(-EINVAL, "%s", ...)
inline std::string refusal(const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	return buf;
}

// gr::filter::firdes::low_pass, Hamming window
inline std::vector<float> design_low_pass(double gain, double fs, double cutoff, double tw)
{
	int ntaps = (int)(53.0 * fs / (22.0 * tw));
	if ((ntaps & 1) == 0)
		ntaps++;
	const int M = (ntaps - 1) / 2;
	std::vector<double> t(ntaps);
	const double fw = 2.0 * M_PI * cutoff / fs;
	for (int n = -M; n <= M; n++) {
		const double w = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)(n + M) / (double)(ntaps - 1));
		t[n + M] = (n == 0 ? fw / M_PI : std::sin(n * fw) / (n * M_PI)) * w;
	}
	double fmax = t[M];
	double tail = 0.0;
	for (int n = 1; n <= M; n++)
		tail += t[n + M];
	fmax += 2.0 * tail;
	std::vector<float> out(ntaps);
	for (int i = 0; i < ntaps; i++)
		out[i] = (float)(t[i] * (gain / fmax));
	return out;
}

// gr::filter::firdes::root_raised_cosine
inline std::vector<float> design_rrc(double gain, double fs, double sym_rate, double alpha, int ntaps)
{
	ntaps |= 1;
	const double spb = fs / sym_rate;
	std::vector<double> t(ntaps, 0.0);
	double scale = 0.0;
	for (int i = 0; i < ntaps; i++) {
		const double xindx = i - ntaps / 2;
		const double x1 = M_PI * xindx / spb;
		double x2 = 4.0 * alpha * xindx / spb;
		double x3 = x2 * x2 - 1.0;
		double num, den;
		if (std::fabs(x3) >= 0.000001) {
			if (i != ntaps / 2)
				num = std::cos((1 + alpha) * x1) + std::sin((1 - alpha) * x1) / (4 * alpha * xindx / spb);
			else
				num = std::cos((1 + alpha) * x1) + (1 - alpha) * M_PI / (4 * alpha);
			den = x3 * M_PI;
		} else {
			if (alpha == 1) {
				t[i] = -1;
				continue;
			}
			x3 = (1 - alpha) * x1;
			x2 = (1 + alpha) * x1;
			num = std::sin(x2) * (1 + alpha) * M_PI - std::cos(x3) * ((1 - alpha) * M_PI * spb) / (4 * alpha * xindx) +
			      std::sin(x3) * spb * spb / (4 * alpha * xindx * xindx);
			den = -32 * M_PI * alpha * alpha * xindx / spb;
		}
		t[i] = 4 * alpha * num / den;
		scale += t[i];
	}
	std::vector<float> out(ntaps);
	for (int i = 0; i < ntaps; i++)
		out[i] = (float)(t[i] * gain / scale);
	return out;
}

// The prototype of the pre-resampler (utils/gmr1_rx_sdr.py:453-461: pfb.arb_resampler_ccf(rate, taps=None, flt_size=32)).
// With taps=None GNU Radio designs it itself, for rates >= 1 -- the only case here: n_chans x 31250 >= samp_rate -- with
// its Parks-McClellan routine (pass band to 0.4 of the input rate, stop band from 0.6, 100 dB), which cannot be
// restated without gr-filter.  OWN DESIGN to the same specification by the window method, at 32 x the input rate, gain 32
// (round 5: the Blackman-Harris design of round 4 had its -6 dB point at 0.5 and was only 36 dB down at 0.6 -- found by
// the test that now holds the specification).  oracle/orc_chan.py: pre_resampler_taps.
inline std::vector<float> design_pre_resampler(int nfilt)
{
	// Kaiser-windowed sinc, 30 taps per phase (what k_resamp<30, ...> holds), beta = 11, -6 dB point at 0.482 of the input
	// rate: within 0.06 dB up to 0.4 and more than 107 dB down from 0.6 (tests/test_oracle_chan.py checks the specification
	// GNU Radio runs its Parks-McClellan design with: 0.1 dB / 100 dB at those edges)
	const double fs = nfilt, cutoff = 0.482, beta = 11.0;
	const int ntaps = 30 * nfilt - 1;
	const int M = (ntaps - 1) / 2;
	auto bessel_i0 = [](double x) {
		double sum = 1.0, term = 1.0;
		const double q = x * x / 4.0;
		for (int k = 1; k < 200; k++) {
			term *= q / ((double)k * (double)k);
			sum += term;
			if (term < 1e-18 * sum)
				break;
		}
		return sum;
	};
	std::vector<double> t(ntaps);
	const double fw = 2.0 * M_PI * cutoff / fs, i0b = bessel_i0(beta);
	double sum = 0.0;
	for (int n = -M; n <= M; n++) {
		const double r = (double)n / (double)M;
		const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
		t[n + M] = (n == 0 ? fw / M_PI : std::sin(n * fw) / (n * M_PI)) * w;
		sum += t[n + M];
	}
	std::vector<float> out(ntaps);
	for (int i = 0; i < ntaps; i++)
		out[i] = (float)(t[i] * ((double)nfilt / sum));
	return out;
}

inline long long gcd(long long a, long long b) { return b ? gcd(b, a % b) : a; }
inline size_t up_to(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One arbitrary-resampler stage (the filterbank path's output resampler, its pre-resampler, the direct mode's resampler):
// a 32-phase bank of rows of tpf taps, filter j0 first, phase step num / den in 1 / 32 input samples, reduced
struct RsStage {
	int tpf = 0, j0 = 0;
	long long num = 0, den = 1;
};
// ... of a prototype of ntaps taps in rows of `row`, at the step num / den (reduced here)
inline RsStage rs_stage(int ntaps, int row, long long num, long long den)
{
	const long long g = gcd(num, den);
	return RsStage{row, (ntaps / 2) % kNfilt, num / g, den / g};
}
// its outputs over T inputs
inline uint64_t resamp_out(const RsStage &s, uint64_t T)
{
	const long long v = ((long long)T * kNfilt - s.j0) * s.den;
	return v > 0 ? (uint64_t)(v / s.num) : 0;
}
// history a streamed k_resamp reads behind its first new output: the row's taps, the input step of one output
// (num / (32 den) samples) and the rounding of both ends
inline int resamp_history(const RsStage &s)
{
	return (int)up_to((size_t)(s.tpf + s.num / (kNfilt * s.den) + 3), 64);
}

// The bank as the kernels read it: row j, place k holds (taps[j + k nfilt], the first difference there; the last one 0),
// zeros behind the prototype's end -- a row longer than the prototype needs (the direct mode's 30 / 96) is padding
inline std::vector<F2> resamp_bank(const std::vector<float> &taps, int nfilt, int row)
{
	const int nt = (int)taps.size();
	std::vector<F2> bank((size_t)nfilt * row, F2{0.f, 0.f});
	for (int j = 0; j < nfilt; j++)
		for (int k = 0; k < row && j + k * nfilt < nt; k++) {
			const int i = j + k * nfilt;
			bank[(size_t)j * row + k] = F2{taps[i], i + 1 < nt ? taps[i + 1] - taps[i] : 0.0f};
		}
	return bank;
}

// global counts after n wideband samples: the first stage's, the second's (the filterbank's instants / stage 2 of the
// direct mode; = the first's where there is no second) and the outputs
struct StreamCounts {
	uint64_t a, b, out;
};

// ---- the filterbank path: PFBBase.__init__ :393-437 and PFBOutputParameters.__init__ :497-531 for width-1 ARFCNs ----------
struct ChanNumbers {
	double samp_rate = 0;
	int sps = 0;
	int n_chans = 0, n_blocks = 0;
	std::vector<float> taps;                 // the filterbank's prototype low-pass
	RsStage rs;                              // the output resampler: root-raised cosine, 2 x 31250 Hz -> 23400 sps Hz
	std::vector<float> rrc;
	std::vector<F2> bank;
	// off the 31.25 kHz grid: the 32-phase pre-resampler to n_chans x 31250 Hz in front of the filterbank
	bool pre = false;
	RsStage pre_rs;
	std::vector<float> pre_taps;
	std::vector<F2> pre_bank;                // 32 x 30
	int ntaps() const { return (int)taps.size(); }
	// samples the filterbank sees for n_in wideband samples
	uint64_t mid_samples(uint64_t n_in) const { return pre ? resamp_out(pre_rs, n_in) : n_in; }
	StreamCounts counts(uint64_t n) const
	{
		const uint64_t a = mid_samples(n), b = a / (uint64_t)(n_chans / 2);
		return StreamCounts{a, b, resamp_out(rs, b)};
	}
};

// false: refused, *why says why (and *out holds what had been worked out until then)
inline bool plan_numbers(double samp_rate, int sps, ChanNumbers *out, std::string *why)
{
	ChanNumbers &p = *out = ChanNumbers();
	p.samp_rate = samp_rate; p.sps = sps;
	p.n_chans = ((int)std::ceil(samp_rate / kChanWidth) + 1) & ~1;
	const double resamp = (p.n_chans * kChanWidth) / samp_rate;
	if (p.n_chans > kPlanMaxChans)
		return *why = refusal("channelize: %d channels (at most %d)", p.n_chans, kPlanMaxChans), false;
	// Off the grid the script resamples the capture to n_chans x 31250 Hz first and designs the filterbank's prototype
	// for ceil(samp_rate / 31250) x 31250 Hz (:413-417; as written that branch reads self.samp_rate before anything
	// sets it and cannot run -- built to its evident intent, the constructor's argument)
	double mid_rate = samp_rate;
	if (std::fabs(resamp - 1.0) >= 1e-5) {
		if ((double)std::llround(samp_rate) != samp_rate)
			return *why = refusal("channelize: the sample rate must be a whole number of Hz"), false;
		p.pre = true;
		mid_rate = std::ceil(samp_rate / kChanWidth) * kChanWidth;
		p.pre_taps = design_pre_resampler(kNfilt);
		const int nt = (int)p.pre_taps.size();
		const int tpf = (nt + kNfilt - 1) / kNfilt;
		if (tpf > kRsTapsShort)
			return *why = refusal("channelize: pre-resampler of %d taps per phase", tpf), false;
		// phase step 32 / rate in 1 / 32 input samples
		p.pre_rs = rs_stage(nt, kRsTapsShort, (long long)kNfilt * std::llround(samp_rate), (long long)p.n_chans * (long long)kChanWidth);
		p.pre_bank = resamp_bank(p.pre_taps, kNfilt, kRsTapsShort);
	}
	p.taps = design_low_pass(1.0, mid_rate, kChanWidth * 0.5, kChanWidth * 0.25);
	p.n_blocks = (p.ntaps() + p.n_chans - 1) / p.n_chans + 1;
	if (p.n_chans == 64 && p.n_blocks > kPlanMaxBlocks)
		return *why = refusal("channelize: prototype filter too long (%d taps)", p.ntaps()), false;
	const double chan_rate2 = kChanWidth * 2.0;                    // 2x oversampled channel rate
	p.rrc = design_rrc(32.0, 32.0 * chan_rate2, kSymRate, 0.35, (int)(11.0 * 32 * chan_rate2 / kSymRate));
	const int nt = (int)p.rrc.size();
	// phase step nfilt / rate, rate = sym_rate sps / chan_rate2
	p.rs = rs_stage(nt, (nt + kNfilt - 1) / kNfilt, (long long)kNfilt * (long long)chan_rate2, (long long)kSymRate * sps);
	p.bank = resamp_bank(p.rrc, kNfilt, p.rs.tpf);
	return true;
}

// the slot of every channel (-1: not kept) for a selection, refusing indices outside the plan and repeats
inline bool select_channels(int nch, int n_sel, const int32_t *chan_idx, std::vector<int32_t> &slot, std::string *why)
{
	slot.assign(nch, -1);
	for (int i = 0; i < n_sel; i++) {
		if (chan_idx[i] < 0 || chan_idx[i] >= nch)
			return *why = refusal("channelize: channel index %d outside 0..%d", chan_idx[i], nch - 1), false;
		if (slot[chan_idx[i]] >= 0)
			return *why = refusal("channelize: channel %d selected twice", chan_idx[i]), false;
		slot[chan_idx[i]] = i;
	}
	return true;
}

// ---- direct mode (utils/gmr1_rx_sdr.py:605-807) ------------------------------------------------------------------
// DirectOutputParameters._factor / _score :637-650
inline std::vector<int> ddc_factor(int decim)
{
	const int d_ideal = (int)std::lround(std::sqrt((double)decim));
	for (int i = d_ideal; i > 1; i--)
		if (decim % i == 0)
			return {decim / i, i};
	return {decim};
}
inline double ddc_score(const std::vector<int> &f)
{
	if (f.size() == 1)
		return f[0];
	return ((double)f[0] * f[0] * f[1]) / (1.0 + (double)f[0] / f[1]);
}

struct DdcNumbers {
	double samp_rate = 0;
	int sps = 0;
	int d1 = 1, d2 = 1;
	double resamp = 1.0;
	std::vector<float> taps1, taps2;         // the two decimating FIRs' low-passes (stage 1's is turned per carrier at call time)
	std::vector<float> rrc;
	int rrc_tpf = 0;                         // taps per phase of the root-raised cosine; the bank's rows (rs.tpf) are the
	RsStage rs;                              // kernel instantiation's 30 or 96, padded with zeros
	std::vector<F2> bank;
	StreamCounts counts(uint64_t n) const
	{
		const uint64_t a = n / (uint64_t)d1, b = a / (uint64_t)d2;
		return StreamCounts{a, b, resamp_out(rs, b)};
	}
};

// (a plan refused for its span, the last refusal, leaves everything but the bank: the host test's search reads its step)
inline bool plan_numbers(double samp_rate, int sps, DdcNumbers *out, std::string *why)
{
	DdcNumbers &p = *out = DdcNumbers();
	p.samp_rate = samp_rate; p.sps = sps;
	const double out_rate = (double)kSymRate * sps;
	if (std::fmod(samp_rate, out_rate) == 0.0)
		return *why = refusal("ddc: %.1f is an exact multiple of %d x %d: the reference's own direct mode cannot run there "
		                      "(_select_decim returns its factors without storing them, gmr1_rx_sdr.py:652-655)", samp_rate, kSymRate, sps), false;
	// _select_decim :657-680
	const int decim_max = (int)std::floor(samp_rate / (2.0 * kSymRate));
	const int decim_min = (int)std::ceil(samp_rate / (3.0 * kSymRate));
	std::vector<int> best;
	double best_score = -1.0;
	for (int i = decim_min; i <= decim_max; i++) {
		const std::vector<int> f = ddc_factor(i);
		const double sc = ddc_score(f);
		if (sc > best_score) { best_score = sc; best = f; }     // the first of equal scores, like Python's stable sort
	}
	if (best.empty())
		return *why = refusal("ddc: sample rate %.1f too low for a direct branch", samp_rate), false;
	if (best.size() == 1)
		best.push_back(1);
	const int decim = best[0] * best[1];
	double resamp = (out_rate * decim) / samp_rate;
	if (best[1] <= 4) {
		resamp /= best[1];
		best[1] = 1;
	}
	p.d1 = best[0]; p.d2 = best[1]; p.resamp = resamp;
	if (resamp == 1.0)
		return *why = refusal("ddc: resampling rate 1 (no resampler stage) is not built"), false;
	// _generate_taps :682-749: root-raised cosine in the resampler, plain low-passes before it
	const double fs2 = samp_rate / (p.d1 * p.d2);
	p.rrc = design_rrc(32.0, 32.0 * fs2, kSymRate, 0.35, (int)(11.0 * 32 * fs2 / kSymRate));
	if (p.d2 != 1)
		p.taps2 = design_low_pass(1.0, 1.0, 0.45 / p.d2, 0.10 / p.d2);
	p.taps1 = design_low_pass(1.0, 1.0, 0.3 / p.d1, 0.3 / p.d1);
	if ((int)p.taps1.size() > kPlanMaxFirTaps || (int)p.taps2.size() > kPlanMaxFirTaps)
		return *why = refusal("ddc: filters of %zu / %zu taps (at most %d)", p.taps1.size(), p.taps2.size(), kPlanMaxFirTaps), false;
	const int nt = (int)p.rrc.size();
	p.rrc_tpf = (nt + kNfilt - 1) / kNfilt;
	// what k_resamp keeps in registers per phase: 30 taps, or 96 in its long instantiation (plans that resample down:
	// 1.0 Msps -> rate 0.468, 95 taps per phase)
	const int row = p.rrc_tpf <= kRsTapsShort ? kRsTapsShort : kRsTapsLong;
	if (p.rrc_tpf > row)
		return *why = refusal("ddc: the resampler of this plan (rate %.4f, %d taps per phase) is longer than the %d the kernel "
		                      "holds", resamp, p.rrc_tpf, row), false;
	if ((double)std::llround(samp_rate) != samp_rate)
		return *why = refusal("ddc: the sample rate must be a whole number of Hz"), false;
	// phase step nfilt / rate = nfilt * samp_rate / (d1 d2 out_rate)
	p.rs = rs_stage(nt, row, (long long)kNfilt * (long long)std::llround(samp_rate), (long long)p.d1 * p.d2 * (long long)out_rate);
	// the 64 output phases of a wave must fit the window its tap bank gets (chan_select.h: the launchers' own rule, so that
	// plan, one-shot call and stream refuse the same plans, here and not at the first launch): 1.0 and 1.5 Msps at sps 1
	int span = 0;
	if (!resamp_plan_runs(p.rs.num, p.rs.den, kNfilt, row, &span))
		return *why = refusal("ddc: %.1f samples/s at sps %d: the resampler (rate %.4f, %d taps per phase) spans %d input samples "
		                      "per wave, the kernel's window holds %d", samp_rate, sps, resamp, p.rrc_tpf, span,
		                      row == kRsTapsLong ? kRsWinLong : kRsWinShort), false;
	p.bank = resamp_bank(p.rrc, kNfilt, row);
	return true;
}

// freq_xlating_fir_filter_ccc: the low-pass turned up to the carrier, taps[k] e^{+j 2 pi f k / fs}; the output is
// turned back by e^{-j 2 pi f m d1 / fs}
inline void ddc_carrier_taps(const DdcNumbers &p, int n_sel, const double *freq_hz, std::vector<F2> &t1, std::vector<double> &rot)
{
	const int nt1 = (int)p.taps1.size();
	t1.resize((size_t)n_sel * nt1);
	rot.resize((size_t)n_sel);
	for (int c = 0; c < n_sel; c++) {
		const double fn = freq_hz[c] / p.samp_rate;
		for (int k = 0; k < nt1; k++) {
			const double ph = 2.0 * M_PI * std::fmod(fn * k, 1.0);
			t1[(size_t)c * nt1 + k] = F2{(float)(p.taps1[k] * std::cos(ph)), (float)(p.taps1[k] * std::sin(ph))};
		}
		rot[c] = fn * p.d1;
	}
}

}  // namespace gmr1
#pragma GCC visibility pop
