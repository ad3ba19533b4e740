// capi_chan.cpp -- C ABI of the wideband -> per-ARFCN channelizer (reference utils/gmr1_rx_sdr.py:391-602:
// PFBBase, PFBOutputParameters, PFBOutputBranch, and the GNU Radio blocks they configure) and of the direct mode (:605-807),
// one-shot.  The filter design runs on the host in double precision, once per (sample rate, sps) (chan_plan.h); everything
// per sample runs on the GPU.  The streaming handle: capi_chan_stream.cpp.

#include "chan_chain.h"

#include <utility>

#include "../../include/gmr1_hip.h"
#include "dev_cache.h"

using namespace gmr1;

namespace {

typedef std::pair<double, int> RateSps;
DevCache<RateSps, ChanPlan> g_plans;
DevCache<RateSps, DdcPlan> g_ddc_plans;

// a plan's device copies; what was uploaded is freed if a later upload fails
int upload_plan(ChanPlan &p)
{
	int r;
	if (!(r = upload(&p.d_taps, p.taps)) && !(r = upload(&p.d_bank, p.bank)) && p.pre)
		r = upload(&p.d_pre_bank, p.pre_bank);
	if (r)
		(void)hipFree(p.d_taps), (void)hipFree(p.d_bank);
	return r;
}

int upload_plan(DdcPlan &p)
{
	std::vector<F2> t2(p.taps2.size());
	for (size_t i = 0; i < t2.size(); i++)
		t2[i] = F2{p.taps2[i], 0.f};
	int r;
	if (!t2.empty() && (r = upload(&p.d_taps2, t2)))
		return r;
	if ((r = upload(&p.d_bank, p.bank)))
		(void)hipFree(p.d_taps2);
	return r;
}

// the cached plan of (rate, sps, current device), or a new one: its numbers, then its device copies
template <typename Plan> int cached_plan(DevCache<RateSps, Plan> &plans, double samp_rate, int sps, const Plan **out)
{
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	return plans.get(dev, RateSps(samp_rate, sps), out, [&](Plan *p) {
		std::string why;
		return plan_numbers(samp_rate, sps, p, &why) ? upload_plan(*p) : fail(-EINVAL, "%s", why.c_str());
	});
}

}  // namespace

namespace gmr1 {

int get_plan(double samp_rate, int sps, const ChanPlan **out) { return cached_plan(g_plans, samp_rate, sps, out); }
int get_plan(double samp_rate, int sps, const DdcPlan **out) { return cached_plan(g_ddc_plans, samp_rate, sps, out); }

int select_slots(int nch, int n_sel, const int32_t *chan_idx, std::vector<int32_t> &slot)
{
	std::string why;
	return select_channels(nch, n_sel, chan_idx, slot, &why) ? 0 : fail(-EINVAL, "%s", why.c_str());
}

int checked_fmt(const char *who, int fmt)
{
	return iq_sample_bytes(fmt) < 0 ? fail(-EINVAL, "%s: fmt=%d is none of GMR1_HIP_IQ_F32 / _S16 / _S8", who, fmt) : 0;
}

int run_resamp(hipStream_t st, const RsStage &rs, const float2 *bank, int n_slots, const Span &s, float rotation, int planar_sps,
               long long plane_stride)
{
	ResampArgs a = {};
	a.n_slots = n_slots; a.nfilt = kNfilt; a.tpf = rs.tpf; a.j0 = rs.j0; a.num = rs.num; a.den = rs.den;
	a.T = s.n_in; a.n_out = s.n_out; a.out_stride = s.y_stride;
	a.y = s.x; a.bank = bank; a.out = s.y; a.rotation = rotation;
	a.planar_sps = planar_sps; a.plane_stride = plane_stride;
	a.st = s.st;
	if (s.st.xt)
		a.st.x_stride = s.x_stride;
	HIP_TRY(launch_resamp(a, st));
	return 0;
}

int run_pfb(hipStream_t st, const ChanPlan &p, const int32_t *d_slot, int n_sel, const Span &s, float rotation)
{
	PfbArgs a = {};
	a.n_chans = p.n_chans; a.n_blocks = p.n_blocks; a.ntaps = p.ntaps();
	a.n_in = s.n_in; a.T = s.n_out; a.rotation = rotation;
	a.x = s.x; a.taps = p.d_taps; a.slot = d_slot; a.y = s.y;
	a.sel = d_slot + kPfbMaxChans; a.n_sel = n_sel;          // slot[n_chans], then sel[n_sel]
	a.fmt = s.fmt;
	a.st = s.st;
	if (s.st.xt)
		a.st.y_stride = s.y_stride;
	HIP_TRY(launch_pfb(a, st));
	return 0;
}

int run_fir(hipStream_t st, int n_sel, int decim, int ntaps, const float2 *taps, const double *rot, const Span &s)
{
	DdcFirArgs a = {};
	a.n_sel = n_sel; a.decim = decim; a.ntaps = ntaps; a.n_in = s.n_in; a.n_out = s.n_out; a.in_stride = 0;
	a.x = s.x; a.taps = taps; a.rot = rot; a.y = s.y;
	a.fmt = s.fmt;
	a.st = s.st;
	if (s.st.xt)
		a.st.y_stride = s.y_stride;
	HIP_TRY(launch_ddc_fir(a, st));
	return 0;
}

int run_fir2(hipStream_t st, const DdcPlan &p, int n_sel, const Span &s)
{
	for (int c = 0; c < n_sel; c++) {
		Span row = s;
		row.x += (size_t)c * s.x_stride;
		row.y += (size_t)c * s.y_stride;
		if (s.st.xt)
			row.st.xt += (size_t)c * s.x_stride;
		if (int r = run_fir(st, 1, p.d2, (int)p.taps2.size(), p.d_taps2, nullptr, row)) return r;
	}
	return 0;
}

}  // namespace gmr1

extern "C" {

int gmr1_hip_ddc_plan(double samp_rate, int sps, uint64_t n_in, int32_t *decim1, int32_t *decim2, double *resamp,
                      uint64_t *n_out)
{
	const DdcPlan *p;
	int r = checked_plan("ddc", samp_rate, sps, &p);
	if (r) return r;
	if (decim1) *decim1 = p->d1;
	if (decim2) *decim2 = p->d2;
	if (resamp) *resamp = p->resamp;
	if (n_out) *n_out = p->counts(n_in).out;
	return 0;
}

static int ddc_dev_impl(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel,
                        const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	if (int r = checked_fmt("ddc", fmt)) return r;
	if (!wide || n_sel < 0 || (n_sel && (!freq_hz || !out)))
		return fail(-EINVAL, "ddc: wide / freq_hz / out are required");
	const DdcPlan *p;
	DevState *s;
	int r = checked_plan("ddc", samp_rate, sps, &p, &s);
	if (r) return r;
	const StreamCounts c = p->counts(n_in);
	const uint64_t n_out = c.out;
	if (n_out_p) *n_out_p = n_out;
	if (n_sel == 0 || n_out == 0)
		return 0;
	if (out_stride < n_out)
		return fail(-EINVAL, "ddc: out_stride %llu < %llu output samples per carrier", (unsigned long long)out_stride,
		            (unsigned long long)n_out);
	hipStream_t st = (hipStream_t)stream;
	const long long n1 = (long long)c.a, n2 = (long long)c.b;
	const int nt1 = (int)p->taps1.size();
	// scratch: per-carrier stage-1 taps and rotation steps, then the two intermediate streams
	const size_t b_t1 = up_to(sizeof(float2) * (size_t)n_sel * nt1, 256), b_rot = up_to(sizeof(double) * (size_t)n_sel, 256);
	const size_t b_y1 = up_to(sizeof(float2) * (size_t)n_sel * (size_t)n1, 256);
	const size_t b_y2 = p->d2 > 1 ? up_to(sizeof(float2) * (size_t)n_sel * (size_t)n2, 256) : 0;
	void *ws;
	WsLease lease;
	if ((r = lease.acquire(s, st))) return r;
	r = dev_workspace(s, b_t1 + b_rot + b_y1 + b_y2, &ws);
	if (r) return r;
	char *w = static_cast<char *>(ws);
	float2 *d_t1 = reinterpret_cast<float2 *>(w);
	double *d_rot = reinterpret_cast<double *>(w + b_t1);
	float2 *d_y1 = reinterpret_cast<float2 *>(w + b_t1 + b_rot);
	float2 *d_y2 = p->d2 > 1 ? reinterpret_cast<float2 *>(w + b_t1 + b_rot + b_y1) : d_y1;
	std::vector<F2> t1;
	std::vector<double> rot;
	ddc_carrier_taps(*p, n_sel, freq_hz, t1, rot);
	HIP_TRY(hipMemcpyAsync(d_t1, t1.data(), t1.size() * sizeof(float2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_rot, rot.data(), rot.size() * sizeof(double), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));       // t1 / rot are host temporaries
	const float2 *x = static_cast<const float2 *>(wide);
	if ((r = run_fir(st, n_sel, p->d1, nt1, d_t1, d_rot, Span{x, (long long)n_in, 0, d_y1, n1, 0, {}, fmt}))) return r;
	if (p->d2 > 1 && (r = run_fir2(st, *p, n_sel, Span{d_y1, n1, n1, d_y2, n2, n2, {}}))) return r;
	return run_resamp(st, p->rs, p->d_bank, n_sel,
	                  Span{d_y2, n2, 0, reinterpret_cast<float2 *>(out), (long long)n_out, (long long)out_stride, {}});
}

int gmr1_hip_ddc_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in, int n_sel,
                     const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return ddc_dev_impl(stream, samp_rate, sps, kIqF32, wide, n_in, n_sel, freq_hz, out, out_stride, n_out_p);
}

int gmr1_hip_ddc_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel,
                        const double *freq_hz, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return ddc_dev_impl(stream, samp_rate, sps, fmt, wide, n_in, n_sel, freq_hz, out, out_stride, n_out_p);
}

// a host capture's device copy, uploaded in its own format: n complex samples of fmt (checked by the caller)
static const void *stage_iq(Stage &sg, int fmt, const void *wide, size_t n)
{
	if (fmt == kIqS16) return sg.in(static_cast<const int16_t *>(wide), n * 2);
	if (fmt == kIqS8) return sg.in(static_cast<const int8_t *>(wide), n * 2);
	return sg.in(static_cast<const float *>(wide), n * 2);
}

static int ddc_host_impl(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel, const double *freq_hz,
                         float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if ((r = checked_fmt("ddc", fmt))) return r;
	if (!wide || n_sel < 0 || (n_sel && (!freq_hz || !out)))
		return fail(-EINVAL, "ddc: wide / freq_hz / out are required");
	uint64_t n_out;
	r = gmr1_hip_ddc_plan(samp_rate, sps, n_in, nullptr, nullptr, nullptr, &n_out);
	if (r) return r;
	if (n_out_p) *n_out_p = n_out;
	if (!n_sel || !n_out) return 0;
	if (out_stride < n_out)
		return fail(-EINVAL, "ddc: out_stride too small");
	Stage sg;
	const void *d_w = stage_iq(sg, fmt, wide, (size_t)n_in);
	float *d_o = sg.out(out, (size_t)n_sel * out_stride * 2);
	if ((r = sg.err())) return r;
	r = ddc_dev_impl(nullptr, samp_rate, sps, fmt, d_w, n_in, n_sel, freq_hz, d_o, out_stride, nullptr);
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_ddc(double samp_rate, int sps, const float *wide, uint64_t n_in, int n_sel, const double *freq_hz,
                 float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return ddc_host_impl(samp_rate, sps, kIqF32, wide, n_in, n_sel, freq_hz, out, out_stride, n_out_p);
}

int gmr1_hip_ddc_iq(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, int n_sel, const double *freq_hz,
                    float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return ddc_host_impl(samp_rate, sps, fmt, wide, n_in, n_sel, freq_hz, out, out_stride, n_out_p);
}

int gmr1_hip_channelize_plan(double samp_rate, int sps, uint64_t n_in,
                             int32_t *n_chans, uint64_t *n_mid, uint64_t *n_out)
{
	const ChanPlan *p;
	int r = checked_plan("channelize", samp_rate, sps, &p);
	if (r) return r;
	const StreamCounts c = p->counts(n_in);
	if (n_chans) *n_chans = p->n_chans;
	if (n_mid) *n_mid = c.b;
	if (n_out) *n_out = c.out;
	return 0;
}

static int channelize_dev_impl(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in,
                               float rotation, int n_sel, const int32_t *chan_idx,
                               float *out, uint64_t out_stride, uint64_t plane_stride, bool planar, uint64_t *n_out_p)
{
	if (int r = checked_fmt("channelize", fmt)) return r;
	if (!wide || n_sel < 0 || (n_sel && (!chan_idx || !out)))
		return fail(-EINVAL, "channelize: wide / chan_idx / out are required");
	if (planar && plane_stride < ((uint64_t)n_sel * out_stride + (uint64_t)sps - 1) / (uint64_t)(sps > 0 ? sps : 1))
		return fail(-EINVAL, "channelize: plane_stride %llu < ceil(n_sel x out_stride / sps)", (unsigned long long)plane_stride);
	const ChanPlan *p;
	DevState *s;
	int r = checked_plan("channelize", samp_rate, sps, &p, &s);
	if (r) return r;
	const uint64_t n_pre = p->mid_samples(n_in), T = p->counts(n_in).b, n_out = p->counts(n_in).out;
	if (n_out_p) *n_out_p = n_out;
	if (n_sel == 0 || n_out == 0)
		return 0;
	if (out_stride < n_out)
		return fail(-EINVAL, "channelize: out_stride %llu < %llu output samples per channel",
		            (unsigned long long)out_stride, (unsigned long long)n_out);
	std::vector<int32_t> slot;
	if ((r = select_slots(p->n_chans, n_sel, chan_idx, slot)))
		return r;
	hipStream_t st = (hipStream_t)stream;
	// scratch: slot table + the 2x oversampled channel streams (+ the pre-resampled capture, off the grid, and in front of
	// that the float copy of an integer capture: the pre-resampler is the one stage that does not read the integers itself)
	const size_t slot_bytes = 2 * kPfbMaxChans * 4;          // slot[n_chans], then sel[n_sel]
	const size_t mid_bytes = up_to((size_t)n_sel * T * sizeof(float2), 256);
	const size_t pre_bytes = p->pre ? up_to((size_t)n_pre * sizeof(float2), 256) : 0;
	const size_t conv_bytes = p->pre && fmt != kIqF32 ? (size_t)n_in * sizeof(float2) : 0;
	void *ws;
	WsLease lease;
	if ((r = lease.acquire(s, st))) return r;
	r = dev_workspace(s, slot_bytes + mid_bytes + pre_bytes + conv_bytes, &ws);
	if (r) return r;
	int32_t *d_slot = static_cast<int32_t *>(ws);
	float2 *d_mid = reinterpret_cast<float2 *>(static_cast<char *>(ws) + slot_bytes);
	float2 *d_pre = reinterpret_cast<float2 *>(static_cast<char *>(ws) + slot_bytes + mid_bytes);
	float2 *d_conv = reinterpret_cast<float2 *>(static_cast<char *>(ws) + slot_bytes + mid_bytes + pre_bytes);
	HIP_TRY(hipMemcpyAsync(d_slot, slot.data(), (size_t)p->n_chans * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_slot + kPfbMaxChans, chan_idx, (size_t)n_sel * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));      // slot[] is a host temporary
	const float2 *x = static_cast<const float2 *>(wide);
	const long long np = (long long)n_pre;
	if (conv_bytes) {
		HIP_TRY(launch_iq_convert(wide, fmt, (long long)n_in, d_conv, st));
		x = d_conv;
		fmt = kIqF32;
	}
	if (p->pre) {
		// rotator (if any), then pfb.arb_resampler_ccf to n_chans x 31250 Hz (gmr1_rx_sdr.py:444-461): one stream
		if ((r = run_resamp(st, p->pre_rs, p->d_pre_bank, 1, Span{x, (long long)n_in, 0, d_pre, np, np, {}}, rotation))) return r;
		x = d_pre;
		rotation = 0.0f;
	}
	if ((r = run_pfb(st, *p, d_slot, n_sel, Span{x, np, 0, d_mid, (long long)T, 0, {}, fmt}, rotation))) return r;
	return run_resamp(st, p->rs, p->d_bank, n_sel,
	                  Span{d_mid, (long long)T, 0, reinterpret_cast<float2 *>(out), (long long)n_out, (long long)out_stride, {}},
	                  0.0f, planar ? sps : 0, planar ? (long long)plane_stride : 0);
}

int gmr1_hip_channelize_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in,
                            float rotation, int n_sel, const int32_t *chan_idx,
                            float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return channelize_dev_impl(stream, samp_rate, sps, kIqF32, wide, n_in, rotation, n_sel, chan_idx, out, out_stride, 0, false,
	                           n_out_p);
}

int gmr1_hip_channelize_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in,
                               float rotation, int n_sel, const int32_t *chan_idx,
                               float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return channelize_dev_impl(stream, samp_rate, sps, fmt, wide, n_in, rotation, n_sel, chan_idx, out, out_stride, 0, false,
	                           n_out_p);
}

int gmr1_hip_channelize_planar_dev(void *stream, double samp_rate, int sps, const float *wide, uint64_t n_in,
                                   float rotation, int n_sel, const int32_t *chan_idx,
                                   float *out_planes, uint64_t out_stride, uint64_t plane_stride, uint64_t *n_out_p)
{
	return channelize_dev_impl(stream, samp_rate, sps, kIqF32, wide, n_in, rotation, n_sel, chan_idx, out_planes, out_stride,
	                           plane_stride, true, n_out_p);
}

int gmr1_hip_channelize_planar_iq_dev(void *stream, double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in,
                                      float rotation, int n_sel, const int32_t *chan_idx,
                                      float *out_planes, uint64_t out_stride, uint64_t plane_stride, uint64_t *n_out_p)
{
	return channelize_dev_impl(stream, samp_rate, sps, fmt, wide, n_in, rotation, n_sel, chan_idx, out_planes, out_stride,
	                           plane_stride, true, n_out_p);
}

static int channelize_host_impl(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, float rotation,
                                int n_sel, const int32_t *chan_idx, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if ((r = checked_fmt("channelize", fmt))) return r;
	if (!wide || n_sel < 0 || (n_sel && (!chan_idx || !out)))
		return fail(-EINVAL, "channelize: wide / chan_idx / out are required");
	uint64_t n_out;
	r = gmr1_hip_channelize_plan(samp_rate, sps, n_in, nullptr, nullptr, &n_out);
	if (r) return r;
	if (n_out_p) *n_out_p = n_out;
	if (!n_sel || !n_out) return 0;
	if (out_stride < n_out)
		return fail(-EINVAL, "channelize: out_stride too small");
	Stage sg;
	const void *d_w = stage_iq(sg, fmt, wide, (size_t)n_in);
	float *d_o = sg.out(out, (size_t)n_sel * out_stride * 2);
	if ((r = sg.err())) return r;
	r = channelize_dev_impl(nullptr, samp_rate, sps, fmt, d_w, n_in, rotation, n_sel, chan_idx, d_o, out_stride, 0, false, nullptr);
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_channelize(double samp_rate, int sps, const float *wide, uint64_t n_in, float rotation,
                        int n_sel, const int32_t *chan_idx, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return channelize_host_impl(samp_rate, sps, kIqF32, wide, n_in, rotation, n_sel, chan_idx, out, out_stride, n_out_p);
}

int gmr1_hip_channelize_iq(double samp_rate, int sps, int fmt, const void *wide, uint64_t n_in, float rotation,
                           int n_sel, const int32_t *chan_idx, float *out, uint64_t out_stride, uint64_t *n_out_p)
{
	return channelize_host_impl(samp_rate, sps, fmt, wide, n_in, rotation, n_sel, chan_idx, out, out_stride, n_out_p);
}

int gmr1_hip_iq_sample_bytes(int fmt)
{
	const int b = iq_sample_bytes(fmt);
	return b < 0 ? -EINVAL : b;
}

}  // extern "C"
