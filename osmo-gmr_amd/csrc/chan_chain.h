// chan_chain.h -- what capi_chan.cpp (plans, cache, one-shot entries) and capi_chan_stream.cpp (the streaming handle) share:
// a plan is chan_plan.h's numbers plus their device copies; a stage of either chain is one function that fills the launch's
// arguments from the plan and a Span and launches it, so that a push and a one-shot call cannot drift apart.
#pragma once

#include "capi_common.h"
#include "chan_plan.h"
#include "iq_format.h"

#pragma GCC visibility push(hidden)
namespace gmr1 {

static_assert(kPlanMaxChans == kPfbMaxChans && kPlanMaxBlocks == kPfbMaxBlocks && kPlanMaxFirTaps == kDdcMaxTaps,
              "chan_plan.h restates the kernels' limits");
static_assert(sizeof(F2) == sizeof(float2), "F2 is uploaded as float2");

struct ChanPlan : ChanNumbers {
	float *d_taps = nullptr;
	float2 *d_bank = nullptr, *d_pre_bank = nullptr;
};
struct DdcPlan : DdcNumbers {
	float2 *d_taps2 = nullptr;               // real taps as (t, 0)
	float2 *d_bank = nullptr;
};
// the plan of (rate, sps) on the current device, made and uploaded once; -EINVAL with the plan's refusal
int get_plan(double samp_rate, int sps, const ChanPlan **out);
int get_plan(double samp_rate, int sps, const DdcPlan **out);
// what every entry starts from: the device's state, sps in range (`who` names the chain in the message), the plan
template <typename Plan> int checked_plan(const char *who, double samp_rate, int sps, const Plan **p, DevState **ds = nullptr)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "%s: sps=%d out of range (1..16)", who, sps);
	if (ds) *ds = s;
	return get_plan(samp_rate, sps, p);
}
// select_channels with its refusal as -EINVAL
int select_slots(int nch, int n_sel, const int32_t *chan_idx, std::vector<int32_t> &slot);

// What one launch of a stage covers.  One-shot: st zeroed, n_in / n_out the call's counts, rows n_in and n_out apart
// whatever the strides say (only the resampler's output stride is read).  A push: x the new samples, st.xt / xt0 / x0 / o0
// set, n_in / n_out the global ends; the stage puts the strides where its kernel reads them.  fmt: what x holds (iq_format.h)
// -- float2 is its type in F32 only; the filterbank and stage 1 of the direct mode read the others, nothing else does.
struct Span {
	const float2 *x;
	long long n_in, x_stride;
	float2 *y;
	long long n_out, y_stride;
	StreamIdx st;
	int fmt = kIqF32;
};
// -EINVAL for a format that is none of GMR1_HIP_IQ_* (`who` names the entry in the message)
int checked_fmt(const char *who, int fmt);
// an arbitrary resampler over n_slots rows (rotation: the pre-resampler's; planar_sps > 0: polyphase-planar output)
int run_resamp(hipStream_t st, const RsStage &rs, const float2 *bank, int n_slots, const Span &s, float rotation = 0.0f,
               int planar_sps = 0, long long plane_stride = 0);
int run_pfb(hipStream_t st, const ChanPlan &p, const int32_t *d_slot, int n_sel, const Span &s, float rotation);
// a decimating FIR of the direct mode: stage 1, every carrier from the one wideband stream ...
int run_fir(hipStream_t st, int n_sel, int decim, int ntaps, const float2 *taps, const double *rot, const Span &s);
// ... and stage 2, carrier by carrier on the one row of real taps (a stride of zero taps rows is not expressible)
int run_fir2(hipStream_t st, const DdcPlan &p, int n_sel, const Span &s);

}  // namespace gmr1
#pragma GCC visibility pop
