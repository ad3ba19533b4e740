// capi_chan_stream.cpp -- streaming: the same channelizer / direct mode (capi_chan.cpp) over a capture that arrives in pieces.
// Every output of both chains is causal -- filterbank instant t reads input up to sample (n_chans / 2) t, resampler output n
// inputs below its plan's T, direct-mode output m input up to m d1 -- and every kernel computes phases, rotations and
// filter positions from GLOBAL indices (StreamIdx, gmr1_dev.h).  So a handle keeps, per stage, only the history the next
// outputs reach back into: the last Lx wideband samples, and each intermediate stream as [retained tail | this push's new
// samples] in one buffer it owns.  A push computes exactly the outputs that have become computable, identical to a one-shot
// call's: each stage is the one-shot call's own function (chan_chain.h) over the handle's buffers and global counts.

#include "chan_chain.h"

#include <memory>

#include "../../include/gmr1_hip.h"

using namespace gmr1;

namespace {

// an intermediate stream of the handle: `rows` rows of `cap` complex samples, the first L the retained tail
struct StageBuf {
	float2 *p = nullptr;
	long long cap = 0;
	int L = 0, rows = 0;
	~StageBuf() { if (p) (void)hipFree(p); }
};

// zeroed: global indices before the stream's start read as zeros, as in a one-shot call
int stage_init(StageBuf &b, int L, int rows)
{
	b.L = L;
	b.rows = rows;
	b.cap = L;
	HIP_TRY(hipMalloc(&b.p, (size_t)(rows > 0 ? rows : 1) * L * sizeof(float2)));
	HIP_TRY(hipMemsetAsync(b.p, 0, (size_t)(rows > 0 ? rows : 1) * L * sizeof(float2), nullptr));
	return 0;
}

// room for n_new samples behind the tail (grow-only: the tails move over, on `st`, before the old buffer goes)
int stage_reserve(StageBuf &b, long long n_new, hipStream_t st)
{
	if (b.L + n_new <= b.cap)
		return 0;
	const long long cap = up_to((size_t)(b.L + n_new), 256);
	float2 *p = nullptr;
	HIP_TRY(hipMalloc(&p, (size_t)(b.rows > 0 ? b.rows : 1) * cap * sizeof(float2)));
	if (b.rows > 0)
		HIP_TRY(hipMemcpy2DAsync(p, cap * sizeof(float2), b.p, b.cap * sizeof(float2), b.L * sizeof(float2), b.rows,
		                         hipMemcpyDeviceToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	HIP_TRY(hipFree(b.p));
	b.p = p;
	b.cap = cap;
	return 0;
}

// the last L samples of each row's [tail | n_new] to the front (a job of the push's k_keep_tail launch)
void stage_keep(KeepTailArgs &k, StageBuf &b, long long n_new)
{
	if (n_new <= 0 || b.rows <= 0)
		return;
	KeepTail &j = k.job[k.n++];
	j.dst = b.p; j.a = b.p; j.b = nullptr;
	j.dst_stride = b.cap; j.a_stride = b.cap; j.b_stride = 0; j.na = b.L + n_new; j.nb = 0;
	j.L = b.L; j.rows = b.rows;
}

// a host array's grow-only device copy (gmr1_hip_chan_stream_push)
struct GrowBuf {
	void *p = nullptr;
	size_t bytes = 0;
	~GrowBuf() { if (p) (void)hipFree(p); }
	int reserve(size_t n)
	{
		if (n <= bytes)
			return 0;
		if (p) {
			HIP_TRY(hipFree(p));
			p = nullptr;
			bytes = 0;
		}
		HIP_TRY(hipMalloc(&p, n));
		bytes = n;
		return 0;
	}
};

}  // namespace

struct gmr1_hip_chan_stream {
	mutable std::mutex mu;               // one push at a time
	int device = -1;
	bool direct = false;                 // gmr1_hip_ddc_stream_create
	int fmt = kIqF32;                    // what a push's `wide` holds (iq_format.h), for life
	int n_sel = 0;
	float rotation = 0.0f;
	const ChanPlan *cp = nullptr;
	const DdcPlan *dp = nullptr;
	const RsStage *rs = nullptr;         // the plan's output resampler and its bank on the device
	const float2 *rs_bank = nullptr;
	uint64_t N = 0;                     // wideband samples pushed so far
	StageBuf xt;                         // the last Lx wideband samples (one row)
	// the two intermediate streams, where the plan has them (p set).  Channelizer: the pre-resampled capture (off the grid),
	// the 2x channel streams.  Direct mode: the two decimating FIRs' outputs (the second with d2 > 1).
	StageBuf a, b;
	StageBuf *rs_in = nullptr;           // the one the output resampler reads
	int32_t *d_slot = nullptr;           // channelizer: slot table, then the selection
	float2 *d_t1 = nullptr;              // direct mode: per-carrier stage-1 taps, then their rotation steps
	double *d_rot = nullptr;
	hipEvent_t ev = nullptr;             // recorded behind the last push
	hipStream_t last = nullptr;
	bool pushed = false;
	GrowBuf h_in, h_out;                 // gmr1_hip_chan_stream_push's device copies (h_in in the handle's format)
	GrowBuf conv;                        // off the grid, an integer push's samples as float2: the pre-resampler reads floats
	~gmr1_hip_chan_stream()
	{
		if (d_slot) (void)hipFree(d_slot);
		if (d_t1) (void)hipFree(d_t1);
		if (d_rot) (void)hipFree(d_rot);
		if (ev) (void)hipEventDestroy(ev);
	}
};

namespace {

StreamCounts stream_counts(const gmr1_hip_chan_stream *h, uint64_t n)
{
	return h->direct ? h->dp->counts(n) : h->cp->counts(n);
}

// a stage's Span in a push: it reads `in` -- [retained tail | the new samples, global x0 .. x1] --
Span reads(const StageBuf &in, uint64_t x0, uint64_t x1)
{
	Span s = {in.p + in.L, (long long)x1, in.cap, nullptr, 0, 0, {}};
	s.st.xt = in.p; s.st.xt0 = (long long)x0 - in.L; s.st.x0 = (long long)x0;
	return s;
}
// ... and writes the global outputs o0 .. o1 behind the tail of `out`
Span writes(Span s, const StageBuf &out, uint64_t o0, uint64_t o1)
{
	s.y = out.p + out.L; s.y_stride = out.cap; s.n_out = (long long)o1;
	s.st.o0 = (long long)o0;
	return s;
}

int stream_finish_create(std::unique_ptr<gmr1_hip_chan_stream> &h, gmr1_hip_chan_stream **out)
{
	HIP_TRY(hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
	HIP_TRY(hipStreamSynchronize(nullptr));     // the zeroed tails and uploaded tables are in place before any stream uses them
	*out = h.release();
	return 0;
}

// the device part of a push; the caller holds h->mu and has validated everything
int stream_push(hipStream_t st, gmr1_hip_chan_stream *h, const void *wide, uint64_t n_in, float2 *out, uint64_t out_stride)
{
	const uint64_t N0 = h->N, N1 = N0 + n_in;
	const StreamCounts c0 = stream_counts(h, N0), c1 = stream_counts(h, N1);
	if (h->pushed && st != h->last)
		HIP_TRY(hipStreamWaitEvent(st, h->ev, 0));
	const long long na = (long long)(c1.a - c0.a), nb = (long long)(c1.b - c0.b);
	int r, fmt = h->fmt;
	if (fmt != kIqF32 && !h->direct && h->cp->pre && n_in > 0) {
		// the one chain that converts up front: everything below, the kept tail included, then sees floats
		if ((r = h->conv.reserve(n_in * sizeof(float2)))) return r;
		HIP_TRY(launch_iq_convert(wide, fmt, (long long)n_in, static_cast<float2 *>(h->conv.p), st));
		wide = h->conv.p;
		fmt = kIqF32;
	}
	Span in = reads(h->xt, N0, N1);      // the wideband chunk behind the retained samples: the caller's, never copied
	in.x = static_cast<const float2 *>(wide); in.x_stride = 0; in.fmt = fmt;
	if (h->a.p && (r = stage_reserve(h->a, na, st))) return r;
	if (h->b.p && (r = stage_reserve(h->b, nb, st))) return r;
	if (!h->direct) {
		const ChanPlan &p = *h->cp;
		if (p.pre && na > 0 && (r = run_resamp(st, p.pre_rs, p.d_pre_bank, 1, writes(in, h->a, c0.a, c1.a), h->rotation)))
			return r;
		if (h->n_sel > 0 && nb > 0 &&
		    (r = run_pfb(st, p, h->d_slot, h->n_sel, writes(p.pre ? reads(h->a, c0.a, c1.a) : in, h->b, c0.b, c1.b),
		                 p.pre ? 0.0f : h->rotation)))
			return r;
	} else {
		const DdcPlan &p = *h->dp;
		if (h->n_sel > 0 && na > 0 &&
		    (r = run_fir(st, h->n_sel, p.d1, (int)p.taps1.size(), h->d_t1, h->d_rot, writes(in, h->a, c0.a, c1.a))))
			return r;
		if (p.d2 > 1 && nb > 0 && (r = run_fir2(st, p, h->n_sel, writes(reads(h->a, c0.a, c1.a), h->b, c0.b, c1.b))))
			return r;
	}
	if (h->n_sel > 0 && c1.out > c0.out) {
		Span s = reads(*h->rs_in, c0.b, c1.b);
		s.y = out; s.y_stride = (long long)out_stride; s.n_out = (long long)c1.out; s.st.o0 = (long long)c0.out;
		if ((r = run_resamp(st, *h->rs, h->rs_bank, h->n_sel, s))) return r;
	}
	// what the next push reaches back into: the input's last Lx samples, each stage's last L
	KeepTailArgs keep;
	std::memset(&keep, 0, sizeof(keep));
	if (n_in > 0) {
		KeepTail &j = keep.job[keep.n++];
		j.dst = h->xt.p; j.a = h->xt.p; j.b = wide; j.na = h->xt.L; j.nb = (long long)n_in; j.L = h->xt.L; j.rows = 1;
		keep.b_fmt = fmt;                    // kept as float2: converted as it is kept
	}
	if (h->a.p)
		stage_keep(keep, h->a, na);
	if (h->b.p)
		stage_keep(keep, h->b, nb);
	HIP_TRY(launch_keep_tail(keep, st));
	HIP_TRY(hipEventRecord(h->ev, st));
	h->last = st;
	h->pushed = true;
	h->N = N1;
	return 0;
}

// the checks every push makes before it touches the handle: -EINVAL leaves the stream as it was.  as_f32: the push came
// through an entry whose `wide` is const float *
int stream_check(gmr1_hip_chan_stream *h, bool as_f32, const void *wide, uint64_t n_in, const float *out, uint64_t out_stride,
                 uint64_t *n_new)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (!h)
		return fail(-EINVAL, "chan_stream: no handle");
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	if (dev != h->device)
		return fail(-EINVAL, "chan_stream: the handle belongs to device %d, the current device is %d", h->device, dev);
	if (as_f32 && h->fmt != kIqF32)
		return fail(-EINVAL, "chan_stream: the handle reads format %d: push it with gmr1_hip_chan_stream_push_iq*", h->fmt);
	if (!wide)
		return fail(-EINVAL, "chan_stream: wide is required");
	if (n_in > (uint64_t)1 << 40)
		return fail(-EINVAL, "chan_stream: %llu samples in one push", (unsigned long long)n_in);
	*n_new = stream_counts(h, h->N + n_in).out - stream_counts(h, h->N).out;
	if (h->n_sel > 0 && *n_new > 0) {
		if (!out)
			return fail(-EINVAL, "chan_stream: out is required");
		if (out_stride < *n_new)
			return fail(-EINVAL, "chan_stream: out_stride %llu < %llu new output samples per stream",
			            (unsigned long long)out_stride, (unsigned long long)*n_new);
	}
	return 0;
}

}  // namespace

extern "C" {

int gmr1_hip_channelize_stream_create_iq(double samp_rate, int sps, int fmt, float rotation, int n_sel,
                                         const int32_t *chan_idx, struct gmr1_hip_chan_stream **out)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if ((r = checked_fmt("channelize_stream", fmt))) return r;
	if (!out || n_sel < 0 || (n_sel && !chan_idx))
		return fail(-EINVAL, "channelize_stream: chan_idx / handle are required");
	const ChanPlan *p;
	if ((r = checked_plan("channelize", samp_rate, sps, &p)))
		return r;
	std::vector<int32_t> slot;
	if ((r = select_slots(p->n_chans, n_sel, chan_idx, slot)))
		return r;
	std::unique_ptr<gmr1_hip_chan_stream> h(new gmr1_hip_chan_stream);
	HIP_TRY(hipGetDevice(&h->device));
	h->fmt = fmt; h->n_sel = n_sel; h->rotation = rotation; h->cp = p; h->rs = &p->rs; h->rs_bank = p->d_bank; h->rs_in = &h->b;
	// history: the filterbank reaches ntaps + n_chans / 2 inputs behind its first new instant (n_blocks n_chans + n_chans
	// covers it); the pre-resampler its taps and one step
	const int l_pfb = (p->n_blocks + 1) * p->n_chans;
	const int lx = p->pre ? resamp_history(p->pre_rs) : l_pfb;
	if ((r = stage_init(h->xt, lx, 1)) || (p->pre && (r = stage_init(h->a, l_pfb, 1))) ||
	    (r = stage_init(h->b, resamp_history(p->rs), n_sel)))
		return r;
	std::vector<int32_t> tab(2 * kPfbMaxChans, -1);
	std::copy(slot.begin(), slot.end(), tab.begin());
	std::copy(chan_idx, chan_idx + n_sel, tab.begin() + kPfbMaxChans);
	HIP_TRY(hipMalloc(&h->d_slot, tab.size() * sizeof(int32_t)));
	HIP_TRY(hipMemcpy(h->d_slot, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
	return stream_finish_create(h, out);
}

int gmr1_hip_channelize_stream_create(double samp_rate, int sps, float rotation, int n_sel, const int32_t *chan_idx,
                                      struct gmr1_hip_chan_stream **out)
{
	return gmr1_hip_channelize_stream_create_iq(samp_rate, sps, kIqF32, rotation, n_sel, chan_idx, out);
}

int gmr1_hip_ddc_stream_create_iq(double samp_rate, int sps, int fmt, int n_sel, const double *freq_hz,
                                  struct gmr1_hip_chan_stream **out)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if ((r = checked_fmt("ddc_stream", fmt))) return r;
	if (!out || n_sel < 0 || (n_sel && !freq_hz))
		return fail(-EINVAL, "ddc_stream: freq_hz / handle are required");
	const DdcPlan *p;
	if ((r = checked_plan("ddc", samp_rate, sps, &p)))
		return r;
	std::unique_ptr<gmr1_hip_chan_stream> h(new gmr1_hip_chan_stream);
	HIP_TRY(hipGetDevice(&h->device));
	h->direct = true; h->fmt = fmt; h->n_sel = n_sel; h->dp = p; h->rs = &p->rs; h->rs_bank = p->d_bank; h->rs_in = p->d2 > 1 ? &h->b : &h->a;
	const int l_rs = resamp_history(p->rs);
	const int l_fir1 = (int)p->taps1.size() + p->d1 + 1;
	if ((r = stage_init(h->xt, (int)up_to((size_t)l_fir1, 64), 1)) ||
	    (r = stage_init(h->a, p->d2 > 1 ? (int)up_to(p->taps2.size() + p->d2 + 1, 64) : l_rs, n_sel)) ||
	    (p->d2 > 1 && (r = stage_init(h->b, l_rs, n_sel))))
		return r;
	std::vector<F2> t1;
	std::vector<double> rot;
	ddc_carrier_taps(*p, n_sel, freq_hz, t1, rot);
	HIP_TRY(hipMalloc(&h->d_t1, (t1.empty() ? 1 : t1.size()) * sizeof(float2)));
	HIP_TRY(hipMalloc(&h->d_rot, (rot.empty() ? 1 : rot.size()) * sizeof(double)));
	HIP_TRY(hipMemcpy(h->d_t1, t1.data(), t1.size() * sizeof(float2), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(h->d_rot, rot.data(), rot.size() * sizeof(double), hipMemcpyHostToDevice));
	return stream_finish_create(h, out);
}

int gmr1_hip_ddc_stream_create(double samp_rate, int sps, int n_sel, const double *freq_hz, struct gmr1_hip_chan_stream **out)
{
	return gmr1_hip_ddc_stream_create_iq(samp_rate, sps, kIqF32, n_sel, freq_hz, out);
}

int gmr1_hip_chan_stream_out_len(const struct gmr1_hip_chan_stream *h, uint64_t n_in, uint64_t *n_out)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (!h || !n_out)
		return fail(-EINVAL, "chan_stream_out_len: handle / n_out are required");
	std::lock_guard<std::mutex> lk(h->mu);
	*n_out = stream_counts(h, h->N + n_in).out - stream_counts(h, h->N).out;
	return 0;
}

static int push_dev_impl(void *stream, struct gmr1_hip_chan_stream *h, bool as_f32, const void *wide, uint64_t n_in,
                         float *out, uint64_t out_stride, uint64_t *n_out)
{
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	uint64_t n_new = 0;
	int r = stream_check(h, as_f32, wide, n_in, out, out_stride, &n_new);
	if (r) return r;
	if ((r = stream_push((hipStream_t)stream, h, wide, n_in, reinterpret_cast<float2 *>(out), out_stride)))
		return r;
	if (n_out) *n_out = n_new;
	return 0;
}

static int push_host_impl(struct gmr1_hip_chan_stream *h, bool as_f32, const void *wide, uint64_t n_in, float *out,
                          uint64_t out_stride, uint64_t *n_out)
{
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	uint64_t n_new = 0;
	int r = stream_check(h, as_f32, wide, n_in, out, out_stride, &n_new);
	if (r) return r;
	const size_t out_rows = h->n_sel > 0 && n_new > 0 ? (size_t)h->n_sel : 0;
	const size_t in_bytes = n_in * (size_t)iq_sample_bytes(h->fmt);      // the upload is the format's bytes
	if ((r = h->h_in.reserve(in_bytes)) || (r = h->h_out.reserve(out_rows * n_new * sizeof(float2))))
		return r;
	if (n_in)
		HIP_TRY(hipMemcpyAsync(h->h_in.p, wide, in_bytes, hipMemcpyHostToDevice, nullptr));
	if ((r = stream_push(nullptr, h, h->h_in.p ? h->h_in.p : h->xt.p, n_in, static_cast<float2 *>(h->h_out.p), n_new)))
		return r;
	if (out_rows)
		HIP_TRY(hipMemcpy2DAsync(out, out_stride * sizeof(float2), h->h_out.p, n_new * sizeof(float2), n_new * sizeof(float2),
		                         out_rows, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	if (n_out) *n_out = n_new;
	return 0;
}

int gmr1_hip_chan_stream_push_dev(void *stream, struct gmr1_hip_chan_stream *h, const float *wide, uint64_t n_in,
                                  float *out, uint64_t out_stride, uint64_t *n_out)
{
	return push_dev_impl(stream, h, true, wide, n_in, out, out_stride, n_out);
}

int gmr1_hip_chan_stream_push_iq_dev(void *stream, struct gmr1_hip_chan_stream *h, const void *wide, uint64_t n_in,
                                     float *out, uint64_t out_stride, uint64_t *n_out)
{
	return push_dev_impl(stream, h, false, wide, n_in, out, out_stride, n_out);
}

int gmr1_hip_chan_stream_push(struct gmr1_hip_chan_stream *h, const float *wide, uint64_t n_in, float *out,
                              uint64_t out_stride, uint64_t *n_out)
{
	return push_host_impl(h, true, wide, n_in, out, out_stride, n_out);
}

int gmr1_hip_chan_stream_push_iq(struct gmr1_hip_chan_stream *h, const void *wide, uint64_t n_in, float *out,
                                 uint64_t out_stride, uint64_t *n_out)
{
	return push_host_impl(h, false, wide, n_in, out, out_stride, n_out);
}

int gmr1_hip_chan_stream_destroy(struct gmr1_hip_chan_stream *h)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (!h)
		return 0;
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	const int own = h->device;
	if (dev != own)
		HIP_TRY(hipSetDevice(own));          // its memory is freed on its own device
	{
		std::lock_guard<std::mutex> lk(h->mu);
		if (h->pushed)
			(void)hipEventSynchronize(h->ev);      // nothing of the handle's is still in use when it goes
	}
	delete h;
	if (dev != own)
		HIP_TRY(hipSetDevice(dev));
	return 0;
}

}  // extern "C"
