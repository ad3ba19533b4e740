// capi_demod.cpp -- the demodulation batch entry points (gmr1_hip_demod_batch*, gmr1_hip_tch3_rx_batch*, gmr1_hip_demod_taps)
// and what the other translation units launch a demodulation through (demod_dev_impl, demod_host_impl, demod_dev_energy).
// Which kernel a batch gets is decided in rx_select.h.
#include "capi_common.h"
#include "rx_debug.h"
#include "rx_select.h"

namespace gmr1 {

int dbg_stop_env()
{
	static const int v = profile_env_int("GMR1_HIP_DBG_STOP", 0);
	return v;
}

namespace {

// the descriptor of a built-in burst type (host copy)
int builtin_type(int burst_id, const DevBurst **out)
{
	if (burst_id < 0 || burst_id >= GMR1_HIP_N_BURSTS)
		return fail(-EINVAL, "bad burst id %d", burst_id);
	int r = host_types();
	if (r) return r;
	*out = &g_host_types[burst_id];
	return 0;
}

// the launch arguments of a demodulation batch, with the kernel chosen for it (RxArgs::impl); `who` opens the error texts
int demod_args(const char *who, int type, const DevBurst &ht,
               int n, int sps, int in_len, const float *iq, const uint64_t *offset,
               const float *freq_shift, int8_t *ebits, int ebits_stride, int32_t *sync_id,
               float *toa, float *freq_err, float *ssyms, int32_t *rv, float *energy, RxArgs *out)
{
	if (n < 0 || !iq || !offset || !rv)
		return fail(-EINVAL, "%s: n/iq/offset/rv are required", who);
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "%s: sps=%d out of range (1..16)", who, sps);
	const int w = in_len - ht.len * sps + 1;
	if (w < 1 || in_len > kMaxInLen)
		return fail(-EINVAL, "%s: window of %d samples gives %d lags (>= 1, <= %d samples supported)", who, in_len, w, kMaxInLen);
	if (ebits && ebits_stride < ht.ebits)
		return fail(-EINVAL, "%s: ebits_stride %d < %d", who, ebits_stride, ht.ebits);
	RxArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.sps = sps; a.in_len[0] = a.in_len[1] = in_len;
	a.fixed_type = type;
	a.ebits_stride = ebits_stride;
	a.ssyms_stride = ht.len;
	a.dbg_stop = dbg_stop_env();
	a.iq = reinterpret_cast<const float2 *>(iq);
	a.offset = offset; a.freq_shift = freq_shift;
	a.ebits = ebits; a.sync_id = sync_id; a.toa = toa; a.freq_err = freq_err; a.ssyms = ssyms; a.rv = rv;
	a.energy = energy;
	// profiling only: GMR1_HIP_RX_GEN=0 keeps every batch on k_rx
	static const bool gen_off = profile_env_int("GMR1_HIP_RX_GEN", 1) == 0;
	if (!gen_off)
		a.impl = demod_kernel_choice(ht, n, sps, in_len, a.dbg_stop, &a.stage_samples);
	*out = a;
	return 0;
}

}  // namespace

int demod_dev_impl(hipStream_t st, int type, const DevBurst &ht,
                   int n, int sps, int in_len, const float *iq, const uint64_t *offset,
                   const float *freq_shift, int8_t *ebits, int ebits_stride, int32_t *sync_id,
                   float *toa, float *freq_err, float *ssyms, int32_t *rv, float *energy)
{
	RxArgs a;
	int r = demod_args("demod", type, ht, n, sps, in_len, iq, offset, freq_shift, ebits, ebits_stride, sync_id, toa, freq_err,
	                   ssyms, rv, energy, &a);
	if (r) return r;
	HIP_TRY(launch_rx(a, false, in_len, st));
	return 0;
}

// built-in burst type, device pointers, with the burst_energy() output the receive loop needs
int demod_dev_energy(hipStream_t st, int burst_id, int n, int sps, int in_len, const float *iq,
                     const uint64_t *offset, const float *freq_shift, int8_t *ebits, int ebits_stride,
                     int32_t *sync_id, float *toa, float *energy, int32_t *rv)
{
	const DevBurst *ht;
	int r = builtin_type(burst_id, &ht);
	if (r) return r;
	DevState *s;
	r = dev_state(&s);
	if (r) return r;
	return demod_dev_impl(st, burst_id, *ht, n, sps, in_len, iq, offset, freq_shift,
	                      ebits, ebits_stride, sync_id, toa, nullptr, nullptr, rv, energy);
}

// host-pointer staging shared by the batch wrapper and the legacy call
int demod_host_impl(int type, const DevBurst &ht, const DevBurst *custom,
                           int n, int sps, int in_len, const float *iq, uint64_t iq_len,
                           const uint64_t *offset, const float *freq_shift,
                           int8_t *ebits, int ebits_stride, int32_t *sync_id,
                           float *toa, float *freq_err, float *ssyms, int32_t *rv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0)
		return 0;
	if ((r = bursts_fit(n, offset, in_len, iq_len))) return r;
	hipStream_t st = nullptr;
	// a caller-defined description occupies the one spare table slot for the duration of the call: two threads
	// demodulating different custom formats must not interleave upload and launch
	std::unique_lock<std::mutex> lk(custom_slots_mutex(), std::defer_lock);
	if (custom) {
		lk.lock();
		HIP_TRY(upload_types(custom, kCustomSlot, 1, st));
	}
	Stage sg(st);
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const uint64_t *d_off = sg.in(offset, (size_t)n);
	const float *d_fs = sg.in(freq_shift, (size_t)n);
	int32_t *d_rv = sg.out(rv, (size_t)n);
	// rows further apart than the soft bits fill: what lies between them is the caller's, and comes back as it was
	int8_t *d_eb = ebits_stride > ht.ebits ? sg.inout(ebits, (size_t)n * ebits_stride) : sg.out(ebits, (size_t)n * ebits_stride);
	int32_t *d_sid = sg.out(sync_id, (size_t)n);
	float *d_toa = sg.out(toa, (size_t)n);
	float *d_fe = sg.out(freq_err, (size_t)n);
	float *d_ss = sg.out(ssyms, (size_t)n * ht.len);
	if ((r = sg.err())) return r;
	r = demod_dev_impl(st, type, ht, n, sps, in_len, d_iq, d_off, d_fs, d_eb, ebits_stride, d_sid, d_toa, d_fe, d_ss,
	                   d_rv);
	if (r) return r;
	return sg.fetch();
}

}  // namespace gmr1

using namespace gmr1;

extern "C" {

// What rx_tch3 does with a speech burst (gmr1_rx.c:551-587): gmr1_pi4cxpsk_demod of the NT3 speech format, then
// gmr1_tch3_decode of its 212 soft bits -- for a batch, in ONE launch where the four-bursts-per-wave demodulator applies
// (k_rx4g_tch3: the soft bits never leave LDS), otherwise as the two launches the separate entry points make.
int gmr1_hip_tch3_rx_batch_dev(void *stream, int n, int sps, int in_len,
                               const float *iq, const uint64_t *offset, const float *freq_shift,
                               int m, const uint8_t *ciph,
                               int8_t *ebits, int32_t *sync_id, float *toa, int32_t *rv,
                               uint8_t *frames, uint8_t *bits_s, int32_t *conv)
{
	if (n < 0 || !iq || !offset || !rv || !frames)
		return fail(-EINVAL, "tch3 rx: n/iq/offset/rv/frames are required");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n == 0) return 0;
	const int type = GMR1_HIP_NT3_SPEECH;
	const DevBurst &ht = g_host_types[type];
	RxArgs a;
	r = demod_args("demod", type, ht, n, sps, in_len, iq, offset, freq_shift, ebits, 212, sync_id, toa, nullptr, nullptr, rv, nullptr, &a);
	if (r) return r;
	Tch3Args t;
	t.n = n; t.m = m ? 1 : 0; t.conv_acc = conv_acc(); t.ebits = ebits; t.ciph = ciph; t.frames = frames; t.bits_s = bits_s;
	t.conv = conv;
	if (a.impl == 3 && ht.ebits == 212 && a.dbg_stop == 0) {
		HIP_TRY(launch_rx_tch3(a, t, (hipStream_t)stream));
		return 0;
	}
	// two launches; the soft bits pass through the caller's buffer or the library's workspace
	WsLease lease;
	if (!ebits) {
		void *ws;
		if ((r = lease.acquire(s, (hipStream_t)stream))) return r;
		r = dev_workspace(s, (size_t)n * 212, &ws);
		if (r) return r;
		a.ebits = reinterpret_cast<int8_t *>(ws);
		t.ebits = a.ebits;
	}
	HIP_TRY(launch_rx(a, false, in_len, (hipStream_t)stream));
	HIP_TRY(launch_tch3(t, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_demod_batch_dev(void *stream, int burst_id, int n, int sps, int in_len,
                             const float *iq, const uint64_t *offset, const float *freq_shift,
                             int8_t *ebits, int ebits_stride, int32_t *sync_id,
                             float *toa, float *freq_err, float *ssyms, int32_t *rv)
{
	const DevBurst *ht;
	int r = builtin_type(burst_id, &ht);
	if (r) return r;
	DevState *s;
	r = dev_state(&s);
	if (r) return r;
	return demod_dev_impl((hipStream_t)stream, burst_id, *ht, n, sps, in_len,
	                      iq, offset, freq_shift, ebits, ebits_stride, sync_id, toa, freq_err, ssyms, rv);
}

// host pointers: staged through HBM
int gmr1_hip_tch3_rx_batch(int n, int sps, int in_len,
                           const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                           int m, const uint8_t *ciph,
                           int8_t *ebits, int32_t *sync_id, float *toa, int32_t *rv,
                           uint8_t *frames, uint8_t *bits_s, int32_t *conv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0)
		return 0;
	if (!iq || !offset || !rv || !frames)
		return fail(-EINVAL, "tch3 rx: n/iq/offset/rv/frames are required");
	if ((r = bursts_fit(n, offset, in_len, iq_len))) return r;
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const uint64_t *d_off = sg.in(offset, (size_t)n);
	const float *d_fs = sg.in(freq_shift, (size_t)n);
	const uint8_t *d_ci = sg.in(ciph, (size_t)n * 208);
	int32_t *d_rv = sg.out(rv, (size_t)n);
	uint8_t *d_fr = sg.out(frames, (size_t)n * 20);
	int8_t *d_eb = sg.out(ebits, (size_t)n * 212);
	int32_t *d_sid = sg.out(sync_id, (size_t)n);
	float *d_toa = sg.out(toa, (size_t)n);
	uint8_t *d_s = sg.out(bits_s, (size_t)n * 4);
	int32_t *d_conv = sg.out(conv, (size_t)n * 2);
	if ((r = sg.err())) return r;
	r = gmr1_hip_tch3_rx_batch_dev(nullptr, n, sps, in_len, d_iq, d_off, d_fs, m, d_ci, d_eb, d_sid, d_toa, d_rv, d_fr,
	                               d_s, d_conv);
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_demod_batch(int burst_id, int n, int sps, int in_len,
                         const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                         int8_t *ebits, int ebits_stride, int32_t *sync_id,
                         float *toa, float *freq_err, float *ssyms, int32_t *rv)
{
	const DevBurst *ht;
	int r = builtin_type(burst_id, &ht);
	if (r) return r;
	return demod_host_impl(burst_id, *ht, nullptr, n, sps, in_len, iq, iq_len, offset,
	                       freq_shift, ebits, ebits_stride, sync_id, toa, freq_err, ssyms, rv);
}

// Debugging aid: one burst demodulated exactly as gmr1_hip_demod_batch does, plus the four intermediate vectors the
// reference writes out under ENABLE_DEBUG_SIGNAL (include/osmocom/gmr1/sdr/defs.h:35-39; pi4cxpsk.c:251,345,545,582).
// Host pointers, blocking, one wave: for looking at ONE burst of a capture that decodes differently, not a data path.
int gmr1_hip_demod_taps(int burst_id, int sps, int in_len, const float *iq, float freq_shift,
                        float *corr, float *burst, float *align, float *final_,
                        int8_t *ebits, int32_t *sync_id, float *toa, float *freq_err, float *ssyms, int32_t *rv)
{
	const DevBurst *htp;
	int r = builtin_type(burst_id, &htp);
	if (r) return r;
	const DevBurst &ht = *htp;
	if (!iq || !rv)
		return fail(-EINVAL, "demod taps: iq and rv are required");
	// the range checks and the launch arguments of a batch of one (never the four-per-wave kernels); the pointers are
	// the staged copies, filled in below, and the debug stops stay off
	const uint64_t zero = 0;
	RxArgs a;
	r = demod_args("demod taps", burst_id, ht, 1, sps, in_len, iq, &zero, nullptr, nullptr, ht.ebits, nullptr, nullptr, nullptr,
	               nullptr, rv, nullptr, &a);
	if (r) return r;
	a.dbg_stop = 0;
	const int w = in_len - ht.len * sps + 1;
	DevState *s;
	r = dev_state(&s);
	if (r) return r;
	Stage sg;
	const size_t n_taps = (size_t)w + 2 * (size_t)in_len + 4 * (size_t)ht.len;     // floats: corr, burst, align, final
	a.iq = reinterpret_cast<const float2 *>(sg.in(iq, (size_t)in_len * 2));
	a.offset = sg.in(&zero, 1);
	a.freq_shift = sg.in(&freq_shift, 1);
	a.ebits = sg.out_always(ebits, (size_t)ht.ebits);
	a.sync_id = sg.out_always(sync_id, 1);
	a.toa = sg.out_always(toa, 1);
	a.freq_err = sg.out_always(freq_err, 1);
	a.ssyms = sg.out_always(ssyms, (size_t)ht.len);
	a.rv = sg.out(rv, 1);
	// (burst / align / final are complex: they come first so that they sit on 8-byte boundaries)
	float *t = sg.dev<float>(n_taps + 4);
	if ((r = sg.err())) return r;
	RxTapsOut o;
	o.burst = reinterpret_cast<float2 *>(t);
	o.align = o.burst + in_len;
	o.final_ = o.align + ht.len;
	o.corr = reinterpret_cast<float *>(o.final_ + ht.len);
	sg.back(corr, o.corr, (size_t)w);
	sg.back(burst, reinterpret_cast<float *>(o.burst), (size_t)in_len * 2);
	sg.back(align, reinterpret_cast<float *>(o.align), (size_t)ht.len * 2);
	sg.back(final_, reinterpret_cast<float *>(o.final_), (size_t)ht.len * 2);
	HIP_TRY(launch_rx_taps(a, o, nullptr));
	return sg.fetch();
}

}  // extern "C"
