// capi_fcch.cpp -- C-ABI entry points of the FCCH acquisition kernels.
#include "capi_common.h"
#include "profile_env.h"
#include "fcch_acq.h"

using namespace gmr1;

namespace {

int fcch_tab_of(const struct gmr1_fcch_burst *bt)
{
	for (int i = 0; i < kFcchTabs; i++)
		if (bt == kFcchBuiltin[i])
			return i;
	// a caller-provided descriptor with the parameters of a built-in one is accepted too
	for (int i = 0; i < kFcchTabs; i++)
		if (bt && bt->len == kFcchBuiltin[i]->len && bt->freq == kFcchBuiltin[i]->freq)
			return i;
	return -1;
}

const AcqTail &no_tail()
{
	static const AcqTail none = [] { AcqTail t; std::memset(&t, 0, sizeof(t)); return t; }();
	return none;
}

int rough_dev(hipStream_t st, int tab, int n, int sps, int len, const float *iq, const uint64_t *offset,
              const float *freq_shift, int32_t *toa, int32_t *rv, float *energy, size_t energy_stride,
              const AcqTail &tl = no_tail())
{
	if (tab < 0 || tab >= kFcchTabs)
		return fail(-EINVAL, "fcch: unknown burst type");
	if (n < 0 || !iq || !offset || (!toa && !energy))
		return fail(-EINVAL, "fcch_rough: NULL argument");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "fcch_rough: sps=%d out of range", sps);
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n == 0) return 0;
	const int ntaps = kFcchBuiltin[tab]->len;
	const int ndec = len / sps;
	const int nlags = ndec - ntaps + 1;
	if (nlags < 5)
		return fail(-EINVAL, "fcch_rough: window of %d samples is too short", len);
	FcchRoughArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.len = len; a.sps = sps; a.tab = tab;
	a.iq = reinterpret_cast<const float2 *>(iq);
	a.offset = offset; a.freq_shift = freq_shift;
	a.n_lag_tiles = fcch_lag_tiles(nlags);
	// the one-pass sweep keeps its statistics partials per lag tile (fcch_kernels.hip: k_fcch_sweep)
	a.n_stat_tiles = fcch_one_pass() ? a.n_lag_tiles : fcch_stat_tiles(len);
	a.dec_stride = ((size_t)ndec + 15) & ~(size_t)15;
	const size_t b_dec = (size_t)n * a.dec_stride * 8;
	const size_t b_par = (((size_t)n * a.n_stat_tiles * 16) + 255) & ~(size_t)255;
	const size_t b_best = (((size_t)n * a.n_lag_tiles * 32) + 255) & ~(size_t)255;
	void *ws;
	WsLease lease;
	if ((r = lease.acquire(s, st))) return r;
	r = dev_workspace(s, b_dec + b_par + b_best, &ws);
	if (r) return r;
	a.dec = static_cast<float2 *>(ws);
	a.partial = reinterpret_cast<float *>(static_cast<char *>(ws) + b_dec);
	a.tile_best = reinterpret_cast<float *>(static_cast<char *>(ws) + b_dec + b_par);
	a.energy = energy; a.energy_stride = energy_stride;
	a.toa = toa; a.rv = rv;
	// the folded sweep's statistics records: a buffer of its own (per device, grow-only, zeroed when made), written by these
	// kernels only, so that a record carrying this launch's epoch can only be this launch's.  Under the workspace lease: one
	// sweep at a time per device.
	{
		// 32 bytes a record slot, slot = stream * tiles + tile; the epoch words only ever hold epochs (or the zero they were made
		// with), so whatever geometry the last sweep had, a word carrying THIS launch's epoch was written by this launch
		struct FoldBuf { char *p = nullptr; size_t slots = 0; uint32_t epoch = 0; };
		static FoldBuf fold_of[64];
		int dev = 0;
		HIP_TRY(hipGetDevice(&dev));
		if (dev >= 0 && dev < 64 && a.n_stat_tiles == a.n_lag_tiles) {
			FoldBuf &fb = fold_of[dev];
			const size_t n_rec = (size_t)n * a.n_stat_tiles;
			if (fb.slots < n_rec) {
				// (a sweep of an earlier call may still be polling the old buffer)
				HIP_TRY(hipDeviceSynchronize());
				if (fb.p) HIP_TRY(hipFree(fb.p));
				fb.p = nullptr; fb.slots = 0;
				const size_t cap = n_rec + n_rec / 2;
				HIP_TRY(hipMalloc(&fb.p, cap * 32));
				HIP_TRY(hipMemset(fb.p, 0, cap * 32));
				fb.slots = cap;
				fb.epoch = 0;
			}
			if (++fb.epoch == 0) {                     // (once in four billion sweeps)
				HIP_TRY(hipDeviceSynchronize());
				HIP_TRY(hipMemset(fb.p, 0, fb.slots * 32));
				fb.epoch = 1;
			}
			a.fold_partial = reinterpret_cast<float *>(fb.p);
			a.epoch = fb.epoch;
			// (a poll is three coherent 8-byte loads and a short sleep, a microsecond or two: the bound is some tens of milliseconds.
			// Profiling build: GMR1_HIP_FCCH_FOLD_POLLS=0 makes every tile give up at once -- the fallback path, for the tests)
			static const int polls = profile_env_int("GMR1_HIP_FCCH_FOLD_POLLS", 1 << 14);
			a.fold_polls = polls;
			// (profiling build: GMR1_HIP_FCCH_FOLD_GIVEUP=k,r makes the tiles with tile % k == r give up as if their wait had run
			// out, the others fold -- a stream whose tiles did not start together; a negative r counts from the stream's end)
			static const std::pair<int, int> giveup = [] {
				const char *e = profile_env("GMR1_HIP_FCCH_FOLD_GIVEUP");
				int k = 0, r = 0;
				if (!e || sscanf(e, "%d,%d", &k, &r) != 2 || k < 1) k = r = 0;
				return std::make_pair(k, r);
			}();
			a.fold_giveup_k = giveup.first;
			a.fold_giveup_r = giveup.second;
		}
	}
	// (profiling build: GMR1_HIP_FCCH_POISON=1 fills the lag / sample scratch with 0x4f bytes, about 3.5e9 a float, first: a lag
	// that no tile wrote then decides the pick, whatever earlier calls left there)
	static const bool poison = profile_env_int("GMR1_HIP_FCCH_POISON", 0) != 0;
	if (poison)
		HIP_TRY(hipMemsetAsync(a.dec, 0x4f, b_dec, st));
	HIP_TRY(launch_fcch_rough_tail(a, ntaps, tl, st));
	return 0;
}

int fine_dev(hipStream_t st, int tab, int mode, int n, int sps, const float *iq, const uint64_t *offset,
             const float *freq_shift, int32_t *toa, float *freq_err, float *snr, const AcqTail &tl = no_tail())
{
	if (tab < 0 || tab >= kFcchTabs)
		return fail(-EINVAL, "fcch: unknown burst type");
	if (n < 0 || !iq || !offset || (mode == 0 && (!toa || !freq_err)) || (mode == 1 && !snr))
		return fail(-EINVAL, "fcch_fine/snr: NULL argument");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "fcch_fine/snr: sps=%d out of range", sps);
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	FcchFineArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.sps = sps; a.tab = tab; a.mode = mode;
	a.iq = reinterpret_cast<const float2 *>(iq);
	a.offset = offset; a.freq_shift = freq_shift;
	a.toa = toa; a.freq_err = freq_err; a.snr = snr;
	HIP_TRY(launch_fcch_fine_tail(a, kFcchBuiltin[tab]->len, tl, st));
	return 0;
}

// shared host staging: iq + offsets (+ freq_shift) in; the callers add their outputs to `sg`
struct Staged {
	Stage sg;
	const float *iq = nullptr, *fs = nullptr;
	const uint64_t *off = nullptr;
	int stage(int n, const float *h_iq, uint64_t iq_len, const uint64_t *h_off, const float *h_fs,
	          uint64_t need)
	{
		for (int i = 0; i < n; i++)
			if (h_off[i] + need > iq_len)
				return fail(-EINVAL, "window %d runs past the end of iq", i);
		iq = sg.in(h_iq, (size_t)iq_len * 2);
		off = sg.in(h_off, (size_t)n);
		fs = sg.in(h_fs, (size_t)n);
		return 0;
	}
};

}  // namespace

extern "C" {

int gmr1_hip_fcch_rough_batch_dev(void *stream, int fcch_type, int n, int sps, int len,
                                  const float *iq, const uint64_t *offset, const float *freq_shift,
                                  int32_t *toa, int32_t *rv)
{
	return rough_dev((hipStream_t)stream, fcch_type, n, sps, len, iq, offset, freq_shift, toa, rv, nullptr, 0);
}

int gmr1_hip_fcch_rough_batch(int fcch_type, int n, int sps, int len,
                              const float *iq, uint64_t iq_len, const uint64_t *offset,
                              const float *freq_shift, int32_t *toa, int32_t *rv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!iq || !offset || !toa)
		return fail(-EINVAL, "fcch_rough: NULL argument");
	Staged st;
	r = st.stage(n, iq, iq_len, offset, freq_shift, (uint64_t)len);
	if (r) return r;
	int32_t *d_toa = st.sg.out(toa, (size_t)n);
	int32_t *d_rv = st.sg.out_always(rv, (size_t)n);
	if ((r = st.sg.err())) return r;
	r = rough_dev(nullptr, fcch_type, n, sps, len, st.iq, st.off, st.fs, d_toa, d_rv, nullptr, 0);
	if (r) return r;
	return st.sg.fetch();
}

int gmr1_hip_fcch_fine_batch_dev(void *stream, int fcch_type, int n, int sps,
                                 const float *iq, const uint64_t *offset, const float *freq_shift,
                                 int32_t *toa, float *freq_error)
{
	return fine_dev((hipStream_t)stream, fcch_type, 0, n, sps, iq, offset, freq_shift, toa, freq_error, nullptr);
}

int gmr1_hip_fcch_snr_batch_dev(void *stream, int fcch_type, int n, int sps,
                                const float *iq, const uint64_t *offset, const float *freq_shift,
                                float *snr)
{
	return fine_dev((hipStream_t)stream, fcch_type, 1, n, sps, iq, offset, freq_shift, nullptr, nullptr, snr);
}

int gmr1_hip_fcch_fine_batch(int fcch_type, int n, int sps,
                             const float *iq, uint64_t iq_len, const uint64_t *offset,
                             const float *freq_shift, int32_t *toa, float *freq_error)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (fcch_type < 0 || fcch_type >= kFcchTabs || !iq || !offset || !toa || !freq_error)
		return fail(-EINVAL, "fcch_fine: bad argument");
	Staged st;
	r = st.stage(n, iq, iq_len, offset, freq_shift, (uint64_t)kFcchBuiltin[fcch_type]->len * sps);
	if (r) return r;
	int32_t *d_toa = st.sg.out(toa, (size_t)n);
	float *d_fe = st.sg.out(freq_error, (size_t)n);
	if ((r = st.sg.err())) return r;
	r = fine_dev(nullptr, fcch_type, 0, n, sps, st.iq, st.off, st.fs, d_toa, d_fe, nullptr);
	if (r) return r;
	return st.sg.fetch();
}

int gmr1_hip_fcch_snr_batch(int fcch_type, int n, int sps,
                            const float *iq, uint64_t iq_len, const uint64_t *offset,
                            const float *freq_shift, float *snr)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (fcch_type < 0 || fcch_type >= kFcchTabs || !iq || !offset || !snr)
		return fail(-EINVAL, "fcch_snr: bad argument");
	Staged st;
	r = st.stage(n, iq, iq_len, offset, freq_shift, (uint64_t)kFcchBuiltin[fcch_type]->len * sps);
	if (r) return r;
	float *d_snr = st.sg.out(snr, (size_t)n);
	if ((r = st.sg.err())) return r;
	r = fine_dev(nullptr, fcch_type, 1, n, sps, st.iq, st.off, st.fs, nullptr, nullptr, d_snr);
	if (r) return r;
	return st.sg.fetch();
}

}  // extern "C"

namespace gmr1 {

int fcch_rough_tail(hipStream_t st, int tab, int n, int sps, int len, const float *iq, const uint64_t *offset,
                    const float *freq_shift, int32_t *toa, int32_t *rv, const AcqTail &t)
{
	return rough_dev(st, tab, n, sps, len, iq, offset, freq_shift, toa, rv, nullptr, 0, t);
}

int fcch_fine_tail(hipStream_t st, int tab, int mode, int n, int sps, const float *iq, const uint64_t *offset,
                   const float *freq_shift, int32_t *toa, float *freq_err, float *snr, const AcqTail &t)
{
	return fine_dev(st, tab, mode, n, sps, iq, offset, freq_shift, toa, freq_err, snr, t);
}

int fcch_rough_multi_tail(hipStream_t stream, int fcch_type, int n, int sps, int len,
                          const float *iq, const uint64_t *offset, const float *freq_shift,
                          int32_t *peaks_toa, int N, int32_t *count, const AcqTail &tl)
{
	if (fcch_type < 0 || fcch_type >= kFcchTabs || !peaks_toa || !count || N < 1 || N > 32)
		return fail(-EINVAL, "fcch_rough_multi: bad argument");
	if (sps < 1 || sps > 16)                                      // before any arithmetic that divides by it
		return fail(-EINVAL, "fcch_rough_multi: sps=%d out of range (1..16)", sps);
	if (len < ((650 * 23400 * sps) / 1000))                       // fcch.c:355-356
		return fail(-EINVAL, "fcch_rough_multi: needs at least 650 ms of signal");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	const int blen = kFcchBuiltin[fcch_type]->len;
	const int nlags = len / sps - blen + 1;
	const size_t estride = ((size_t)nlags + 63) & ~(size_t)63;
	// the energy plane lives behind the rough sweep's own scratch: ask for both at once
	const int ndec = len / sps;
	const size_t b_dec = (size_t)n * ((((size_t)ndec + 15) & ~(size_t)15) * 8);
	// (the statistics partials sized exactly as rough_dev sizes them -- per lag tile in the one-pass form, more of them than
	// kStatSpan tiles below 4 samples a symbol -- or the energy plane would start inside rough_dev's tile results)
	const int n_stat_tiles = fcch_one_pass() ? fcch_lag_tiles(nlags) : fcch_stat_tiles(len);
	const size_t b_par = (((size_t)n * n_stat_tiles * 16) + 255) & ~(size_t)255;
	const size_t b_best = (((size_t)n * fcch_lag_tiles(nlags) * 32) + 255) & ~(size_t)255;
	const size_t b_rough = b_dec + b_par + b_best;
	void *ws;
	WsLease lease;
	if ((r = lease.acquire(s, (hipStream_t)stream))) return r;
	r = dev_workspace(s, b_rough + (size_t)n * estride * 4, &ws);
	if (r) return r;
	float *energy = reinterpret_cast<float *>(static_cast<char *>(ws) + b_rough);
	r = rough_dev((hipStream_t)stream, fcch_type, n, sps, len, iq, offset, freq_shift, nullptr, nullptr,
	              energy, estride);
	if (r) return r;
	FcchMultiArgs m;
	std::memset(&m, 0, sizeof(m));
	m.n = n; m.sps = sps; m.burst_len = blen; m.N = N;
	m.nlags = nlags;
	m.Lp = (320 * 23400) / 1000;                                  // fcch.c:380-383
	m.Lw = m.Lp + blen;
	m.energy = energy; m.energy_stride = estride;
	m.toa = peaks_toa; m.count = count;
	HIP_TRY(launch_fcch_multi_tail(m, tl, stream));
	return 0;
}

namespace {
struct AcqBuf { void *p = nullptr; size_t n = 0; int dev = -1; };

// (per thread AND per device: a thread that moves on to another GPU must not hand that GPU's kernels this one's memory)
int acq_buf(AcqBuf &b, size_t bytes, bool *grew)
{
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	*grew = false;
	if (b.n >= bytes && b.dev == dev)
		return 0;
	if (b.p) {
		int back = dev;
		if (b.dev >= 0 && b.dev != dev && hipSetDevice(b.dev) == hipSuccess) {
			(void)hipFree(b.p);
			(void)hipSetDevice(back);
		} else {
			(void)hipFree(b.p);
		}
	}
	b.p = nullptr;
	b.n = 0;
	b.dev = dev;
	HIP_TRY(hipMalloc(&b.p, bytes + bytes / 4));
	b.n = bytes + bytes / 4;
	*grew = true;
	return 0;
}

// the spare window of the chain (AcqArgs::spare): n complex samples of noise, written once when the buffer is made
int acq_spare(size_t n, hipStream_t st, const float2 **out)
{
	static thread_local AcqBuf b;
	bool grew;
	int r = acq_buf(b, n * sizeof(float2), &grew);
	if (r) return r;
	if (grew) {
		// (later calls may come on other streams: the samples are there before this one returns)
		HIP_TRY(launch_acq_spare_fill(static_cast<float2 *>(b.p), b.n / sizeof(float2), st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	*out = static_cast<const float2 *>(b.p);
	return 0;
}

int acq_check(int tab, int n, int sps, const float *iq, const uint64_t *offset, const uint64_t *length, const void *out)
{
	if (tab < 0 || tab >= kFcchTabs)
		return fail(-EINVAL, "fcch_acquire: unknown burst type");
	if (n < 0 || !iq || !offset || !length || !out)
		return fail(-EINVAL, "fcch_acquire: NULL argument");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "fcch_acquire: sps=%d out of range (1..16)", sps);
	// (the spare window is addressed as iq + whole samples)
	if ((uintptr_t)iq & 7)
		return fail(-EINVAL, "fcch_acquire: iq is not aligned to a complex sample");
	return 0;
}
}  // namespace

int acq_scratch(int slot, size_t bytes, unsigned char **out)
{
	static thread_local AcqBuf b[2];
	bool grew;
	int r = acq_buf(b[slot & 1], bytes, &grew);
	if (r) return r;
	*out = static_cast<unsigned char *>(b[slot & 1].p);
	return 0;
}

int fcch_acquire_enqueue(hipStream_t st, int tab, int n, int sps, const float *iq, const uint64_t *offset,
                         const uint64_t *length, const int32_t *start, const uint64_t *h_length,
                         struct gmr1_hip_fcch_acq *out)
{
	// The five sweeps of fcch_single_init / fcch_multi_process (gmr1_rx.c:605-744) follow each other on the stream
	// without the host: k_acq_glue's steps (fcch_kernels.hip) do the additions and bound checks between them on the device
	// and lay out each next sweep's windows; candidate stages run over all kAcqPeaks slots of every carrier (a slot
	// without a candidate gets a harmless window).  k_acq_begin in front takes the checks on the lengths, k_acq_decide
	// behind takes the decisions from the sweeps' results and writes the caller's records.
	int r = acq_check(tab, n, sps, iq, offset, length, out);
	if (r) return r;
	if (n == 0) return 0;
	const int flen = kFcchBuiltin[tab]->len * sps;
	const int wl1 = (330 * 23400 * sps) / 1000, wl3 = (650 * 23400 * sps) / 1000;
	const size_t S = (size_t)n * kAcqPeaks;
	unsigned char *d;
	if ((r = acq_scratch(0, AcqScratch(nullptr, (size_t)n, kAcqPeaks).bytes, &d))) return r;
	const AcqScratch o(d, (size_t)n, kAcqPeaks);
	const float2 *spare;
	if ((r = acq_spare((size_t)wl3, st, &spare))) return r;

	AcqArgs g;
	std::memset(&g, 0, sizeof(g));
	g.n = n; g.sps = sps; g.flen = flen; g.wl3 = wl3;
	// (both are 8-byte aligned, so the difference is whole samples; windows are iq + offset in 64-bit arithmetic)
	g.spare = (uint64_t)((uintptr_t)spare - (uintptr_t)iq) / sizeof(float2);
	g.base = o.base; g.len = o.len; g.stat = o.stat; g.align = o.align; g.base_align = o.base_align; g.ferr = o.ferr;
	g.can3 = o.can3; g.toa1 = o.toa1; g.rv1 = o.rv1; g.ftoa = o.ftoa; g.fe = o.fe; g.peaks = o.peaks; g.count = o.count;
	g.ctoa = o.ctoa; g.cfe = o.cfe; g.off = o.off; g.fs = o.fs; g.live = o.live;
	AcqIo io;
	std::memset(&io, 0, sizeof(io));
	io.offset = offset; io.length = length; io.start = start;
	io.wl1 = wl1;
	io.snr = o.snr;
	io.out = out;
	HIP_TRY(launch_acq_begin(g, io, st));

	// What the reference does between two sweeps (k_acq_glue's steps) is done by the producing sweep's last thread
	// (AcqTail, fcch_acq.h) -- four launches fewer in a chain of small dependent ones; the profiling build keeps the
	// other form for the comparison (GMR1_HIP_ACQ_UNFUSED).
	static const bool unfused = profile_env("GMR1_HIP_ACQ_UNFUSED") != nullptr;
	auto tail = [&](int step, bool skip_dead) {
		AcqTail t;
		std::memset(&t, 0, sizeof(t));
		if (!unfused) {
			t.step = step;
			t.skip_dead = skip_dead ? g.live : nullptr;
			t.g = g;
		}
		return t;
	};
	// fcch_single_init (gmr1_rx.c:605-639): rough over 330 ms, then fine
	if ((r = fcch_rough_tail(st, tab, n, sps, wl1, iq, o.off, nullptr, o.toa1, o.rv1, tail(1, false)))) return r;
	if (unfused) HIP_TRY(launch_acq_glue(1, g, st));
	if ((r = fcch_fine_tail(st, tab, 0, n, sps, iq, o.off, nullptr, o.ftoa, o.fe, nullptr, tail(2, false)))) return r;
	if (unfused) HIP_TRY(launch_acq_glue(2, g, st));
	// fcch_multi_process (gmr1_rx.c:643-744); a carrier shorter than 650 ms can only fail here: where the host knows the
	// lengths the sweep runs over the others (where it does not, over everything: such a carrier's window is the spare one)
	std::vector<int> k3;
	for (int k = 0; k < n; k++)
		if (!h_length || h_length[k] >= (uint64_t)wl3)
			k3.push_back(k);
	const bool all3 = (int)k3.size() == n;
	if (!k3.empty()) {
		if (all3) {
			if ((r = fcch_rough_multi_tail(st, tab, n, sps, wl3, iq, o.off, o.fs, o.peaks, kAcqPeaks, o.count,
			                               tail(3, false)))) return r;
		} else {
			// mixed lengths: the long-enough carriers one by one at their own slots (rare; captures come in equal lengths)
			for (int k : k3)
				if ((r = gmr1_hip_fcch_rough_multi_batch_dev(st, tab, 1, sps, wl3, iq, o.off + k, o.fs + k,
				                                             o.peaks + (size_t)k * kAcqPeaks, kAcqPeaks, o.count + k))) return r;
		}
	}
	// (mixed lengths, or no carrier long enough: the step that lays out the candidate slots runs as its own launch)
	if (unfused || !all3) HIP_TRY(launch_acq_glue(3, g, st));
	if ((r = fcch_fine_tail(st, tab, 0, (int)S, sps, iq, o.off, o.fs, o.ctoa, o.cfe, nullptr, tail(4, true)))) return r;
	if (unfused) HIP_TRY(launch_acq_glue(4, g, st));
	if ((r = fcch_fine_tail(st, tab, 1, (int)S, sps, iq, o.off, o.fs, nullptr, nullptr, o.snr, tail(0, true)))) return r;
	HIP_TRY(launch_acq_decide(g, io, st));
	return 0;
}

}  // namespace gmr1

extern "C" {

int gmr1_hip_fcch_acquire_batch_dev(void *stream, int fcch_type, int n, int sps, const float *iq,
                                    const uint64_t *offset, const uint64_t *length, const int32_t *start,
                                    struct gmr1_hip_fcch_acq *out)
{
	int r = acq_check(fcch_type, n, sps, iq, offset, length, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0) return 0;
	// (the chain's scratch and the sweeps' workspace are this call's until its last launch)
	WsLease lease;
	if ((r = lease.acquire(s, (hipStream_t)stream))) return r;
	return fcch_acquire_enqueue((hipStream_t)stream, fcch_type, n, sps, iq, offset, length, start, nullptr, out);
}

int gmr1_hip_fcch_acquire_batch(int fcch_type, int n, int sps, const float *iq, uint64_t iq_len,
                                const uint64_t *offset, const uint64_t *length, const int32_t *start,
                                struct gmr1_hip_fcch_acq *out)
{
	int r = acq_check(fcch_type, n, sps, iq, offset, length, out);
	if (r) return r;
	for (int i = 0; i < n; i++) {
		if (length[i] > 0x7fffffffull || offset[i] > iq_len || length[i] > iq_len - offset[i])
			return fail(-EINVAL, "fcch_acquire: stream %d is longer than 2^31-1 samples or runs past the end of iq", i);
		if (start && start[i] < 0)
			return fail(-EINVAL, "fcch_acquire: start[%d] is negative", i);
	}
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0) return 0;
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const uint64_t *d_off = sg.in(offset, (size_t)n), *d_len = sg.in(length, (size_t)n);
	const int32_t *d_start = sg.in(start, (size_t)n);
	struct gmr1_hip_fcch_acq *d_out = sg.out(out, (size_t)n);
	if ((r = sg.err())) return r;
	{
		WsLease lease;
		if ((r = lease.acquire(s, nullptr))) return r;
		if ((r = fcch_acquire_enqueue(nullptr, fcch_type, n, sps, d_iq, d_off, d_len, d_start, length, d_out))) return r;
	}
	return sg.fetch();
}

int gmr1_hip_fcch_rough_multi_batch_dev(void *stream, int fcch_type, int n, int sps, int len,
                                        const float *iq, const uint64_t *offset, const float *freq_shift,
                                        int32_t *peaks_toa, int N, int32_t *count)
{
	return fcch_rough_multi_tail((hipStream_t)stream, fcch_type, n, sps, len, iq, offset, freq_shift, peaks_toa, N, count,
	                             no_tail());
}

int gmr1_hip_fcch_rough_multi_batch(int fcch_type, int n, int sps, int len,
                                    const float *iq, uint64_t iq_len, const uint64_t *offset,
                                    const float *freq_shift, int32_t *peaks_toa, int N, int32_t *count)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!iq || !offset || !peaks_toa || !count || N < 1 || N > 32)
		return fail(-EINVAL, "fcch_rough_multi: bad argument");
	if (len < ((650 * 23400 * sps) / 1000))
		return fail(-EINVAL, "fcch_rough_multi: needs at least 650 ms of signal");
	Staged st;
	r = st.stage(n, iq, iq_len, offset, freq_shift, (uint64_t)len);
	if (r) return r;
	int32_t *d_toa = st.sg.out(peaks_toa, (size_t)n * N);
	int32_t *d_cnt = st.sg.out(count, (size_t)n);
	if ((r = st.sg.err())) return r;
	HIP_TRY(hipMemset(d_toa, 0, (size_t)n * N * 4));
	r = gmr1_hip_fcch_rough_multi_batch_dev(nullptr, fcch_type, n, sps, len, st.iq, st.off, st.fs, d_toa, N, d_cnt);
	if (r) return r;
	return st.sg.fetch();
}

// ---- reference-compatible single calls (fcch.h:47-61) ---------------------------------------
int gmr1_fcch_rough(const struct gmr1_fcch_burst *burst_type,
                    struct osmo_cxvec *search_win_in, int sps, float freq_shift, int *toa)
{
	if (!burst_type || !search_win_in || !search_win_in->data || !toa)
		return fail(-EINVAL, "gmr1_fcch_rough: NULL argument");
	const int tab = fcch_tab_of(burst_type);
	if (tab < 0)
		return fail(-EINVAL, "gmr1_fcch_rough: unknown FCCH burst type");
	const uint64_t off = 0;
	int32_t t = 0, rv = 0;
	int r = gmr1_hip_fcch_rough_batch(tab, 1, sps, search_win_in->len,
	                                  reinterpret_cast<const float *>(search_win_in->data),
	                                  (uint64_t)search_win_in->len, &off, &freq_shift, &t, &rv);
	if (r) return r;
	if (rv) return rv;
	*toa = t;
	return 0;
}

int gmr1_fcch_rough_multi(const struct gmr1_fcch_burst *burst_type,
                          struct osmo_cxvec *search_win_in, int sps, float freq_shift, int *peaks_toa, int N)
{
	if (!burst_type || !search_win_in || !search_win_in->data || !peaks_toa)
		return fail(-EINVAL, "gmr1_fcch_rough_multi: NULL argument");
	const int tab = fcch_tab_of(burst_type);
	if (tab < 0)
		return fail(-EINVAL, "gmr1_fcch_rough_multi: unknown FCCH burst type");
	if (N < 1 || N > 32)
		return fail(-EINVAL, "gmr1_fcch_rough_multi: N must be 1..32");
	const uint64_t off = 0;
	int32_t cnt = 0;
	int32_t tmp[32] = {0};
	int r = gmr1_hip_fcch_rough_multi_batch(tab, 1, sps, search_win_in->len,
	                                        reinterpret_cast<const float *>(search_win_in->data),
	                                        (uint64_t)search_win_in->len, &off, &freq_shift, tmp, N, &cnt);
	if (r) return r;
	for (int i = 0; i < N && i < cnt; i++)
		peaks_toa[i] = tmp[i];
	return cnt;
}

int gmr1_fcch_fine(const struct gmr1_fcch_burst *burst_type,
                   struct osmo_cxvec *burst_in, int sps, float freq_shift, int *toa, float *freq_error)
{
	if (!burst_type || !burst_in || !burst_in->data || !toa || !freq_error)
		return fail(-EINVAL, "gmr1_fcch_fine: NULL argument");
	const int tab = fcch_tab_of(burst_type);
	if (tab < 0)
		return fail(-EINVAL, "gmr1_fcch_fine: unknown FCCH burst type");
	if (sps < 1 || burst_in->len / sps != burst_type->len)      // fcch.c:546-551
		return fail(-EINVAL, "gmr1_fcch_fine: burst must be len*sps samples");
	const uint64_t off = 0;
	int32_t t = 0;
	float fe = 0.f;
	int r = gmr1_hip_fcch_fine_batch(tab, 1, sps, reinterpret_cast<const float *>(burst_in->data),
	                                 (uint64_t)burst_in->len, &off, &freq_shift, &t, &fe);
	if (r) return r;
	*toa = t;
	*freq_error = fe;
	return 0;
}

int gmr1_fcch_snr(const struct gmr1_fcch_burst *burst_type,
                  struct osmo_cxvec *burst_in, int sps, float freq_shift, float *snr)
{
	if (!burst_type || !burst_in || !burst_in->data || !snr)
		return fail(-EINVAL, "gmr1_fcch_snr: NULL argument");
	const int tab = fcch_tab_of(burst_type);
	if (tab < 0)
		return fail(-EINVAL, "gmr1_fcch_snr: unknown FCCH burst type");
	if (sps < 1 || burst_in->len / sps != burst_type->len)      // fcch.c:671-675
		return fail(-EINVAL, "gmr1_fcch_snr: burst must be len*sps samples");
	const uint64_t off = 0;
	float v = 0.f;
	int r = gmr1_hip_fcch_snr_batch(tab, 1, sps, reinterpret_cast<const float *>(burst_in->data),
	                                (uint64_t)burst_in->len, &off, &freq_shift, &v);
	if (r) return r;
	*snr = v;
	return 0;
}

}  // extern "C"
