// capi_common.h -- helpers shared by the C-ABI translation units (host only).
#pragma once

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include <hip/hip_runtime.h>

#include "gmr1_dev.h"
#include "host_tables.h"
#include "rx4_operands.h"
#include "scratch_layouts.h"

namespace gmr1 {

int fail(int code, const char *fmt, ...);
const char *last_error();
// -EINVAL if one of n windows of in_len samples, window i at offset[i], does not lie within the iq_len samples of iq
int bursts_fit(int n, const uint64_t *offset, int in_len, uint64_t iq_len);
// 1 when the layer-1 chains follow libosmocore's accelerated Viterbi decoder (gmr1_hip_set_conv_decoder), else 0
int conv_acc();

#define HIP_TRY(expr)                                                                  \
	do {                                                                               \
		hipError_t e_ = (expr);                                                        \
		if (e_ != hipSuccess)                                                          \
			return ::gmr1::fail(e_ == hipErrorNoDevice ? -ENODEV : -EIO, "%s: %s", #expr, \
			                    hipGetErrorString(e_));                                \
	} while (0)

// a vector to a new device buffer, as it lies (blocking): what the per-device caches' makers upload with (dev_cache.h).
// Frees the buffer if the copy fails; *dst is null after any failure.
template <typename T, typename D> static int upload(D **dst, const std::vector<T> &v)
{
	static_assert(sizeof(T) == sizeof(D), "uploaded as it lies");
	*dst = nullptr;
	HIP_TRY(hipMalloc(dst, v.size() * sizeof(T)));
	const hipError_t e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		(void)hipFree(*dst);
		*dst = nullptr;
		return fail(e == hipErrorNoDevice ? -ENODEV : -EIO, "upload: hipMemcpy: %s", hipGetErrorString(e));
	}
	return 0;
}

struct DevState {
	bool ready = false;       // constant tables uploaded to this device
	void *ws = nullptr;       // grow-only scratch for kernels that need workspace
	size_t ws_bytes = 0;
	// users of the workspace (and of the receive loop's side stream and events) take turns: WsLease
	std::recursive_mutex ws_mu;
	hipEvent_t ws_ev = nullptr;   // recorded behind the last user's kernels
	int ws_depth = 0;
};

// One user of the device's shared workspace at a time, from any thread on any stream.  The host part of a call runs under
// the device's lock (a second thread waits its turn); the device part is ordered by an event: a call on another stream
// first makes ITS stream wait for the kernels of the previous user, so nobody's scratch is overwritten or freed under
// running kernels.  Re-entrant (a workspace user may call another one on the same stream: the receive loop calls the
// FCCH sweeps).  Calls that need no workspace (every burst-level _batch_dev entry in its usual shape) take no lease.
class WsLease {
public:
	WsLease() = default;
	WsLease(const WsLease &) = delete;
	WsLease &operator=(const WsLease &) = delete;
	~WsLease();
	int acquire(DevState *s, hipStream_t st);

private:
	DevState *s_ = nullptr;
	hipStream_t st_ = nullptr;
};

extern DevBurst g_host_types[kNumTypes];
extern Rx4Ord4 g_host_ord4;      // the fused batch kernel's packed view of the BCCH / DC6 descriptors, made with them (rx4_operands.h)
// guards the descriptor-table slots caller-defined burst types are uploaded into (one demodulator slot, four detector
// slots): held from the upload until the kernel that reads them has finished
std::mutex &custom_slots_mutex();
int host_types();
// state of the CURRENT device; uploads the constant tables on first use
int dev_state(DevState **out);
// grow-only device scratch of the current device; the caller holds a WsLease from here to its last launch
int dev_workspace(DevState *s, size_t bytes, void **out);

// What every burst of the fused BCCH / DC6 path shares (window lengths, strides, staging size, decoder), written into `a`,
// which the caller has zeroed and given its pointers (capi_rx_fused.cpp).  -EINVAL below min_sps samples per symbol, or
// if the burst tables are not what the fused kernels are built for.
int rx_fused_base_args(int sps, RxArgs *a, int min_sps = 4);
// The fused BCCH / CCCH receive of a.n bursts (capi_rx_fused.cpp).  `a`: zeroed, then n, sps, plane_stride, iq and the
// per-burst pointers (offset, kind, l2, crc, conv, rv required; energy: the optional burst_energy() output); the rest is
// filled in here.
int rx_fused_launch(hipStream_t stream, RxArgs a);

// process_bcch of n_chains chains in one launch (capi_rx_fused.cpp / launch_rx_loop); every pointer in `la` is device memory
int rx_loop_dev_impl(hipStream_t stream, int n_chains, int sps, const float *iq, const RxLoopArgs &la);

// gmr1_hip_rx_run_dev that also reports how many records each carrier contributed (capi_rx.cpp; the sharded entry keeps
// the records on the device and still needs the per-carrier counts)
int rx_run_dev_counted(void *stream, int n_arfcn, int sps, const float *iq, const uint64_t *offset, const uint64_t *length,
                       const uint16_t *arfcn, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                       int32_t *status, int32_t *n_chains, int32_t *rec_per_carrier);

// TCH9 bursts of several interleaver runs of unequal length in one launch (capi_nt9.cpp)
int tch9_runs_dev_impl(hipStream_t st, int mode, int n, const int32_t *seq_pos, const int8_t *ebits, const uint8_t *ciph,
                       uint8_t *l2, int32_t *conv);

// what an NT9 decoder launch of one kind (0..2 TCH9 mode, 3 FACCH9) shares, into a zeroed `a` (capi_nt9.cpp)
int nt9_kind_args(int kind, Nt9Args *a);

// gmr1_hip_demod_batch_dev of a built-in burst type, plus burst_energy() of each window (capi_demod.cpp)
int demod_dev_energy(hipStream_t st, int burst_id, int n, int sps, int in_len, const float *iq,
                     const uint64_t *offset, const float *freq_shift, int8_t *ebits, int ebits_stride,
                     int32_t *sync_id, float *toa, float *energy, int32_t *rv);

// One demodulation launch of n bursts of one format (capi_demod.cpp): `type` is the descriptor-table slot `ht` is uploaded
// in.  demod_dev_impl: device pointers.  demod_host_impl: host pointers staged through HBM, blocking; `custom` is a
// caller-defined description to upload into its slot first (NULL for a built-in type).
int demod_dev_impl(hipStream_t st, int type, const DevBurst &ht,
                   int n, int sps, int in_len, const float *iq, const uint64_t *offset,
                   const float *freq_shift, int8_t *ebits, int ebits_stride, int32_t *sync_id,
                   float *toa, float *freq_err, float *ssyms, int32_t *rv, float *energy = nullptr);
int demod_host_impl(int type, const DevBurst &ht, const DevBurst *custom,
                    int n, int sps, int in_len, const float *iq, uint64_t iq_len,
                    const uint64_t *offset, const float *freq_shift,
                    int8_t *ebits, int ebits_stride, int32_t *sync_id,
                    float *toa, float *freq_err, float *ssyms, int32_t *rv);
// the profiling switch GMR1_HIP_DBG_STOP (RxArgs::dbg_stop; 0 in the product build), read once (capi_demod.cpp)
int dbg_stop_env();

// One encode of n units of chain `id` (enc_plan.h's PlanId) through k_encode (capi_encode.cpp): what a chain does not take
// stays null.  encode_dev: device pointers, enqueued on `st`.  encode_host: host pointers staged through HBM, blocking.
struct EncIo { const uint8_t *in0, *in1, *aux0, *aux1, *ciph; uint8_t *ebits; };
#pragma GCC visibility push(hidden)
int encode_dev(hipStream_t st, int id, int n, int seq_len, const EncIo &io, const char *what);
int encode_host(int id, int n, int seq_len, const EncIo &io, const char *what);
// the chain of a gmr1_tch9_mode, -1 for none (capi_encode.cpp)
int tch9_plan(int mode);
#pragma GCC visibility pop

// BCCH / CCCH batch decode, chain = kChainBcch / kChainCcch (capi_l1.cpp): device pointers; host pointers, blocking
int l1_dev(hipStream_t st, int chain, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv);
int l1_host(int chain, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv);

// gmr1_hip_tch3_follow_batch_dev on scratch of the caller's (capi_tch3_follow.cpp): tch3_follow_scratch_bytes(n_frames)
// (scratch_layouts.h) of device memory on a 128-byte boundary.  The arguments are not checked; the caller holds a WsLease.
int tch3_follow_enqueue(hipStream_t st, void *scratch, int n_calls, int sps, int in_len, const float *iq, const int32_t *first,
                        int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                        struct gmr1_hip_tch3_state *state, struct gmr1_hip_tch3_frame *out);

// The speech decoder over the TCH3 follower's records (capi_ambe.cpp), shared by gmr1_hip_tch3_frames_to_pcm* and
// gmr1_hip_tch3_voice_batch*.  _check: counts, required pointers (codec_state only where state_required), flag bits outside
// flags_known, alignment -- needs no device.  _first_check: first[] is a partition of 0..n_frames (host memory; every
// follower's host form asks it under its own name).  _prepare: the decoder's tables are on the current device (the first
// use uploads and builds them).  _fresh: gmr1_hip_codec_init_dev.
// _enqueue: one launch on `st`, device pointers, arguments not checked.
int tch3_pcm_check(const char *who, int n_calls, const int32_t *first, int n_frames, const void *frames, const void *codec_state,
                   bool state_required, int flags, int flags_known, const void *pcm);
int tch3_pcm_first_check(const char *who, int n_calls, const int32_t *first, int n_frames);
int tch3_pcm_prepare();
int tch3_pcm_fresh(hipStream_t st, int n_calls, void *codec_state, int flags);
int tch3_pcm_enqueue(hipStream_t st, int n_calls, const int32_t *first, int n_frames, const struct gmr1_hip_tch3_frame *frames,
                     void *codec_state, int16_t *pcm, int32_t *rv);

// The follower's records closed up into audio blocks (capi_ambe.cpp; the rule: tch3_audio.h): what
// gmr1_hip_tch3_frames_to_audio_dev runs, on scratch of the caller's -- tch3_audio_scratch_bytes (scratch_layouts.h) of
// device memory on a 128-byte boundary -- with the arguments not checked.  call_base (optional, device, n_calls entries): the blocks in front
// of each call.  codec_init_list: gmr1_hip_codec_init_list_dev.
int tch3_audio_enqueue(hipStream_t st, void *scratch, int n_calls, const int32_t *first, int n_frames,
                       const struct gmr1_hip_tch3_frame *frames, const uint32_t *fn, const uint64_t *label, void *codec_state,
                       struct gmr1_hip_rx_audio *out, int max_out, int32_t *call_base, int32_t *n_out);
int codec_init_list(hipStream_t st, int n, const int32_t *call, void *state, int flags);

// gmr1_hip_tch9_follow_batch_dev on scratch of the caller's (capi_tch9_follow.cpp), under the same terms
int tch9_follow_enqueue(hipStream_t st, void *scratch, int n_calls, int sps, int in_len, int mode, const float *iq, const int32_t *first,
                        int n_frames, const uint64_t *offset, const float *freq_shift, const uint32_t *fn,
                        struct gmr1_hip_tch9_state *state, struct gmr1_hip_tch9_frame *out);

// Device scratch of a traffic pass: one carve-up of the grow-only device workspace (none of the kernels the
// passes launch uses it) instead of dozens of hipMalloc / hipFree pairs per call.  No byte count is summed for it: a pass
// is written once and run twice (sized_by) -- on the arena measuring, when it has no memory, take() only adds up and a
// Stage on it copies nothing; then on memory of the size that took.
struct Arena {
	unsigned char *base = nullptr;
	size_t cap = 0, off = 0;
	bool measures = false;
	template <class F> int sized_by(F &&pass)
	{
		base = nullptr; cap = ~(size_t)0; off = 0; measures = true;
		pass(*this);
		const int r = init(off);
		return r ? r : pass(*this);
	}
	int init(size_t bytes)
	{
		DevState *ds;
		int r = dev_state(&ds);
		if (r) return r;
		void *ws;
		r = dev_workspace(ds, bytes + 256, &ws);
		if (r) return r;
		base = reinterpret_cast<unsigned char *>(up128((uintptr_t)ws));
		cap = bytes;
		off = 0;
		measures = false;
		return 0;
	}
	void *take(size_t n)
	{
		n = up128(n ? n : 1);
		if (off + n > cap)
			return nullptr;
		void *p = measures ? static_cast<void *>(this) : base + off;      // (measuring: a pointer nobody follows)
		off += n;
		return p;
	}
};

// The device copies of one call's host buffers.  Counts are elements of T, so a buffer's size is written once.
// in() and out() turn a null host pointer into a null device pointer and allocate nothing.  The first HIP error is
// kept and everything after it does nothing: the caller asks err() once before it launches and returns what fetch()
// returns, both with HIP_TRY's codes.  Plain: hipMalloc and blocking copies, freed on scope exit.  On an Arena:
// memory from it and hipMemcpyAsync on the stream.
class Stage {
public:
	explicit Stage(hipStream_t st = nullptr, Arena *arena = nullptr) : st_(st), arena_(arena) {}
	Stage(const Stage &) = delete;
	Stage &operator=(const Stage &) = delete;
	~Stage() { for (void *p : owned_) (void)hipFree(p); }

	// n elements that only the device sees
	template <typename T> T *dev(size_t n) { return static_cast<T *>(take(n * sizeof(T))); }
	// uploaded
	template <typename T> const T *in(const T *h, size_t n)
	{
		T *d = h || measures() ? dev<T>(n) : nullptr;
		if (d) copy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
		return d;
	}
	// copied back by fetch()
	template <typename T> T *out(T *h, size_t n) { return h || measures() ? out_always(h, n) : nullptr; }
	// an output the kernel writes whether the caller wants it or not: copied back by fetch() if h is not null
	template <typename T> T *out_always(T *h, size_t n)
	{
		T *d = dev<T>(n);
		back(h, d, n);
		return d;
	}
	// uploaded, and copied back by fetch()
	template <typename T> T *inout(T *h, size_t n)
	{
		T *d = const_cast<T *>(in(h, n));
		back(h, d, n);
		return d;
	}
	// fetch() copies the n elements at d, which lie in a buffer of this stage, to h (nothing if h is null)
	template <typename T> void back(T *h, const T *d, size_t n) { if (h && d && !measures()) backs_.push_back({h, d, n * sizeof(T)}); }
	// on a measuring Arena: every buffer is charged for, a null or empty host side too, and nothing is copied or booked
	bool measures() const { return arena_ && arena_->measures; }

	int err() const
	{
		return e_ == hipSuccess ? 0 : fail(e_ == hipErrorNoDevice ? -ENODEV : -EIO, "%s: %s", what_, hipGetErrorString(e_));
	}
	// on an Arena: queues the copies back booked so far and does not wait; a later fetch() waits for them
	void queue_backs()
	{
		for (const Back &b : backs_)
			copy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
		backs_.clear();
	}
	// one synchronisation of the stream, ahead of the blocking copies back and behind the queued ones
	int fetch()
	{
		if (!arena_) note("hipStreamSynchronize", hipStreamSynchronize(st_));
		queue_backs();
		if (arena_ && e_ == hipSuccess) note("hipStreamSynchronize", hipStreamSynchronize(st_));
		return err();
	}

private:
	struct Back { void *h; const void *d; size_t bytes; };
	void note(const char *what, hipError_t e) { if (e_ == hipSuccess && e != hipSuccess) { e_ = e; what_ = what; } }
	void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
	{
		if (e_ != hipSuccess || measures()) return;
		if (arena_) note("hipMemcpyAsync", hipMemcpyAsync(dst, src, bytes, kind, st_));
		else note("hipMemcpy", hipMemcpy(dst, src, bytes, kind));
	}
	void *take(size_t bytes)
	{
		void *p = nullptr;
		if (e_ != hipSuccess) return p;
		if (arena_) {
			p = arena_->take(bytes);
			note("the traffic pass's arena", p ? hipSuccess : hipErrorOutOfMemory);
		} else {
			note("hipMalloc", hipMalloc(&p, bytes ? bytes : 1));
			if (p) owned_.push_back(p);
		}
		return p;
	}
	hipStream_t st_;
	Arena *arena_;
	hipError_t e_ = hipSuccess;
	const char *what_ = "";
	std::vector<void *> owned_;
	std::vector<Back> backs_;
};

// The output of a host form that writes n windows of in_len samples into the caller's array (the shaping calls, the FCCH
// chirps): check() refuses a window that leaves out_len and windows that overlap; stage() gives the device copy of the
// windows' hull and the offsets relative to it, and books one copy back per run of windows that touch -- so what lies
// between the windows in the caller's array stays.
struct HostWindows {
	std::vector<uint64_t> order;       // the offsets, sorted
	int check(const char *who, int n, int in_len, const uint64_t *offset, uint64_t out_len);
	float *stage(Stage &sg, int in_len, const uint64_t *offset, float *out, const uint64_t **d_offset);     // n > 0
private:
	std::vector<uint64_t> rel_;
};

// One turn on the device's workspace: leases it for `st`, hands enqueue(scratch) `bytes` of it, gives the lease back on return
template <class F> int with_scratch(DevState *s, hipStream_t st, size_t bytes, F &&enqueue)
{
	WsLease lease;
	int r = lease.acquire(s, st);
	if (r) return r;
	Arena ws;
	if ((r = ws.init(bytes))) return r;
	return enqueue(static_cast<void *>(ws.base));
}

// The device copies of what a call follower's host form is handed: the samples and the per-frame arrays (the bits form has
// neither samples nor windows: null, nothing staged), the calls' states in and out, the records out.
template <class State, class Frame> struct FollowStaged {
	const float *iq; const int32_t *first; const uint64_t *off; const float *fs; const uint32_t *fn;
	State *state; Frame *out;
};
template <class State, class Frame>
FollowStaged<State, Frame> stage_follow(Stage &sg, int n_calls, const float *iq, uint64_t iq_len, const int32_t *first, int n_frames,
                                        const uint64_t *off, const float *fs, const uint32_t *fn, State *state, Frame *out)
{
	const size_t n = (size_t)n_frames;
	return {sg.in(iq, (size_t)iq_len * 2), sg.in(first, (size_t)n_calls + 1), sg.in(off, n), sg.in(fs, n), sg.in(fn, n),
	        sg.inout(state, (size_t)n_calls), sg.out(out, n)};
}

}  // namespace gmr1
