// capi_rx_stream.cpp -- the streaming receive loop (gmr1_hip_rx_stream_*): gmr1_hip_rx_run over a capture pushed piece
// by piece.
//
// A handle holds, per carrier, the samples it still needs in one buffer of a device ping-pong pair, and every chain's
// RxLoopState in device memory.  A push stages [kept tail | new chunk] into the other buffer (k_rx_stage, which also
// rebases the states), runs the acquisition once enough samples are there (rx_stream_acq_need), then walks every chain
// with the one-shot loop (RxRun::frame_loop, capi_rx.cpp) up to the samples available.  A walk only ever processes a frame after
// rx_loop_advance's check `align + 2 * frame_len <= len` admitted it, and every window of such a frame ends before
// align + 2 * frame_len, so a walk to H samples does exactly what the one-shot walk does up to there; the only thing the
// horizon adds is a stop that the next push may lift (rx_stream_next_done).  A carrier then keeps its samples from
// rx_stream_keep_from(min chain align): no window of the next walk starts before that (rx_stream_reach_back).
//
// A handle made by gmr1_hip_rx_stream_create_tch also follows TCH3 calls (gmr1_hip_rx_run_tch over pushes).  It holds the
// traffic carrier's samples in a second ping-pong pair with the first one's stride, held and keep (k_rx_stage_copy), one
// struct gmr1_hip_tch3_state per chain in device memory and, on the host, each chain's assigned timeslot.  A push walks the
// chains with the frame log on, then hands this push's frames to tch3_follow_chains (capi_rx_follow.cpp) -- the one-shot
// pass's own rule for frames, assignments and windows -- on those states: the call a push leaves is the call the next one
// continues.  The traffic windows of admitted frames fit the samples held for the same reason the walk's own do
// (DESIGN.md 4.4b).  The handle keeps chains, never walks: what a push found reaches the next one only through the device
// states and `carry`.
//
// A handle made by gmr1_hip_rx_stream_create_full follows TCH9 data calls as well (gmr1_hip_rx_run_full over pushes): a
// third ping-pong pair for the CSD carrier, one struct gmr1_hip_tch9_state per chain in device memory and the timeslot of
// each chain's last ASSIGNMENT COMMAND 1 on the host (`carry9`).  tch3_follow_chains notes this push's commands, and
// tch9_follow_push (capi_rx_follow.cpp) follows them through the batched TCH9 call follower in one invocation.
//
// A handle made by gmr1_hip_rx_stream_create_voice is a tch handle that also decodes the calls it follows
// (gmr1_hip_rx_run_voice over pushes): one AMBE decoder state per chain in device memory beside d_tstate and each chain's
// count of assignments on the host (`n_assigned`), handed to tch3_follow_chains as an RxVoice; a push's audio blocks come
// back beside its records.  It brings two carriers a push, as a tch handle does: rx_stream_planes (rx_stream.h).

#include "fcch_acq.h"
#include "rx_run.h"

#include <memory>
#include <numeric>

using namespace gmr1;

static_assert(kRxStartDiscard == kAcqStart, "one start discard");      // gmr1_rx.c:52

struct gmr1_hip_rx_stream {
	mutable std::mutex mu;               // one push at a time
	int device = -1;
	int A = 0, sps = 0;
	std::vector<uint16_t> arfcn;         // empty: records carry the carrier index
	uint64_t N = 0;                      // samples pushed per carrier so far
	bool acquired = false, ended = false, broken = false;
	std::vector<int32_t> stat, nch;
	std::vector<int32_t> acq_stat;       // per carrier: status the acquisition left (the loop may set stat to -EIO later)
	std::vector<long long> held;         // per carrier: samples in the current buffer
	std::vector<long long> keep;         // per carrier: first of them the next push keeps (held: none)
	std::vector<int> rebased;            // per carrier: 1 once samples were dropped
	std::vector<RxChain> chains;         // host mirror of the chains (carrier by carrier, chain by chain)
	std::vector<int> c0;                 // per carrier: its first chain (A + 1 entries, all 0 until the acquisition)
	float2 *buf[2] = {nullptr, nullptr};
	int cur = 0;
	long long stride = 0;                // samples per carrier in each buffer (a multiple of kRxKeepAlign)
	RxLoopState *d_state = nullptr;
	RxStageCarrier *d_car = nullptr;
	int32_t *d_err = nullptr;
	RxStageCarrier *h_car = nullptr;     // pinned: the staging parameters go up from here
	int32_t *h_err = nullptr;
	float *h_in = nullptr;               // pinned: gmr1_hip_rx_stream_push's host chunk (grow-only)
	size_t h_in_bytes = 0;
	float *d_in = nullptr;
	size_t d_in_bytes = 0;
	// a handle that follows TCH3 calls (gmr1_hip_rx_stream_create_tch)
	bool tch = false;
	std::vector<uint8_t> kc;             // A x 8 (empty: the all-zero key)
	float2 *tbuf[2] = {nullptr, nullptr};          // the traffic carrier's samples: buf's layout, stride, held and keep
	gmr1_hip_tch3_state *d_tstate = nullptr;       // one per chain, parallel to d_state
	std::vector<TchCarry> carry;         // per chain
	// a handle that follows TCH9 calls too (gmr1_hip_rx_stream_create_full; tch is set as well)
	bool full = false;
	float2 *cbuf[2] = {nullptr, nullptr};          // the CSD carrier's samples, held as tbuf is
	gmr1_hip_tch9_state *d_t9state = nullptr;      // one per chain, parallel to d_state
	std::vector<Tch9CallCarry> carry9;   // per chain
	// a handle that decodes the TCH3 calls it follows (gmr1_hip_rx_stream_create_voice; tch is set as well)
	bool voice = false;
	void *d_codec = nullptr;             // one AMBE decoder state per chain, beside d_tstate
	std::vector<int> n_assigned;         // per chain: IMMEDIATE ASSIGNMENTs followed so far
	int kind() const { return full ? kRxStreamFull : voice ? kRxStreamVoice : tch ? kRxStreamTch : kRxStreamPlain; }
	~gmr1_hip_rx_stream()
	{
		for (void *p : std::initializer_list<void *>{buf[0], buf[1], tbuf[0], tbuf[1], cbuf[0], cbuf[1], d_tstate, d_t9state, d_state,
		                                             d_codec, d_car, d_err, d_in})
			if (p) (void)hipFree(p);
		for (void *p : std::initializer_list<void *>{h_car, h_err, h_in})
			if (p) (void)hipHostFree(p);
	}
};

namespace {

// a carrier keeps nothing once its acquisition failed, or when none of its chains is left to walk (none found, or every
// one outgrew the loop's buffers; as in the one-shot call, the others of a carrier go on when one does)
bool rx_stream_dead(const gmr1_hip_rx_stream *h, int i)
{
	if (!h->acquired)
		return false;
	if (h->acq_stat[i] != 0)
		return true;
	for (int k = h->c0[i]; k < h->c0[i + 1]; k++)
		if (!h->chains[k].outgrew)
			return false;
	return true;
}

// samples carrier i holds after a push of n
long long rx_stream_next_held(const gmr1_hip_rx_stream *h, int i, uint64_t n)
{
	if (rx_stream_dead(h, i))
		return 0;
	return h->held[i] - h->keep[i] + (long long)n;
}

long long rx_stream_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	if (h->ended)
		return 0;
	long long chains = 0, len = 0;
	for (int i = 0; i < h->A; i++) {
		if (rx_stream_dead(h, i))
			continue;
		chains += h->acquired ? h->c0[i + 1] - h->c0[i] : kMaxPeaks;
		len = std::max(len, rx_stream_next_held(h, i, n));
	}
	if (!chains)
		return 0;
	return chains * (h->tch ? rx_stream_tch_rec_per_chain(len, h->sps) : rx_stream_rec_per_chain(len, h->sps));
}

long long rx_stream_big_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	if (h->ended || !h->full)
		return 0;
	long long chains = 0, len = 0;
	for (int i = 0; i < h->A; i++) {
		if (rx_stream_dead(h, i))
			continue;
		chains += h->acquired ? h->c0[i + 1] - h->c0[i] : kMaxPeaks;
		len = std::max(len, rx_stream_next_held(h, i, n));
	}
	return rx_stream_max_big(chains, len, h->sps);
}

long long rx_stream_audio_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	if (h->ended || !h->voice)
		return 0;
	long long chains = 0, len = 0;
	for (int i = 0; i < h->A; i++) {
		if (rx_stream_dead(h, i))
			continue;
		chains += h->acquired ? h->c0[i + 1] - h->c0[i] : kMaxPeaks;
		len = std::max(len, rx_stream_next_held(h, i, n));
	}
	return rx_stream_max_audio(chains, len, h->sps);
}

// what a push entry hands in beside iq: `kind` says which entry it is (_push*, _push_tch*, _push_full*, _push_voice*)
struct RxStreamPush {
	int kind;
	const float *tch, *csd;
	gmr1_hip_rx_big_record *big_out;
	int max_big;
	int *n_big;
	gmr1_hip_rx_audio *audio_out = nullptr;
	int max_audio = 0;
	int *n_audio = nullptr;
};

int rx_stream_check(const gmr1_hip_rx_stream *h, const RxStreamPush &p, const float *iq, uint64_t iq_stride, uint64_t n,
                    const gmr1_hip_rx_record *out, int max_records, const int *n_records)
{
	if (!h || !n_records || max_records < 0 || (max_records > 0 && !out) || (n > 0 && !iq))
		return fail(-EINVAL, "rx_stream_push: handle / n_records (and iq when n > 0, out when max_records > 0) are required");
	if (h->kind() != p.kind) {
		static const char *const entry[kRxStreamKinds] = {"gmr1_hip_rx_stream_push*", "gmr1_hip_rx_stream_push_tch*",
		                                                  "gmr1_hip_rx_stream_push_full*", "gmr1_hip_rx_stream_push_voice*"};
		static const char *const maker[kRxStreamKinds] = {"gmr1_hip_rx_stream_create", "gmr1_hip_rx_stream_create_tch",
		                                                  "gmr1_hip_rx_stream_create_full", "gmr1_hip_rx_stream_create_voice"};
		return fail(-EINVAL, "rx_stream_push: a handle of %s takes %s, not %s", maker[h->kind()], entry[h->kind()], entry[p.kind]);
	}
	if (p.kind != kRxStreamPlain && n > 0 && !p.tch)
		return fail(-EINVAL, "rx_stream_push_tch: tch is required when n > 0");
	if (p.kind == kRxStreamFull) {
		if (n > 0 && !p.csd)
			return fail(-EINVAL, "rx_stream_push_full: csd is required when n > 0");
		if (!p.n_big || p.max_big < 0 || (p.max_big > 0 && !p.big_out))
			return fail(-EINVAL, "rx_stream_push_full: n_big (and big_out when max_big > 0) are required");
	}
	if (p.kind == kRxStreamVoice && (!p.n_audio || p.max_audio < 0 || (p.max_audio > 0 && !p.audio_out)))
		return fail(-EINVAL, "rx_stream_push_voice: n_audio (and audio_out when max_audio > 0) are required");
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	if (dev != h->device)
		return fail(-EINVAL, "rx_stream_push: the handle belongs to device %d, the current device is %d", h->device, dev);
	if (h->broken)
		return fail(-EIO, "rx_stream_push: the handle failed in an earlier push");
	if (h->ended)
		return fail(-EINVAL, "rx_stream_push: the last push has been made");
	if (h->A > 1 && n > 0 && iq_stride < n)
		return fail(-EINVAL, "rx_stream_push: iq_stride %llu < n %llu", (unsigned long long)iq_stride, (unsigned long long)n);
	if (n > 0x7fffffffull)
		return fail(-EINVAL, "rx_stream_push: n above 2^31-1");
	for (int i = 0; i < h->A; i++)
		if (rx_stream_next_held(h, i, n) > 0x7fffffffll)
			return fail(-EINVAL, "rx_stream_push: carrier %d would hold more than 2^31-1 samples", i);
	const long long bound = rx_stream_bound(h, n);
	if ((long long)max_records < bound)
		return fail(-EINVAL, "rx_stream_push: max_records %d below the bound %lld", max_records, bound);
	const long long big_bound = rx_stream_big_bound(h, n);
	if (p.kind == kRxStreamFull && (long long)p.max_big < big_bound)
		return fail(-EINVAL, "rx_stream_push_full: max_big %d below the bound %lld", p.max_big, big_bound);
	const long long audio_bound = rx_stream_audio_bound(h, n);
	if (p.kind == kRxStreamVoice && (long long)p.max_audio < audio_bound)
		return fail(-EINVAL, "rx_stream_push_voice: max_audio %d below the bound %lld", p.max_audio, audio_bound);
	return 0;
}

// the destination of a staging of `need` samples per carrier in a ping-pong pair
int rx_stream_other(gmr1_hip_rx_stream *h, float2 **pair, long long need, bool grow)
{
	float2 *&o = pair[1 - h->cur];
	if (grow) {
		// grow-only: a new pair; the old current buffer is the source of this one staging and then goes
		float2 *fresh = nullptr;
		HIP_TRY(hipMalloc(&fresh, (size_t)h->A * (size_t)need * sizeof(float2)));
		if (o) (void)hipFree(o);
		o = fresh;
	} else if (!o && need > 0) {
		HIP_TRY(hipMalloc(&o, (size_t)h->A * (size_t)h->stride * sizeof(float2)));
	}
	return 0;
}

// staging: [kept tail | chunk] -> the other buffer, states rebased; the handle's host mirror moves with it
int rx_stream_stage(hipStream_t st, gmr1_hip_rx_stream *h, const float2 *iq, const float2 *tch, const float2 *csd, uint64_t iq_stride,
                    uint64_t n, int last)
{
	const int A = h->A;
	std::vector<long long> next((size_t)A);
	long long need = 0, max_pairs = 0;
	for (int i = 0; i < A; i++) {
		next[i] = rx_stream_next_held(h, i, n);
		need = std::max(need, next[i]);
	}
	need = (need + kRxKeepAlign - 1) / kRxKeepAlign * kRxKeepAlign;
	float2 *src = h->buf[h->cur], *tsrc = h->tbuf[h->cur], *csrc = h->cbuf[h->cur];
	const long long src_stride = h->stride;
	const bool grow = need > h->stride;
	int r = rx_stream_other(h, h->buf, need, grow);
	if (!r && h->tch) r = rx_stream_other(h, h->tbuf, need, grow);   // (the traffic pair follows the first one's decision)
	if (!r && h->full) r = rx_stream_other(h, h->cbuf, need, grow);  // (and so does the CSD pair)
	if (r) return r;
	if (grow) h->stride = need;
	float2 *dst = h->buf[1 - h->cur], *tdst = h->tbuf[1 - h->cur], *cdst = h->cbuf[1 - h->cur];
	for (int i = 0; i < A; i++) {
		RxStageCarrier &c = h->h_car[i];
		const bool dead = rx_stream_dead(h, i);
		c.src = (uint64_t)((long long)i * src_stride + h->keep[i]);
		c.dst = (uint64_t)((long long)i * h->stride);
		c.iq = (long long)i * (long long)iq_stride;
		c.kept = dead ? 0 : (int32_t)(h->held[i] - h->keep[i]);
		c.n_new = dead ? 0 : (int32_t)n;
		c.shift = dead ? 0 : (int32_t)h->keep[i];
		c.c0 = h->c0[i];
		c.c1 = h->c0[i + 1];
		if (c.shift > 0) h->rebased[i] = 1;
		c.rebased = h->rebased[i];
		max_pairs = std::max(max_pairs, ((long long)c.kept + c.n_new + 1) / 2);
	}
	*h->h_err = 0;
	HIP_TRY(hipMemcpyAsync(h->d_car, h->h_car, (size_t)A * sizeof(RxStageCarrier), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(h->d_err, h->h_err, 4, hipMemcpyHostToDevice, st));
	if (dst) {
		RxStageArgs sa;
		std::memset(&sa, 0, sizeof(sa));
		sa.n_carriers = A; sa.sps = h->sps; sa.last = last ? 1 : 0;
		sa.max_pairs = (int)std::min<long long>(max_pairs, 0x7fffffff);
		sa.src = src ? src : dst;
		sa.dst = dst;
		sa.iq = iq ? iq : dst;
		sa.car = h->d_car;
		sa.state = h->d_state;
		sa.err = h->d_err;
		HIP_TRY(launch_rx_stage(sa, st));
		if (tdst) {
			sa.src = tsrc ? tsrc : tdst;
			sa.dst = tdst;
			sa.iq = tch ? tch : tdst;
			sa.state = nullptr;
			sa.err = nullptr;
			HIP_TRY(launch_rx_stage_copy(sa, st));
		}
		if (cdst) {
			sa.src = csrc ? csrc : cdst;
			sa.dst = cdst;
			sa.iq = csd ? csd : cdst;
			sa.state = nullptr;
			sa.err = nullptr;
			HIP_TRY(launch_rx_stage_copy(sa, st));
		}
	}
	if (grow && (src || tsrc || csrc)) {
		HIP_TRY(hipStreamSynchronize(st));     // the staging has read the old buffers
		if (src) (void)hipFree(src);
		if (tsrc) (void)hipFree(tsrc);
		if (csrc) (void)hipFree(csrc);
		h->buf[h->cur] = nullptr;
		h->tbuf[h->cur] = nullptr;
		h->cbuf[h->cur] = nullptr;
	}
	h->cur = 1 - h->cur;
	for (int i = 0; i < A; i++) {
		if (!rx_stream_dead(h, i))
			for (int k = h->c0[i]; k < h->c0[i + 1]; k++)
				h->chains[k].align -= (int)h->keep[i];
		h->held[i] = next[i];
		h->keep[i] = 0;
	}
	h->N += n;
	if (last) h->ended = true;
	return 0;
}

std::vector<int> all_chains(size_t n)
{
	std::vector<int> calls(n);
	std::iota(calls.begin(), calls.end(), 0);
	return calls;
}

// the acquisition, once (nothing has been dropped yet: coordinates are absolute): the handle's chains and their states on the
// device.  t0 and t9, the calls' first states, live until the push's synchronisation.
int rx_stream_acquire(gmr1_hip_rx_stream *h, RxRun &run, int last, std::vector<gmr1_hip_tch3_state> &t0,
                      std::vector<gmr1_hip_tch9_state> &t9)
{
	int r = run.acquire();
	if (r) return r;
	h->stat = run.stat; h->nch = run.nch;
	h->acq_stat = run.stat;
	h->chains = std::move(run.chains);
	run.chains.clear();
	h->c0.assign((size_t)h->A + 1, 0);
	for (const RxChain &c : h->chains)
		h->c0[c.a + 1]++;
	for (int i = 0; i < h->A; i++)
		h->c0[i + 1] += h->c0[i];
	const size_t nc = h->chains.size();
	if (nc) {
		HIP_TRY(hipMalloc(&h->d_state, nc * sizeof(RxLoopState)));
		std::vector<RxLoopState> s0;
		for (const RxChain &c : h->chains)
			s0.push_back(rx_first_state(c, rx_label(run.arfcn, c.a), rx_stream_next_done(kRxDoneUnstarted, c.align, c.len, h->sps, last)));
		HIP_TRY(hipMemcpyAsync(h->d_state, s0.data(), nc * sizeof(RxLoopState), hipMemcpyHostToDevice, run.st));
		if (h->tch) {
			t0 = tch3_first_states(h->chains, all_chains(nc), h->kc.empty() ? nullptr : h->kc.data());
			HIP_TRY(hipMalloc(&h->d_tstate, nc * sizeof(gmr1_hip_tch3_state)));
			HIP_TRY(hipMemcpyAsync(h->d_tstate, t0.data(), nc * sizeof(gmr1_hip_tch3_state), hipMemcpyHostToDevice, run.st));
			h->carry.assign(nc, TchCarry());
		}
		if (h->voice) {
			// no decoder is read before an assignment made it fresh; zeros until then
			const size_t bytes = nc * gmr1_hip_codec_state_bytes();
			HIP_TRY(hipMalloc(&h->d_codec, bytes));
			HIP_TRY(hipMemsetAsync(h->d_codec, 0, bytes, run.st));
			h->n_assigned.assign(nc, 0);
		}
		if (h->full) {
			// no call, nothing held, the carrier's key (rx_tch9_init keeps the key)
			t9.resize(nc);
			std::memset(t9.data(), 0, nc * sizeof(gmr1_hip_tch9_state));
			for (size_t k = 0; k < nc && !h->kc.empty(); k++)
				std::memcpy(t9[k].kc, h->kc.data() + (size_t)h->chains[k].a * 8, 8);
			HIP_TRY(hipMalloc(&h->d_t9state, nc * sizeof(gmr1_hip_tch9_state)));
			HIP_TRY(hipMemcpyAsync(h->d_t9state, t9.data(), nc * sizeof(gmr1_hip_tch9_state), hipMemcpyHostToDevice, run.st));
			h->carry9.assign(nc, Tch9CallCarry());
		}
	}
	h->acquired = true;
	return 0;
}

// the walk up to the samples available: the handle's chains through the run and back, the walks stay with the run
int rx_stream_walk(gmr1_hip_rx_stream *h, RxRun &run)
{
	run.chains = std::move(h->chains);
	for (RxChain &c : run.chains) {
		c.base = run.offset[c.a];
		c.len = (int)h->held[c.a];
	}
	run.loop_state = h->d_state;
	const int r = run.frame_loop();
	h->chains = std::move(run.chains);
	if (r) return r;
	h->stat = run.stat;
	for (size_t k = 0; k < h->chains.size(); k++)
		if (h->chains[k].outgrew) {
			// stopped for good, as in the one-shot call
			static const int32_t fin = kRxDoneFinal;
			HIP_TRY(hipMemcpyAsync(&h->d_state[k].done, &fin, 4, hipMemcpyHostToDevice, run.st));
		}
	return 0;
}

// what each carrier keeps for the next push
void rx_stream_keep(gmr1_hip_rx_stream *h)
{
	for (int i = 0; i < h->A; i++) {
		if (h->ended || rx_stream_dead(h, i)) {
			h->keep[i] = h->held[i];
			continue;
		}
		if (!h->acquired) {
			h->keep[i] = 0;
			continue;
		}
		long long lo = h->held[i];
		for (int k = h->c0[i]; k < h->c0[i + 1]; k++)
			if (!h->chains[k].outgrew)
				lo = std::min<long long>(lo, h->chains[k].align);
		h->keep[i] = std::min(h->held[i], rx_stream_keep_from(lo, h->sps));
	}
}

// the device part of a push -- stage, acquire (once), walk, follow, keep; the caller holds h->mu and the workspace lease,
// and has validated everything (p.tch, p.csd: the traffic and the CSD carrier's chunks, laid out as iq, for a handle that
// follows calls on them)
int rx_stream_push_impl(hipStream_t st, gmr1_hip_rx_stream *h, const float2 *iq, const RxStreamPush &p, uint64_t iq_stride, uint64_t n,
                        int last, gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	const int A = h->A, sps = h->sps;
	int r;
	if ((r = rx_stream_stage(st, h, iq, reinterpret_cast<const float2 *>(p.tch), reinterpret_cast<const float2 *>(p.csd), iq_stride, n,
	                         last))) return r;
	std::vector<uint64_t> offset((size_t)A), length((size_t)A);
	for (int i = 0; i < A; i++) {
		offset[i] = (uint64_t)((long long)i * h->stride);
		length[i] = (uint64_t)h->held[i];
	}
	// (a traffic carrier makes the walk log its frames and hand its records back chain by chain, as in gmr1_hip_rx_run_tch)
	RxRun run(st, sps, reinterpret_cast<const float *>(h->buf[h->cur]), h->tch ? reinterpret_cast<const float *>(h->tbuf[h->cur]) : nullptr,
	          nullptr, A, offset.data(), length.data(), h->arfcn.empty() ? nullptr : h->arfcn.data(), nullptr, out, max_records);
	run.stat = h->stat; run.nch = h->nch;
	std::vector<gmr1_hip_tch3_state> t0;
	std::vector<gmr1_hip_tch9_state> t9;
	// the acquisition, once every carrier holds what it reads
	if (!h->acquired && ((long long)h->N >= rx_stream_acq_need(sps) || last) && (r = rx_stream_acquire(h, run, last, t0, t9))) return r;
	const bool walking = h->acquired && !h->chains.empty();
	if (walking && (r = rx_stream_walk(h, run))) return r;
	HIP_TRY(hipMemcpyAsync(h->h_err, h->d_err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (*h->h_err) {
		h->broken = true;
		return fail(-EIO, "rx_stream_push: a chain could reach before its carrier's kept samples");
	}
	*n_records = run.direct ? run.direct_total : 0;
	// the TCH3 follow-up over this push's frames, and the records chain by chain in frame order
	if (h->tch && walking) {
		RxVoice voice;
		if (h->voice) {
			voice.d_codec = h->d_codec;
			voice.count = h->n_assigned.data();
			voice.out = p.audio_out;
			voice.max_out = p.max_audio;
		}
		if ((r = tch3_follow_chains(st, sps, run.tch, run.arfcn, h->full, !last, h->chains, run.walks, all_chains(h->chains.size()), nullptr,
		                            h->d_tstate, h->carry.data(), h->voice ? &voice : nullptr))) return r;
		if (h->voice) *p.n_audio = voice.found;
		*n_records = rx_hand_back(run.walks, out, max_records);
		// the TCH9 follow-up over the same frames, from the commands the TCH3 records of this push carry
		if (h->full && (r = tch9_follow_push(st, sps, reinterpret_cast<const float *>(h->cbuf[h->cur]), run.arfcn, !last, h->chains,
		                                     run.walks, h->d_t9state, h->carry9.data(), p.big_out, p.max_big, p.n_big))) return r;
	}
	rx_stream_keep(h);
	return 0;
}

// the host form's chunk goes up packed (stride n) through the handle's pinned block, the traffic carrier's *half bytes
// behind, the CSD carrier's as many behind that
int rx_stream_pin_chunk(gmr1_hip_rx_stream *h, const RxStreamPush &p, const float *iq, uint64_t iq_stride, uint64_t n, size_t *half)
{
	*half = (size_t)h->A * (size_t)n * sizeof(float2);
	const size_t bytes = (size_t)rx_stream_planes(p.kind) * *half;
	if (bytes > h->h_in_bytes) {
		if (h->h_in) (void)hipHostFree(h->h_in);
		if (h->d_in) (void)hipFree(h->d_in);
		h->h_in = nullptr; h->d_in = nullptr; h->h_in_bytes = h->d_in_bytes = 0;
		HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_in), bytes, hipHostMallocDefault));
		h->h_in_bytes = bytes;
		HIP_TRY(hipMalloc(&h->d_in, bytes));
		h->d_in_bytes = bytes;
	}
	for (int i = 0; i < h->A && n > 0; i++) {
		std::memcpy(h->h_in + (size_t)i * n * 2, iq + (size_t)i * iq_stride * 2, (size_t)n * sizeof(float2));
		if (p.kind != kRxStreamPlain)
			std::memcpy(h->h_in + *half / 4 + (size_t)i * n * 2, p.tch + (size_t)i * iq_stride * 2, (size_t)n * sizeof(float2));
		if (p.kind == kRxStreamFull)
			std::memcpy(h->h_in + 2 * (*half / 4) + (size_t)i * n * 2, p.csd + (size_t)i * iq_stride * 2, (size_t)n * sizeof(float2));
	}
	return 0;
}

// what needs neither the handle's contents nor the device to be refused
int rx_stream_full_args(const gmr1_hip_rx_stream *h, int max_records, int *n_records, int max_big, int *n_big)
{
	if (n_records) *n_records = 0;
	if (n_big) *n_big = 0;
	if (!h || !n_records || !n_big || max_records < 0 || max_big < 0)
		return fail(-EINVAL, "rx_stream_push_full: handle / n_records / n_big are required, and no negative count");
	return 0;
}

// every push entry: p says which one, host is for the forms that take host memory (on the null stream)
int rx_stream_push_any(void *stream, gmr1_hip_rx_stream *h, RxStreamPush p, bool host, const float *iq,
                       uint64_t iq_stride, uint64_t n, int last, gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_records) *n_records = 0;
	if (p.n_big) *p.n_big = 0;
	if (p.n_audio) *p.n_audio = 0;
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	if ((r = rx_stream_check(h, p, iq, iq_stride, n, out, max_records, n_records)))
		return r;
	hipStream_t st = host ? nullptr : (hipStream_t)stream;
	size_t half = 0;
	if (host && (r = rx_stream_pin_chunk(h, p, iq, iq_stride, n, &half))) return r;
	// the loop holds the device's workspace, side stream and events: pushes of other handles wait their turn
	WsLease lease;
	if ((r = lease.acquire(ds, st))) return r;
	if (host) {
		if (half)
			HIP_TRY(hipMemcpyAsync(h->d_in, h->h_in, (size_t)rx_stream_planes(p.kind) * half, hipMemcpyHostToDevice, st));
		iq = h->d_in;
		p.tch = p.kind != kRxStreamPlain ? h->d_in + half / 4 : nullptr;
		p.csd = p.kind == kRxStreamFull ? h->d_in + 2 * (half / 4) : nullptr;
		iq_stride = n;
	}
	r = rx_stream_push_impl(st, h, reinterpret_cast<const float2 *>(iq), p, iq_stride, n, last, out, max_records, n_records);
	if (r) h->broken = true;
	return r;
}

int rx_stream_create_check(const char *who, int n_arfcn, int sps, struct gmr1_hip_rx_stream **out)
{
	if (!out)
		return fail(-EINVAL, "%s: h is required", who);
	*out = nullptr;
	if (n_arfcn < 1 || n_arfcn > 65535)
		return fail(-EINVAL, "%s: n_arfcn=%d (1..65535)", who, n_arfcn);
	if (sps < 1 || sps > 16)                  // gmr1_rx.c:919-922
		return fail(-EINVAL, "%s: sps=%d unsupported (1..16)", who, sps);
	return 0;
}

// kind: what the handle follows; kc: n_arfcn x 8 key bytes for a handle that follows calls, or NULL for the all-zero key
int rx_stream_make(int n_arfcn, int sps, const uint16_t *arfcn, int kind, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	std::unique_ptr<gmr1_hip_rx_stream> h(new gmr1_hip_rx_stream);
	HIP_TRY(hipGetDevice(&h->device));
	h->A = n_arfcn;
	h->sps = sps;
	h->tch = kind != kRxStreamPlain;
	h->full = kind == kRxStreamFull;
	h->voice = kind == kRxStreamVoice;
	if (arfcn)
		h->arfcn.assign(arfcn, arfcn + n_arfcn);
	if (kc)
		h->kc.assign(kc, kc + (size_t)n_arfcn * 8);
	h->stat.assign(n_arfcn, 0);
	h->nch.assign(n_arfcn, 0);
	h->held.assign(n_arfcn, 0);
	h->keep.assign(n_arfcn, 0);
	h->rebased.assign(n_arfcn, 0);
	h->c0.assign((size_t)n_arfcn + 1, 0);
	HIP_TRY(hipMalloc(&h->d_car, (size_t)n_arfcn * sizeof(RxStageCarrier)));
	HIP_TRY(hipMalloc(&h->d_err, 4));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_car), (size_t)n_arfcn * sizeof(RxStageCarrier), hipHostMallocDefault));
	HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_err), 4, hipHostMallocDefault));
	*out = h.release();
	return 0;
}

}  // namespace

extern "C" {

int gmr1_hip_rx_stream_create(int n_arfcn, int sps, const uint16_t *arfcn, struct gmr1_hip_rx_stream **out)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if ((r = rx_stream_create_check("rx_stream_create", n_arfcn, sps, out))) return r;
	return rx_stream_make(n_arfcn, sps, arfcn, kRxStreamPlain, nullptr, out);
}

int gmr1_hip_rx_stream_create_tch(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	int r = rx_stream_create_check("rx_stream_create_tch", n_arfcn, sps, out);
	if (r) return r;
	DevState *ds;
	if ((r = dev_state(&ds))) return r;
	return rx_stream_make(n_arfcn, sps, arfcn, kRxStreamTch, kc, out);
}

int gmr1_hip_rx_stream_create_full(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	int r = rx_stream_create_check("rx_stream_create_full", n_arfcn, sps, out);
	if (r) return r;
	// the NT9 window of 351 sps + sps + sps / 2 samples has to fit the demodulator's (gmr1_hip_rx_run_full finds out at
	// its first NT9 frame)
	if (rx_tch9_in_len(sps) > kMaxInLen)
		return fail(-EINVAL, "rx_stream_create_full: sps=%d: the NT9 window of %d samples is above %d (sps 1..%d)", sps,
		            rx_tch9_in_len(sps), kMaxInLen, rx_stream_full_max_sps());
	DevState *ds;
	if ((r = dev_state(&ds))) return r;
	return rx_stream_make(n_arfcn, sps, arfcn, kRxStreamFull, kc, out);
}

int gmr1_hip_rx_stream_create_voice(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	int r = rx_stream_create_check("rx_stream_create_voice", n_arfcn, sps, out);
	if (r) return r;
	DevState *ds;
	if ((r = dev_state(&ds))) return r;
	if ((r = tch3_pcm_prepare())) return r;       // the decoder's tables, built once per device
	return rx_stream_make(n_arfcn, sps, arfcn, kRxStreamVoice, kc, out);
}

int gmr1_hip_rx_stream_max_audio(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_audio)
{
	if (!h || !max_audio)
		return fail(-EINVAL, "rx_stream_max_audio: handle / max_audio are required");
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	std::lock_guard<std::mutex> lk(h->mu);
	const long long b = rx_stream_audio_bound(h, n);
	if (b > 0x7fffffffll)
		return fail(-EINVAL, "rx_stream_max_audio: %lld blocks do not fit an int", b);
	*max_audio = (int)b;
	return 0;
}

int gmr1_hip_rx_stream_push_voice_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride,
                                      uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                      struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	return rx_stream_push_any(stream, h, {kRxStreamVoice, tch, nullptr, nullptr, 0, nullptr, audio_out, max_audio, n_audio}, false, iq,
	                          iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_voice(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                                  int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                  struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	return rx_stream_push_any(nullptr, h, {kRxStreamVoice, tch, nullptr, nullptr, 0, nullptr, audio_out, max_audio, n_audio}, true, iq,
	                          iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_max_big(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_big)
{
	if (!h || !max_big)
		return fail(-EINVAL, "rx_stream_max_big: handle / max_big are required");
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	std::lock_guard<std::mutex> lk(h->mu);
	const long long b = rx_stream_big_bound(h, n);
	if (b > 0x7fffffffll)
		return fail(-EINVAL, "rx_stream_max_big: %lld records do not fit an int", b);
	*max_big = (int)b;
	return 0;
}

int gmr1_hip_rx_stream_max_records(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_records)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (!h || !max_records)
		return fail(-EINVAL, "rx_stream_max_records: handle / max_records are required");
	std::lock_guard<std::mutex> lk(h->mu);
	const long long b = rx_stream_bound(h, n);
	if (b > 0x7fffffffll)
		return fail(-EINVAL, "rx_stream_max_records: %lld records do not fit an int", b);
	*max_records = (int)b;
	return 0;
}

int gmr1_hip_rx_stream_push_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n,
                                int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_any(stream, h, {kRxStreamPlain, nullptr, nullptr, nullptr, 0, nullptr}, false, iq, iq_stride, n, last, out,
	                          max_records, n_records);
}

int gmr1_hip_rx_stream_push(struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n, int last,
                            struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_any(nullptr, h, {kRxStreamPlain, nullptr, nullptr, nullptr, 0, nullptr}, true, iq, iq_stride, n, last, out,
	                          max_records, n_records);
}

int gmr1_hip_rx_stream_push_tch_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                    uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records,
                                    int *n_records)
{
	return rx_stream_push_any(stream, h, {kRxStreamTch, tch, nullptr, nullptr, 0, nullptr}, false, iq, iq_stride, n, last, out, max_records,
	                          n_records);
}

int gmr1_hip_rx_stream_push_tch(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                                int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_any(nullptr, h, {kRxStreamTch, tch, nullptr, nullptr, 0, nullptr}, true, iq, iq_stride, n, last, out, max_records,
	                          n_records);
}

int gmr1_hip_rx_stream_push_full_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, const float *csd,
                                     uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records,
                                     int *n_records, struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big)
{
	const int r = rx_stream_full_args(h, max_records, n_records, max_big, n_big);
	if (r) return r;
	return rx_stream_push_any(stream, h, {kRxStreamFull, tch, csd, big_out, max_big, n_big}, false, iq, iq_stride, n, last, out,
	                          max_records, n_records);
}

int gmr1_hip_rx_stream_push_full(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, const float *csd, uint64_t iq_stride,
                                 uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                 struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big)
{
	const int r = rx_stream_full_args(h, max_records, n_records, max_big, n_big);
	if (r) return r;
	return rx_stream_push_any(nullptr, h, {kRxStreamFull, tch, csd, big_out, max_big, n_big}, true, iq, iq_stride, n, last, out,
	                          max_records, n_records);
}

int gmr1_hip_rx_stream_status(const struct gmr1_hip_rx_stream *h, int32_t *status, int32_t *n_chains, uint64_t *retained)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (!h)
		return fail(-EINVAL, "rx_stream_status: handle is required");
	std::lock_guard<std::mutex> lk(h->mu);
	for (int i = 0; i < h->A; i++) {
		if (status) status[i] = h->stat[i];
		if (n_chains) n_chains[i] = h->nch[i];
		if (retained) retained[i] = (uint64_t)(h->held[i] - h->keep[i]);
	}
	return 0;
}

int gmr1_hip_rx_stream_destroy(struct gmr1_hip_rx_stream *h)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (!h)
		return 0;
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	const int own = h->device;
	if (dev != own)
		HIP_TRY(hipSetDevice(own));          // its memory is freed on its own device
	{
		std::lock_guard<std::mutex> lk(h->mu);    // a push in progress on another thread finishes first (pushes are synchronous)
	}
	delete h;
	if (dev != own)
		HIP_TRY(hipSetDevice(dev));
	return 0;
}

}  // extern "C"
