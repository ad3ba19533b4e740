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
// What a handle follows is its `kind`, and the kind's one description (RxStreamKind, rx_stream.h) is what the handle, the
// entries and the checks ask: how many carriers a push brings -- the handle holds one ping-pong pair per such carrier,
// plane[0] the BCCH carrier's, plane[1] the traffic carrier's, plane[2] the CSD carrier's, all with the first one's stride,
// held and keep (k_rx_stage_copy) -- and which follow-ups run behind the walk.
//
// A handle made by gmr1_hip_rx_stream_create_tch also follows TCH3 calls (gmr1_hip_rx_run_tch over pushes).  It holds one
// struct gmr1_hip_tch3_state per chain in device memory and, on the host, each chain's assigned timeslot.  A push walks the
// chains with the frame log on, then hands this push's frames to tch3_follow_chains (capi_rx_follow.cpp) -- the one-shot
// pass's own rule for frames, assignments and windows -- on those states: the call a push leaves is the call the next one
// continues.  The traffic windows of admitted frames fit the samples held for the same reason the walk's own do
// (DESIGN.md 4.4b).  The handle keeps chains, never walks: what a push found reaches the next one only through the device
// states and `carry`.
//
// A handle made by gmr1_hip_rx_stream_create_full follows TCH9 data calls as well (gmr1_hip_rx_run_full over pushes): the
// CSD carrier's samples, one struct gmr1_hip_tch9_state per chain in device memory and the timeslot of
// each chain's last ASSIGNMENT COMMAND 1 on the host (`carry9`).  tch3_follow_chains notes this push's commands, and
// tch9_follow_push (capi_rx_follow.cpp) follows them through the batched TCH9 call follower in one invocation.
//
// A handle made by gmr1_hip_rx_stream_create_voice is a tch handle that also decodes the calls it follows
// (gmr1_hip_rx_run_voice over pushes): one AMBE decoder state per chain in device memory beside d_tstate and each chain's
// count of assignments on the host (`n_assigned`), handed to tch3_follow_chains as an RxVoice; a push's audio blocks come
// back beside its records.  It brings two carriers a push, as a tch handle does.

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
	int kind = kRxStreamPlain;           // what it follows; everything that depends on it asks what()
	float2 *plane[kRxStreamMaxPlanes][2] = {};     // per carrier a push brings (what().planes of them): its ping-pong pair
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
	std::vector<uint8_t> kc;             // a handle that follows calls: A x 8 (empty: the all-zero key)
	// what().tch3: the TCH3 follow-up
	gmr1_hip_tch3_state *d_tstate = nullptr;       // one per chain, parallel to d_state
	std::vector<TchCarry> carry;         // per chain
	// what().tch9: the TCH9 follow-up
	gmr1_hip_tch9_state *d_t9state = nullptr;      // one per chain, parallel to d_state
	std::vector<Tch9CallCarry> carry9;   // per chain
	// what().audio: the decoders of the TCH3 calls
	void *d_codec = nullptr;             // one AMBE decoder state per chain, beside d_tstate
	std::vector<int> n_assigned;         // per chain: IMMEDIATE ASSIGNMENTs followed so far
	const RxStreamKind &what() const { return rx_stream_kind(kind); }
	~gmr1_hip_rx_stream()
	{
		for (float2 *(&pair)[2] : plane)
			for (float2 *p : pair)
				if (p) (void)hipFree(p);
		for (void *p : std::initializer_list<void *>{d_tstate, d_t9state, d_state, d_codec, d_car, d_err, d_in})
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

// the chains a push of n can walk, and the most samples one of them walks over
struct RxStreamReach {
	long long chains = 0, len = 0;
};

RxStreamReach rx_stream_reach(const gmr1_hip_rx_stream *h, uint64_t n)
{
	RxStreamReach r;
	for (int i = 0; i < h->A && !h->ended; i++) {
		if (rx_stream_dead(h, i))
			continue;
		r.chains += h->acquired ? h->c0[i + 1] - h->c0[i] : kMaxPeaks;
		r.len = std::max(r.len, rx_stream_next_held(h, i, n));
	}
	return r;
}

// the most records, big records and audio blocks a push of n can hand back
long long rx_stream_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	const RxStreamReach r = rx_stream_reach(h, n);
	return r.chains * (h->what().tch3 ? rx_stream_tch_rec_per_chain(r.len, h->sps) : rx_stream_rec_per_chain(r.len, h->sps));
}

long long rx_stream_big_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	const RxStreamReach r = rx_stream_reach(h, n);
	return h->what().tch9 ? rx_stream_max_big(r.chains, r.len, h->sps) : 0;
}

long long rx_stream_audio_bound(const gmr1_hip_rx_stream *h, uint64_t n)
{
	const RxStreamReach r = rx_stream_reach(h, n);
	return h->what().audio ? rx_stream_max_audio(r.chains, r.len, h->sps) : 0;
}

// what a push entry hands in: `kind` says which entry it is (_push*, _push_tch*, _push_full*, _push_voice*)
struct RxStreamPush {
	int kind = kRxStreamPlain;
	const float *chunk[kRxStreamMaxPlanes] = {};   // by plane: iq (rx_stream_push_any puts it there), tch, csd
	gmr1_hip_rx_big_record *big_out = nullptr;     // _push_full*
	int max_big = 0;
	int *n_big = nullptr;
	gmr1_hip_rx_audio *audio_out = nullptr;        // _push_voice*
	int max_audio = 0;
	int *n_audio = nullptr;
};

int rx_stream_check(const gmr1_hip_rx_stream *h, const RxStreamPush &p, uint64_t iq_stride, uint64_t n, const gmr1_hip_rx_record *out,
                    int max_records, const int *n_records)
{
	if (!h || !n_records || max_records < 0 || (max_records > 0 && !out) || (n > 0 && !p.chunk[0]))
		return fail(-EINVAL, "rx_stream_push: handle / n_records (and iq when n > 0, out when max_records > 0) are required");
	const RxStreamKind &k = h->what();
	if (h->kind != p.kind)
		return fail(-EINVAL, "rx_stream_push: a handle of %s takes %s, not %s", k.maker, k.entry, rx_stream_kind(p.kind).entry);
	static const char *const chunk_of[kRxStreamMaxPlanes] = {nullptr, "rx_stream_push_tch: tch", "rx_stream_push_full: csd"};
	for (int pl = 1; pl < k.planes; pl++)
		if (n > 0 && !p.chunk[pl])
			return fail(-EINVAL, "%s is required when n > 0", chunk_of[pl]);
	if (k.tch9 && (!p.n_big || p.max_big < 0 || (p.max_big > 0 && !p.big_out)))
		return fail(-EINVAL, "rx_stream_push_full: n_big (and big_out when max_big > 0) are required");
	if (k.audio && (!p.n_audio || p.max_audio < 0 || (p.max_audio > 0 && !p.audio_out)))
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
	if (k.tch9 && (long long)p.max_big < big_bound)
		return fail(-EINVAL, "rx_stream_push_full: max_big %d below the bound %lld", p.max_big, big_bound);
	const long long audio_bound = rx_stream_audio_bound(h, n);
	if (k.audio && (long long)p.max_audio < audio_bound)
		return fail(-EINVAL, "rx_stream_push_voice: max_audio %d below the bound %lld", p.max_audio, audio_bound);
	return 0;
}

// the destination of a staging of `need` samples per carrier in a ping-pong pair
int rx_stream_other(gmr1_hip_rx_stream *h, float2 *(&pair)[2], long long need, bool grow)
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

// staging: [kept tail | chunk] -> the other buffer of every plane, states rebased; the handle's host mirror moves with it
int rx_stream_stage(hipStream_t st, gmr1_hip_rx_stream *h, const float *const *chunk, uint64_t iq_stride, uint64_t n, int last)
{
	const int A = h->A, planes = h->what().planes;
	std::vector<long long> next((size_t)A);
	long long need = 0, max_pairs = 0;
	for (int i = 0; i < A; i++) {
		next[i] = rx_stream_next_held(h, i, n);
		need = std::max(need, next[i]);
	}
	need = (need + kRxKeepAlign - 1) / kRxKeepAlign * kRxKeepAlign;
	float2 *src[kRxStreamMaxPlanes] = {};
	const long long src_stride = h->stride;
	const bool grow = need > h->stride;         // (every pair follows the first one's decision)
	for (int pl = 0; pl < planes; pl++) {
		src[pl] = h->plane[pl][h->cur];
		const int r = rx_stream_other(h, h->plane[pl], need, grow);
		if (r) return r;
	}
	if (grow) h->stride = need;
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
	// (no destination: nothing is held and nothing came; the pairs are allocated together)
	for (int pl = 0; pl < planes; pl++) {
		float2 *dst = h->plane[pl][1 - h->cur];
		if (!dst) break;
		RxStageArgs sa;
		std::memset(&sa, 0, sizeof(sa));
		sa.n_carriers = A; sa.sps = h->sps; sa.last = last ? 1 : 0;
		sa.max_pairs = (int)std::min<long long>(max_pairs, 0x7fffffff);
		sa.src = src[pl] ? src[pl] : dst;
		sa.dst = dst;
		sa.iq = chunk[pl] ? reinterpret_cast<const float2 *>(chunk[pl]) : dst;
		sa.car = h->d_car;
		// the first plane's staging also rebases the states; the others only move samples
		sa.state = pl ? nullptr : h->d_state;
		sa.err = pl ? nullptr : h->d_err;
		HIP_TRY(pl ? launch_rx_stage_copy(sa, st) : launch_rx_stage(sa, st));
	}
	if (grow && std::any_of(src, src + planes, [](const float2 *s) { return s != nullptr; })) {
		HIP_TRY(hipStreamSynchronize(st));     // the staging has read the old buffers
		for (int pl = 0; pl < planes; pl++) {
			if (src[pl]) (void)hipFree(src[pl]);
			h->plane[pl][h->cur] = nullptr;
		}
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
		if (h->what().tch3) {
			t0 = tch3_first_states(h->chains, all_chains(nc), h->kc.empty() ? nullptr : h->kc.data());
			HIP_TRY(hipMalloc(&h->d_tstate, nc * sizeof(gmr1_hip_tch3_state)));
			HIP_TRY(hipMemcpyAsync(h->d_tstate, t0.data(), nc * sizeof(gmr1_hip_tch3_state), hipMemcpyHostToDevice, run.st));
			h->carry.assign(nc, TchCarry());
		}
		if (h->what().audio) {
			// no decoder is read before an assignment made it fresh; zeros until then
			const size_t bytes = nc * gmr1_hip_codec_state_bytes();
			HIP_TRY(hipMalloc(&h->d_codec, bytes));
			HIP_TRY(hipMemsetAsync(h->d_codec, 0, bytes, run.st));
			h->n_assigned.assign(nc, 0);
		}
		if (h->what().tch9) {
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
// and has validated everything (p.chunk: device memory, the traffic and the CSD carrier's chunks laid out as iq)
int rx_stream_push_impl(hipStream_t st, gmr1_hip_rx_stream *h, const RxStreamPush &p, uint64_t iq_stride, uint64_t n, int last,
                        gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	const int A = h->A, sps = h->sps;
	const RxStreamKind &k = h->what();
	int r;
	if ((r = rx_stream_stage(st, h, p.chunk, iq_stride, n, last))) return r;
	std::vector<uint64_t> offset((size_t)A), length((size_t)A);
	for (int i = 0; i < A; i++) {
		offset[i] = (uint64_t)((long long)i * h->stride);
		length[i] = (uint64_t)h->held[i];
	}
	// (a traffic carrier makes the walk log its frames and hand its records back chain by chain, as in gmr1_hip_rx_run_tch;
	// a plain handle has none: its plane[1] is null)
	const auto held = [&](int pl) { return reinterpret_cast<const float *>(h->plane[pl][h->cur]); };
	RxRun run(st, sps, held(0), held(1), nullptr, A, offset.data(), length.data(), h->arfcn.empty() ? nullptr : h->arfcn.data(), nullptr,
	          out, max_records);
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
	if (k.tch3 && walking) {
		RxVoice voice;
		if (k.audio) {
			voice.d_codec = h->d_codec;
			voice.count = h->n_assigned.data();
			voice.out = p.audio_out;
			voice.max_out = p.max_audio;
		}
		if ((r = tch3_follow_chains(st, sps, run.tch, run.arfcn, k.tch9, !last, h->chains, run.walks, all_chains(h->chains.size()), nullptr,
		                            h->d_tstate, h->carry.data(), k.audio ? &voice : nullptr))) return r;
		if (k.audio) *p.n_audio = voice.found;
		*n_records = rx_hand_back(run.walks, out, max_records);
		// the TCH9 follow-up over the same frames, from the commands the TCH3 records of this push carry
		if (k.tch9 && (r = tch9_follow_push(st, sps, held(2), run.arfcn, !last, h->chains, run.walks, h->d_t9state, h->carry9.data(),
		                                    p.big_out, p.max_big, p.n_big))) return r;
	}
	rx_stream_keep(h);
	return 0;
}

// the host form's chunks go up packed (stride n) through the handle's pinned block, plane after plane, *each bytes apart
// (rx_stream_check has passed: p is of the handle's kind and holds a chunk for every plane when n > 0)
int rx_stream_pin_chunk(gmr1_hip_rx_stream *h, const RxStreamPush &p, uint64_t iq_stride, uint64_t n, size_t *each)
{
	const int planes = h->what().planes;
	*each = (size_t)h->A * (size_t)n * sizeof(float2);
	const size_t bytes = (size_t)planes * *each;
	if (bytes > h->h_in_bytes) {
		if (h->h_in) (void)hipHostFree(h->h_in);
		if (h->d_in) (void)hipFree(h->d_in);
		h->h_in = nullptr; h->d_in = nullptr; h->h_in_bytes = h->d_in_bytes = 0;
		HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_in), bytes, hipHostMallocDefault));
		h->h_in_bytes = bytes;
		HIP_TRY(hipMalloc(&h->d_in, bytes));
		h->d_in_bytes = bytes;
	}
	for (int pl = 0; pl < planes; pl++)
		for (int i = 0; i < h->A && n > 0; i++)
			std::memcpy(h->h_in + pl * (*each / 4) + (size_t)i * n * 2, p.chunk[pl] + (size_t)i * iq_stride * 2, (size_t)n * sizeof(float2));
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
	p.chunk[0] = iq;
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	if ((r = rx_stream_check(h, p, iq_stride, n, out, max_records, n_records)))
		return r;
	hipStream_t st = host ? nullptr : (hipStream_t)stream;
	size_t each = 0;
	if (host && (r = rx_stream_pin_chunk(h, p, iq_stride, n, &each))) return r;
	// the loop holds the device's workspace, side stream and events: pushes of other handles wait their turn
	WsLease lease;
	if ((r = lease.acquire(ds, st))) return r;
	if (host) {
		const int planes = h->what().planes;
		if (each)
			HIP_TRY(hipMemcpyAsync(h->d_in, h->h_in, (size_t)planes * each, hipMemcpyHostToDevice, st));
		for (int pl = 0; pl < planes; pl++)
			p.chunk[pl] = h->d_in + pl * (each / 4);
		iq_stride = n;
	}
	r = rx_stream_push_impl(st, h, p, iq_stride, n, last, out, max_records, n_records);
	if (r) h->broken = true;
	return r;
}

// the three gmr1_hip_rx_stream_max_* entries: `what` is the entry's output ("max_big"), `unit` what it counts.  (_max_records
// asks for the device before it looks at its arguments, the other two after: each entry's order is kept.)
int rx_stream_max_any(const char *what, const char *unit, bool device_first, const gmr1_hip_rx_stream *h, uint64_t n,
                      long long (*bound)(const gmr1_hip_rx_stream *, uint64_t), int *out)
{
	DevState *ds;
	int r;
	if (device_first && (r = dev_state(&ds))) return r;
	if (!h || !out)
		return fail(-EINVAL, "rx_stream_%s: handle / %s are required", what, what);
	if (!device_first && (r = dev_state(&ds))) return r;
	std::lock_guard<std::mutex> lk(h->mu);
	const long long b = bound(h, n);
	if (b > 0x7fffffffll)
		return fail(-EINVAL, "rx_stream_%s: %lld %s do not fit an int", what, b, unit);
	*out = (int)b;
	return 0;
}

// the four create entries.  kind: what the handle follows; kc: n_arfcn x 8 key bytes for a handle that follows calls, or
// NULL for the all-zero key.  (The plain entry asks for the device before it looks at its arguments, the others after.)
int rx_stream_create(int kind, int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	const RxStreamKind &k = rx_stream_kind(kind);
	const char *who = k.maker + sizeof("gmr1_hip_") - 1;
	const bool device_first = kind == kRxStreamPlain;
	DevState *ds;
	int r;
	if (device_first && (r = dev_state(&ds))) return r;
	if (!out)
		return fail(-EINVAL, "%s: h is required", who);
	*out = nullptr;
	if (n_arfcn < 1 || n_arfcn > 65535)
		return fail(-EINVAL, "%s: n_arfcn=%d (1..65535)", who, n_arfcn);
	if (sps < 1 || sps > 16)                  // gmr1_rx.c:919-922
		return fail(-EINVAL, "%s: sps=%d unsupported (1..16)", who, sps);
	// the NT9 window of 351 sps + sps + sps / 2 samples has to fit the demodulator's (gmr1_hip_rx_run_full finds out at
	// its first NT9 frame)
	if (k.tch9 && rx_tch9_in_len(sps) > kMaxInLen)
		return fail(-EINVAL, "%s: sps=%d: the NT9 window of %d samples is above %d (sps 1..%d)", who, sps, rx_tch9_in_len(sps), kMaxInLen,
		            rx_stream_full_max_sps());
	if (!device_first && (r = dev_state(&ds))) return r;
	if (k.audio && (r = tch3_pcm_prepare())) return r;       // the decoder's tables, built once per device
	std::unique_ptr<gmr1_hip_rx_stream> h(new gmr1_hip_rx_stream);
	HIP_TRY(hipGetDevice(&h->device));
	h->A = n_arfcn;
	h->sps = sps;
	h->kind = kind;
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
	return rx_stream_create(kRxStreamPlain, n_arfcn, sps, arfcn, nullptr, out);
}

int gmr1_hip_rx_stream_create_tch(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	return rx_stream_create(kRxStreamTch, n_arfcn, sps, arfcn, kc, out);
}

int gmr1_hip_rx_stream_create_full(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	return rx_stream_create(kRxStreamFull, n_arfcn, sps, arfcn, kc, out);
}

int gmr1_hip_rx_stream_create_voice(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	return rx_stream_create(kRxStreamVoice, n_arfcn, sps, arfcn, kc, out);
}

int gmr1_hip_rx_stream_max_records(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_records)
{
	return rx_stream_max_any("max_records", "records", true, h, n, rx_stream_bound, max_records);
}

int gmr1_hip_rx_stream_max_big(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_big)
{
	return rx_stream_max_any("max_big", "records", false, h, n, rx_stream_big_bound, max_big);
}

int gmr1_hip_rx_stream_max_audio(const struct gmr1_hip_rx_stream *h, uint64_t n, int *max_audio)
{
	return rx_stream_max_any("max_audio", "blocks", false, h, n, rx_stream_audio_bound, max_audio);
}

int gmr1_hip_rx_stream_push_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n,
                                int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_any(stream, h, RxStreamPush(), false, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push(struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n, int last,
                            struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_any(nullptr, h, RxStreamPush(), true, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_tch_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                    uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records,
                                    int *n_records)
{
	const RxStreamPush p = {.kind = kRxStreamTch, .chunk = {nullptr, tch}};
	return rx_stream_push_any(stream, h, p, false, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_tch(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                                int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	const RxStreamPush p = {.kind = kRxStreamTch, .chunk = {nullptr, tch}};
	return rx_stream_push_any(nullptr, h, p, true, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_full_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, const float *csd,
                                     uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records,
                                     int *n_records, struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big)
{
	const int r = rx_stream_full_args(h, max_records, n_records, max_big, n_big);
	if (r) return r;
	const RxStreamPush p = {.kind = kRxStreamFull, .chunk = {nullptr, tch, csd}, .big_out = big_out, .max_big = max_big, .n_big = n_big};
	return rx_stream_push_any(stream, h, p, false, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_full(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, const float *csd, uint64_t iq_stride,
                                 uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                 struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big)
{
	const int r = rx_stream_full_args(h, max_records, n_records, max_big, n_big);
	if (r) return r;
	const RxStreamPush p = {.kind = kRxStreamFull, .chunk = {nullptr, tch, csd}, .big_out = big_out, .max_big = max_big, .n_big = n_big};
	return rx_stream_push_any(nullptr, h, p, true, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_voice_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride,
                                      uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                      struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	const RxStreamPush p = {.kind = kRxStreamVoice, .chunk = {nullptr, tch}, .audio_out = audio_out, .max_audio = max_audio, .n_audio = n_audio};
	return rx_stream_push_any(stream, h, p, false, iq, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_voice(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                                  int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                                  struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	const RxStreamPush p = {.kind = kRxStreamVoice, .chunk = {nullptr, tch}, .audio_out = audio_out, .max_audio = max_audio, .n_audio = n_audio};
	return rx_stream_push_any(nullptr, h, p, true, iq, iq_stride, n, last, out, max_records, n_records);
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
