// capi_rx.cpp -- the receive control loop of the reference's gmr1_rx application
// (reference src/gmr1_rx.c:605-895, main() :897-975) over MANY BCCH carriers at once.
//
// The reference walks one carrier frame by frame on the CPU: one FCCH acquisition, then per
// 40 ms frame one BCCH or CCCH burst through demod + decode, feeding time / frequency / TDMA
// position back into the next frame.  That feedback only crosses a BCCH frame (rx_bcch is the
// only writer of align / freq_err / fn / sa_*), so between two BCCH frames of one chain every
// burst is independent, and different chains / carriers are independent throughout.  The frame
// loop therefore runs in ROUNDS -- a chain's CCCH bursts up to and including its next BCCH burst,
// then the BCCH feedback -- and it runs them ON THE GPU: k_rx_chain (rx_kernels.hip) walks every
// chain's feedback path from the first frame to the end of the capture and lists its CCCH bursts, one
// k_rx4 batch takes those, k_rx_merge writes the records (the integer control logic is in rx_loop.h);
// the host only collects them.  FCCH acquisition is one chain of batched sweeps
// (rough / fine / rough_multi / fine + snr) over all carriers with its decisions taken on the device (capi_fcch.cpp).  The arithmetic of every step runs on the
// GPU; the host keeps only the per-chain integers the reference keeps in struct chan_desc.
// There is no CPU fallback.
//
// The traffic channels never feed back into that loop, so their follow-ups run after it as batched passes of their own
// (capi_rx_follow.cpp).  The same phases over a capture pushed piece by piece: capi_rx_stream.cpp.  GSMTAP transport and
// per-burst stderr logging are out of scope; what GSMTAP would have carried comes back as records
// (capi_gsmtap.cpp packs them).

#include "fcch_acq.h"
#include "rx_run.h"

#include <cmath>

using namespace gmr1;

namespace {

// grow-only pinned host buffer of the calling thread: the burst log of the receive loop comes back through it
// (a fresh hipHostMalloc of some megabytes per call would cost more than the loop itself)
int host_log(size_t bytes, unsigned char **out)
{
	struct Buf {                 // never freed: the runtime may be gone by the time thread-locals are destroyed
		void *p = nullptr;
		size_t n = 0;
	};
	static thread_local Buf b;
	if (b.n < bytes) {
		if (b.p) (void)hipHostFree(b.p);
		b.p = nullptr;
		b.n = 0;
		HIP_TRY(hipHostMalloc(&b.p, bytes + bytes / 4, hipHostMallocDefault));
		b.n = bytes + bytes / 4;
	}
	*out = static_cast<unsigned char *>(b.p);
	return 0;
}

// (profiling build, GMR1_HIP_RX_TIMING: host-side stamps of a call's stages on stderr)
bool rx_timing()
{
	static const bool timing = profile_env("GMR1_HIP_RX_TIMING") != nullptr;
	return timing;
}

// wall time of the phases of this thread's last gmr1_hip_rx_run* call, microseconds (gmr1_hip_rx_run_last_timing)
thread_local double t_last_timing[5] = {0, 0, 0, 0, 0};

}  // namespace

int RxRun::acquire()
{
	// The acquisition (fcch_single_init / fcch_multi_process, gmr1_rx.c:605-744) is one chain on the stream, decisions
	// included (fcch_acquire_enqueue, capi_fcch.cpp -- what gmr1_hip_fcch_acquire_batch_dev runs): the carriers' offsets and
	// lengths go up in one copy, one struct gmr1_hip_fcch_acq per carrier comes back, and the chains are set up from those.
	static_assert(kMaxPeaks == kAcqPeaks && kMaxPeaks == GMR1_HIP_ACQ_MAX_CHAINS, "candidate slots");
	const bool timing = rx_timing();
	RxClock::time_point tp[6];
	int n_tp = 0;
	auto stamp = [&] { if (timing && n_tp < 6) tp[n_tp++] = RxClock::now(); };
	stamp();
	// one block, device and pinned host mirror
	const size_t total = AcqBlock(nullptr, (size_t)A).bytes;
	unsigned char *d, *h;
	if ((r = acq_scratch(1, total, &d))) return r;
	if ((r = host_log(total, &h))) return r;
	const AcqBlock da(d, (size_t)A), ha(h, (size_t)A);
	std::memcpy(ha.offset, offset, (size_t)A * 8);
	std::memcpy(ha.length, length, (size_t)A * 8);
	HIP_TRY(hipMemcpyAsync(da.offset, ha.offset, da.up_bytes, hipMemcpyHostToDevice, st));
	stamp();
	if ((r = fcch_acquire_enqueue(st, 0, A, sps, iq, da.offset, da.length, nullptr, length, da.results))) return r;
	stamp();
	HIP_TRY(hipMemcpyAsync(ha.results, da.results, (size_t)A * sizeof(gmr1_hip_fcch_acq), hipMemcpyDeviceToHost, st));
	stamp();
	HIP_TRY(hipStreamSynchronize(st));
	stamp();
	if (timing)
		fprintf(stderr, "acquire: prepare + first copy %.1f us, launches %.1f us, copy back enqueued %.1f us, waited %.1f us\n",
		        us_between(tp[0], tp[1]), us_between(tp[1], tp[2]), us_between(tp[2], tp[3]), us_between(tp[3], tp[4]));
	const gmr1_hip_fcch_acq *res = ha.results;
	for (int i = 0; i < A; i++) {
		if (res[i].status) { stat[i] = res[i].status; continue; }
		for (int j = 0; j < res[i].n_chains; j++)
			chains.push_back({i, nch[i]++, offset[i], (int)length[i], res[i].chain_align[j], res[i].freq_err, 0, 0, 0,
			                  std::nanf("inf"), false});
	}
	return 0;
}

namespace {

// ---- process_bcch (gmr1_rx.c:852-895) for every chain ------------------------------------------
// Three launches (launch_rx_loop): k_rx_chain walks each chain through all of its frames on the GPU (rounds of
// CCCH bursts up to the next BCCH burst, whose result feeds back before the next round; rx_loop.h), k_rx4 takes the
// CCCH bursts it listed, k_rx_merge writes what the reference hands to GSMTAP -- the records, in frame order -- plus,
// when a traffic pass follows, the per-frame context rx_tch3 sees.  The host only collects them.

// The loop's one block of device memory.  Its front part has a mirror in pinned host memory:
// [records | counters (n_rounds, n_rec, n_frames, the packed total) | states | frame index, gate level per record | frame log];
// behind it, device only, what passes between the loop's three launches (RxLoopArgs): the round logs, the CCCH lists
// (a frame holds at most one burst of the list; each time slice of the walk starts its part at a multiple of four).
struct LoopLayout {
	int nc, max_frames, max_rounds, rec_stride, c_stride;
	bool want_ctx, pack;
	size_t mirrored = 0, bytes = 0;      // the front part; the whole block

	explicit LoopLayout(const RxRun &run) : nc((int)run.chains.size()), want_ctx(run.tch != nullptr), pack(!run.tch && !run.csd)
	{
		const int frame_len = run.sps * 24 * 39;
		max_frames = 0;
		for (const RxChain &c : run.chains)
			max_frames = std::max(max_frames, c.len / frame_len + 2);
		// every round but the last covers at least seven frames (seven CCCH bursts, or fewer and the BCCH burst
		// that closes its eight-frame cycle); burst_map only refuses windows at the very ends of the capture
		max_rounds = max_frames / 7 + 8;
		rec_stride = max_rounds * kLoopPerRound;
		c_stride = ((max_frames + 3) & ~3) + 4 * kLoopSlices;
		RxLoopArgs none;
		bytes = carve(nullptr, &none);
	}

	// The one description of the block: on a null base it measures it, on the device block it gives the kernels their
	// pointers, on the pinned mirror the host the same names for the front part.  Returns the bytes taken.
	size_t carve(unsigned char *base, RxLoopArgs *la)
	{
		Carve c(base);
		const size_t nrec = (size_t)nc * rec_stride, nslot = (size_t)nc * c_stride;
		std::memset(la, 0, sizeof(*la));
		la->rec_stride = rec_stride;
		la->max_rounds = max_rounds;
		la->c_stride = c_stride;
		la->rec = c.take<gmr1_hip_rx_record>(nrec);
		la->n_rounds = c.take<int32_t>((size_t)nc * 3 + 1);
		la->n_rec = la->n_rounds + nc;
		la->n_frames = la->n_rec + nc;
		la->state = c.take<RxLoopState>((size_t)nc);
		if (want_ctx) {
			la->rec_frame = c.take<int32_t>(nrec);
			la->rec_minen = c.take<float>(nrec);
			la->flog = c.take<RxLoopFrame>((size_t)nc * max_frames);
			la->flog_stride = max_frames;
		}
		mirrored = c.bytes();
		la->rounds = c.take<RxLoopRound>((size_t)nc * max_rounds);
		la->n_ccch = c.take<int32_t>((size_t)nc);
		la->fin = c.take<int32_t>((size_t)nc);
		la->slice_end = c.take<int32_t>(up128((size_t)nc * 4) / 4 * (kLoopSlices + 1));
		la->c_off = c.take<uint64_t>(nslot);
		la->c_fs = c.take<float>(nslot);
		la->c_kind = c.take<uint8_t>(nslot);
		la->c_meta = c.take<RxLoopCcch>(nslot);
		la->c_l2 = c.take<uint8_t>(nslot * 24);
		la->c_crc = c.take<int32_t>(nslot);
		la->c_conv = c.take<int32_t>(nslot);
		la->c_rv = c.take<int32_t>(nslot);
		la->c_en = c.take<float>(nslot);
		if (pack) {
			la->packed = c.take<gmr1_hip_rx_record>(nrec);
			la->n_packed = la->n_frames + nc;
		}
		return c.bytes();
	}
};

// the launches, and what they wrote back on the host: la names the device block, ha its pinned mirror
int loop_launch(RxRun &run, const LoopLayout &lay, RxLoopArgs la, const RxLoopArgs &ha, RxClock::time_point t_start)
{
	hipStream_t st = run.st;
	const int nc = lay.nc;
	const size_t st_bytes = (size_t)nc * sizeof(RxLoopState);
	const size_t cnt_bytes = (size_t)((unsigned char *)ha.state - (unsigned char *)ha.n_rounds);
	const auto t_a = RxClock::now();
	if (run.loop_state) {
		la.state = run.loop_state;
	} else {
		std::vector<RxLoopState> st0((size_t)nc);
		for (int ci = 0; ci < nc; ci++)
			st0[ci] = rx_first_state(run.chains[ci], rx_label(run.arfcn, run.chains[ci].a), run.chains[ci].done ? 1 : 0);
		HIP_TRY(hipMemcpyAsync(la.state, st0.data(), st_bytes, hipMemcpyHostToDevice, st));
	}
	const auto t_b = RxClock::now();
	int r = rx_loop_dev_impl(st, nc, run.sps, run.iq, la);
	if (r) return r;
	if (rx_timing())
		fprintf(stderr, "frame loop: prepare %.1f us, states copy enqueued %.1f us, launches %.1f us\n", us_between(t_start, t_a),
		        us_between(t_a, t_b), us_since(t_b));
	if (!lay.pack) {
		HIP_TRY(hipMemcpyAsync(ha.rec, la.rec, lay.mirrored, hipMemcpyDeviceToHost, st));
		if (run.loop_state)
			HIP_TRY(hipMemcpyAsync(ha.state, run.loop_state, st_bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		run.t_loop_gpu_us = us_since(t_start);
		return 0;
	}
	// counters and states first (a few KB), then exactly the records there are
	if (run.loop_state) {
		HIP_TRY(hipMemcpyAsync(ha.n_rounds, la.n_rounds, cnt_bytes, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(ha.state, run.loop_state, st_bytes, hipMemcpyDeviceToHost, st));
	} else {
		HIP_TRY(hipMemcpyAsync(ha.n_rounds, la.n_rounds, cnt_bytes + up128(st_bytes), hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	run.t_chain_us = us_since(t_start);
	const int n_total = ha.n_rounds[3 * nc];
	if (n_total < 0 || (size_t)n_total > (size_t)nc * lay.rec_stride)
		return fail(-EIO, "rx loop: packed record count %d out of range", n_total);
	const int fit = std::max(0, std::min(n_total, run.max_records));
	if (fit) {
		// device memory and pinned / registered host memory take the copy directly; pageable memory goes through the pinned block
		hipPointerAttribute_t at;
		const bool known = hipPointerGetAttributes(&at, run.out) == hipSuccess &&
		                   (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged);
		if (!known)
			(void)hipGetLastError();
		const size_t nb = (size_t)fit * sizeof(gmr1_hip_rx_record);
		HIP_TRY(hipMemcpyAsync(known ? run.out : ha.rec, la.packed, nb, known ? hipMemcpyDefault : hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if (!known)
			std::memcpy(run.out, ha.rec, nb);
	}
	run.direct = true;
	run.direct_total = n_total;
	run.t_loop_gpu_us = us_since(t_start);
	return 0;
}

// the mirror into the chains (where the walk left them) and their walks (what it found)
void loop_collect(RxRun &run, const LoopLayout &lay, const RxLoopArgs &ha)
{
	const int rec_stride = lay.rec_stride;
	for (int ci = 0; ci < lay.nc; ci++) {
		RxChain &c = run.chains[ci];
		RxWalk &w = run.walks[ci];
		const int n_rec = ha.n_rec[ci], n_fr = ha.n_frames[ci];
		if (ha.n_rounds[ci] >= lay.max_rounds || n_rec > rec_stride || (lay.want_ctx && n_fr > lay.max_frames)) {
			// this chain outgrew its buffers: its carrier's status says so, its records are dropped, the others go on
			fail(-EIO, "rx loop: chain %d of carrier %d outgrew its buffers (%d rounds, %d records, %d frames)", c.chain,
			     c.a, ha.n_rounds[ci], n_rec, n_fr);
			run.stat[c.a] = -EIO;
			c.done = true;
			c.outgrew = true;
			continue;
		}
		const gmr1_hip_rx_record *rp = ha.rec + (size_t)ci * rec_stride;
		if (!lay.pack)
			w.rec.assign(rp, rp + n_rec);
		w.n_rec = n_rec;
		if (lay.want_ctx) {
			const int32_t *fp = ha.rec_frame + (size_t)ci * rec_stride;
			const float *mp = ha.rec_minen + (size_t)ci * rec_stride;
			const RxLoopFrame *lp = ha.flog + (size_t)ci * lay.max_frames;
			w.rec_frame.assign(fp, fp + n_rec);
			w.log.resize((size_t)n_fr);
			for (int f = 0; f < n_fr; f++)
				w.log[f] = {lp[f].align, lp[f].freq_err, lp[f].fn};
			// IMM.ASS on the CCCH starts the TCH3 follow-up in that very frame (gmr1_rx.c:235-246, 836-841)
			for (int k = 0; k < n_rec; k++) {
				const uint8_t *l2 = rp[k].l2;
				if (rp[k].type == 2 && l2[1] == 0x06 && l2[2] == 0x3f)
					w.events.push_back({fp[k], ((l2[8] & 0x03) << 3) | (l2[9] >> 5), (l2[8] & 0xfc) >> 2, mp[k]});
			}
		} else if (!lay.pack) {
			w.rec_frame.assign((size_t)n_rec, 0);
		}
		const RxLoopState &s = ha.state[ci];
		c.align = s.align; c.freq_err = s.freq_err; c.fn = s.fn; c.delay = s.delay; c.stn = s.stn;
		c.bcch_energy = s.bcch_energy;
		c.done = s.done != 0;
	}
}

}  // namespace

int RxRun::frame_loop()
{
	walks.assign(chains.size(), RxWalk());
	if (chains.empty())
		return 0;
	const auto t_start = RxClock::now();
	LoopLayout lay(*this);
	DevState *ds;
	if ((r = dev_state(&ds))) return r;
	void *ws;
	if ((r = dev_workspace(ds, lay.bytes + 128, &ws))) return r;
	unsigned char *h;
	if ((r = host_log(lay.mirrored, &h))) return r;
	RxLoopArgs la, ha;
	lay.carve(reinterpret_cast<unsigned char *>(up128((uintptr_t)ws)), &la);
	lay.carve(h, &ha);
	if ((r = loop_launch(*this, lay, la, ha, t_start))) return r;
	loop_collect(*this, lay, ha);
	return 0;
}

namespace {

// What one device-form call hands in: the arguments of gmr1_hip_rx_run_full_dev under their names, plus what only some
// entries have, in the order the entries name them.  Everything is device memory but the outputs named otherwise in gmr1_hip.h.
struct RxRunCall {
	void *stream = nullptr;
	int n_arfcn = 0, sps = 0;
	const float *iq = nullptr, *tch = nullptr, *csd = nullptr;
	const uint64_t *offset = nullptr, *length = nullptr;
	const uint16_t *arfcn = nullptr;
	const uint8_t *kc = nullptr;
	gmr1_hip_rx_record *out = nullptr;
	int max_records = 0;
	int *n_records = nullptr;
	gmr1_hip_rx_big_record *big_out = nullptr;
	int max_big = 0;
	int *n_big = nullptr;
	int32_t *status = nullptr, *n_chains = nullptr;
	int32_t *rec_per_carrier = nullptr;          // optional: how many of the records each carrier contributed
	bool want_audio = false;                     // gmr1_hip_rx_run_voice*: the audio outputs are required
	gmr1_hip_rx_audio *audio_out = nullptr;
	int max_audio = 0;
	int *n_audio = nullptr;
};

// every one-shot entry
int rx_run_full_impl(const RxRunCall &c)
{
	hipStream_t st = (hipStream_t)c.stream;
	if (c.n_records) *c.n_records = 0;
	if (c.n_big) *c.n_big = 0;
	if (c.n_audio) *c.n_audio = 0;
	if (c.want_audio && (!c.n_audio || c.max_audio < 0 || (c.max_audio > 0 && !c.audio_out)))
		return fail(-EINVAL, "rx_run_voice: n_audio (and audio_out when max_audio > 0) are required, and no negative count");
	if (c.csd && (!c.tch || !c.n_big || c.max_big < 0 || (c.max_big > 0 && !c.big_out)))
		return fail(-EINVAL, "rx_run: the CSD carrier needs the traffic carrier and the big-record outputs");
	if (c.n_arfcn < 0 || !c.iq || !c.offset || !c.length || !c.n_records || (c.max_records > 0 && !c.out) || c.max_records < 0)
		return fail(-EINVAL, "rx_run: iq/offset/length/n_records (and out when max_records > 0) are required");
	if (c.sps < 1 || c.sps > 16)                  // gmr1_rx.c:919-922
		return fail(-EINVAL, "rx_run: sps=%d unsupported (1..16)", c.sps);
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (c.n_arfcn == 0) return 0;
	// the whole call holds the device's workspace, the loop's side stream and its events: calls from other threads wait
	WsLease lease;
	if ((r = lease.acquire(ds, st))) return r;
	for (int i = 0; i < c.n_arfcn; i++)
		if (c.length[i] > 0x7fffffffull)
			return fail(-EINVAL, "rx_run: carrier %d longer than 2^31-1 samples", i);

	RxRun run(st, c.sps, c.iq, c.tch, c.csd, c.n_arfcn, c.offset, c.length, c.arfcn, c.kc, c.out, c.max_records);
	RxVoice voice;
	if (c.want_audio && c.tch) {
		voice.out = c.audio_out;
		voice.max_out = c.max_audio;
		run.voice = &voice;
	}
	const auto t0 = RxClock::now();
	if ((r = run.acquire())) return r;
	const auto t1 = RxClock::now();
	if ((r = run.frame_loop())) return r;
	const auto t2 = RxClock::now();
	if (c.tch && (r = run.tch3_pass())) return r;
	if (c.csd && (r = tch9_follow_chains(st, c.sps, c.csd, c.arfcn, c.kc, run.chains, run.walks))) return r;
	const double t_acq = us_between(t0, t1), t_loop = us_between(t1, t2), t_tch = us_since(t2);
	const double chain = run.t_chain_us > 0 ? run.t_chain_us : run.t_loop_gpu_us;
	t_last_timing[0] = t_acq;                                   // FCCH acquisition incl. the chains set up from its result
	t_last_timing[1] = chain;                                   // frame loop: launches until its kernels are through
	t_last_timing[2] = run.t_loop_gpu_us - chain;               // records to the caller's buffer
	t_last_timing[3] = t_loop - run.t_loop_gpu_us;              // host work around the loop (chains set up, states read)
	t_last_timing[4] = t_tch;                                   // traffic-channel passes
	// GMR1_HIP_RX_TIMING=1: wall time of the phases on stderr (profiling only)
	if (rx_timing())
		fprintf(stderr, "rx_run: acquire %.0f us, frame loop %.0f us (launch+copy %.0f, collect %.0f), traffic passes %.0f us\n",
		        t_acq, t_loop, run.t_loop_gpu_us, t_loop - run.t_loop_gpu_us, t_tch);

	// ---- hand back: carriers in order, chains in order, frames in order -------------------------
	// (a direct run's records are already in the caller's buffer, in this very order: k_rx_pack)
	*c.n_records = run.direct ? run.direct_total : rx_hand_back(run.walks, c.out, c.max_records);
	if (c.n_audio) *c.n_audio = voice.found;
	if (c.n_big) {
		int tb = 0;
		for (const RxWalk &w : run.walks)
			for (const gmr1_hip_rx_big_record &rec : w.big) {
				if (tb < c.max_big)
					c.big_out[tb] = rec;
				tb++;
			}
		*c.n_big = tb;
	}
	for (int i = 0; i < c.n_arfcn; i++) {
		if (c.status) c.status[i] = run.stat[i];
		if (c.n_chains) c.n_chains[i] = run.nch[i];
		if (c.rec_per_carrier) c.rec_per_carrier[i] = 0;
	}
	if (c.rec_per_carrier)
		for (size_t ci = 0; ci < run.walks.size(); ci++)
			c.rec_per_carrier[run.chains[ci].a] += run.direct ? run.walks[ci].n_rec : (int)run.walks[ci].rec.size();
	return 0;
}

}  // namespace

namespace gmr1 {
int rx_run_dev_counted(void *stream, int n_arfcn, int sps, const float *iq, const uint64_t *offset, const uint64_t *length,
                       const uint16_t *arfcn, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                       int32_t *status, int32_t *n_chains, int32_t *rec_per_carrier)
{
	return rx_run_full_impl({.stream = stream, .n_arfcn = n_arfcn, .sps = sps, .iq = iq, .offset = offset, .length = length, .arfcn = arfcn,
	                         .out = out, .max_records = max_records, .n_records = n_records, .status = status, .n_chains = n_chains,
	                         .rec_per_carrier = rec_per_carrier});
}
}  // namespace gmr1

namespace {

// what the host forms do before their device form: the carriers lie inside iq_len, and iq / tch / csd (each iq_len
// samples, or NULL; csd itself may be NULL: the entry has none) go to the device, their device copies put in their place
int rx_run_stage_in(Stage &sg, int n_arfcn, uint64_t iq_len, const uint64_t *offset, const uint64_t *length, const float **iq,
                    const float **tch, const float **csd)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_arfcn < 0 || !*iq || !offset || !length)
		return fail(-EINVAL, "rx_run: iq/offset/length are required");
	for (int i = 0; i < n_arfcn; i++)
		if (offset[i] + length[i] > iq_len)
			return fail(-EINVAL, "rx_run: carrier %d runs past the end of iq", i);
	for (const float **x : {iq, tch, csd})
		if (x) *x = sg.in(*x, (size_t)iq_len * 2);
	return sg.err();
}

}  // namespace

extern "C" {

int gmr1_hip_rx_run_last_timing(double *us5)
{
	if (!us5)
		return -EINVAL;
	for (int i = 0; i < 5; i++)
		us5[i] = t_last_timing[i];
	return 0;
}

int gmr1_hip_rx_run_full_dev(void *stream_, int n_arfcn, int sps, const float *iq, const float *tch,
                             const float *csd, const uint64_t *offset, const uint64_t *length,
                             const uint16_t *arfcn, const uint8_t *kc,
                             struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                             struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                             int32_t *status, int32_t *n_chains)
{
	return rx_run_full_impl({.stream = stream_, .n_arfcn = n_arfcn, .sps = sps, .iq = iq, .tch = tch, .csd = csd, .offset = offset,
	                         .length = length, .arfcn = arfcn, .kc = kc, .out = out, .max_records = max_records, .n_records = n_records,
	                         .big_out = big_out, .max_big = max_big, .n_big = n_big, .status = status, .n_chains = n_chains});
}

int gmr1_hip_rx_run_tch_dev(void *stream, int n_arfcn, int sps, const float *iq, const float *tch,
                            const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                            const uint8_t *kc,
                            struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                            int32_t *status, int32_t *n_chains)
{
	return gmr1_hip_rx_run_full_dev(stream, n_arfcn, sps, iq, tch, nullptr, offset, length, arfcn, kc,
	                                out, max_records, n_records, nullptr, 0, nullptr, status, n_chains);
}

// the TCH3 follow-up with the followed calls decoded to audio: the pass hands its frames to the speech decoder where they lie
int gmr1_hip_rx_run_voice_dev(void *stream, int n_arfcn, int sps, const float *iq, const float *tch,
                              const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                              struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                              int32_t *status, int32_t *n_chains,
                              struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	return rx_run_full_impl({.stream = stream, .n_arfcn = n_arfcn, .sps = sps, .iq = iq, .tch = tch, .offset = offset, .length = length,
	                         .arfcn = arfcn, .kc = kc, .out = out, .max_records = max_records, .n_records = n_records, .status = status,
	                         .n_chains = n_chains, .want_audio = true, .audio_out = audio_out, .max_audio = max_audio, .n_audio = n_audio});
}

int gmr1_hip_rx_run_voice(int n_arfcn, int sps, const float *iq, const float *tch, uint64_t iq_len,
                          const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                          struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                          int32_t *status, int32_t *n_chains,
                          struct gmr1_hip_rx_audio *audio_out, int max_audio, int *n_audio)
{
	if (n_records) *n_records = 0;
	if (n_audio) *n_audio = 0;
	if (!n_audio || max_audio < 0 || (max_audio > 0 && !audio_out))
		return fail(-EINVAL, "rx_run_voice: n_audio (and audio_out when max_audio > 0) are required, and no negative count");
	Stage sg;
	const int r = rx_run_stage_in(sg, n_arfcn, iq_len, offset, length, &iq, &tch, nullptr);
	if (r) return r;
	return gmr1_hip_rx_run_voice_dev(nullptr, n_arfcn, sps, iq, tch, offset, length, arfcn, kc, out, max_records, n_records,
	                                 status, n_chains, audio_out, max_audio, n_audio);
}

int gmr1_hip_rx_run_full(int n_arfcn, int sps, const float *iq, const float *tch, const float *csd, uint64_t iq_len,
                         const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                         struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                         struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                         int32_t *status, int32_t *n_chains)
{
	if (n_records) *n_records = 0;
	if (n_big) *n_big = 0;
	Stage sg;
	const int r = rx_run_stage_in(sg, n_arfcn, iq_len, offset, length, &iq, &tch, &csd);
	if (r) return r;
	return gmr1_hip_rx_run_full_dev(nullptr, n_arfcn, sps, iq, tch, csd, offset, length, arfcn, kc, out, max_records,
	                                n_records, big_out, max_big, n_big, status, n_chains);
}

int gmr1_hip_rx_run_dev(void *stream, int n_arfcn, int sps, const float *iq,
                        const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                        struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                        int32_t *status, int32_t *n_chains)
{
	return gmr1_hip_rx_run_tch_dev(stream, n_arfcn, sps, iq, nullptr, offset, length, arfcn, nullptr,
	                               out, max_records, n_records, status, n_chains);
}

int gmr1_hip_rx_run_tch(int n_arfcn, int sps, const float *iq, const float *tch, uint64_t iq_len,
                        const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                        struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                        int32_t *status, int32_t *n_chains)
{
	return gmr1_hip_rx_run_full(n_arfcn, sps, iq, tch, nullptr, iq_len, offset, length, arfcn, kc, out, max_records, n_records,
	                            nullptr, 0, nullptr, status, n_chains);
}

int gmr1_hip_rx_run(int n_arfcn, int sps, const float *iq, uint64_t iq_len,
                    const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn,
                    struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                    int32_t *status, int32_t *n_chains)
{
	return gmr1_hip_rx_run_tch(n_arfcn, sps, iq, nullptr, iq_len, offset, length, arfcn, nullptr, out, max_records, n_records,
	                           status, n_chains);
}

}  // extern "C"
