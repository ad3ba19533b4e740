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
// The traffic channels never feed back into that loop, so their follow-ups run after it as batched
// passes of their own: RxRun::tch3_pass hands every chain with an IMMEDIATE ASSIGNMENT to the batched call follower
// (capi_tch3_follow.cpp), whose state machine runs on the device, one invocation per assignment a chain sees
// (tch3_follow_chains, which a push of the streaming loop runs over its own frames too);
// RxRun::tch9_pass demodulates, classifies on the host and decodes.  GSMTAP transport and per-burst stderr
// logging are out of scope; what GSMTAP would have carried comes back as records.

#include "capi_common.h"
#include "fcch_acq.h"
#include "rx_stream.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "../../include/gmr1_hip.h"

using namespace gmr1;

namespace {

constexpr int kStartDiscard = 8000;   // gmr1_rx.c:52
constexpr int kMaxPeaks = 16;         // gmr1_rx.c:650

struct FrameCtx { int align; float freq_err; int fn; };       // what rx_tch3 sees in a frame
struct AssEvt { int frame; int tn, p; float ref_energy; };     // an IMMEDIATE ASSIGNMENT taken from the CCCH

struct RxChain {
	int a;                // carrier index
	int chain;            // chain index within the carrier
	uint64_t base;        // first sample of the carrier in iq
	int len;              // samples of the carrier
	int align;
	float freq_err;
	int fn, delay, stn;
	float bcch_energy;
	bool done;
	bool outgrew = false;                // its walk outgrew the loop's buffers (the carrier's status is -EIO)
	std::vector<gmr1_hip_rx_record> rec;
	int n_rec = 0;                       // records of the chain when they went straight to the caller (RxRun::direct)
	std::vector<int> rec_frame;          // frame (index into log) each record belongs to
	std::vector<FrameCtx> log;           // one entry per loop iteration of process_bcch (only with a traffic carrier)
	std::vector<AssEvt> events;
	std::vector<AssEvt> events9;         // ASSIGNMENT COMMAND 1 taken from a FACCH3 (frame, tn)
	std::vector<gmr1_hip_rx_big_record> big;
};

void emit(RxChain &c, uint16_t arfcn, int type, int fn, int tn, const uint8_t *l2, int conv, int frame, int len = 24)
{
	gmr1_hip_rx_record r;
	std::memset(&r, 0, sizeof(r));
	r.arfcn = arfcn;
	r.chain = (uint8_t)c.chain;
	r.type = (uint8_t)type;
	r.fn = (uint32_t)fn;
	r.tn = (uint8_t)tn;
	r.crc = 0;
	r.len = (uint8_t)len;
	r.conv = conv;
	std::memcpy(r.l2, l2, (size_t)len);
	c.rec.push_back(r);
	c.rec_frame.push_back(frame);
}

size_t up128(size_t x) { return (x + 127) & ~(size_t)127; }

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


// One call of gmr1_hip_rx_run*: what the phases share.  The phases run in the order the reference's main()
// runs them (gmr1_rx.c:897-975); each is one member function below.
struct RxRun {
	hipStream_t st;
	int sps;
	const float *iq, *tch, *csd;
	const uint64_t *offset, *length;
	const uint16_t *arfcn;
	const uint8_t *kc;
	int A;                                   // carriers
	int r = 0;
	std::vector<int32_t> stat, nch;          // per carrier: status, chains followed
	std::vector<RxChain> chains;
	double t_loop_gpu_us = 0;                // launch to log-on-host
	double t_chain_us = 0;                   // ... of which: launches until the loop's kernels are through (counters on the host)
	// hand-back of a plain BCCH / CCCH run (no traffic follow-up): the records are closed up on the device in the order
	// they are returned in (k_rx_pack) and copied ONCE, as many as there are -- straight into the caller's buffer when
	// that is device memory or pinned host memory, else through the library's pinned block
	gmr1_hip_rx_record *out = nullptr;
	int max_records = 0;
	bool direct = false;
	int direct_total = 0;
	// the streaming loop (gmr1_hip_rx_stream_*): the chains' states live in this device array across pushes -- the walk
	// starts from and writes back to it, nothing is uploaded
	RxLoopState *loop_state = nullptr;

	int acquire();        // fcch_single_init + fcch_multi_process
	int frame_loop();     // process_bcch: BCCH / CCCH, in rounds
	int tch3_pass();      // rx_tch3 and its helpers
	int tch9_pass();      // rx_tch9
};


// wall time of the phases of this thread's last gmr1_hip_rx_run* call, microseconds (gmr1_hip_rx_run_last_timing)
static thread_local double t_last_timing[5] = {0, 0, 0, 0, 0};

int RxRun::acquire()
{
	// The acquisition (fcch_single_init / fcch_multi_process, gmr1_rx.c:605-744) is one chain on the stream, decisions
	// included (fcch_acquire_enqueue, capi_fcch.cpp -- what gmr1_hip_fcch_acquire_batch_dev runs): the carriers' offsets and
	// lengths go up in one copy, one struct gmr1_hip_fcch_acq per carrier comes back, and the chains are set up from those.
	static_assert(kMaxPeaks == kAcqPeaks && kMaxPeaks == GMR1_HIP_ACQ_MAX_CHAINS, "candidate slots");
	// (profiling build, GMR1_HIP_RX_TIMING: host-side stamps of this call's stages on stderr)
	static const bool timing = profile_env("GMR1_HIP_RX_TIMING") != nullptr;
	std::chrono::steady_clock::time_point tp[6];
	int n_tp = 0;
	auto stamp = [&] { if (timing && n_tp < 6) tp[n_tp++] = std::chrono::steady_clock::now(); };
	stamp();
	// one block, device and pinned host mirror: [offset | length | results]
	const size_t o_len = up128((size_t)A * 8), o_res = o_len + up128((size_t)A * 8);
	const size_t total = o_res + (size_t)A * sizeof(gmr1_hip_fcch_acq);
	unsigned char *d, *h;
	if ((r = acq_scratch(1, total, &d))) return r;
	if ((r = host_log(total, &h))) return r;
	std::memcpy(h, offset, (size_t)A * 8);
	std::memcpy(h + o_len, length, (size_t)A * 8);
	HIP_TRY(hipMemcpyAsync(d, h, o_res, hipMemcpyHostToDevice, st));
	stamp();
	if ((r = fcch_acquire_enqueue(st, 0, A, sps, iq, reinterpret_cast<const uint64_t *>(d),
	                              reinterpret_cast<const uint64_t *>(d + o_len), nullptr, length,
	                              reinterpret_cast<gmr1_hip_fcch_acq *>(d + o_res)))) return r;
	stamp();
	HIP_TRY(hipMemcpyAsync(h + o_res, d + o_res, (size_t)A * sizeof(gmr1_hip_fcch_acq), hipMemcpyDeviceToHost, st));
	stamp();
	HIP_TRY(hipStreamSynchronize(st));
	stamp();
	if (timing) {
		auto us = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3; };
		fprintf(stderr, "acquire: prepare + first copy %.1f us, launches %.1f us, copy back enqueued %.1f us, waited %.1f us\n",
		        us(tp[0], tp[1]), us(tp[1], tp[2]), us(tp[2], tp[3]), us(tp[3], tp[4]));
	}
	const gmr1_hip_fcch_acq *res = reinterpret_cast<const gmr1_hip_fcch_acq *>(h + o_res);
	for (int i = 0; i < A; i++) {
		if (res[i].status) { stat[i] = res[i].status; continue; }
		for (int j = 0; j < res[i].n_chains; j++) {
			RxChain c;
			c.a = i;
			c.chain = nch[i]++;
			c.base = offset[i];
			c.len = (int)length[i];
			c.align = res[i].chain_align[j];
			c.freq_err = res[i].freq_err;
			c.fn = 0; c.delay = 0; c.stn = 0;
			c.bcch_energy = std::nanf("inf");
			c.done = false;
			chains.push_back(std::move(c));
		}
	}
	return 0;
}

int RxRun::frame_loop()
{
	// ---- process_bcch (gmr1_rx.c:852-895) for every chain ------------------------------------------
	// Three launches (launch_rx_loop): k_rx_chain walks each chain through all of its frames on the GPU (rounds of
	// CCCH bursts up to the next BCCH burst, whose result feeds back before the next round; rx_loop.h), k_rx4 takes the
	// CCCH bursts it listed, k_rx_merge writes what the reference hands to GSMTAP -- the records, in frame order -- plus,
	// when a traffic pass follows, the per-frame context rx_tch3 sees.  The host only collects them.
	const int nc = (int)chains.size();
	if (!nc)
		return 0;
	const auto t_start = std::chrono::steady_clock::now();
	const int frame_len = sps * 24 * 39;
	int max_frames = 0;
	for (const RxChain &c : chains)
		max_frames = std::max(max_frames, c.len / frame_len + 2);
	// every round but the last covers at least seven frames (seven CCCH bursts, or fewer and the BCCH burst
	// that closes its eight-frame cycle); burst_map only refuses windows at the very ends of the capture
	const int max_rounds = max_frames / 7 + 8;
	const int rec_stride = max_rounds * kLoopPerRound;
	const bool want_ctx = tch != nullptr;
	std::vector<RxLoopState> st0((size_t)nc);
	for (int ci = 0; ci < nc; ci++) {
		const RxChain &c = chains[ci];
		st0[ci] = {c.base, c.len, c.align, c.freq_err, c.fn, c.delay, c.stn, c.done ? 1 : 0, c.bcch_energy,
		           (uint16_t)(arfcn ? arfcn[c.a] : (uint16_t)c.a), (uint16_t)c.chain};
	}
	// one block of device memory and its mirror in pinned host memory:
	// [records | counters (n_rounds, n_rec, n_frames) | states | frame index + gate level per record | frame log]
	const size_t rec_bytes = up128((size_t)nc * rec_stride * sizeof(gmr1_hip_rx_record));
	const size_t cnt_bytes = up128(((size_t)nc * 3 + 1) * 4);      // + the packed total
	const bool pack = !tch && !csd;
	const size_t st_bytes = up128((size_t)nc * sizeof(RxLoopState));
	const size_t rf_bytes = want_ctx ? up128((size_t)nc * rec_stride * 4) : 0;
	const size_t fl_bytes = want_ctx ? up128((size_t)nc * max_frames * sizeof(RxLoopFrame)) : 0;
	const size_t total = rec_bytes + cnt_bytes + st_bytes + 2 * rf_bytes + fl_bytes;
	// ... and, device only, what passes between the loop's three launches (RxLoopArgs): the round logs, the CCCH lists
	// (a frame holds at most one burst of the list; each time slice of the walk starts its part at a multiple of four)
	const int c_stride = ((max_frames + 3) & ~3) + 4 * kLoopSlices;
	const size_t nslot = (size_t)nc * c_stride;
	const size_t rl_bytes = up128((size_t)nc * max_rounds * sizeof(RxLoopRound));
	const size_t s8 = up128(nslot * 8), s4 = up128(nslot * 4), s1 = up128(nslot), s12 = up128(nslot * sizeof(RxLoopCcch)),
	             s24 = up128(nslot * 24);
	const size_t scratch = rl_bytes + up128((size_t)nc * 4) * (2 + kLoopSlices + 1) + s8 + s4 + s1 + s12 + s24 + 4 * s4;
	DevState *ds;
	r = dev_state(&ds);
	if (r) return r;
	void *ws;
	r = dev_workspace(ds, total + scratch + (pack ? rec_bytes : 0) + 128, &ws);
	if (r) return r;
	unsigned char *d = reinterpret_cast<unsigned char *>(((uintptr_t)ws + 127) & ~(uintptr_t)127);
	unsigned char *h;
	r = host_log(total, &h);
	if (r) return r;
	const size_t o_cnt = rec_bytes, o_st = o_cnt + cnt_bytes, o_rf = o_st + st_bytes, o_me = o_rf + rf_bytes,
	             o_fl = o_me + rf_bytes;
	RxLoopArgs la;
	std::memset(&la, 0, sizeof(la));
	la.state = reinterpret_cast<RxLoopState *>(d + o_st);
	la.rec = reinterpret_cast<gmr1_hip_rx_record *>(d);
	la.rec_stride = rec_stride;
	la.max_rounds = max_rounds;
	la.n_rounds = reinterpret_cast<int32_t *>(d + o_cnt);
	la.n_rec = la.n_rounds + nc;
	la.n_frames = la.n_rec + nc;
	if (want_ctx) {
		la.rec_frame = reinterpret_cast<int32_t *>(d + o_rf);
		la.rec_minen = reinterpret_cast<float *>(d + o_me);
		la.flog = reinterpret_cast<RxLoopFrame *>(d + o_fl);
		la.flog_stride = max_frames;
	}
	{
		unsigned char *q = d + total;
		auto take = [&](size_t bytes) { unsigned char *p = q; q += bytes; return p; };
		la.rounds = reinterpret_cast<RxLoopRound *>(take(rl_bytes));
		la.n_ccch = reinterpret_cast<int32_t *>(take(up128((size_t)nc * 4)));
		la.fin = reinterpret_cast<int32_t *>(take(up128((size_t)nc * 4)));
		la.slice_end = reinterpret_cast<int32_t *>(take(up128((size_t)nc * 4) * (kLoopSlices + 1)));
		la.c_stride = c_stride;
		la.c_off = reinterpret_cast<uint64_t *>(take(s8));
		la.c_fs = reinterpret_cast<float *>(take(s4));
		la.c_kind = reinterpret_cast<uint8_t *>(take(s1));
		la.c_meta = reinterpret_cast<RxLoopCcch *>(take(s12));
		la.c_l2 = reinterpret_cast<uint8_t *>(take(s24));
		la.c_crc = reinterpret_cast<int32_t *>(take(s4));
		la.c_conv = reinterpret_cast<int32_t *>(take(s4));
		la.c_rv = reinterpret_cast<int32_t *>(take(s4));
		la.c_en = reinterpret_cast<float *>(take(s4));
		if (pack) {
			la.packed = reinterpret_cast<gmr1_hip_rx_record *>(take(rec_bytes));
			la.n_packed = la.n_frames + nc;
		}
	}
	static const bool timing = profile_env("GMR1_HIP_RX_TIMING") != nullptr;
	const auto t_a = std::chrono::steady_clock::now();
	if (loop_state)
		la.state = loop_state;
	else
		HIP_TRY(hipMemcpyAsync(la.state, st0.data(), (size_t)nc * sizeof(RxLoopState), hipMemcpyHostToDevice, st));
	const auto t_b = std::chrono::steady_clock::now();
	r = rx_loop_dev_impl(st, nc, sps, iq, la);
	if (r) return r;
	if (timing) {
		auto us = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3; };
		fprintf(stderr, "frame loop: prepare %.1f us, states copy enqueued %.1f us, launches %.1f us\n", us(t_start, t_a), us(t_a, t_b),
		        us(t_b, std::chrono::steady_clock::now()));
	}
	if (pack) {
		// counters and states first (a few KB), then exactly the records there are
		if (loop_state) {
			HIP_TRY(hipMemcpyAsync(h + o_cnt, d + o_cnt, cnt_bytes, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h + o_st, loop_state, (size_t)nc * sizeof(RxLoopState), hipMemcpyDeviceToHost, st));
		} else {
			HIP_TRY(hipMemcpyAsync(h + o_cnt, d + o_cnt, cnt_bytes + st_bytes, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipStreamSynchronize(st));
		t_chain_us = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_start).count() / 1e3;
		const int n_total = reinterpret_cast<const int32_t *>(h + o_cnt)[3 * nc];
		if (n_total < 0 || (size_t)n_total > (size_t)nc * rec_stride)
			return fail(-EIO, "rx loop: packed record count %d out of range", n_total);
		const int fit = std::max(0, std::min(n_total, max_records));
		if (fit) {
			// device memory and pinned / registered host memory take the copy directly; pageable memory goes through the pinned block
			hipPointerAttribute_t at;
			const bool known = hipPointerGetAttributes(&at, out) == hipSuccess &&
			                   (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged);
			if (!known)
				(void)hipGetLastError();
			const size_t nb = (size_t)fit * sizeof(gmr1_hip_rx_record);
			if (known) {
				HIP_TRY(hipMemcpyAsync(out, la.packed, nb, hipMemcpyDefault, st));
				HIP_TRY(hipStreamSynchronize(st));
			} else {
				HIP_TRY(hipMemcpyAsync(h, la.packed, nb, hipMemcpyDeviceToHost, st));
				HIP_TRY(hipStreamSynchronize(st));
				std::memcpy(out, h, nb);
			}
		}
		direct = true;
		direct_total = n_total;
	} else {
		HIP_TRY(hipMemcpyAsync(h, d, total, hipMemcpyDeviceToHost, st));
		if (loop_state)
			HIP_TRY(hipMemcpyAsync(h + o_st, loop_state, (size_t)nc * sizeof(RxLoopState), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	t_loop_gpu_us = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_start).count() / 1e3;

	const int32_t *h_nr = reinterpret_cast<const int32_t *>(h + o_cnt), *h_nrec = h_nr + nc, *h_nfr = h_nrec + nc;
	const RxLoopState *h_st = reinterpret_cast<const RxLoopState *>(h + o_st);
	for (int ci = 0; ci < nc; ci++) {
		RxChain &c = chains[ci];
		if (h_nr[ci] >= max_rounds || h_nrec[ci] > rec_stride || (want_ctx && h_nfr[ci] > max_frames)) {
			// this chain outgrew its buffers: its carrier's status says so, its records are dropped, the others go on
			fail(-EIO, "rx loop: chain %d of carrier %d outgrew its buffers (%d rounds, %d records, %d frames)", c.chain,
			     c.a, h_nr[ci], h_nrec[ci], h_nfr[ci]);
			stat[c.a] = -EIO;
			c.done = true;
			c.outgrew = true;
			continue;
		}
		const gmr1_hip_rx_record *rp = reinterpret_cast<const gmr1_hip_rx_record *>(h) + (size_t)ci * rec_stride;
		if (!pack)
			c.rec.assign(rp, rp + h_nrec[ci]);
		c.n_rec = h_nrec[ci];
		if (want_ctx) {
			const int32_t *fp = reinterpret_cast<const int32_t *>(h + o_rf) + (size_t)ci * rec_stride;
			const float *mp = reinterpret_cast<const float *>(h + o_me) + (size_t)ci * rec_stride;
			const RxLoopFrame *lp = reinterpret_cast<const RxLoopFrame *>(h + o_fl) + (size_t)ci * max_frames;
			c.rec_frame.assign(fp, fp + h_nrec[ci]);
			c.log.resize((size_t)h_nfr[ci]);
			for (int f = 0; f < h_nfr[ci]; f++)
				c.log[f] = {lp[f].align, lp[f].freq_err, lp[f].fn};
			// IMM.ASS on the CCCH starts the TCH3 follow-up in that very frame (gmr1_rx.c:235-246, 836-841)
			for (int k = 0; k < h_nrec[ci]; k++) {
				const uint8_t *l2 = rp[k].l2;
				if (rp[k].type == 2 && l2[1] == 0x06 && l2[2] == 0x3f)
					c.events.push_back({fp[k], ((l2[8] & 0x03) << 3) | (l2[9] >> 5), (l2[8] & 0xfc) >> 2, mp[k]});
			}
		} else if (!pack) {
			c.rec_frame.assign((size_t)h_nrec[ci], 0);
		}
		const RxLoopState &s = h_st[ci];
		c.align = s.align; c.freq_err = s.freq_err; c.fn = s.fn; c.delay = s.delay; c.stn = s.stn;
		c.bcch_energy = s.bcch_energy;
		c.done = s.done != 0;
	}
	return 0;
}

// What a chain's TCH3 follow-up carries from one run of tch3_follow_chains to the next: a push of the streaming loop
// continues the call the pushes before it found (the one-shot pass starts from nothing)
struct TchCarry {
	int tn = 0;               // the timeslot of the last assignment
	bool assigned = false;    // there was one
};

// ---- TCH3 follow-up (rx_tch3, gmr1_rx.c:355-600) ----------------------------------------------
// Nothing the traffic channel does feeds back into the BCCH / CCCH loop, so it runs afterwards, for all chains at once,
// through the batched call follower (tch3_follow_enqueue, capi_tch3_follow.cpp -- what gmr1_hip_tch3_follow_batch_dev
// runs): chain calls[q] is call q, its state is slot q of a device array.  This function knows which frames of which
// chain belong to which assignment, which window each reads and where the records go -- for the one-shot pass (the whole
// capture's log; the states start from h_state0 and die with the call) and for a push of the streaming loop (this push's
// log; the states are the handle's d_state, the timeslots the handle's `carry`); the per-frame work, the state machine,
// the decodes and the ciphering state are the follower's, on the device.  rx_tch3_init runs between two invocations
// (k_tch3f_assign, on the states where they lie), so invocation g takes, of every call, the frames from its g-th
// assignment of this log up to the next one, and invocation 0 the frames before the first, which belong to the call
// carried in: a chain that is assigned once -- the usual case -- costs one invocation and one synchronisation.
// horizon: the log was walked against samples that more will follow (a push that is not the last): every logged frame
// was admitted by align + 2 * frame_len <= len, which its TCH3 window fits, so a window that does not
// is an error (-EIO) instead of a frame dropped that the one-shot call reads.
int tch3_follow_chains(hipStream_t st, int sps, const float *tch, const uint16_t *arfcn, bool want9, bool horizon,
                       std::vector<RxChain> &chains, const std::vector<int> &calls, const gmr1_hip_tch3_state *h_state0,
                       gmr1_hip_tch3_state *d_state, TchCarry *carry)
{
	struct TchItem {          // one frame of a call in which rx_tch3 maps a burst
		int call, frame;
		int tn, gen;          // the assignment it belongs to: its timeslot; 1 + its index in the log's events, 0: carried in
	};
	int r = 0;
	std::vector<TchItem> titems;
	const int n_calls = (int)calls.size();
	std::vector<size_t> next((size_t)n_calls);   // per call: its first item no invocation has taken yet
	std::vector<char> touched((size_t)n_calls, 0);
	const int t_in_len = rx_tch3_in_len(sps);
	size_t n_gen = 0;                            // invocations: one per assignment any call sees, and one before them
	bool any_event = false;
	for (int q = 0; q < n_calls; q++) {
		const RxChain &c = chains[calls[q]];
		next[q] = titems.size();
		any_event |= !c.events.empty();
		bool have = carry && carry[q].assigned;
		int tn = have ? carry[q].tn : 0;
		if (!have && c.events.empty())
			continue;
		n_gen = std::max(n_gen, c.events.size() + 1);
		size_t ev = 0;
		// IMM.ASS on the CCCH starts the follow-up in that very frame (gmr1_rx.c:235-246, 836-841)
		for (int f = have ? 0 : c.events[0].frame; f < (int)c.log.size(); f++) {
			while (ev < c.events.size() && c.events[ev].frame <= f)
				tn = c.events[ev++].tn;
			const long long begin = rx_tch3_begin(c.log[f].align, sps, tn);
			if (begin + t_in_len > c.len && horizon)
				return fail(-EIO, "tch3 follow-up: a frame the walk admitted does not hold its traffic window");
			if (begin < 0 || begin + t_in_len > c.len)
				continue;                         // burst_map fails: rx_tch3 returns before touching anything
			titems.push_back({q, f, tn, (int)ev});
		}
	}
	const int nt = (int)titems.size();
	if (!nt && (h_state0 || !any_event))
		return 0;
	// the states if they start here, first[] and an assignment per call, per frame 56 B staged and the follower's scratch;
	// no invocation has more than nt frames
	Arena arena;
	if ((r = arena.init((h_state0 ? (size_t)n_calls * sizeof(gmr1_hip_tch3_state) + 128 : 0) + ((size_t)n_calls + 1) * 4 +
	                    (size_t)n_calls * 12 + (size_t)nt * 56 + 10 * 128 + tch3_follow_scratch_bytes(nt)))) return r;
	if (h_state0) {
		Stage s0(st, &arena);
		d_state = const_cast<gmr1_hip_tch3_state *>(s0.in(h_state0, (size_t)n_calls));
		if ((r = s0.err())) return r;
	}
	const size_t arena_kept = arena.off;
	std::vector<int32_t> first((size_t)n_calls + 1), a_call, a_p;
	std::vector<float> a_en;
	std::vector<int> item;                       // of each frame handed in
	std::vector<uint64_t> t_off;
	std::vector<float> t_fs;
	std::vector<uint32_t> t_fn;
	std::vector<gmr1_hip_tch3_frame> got;
	for (size_t g = 0; g < n_gen; g++) {
		item.clear(); t_off.clear(); t_fs.clear(); t_fn.clear();
		a_call.clear(); a_p.clear(); a_en.clear();
		for (int q = 0; q < n_calls; q++) {
			const RxChain &c = chains[calls[q]];
			first[q] = (int32_t)item.size();
			if (g > c.events.size())
				continue;
			// rx_tch3_init.  An assignment none of whose frames fits hands no frame in, and the next one's follows it on
			// the same state: every assignment is applied, in the order the reference applies them
			if (g > 0) {
				a_call.push_back(q);
				a_p.push_back(c.events[g - 1].p);
				a_en.push_back(c.events[g - 1].ref_energy);
			}
			for (size_t &k = next[q]; k < titems.size() && titems[k].call == q && titems[k].gen == (int)g; k++) {
				const FrameCtx &x = c.log[titems[k].frame];
				item.push_back((int)k);
				t_off.push_back(c.base + (uint64_t)rx_tch3_begin(x.align, sps, titems[k].tn));
				t_fs.push_back(-x.freq_err);
				t_fn.push_back((uint32_t)x.fn);
			}
		}
		const int n = (int)item.size(), n_assign = (int)a_call.size();
		first[n_calls] = n;
		if (!n && !n_assign)
			continue;
		got.resize((size_t)n);
		arena.off = arena_kept;                   // the invocation before is through (fetch)
		Stage sg(st, &arena);
		if (n_assign) {
			const int32_t *d_call = sg.in(a_call.data(), (size_t)n_assign), *d_p = sg.in(a_p.data(), (size_t)n_assign);
			const float *d_en = sg.in(a_en.data(), (size_t)n_assign);
			if ((r = sg.err())) return r;
			if ((r = gmr1_hip_tch3_state_assign_batch_dev(st, n_assign, d_call, d_p, d_en, d_state))) return r;
		}
		if (n) {
			const int32_t *d_first = sg.in(first.data(), first.size());
			const uint64_t *d_off = sg.in(t_off.data(), (size_t)n);
			const float *d_fs = sg.in(t_fs.data(), (size_t)n);
			const uint32_t *d_fn = sg.in(t_fn.data(), (size_t)n);
			gmr1_hip_tch3_frame *d_got = sg.out(got.data(), (size_t)n);
			unsigned char *scratch = sg.dev<unsigned char>(tch3_follow_scratch_bytes(n));
			if ((r = sg.err())) return r;
			r = tch3_follow_enqueue(st, scratch, n_calls, sps, t_in_len, tch, d_first, n, d_off, d_fs, d_fn, d_state, d_got);
			if (r) return r;
		}
		if ((r = sg.fetch())) return r;           // (also ahead of the next invocation's staging: the vectors are reused)

		// records, chain by chain in frame order
		for (int k = 0; k < n; k++) {
			const gmr1_hip_tch3_frame &fr = got[k];
			if (!fr.type)
				continue;
			const TchItem &ti = titems[item[k]];
			RxChain &c = chains[calls[ti.call]];
			touched[ti.call] = 1;
			emit(c, arfcn ? arfcn[c.a] : (uint16_t)c.a, fr.type, (int)fr.fn, ti.tn, fr.l2, fr.conv, ti.frame, fr.len);
			// ASSIGNMENT COMMAND 1 on the FACCH3 starts the TCH9 follow-up (gmr1_rx.c:248-258, 436-442)
			const uint8_t *m = fr.l2;
			if (want9 && fr.type == 0x12 /* GSMTAP_GMR1_TCH3 | GSMTAP_GMR1_FACCH */ && m[3] == 0x06 && m[4] == 0x2e)
				c.events9.push_back({ti.frame, ((m[5] & 0x03) << 3) | (m[6] >> 5), 0, 0.f});
		}
	}

	for (int q = 0; q < n_calls; q++) {
		RxChain &c = chains[calls[q]];
		if (carry && !c.events.empty())
			carry[q] = {c.events.back().tn, true};
		if (!touched[q])
			continue;
		// frame order within each chain: BCCH / CCCH of a frame come before its TCH records
		std::vector<size_t> order(c.rec.size());
		for (size_t i = 0; i < order.size(); i++) order[i] = i;
		std::stable_sort(order.begin(), order.end(),
		                 [&](size_t x, size_t y) { return c.rec_frame[x] < c.rec_frame[y]; });
		std::vector<gmr1_hip_rx_record> sorted(c.rec.size());
		for (size_t i = 0; i < order.size(); i++) sorted[i] = c.rec[order[i]];
		c.rec.swap(sorted);
	}
	return 0;
}

int RxRun::tch3_pass()
{
	// every chain with an IMMEDIATE ASSIGNMENT is one call of tch3_follow_chains
	if (!tch)
		return 0;
	std::vector<int> calls;
	for (size_t ci = 0; ci < chains.size(); ci++)
		if (!chains[ci].events.empty())
			calls.push_back((int)ci);
	if (calls.empty())
		return 0;
	// the calls' states: no call, not ciphered, the carrier's key (ciphering outlives a re-assignment, gmr1_rx.c:358-376)
	std::vector<gmr1_hip_tch3_state> state(calls.size());
	std::memset(state.data(), 0, state.size() * sizeof(state[0]));
	if (kc)
		for (size_t q = 0; q < calls.size(); q++)
			std::memcpy(state[q].kc, kc + (size_t)chains[calls[q]].a * 8, 8);
	return r = tch3_follow_chains(st, sps, tch, arfcn, csd != nullptr, false, chains, calls, state.data(), nullptr, nullptr);
}

int RxRun::tch9_pass()
{
	// ---- TCH9 follow-up (rx_tch9, gmr1_rx.c:262-353) ----------------------------------------------
	// From the frame of a chain's first ASSIGNMENT COMMAND 1 on, every frame's NT9 burst on the assigned
	// timeslot of the CSD carrier: demodulate (sync sequence 0 = FACCH9, 1 = TCH9), decipher with A5/1 of the
	// frame number, decode.  Nothing feeds back, so it is one more batched pass: one demodulation launch, one
	// keystream launch, one FACCH9 launch, one TCH9 launch per interleaver run (a run starts at every
	// assignment; gmr1_deinterleave_inter only advances on TCH9 bursts).
	if (csd) {
		struct Nt9Item { int chain_idx, frame, tn; };
		std::vector<Nt9Item> items9;
		const int win9 = sps + (sps / 2), in_len9 = 351 * sps + win9, etoa9 = win9 >> 1;
		for (size_t ci = 0; ci < chains.size(); ci++) {
			RxChain &c = chains[ci];
			if (c.events9.empty())
				continue;
			size_t ev = 0;
			for (int f = c.events9[0].frame; f < (int)c.log.size(); f++) {
				while (ev + 1 < c.events9.size() && c.events9[ev + 1].frame <= f)
					ev++;
				const int tn = c.events9[ev].tn;
				const int64_t begin = (int64_t)c.log[f].align + sps * tn * 39 - etoa9;
				if (begin < 0 || begin + in_len9 > c.len)
					continue;
				items9.push_back({(int)ci, f, tn});
			}
		}
		const int n9 = (int)items9.size();
		if (n9) {
			// demodulation 682 B per frame, keystreams and decodes at most 662 + 8 + 4 + 658 + 64 B per frame
			Arena arena;
			if ((r = arena.init((size_t)n9 * 2300 + 64 * 1024))) return r;
			Stage sg(st, &arena);
			std::vector<uint64_t> off9(n9);
			std::vector<float> fs9(n9);
			for (int k = 0; k < n9; k++) {
				const RxChain &c = chains[items9[k].chain_idx];
				const FrameCtx &x = c.log[items9[k].frame];
				off9[k] = c.base + (uint64_t)((int64_t)x.align + sps * items9[k].tn * 39 - etoa9);
				fs9[k] = -x.freq_err;
			}
			std::vector<int8_t> h_eb((size_t)n9 * 662);
			std::vector<int32_t> h_sid(n9), h_rv(n9);
			const uint64_t *d_o = sg.in(off9.data(), (size_t)n9);
			const float *d_f = sg.in(fs9.data(), (size_t)n9);
			int8_t *d_eb = sg.out(h_eb.data(), (size_t)n9 * 662);
			int32_t *d_sid = sg.out(h_sid.data(), (size_t)n9);
			int32_t *d_rv = sg.out(h_rv.data(), (size_t)n9);
			if ((r = sg.err())) return r;
			r = demod_dev_energy(st, GMR1_HIP_NT9, n9, sps, in_len9, csd, d_o, d_f, d_eb, 662, d_sid, nullptr, nullptr, d_rv);
			if (r) return r;
			if ((r = sg.fetch())) return r;
			// classify; TCH9 bursts are laid out run after run (one run per interleaver life)
			std::vector<int> fj, tj;                 // item indices: FACCH9 jobs, TCH9 jobs (run-major)
			std::vector<int> run_len;
			{
				int k = 0;
				while (k < n9) {
					const int ci = items9[k].chain_idx;
					const RxChain &c = chains[ci];
					size_t ev = 0;
					int cur = 0;
					bool open = false;
					for (; k < n9 && items9[k].chain_idx == ci; k++) {
						// a (re-)assignment at or before this frame restarts the interleaver (rx_tch9_init)
						bool restart = !open;
						while (ev < c.events9.size() && c.events9[ev].frame <= items9[k].frame) { ev++; restart = true; }
						if (restart) {
							if (open && cur) run_len.push_back(cur);
							cur = 0;
							open = true;
						}
						if (h_rv[k])
							continue;                    // decision D8: a failed demodulation is no burst
						if (h_sid[k] == 0)
							fj.push_back(k);
						else {
							tj.push_back(k);
							cur++;
						}
					}
					if (cur) run_len.push_back(cur);
				}
			}
			const int nf = (int)fj.size(), nt9 = (int)tj.size(), nj = nf + nt9;
			if (nj) {
				std::vector<int8_t> eb((size_t)nj * 662);
				std::vector<uint8_t> keys((size_t)nj * 8, 0);
				std::vector<uint32_t> fns(nj);
				for (int i = 0; i < nj; i++) {
					const int k = i < nf ? fj[i] : tj[i - nf];
					const RxChain &c = chains[items9[k].chain_idx];
					std::memcpy(&eb[(size_t)i * 662], &h_eb[(size_t)k * 662], 662);
					if (kc) std::memcpy(&keys[(size_t)i * 8], kc + (size_t)c.a * 8, 8);
					fns[i] = (uint32_t)c.log[items9[k].frame].fn;
				}
				std::vector<uint8_t> l2f((size_t)nf * 38), l2t((size_t)nt9 * 60);
				std::vector<int32_t> crcf(nf), cvf(nf), cvt(nt9);
				const int8_t *d_e2 = sg.in(eb.data(), eb.size());
				const uint8_t *d_k = sg.in(keys.data(), keys.size());
				const uint32_t *d_fn = sg.in(fns.data(), (size_t)nj);
				uint8_t *d_ks = sg.dev<uint8_t>((size_t)nj * 658);
				uint8_t *d_l2f = sg.dev<uint8_t>((size_t)nf * 38), *d_l2t = sg.dev<uint8_t>((size_t)nt9 * 60);
				int32_t *d_crc = sg.dev<int32_t>((size_t)nf), *d_cvf = sg.dev<int32_t>((size_t)nf), *d_cvt = sg.dev<int32_t>((size_t)nt9);
				if ((r = sg.err())) return r;
				r = gmr1_hip_a5_batch_dev(st, nj, 1, 658, d_k, d_fn, d_ks, nullptr);
				if (r) return r;
				if (nf) {
					r = gmr1_hip_facch9_decode_batch_dev(st, nf, d_e2, d_ks, d_l2f, nullptr, nullptr, d_crc, d_cvf);
					if (r) return r;
					sg.back(l2f.data(), d_l2f, l2f.size());
					sg.back(crcf.data(), d_crc, (size_t)nf);
					sg.back(cvf.data(), d_cvf, (size_t)nf);
					sg.queue_backs();
				}
				std::vector<int32_t> pos((size_t)nt9);       // lives until the synchronisation below
				if (nt9) {
					// all runs in one launch: every burst knows its position in its own run
					size_t i = 0;
					for (int len_run : run_len)
						for (int q = 0; q < len_run; q++)
							pos[i++] = q;
					const int32_t *d_pos = sg.in(pos.data(), (size_t)nt9);
					if ((r = sg.err())) return r;
					r = tch9_runs_dev_impl(st, 2 /* GMR1_TCH9_9k6, gmr1_rx.c:333 */, nt9, d_pos, d_e2 + (size_t)nf * 662,
					                       d_ks + (size_t)nf * 658, d_l2t, d_cvt);
					if (r) return r;
					sg.back(l2t.data(), d_l2t, l2t.size());
					sg.back(cvt.data(), d_cvt, (size_t)nt9);
				}
				if ((r = sg.fetch())) return r;
				// records in frame order per chain: merge the two job lists by item index
				int a9 = 0, b9 = 0;
				while (a9 < nf || b9 < nt9) {
					const bool take_f = b9 >= nt9 || (a9 < nf && fj[a9] < tj[b9]);
					const int k = take_f ? fj[a9] : tj[b9];
					RxChain &c = chains[items9[k].chain_idx];
					gmr1_hip_rx_big_record rec;
					std::memset(&rec, 0, sizeof(rec));
					rec.arfcn = arfcn ? arfcn[c.a] : (uint16_t)c.a;
					rec.chain = (uint8_t)c.chain;
					rec.fn = (uint32_t)c.log[items9[k].frame].fn;
					rec.tn = (uint8_t)items9[k].tn;
					if (take_f) {
						if (!crcf[a9]) {
							rec.type = 0x1a;     // GSMTAP_GMR1_TCH9 | GSMTAP_GMR1_FACCH
							rec.len = 38;
							rec.conv = cvf[a9];
							std::memcpy(rec.l2, &l2f[(size_t)a9 * 38], 38);
							c.big.push_back(rec);
						}
						a9++;
					} else {
						rec.type = 0x18;         // GSMTAP_GMR1_TCH9 (no CRC to check, gmr1_rx.c:336-339)
						rec.len = 60;
						rec.conv = cvt[b9];
						std::memcpy(rec.l2, &l2t[(size_t)b9 * 60], 60);
						c.big.push_back(rec);
						b9++;
					}
				}
			}
		}
	}

	return 0;
}

// gmr1_hip_rx_run_full_dev, plus (optional) how many of the records each carrier contributed
int rx_run_full_impl(void *stream_, int n_arfcn, int sps, const float *iq, const float *tch,
                     const float *csd, const uint64_t *offset, const uint64_t *length,
                     const uint16_t *arfcn, const uint8_t *kc,
                     struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                     struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                     int32_t *status, int32_t *n_chains, int32_t *rec_per_carrier)
{
	hipStream_t st = (hipStream_t)stream_;
	if (n_records) *n_records = 0;
	if (n_big) *n_big = 0;
	if (csd && (!tch || !n_big || max_big < 0 || (max_big > 0 && !big_out)))
		return fail(-EINVAL, "rx_run: the CSD carrier needs the traffic carrier and the big-record outputs");
	if (n_arfcn < 0 || !iq || !offset || !length || !n_records || (max_records > 0 && !out) || max_records < 0)
		return fail(-EINVAL, "rx_run: iq/offset/length/n_records (and out when max_records > 0) are required");
	if (sps < 1 || sps > 16)                  // gmr1_rx.c:919-922
		return fail(-EINVAL, "rx_run: sps=%d unsupported (1..16)", sps);
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_arfcn == 0) return 0;
	// the whole call holds the device's workspace, the loop's side stream and its events: calls from other threads wait
	WsLease lease;
	if ((r = lease.acquire(ds, st))) return r;
	for (int i = 0; i < n_arfcn; i++)
		if (length[i] > 0x7fffffffull)
			return fail(-EINVAL, "rx_run: carrier %d longer than 2^31-1 samples", i);

	RxRun run;
	run.st = st; run.sps = sps; run.iq = iq; run.tch = tch; run.csd = csd;
	run.offset = offset; run.length = length; run.arfcn = arfcn; run.kc = kc;
	run.A = n_arfcn;
	run.out = out; run.max_records = max_records;
	run.stat.assign(n_arfcn, 0); run.nch.assign(n_arfcn, 0);
	// GMR1_HIP_RX_TIMING=1: wall time of the phases on stderr (profiling only)
	static const bool timing = profile_env("GMR1_HIP_RX_TIMING") != nullptr;
	auto now = [] { return std::chrono::steady_clock::now(); };
	const auto t0 = now();
	if ((r = run.acquire())) return r;
	const auto t1 = now();
	if ((r = run.frame_loop())) return r;
	const auto t2 = now();
	if (tch && (r = run.tch3_pass())) return r;
	if (csd && (r = run.tch9_pass())) return r;
	{
		auto us = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3; };
		const double chain = run.t_chain_us > 0 ? run.t_chain_us : run.t_loop_gpu_us;
		t_last_timing[0] = us(t0, t1);                              // FCCH acquisition incl. the chains set up from its result
		t_last_timing[1] = chain;                                   // frame loop: launches until its kernels are through
		t_last_timing[2] = run.t_loop_gpu_us - chain;               // records to the caller's buffer
		t_last_timing[3] = us(t1, t2) - run.t_loop_gpu_us;          // host work around the loop (chains set up, states read)
		t_last_timing[4] = us(t2, now());                           // traffic-channel passes
	}
	if (timing) {
		auto us = [](auto a, auto b) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3; };
		fprintf(stderr, "rx_run: acquire %.0f us, frame loop %.0f us (launch+copy %.0f, collect %.0f), traffic passes %.0f us\n",
		        us(t0, t1), us(t1, t2), run.t_loop_gpu_us, us(t1, t2) - run.t_loop_gpu_us, us(t2, now()));
	}
	const std::vector<RxChain> &chains = run.chains;
	const std::vector<int32_t> &stat = run.stat, &nch = run.nch;
	const int A = n_arfcn;

	// ---- hand back: carriers in order, chains in order, frames in order -------------------------
	int total = 0;
	if (run.direct) {
		total = run.direct_total;            // already in the caller's buffer, in this very order (k_rx_pack)
	} else {
		for (const RxChain &c : chains) {       // chains were created carrier by carrier, chain by chain
			const int cnt = (int)c.rec.size();
			const int fit = std::max(0, std::min(cnt, max_records - total));
			if (fit)
				std::memcpy(out + total, c.rec.data(), (size_t)fit * sizeof(gmr1_hip_rx_record));
			total += cnt;
		}
	}
	*n_records = total;
	if (n_big) {
		int tb = 0;
		for (const RxChain &c : chains)
			for (const gmr1_hip_rx_big_record &rec : c.big) {
				if (tb < max_big)
					big_out[tb] = rec;
				tb++;
			}
		*n_big = tb;
	}
	for (int i = 0; i < A; i++) {
		if (status) status[i] = stat[i];
		if (n_chains) n_chains[i] = nch[i];
		if (rec_per_carrier) rec_per_carrier[i] = 0;
	}
	if (rec_per_carrier)
		for (const RxChain &c : chains)
			rec_per_carrier[c.a] += run.direct ? c.n_rec : (int)c.rec.size();
	return 0;
}

}  // namespace

namespace gmr1 {
int rx_run_dev_counted(void *stream, int n_arfcn, int sps, const float *iq, const uint64_t *offset, const uint64_t *length,
                       const uint16_t *arfcn, struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                       int32_t *status, int32_t *n_chains, int32_t *rec_per_carrier)
{
	return rx_run_full_impl(stream, n_arfcn, sps, iq, nullptr, nullptr, offset, length, arfcn, nullptr, out, max_records, n_records,
	                        nullptr, 0, nullptr, status, n_chains, rec_per_carrier);
}
}  // namespace gmr1

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
	return rx_run_full_impl(stream_, n_arfcn, sps, iq, tch, csd, offset, length, arfcn, kc, out, max_records, n_records,
	                        big_out, max_big, n_big, status, n_chains, nullptr);
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

int gmr1_hip_rx_run_full(int n_arfcn, int sps, const float *iq, const float *tch, const float *csd, uint64_t iq_len,
                         const uint64_t *offset, const uint64_t *length, const uint16_t *arfcn, const uint8_t *kc,
                         struct gmr1_hip_rx_record *out, int max_records, int *n_records,
                         struct gmr1_hip_rx_big_record *big_out, int max_big, int *n_big,
                         int32_t *status, int32_t *n_chains)
{
	if (n_records) *n_records = 0;
	if (n_big) *n_big = 0;
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_arfcn < 0 || !iq || !offset || !length)
		return fail(-EINVAL, "rx_run: iq/offset/length are required");
	for (int i = 0; i < n_arfcn; i++)
		if (offset[i] + length[i] > iq_len)
			return fail(-EINVAL, "rx_run: carrier %d runs past the end of iq", i);
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const float *d_tch = sg.in(tch, (size_t)iq_len * 2);
	const float *d_csd = sg.in(csd, (size_t)iq_len * 2);
	if ((r = sg.err())) return r;
	return gmr1_hip_rx_run_full_dev(nullptr, n_arfcn, sps, d_iq, d_tch, d_csd, offset, length, arfcn, kc, out, max_records,
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

// What gmr1_gsmtap_makemsg (reference src/gsmtap.c:43-71) puts on the wire for one decoded frame:
// the 16-byte struct gsmtap_hdr of libosmocore (version 2, hdr_len 4 words, type GMR1_UM = 0x0a,
// timeslot, arfcn BE16, signal_dbm, snr_db, frame_number BE32, sub_type, antenna_nr, sub_slot, res)
// followed by the L2 bytes.  The reference leaves the arfcn field 0; with_arfcn != 0 fills it.
// Host-only byte packing (the I/O sink itself -- the UDP socket -- stays with the caller).
static int gsmtap_pack_any(uint16_t arfcn, uint8_t type, uint32_t fn, uint8_t tn, const uint8_t *l2, int len,
                           int max_len, int with_arfcn, uint8_t *buf, int buf_len)
{
	const int total = 16 + len;
	if (len > max_len || buf_len < total)
		return fail(-EINVAL, "gsmtap_pack: need %d bytes, have %d", total, buf_len);
	std::memset(buf, 0, 16);
	buf[0] = 2;                       // GSMTAP_VERSION
	buf[1] = 4;                       // sizeof(struct gsmtap_hdr) / 4
	buf[2] = 0x0a;                    // GSMTAP_TYPE_GMR1_UM
	buf[3] = tn;
	if (with_arfcn) {
		buf[4] = (uint8_t)((arfcn >> 8) & 0x3f);     // 14-bit ARFCN, flags clear
		buf[5] = (uint8_t)(arfcn & 0xff);
	}
	buf[8] = (uint8_t)(fn >> 24);                    // htonl(fn)
	buf[9] = (uint8_t)(fn >> 16);
	buf[10] = (uint8_t)(fn >> 8);
	buf[11] = (uint8_t)fn;
	buf[12] = type;                   // GSMTAP_GMR1_BCCH 0x01, CCCH 0x02, TCH3 0x10 (| FACCH 0x02), TCH9 0x18 (| FACCH 0x02)
	std::memcpy(buf + 16, l2, (size_t)len);
	return total;
}

int gmr1_hip_gsmtap_pack(const struct gmr1_hip_rx_record *rec, int with_arfcn, uint8_t *buf, int buf_len)
{
	if (!rec || !buf)
		return fail(-EINVAL, "gsmtap_pack: rec / buf are required");
	return gsmtap_pack_any(rec->arfcn, rec->type, rec->fn, rec->tn, rec->l2, rec->len, 24, with_arfcn, buf, buf_len);
}

int gmr1_hip_gsmtap_pack_big(const struct gmr1_hip_rx_big_record *rec, int with_arfcn, uint8_t *buf, int buf_len)
{
	if (!rec || !buf)
		return fail(-EINVAL, "gsmtap_pack: rec / buf are required");
	return gsmtap_pack_any(rec->arfcn, rec->type, rec->fn, rec->tn, rec->l2, rec->len, 64, with_arfcn, buf, buf_len);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The streaming receive loop (gmr1_hip_rx_stream_*): gmr1_hip_rx_run over a capture pushed piece by piece.
//
// A handle holds, per carrier, the samples it still needs in one buffer of a device ping-pong pair, and every chain's
// RxLoopState in device memory.  A push stages [kept tail | new chunk] into the other buffer (k_rx_stage, which also
// rebases the states), runs the acquisition once enough samples are there (rx_stream_acq_need), then walks every chain
// with the one-shot loop (RxRun::frame_loop) up to the samples available.  A walk only ever processes a frame after
// rx_loop_advance's check `align + 2 * frame_len <= len` admitted it, and every window of such a frame ends before
// align + 2 * frame_len, so a walk to H samples does exactly what the one-shot walk does up to there; the only thing the
// horizon adds is a stop that the next push may lift (rx_stream_next_done).  A carrier then keeps its samples from
// rx_stream_keep_from(min chain align): no window of the next walk starts before that (rx_stream_reach_back).
//
// A handle made by gmr1_hip_rx_stream_create_tch also follows TCH3 calls (gmr1_hip_rx_run_tch over pushes).  It holds the
// traffic carrier's samples in a second ping-pong pair with the first one's stride, held and keep (k_rx_stage_copy), one
// struct gmr1_hip_tch3_state per chain in device memory and, on the host, each chain's assigned timeslot.  A push walks the
// chains with the frame log on, then hands this push's frames to tch3_follow_chains -- the one-shot pass's own rule for
// frames, assignments and windows -- on those states: the call a push leaves is the call the next one continues.  The
// traffic windows of admitted frames fit the samples held for the same reason the walk's own do.
// ---------------------------------------------------------------------------------------------------------------------
static_assert(kStartDiscard == kRxStartDiscard && kStartDiscard == kAcqStart, "one start discard");

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
	std::vector<int> c0;                 // per carrier: its first chain (A + 1 entries)
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
	~gmr1_hip_rx_stream()
	{
		for (float2 *p : buf)
			if (p) (void)hipFree(p);
		for (float2 *p : tbuf)
			if (p) (void)hipFree(p);
		if (d_tstate) (void)hipFree(d_tstate);
		if (d_state) (void)hipFree(d_state);
		if (d_car) (void)hipFree(d_car);
		if (d_err) (void)hipFree(d_err);
		if (d_in) (void)hipFree(d_in);
		if (h_car) (void)hipHostFree(h_car);
		if (h_err) (void)hipHostFree(h_err);
		if (h_in) (void)hipHostFree(h_in);
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

// with_tch: the call is one of gmr1_hip_rx_stream_push_tch*
int rx_stream_check(const gmr1_hip_rx_stream *h, bool with_tch, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                    int last, const gmr1_hip_rx_record *out, int max_records, const int *n_records)
{
	if (!h || !n_records || max_records < 0 || (max_records > 0 && !out) || (n > 0 && !iq))
		return fail(-EINVAL, "rx_stream_push: handle / n_records (and iq when n > 0, out when max_records > 0) are required");
	if (h->tch != with_tch)
		return fail(-EINVAL, h->tch ? "rx_stream_push: a handle of gmr1_hip_rx_stream_create_tch takes gmr1_hip_rx_stream_push_tch*"
		                            : "rx_stream_push_tch: the handle was not made by gmr1_hip_rx_stream_create_tch");
	if (with_tch && n > 0 && !tch)
		return fail(-EINVAL, "rx_stream_push_tch: tch is required when n > 0");
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
	(void)last;
	return 0;
}

// the device part of a push; the caller holds h->mu and the workspace lease, and has validated everything
// (tch: the traffic carrier's chunk, laid out as iq, for a handle that follows TCH3 calls)
int rx_stream_push_impl(hipStream_t st, gmr1_hip_rx_stream *h, const float2 *iq, const float2 *tch, uint64_t iq_stride, uint64_t n,
                        int last, gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	const int A = h->A, sps = h->sps;
	// 1. staging: [kept tail | chunk] -> the other buffer, states rebased
	std::vector<long long> next((size_t)A);
	long long need = 0, max_pairs = 0;
	for (int i = 0; i < A; i++) {
		next[i] = rx_stream_next_held(h, i, n);
		need = std::max(need, next[i]);
	}
	need = (need + kRxKeepAlign - 1) / kRxKeepAlign * kRxKeepAlign;
	float2 *src = h->buf[h->cur], *tsrc = h->tbuf[h->cur];
	const long long src_stride = h->stride;
	const bool grow = need > h->stride;
	// the destination of this staging in a pair (the traffic pair follows the first one's decision)
	auto other = [&](float2 **pair) -> int {
		float2 *&o = pair[1 - h->cur];
		if (grow) {
			// grow-only: a new pair; the old current buffer is the source of this one staging and then goes
			float2 *fresh = nullptr;
			HIP_TRY(hipMalloc(&fresh, (size_t)A * (size_t)need * sizeof(float2)));
			if (o) (void)hipFree(o);
			o = fresh;
		} else if (!o && need > 0) {
			HIP_TRY(hipMalloc(&o, (size_t)A * (size_t)h->stride * sizeof(float2)));
		}
		return 0;
	};
	int r = other(h->buf);
	if (!r && h->tch) r = other(h->tbuf);
	if (r) return r;
	if (grow) h->stride = need;
	float2 *dst = h->buf[1 - h->cur], *tdst = h->tbuf[1 - h->cur];
	for (int i = 0; i < A; i++) {
		RxStageCarrier &c = h->h_car[i];
		const bool dead = rx_stream_dead(h, i);
		c.src = (uint64_t)((long long)i * src_stride + h->keep[i]);
		c.dst = (uint64_t)((long long)i * h->stride);
		c.iq = (long long)i * (long long)iq_stride;
		c.kept = dead ? 0 : (int32_t)(h->held[i] - h->keep[i]);
		c.n_new = dead ? 0 : (int32_t)n;
		c.shift = dead ? 0 : (int32_t)h->keep[i];
		c.c0 = h->c0.empty() ? 0 : h->c0[i];
		c.c1 = h->c0.empty() ? 0 : h->c0[i + 1];
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
		sa.n_carriers = A; sa.sps = sps; sa.last = last ? 1 : 0;
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
	}
	if (grow && (src || tsrc)) {
		HIP_TRY(hipStreamSynchronize(st));     // the staging has read the old buffers
		if (src) (void)hipFree(src);
		if (tsrc) (void)hipFree(tsrc);
		h->buf[h->cur] = nullptr;
		h->tbuf[h->cur] = nullptr;
	}
	h->cur = 1 - h->cur;
	for (int i = 0; i < A; i++) {
		const bool dead = rx_stream_dead(h, i);
		if (!dead) {
			for (int k = h->c0.empty() ? 0 : h->c0[i]; k < (h->c0.empty() ? 0 : h->c0[i + 1]); k++)
				h->chains[k].align -= (int)h->keep[i];
		}
		h->held[i] = next[i];
		h->keep[i] = 0;
	}
	h->N += n;
	if (last) h->ended = true;

	RxRun run;
	run.st = st; run.sps = sps; run.iq = reinterpret_cast<const float *>(h->buf[h->cur]);
	// (a traffic carrier makes the walk log its frames and hand its records back chain by chain, as in gmr1_hip_rx_run_tch)
	run.tch = h->tch ? reinterpret_cast<const float *>(h->tbuf[h->cur]) : nullptr;
	run.csd = nullptr; run.kc = nullptr;
	run.arfcn = h->arfcn.empty() ? nullptr : h->arfcn.data();
	run.A = A;
	run.out = out; run.max_records = max_records;
	run.stat = h->stat; run.nch = h->nch;
	std::vector<uint64_t> offset((size_t)A), length((size_t)A);
	for (int i = 0; i < A; i++) {
		offset[i] = (uint64_t)((long long)i * h->stride);
		length[i] = (uint64_t)h->held[i];
	}
	run.offset = offset.data(); run.length = length.data();
	std::vector<gmr1_hip_tch3_state> t0;     // the calls' first states: lives until this push's synchronisation

	// 2. the acquisition, once every carrier holds what it reads (nothing has been dropped yet: coordinates are absolute)
	if (!h->acquired && ((long long)h->N >= rx_stream_acq_need(sps) || last)) {
		if ((r = run.acquire())) return r;
		h->stat = run.stat; h->nch = run.nch;
		h->acq_stat = run.stat;
		h->chains = std::move(run.chains);
		run.chains.clear();
		h->c0.assign((size_t)A + 1, 0);
		for (const RxChain &c : h->chains)
			h->c0[c.a + 1]++;
		for (int i = 0; i < A; i++)
			h->c0[i + 1] += h->c0[i];
		const int nc = (int)h->chains.size();
		if (nc) {
			HIP_TRY(hipMalloc(&h->d_state, (size_t)nc * sizeof(RxLoopState)));
			std::vector<RxLoopState> s0((size_t)nc);
			for (int k = 0; k < nc; k++) {
				const RxChain &c = h->chains[k];
				s0[k] = {c.base, c.len, c.align, c.freq_err, c.fn, c.delay, c.stn, kRxDoneUnstarted, c.bcch_energy,
				         (uint16_t)(run.arfcn ? run.arfcn[c.a] : (uint16_t)c.a), (uint16_t)c.chain};
				s0[k].done = rx_stream_next_done(kRxDoneUnstarted, c.align, c.len, sps, last);
			}
			HIP_TRY(hipMemcpyAsync(h->d_state, s0.data(), (size_t)nc * sizeof(RxLoopState), hipMemcpyHostToDevice, st));
			if (h->tch) {
				// the chains' calls: none yet, not ciphered, the carrier's key (RxRun::tch3_pass)
				t0.resize((size_t)nc);
				std::memset(t0.data(), 0, t0.size() * sizeof(t0[0]));
				if (!h->kc.empty())
					for (int k = 0; k < nc; k++)
						std::memcpy(t0[k].kc, &h->kc[(size_t)h->chains[k].a * 8], 8);
				HIP_TRY(hipMalloc(&h->d_tstate, (size_t)nc * sizeof(gmr1_hip_tch3_state)));
				HIP_TRY(hipMemcpyAsync(h->d_tstate, t0.data(), (size_t)nc * sizeof(gmr1_hip_tch3_state), hipMemcpyHostToDevice, st));
				h->carry.assign((size_t)nc, TchCarry());
			}
		}
		h->acquired = true;
	}

	// 3. the walk up to the samples available
	if (h->acquired && !h->chains.empty()) {
		run.chains = std::move(h->chains);
		for (RxChain &c : run.chains) {
			c.base = offset[c.a];
			c.len = (int)h->held[c.a];
		}
		run.loop_state = h->d_state;
		r = run.frame_loop();
		h->chains = std::move(run.chains);
		if (r) return r;
		h->stat = run.stat;
		for (int k = 0; k < (int)h->chains.size(); k++)
			if (h->chains[k].outgrew) {
				// stopped for good, as in the one-shot call
				static const int32_t fin = kRxDoneFinal;
				HIP_TRY(hipMemcpyAsync(&h->d_state[k].done, &fin, 4, hipMemcpyHostToDevice, st));
			}
	}
	HIP_TRY(hipMemcpyAsync(h->h_err, h->d_err, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (*h->h_err) {
		h->broken = true;
		return fail(-EIO, "rx_stream_push: a chain could reach before its carrier's kept samples");
	}
	*n_records = run.direct ? run.direct_total : 0;

	// 3b. the TCH3 follow-up over this push's frames, and the records chain by chain in frame order
	if (h->tch && h->acquired && !h->chains.empty()) {
		std::vector<int> calls(h->chains.size());
		for (size_t k = 0; k < calls.size(); k++)
			calls[k] = (int)k;
		if ((r = tch3_follow_chains(st, sps, run.tch, run.arfcn, false, !last, h->chains, calls, nullptr, h->d_tstate,
		                            h->carry.data()))) return r;
		int total = 0;
		for (RxChain &c : h->chains) {
			const int cnt = (int)c.rec.size();
			const int fit = std::max(0, std::min(cnt, max_records - total));
			if (fit)
				std::memcpy(out + total, c.rec.data(), (size_t)fit * sizeof(gmr1_hip_rx_record));
			total += cnt;
			c.rec.clear(); c.rec_frame.clear(); c.log.clear(); c.events.clear();     // the next push's walk starts them over
		}
		*n_records = total;
	}

	// 4. what each carrier keeps for the next push
	for (int i = 0; i < A; i++) {
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
		h->keep[i] = std::min(h->held[i], rx_stream_keep_from(lo, sps));
	}
	return 0;
}

// gmr1_hip_rx_stream_push_dev and _push_tch_dev (tch_entry)
int rx_stream_push_dev_any(void *stream, gmr1_hip_rx_stream *h, bool tch_entry, const float *iq, const float *tch, uint64_t iq_stride,
                           uint64_t n, int last, gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_records) *n_records = 0;
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	if ((r = rx_stream_check(h, tch_entry, iq, tch, iq_stride, n, last, out, max_records, n_records)))
		return r;
	hipStream_t st = (hipStream_t)stream;
	// the loop holds the device's workspace, side stream and events: pushes of other handles wait their turn
	WsLease lease;
	if ((r = lease.acquire(ds, st))) return r;
	r = rx_stream_push_impl(st, h, reinterpret_cast<const float2 *>(iq), reinterpret_cast<const float2 *>(tch), iq_stride, n, last,
	                        out, max_records, n_records);
	if (r) h->broken = true;
	return r;
}

// gmr1_hip_rx_stream_push and _push_tch (tch_entry)
int rx_stream_push_host_any(gmr1_hip_rx_stream *h, bool tch_entry, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                            int last, gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	DevState *ds;
	int r = dev_state(&ds);
	if (r) return r;
	if (n_records) *n_records = 0;
	std::unique_lock<std::mutex> lk;
	if (h)
		lk = std::unique_lock<std::mutex>(h->mu);
	if ((r = rx_stream_check(h, tch_entry, iq, tch, iq_stride, n, last, out, max_records, n_records)))
		return r;
	// the chunk goes up packed (stride n) through the handle's pinned block, the traffic carrier's behind it
	const size_t half = (size_t)h->A * (size_t)n * sizeof(float2), bytes = tch_entry ? 2 * half : half;
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
		if (tch_entry)
			std::memcpy(h->h_in + half / 4 + (size_t)i * n * 2, tch + (size_t)i * iq_stride * 2, (size_t)n * sizeof(float2));
	}
	WsLease lease;
	if ((r = lease.acquire(ds, nullptr))) return r;
	if (bytes)
		HIP_TRY(hipMemcpyAsync(h->d_in, h->h_in, bytes, hipMemcpyHostToDevice, nullptr));
	r = rx_stream_push_impl(nullptr, h, reinterpret_cast<const float2 *>(h->d_in),
	                        tch_entry ? reinterpret_cast<const float2 *>(h->d_in + half / 4) : nullptr, n, n, last, out, max_records,
	                        n_records);
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

// kc: the handle follows TCH3 calls (tch); n_arfcn x 8 key bytes, or NULL for the all-zero key
int rx_stream_make(int n_arfcn, int sps, const uint16_t *arfcn, bool tch, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	std::unique_ptr<gmr1_hip_rx_stream> h(new gmr1_hip_rx_stream);
	HIP_TRY(hipGetDevice(&h->device));
	h->A = n_arfcn;
	h->sps = sps;
	h->tch = tch;
	if (arfcn)
		h->arfcn.assign(arfcn, arfcn + n_arfcn);
	if (kc)
		h->kc.assign(kc, kc + (size_t)n_arfcn * 8);
	h->stat.assign(n_arfcn, 0);
	h->nch.assign(n_arfcn, 0);
	h->held.assign(n_arfcn, 0);
	h->keep.assign(n_arfcn, 0);
	h->rebased.assign(n_arfcn, 0);
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
	return rx_stream_make(n_arfcn, sps, arfcn, false, nullptr, out);
}

int gmr1_hip_rx_stream_create_tch(int n_arfcn, int sps, const uint16_t *arfcn, const uint8_t *kc, struct gmr1_hip_rx_stream **out)
{
	int r = rx_stream_create_check("rx_stream_create_tch", n_arfcn, sps, out);
	if (r) return r;
	DevState *ds;
	if ((r = dev_state(&ds))) return r;
	return rx_stream_make(n_arfcn, sps, arfcn, true, kc, out);
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
	return rx_stream_push_dev_any(stream, h, false, iq, nullptr, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push(struct gmr1_hip_rx_stream *h, const float *iq, uint64_t iq_stride, uint64_t n, int last,
                            struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_host_any(h, false, iq, nullptr, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_tch_dev(void *stream, struct gmr1_hip_rx_stream *h, const float *iq, const float *tch,
                                    uint64_t iq_stride, uint64_t n, int last, struct gmr1_hip_rx_record *out, int max_records,
                                    int *n_records)
{
	return rx_stream_push_dev_any(stream, h, true, iq, tch, iq_stride, n, last, out, max_records, n_records);
}

int gmr1_hip_rx_stream_push_tch(struct gmr1_hip_rx_stream *h, const float *iq, const float *tch, uint64_t iq_stride, uint64_t n,
                                int last, struct gmr1_hip_rx_record *out, int max_records, int *n_records)
{
	return rx_stream_push_host_any(h, true, iq, tch, iq_stride, n, last, out, max_records, n_records);
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
