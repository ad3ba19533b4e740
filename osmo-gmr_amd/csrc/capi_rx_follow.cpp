// capi_rx_follow.cpp -- the traffic follow-ups of the receive loop (capi_rx.cpp, capi_rx_stream.cpp).  The traffic channels
// never feed back into the BCCH / CCCH loop, so they run after it as batched passes over chains and the walks the loop made
// of them: tch3_follow_chains hands every chain with an IMMEDIATE ASSIGNMENT to the batched call follower, one invocation
// per assignment a chain sees (a push of the streaming loop runs it over its own frames too); tch9_follow_chains
// demodulates, classifies on the host and decodes; tch9_follow_push is the TCH9 follow-up of one push of the streaming
// loop, through the batched TCH9 call follower with every state and frame left on the device.  Which frame belongs to which assignment, invocation and interleaver
// run is integer work: rx_follow.h.

#include "rx_run.h"
#include "tch3_audio.h"

using namespace gmr1;

namespace {

// a frame the follower reported: its TCH3 record, and the TCH9 assignment it may carry
void emit(RxWalk &w, const uint16_t *arfcn, const RxChain &c, const Tch3Item &ti, const gmr1_hip_tch3_frame &fr, bool want9)
{
	gmr1_hip_rx_record r;
	std::memset(&r, 0, sizeof(r));
	r.arfcn = rx_label(arfcn, c.a);
	r.chain = (uint8_t)c.chain;
	r.type = fr.type;
	r.fn = fr.fn;
	r.tn = (uint8_t)ti.tn;
	r.len = fr.len;
	r.conv = fr.conv;
	std::memcpy(r.l2, fr.l2, fr.len);
	w.rec.push_back(r);
	w.rec_frame.push_back(ti.frame);
	// ASSIGNMENT COMMAND 1 on the FACCH3 starts the TCH9 follow-up (gmr1_rx.c:248-258, 436-442)
	const uint8_t *m = fr.l2;
	if (want9 && fr.type == 0x12 /* GSMTAP_GMR1_TCH3 | GSMTAP_GMR1_FACCH */ && m[3] == 0x06 && m[4] == 0x2e)
		w.events9.push_back({ti.frame, ((m[5] & 0x03) << 3) | (m[6] >> 5), 0, 0.f});
}

// What one invocation of the call follower takes: the assignments applied before it, and the frames handed in call by call
struct Tch3Batch {
	std::vector<int32_t> first, a_call, a_p;
	std::vector<float> a_en, t_fs;
	std::vector<int> item;                       // of each frame handed in: its index in the plan
	std::vector<uint64_t> t_off;
	std::vector<uint32_t> t_fn;
	std::vector<gmr1_hip_tch3_frame> got;
	// with audio: the calls' labels going in; coming back, the blocks in front of each call and, last, their number
	std::vector<uint64_t> label;
	std::vector<int32_t> call_base;
	gmr1_hip_rx_audio *d_audio = nullptr;        // the blocks, in the pass's arena until the next invocation
};

// one invocation: staged, rx_tch3_init on the states where they lie, the follower, b.got on the host (one synchronisation,
// which also comes ahead of the next invocation's staging: the vectors are reused).  d_codec: the calls' decoders, for a
// pass that gives audio -- made fresh for the very calls rx_tch3_init runs on, then run over the frames where they lie;
// the block counts come back with b.got.  On a measuring arena it stages (nothing) and launches nothing.
int tch3_invoke(hipStream_t st, Arena &arena, int n_calls, int sps, const float *tch, gmr1_hip_tch3_state *d_state, Tch3Batch &b,
                void *d_codec)
{
	int r = 0;
	const size_t n = b.item.size(), n_assign = b.a_call.size();
	const bool live = !arena.measures;
	b.got.resize(n);
	Stage sg(st, &arena);
	if (n_assign) {
		const int32_t *d_call = sg.in(b.a_call.data(), n_assign), *d_p = sg.in(b.a_p.data(), n_assign);
		const float *d_en = sg.in(b.a_en.data(), n_assign);
		if ((r = sg.err())) return r;
		if (live && (r = gmr1_hip_tch3_state_assign_batch_dev(st, (int)n_assign, d_call, d_p, d_en, d_state))) return r;
		if (live && d_codec && (r = codec_init_list(st, (int)n_assign, d_call, d_codec, 0))) return r;
	}
	b.d_audio = nullptr;
	b.call_base.assign((size_t)n_calls + 1, 0);
	if (n) {
		const int32_t *d_first = sg.in(b.first.data(), b.first.size());
		const uint64_t *d_off = sg.in(b.t_off.data(), n);
		const float *d_fs = sg.in(b.t_fs.data(), n);
		const uint32_t *d_fn = sg.in(b.t_fn.data(), n);
		gmr1_hip_tch3_frame *d_got = sg.out(b.got.data(), n);
		unsigned char *scratch = sg.dev<unsigned char>(tch3_follow_scratch_bytes((int)n));
		if ((r = sg.err())) return r;
		if (live && (r = tch3_follow_enqueue(st, scratch, n_calls, sps, rx_tch3_in_len(sps), tch, d_first, (int)n, d_off, d_fs, d_fn,
		                                     d_state, d_got))) return r;
		if (d_codec) {
			const uint64_t *d_label = sg.in(b.label.data(), (size_t)n_calls);
			int32_t *d_base = sg.out(b.call_base.data(), (size_t)n_calls + 1);
			b.d_audio = sg.dev<gmr1_hip_rx_audio>(n);
			unsigned char *a_scratch = sg.dev<unsigned char>(tch3_audio_scratch_bytes(n_calls, (int)n));
			if ((r = sg.err())) return r;
			if (live && (r = tch3_audio_enqueue(st, a_scratch, n_calls, d_first, (int)n, d_got, d_fn, d_label, d_codec, b.d_audio,
			                                    (int)n, d_base, d_base + n_calls))) return r;
		}
	}
	return live ? sg.fetch() : 0;
}

// frame order within a chain: BCCH / CCCH of a frame come before its TCH records
void sort_by_frame(RxWalk &w)
{
	std::vector<size_t> order(w.rec.size());
	for (size_t i = 0; i < order.size(); i++) order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return w.rec_frame[x] < w.rec_frame[y]; });
	std::vector<gmr1_hip_rx_record> sorted(w.rec.size());
	for (size_t i = 0; i < order.size(); i++) sorted[i] = w.rec[order[i]];
	w.rec.swap(sorted);
}

}  // namespace

namespace gmr1 {

// ---- TCH3 follow-up (rx_tch3, gmr1_rx.c:355-600) ----------------------------------------------
// All chains at once through the batched call follower (tch3_follow_enqueue, capi_tch3_follow.cpp -- what
// gmr1_hip_tch3_follow_batch_dev runs): chain calls[q] is call q, its state is slot q of a device array.  tch3_plan
// (rx_follow.h) says which frames belong to which assignment and invocation; this function stages them and says where the
// records go -- for the one-shot pass (the whole capture's log; the states start from h_state0 and die with the call) and
// for a push of the streaming loop (this push's log; the states are the handle's d_state, the timeslots its `carry`); the
// per-frame work, the state machine, the decodes and the ciphering state are the follower's, on the device.  rx_tch3_init
// runs between two invocations (k_tch3f_assign, on the states where they lie): a chain that is assigned once -- the usual
// case -- costs one invocation and one synchronisation.
// voice: the pass also gives audio (RxVoice, rx_run.h).  Every invocation then makes the decoders of its assigned calls
// fresh on the device and closes its frames up into audio blocks behind the follower (tch3_invoke); the block counts come
// back with the frames, then the blocks are copied -- straight to the caller where one invocation holds them all (rx_follow.h).
// horizon: a push that is not the last.  Every logged frame was admitted by align + 2 * frame_len <= len, which its TCH3
// window fits, so a window that does not is an error (-EIO), not a frame dropped that the one-shot reads.
int tch3_follow_chains(hipStream_t st, int sps, const float *tch, const uint16_t *arfcn, bool want9, bool horizon,
                       const std::vector<RxChain> &chains, std::vector<RxWalk> &walks, const std::vector<int> &calls,
                       const gmr1_hip_tch3_state *h_state0, gmr1_hip_tch3_state *d_state, TchCarry *carry, RxVoice *voice)
{
	int r = 0;
	const int n_calls = (int)calls.size();
	if (voice)
		voice->found = 0;
	std::vector<Tch3Call> pc((size_t)n_calls);
	for (int q = 0; q < n_calls; q++) {
		const RxWalk &w = walks[calls[q]];
		pc[q] = {&w.log, &w.events, carry && carry[q].assigned, carry ? carry[q].tn : 0, chains[calls[q]].len};
	}
	Tch3Plan plan;
	if (!tch3_plan(pc, sps, horizon, &plan))
		return fail(-EIO, "tch3 follow-up: a frame the walk admitted does not hold its traffic window");
	const std::vector<Tch3Item> &titems = plan.items;
	const int nt = (int)titems.size();
	if (!nt && (h_state0 || !plan.any_event))
		return 0;
	const size_t codec_bytes = gmr1_hip_codec_state_bytes();
	const bool own_codec = voice && !voice->d_codec;
	if (voice && (r = tch3_pcm_prepare())) return r;  // the decoder's tables, before anything is enqueued
	void *d_codec = voice ? voice->d_codec : nullptr;
	// What the pass keeps: the states and the decoders if they start here (no decoder is read before an assignment made it
	// fresh: frames are handed in from a call's first assignment on).  Measuring, the largest invocation comes behind that:
	// none has more than n_calls assignments or nt frames.
	Tch3Batch b;
	b.first.resize((size_t)n_calls + 1); b.a_call.resize((size_t)n_calls); b.item.resize((size_t)nt);
	auto keep = [&](Arena &ar) -> int {
		Stage s0(st, &ar);
		if (h_state0) d_state = const_cast<gmr1_hip_tch3_state *>(s0.in(h_state0, (size_t)n_calls));
		if (own_codec) d_codec = s0.dev<unsigned char>((size_t)n_calls * codec_bytes);
		return ar.measures ? tch3_invoke(st, ar, n_calls, sps, tch, d_state, b, d_codec) : s0.err();
	};
	Arena arena;
	if ((r = arena.sized_by(keep))) return r;
	const size_t arena_kept = arena.off;
	// where the blocks go (rx_follow.h): straight to the caller when one invocation has them all
	const bool direct = voice && tch3_voice_invocations(plan) <= 1;
	struct Kept { std::vector<gmr1_hip_rx_audio> blocks; std::vector<int32_t> call_base; };
	std::vector<Kept> kept;
	std::vector<size_t> next(plan.start.begin(), plan.start.end() - 1);   // per call: its first item no invocation has taken yet
	std::vector<char> touched((size_t)n_calls, 0);
	for (size_t g = 0; g < plan.n_gen; g++) {
		b.item.clear(); b.t_off.clear(); b.t_fs.clear(); b.t_fn.clear();
		b.a_call.clear(); b.a_p.clear(); b.a_en.clear();
		for (int q = 0; q < n_calls; q++) {
			const RxChain &c = chains[calls[q]];
			const RxWalk &w = walks[calls[q]];
			b.first[q] = (int32_t)b.item.size();
			if (g > w.events.size())
				continue;
			// rx_tch3_init.  An assignment none of whose frames fits hands no frame in, and the next one's follows it on
			// the same state: every assignment is applied, in the order the reference applies them
			if (g > 0) {
				b.a_call.push_back(q);
				b.a_p.push_back(w.events[g - 1].p);
				b.a_en.push_back(w.events[g - 1].ref_energy);
			}
			for (size_t &k = next[q]; k < plan.start[q + 1] && titems[k].gen == (int)g; k++) {
				const FrameCtx &x = w.log[titems[k].frame];
				b.item.push_back((int)k);
				b.t_off.push_back(c.base + (uint64_t)rx_tch3_begin(x.align, sps, titems[k].tn));
				b.t_fs.push_back(-x.freq_err);
				b.t_fn.push_back((uint32_t)x.fn);
			}
		}
		b.first[n_calls] = (int32_t)b.item.size();
		if (b.item.empty() && b.a_call.empty())
			continue;
		arena.off = arena_kept;                   // the invocation before is through (fetch)
		if (voice) {
			b.label.assign((size_t)n_calls, 0);
			for (int q = 0; q < n_calls; q++)
				if (b.first[q + 1] > b.first[q]) {
					const RxChain &c = chains[calls[q]];
					b.label[q] = tch3_audio_label(rx_label(arfcn, c.a), (unsigned)c.chain, (unsigned)titems[b.item[b.first[q]]].tn,
					                              (unsigned)tch3_voice_call(voice->count ? voice->count[q] : 0, (int)g));
				}
		}
		if ((r = tch3_invoke(st, arena, n_calls, sps, tch, d_state, b, d_codec))) return r;
		// the invocation's blocks: the count came back with the frames, now exactly that many (one more synchronisation)
		if (voice && b.d_audio) {
			const int count = b.call_base[n_calls];
			gmr1_hip_rx_audio *to = voice->out;
			int fit = std::min(count, voice->max_out);
			if (!direct) {
				kept.push_back({std::vector<gmr1_hip_rx_audio>((size_t)count), b.call_base});
				to = kept.back().blocks.data();
				fit = count;
			}
			voice->found += count;
			if (fit > 0) {
				HIP_TRY(hipMemcpyAsync(to, b.d_audio, (size_t)fit * sizeof(gmr1_hip_rx_audio), hipMemcpyDeviceToHost, st));
				HIP_TRY(hipStreamSynchronize(st));
			}
		}
		// records, chain by chain in frame order
		for (size_t k = 0; k < b.item.size(); k++) {
			const Tch3Item &ti = titems[b.item[k]];
			if (!b.got[k].type)
				continue;
			touched[ti.call] = 1;
			emit(walks[calls[ti.call]], arfcn, chains[calls[ti.call]], ti, b.got[k], want9);
		}
	}

	// blocks of more than one invocation: call by call, and within a call in the invocations' order, which is the frames'
	if (voice && !direct) {
		int total = 0;
		for (int q = 0; q < n_calls; q++)
			for (const Kept &k : kept) {
				const int cnt = k.call_base[q + 1] - k.call_base[q];
				const int fit = std::max(0, std::min(cnt, voice->max_out - total));
				if (fit)
					std::memcpy(voice->out + total, k.blocks.data() + k.call_base[q], (size_t)fit * sizeof(gmr1_hip_rx_audio));
				total += cnt;
			}
	}
	for (int q = 0; q < n_calls; q++) {
		RxWalk &w = walks[calls[q]];
		if (voice && voice->count)
			voice->count[q] = tch3_voice_carry(voice->count[q], w.events.size());
		if (carry && !w.events.empty())
			carry[q] = {w.events.back().tn, true};
		if (touched[q])
			sort_by_frame(w);
	}
	return 0;
}

int RxRun::tch3_pass()
{
	// every chain with an IMMEDIATE ASSIGNMENT is one call of tch3_follow_chains
	if (!tch)
		return 0;
	std::vector<int> calls;
	for (size_t ci = 0; ci < walks.size(); ci++)
		if (!walks[ci].events.empty())
			calls.push_back((int)ci);
	if (calls.empty())
		return 0;
	const std::vector<gmr1_hip_tch3_state> state = tch3_first_states(chains, calls, kc);
	return r = tch3_follow_chains(st, sps, tch, arfcn, csd != nullptr, false, chains, walks, calls, state.data(), nullptr, nullptr, voice);
}

}  // namespace gmr1

namespace {

// The FACCH9 / TCH9 jobs `jobs` of the demodulated items: keystreams, the two decodes, and the big records in frame order
// per chain.  sg is the pass's stage; h_eb: the items' demodulated bits (662 each).  bound: measuring, with no jobs: as many
// jobs in all and of either kind, which no split of the pass's frames into jobs exceeds in any take.
int tch9_decode_jobs(hipStream_t st, Stage &sg, const uint16_t *arfcn, const uint8_t *kc, const std::vector<RxChain> &chains,
                     std::vector<RxWalk> &walks, const std::vector<Nt9Item> &items9, const Tch9Jobs &jobs,
                     const std::vector<int8_t> &h_eb, int bound = 0)
{
	int r = 0;
	const std::vector<int> &fj = jobs.facch, &tj = jobs.tch;
	const int nf = bound + (int)fj.size(), nt9 = bound + (int)tj.size(), nj = bound ? bound : nf + nt9;
	std::vector<int8_t> eb((size_t)nj * 662);
	std::vector<uint8_t> keys((size_t)nj * 8, 0);
	std::vector<uint32_t> fns(nj);
	for (int i = 0; i < (int)(fj.size() + tj.size()); i++) {
		const int k = i < nf ? fj[i] : tj[i - nf];
		std::memcpy(&eb[(size_t)i * 662], &h_eb[(size_t)k * 662], 662);
		if (kc) std::memcpy(&keys[(size_t)i * 8], kc + (size_t)chains[items9[k].chain].a * 8, 8);
		fns[i] = (uint32_t)walks[items9[k].chain].log[items9[k].frame].fn;
	}
	std::vector<uint8_t> l2f((size_t)nf * 38), l2t((size_t)nt9 * 60);
	std::vector<int32_t> crcf(nf), cvf(nf), cvt(nt9);
	const int8_t *d_e2 = sg.in(eb.data(), eb.size());
	const uint8_t *d_k = sg.in(keys.data(), keys.size());
	const uint32_t *d_fn = sg.in(fns.data(), (size_t)nj);
	uint8_t *d_ks = sg.dev<uint8_t>((size_t)nj * 658);
	uint8_t *d_l2f = sg.dev<uint8_t>((size_t)nf * 38), *d_l2t = sg.dev<uint8_t>((size_t)nt9 * 60);
	int32_t *d_crc = sg.dev<int32_t>((size_t)nf), *d_cvf = sg.dev<int32_t>((size_t)nf), *d_cvt = sg.dev<int32_t>((size_t)nt9);
	// all runs in one launch: every burst knows its position in its own run (jobs.pos lives until the synchronisation below)
	const int32_t *d_pos = nt9 ? sg.in(jobs.pos.data(), (size_t)nt9) : nullptr;
	if ((r = sg.err()) || sg.measures()) return r;
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
	if (nt9) {
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
		const Nt9Item &it = items9[take_f ? fj[a9] : tj[b9]];
		const RxChain &c = chains[it.chain];
		gmr1_hip_rx_big_record rec;
		std::memset(&rec, 0, sizeof(rec));
		rec.arfcn = rx_label(arfcn, c.a);
		rec.chain = (uint8_t)c.chain;
		rec.fn = (uint32_t)walks[it.chain].log[it.frame].fn;
		rec.tn = (uint8_t)it.tn;
		rec.type = take_f ? 0x1a : 0x18;     // GSMTAP_GMR1_TCH9 | GSMTAP_GMR1_FACCH; GSMTAP_GMR1_TCH9
		rec.len = take_f ? 38 : 60;
		rec.conv = take_f ? cvf[a9] : cvt[b9];
		std::memcpy(rec.l2, take_f ? &l2f[(size_t)a9 * 38] : &l2t[(size_t)b9 * 60], rec.len);
		if (!take_f || !crcf[a9])            // (a TCH9 burst has no CRC to check, gmr1_rx.c:336-339)
			walks[it.chain].big.push_back(rec);
		take_f ? a9++ : b9++;
	}
	return 0;
}

}  // namespace

namespace gmr1 {

// ---- TCH9 follow-up (rx_tch9, gmr1_rx.c:262-353) ----------------------------------------------
// From the frame of a chain's first ASSIGNMENT COMMAND 1 on, every frame's NT9 burst on the assigned
// timeslot of the CSD carrier: demodulate (sync sequence 0 = FACCH9, 1 = TCH9), decipher with A5/1 of the
// frame number, decode.  Nothing feeds back, so it is one more batched pass: one demodulation launch, one
// keystream launch, one FACCH9 launch, one TCH9 launch over all interleaver runs (a run starts at every
// assignment; gmr1_deinterleave_inter only advances on TCH9 bursts).  The frames and the runs: rx_follow.h.
int tch9_follow_chains(hipStream_t st, int sps, const float *csd, const uint16_t *arfcn, const uint8_t *kc,
                       const std::vector<RxChain> &chains, std::vector<RxWalk> &walks)
{
	int r = 0;
	std::vector<Nt9Item> items9;
	for (size_t ci = 0; ci < chains.size(); ci++)
		tch9_plan_items((int)ci, walks[ci].log, walks[ci].events9, chains[ci].len, sps, &items9);
	const int n9 = (int)items9.size();
	if (!n9)
		return 0;
	std::vector<uint64_t> off9(n9);
	std::vector<float> fs9(n9);
	for (int k = 0; k < n9; k++) {
		const FrameCtx &x = walks[items9[k].chain].log[items9[k].frame];
		off9[k] = chains[items9[k].chain].base + (uint64_t)rx_tch9_begin(x.align, sps, items9[k].tn);
		fs9[k] = -x.freq_err;
	}
	std::vector<int8_t> h_eb((size_t)n9 * 662);
	std::vector<int32_t> h_sid(n9), h_rv(n9);
	// the pass: the demodulation and, behind it, the decodes of the frames that ask for one.  Run first on a measuring arena,
	// with every frame asking for both decodes, it sizes the arena it then runs on.
	auto pass = [&](Arena &arena) -> int {
		Stage sg(st, &arena);
		const uint64_t *d_o = sg.in(off9.data(), (size_t)n9);
		const float *d_f = sg.in(fs9.data(), (size_t)n9);
		int8_t *d_eb = sg.out(h_eb.data(), (size_t)n9 * 662);
		int32_t *d_sid = sg.out(h_sid.data(), (size_t)n9);
		int32_t *d_rv = sg.out(h_rv.data(), (size_t)n9);
		if ((r = sg.err())) return r;
		if (arena.measures) return tch9_decode_jobs(st, sg, arfcn, kc, chains, walks, items9, Tch9Jobs(), h_eb, n9);
		r = demod_dev_energy(st, GMR1_HIP_NT9, n9, sps, rx_tch9_in_len(sps), csd, d_o, d_f, d_eb, 662, d_sid, nullptr, nullptr, d_rv);
		if (r) return r;
		if ((r = sg.fetch())) return r;
		const Tch9Jobs jobs = tch9_plan_jobs(items9, h_sid.data(), h_rv.data());
		if (jobs.facch.empty() && jobs.tch.empty())
			return 0;
		return tch9_decode_jobs(st, sg, arfcn, kc, chains, walks, items9, jobs, h_eb);
	};
	Arena arena;
	return arena.sized_by(pass);
}

// ---- TCH9 follow-up of one push of the streaming loop -------------------------------------------
// This push's frames of every chain with a data call through the batched call follower (tch9_follow_enqueue: what
// gmr1_hip_tch9_follow_batch_dev runs), in ONE invocation however many commands the push holds: tch9_plan_push
// (rx_follow.h) cuts a chain's frames into segments, one per command and one for the call carried in, and every segment
// is a call of the follower.  The follower finds call q's state at slot q, and the big records come out in call order, so
// the calls have to stand chain by chain, segment by segment: their states are gathered into that order in the pass's
// scratch (k_tch9f_move: the chain's own state for the call carried in, and for a command, whose state is fresh anyway,
// as the carrier of the key under k_tch9f_assign), and the last segment's state of every chain goes back to the chain's
// slot of d_state afterwards.  No state and no frame visits the host: k_tch9f_big closes the reporting frames up into big
// records on the device, the count comes back, then exactly that many records.
int tch9_follow_push(hipStream_t st, int sps, const float *csd, const uint16_t *arfcn, bool horizon, const std::vector<RxChain> &chains,
                     const std::vector<RxWalk> &walks, gmr1_hip_tch9_state *d_state, Tch9CallCarry *carry,
                     gmr1_hip_rx_big_record *big_out, int max_big, int *n_big)
{
	int r = 0;
	*n_big = 0;
	std::vector<Tch9PushCall> pc(chains.size());
	for (size_t ci = 0; ci < chains.size(); ci++)
		pc[ci] = {&walks[ci].log, &walks[ci].events9, carry[ci], chains[ci].len};
	Tch9PushPlan plan;
	if (!tch9_plan_push(pc, sps, horizon, &plan))
		return fail(-EIO, "tch9 follow-up: a frame the walk admitted does not hold its NT9 window");
	for (size_t ci = 0; ci < chains.size(); ci++)
		carry[ci] = plan.carry[ci];
	const int n_seg = (int)plan.segs.size(), n = (int)plan.items.size();
	if (!n_seg)
		return 0;
	std::vector<int32_t> first((size_t)n_seg + 1), at((size_t)n_seg), own((size_t)n_seg), fresh, back_at, back_own;
	std::vector<uint32_t> label((size_t)n_seg), fn((size_t)n);
	std::vector<uint64_t> off((size_t)n);
	std::vector<float> fs((size_t)n);
	for (int q = 0; q < n_seg; q++) {
		const Tch9Seg &sgm = plan.segs[q];
		const RxChain &c = chains[sgm.chain];
		first[q] = (int32_t)sgm.first;
		at[q] = q;
		own[q] = sgm.chain;
		label[q] = (uint32_t)rx_label(arfcn, c.a) | ((uint32_t)(c.chain & 0xff) << 16) | ((uint32_t)(sgm.tn & 0xff) << 24);
		if (sgm.ev)
			fresh.push_back(q);
	}
	first[n_seg] = n;
	for (size_t ci = 0; ci < chains.size(); ci++)
		if (plan.last_seg[ci] >= 0) {
			back_at.push_back(plan.last_seg[ci]);
			back_own.push_back((int32_t)ci);
		}
	for (int k = 0; k < n; k++) {
		const Nt9Item &it = plan.items[k];
		const FrameCtx &x = walks[it.chain].log[it.frame];
		off[k] = chains[it.chain].base + (uint64_t)rx_tch9_begin(x.align, sps, it.tn);
		fs[k] = -x.freq_err;
		fn[k] = (uint32_t)x.fn;
	}
	// the pass: the calls' states, the index arrays, the frames, the follower's frames and their big records, the count, the
	// follower's scratch.  Run first on a measuring arena, it sizes the arena it then runs on.
	auto pass = [&](Arena &arena) -> int {
		Stage sg(st, &arena);
		gmr1_hip_tch9_state *d_call = sg.dev<gmr1_hip_tch9_state>((size_t)n_seg);
		const int32_t *d_first = sg.in(first.data(), first.size());
		const int32_t *d_at = sg.in(at.data(), at.size()), *d_own = sg.in(own.data(), own.size());
		const int32_t *d_fresh = sg.in(fresh.data(), fresh.size());
		const int32_t *d_back_at = sg.in(back_at.data(), back_at.size()), *d_back_own = sg.in(back_own.data(), back_own.size());
		const uint32_t *d_label = sg.in(label.data(), label.size());
		const uint64_t *d_off = sg.in(off.data(), (size_t)n);
		const float *d_fs = sg.in(fs.data(), (size_t)n);
		const uint32_t *d_fn = sg.in(fn.data(), (size_t)n);
		gmr1_hip_tch9_frame *d_got = sg.dev<gmr1_hip_tch9_frame>((size_t)n);
		gmr1_hip_rx_big_record *d_big = sg.dev<gmr1_hip_rx_big_record>((size_t)n);
		int32_t h_count = 0;
		int32_t *d_count = sg.dev<int32_t>(1);
		unsigned char *scratch = sg.dev<unsigned char>(tch9_follow_scratch_bytes(n));
		if ((r = sg.err()) || arena.measures) return r;
		HIP_TRY(launch_tch9f_move(n_seg, d_call, d_at, d_state, d_own, st));
		HIP_TRY(launch_tch9f_assign((int)fresh.size(), d_fresh, d_call, st));
		if (n) {
			r = tch9_follow_enqueue(st, scratch, n_seg, sps, rx_tch9_in_len(sps), 2 /* GMR1_TCH9_9k6, gmr1_rx.c:333 */, csd, d_first, n,
			                        d_off, d_fs, d_fn, d_call, d_got);
			if (r) return r;
		}
		HIP_TRY(launch_tch9f_move((int)back_at.size(), d_state, d_back_own, d_call, d_back_at, st));
		if (!n)
			return sg.fetch();                        // (the staged arrays are the host's until the stream is through)
		Tch9BigArgs ba;
		std::memset(&ba, 0, sizeof(ba));
		ba.n_calls = n_seg; ba.n_frames = n; ba.max_out = n;
		ba.first = d_first; ba.frames = d_got; ba.label = d_label; ba.out = d_big; ba.n_out = d_count;
		HIP_TRY(launch_tch9f_big(ba, st));
		sg.back(&h_count, d_count, 1);
		if ((r = sg.fetch())) return r;
		*n_big = h_count;
		const int fit = std::min((int)h_count, max_big);
		if (fit > 0)
			HIP_TRY(hipMemcpyAsync(big_out, d_big, (size_t)fit * sizeof(gmr1_hip_rx_big_record), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return 0;
	};
	Arena arena;
	return arena.sized_by(pass);
}

}  // namespace gmr1
