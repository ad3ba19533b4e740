// capi_one.cpp -- the reference's one-burst calls (gmr1_pi4cxpsk_demod, pi4cxpsk.h:101-105; gmr1_bcch_decode, bcch.h:38;
// gmr1_ccch_decode, ccch.h:38) without per-call allocations: the pinned block, the decode memo and the host side of the
// resident server's mailbox protocol (rx_server.h).
#include <cstddef>
#include <chrono>
#include <atomic>
#include <mutex>

#include <osmocom/gmr1/l1/bcch.h>
#include <osmocom/gmr1/l1/ccch.h>

#include "capi_common.h"
#include "rx_select.h"
#include "rx_server.h"

using namespace gmr1;

namespace {

// ---- the reference's one-burst calls without per-call allocations -----------------------------------------------
// An unchanged gmr1_rx.c makes ~1300 blocking calls per carrier-minute (gmr1_pi4cxpsk_demod, then gmr1_bcch_decode /
// gmr1_ccch_decode on what it returned).  Each used to cost a handful of hipMalloc / pageable hipMemcpy / hipFree
// round trips; now operands and results live in ONE pinned, device-mapped host block created on first use: the call
// copies its input there (<= 16 KB), launches on a private stream, the kernel reads and writes the block over the
// link (zero copy), and the call returns when the stream has drained.  For the BCCH and DC6 formats the demodulator
// call runs the fused kernel (the layer-1 chain on the soft bits it has just produced costs nothing extra) and
// remembers (soft bits -> L2, CRC, metric); the decode call that follows with those very soft bits -- compared byte
// by byte -- is answered from that memo, anything else is decoded on the GPU as before.  Process-wide, one call at a
// time (the reference's calls are not re-entrant either).

// The block.  Four groups of 64 bytes behind the samples: the request's scalars, the answer's scalars with the L2 message,
// the soft bits, the mailbox -- the kernels' loads from iq and the mailbox words rely on these boundaries.
struct alignas(64) OneBlock {
	float iq[kMaxInLen * 2];            // the window, complex samples
	alignas(64) uint64_t offset;        // 0
	uint8_t kind;
	float freq_shift;
	alignas(64) int32_t rv;
	int32_t sync_id;
	float toa, freq_err;
	int32_t crc, conv;
	alignas(32) uint8_t l2[24];
	alignas(64) int8_t eb[1024];
	alignas(64) OneMail mail;
};
constexpr size_t kOneOff = (size_t)kMaxInLen * 8, kOneOut = kOneOff + 64, kOneEb = kOneOut + 64, kOneMail = kOneEb + 1024;
static_assert(offsetof(OneBlock, iq) == 0 && offsetof(OneBlock, offset) == kOneOff && offsetof(OneBlock, kind) == kOneOff + 8 &&
              offsetof(OneBlock, freq_shift) == kOneOff + 12, "one-burst block: the request");
static_assert(offsetof(OneBlock, rv) == kOneOut && offsetof(OneBlock, sync_id) == kOneOut + 4 && offsetof(OneBlock, toa) == kOneOut + 8 &&
              offsetof(OneBlock, freq_err) == kOneOut + 12 && offsetof(OneBlock, crc) == kOneOut + 16 &&
              offsetof(OneBlock, conv) == kOneOut + 20 && offsetof(OneBlock, l2) == kOneOut + 32, "one-burst block: the answer");
static_assert(offsetof(OneBlock, eb) == kOneEb && offsetof(OneBlock, mail) == kOneMail && sizeof(OneBlock) == kOneMail + 64,
              "one-burst block: soft bits and mailbox");

// (soft bits -> L2, CRC, metric) of the last fused demodulator call
struct OneMemo {
	bool valid = false;
	int chain = 0, n = 0, acc = 0;
	int8_t eb[432];
	uint8_t l2[24];
	int32_t crc = 0, conv = 0;
	void store(int chain_, int neb, const OneBlock *b)
	{
		valid = true;
		chain = chain_;
		acc = conv_acc();
		n = neb;
		std::memcpy(eb, b->eb, (size_t)neb);
		std::memcpy(l2, b->l2, 24);
		crc = b->crc;
		conv = b->conv;
	}
	bool match(int chain_, int neb, const sbit_t *bits) const
	{
		return valid && chain == chain_ && n == neb && acc == conv_acc() && !std::memcmp(eb, bits, (size_t)neb);
	}
};

struct OneBurst {
	std::mutex mu;
	int dev = -1;
	hipStream_t st = nullptr;
	OneBlock *h = nullptr, *d = nullptr;           // the block: host address, device address
	// the resident server of the fused BCCH / DC6 call at 4 samples per symbol (rx_server.h)
	hipStream_t srv_st = nullptr;
	uint32_t seq = 0, gen = 0;
	int srv_acc = -1;
	OneMemo memo;
};
OneBurst g_one;

// g_one.mu held.  0, or -errno; *usable = false when the context belongs to another device (caller takes the slow path)
int one_ready(bool *usable)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	if (!g_one.h) {
		HIP_TRY(hipStreamCreateWithFlags(&g_one.st, hipStreamNonBlocking));
		void *h = nullptr, *d = nullptr;
		HIP_TRY(hipHostMalloc(&h, sizeof(OneBlock), hipHostMallocMapped));
		HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
		std::memset(h, 0, sizeof(OneBlock));        // (the mailbox: no request, no answer, generation 0 = no server yet)
		g_one.h = static_cast<OneBlock *>(h);
		g_one.d = static_cast<OneBlock *>(d);
		g_one.dev = dev;
	}
	*usable = g_one.dev == dev;
	return 0;
}

// one burst of the fused path with its operands and results in the block (device addresses); sps is the caller's
void one_fused_args(RxArgs *a)
{
	OneBlock *d = g_one.d;
	std::memset(a, 0, sizeof(*a));
	a->n = 1;
	a->iq = reinterpret_cast<const float2 *>(d->iq);
	a->offset = &d->offset; a->kind = &d->kind; a->freq_shift = &d->freq_shift;
	a->l2 = d->l2; a->crc = &d->crc; a->conv = &d->conv;
	a->toa = &d->toa; a->freq_err = &d->freq_err;
	a->ebits = d->eb; a->rv = &d->rv;
}

// The fused one-burst call through the resident server (rx_server_kernels.inc): the request is in the block; post its number,
// start a server if none is alive (or the one alive decodes with the other Viterbi decoder), spin on the answer's number.
// GMR1_HIP_ONE_BURST_SERVER=0 in the environment keeps the launch per call.  g_one.mu held.  0, 1 = not taken (the caller
// launches as before), or -errno.
constexpr unsigned kServerIdleUs = 200, kServerLifeUs = 500000;
// the next server generation, on the servers' one stream: it starts when the last one has gone, so there is never more
// than one at work.  The generation number is written BEFORE any request it is to answer, and a server reads the request
// number before the generation: a superseded server cannot take a request posted behind the change.
int one_server_start(OneMail *mh)
{
	RxArgs a;
	one_fused_args(&a);
	int r = rx_fused_base_args(4, &a);
	if (r) return r;
	volatile uint32_t *v_ended = &mh->ended, *v_gen = &mh->gen;
	*v_gen = ++g_one.gen;
	std::atomic_thread_fence(std::memory_order_seq_cst);
	const hipError_t e = launch_one_server(a, &g_one.d->mail, g_one.gen, kServerIdleUs, kServerLifeUs, g_one.srv_st);
	if (e != hipSuccess) {
		*v_ended = g_one.gen;                     // it never ran: the next call starts another
		return fail(-EIO, "one-burst server: launch failed: %s", hipGetErrorString(e));
	}
	g_one.srv_acc = conv_acc();
	return 0;
}

int one_server_call()
{
	static const bool enabled = [] { const char *e = getenv("GMR1_HIP_ONE_BURST_SERVER"); return !(e && e[0] == '0'); }();
	if (!enabled)
		return 1;
	if (!g_one.srv_st)
		HIP_TRY(hipStreamCreateWithFlags(&g_one.srv_st, hipStreamNonBlocking));
	OneMail *mh = &g_one.h->mail;
	volatile uint32_t *v_req = &mh->req, *v_done = &mh->done, *v_ended = &mh->ended;
	int launches = 0, r;
	// a server that decodes with the other Viterbi decoder is retired before the request exists
	if (g_one.gen != 0 && g_one.srv_acc != conv_acc()) {
		launches++;
		if ((r = one_server_start(mh))) return r;
	}
	const uint32_t seq = ++g_one.seq;
	std::atomic_thread_fence(std::memory_order_release);
	*v_req = seq;
	// Giving up on the server must not leave a live request behind: a server that starts late (queued behind a long kernel)
	// would serve it after this call has returned and the lock is released -- into a block the next call is rewriting.  So
	// the generation is retired first (a server reads the request number BEFORE the generation: none of an older generation
	// takes the request any more), the servers' stream is drained (one that was in the middle of the request finishes; every
	// server ends by itself), and the call goes on as a launch per call (return 1) instead of failing.
	auto give_up = [&](const char *why) -> int {
		volatile uint32_t *v_gen = &mh->gen;
		*v_gen = ++g_one.gen;
		std::atomic_thread_fence(std::memory_order_seq_cst);
		const hipError_t e = hipStreamSynchronize(g_one.srv_st);
		*v_ended = g_one.gen;                         // nothing is alive: the next call starts a server of its own
		*v_done = seq;                                // (and no later server may mistake the abandoned request for a new one)
		if (e != hipSuccess)
			return fail(-EIO, "one-burst server: %s, and its stream does not drain: %s", why, hipGetErrorString(e));
		return 1;
	};
	const auto t0 = std::chrono::steady_clock::now();
	for (unsigned spins = 0;; spins++) {
		if (*v_done == seq)
			break;
		if (*v_ended == g_one.gen) {
			// the current generation has ended (idle, lifetime; or none was ever started: both numbers 0): the next one
			// finds the request waiting
			if (launches++ >= 4)
				return give_up("ends without answering");
			if ((r = one_server_start(mh))) return r;
		}
		if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5))
			return give_up("no answer within 5 s");
#if defined(__x86_64__)
		__builtin_ia32_pause();
#endif
	}
	std::atomic_thread_fence(std::memory_order_acquire);
	return 0;
}

// the burst description of a demodulator call: a built-in type, or a caller-defined one flattened into *custom for the
// spare table slot (*is_custom)
int resolve_burst(struct gmr1_pi4cxpsk_burst *burst_type, int *type, DevBurst *custom, bool *is_custom)
{
	int r = host_types();
	if (r) return r;
	*type = -1;
	for (int i = 0; i < GMR1_HIP_N_BURSTS; i++)
		if (burst_type == kBuiltin[i])
			*type = i;
	*is_custom = *type < 0;
	if (*is_custom) {
		gmr1_hip_burst_flat f;
		r = flatten(burst_type, &f, "custom");
		if (r == 0) r = to_dev(f, custom);
		if (r) return fail(r, "gmr1_pi4cxpsk_demod: unsupported burst description");
		*type = kCustomSlot;
	}
	return 0;
}

// A built-in format's burst through the block.  *taken = false: the block belongs to another device's context, nothing was
// done and the caller stages the call; otherwise what gmr1_pi4cxpsk_demod returns.
int demod_one_block(int type, const DevBurst &ht, const struct osmo_cxvec *burst_in, int sps, float freq_shift,
                    sbit_t *ebits, int *sync_id_p, float *toa_p, float *freq_err_p, bool *taken)
{
	std::lock_guard<std::mutex> lk(g_one.mu);
	int r = one_ready(taken);
	if (r) return r;
	if (!*taken)
		return 0;
	OneBlock *h = g_one.h, *d = g_one.d;
	const int in_len = burst_in->len;
	std::memcpy(h->iq, burst_in->data, (size_t)in_len * 8);
	h->offset = 0;
	h->freq_shift = freq_shift;
	g_one.memo.valid = false;
	// the fused kernel takes the two formats of rx_bcch / rx_ccch at the window lengths they use (gmr1_rx.c:759, 809)
	const int kind = type == GMR1_HIP_BCCH ? 0 : (type == GMR1_HIP_DC6 ? 1 : -1);
	const bool fused = kind >= 0 && sps >= 4 && sps <= 8 && in_len == fused_window_len(kind, sps);
	bool served = false;
	if (fused && sps == 4) {
		h->kind = (uint8_t)kind;
		r = one_server_call();
		if (r < 0) return r;
		served = r == 0;
		r = 0;
		h->sync_id = 0;
	}
	if (served) {
		// (answered by the resident server)
	} else if (fused) {
		h->kind = (uint8_t)kind;
		RxArgs a;
		one_fused_args(&a);
		a.sps = sps;
		r = rx_fused_launch(g_one.st, a);
		h->sync_id = 0;                                // one training sequence: sync_id 0 when found
	} else {
		r = demod_dev_impl(g_one.st, type, ht, 1, sps, in_len, d->iq, &d->offset, &d->freq_shift, d->eb, ht.ebits, &d->sync_id,
		                   &d->toa, &d->freq_err, nullptr, &d->rv);
	}
	if (r) return r;
	if (!served)
		HIP_TRY(hipStreamSynchronize(g_one.st));
	if (h->rv) return h->rv;
	std::memcpy(ebits, h->eb, (size_t)ht.ebits);
	if (sync_id_p) *sync_id_p = h->sync_id;
	if (toa_p) *toa_p = h->toa;
	if (freq_err_p) *freq_err_p = h->freq_err;
	if (fused)
		g_one.memo.store(kind ? kChainCcch : kChainBcch, ht.ebits, h);
	return 0;
}

}  // namespace

extern "C" {

int gmr1_pi4cxpsk_demod(struct gmr1_pi4cxpsk_burst *burst_type,
                        struct osmo_cxvec *burst_in, int sps, float freq_shift,
                        sbit_t *ebits, int *sync_id_p, float *toa_p, float *freq_err_p)
{
	if (!burst_type || !burst_in || !burst_in->data || !ebits)
		return fail(-EINVAL, "gmr1_pi4cxpsk_demod: NULL argument");
	int type;
	DevBurst custom;
	bool is_custom;
	int r = resolve_burst(burst_type, &type, &custom, &is_custom);
	if (r) return r;
	const DevBurst &ht = is_custom ? custom : g_host_types[type];
	if (!is_custom && burst_in->len >= 1 && burst_in->len <= kMaxInLen) {
		bool taken = false;
		r = demod_one_block(type, ht, burst_in, sps, freq_shift, ebits, sync_id_p, toa_p, freq_err_p, &taken);
		if (r || taken) return r;
	}
	const uint64_t off = 0;
	int32_t rv = 0, sid = -1;
	float toa = 0.f, fe = 0.f;
	r = demod_host_impl(type, ht, is_custom ? &custom : nullptr, 1, sps, burst_in->len,
	                    reinterpret_cast<const float *>(burst_in->data),
	                    (uint64_t)burst_in->len, &off, &freq_shift, reinterpret_cast<int8_t *>(ebits), ht.ebits,
	                    &sid, &toa, &fe, nullptr, &rv);
	if (r) return r;
	if (rv) return rv;
	if (sync_id_p) *sync_id_p = sid;
	if (toa_p) *toa_p = toa;
	if (freq_err_p) *freq_err_p = fe;
	return 0;
}

// reference-compatible single-burst decoders (bcch.h:38, ccch.h:38).  A device
// failure cannot be reported through the reference's "crc result" return value
// without being mistaken for a CRC verdict, so it is returned as -errno (< 0).
static int decode_one(int chain, uint8_t *l2, const sbit_t *bits_e, int *conv_rv)
{
	if (!l2 || !bits_e)
		return fail(-EINVAL, "decode: NULL argument");
	const int neb = chain == kChainCcch ? 432 : 424;
	int32_t crc = 0, conv = 0;
	{
		std::lock_guard<std::mutex> lk(g_one.mu);
		bool usable = false;
		int r = one_ready(&usable);
		if (r) return r;
		if (usable) {
			const OneMemo &m = g_one.memo;
			if (m.match(chain, neb, bits_e)) {
				// these very soft bits were decoded by the demodulator call that produced them
				std::memcpy(l2, m.l2, 24);
				if (conv_rv) *conv_rv = m.conv;
				return m.crc;
			}
			OneBlock *h = g_one.h, *d = g_one.d;
			std::memcpy(h->eb, bits_e, (size_t)neb);
			r = l1_dev(g_one.st, chain, 1, d->eb, d->l2, &d->crc, &d->conv);
			if (r) return r;
			HIP_TRY(hipStreamSynchronize(g_one.st));
			std::memcpy(l2, h->l2, 24);
			if (conv_rv) *conv_rv = h->conv;
			return h->crc;
		}
	}
	int r = l1_host(chain, 1, reinterpret_cast<const int8_t *>(bits_e), l2, &crc, &conv);
	if (r) return r;
	if (conv_rv) *conv_rv = conv;
	return crc;
}

int gmr1_bcch_decode(uint8_t *l2, const sbit_t *bits_e, int *conv_rv) { return decode_one(kChainBcch, l2, bits_e, conv_rv); }

int gmr1_ccch_decode(uint8_t *l2, const sbit_t *bits_e, int *conv_rv) { return decode_one(kChainCcch, l2, bits_e, conv_rv); }

}  // extern "C"
