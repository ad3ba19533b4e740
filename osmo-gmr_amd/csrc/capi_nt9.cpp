// capi_nt9.cpp -- C ABI of the NT9 burst decoders: FACCH9 (reference include/osmocom/gmr1/l1/facch9.h:39-41)
// and TCH9 (include/osmocom/gmr1/l1/tch9.h:40-53).  The map that tells the kernel where the soft bit of every coded
// bit of every trellis step sits in the burst is nt9_map.h's, built from l1_codes.h; this file uploads it once per
// kind and device.  Everything per burst runs on the GPU.

#include "capi_common.h"

#include "../../include/gmr1_hip.h"
#include "../../include/osmocom/gmr1/l1/facch9.h"
#include "../../include/osmocom/gmr1/l1/interleave.h"
#include "../../include/osmocom/gmr1/l1/tch9.h"
#include "dev_cache.h"
#include "nt9_map.h"

using namespace gmr1;

namespace {

DevCache<int, uint32_t *> g_maps;

int get_map(int kind, const uint32_t **out)
{
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	uint32_t *const *d;
	const int r = g_maps.get(dev, kind, &d, [kind](uint32_t **m) { return upload(m, nt9_build_map(kind)); });
	if (!r) *out = *d;
	return r;
}

int nt9_dev(hipStream_t st, int kind, int n, int seq_len, const int8_t *ebits, const uint8_t *ciph,
            uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv)
{
	if (n < 0 || !ebits || !l2)
		return fail(-EINVAL, "nt9: ebits / l2 are required");
	if (kind < 0 || kind > 3)
		return fail(-EINVAL, "nt9: mode %d unknown", kind);
	if (seq_len < 1 || (n % seq_len) != 0)
		return fail(-EINVAL, "nt9: %d bursts are not a whole number of sequences of %d", n, seq_len);
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	Nt9Args a;
	std::memset(&a, 0, sizeof(a));
	if ((r = nt9_kind_args(kind, &a))) return r;
	a.n = n; a.seq_len = seq_len; a.ebits = ebits; a.ciph = ciph; a.l2 = l2;
	a.sacch = sacch; a.status = status; a.crc = crc; a.conv = conv;
	HIP_TRY(launch_nt9(a, st));
	return 0;
}

}  // namespace

namespace gmr1 {
// TCH9 bursts of several interleaver runs of unequal length, run after run, in one launch: seq_pos[i] (device)
// = position of burst i in its run (the receive loop's TCH9 follow-up, capi_rx_follow.cpp)
int tch9_runs_dev_impl(hipStream_t st, int mode, int n, const int32_t *seq_pos, const int8_t *ebits, const uint8_t *ciph,
                       uint8_t *l2, int32_t *conv)
{
	if (n < 0 || mode < 0 || mode > 2 || !seq_pos || !ebits || !l2)
		return fail(-EINVAL, "tch9 runs: bad arguments");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	Nt9Args a;
	std::memset(&a, 0, sizeof(a));
	if ((r = nt9_kind_args(mode, &a))) return r;
	a.n = n; a.seq_len = 1; a.seq_pos = seq_pos; a.ebits = ebits; a.ciph = ciph; a.l2 = l2; a.conv = conv;
	HIP_TRY(launch_nt9(a, st));
	return 0;
}

// What a launch of kind 0..2 (TCH9 mode) or 3 (FACCH9) shares, into `a`, which the caller has zeroed: the code's constants, the
// selected Viterbi decoder and the current device's map (the TCH9 follower's launches, capi_tch9_follow.cpp)
int nt9_kind_args(int kind, Nt9Args *a)
{
	const uint32_t *map;
	int r = get_map(kind, &map);
	if (r) return r;
	a->kind = kind; a->conv_acc = conv_acc(); a->N = kNt9Kinds[kind].N; a->len = kNt9Kinds[kind].len;
	a->map = map; a->l2_bytes = kNt9Kinds[kind].l2_bytes;
	return 0;
}
}  // namespace gmr1

namespace {

int nt9_host(int kind, int n, int seq_len, const int8_t *ebits, const uint8_t *ciph,
             uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!ebits || !l2)
		return fail(-EINVAL, "nt9: ebits / l2 are required");
	if (kind < 0 || kind > 3)
		return fail(-EINVAL, "nt9: mode %d unknown", kind);
	const int nb = kNt9Kinds[kind].l2_bytes;
	Stage sg;
	const int8_t *d_e = sg.in(ebits, (size_t)n * 662);
	const uint8_t *d_c = sg.in(ciph, (size_t)n * 658);
	uint8_t *d_l2 = sg.out(l2, (size_t)n * nb);
	int8_t *d_sa = sg.out_always(sacch, (size_t)n * 10);
	int8_t *d_st = sg.out_always(status, (size_t)n * 4);
	int32_t *d_crc = sg.out_always(crc, (size_t)n);
	int32_t *d_cv = sg.out_always(conv, (size_t)n);
	if ((r = sg.err())) return r;
	r = nt9_dev(nullptr, kind, n, seq_len, d_e, d_c, d_l2, d_sa, d_st, d_crc, d_cv);
	if (r) return r;
	return sg.fetch();
}

}  // namespace

extern "C" {

int gmr1_hip_facch9_decode_batch_dev(void *stream, int n, const int8_t *ebits, const uint8_t *ciph,
                                     uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv)
{
	if (!crc)
		return fail(-EINVAL, "facch9: crc is required");
	return nt9_dev((hipStream_t)stream, 3, n, 1, ebits, ciph, l2, sacch, status, crc, conv);
}

int gmr1_hip_facch9_decode_batch(int n, const int8_t *ebits, const uint8_t *ciph,
                                 uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *crc, int32_t *conv)
{
	if (n > 0 && !crc)
		return fail(-EINVAL, "facch9: crc is required");
	return nt9_host(3, n, 1, ebits, ciph, l2, sacch, status, crc, conv);
}

int gmr1_hip_tch9_decode_batch_dev(void *stream, int n_chan, int seq_len, int mode, const int8_t *ebits,
                                   const uint8_t *ciph, uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *conv)
{
	if (mode < 0 || mode > 2)
		return fail(-EINVAL, "tch9: mode %d unknown (0 2k4, 1 4k8, 2 9k6)", mode);
	if (n_chan < 0 || seq_len < 1)
		return fail(-EINVAL, "tch9: n_chan / seq_len");
	return nt9_dev((hipStream_t)stream, mode, n_chan * seq_len, seq_len, ebits, ciph, l2, sacch, status, nullptr, conv);
}

int gmr1_hip_tch9_decode_batch(int n_chan, int seq_len, int mode, const int8_t *ebits, const uint8_t *ciph,
                               uint8_t *l2, int8_t *sacch, int8_t *status, int32_t *conv)
{
	if (mode < 0 || mode > 2)
		return fail(-EINVAL, "tch9: mode %d unknown (0 2k4, 1 4k8, 2 9k6)", mode);
	if (n_chan < 0 || seq_len < 1)
		return fail(-EINVAL, "tch9: n_chan / seq_len");
	return nt9_host(mode, n_chan * seq_len, seq_len, ebits, ciph, l2, sacch, status, nullptr, conv);
}

// reference-compatible single call (facch9.h:39-41)
int gmr1_facch9_decode(uint8_t *l2, sbit_t *bits_sacch, sbit_t *bits_status,
                       const sbit_t *bits_e, const ubit_t *ciph, int *conv_rv)
{
	if (!l2 || !bits_sacch || !bits_status || !bits_e)
		return fail(-EINVAL, "gmr1_facch9_decode: NULL argument");
	int32_t crc = -1, conv = 0;
	int r = nt9_host(3, 1, 1, reinterpret_cast<const int8_t *>(bits_e), reinterpret_cast<const uint8_t *>(ciph), l2,
	                 reinterpret_cast<int8_t *>(bits_sacch), reinterpret_cast<int8_t *>(bits_status), &crc, &conv);
	if (r) return r;
	if (conv_rv) *conv_rv = conv;
	return crc;
}

// ---- the reference's stateful single-burst TCH9 call (tch9.h:47-50, interleave.h:40-56) -----------------
// The history the depth-3 de-interleaver needs is kept as the previous two bursts AS RECEIVED (kNt9IlSlot,
// nt9_map.h); every call decodes the three-burst sequence on the GPU, where the de-interleaving is part of
// the gather (nt9_kernels.hip), and returns the newest burst's outputs.

int gmr1_interleaver_init(struct gmr1_interleaver *il, int N, int K)
{
	if (!il)
		return fail(-EINVAL, "gmr1_interleaver_init: NULL");
	std::memset(il, 0, sizeof(*il));
	if (N != 3 || K != 648)
		return fail(-EINVAL, "gmr1_interleaver_init: only the (3, 648) geometry of TCH9 is provided");
	uint8_t *b = static_cast<uint8_t *>(std::calloc(2, kNt9IlSlot));
	if (!b)
		return fail(-ENOMEM, "gmr1_interleaver_init: out of memory");
	il->N = N;
	il->K = K;
	il->bits_cpp = b;
	return 0;
}

void gmr1_interleaver_fini(struct gmr1_interleaver *il)
{
	if (!il)
		return;
	std::free(il->bits_cpp);
	std::memset(il, 0, sizeof(*il));
}

void gmr1_tch9_decode(uint8_t *l2, sbit_t *bits_sacch, sbit_t *bits_status, const sbit_t *bits_e,
                      enum gmr1_tch9_mode mode, const ubit_t *ciph, struct gmr1_interleaver *il, int *conv_rv)
{
	if (!l2 || !bits_e || !il || !il->bits_cpp || il->N != 3 || il->K != 648 || (int)mode < 0 || (int)mode > 2) {
		(void)fail(-EINVAL, "gmr1_tch9_decode: bad argument");
		return;
	}
	const int nb = kNt9Kinds[(int)mode].l2_bytes;
	// sequence = [burst n-2, burst n-1, this burst]; slot (n & 1) holds burst n-2
	uint8_t *older = il->bits_cpp + (size_t)(il->n & 1) * kNt9IlSlot, *newer = il->bits_cpp + (size_t)((il->n + 1) & 1) * kNt9IlSlot;
	int8_t seq_e[3 * 662];
	uint8_t seq_c[3 * 658];
	std::memcpy(seq_e, older, 662);
	std::memcpy(seq_c, older + 662, 658);
	std::memcpy(seq_e + 662, newer, 662);
	std::memcpy(seq_c + 658, newer + 662, 658);
	std::memcpy(seq_e + 2 * 662, bits_e, 662);
	if (ciph)
		std::memcpy(seq_c + 2 * 658, ciph, 658);
	else
		std::memset(seq_c + 2 * 658, 0, 658);
	uint8_t out[3 * 60] = {0};
	int8_t sa[3 * 10] = {0}, stt[3 * 4] = {0};
	int32_t conv[3] = {0, 0, 0};
	(void)nt9_host((int)mode, 3, 3, seq_e, seq_c, out, sa, stt, nullptr, conv);
	std::memcpy(l2, out + 2 * nb, (size_t)nb);
	if (bits_sacch) std::memcpy(bits_sacch, sa + 20, 10);
	if (bits_status) std::memcpy(bits_status, stt + 8, 4);
	if (conv_rv) *conv_rv = conv[2];
	// this burst replaces burst n-2
	std::memcpy(older, seq_e + 2 * 662, 662);
	std::memcpy(older + 662, seq_c + 2 * 658, 658);
	il->n++;
}

}  // extern "C"
