// capi_tx_ref.cpp -- the transmit direction behind the reference's own calls: the single-burst encoders (reference
// include/osmocom/gmr1/l1/bcch.h:37, ccch.h:37, facch3.h:37-38, tch3.h:37-39, facch9.h:37-39, tch9.h:47-49, rach.h:37,
// xch_dc12.h:37), each one encode_host of a batch of one (capi_encode.cpp), and the stand-alone layer-1 primitives
// (scramb.h:36-37, interleave.h:36-56), each one blocking k_bitmap over a position table the host writes down.

#include "capi_common.h"

#include "../../include/osmocom/gmr1/l1/bcch.h"
#include "../../include/osmocom/gmr1/l1/ccch.h"
#include "../../include/osmocom/gmr1/l1/facch3.h"
#include "../../include/osmocom/gmr1/l1/facch9.h"
#include "../../include/osmocom/gmr1/l1/interleave.h"
#include "../../include/osmocom/gmr1/l1/rach.h"
#include "../../include/osmocom/gmr1/l1/scramb.h"
#include "../../include/osmocom/gmr1/l1/tch3.h"
#include "../../include/osmocom/gmr1/l1/tch9.h"
#include "../../include/osmocom/gmr1/l1/xch_dc12.h"
#include "nt9_map.h"

using namespace gmr1;

namespace {

// one blocking H2D -> k_bitmap -> D2H; perm / mask are position tables the host writes down (no data passes through them)
int bitmap_host(int n_in, int n_out, int soft, const void *in, const std::vector<int32_t> *perm,
                const std::vector<uint8_t> *mask, void *out, const char *what)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n_out < 0 || n_in < 0 || (n_out > 0 && (!in || !out)))
		return fail(-EINVAL, "%s: bad argument", what);
	if (n_out == 0)
		return 0;
	Stage sg;
	BitMapArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n_out; a.soft = soft;
	a.in = sg.in(static_cast<const uint8_t *>(in), (size_t)n_in);
	a.out = sg.out(static_cast<uint8_t *>(out), (size_t)n_out);
	a.perm = perm ? sg.in(perm->data(), (size_t)n_out) : nullptr;
	a.mask = mask ? sg.in(mask->data(), (size_t)n_out) : nullptr;
	if ((r = sg.err())) return r;
	HIP_TRY(launch_bitmap(a, nullptr));
	return sg.fetch();
}

std::vector<uint8_t> scramble_mask(int len)         // scramb.c:39-52
{
	std::vector<uint8_t> m((size_t)(len > 0 ? len : 0));
	l1c::Scrambler g;
	for (uint8_t &b : m)
		b = (uint8_t)g.next();
	return m;
}

}  // namespace

extern "C" {

// ---- the reference's own single calls; the void ones report a device failure through gmr1_hip_last_error() ----
void gmr1_bcch_encode(ubit_t *bits_e, const uint8_t *l2)
{
	(void)encode_host(kPlBcch, 1, 1, {.in0 = l2, .ebits = bits_e}, "gmr1_bcch_encode");
}
void gmr1_ccch_encode(ubit_t *bits_e, const uint8_t *l2)
{
	(void)encode_host(kPlCcch, 1, 1, {.in0 = l2, .ebits = bits_e}, "gmr1_ccch_encode");
}
int gmr1_xch_dc12_encode(ubit_t *bits_e, const uint8_t *l2)
{
	return encode_host(kPlXch, 1, 1, {.in0 = l2, .ebits = bits_e}, "gmr1_xch_dc12_encode");
}
void gmr1_facch3_encode(ubit_t *bits_e, const uint8_t *l2, const ubit_t *bits_s, const ubit_t *ciph)
{
	(void)encode_host(kPlFacch3, 1, 1, {.in0 = l2, .aux0 = bits_s, .ciph = ciph, .ebits = bits_e}, "gmr1_facch3_encode");
}
void gmr1_tch3_encode(ubit_t *bits_e, const uint8_t *frame0, const uint8_t *frame1, const ubit_t *bits_s,
                      const ubit_t *ciph, int m)
{
	if (!frame0 || !frame1) {
		(void)fail(-EINVAL, "gmr1_tch3_encode: NULL frame");
		return;
	}
	uint8_t frames[20];
	std::memcpy(frames, frame0, 10);
	std::memcpy(frames + 10, frame1, 10);
	(void)encode_host(m ? kPlTch3M1 : kPlTch3M0, 1, 1, {.in0 = frames, .aux0 = bits_s, .ciph = ciph, .ebits = bits_e},
	                  "gmr1_tch3_encode");
}
void gmr1_facch9_encode(ubit_t *bits_e, const uint8_t *l2, const ubit_t *bits_sacch, const ubit_t *bits_status,
                        const ubit_t *ciph)
{
	(void)encode_host(kPlFacch9, 1, 1, {.in0 = l2, .aux0 = bits_sacch, .aux1 = bits_status, .ciph = ciph, .ebits = bits_e},
	                  "gmr1_facch9_encode");
}
// tch9.h:47-49: stateful, one burst per call.  What the depth-3 interleaver remembers is kept as the payloads of the
// previous two bursts (first 60 bytes of the two private slots of struct gmr1_interleaver: kNt9IlSlot, nt9_map.h); each
// call encodes the run [n-2, n-1, n] on the GPU and returns the newest burst (slots start zeroed = empty interleaver).
void gmr1_tch9_encode(ubit_t *bits_e, const uint8_t *l2, enum gmr1_tch9_mode mode, const ubit_t *bits_sacch,
                      const ubit_t *bits_status, const ubit_t *ciph, struct gmr1_interleaver *il)
{
	if (!bits_e || !l2 || !bits_sacch || !bits_status || !il || !il->bits_cpp || il->N != 3 || il->K != 648 ||
	    tch9_plan((int)mode) < 0) {
		(void)fail(-EINVAL, "gmr1_tch9_encode: bad argument");
		return;
	}
	const int nb = kNt9Kinds[(int)mode].l2_bytes;
	uint8_t *older = il->bits_cpp + (size_t)(il->n & 1) * kNt9IlSlot, *newer = il->bits_cpp + (size_t)((il->n + 1) & 1) * kNt9IlSlot;
	uint8_t pay[3 * 60], sa[3 * 10] = {0}, stt[3 * 4] = {0}, out[3 * 662];
	std::vector<uint8_t> cs;
	std::memcpy(pay, older, (size_t)nb);
	std::memcpy(pay + nb, newer, (size_t)nb);
	std::memcpy(pay + 2 * nb, l2, (size_t)nb);
	std::memcpy(sa + 20, bits_sacch, 10);
	std::memcpy(stt + 8, bits_status, 4);
	if (ciph) {
		cs.assign(3 * 658, 0);
		std::memcpy(cs.data() + 2 * 658, ciph, 658);
	}
	if (encode_host(tch9_plan((int)mode), 3, 3, {.in0 = pay, .aux0 = sa, .aux1 = stt, .ciph = ciph ? cs.data() : nullptr, .ebits = out},
	                "gmr1_tch9_encode"))
		return;
	std::memcpy(bits_e, out + 2 * 662, 662);
	std::memcpy(older, l2, (size_t)nb);                        // this burst replaces burst n-2
	il->n++;
}

void gmr1_rach_encode(ubit_t *bits_e, const uint8_t *rach, uint8_t sb_mask)
{
	(void)encode_host(kPlRach, 1, 1, {.in0 = rach, .in1 = &sb_mask, .ebits = bits_e}, "gmr1_rach_encode");
}

// ---- the stand-alone layer-1 primitives (scramb.h:36-37, interleave.h:36-56); each is one blocking call to the GPU ----
void gmr1_scramble_sbit(sbit_t *out, const sbit_t *in, int len)
{
	const std::vector<uint8_t> m = scramble_mask(len);
	(void)bitmap_host(len, len, 1, in, nullptr, &m, out, "gmr1_scramble_sbit");
}

void gmr1_scramble_ubit(ubit_t *out, const ubit_t *in, int len)
{
	const std::vector<uint8_t> m = scramble_mask(len);
	(void)bitmap_host(len, len, 0, in, nullptr, &m, out, "gmr1_scramble_ubit");
}

void gmr1_interleave_intra(void *out, const void *in, int N)
{
	if (N < 0) { (void)fail(-EINVAL, "gmr1_interleave_intra: N < 0"); return; }
	std::vector<int32_t> perm((size_t)8 * N);
	for (int kc = 0; kc < 8 * N; kc++)
		perm[l1c::intra_pos(N, kc)] = kc;                          // interleave.c:48-61
	(void)bitmap_host(8 * N, 8 * N, 0, in, &perm, nullptr, out, "gmr1_interleave_intra");
}

void gmr1_deinterleave_intra(void *out, const void *in, int N)
{
	if (N < 0) { (void)fail(-EINVAL, "gmr1_deinterleave_intra: N < 0"); return; }
	std::vector<int32_t> perm((size_t)8 * N);
	for (int kc = 0; kc < 8 * N; kc++)
		perm[kc] = l1c::intra_pos(N, kc);                          // interleave.c:73-87
	(void)bitmap_host(8 * N, 8 * N, 0, in, &perm, nullptr, out, "gmr1_deinterleave_intra");
}

// interleave.c:128-158.  The state is the reference's: N rows of K bits in il->bits_cpp (an object used with these two
// calls must not also be handed to gmr1_tch9_encode / gmr1_tch9_decode, which keep their own history there).
void gmr1_interleave_inter(struct gmr1_interleaver *il, void *bits_epp, void *bits_ep)
{
	if (!il || !il->bits_cpp || il->N != 3 || il->K != 648 || !bits_epp || !bits_ep) {
		(void)fail(-EINVAL, "gmr1_interleave_inter: bad argument");
		return;
	}
	const int N = il->N, K = il->K, cur = il->n % N;
	// staging = [state with this burst in row cur]: the row copy is the upload itself
	std::vector<uint8_t> stage(il->bits_cpp, il->bits_cpp + (size_t)N * K);
	std::memcpy(stage.data() + (size_t)cur * K, bits_ep, (size_t)K);
	std::vector<int32_t> perm((size_t)K);
	for (int jk = 0; jk < K; jk++)
		perm[jk] = ((cur - (jk % N) + N) % N) * K + jk;
	if (bitmap_host(N * K, K, 0, stage.data(), &perm, nullptr, bits_epp, "gmr1_interleave_inter"))
		return;
	std::memcpy(il->bits_cpp + (size_t)cur * K, stage.data() + (size_t)cur * K, (size_t)K);
	il->n++;
}

// interleave.c:163-190
void gmr1_deinterleave_inter(struct gmr1_interleaver *il, void *bits_ep, void *bits_epp)
{
	if (!il || !il->bits_cpp || il->N != 3 || il->K != 648 || !bits_ep || !bits_epp) {
		(void)fail(-EINVAL, "gmr1_deinterleave_inter: bad argument");
		return;
	}
	const int N = il->N, K = il->K, cur = il->n % N;
	// source = [state | received burst]; the new state takes bit jk of row (cur - jk mod N) from the burst
	std::vector<uint8_t> src((size_t)(N + 1) * K);
	std::memcpy(src.data(), il->bits_cpp, (size_t)N * K);
	std::memcpy(src.data() + (size_t)N * K, bits_epp, (size_t)K);
	std::vector<int32_t> perm((size_t)N * K);
	for (int i = 0; i < N; i++)
		for (int jk = 0; jk < K; jk++)
			perm[(size_t)i * K + jk] = (i == (cur - (jk % N) + N) % N) ? N * K + jk : i * K + jk;
	std::vector<uint8_t> state((size_t)N * K);
	if (bitmap_host((N + 1) * K, N * K, 0, src.data(), &perm, nullptr, state.data(), "gmr1_deinterleave_inter"))
		return;
	std::memcpy(il->bits_cpp, state.data(), (size_t)N * K);
	std::memcpy(bits_ep, state.data() + (size_t)((il->n + 1) % N) * K, (size_t)K);
	il->n++;
}

}  // extern "C"
