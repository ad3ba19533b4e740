// The encoder plans without the library or a GPU (osmo-gmr_amd/csrc/enc_plan.h, enc_plan.cpp, compiled with plain g++ and no
// ROCm include path).  Every chain is built twice, into memory filled with different bytes, and must come out the same both
// times -- every byte of the plan is written -- with the sizes the public header and the chain's plan_* function state and
// every descriptor in range: what k_encode (tx_kernels.hip) indexes with them exists.  Whether the maps are the RIGHT ones is
// tests/test_tx_plan.py's question (bit by bit against the oracle's encoders).  Run once plain and once under the address
// and undefined-behaviour sanitizers by tests/test_enc_plan_host.py (a stand-alone program: nothing is preloaded).
#include <cstdio>
#include <cstring>

#include "enc_plan.h"

using namespace gmr1;

namespace {

// per chain, in PlanId's order: the burst bits of include/gmr1_hip.h, the counts of enc_plan.cpp's plan_* functions, and the
// bits of the CRC registers A and B the chain computes (RACH: CRC8 and CRC12; the traffic channels: none)
struct Want { const char *name; int n_out, n_in0, n_in1, n_aux0, n_aux1, n_ciph, depth, crc_a, crc_b; };
const Want kWant[kPlCount] = {
	{"bcch", 424, 24, 0, 0, 0, 0, 1, 16, 0},
	{"ccch", 432, 24, 0, 0, 0, 0, 1, 16, 0},
	{"facch3", 416, 10, 0, 32, 0, 384, 1, 16, 0},
	{"tch3_m0", 212, 20, 0, 4, 0, 208, 1, 0, 0},
	{"tch3_m1", 212, 20, 0, 4, 0, 208, 1, 0, 0},
	{"facch9", 662, 38, 0, 10, 4, 658, 1, 16, 0},
	{"tch9_2k4", 662, 18, 0, 10, 4, 658, 3, 0, 0},
	{"tch9_4k8", 662, 30, 0, 10, 4, 658, 3, 0, 0},
	{"tch9_9k6", 662, 60, 0, 10, 4, 658, 3, 0, 0},
	{"rach", 494, 18, 1, 0, 0, 0, 1, 8, 12},
	{"xch_dc12", 432, 24, 0, 0, 0, 0, 1, 16, 0},
};

int g_bad = 0;

#define CHECK(cond, ...)                                   \
	do {                                                   \
		if (!(cond)) {                                     \
			std::printf("%s: %s: ", w.name, #cond);        \
			std::printf(__VA_ARGS__);                      \
			std::printf("\n");                             \
			g_bad++;                                       \
		}                                                  \
	} while (0)

void check(int id)
{
	const Want &w = kWant[id];
	static EncPlan a, b;
	std::memset(&a, 0x00, sizeof(a));
	std::memset(&b, 0xa5, sizeof(b));
	build_enc_plan(id, &a);
	build_enc_plan(id, &b);
	CHECK(std::memcmp(&a, &b, sizeof(a)) == 0, "two builds differ");
	const EncPlan &P = a;
	CHECK(P.n_out == w.n_out, "%d", (int)P.n_out);
	CHECK(P.n_in0 == w.n_in0 && P.n_in1 == w.n_in1, "%d %d", (int)P.n_in0, (int)P.n_in1);
	CHECK(P.n_aux0 == w.n_aux0 && P.n_aux1 == w.n_aux1, "%d %d", (int)P.n_aux0, (int)P.n_aux1);
	CHECK(P.n_ciph == w.n_ciph && P.depth == w.depth, "%d %d", (int)P.n_ciph, (int)P.depth);
	CHECK(P.n_in0 + P.n_in1 <= kEncMaxIn && P.n_ext > 0 && P.n_ext <= kEncMaxExt && P.n_out <= kEncMaxOut, "%d", (int)P.n_ext);
	if (g_bad)
		return;                        // (the counts bound the loops below)
	// the window masks: allocated slots hold a mask of at most nine bits (K <= 9), and they come first
	int n_poly = 0;
	while (n_poly < 8 && P.poly[n_poly])
		n_poly++;
	for (int i = 0; i < 8; i++)
		CHECK((i < n_poly) == (P.poly[i] != 0) && P.poly[i] < (1u << 9), "poly[%d] = %#x", i, (unsigned)P.poly[i]);
	for (int e = 0; e < P.n_out; e++) {
		const uint32_t ds = P.out[e];
		const int t = ds & 1023, poly = (ds >> 10) & 7, kind = (ds >> 13) & 3, ci = (ds >> 16) & 1023, d = (ds >> 26) & 3;
		CHECK((ds >> 28) == 0 && kind <= 2, "out[%d] = %#x", e, (unsigned)ds);
		if (kind == 0)
			CHECK(t < P.n_ext && poly < n_poly, "out[%d]: window %d of %d, slot %d of %d", e, t, (int)P.n_ext, poly, n_poly);
		if (kind == 2)
			CHECK(t < P.n_aux0 + P.n_aux1, "out[%d]: multiplexed bit %d of %d", e, t, (int)(P.n_aux0 + P.n_aux1));
		CHECK(ci == 0 || ci - 1 < P.n_ciph, "out[%d]: keystream bit %d of %d", e, ci - 1, (int)P.n_ciph);
		CHECK(d < P.depth, "out[%d]: delay %d of %d", e, d, (int)P.depth);
	}
	for (int e = P.n_out; e < kEncMaxOut; e++)
		CHECK(P.out[e] == 0, "out[%d] = %#x behind the burst", e, (unsigned)P.out[e]);
	const int n_pay = 8 * (P.n_in0 + P.n_in1);
	for (int i = 0; i < P.n_ext; i++) {
		const unsigned s = P.ext_src[i];
		if (s == 0xffffu)
			continue;
		if (s < 0x4000u)
			CHECK((int)s < n_pay, "ext_src[%d]: payload bit %u of %d", i, s, n_pay);
		else if (s < 0x8000u)
			CHECK((int)(s - 0x4000u) < w.crc_a, "ext_src[%d]: bit %u of register A (%d bits)", i, s - 0x4000u, w.crc_a);
		else
			CHECK((int)(s - 0x8000u) < w.crc_b, "ext_src[%d]: bit %u of register B (%d bits)", i, s - 0x8000u, w.crc_b);
	}
	// the CRC tables: nothing behind the payload, nothing above the register's width
	for (int k = 0; k < kEncMaxIn * 8; k++) {
		CHECK((k < n_pay || P.crc_tab[k] == 0) && (P.crc_tab[k] >> w.crc_a) == 0, "crc_tab[%d] = %#x", k, (unsigned)P.crc_tab[k]);
		CHECK((k < n_pay || P.crc_tab2[k] == 0) && (P.crc_tab2[k] >> w.crc_b) == 0, "crc_tab2[%d] = %#x", k, (unsigned)P.crc_tab2[k]);
	}
}

}  // namespace

int main()
{
	static_assert(sizeof(EncPlan) == 5824, "the size gmr1_hip_encoder_plan reports");
	for (int id = 0; id < kPlCount; id++)
		check(id);
	if (g_bad) {
		std::printf("%d checks failed\n", g_bad);
		return 1;
	}
	std::printf("ok\n");
	return 0;
}
