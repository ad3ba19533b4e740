// l1_codes_host.cpp -- prints what osmo-gmr_amd/csrc/l1_codes.h and nt9_map.h describe, one "section name values..."
// line each, for tests/test_l1_codes_host.py to compare with the reference's files.  Host code only: no GPU call, built
// plain and under the address and undefined-behaviour sanitizers.  Every table is also made once in a constant
// expression and held against its run-time twin, since the kernels' tables are made the first way and the host's the
// second.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "l1_codes.h"
#include "nt9_map.h"

using namespace gmr1;
using namespace gmr1::l1c;

namespace {

int g_bad = 0;

// the generators, and the code word of every register value (state << 1 | input), g0 in the MSB: what a trellis is made of
template <int N>
void polys(const char *name, int K, const unsigned (&p)[N])
{
	printf("polys %s", name);
	for (int i = 0; i < N; i++)
		printf(" %u", p[i]);
	printf("\nwords %s", name);
	for (uint32_t reg = 0; reg < (1u << K); reg++)
		printf(" %u", conv_word(p, reg));
	printf("\n");
}

template <int M>
void mask(const char *name, const Punct<M> &p)
{
	printf("punct gmr1_punct_%s %d %d %d", name, p.r, p.L, p.N);
	for (int i = 0; i < M; i++)
		printf(" %d", p.mask[i]);
	printf("\n");
}

void positions(const char *name, const std::vector<uint8_t> &flag)
{
	printf("punctured %s", name);
	for (size_t i = 0; i < flag.size(); i++)
		if (flag[i])
			printf(" %d", (int)i);
	printf("\n");
}

// the xCH and TCH3 lists as a table maker builds them: in a constant expression
template <int TOTAL>
struct Flags { uint8_t f[TOTAL]; };
template <int TOTAL, int M>
constexpr Flags<TOTAL> flags_of(const Punct<M> &mn)
{
	Flags<TOTAL> t{};
	punctured_bits(t.f, TOTAL, kNoScheme, scheme(mn), kNoScheme, 0);
	return t;
}
constexpr Flags<624> kXchFlags = flags_of<624>(k9_13_P1213);

struct Units { uint32_t v[300]; };
constexpr Units units_of(const Crc &c, int n)
{
	Units t{};
	for (int k = 0; k < n; k++)
		t.v[k] = crc_unit(c, k, n);
	return t;
}
constexpr Units kUnits16_192 = units_of(kCrc16, 192);
constexpr ScrambleSeq<662> kScr = scramble_seq<662>();
static_assert(intra_pos(53, 9) == 53 * 5 + 1 && tch3_pos(25) == 6, "positions in a constant expression");

}  // namespace

int main()
{
	polys("gmr1_conv_k5_12", 5, kK5_12);
	polys("gmr1_conv_k5_13", 5, kK5_13);
	polys("gmr1_conv_k5_14", 5, kK5_14);
	polys("gmr1_conv_k5_15", 5, kK5_15);
	polys("gmr1_conv_k6_14", 6, kK6_14);
	polys("gmr1_conv_k9_12", 9, kK9_12);
	polys("gmr1_conv_k9_13", 9, kK9_13);
	polys("gmr1_conv_k9_14", 9, kK9_14);
	polys("gmr1_conv_tch3", 7, kTch3);

	printf("crc gmr1_crc8 %d %u\ncrc gmr1_crc12 %d %u\ncrc gmr1_crc16 %d %u\n", kCrc8.bits, kCrc8.poly, kCrc12.bits,
	       kCrc12.poly, kCrc16.bits, kCrc16.poly);

#define MASK(name, L, N, r, two, ...) mask(#name, name);
	GMR1_L1_PUNCT_LIST(MASK)
#undef MASK

	printf("scramble");
	Scrambler g;
	for (int i = 0; i < 662; i++) {
		const uint32_t b = g.next();
		g_bad += (b != 0) != kScr.bit[i];
		printf(" %u", b);
	}
	printf("\n");

	static const int kN[] = {12, 14, 33, 53, 54, 80, 81};
	for (int N : kN) {
		printf("intra %d", N);
		for (int k = 0; k < 8 * N; k++)
			printf(" %d", intra_pos(N, k));
		printf("\n");
	}
	printf("tch3_pos");
	for (int kc = 0; kc < 104; kc++)
		printf(" %d", tch3_pos(kc));
	printf("\n");

	positions("tch9_2k4", nt9_punctured(0));
	positions("tch9_4k8", nt9_punctured(1));
	positions("tch9_9k6", nt9_punctured(2));
	positions("facch9", nt9_punctured(3));
	{
		std::vector<uint8_t> x(624, 0), t3(96, 0);
		punctured_bits(x.data(), 624, kNoScheme, scheme(k9_13_P1213), kNoScheme, 0);
		punctured_bits(t3.data(), 96, kNoScheme, scheme(k5_12_P12), kNoScheme, 0);
		for (int i = 0; i < 624; i++)
			g_bad += x[i] != kXchFlags.f[i];
		positions("xch_dc12", x);
		positions("tch3", t3);
	}

	static const struct { const char *name; Crc c; } kCrcs[] = {{"gmr1_crc8", kCrc8}, {"gmr1_crc12", kCrc12}, {"gmr1_crc16", kCrc16}};
	static const int kLens[] = {16, 76, 123, 192, 300};
	for (const auto &c : kCrcs)
		for (int n : kLens) {
			printf("crc_unit %s %d", c.name, n);
			for (int k = 0; k < n; k++)
				printf(" %u", crc_unit(c.c, k, n));
			printf("\n");
		}
	for (int k = 0; k < 192; k++)
		g_bad += kUnits16_192.v[k] != crc_unit(kCrc16.bits, kCrc16.poly, k, 192);

	for (int kind = 0; kind < 4; kind++) {
		const std::vector<uint32_t> map = nt9_build_map(kind);
		printf("nt9_map %d", kind);
		for (uint32_t e : map)
			printf(" %u", e);
		printf("\n");
	}
	printf("constexpr_mismatches %d\n", g_bad);
	return g_bad ? 1 : 0;
}
