// Host-side check of the fused batch kernel's packed per-lane operand tables (osmo-gmr_amd/csrc/rx4_operands.h) against what
// they pack: the ord_of_sym rows of the built-in BCCH / DC6 descriptors, built as the library builds them (tables_init,
// flatten, to_dev), and the trellis-step table, worked out here once more from the interleaver and the scrambler
// (l1_codes.h).  Then the rule that keeps the fused path from starting on tables that disagree (fused_operands_match,
// rx_select.h): it must hold for the tables as made and fail for each of them perturbed in one place.
// tests/test_rx4_operand_tables.py builds and runs it (once more under the address and undefined-behaviour sanitizers).
#include <cstdio>
#include <cstring>

#include "host_tables.h"
#include "rx_select.h"

using namespace gmr1;

#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d: %s\n", __LINE__, #x); return 1; } } while (0)

namespace {

DevBurst g_types[kNumTypes], g_copy[kNumTypes];

int build_types()
{
	tables_init();
	std::memset(g_types, 0, sizeof(g_types));
	for (int i = 0; i < GMR1_HIP_N_BURSTS; i++) {
		gmr1_hip_burst_flat f;
		int rv = flatten(kBuiltin[i], &f, kBuiltinName[i]);
		if (rv == 0)
			rv = to_dev(f, &g_types[i]);
		if (rv) {
			std::printf("FAIL: built-in burst table %d is inconsistent\n", i);
			return 1;
		}
	}
	return 0;
}

// a step's descriptor from the codes themselves: the two coded bits 2k, 2k + 1 travel at intra_pos(53, .) (+ 4 pad bits on
// the CCCH), bit 10 / 26 = the scrambler's bit at that place
uint32_t step_word(int chain, int k)
{
	static const auto scr = l1c::scramble_seq<448>();
	uint32_t w = 0;
	for (int j = 0; j < 2; j++) {
		const int ei = l1c::intra_pos(53, 2 * k + j) + (chain ? 4 : 0);
		w |= ((uint32_t)ei | (scr.bit[ei] ? 0x400u : 0u)) << (16 * j);
	}
	return w;
}

int check_ord4()
{
	static_assert(sizeof(Rx4Ord4) == 2 * 64 * 8, "8 bytes per (kind, lane)");
	Rx4Ord4 o;
	std::memset(&o, 0x5a, sizeof(o));
	make_ord4(g_types, &o);
	const int types[2] = {GMR1_HIP_BCCH, GMR1_HIP_DC6};
	int fills = 0;
	for (int kind = 0; kind < 2; kind++) {
		const DevBurst &bt = g_types[types[kind]];
		CHECK(bt.len == 234);
		for (int lane = 0; lane < 64; lane++)
			for (int r = 0; r < 4; r++) {
				const int i = lane + 64 * r;
				const int want = i < bt.len ? bt.ord_of_sym[i] : -1;
				if (o.v[kind][lane][r] != want) {
					std::printf("FAIL: ord4[%d][%d][%d] = %d, expected %d\n", kind, lane, r, o.v[kind][lane][r], want);
					return 1;
				}
				fills += i >= bt.len;
			}
		// (the first data symbol is symbol 2, the sync chunk at 28 is no data)
		CHECK(o.v[kind][0][0] == -1 && o.v[kind][2][0] == 0 && o.v[kind][28][0] == -1);
	}
	CHECK(fills == 2 * (256 - 234));
	// every data symbol's place is there exactly once: 212 (BCCH), 216 (DC6) of them
	for (int kind = 0; kind < 2; kind++) {
		const int nd = g_types[types[kind]].ebits / 2;
		bool seen[256] = {};
		int n = 0;
		for (int lane = 0; lane < 64; lane++)
			for (int r = 0; r < 4; r++) {
				const int v = o.v[kind][lane][r];
				if (v < 0)
					continue;
				CHECK(v < nd && !seen[v]);
				seen[v] = true;
				n++;
			}
		CHECK(n == nd);
	}
	return 0;
}

int check_steps4()
{
	static_assert(sizeof(Rx4Steps4) == 2 * 64 * 16, "16 bytes per (chain, lane)");
	const StepTable st = make_steps();
	const Rx4Steps4 s4 = make_steps4(st);
	int fills = 0;
	for (int chain = 0; chain < 2; chain++)
		for (int lane = 0; lane < 64; lane++)
			for (int it = 0; it < 4; it++) {
				const int k = lane + 64 * it;
				const uint32_t want = k < kSteps12 ? step_word(chain, k) : 0u;
				if (k < kSteps12)
					CHECK(st.w[chain][k] == want);
				if (s4.w[chain][lane][it] != want) {
					std::printf("FAIL: steps4[%d][%d][%d] = %08x, expected %08x\n", chain, lane, it, s4.w[chain][lane][it], want);
					return 1;
				}
				fills += k >= kSteps12;
			}
	CHECK(fills == 2 * (256 - 212));
	CHECK(std::memcmp(&s4, &kHostSteps4, sizeof(s4)) == 0);
	return 0;
}

int check_refusal()
{
	static Rx4Ord4 o;
	static Rx4Steps4 s;
	auto reset = [] {
		std::memcpy(g_copy, g_types, sizeof(g_copy));
		make_ord4(g_types, &o);
		s = kHostSteps4;
	};
	reset();
	CHECK(fused_operands_match(g_types, o, s));
	CHECK(fused_operands_match(g_copy, o, s));
	o.v[0][17][1] += 1;                                    // one BCCH place
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	o.v[1][63][3] = 0;                                     // a fill (symbol 255 of a 234-symbol burst) that is no -1
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	o.v[1][28][0] = 5;                                     // a DC6 sync symbol given a place
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	g_copy[GMR1_HIP_DC6].ord_of_sym[100] += 1;             // the descriptor moves, the packed copy does not
	CHECK(!fused_operands_match(g_copy, o, s));
	reset();
	g_copy[GMR1_HIP_BCCH].len = 230;                       // the last data symbol, 230 (lane 38, r 3), falls off the burst
	CHECK(!fused_operands_match(g_copy, o, s));
	reset();
	s.w[0][5][2] ^= 0x400u;                                // one scrambling bit of the BCCH chain
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	s.w[1][0][0] += 1;                                     // one soft-bit index of the CCCH chain
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	s.w[1][63][3] = 1;                                     // a fill (step 255 of 212) that is not 0
	CHECK(!fused_operands_match(g_types, o, s));
	reset();
	CHECK(fused_operands_match(g_copy, o, s));
	return 0;
}

}  // namespace

int main()
{
	if (build_types() || check_ord4() || check_steps4() || check_refusal())
		return 1;
	std::printf("ok\n");
	return 0;
}
