// Host-side check of the kernel-choice and fused-path rules (osmo-gmr_amd/csrc/rx_select.h) against the built-in burst
// tables, built as the library builds them (tables_init, flatten, to_dev).  A wrong answer of demod_kernel_choice leaves
// every output correct on a GPU and only moves a time, so the expected values are written down here: the table is what the
// two condition blocks gave for these tables before they became a function.
// tests/test_rx_select_host.py builds and runs it (once more under the address and undefined-behaviour sanitizers).
#include <cstdio>
#include <cstring>

#include "host_tables.h"
#include "rx_select.h"

using namespace gmr1;

#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d: %s\n", __LINE__, #x); return 1; } } while (0)

namespace {

DevBurst g_types[kNumTypes];

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

struct Want { int impl, stage; };
constexpr int kExtra[6] = {4, 8, 20, 40, 80, 128};
struct Row { int type, len; Want want[6]; };
const Row kRows[] = {
	{GMR1_HIP_BCCH, 234, {{2, 80}, {2, 92}, {2, 128}, {2, 188}, {2, 308}, {0, 0}}},
	{GMR1_HIP_DC2, 78, {{3, 32}, {3, 36}, {3, 48}, {2, 68}, {2, 108}, {0, 0}}},
	{GMR1_HIP_DC6, 234, {{2, 64}, {2, 76}, {2, 112}, {2, 172}, {2, 292}, {0, 0}}},
	{GMR1_HIP_NT3_SPEECH, 117, {{3, 28}, {3, 32}, {3, 44}, {3, 64}, {2, 104}, {0, 0}}},
	{GMR1_HIP_NT3_FACCH, 117, {{4, 36}, {4, 40}, {4, 52}, {0, 0}, {0, 0}, {0, 0}}},
	{GMR1_HIP_DC12, 0, {}},
	{GMR1_HIP_NT6, 0, {}},
	{GMR1_HIP_NT9, 0, {}},
	{GMR1_HIP_RACH, 0, {}},
	{GMR1_HIP_SDCCH, 0, {}},
};

int check_kernel_choice()
{
	int stage;
	for (const Row &row : kRows) {
		const DevBurst &ht = g_types[row.type];
		if (row.len)
			CHECK(ht.len == row.len);
		for (int e = 0; e < 6; e++) {
			stage = -1;
			const int impl = demod_kernel_choice(ht, 4097, 4, ht.len * 4 + kExtra[e], 0, &stage);
			if (impl != row.want[e].impl || stage != row.want[e].stage) {
				std::printf("FAIL: %s +%d: %d/%d, expected %d/%d\n", kBuiltinName[row.type], kExtra[e], impl, stage,
				            row.want[e].impl, row.want[e].stage);
				return 1;
			}
		}
	}
	for (int t = 0; t < GMR1_HIP_N_BURSTS; t++) {
		const DevBurst &ht = g_types[t];
		// a batch at the threshold stays one burst per wave; so does every format at 8 samples per symbol
		CHECK(demod_kernel_choice(ht, 4096, 4, ht.len * 4 + 20, 0, &stage) == 0 && stage == 0);
		CHECK(demod_kernel_choice(ht, 4097, 8, ht.len * 8 + 40, 0, &stage) == 0 && stage == 0);
	}
	// The table's columns do not land on the rules' own limits, so the limits are met here, each worked out from the
	// conditions by hand: a sync chunk of L symbols takes L * 4 + extra window samples at in_len = len * 4 + extra.
	struct Edge { int type, extra; Want want; };
	const Edge edges[] = {
		// BCCH, chunks of 11, 3, 3 symbols: the longest chunk window is 44 + extra <= 128; stage 128 + 2 * 96
		{GMR1_HIP_BCCH, 84, {2, 320}}, {GMR1_HIP_BCCH, 85, {0, 0}},
		// DC6, chunks of 7, 3, 3: its chunk windows would fit up to +100, the window of 936 + extra <= 1024 samples ends it first
		{GMR1_HIP_DC6, 88, {2, 316}}, {GMR1_HIP_DC6, 89, {0, 0}},
		// the small variant stages at most 64 samples: DC2's one chunk of 7 symbols, NT3 speech's of 6 (its +40 is in the table)
		{GMR1_HIP_DC2, 36, {3, 64}}, {GMR1_HIP_DC2, 37, {2, 65}}, {GMR1_HIP_NT3_SPEECH, 41, {2, 65}},
		// the two-sequence variant as well: NT3 FACCH's chunk of 8 symbols
		{GMR1_HIP_NT3_FACCH, 32, {4, 64}}, {GMR1_HIP_NT3_FACCH, 33, {0, 0}},
	};
	for (const Edge &e : edges) {
		const DevBurst &ht = g_types[e.type];
		stage = -1;
		const int impl = demod_kernel_choice(ht, 4097, 4, ht.len * 4 + e.extra, 0, &stage);
		if (impl != e.want.impl || stage != e.want.stage) {
			std::printf("FAIL: %s +%d: %d/%d, expected %d/%d\n", kBuiltinName[e.type], e.extra, impl, stage, e.want.impl, e.want.stage);
			return 1;
		}
	}
	// the two-sequence variant has no debug stops; the others have
	const DevBurst &facch = g_types[GMR1_HIP_NT3_FACCH], &speech = g_types[GMR1_HIP_NT3_SPEECH];
	CHECK(demod_kernel_choice(facch, 4097, 4, facch.len * 4 + 20, 1, &stage) == 0 && stage == 0);
	CHECK(demod_kernel_choice(speech, 4097, 4, speech.len * 4 + 20, 1, &stage) == 3 && stage == 44);
	return 0;
}

// static: 35 KB of descriptors, off the stack
DevBurst g_copy[kNumTypes];

int check_fused_rules()
{
	CHECK(fused_formats_match(g_types));
	auto reset = [] { std::memcpy(g_copy, g_types, sizeof(g_copy)); };
	reset();
	CHECK(fused_formats_match(g_copy));
	g_copy[GMR1_HIP_BCCH].sync[0][0].syms[4] ^= 2;        // one BCCH training symbol
	CHECK(!fused_formats_match(g_copy));
	reset();
	g_copy[GMR1_HIP_DC6].sync[0][1].pos += 1;             // one DC6 chunk position
	CHECK(!fused_formats_match(g_copy));
	reset();
	g_copy[GMR1_HIP_BCCH].nbits = 1;
	CHECK(!fused_formats_match(g_copy));
	reset();
	g_copy[GMR1_HIP_DC6].nbits = 1;
	CHECK(!fused_formats_match(g_copy));

	// BCCH: 17 training symbols and three windows of 20 sps + 1 lags, 17 sps + 3 * 20 sps; DC6 gives 13 sps + 3 * 10 sps
	const int spss[4] = {1, 4, 8, 16};
	for (int sps : spss)
		CHECK(fused_stage_samples(g_types, sps) == 77 * sps);
	CHECK(fused_window_len(0, 4) == 1016 && fused_window_len(1, 4) == 976);
	CHECK(window_len(234, 4, 80) == 1016);

	const long long strides[3] = {0, 1, 1 << 20};
	for (int env = 0; env < 3; env++)
		for (long long ps : strides) {
			for (int sps = 1; sps < 4; sps++)
				CHECK(fused_impl(sps, ps, env) == 1);
			for (int sps = 4; sps <= 16; sps++)
				CHECK(fused_impl(sps, ps, env) == (ps ? 0 : env));
		}
	return 0;
}

// A test's own cells, "type:extra:n" each (a built-in burst id, in_len = len * 4 + extra at 4 samples per symbol, n bursts):
// one line "type extra n impl stage_samples" per cell, what demod_kernel_choice gives the product's call
int report_cells(int argc, char **argv)
{
	for (int i = 1; i < argc; i++) {
		int type, extra, n;
		if (std::sscanf(argv[i], "%d:%d:%d", &type, &extra, &n) != 3 || type < 0 || type >= GMR1_HIP_N_BURSTS || extra < 0 || n < 0) {
			std::printf("FAIL: cell '%s' is not type:extra:n\n", argv[i]);
			return 1;
		}
		const DevBurst &ht = g_types[type];
		int stage = -1;
		const int impl = demod_kernel_choice(ht, n, 4, ht.len * 4 + extra, 0, &stage);
		std::printf("%d %d %d %d %d\n", type, extra, n, impl, stage);
	}
	return 0;
}

}  // namespace

int main(int argc, char **argv)
{
	if (build_types() || check_kernel_choice() || check_fused_rules() || report_cells(argc, argv))
		return 1;
	std::printf("ok\n");
	return 0;
}
