// l1_tables.cpp -- the code description objects of libgmr1-l1's API (reference include/osmocom/gmr1/l1/conv.h:36-44,
// l1/punct.h:54-106, l1/crc.h:36-38), exported for consumers that drive libosmocore's own encoder / decoder with them.
// They are expanded at compile time from l1_codes.h, the description the GPU path reads as well: the kernels' table
// makers, the NT9 gather maps (nt9_map.h) and the encoder plans (enc_plan.cpp) take their polynomials, masks and CRCs
// from the same header.
//
// A trellis is its generator polynomials (bit i = D^i; the output word has g0 in its MSB), a puncturing scheme is the
// list of its punctured mask positions.  tests/test_ref_tables.py compares every expanded table with the one printed
// in the reference's conv.c / punct.c / crc.c.
#include <stdint.h>

#include <osmocom/gmr1/l1/conv.h>
#include <osmocom/gmr1/l1/crc.h>
// (not l1/punct.h: its objects end in a flexible array member, which C++ cannot initialise; they are defined below
// as l1c::Punct<M>, a fixed-size twin of the same layout)

#include "l1_codes.h"

using namespace gmr1;

namespace {

template <int K>
struct Trellis {
	uint8_t out[1 << (K - 1)][2];
	uint8_t nxt[1 << (K - 1)][2];
};

template <int K, int N>
constexpr Trellis<K> make_trellis(const unsigned (&polys)[N])
{
	Trellis<K> t{};
	for (unsigned s = 0; s < (1u << (K - 1)); s++)
		for (unsigned b = 0; b < 2; b++) {
			const unsigned reg = (s << 1) | b;            // bit i = D^i
			t.out[s][b] = (uint8_t)l1c::conv_word(polys, reg);
			t.nxt[s][b] = (uint8_t)(reg & ((1u << (K - 1)) - 1u));
		}
	return t;
}

constexpr Trellis<5> t_k5_12 = make_trellis<5>(l1c::kK5_12);
constexpr Trellis<5> t_k5_13 = make_trellis<5>(l1c::kK5_13);
constexpr Trellis<5> t_k5_14 = make_trellis<5>(l1c::kK5_14);
constexpr Trellis<5> t_k5_15 = make_trellis<5>(l1c::kK5_15);
constexpr Trellis<6> t_k6_14 = make_trellis<6>(l1c::kK6_14);
constexpr Trellis<9> t_k9_12 = make_trellis<9>(l1c::kK9_12);
constexpr Trellis<9> t_k9_13 = make_trellis<9>(l1c::kK9_13);
constexpr Trellis<9> t_k9_14 = make_trellis<9>(l1c::kK9_14);
constexpr Trellis<7> t_tch3  = make_trellis<7>(l1c::kTch3);

}  // namespace

extern "C" {

#define CONV(name, n, k, term, t)                                                                        \
	extern const struct osmo_conv_code gmr1_conv_##name;                                                 \
	const struct osmo_conv_code gmr1_conv_##name = {n, k, 0, term, t.out, t.nxt, nullptr, nullptr, nullptr};

CONV(k5_12, 2, 5, CONV_TERM_FLUSH, t_k5_12)
CONV(k5_13, 3, 5, CONV_TERM_FLUSH, t_k5_13)
CONV(k5_14, 4, 5, CONV_TERM_FLUSH, t_k5_14)
CONV(k5_15, 5, 5, CONV_TERM_FLUSH, t_k5_15)
CONV(k6_14, 4, 6, CONV_TERM_FLUSH, t_k6_14)
CONV(k9_12, 2, 9, CONV_TERM_FLUSH, t_k9_12)
CONV(k9_13, 3, 9, CONV_TERM_FLUSH, t_k9_13)
CONV(k9_14, 4, 9, CONV_TERM_FLUSH, t_k9_14)
CONV(tch3, 2, 7, CONV_TERM_TAIL_BITING, t_tch3)

// crc.c:40-63
extern const struct osmo_crc8gen_code gmr1_crc8;
extern const struct osmo_crc16gen_code gmr1_crc12, gmr1_crc16;
const struct osmo_crc8gen_code gmr1_crc8 = {l1c::kCrc8.bits, (uint8_t)l1c::kCrc8.poly, 0x00, 0x00};
const struct osmo_crc16gen_code gmr1_crc12 = {l1c::kCrc12.bits, (uint16_t)l1c::kCrc12.poly, 0x0000, 0x0000};
const struct osmo_crc16gen_code gmr1_crc16 = {l1c::kCrc16.bits, (uint16_t)l1c::kCrc16.poly, 0x0000, 0x0000};

#define PUNCT(name, L, N, r, two, ...)                                                                   \
	extern const l1c::Punct<(L) * (N)> gmr1_punct_##name;                                                \
	const l1c::Punct<(L) * (N)> gmr1_punct_##name = l1c::name;
GMR1_L1_PUNCT_LIST(PUNCT)
}  // extern "C"
