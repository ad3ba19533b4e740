// l1_codes.h -- the GMR-1 layer-1 codes, written down once: generator polynomials (reference src/l1/conv.c), CRCs (crc.c),
// the 51 puncturing masks and gmr1_puncturer_generate's walk (punct.c), the scrambler (scramb.c), the intra-burst
// interleaver and the TCH3 permutation (interleave.c, tch3.c).  Plain C++17 without HIP; everything works in a constant
// expression and at run time, so the kernels' compile-time table makers, the host's plan and map builders and the exported
// libgmr1-l1 objects (l1_tables.cpp, which tests/test_ref_tables.py holds entry by entry to the reference's files) all read
// this one description.  tests/test_l1_codes_host.py checks the functions here against the reference without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gmr1 {
namespace l1c {

// ---- convolutional codes: generator polynomials, bit i = D^i ------------------------------------------------
// conv.c:123-128, 148-154, 174-181, 201-209, 229-236, 260-265, 345-351, 431-438 (k9_14: g3 as its TABLE has it), 518-523
constexpr unsigned kK5_12[] = {0x19, 0x17};
constexpr unsigned kK5_13[] = {0x15, 0x1b, 0x1f};
constexpr unsigned kK5_14[] = {0x19, 0x17, 0x15, 0x1f};
constexpr unsigned kK5_15[] = {0x15, 0x1b, 0x1f, 0x1d, 0x17};
constexpr unsigned kK6_14[] = {0x25, 0x2d, 0x3b, 0x3f};
constexpr unsigned kK9_12[] = {0x11d, 0x1af};
constexpr unsigned kK9_13[] = {0x1ed, 0x19b, 0x127};
constexpr unsigned kK9_14[] = {0x1b9, 0x1a5, 0x13b, 0x15f};
constexpr unsigned kTch3[] = {0x6d, 0x4f};

constexpr uint32_t parity(uint32_t v)
{
	v ^= v >> 16; v ^= v >> 8; v ^= v >> 4; v ^= v >> 2; v ^= v >> 1;
	return v & 1u;
}

// the N coded bits of one step, g0 in the MSB; reg = (state << 1) | input bit
template <int N>
constexpr uint32_t conv_word(const unsigned (&polys)[N], uint32_t reg)
{
	uint32_t w = 0;
	for (int j = 0; j < N; j++)
		w = (w << 1) | parity(reg & polys[j]);
	return w;
}

// ---- CRCs (crc.c:36-63): init 0, no final xor --------------------------------------------------------------
struct Crc { int bits; unsigned poly; };
constexpr Crc kCrc8 = {8, 0x9b}, kCrc12 = {12, 0x80f}, kCrc16 = {16, 0x1021};

// the register a lone 1 at bit k of an n-bit message leaves: the CRC is linear, so the check word of a message is the
// xor of these over its set bits
constexpr uint32_t crc_unit(int bits, uint32_t poly, int k, int n)
{
	const uint32_t top = 1u << (bits - 1), mask = (top << 1) - 1u;
	uint32_t crc = top;                            // the bit is about to leave the register
	for (int i = k; i < n; i++)
		crc = ((crc & top) ? ((crc << 1) ^ poly) : (crc << 1)) & mask;
	return crc;
}
constexpr uint32_t crc_unit(const Crc &c, int k, int n) { return crc_unit(c.bits, c.poly, k, n); }

// ---- puncturing masks (punct.c:136-1166) ----------------------------------------------------------------------
// same layout as struct gmr1_puncturer { int r, L, N; const uint8_t mask[]; } with the mask given its size
template <int M>
struct Punct {
	int r, L, N;
	uint8_t mask[M];                               // L * N entries: 0 = punctured, 1 = sent, 2 = sent twice (scheme E)
};

template <int M, int NZ>
constexpr Punct<M> make_punct(int r, int L, int N, int two, const int (&zeros)[NZ])
{
	Punct<M> p{r, L, N, {}};
	for (int i = 0; i < M; i++)
		p.mask[i] = 1;
	for (int i = 0; i < NZ; i++)
		if (zeros[i] >= 0)        // (the lists start with a -1 so that an empty one is still an array)
			p.mask[zeros[i]] = 0;
	if (two >= 0)
		p.mask[two] = 2;          // scheme E repeats a bit: the reference writes a 2 there (punct.c:313-324)
	return p;
}

// X(scheme, mask steps L, code outputs N, r, position of the one "2" (-1: none), punctured mask positions...)
#define GMR1_L1_PUNCT_LIST(X)                                                               \
	X(k5_12_P23, 3, 2, 2, -1, 0, 3)                                                         \
	X(k5_12_P25, 5, 2, 2, -1, 1, 5)                                                         \
	X(k5_12_Ps25, 5, 2, 2, -1, 5, 9)                                                        \
	X(k5_12_P311, 11, 2, 3, -1, 1, 5, 11)                                                   \
	X(k5_12_P412, 12, 2, 4, -1, 1, 5, 9, 13)                                                \
	X(k5_12_Ps412, 12, 2, 4, -1, 11, 15, 19, 23)                                            \
	X(k5_12_P12, 2, 2, 1, -1, 3)                                                            \
	X(k5_12_Ps12, 2, 2, 1, -1, 1)                                                           \
	X(k5_12_A, 4, 2, 0, -1)                                                                 \
	X(k5_12_B, 4, 2, 1, -1, 1)                                                              \
	X(k5_12_C, 4, 2, 2, -1, 1, 5)                                                           \
	X(k5_12_D, 4, 2, 3, -1, 0, 3, 4)                                                        \
	X(k5_12_E, 4, 2, 1, 1)                                                                  \
	X(k5_12_P38, 8, 2, 3, -1, 0, 4, 13)                                                     \
	X(k5_12_P26, 6, 2, 2, -1, 1, 7)                                                         \
	X(k5_12_P37, 7, 2, 3, -1, 1, 5, 9)                                                      \
	X(k5_13_P16, 6, 3, 1, -1, 2)                                                            \
	X(k5_13_P25, 5, 3, 2, -1, 7, 13)                                                        \
	X(k5_13_P15, 5, 3, 1, -1, 1)                                                            \
	X(k5_13_Ps15, 5, 3, 1, -1, 13)                                                          \
	X(k5_13_P78, 8, 3, 7, -1, 0, 1, 5, 9, 17, 19, 22)                                       \
	X(k5_15_P23, 3, 5, 2, -1, 7, 14)                                                        \
	X(k5_15_P53, 3, 5, 5, -1, 3, 6, 7, 13, 14)                                              \
	X(k5_15_Ps53, 3, 5, 5, -1, 3, 4, 6, 7, 13)                                              \
	X(k7_12_P23, 3, 2, 2, -1, 3, 4)                                                         \
	X(k7_12_P410, 10, 2, 4, -1, 1, 5, 9, 17)                                                \
	X(k7_12_P512, 12, 2, 5, -1, 3, 7, 15, 19, 23)                                           \
	X(k7_12_P116, 16, 2, 1, -1, 1)                                                          \
	X(k7_12_P148, 48, 2, 1, -1, 1)                                                          \
	X(k7_12_P184, 84, 2, 1, -1, 1)                                                          \
	X(k7_12_P1152, 152, 2, 1, -1, 1)                                                        \
	X(k7_12_P45, 5, 2, 4, -1, 0, 5, 6, 9)                                                   \
	X(k7_12_P245, 5, 2, 4, -1, 1, 2, 5, 6)                                                  \
	X(k9_12_P13, 3, 2, 1, -1, 1)                                                            \
	X(k9_12_P47, 7, 2, 4, -1, 0, 5, 9, 13)                                                  \
	X(k9_12_P34, 4, 2, 3, -1, 3, 4, 7)                                                      \
	X(k9_12_P17, 7, 2, 1, -1, 1)                                                            \
	X(k9_12_P19, 9, 2, 1, -1, 0)                                                            \
	X(k9_12_P26, 6, 2, 2, -1, 1, 7)                                                         \
	X(k9_12_P110, 10, 2, 1, -1, 0)                                                          \
	X(k9_12_P14, 4, 2, 1, -1, 1)                                                            \
	X(k9_12_P45, 5, 2, 4, -1, 0, 4, 7, 9)                                                   \
	X(k9_12_P234, 4, 2, 3, -1, 1, 2, 5)                                                     \
	X(k6_14_P45, 5, 4, 4, -1, 1, 5, 11, 19)                                                 \
	X(k9_14_P148, 8, 4, 14, -1, 1, 2, 5, 7, 9, 11, 13, 14, 18, 21, 22, 25, 26, 30)          \
	X(k9_14_P65, 5, 4, 6, -1, 0, 5, 12, 13, 15, 17)                                         \
	X(k9_13_P12, 2, 3, 1, -1, 3)                                                            \
	X(k9_13_P1213, 13, 3, 12, -1, 2, 4, 6, 11, 13, 15, 20, 22, 24, 29, 31, 33)              \
	X(k9_13_P44, 4, 3, 4, -1, 2, 3, 7, 11)                                                  \
	X(k9_13_P33, 3, 3, 3, -1, 0, 4, 8)                                                      \
	X(k9_13_P65, 5, 3, 6, -1, 1, 3, 7, 8, 9, 14)

#define GMR1_L1_PUNCT_OBJECT(name, L, N, r, two, ...)                                       \
	constexpr int z_##name[] = {-1, __VA_ARGS__};                                           \
	constexpr Punct<(L) * (N)> name = make_punct<(L) * (N)>(r, L, N, two, z_##name);
GMR1_L1_PUNCT_LIST(GMR1_L1_PUNCT_OBJECT)
#undef GMR1_L1_PUNCT_OBJECT

// ---- the puncturer (gmr1_puncturer_generate, punct.c:48-133) ------------------------------------------------
// a scheme as the walk reads it: the L * N mask entries (a struct gmr1_puncturer's or a Punct<M>'s); len 0 = no scheme
struct Scheme {
	int len;
	const uint8_t *mask;
};
constexpr Scheme kNoScheme = {0, nullptr};
template <int M>
constexpr Scheme scheme(const Punct<M> &p) { return {p.L * p.N, p.mask}; }

// flag[i] = 1 for every punctured bit i of the `total` unpunctured coded bits (the caller zeroes flag[0..total)): the
// first block under `pre`, then `repeat` blocks under `mn` (0: as many as cover the stretch between the first and the
// last block), the last block under `post`
constexpr void punctured_bits(uint8_t *flag, int total, Scheme pre, Scheme mn, Scheme post, int repeat)
{
	const int body_end = total - post.len;         // where the main scheme stops and the last block starts
	if (!repeat)
		repeat = (body_end - pre.len + mn.len - 1) / mn.len;
	int pos = 0;
	for (int k = 0; k < pre.len && pos < total; k++, pos++)
		if (pre.mask[k] == 0)
			flag[pos] = 1;
	for (int r = 0; r < repeat; r++)
		for (int k = 0; k < mn.len && pos < body_end; k++, pos++)
			if (mn.mask[k] == 0)
				flag[pos] = 1;
	// the last block starts at body_end wherever the main scheme stopped; the reference's guard on it is `position > 0`
	// (punct.c:121-124), kept
	pos = body_end;
	for (int k = 0; k < post.len && pos > 0; k++, pos++)
		if (post.mask[k] == 0)
			flag[pos] = 1;
}

// ---- scrambler (scramb.c:39-52): 15-bit LFSR, restarted for every burst; next() gives bit 0, 1, 2 ... ------
struct Scrambler {
	uint16_t reg = 0x4d4b;
	constexpr uint32_t next()
	{
		const uint32_t b = ((uint32_t)(reg >> 14) ^ reg) & 1u;
		reg = (uint16_t)((reg << 1) | b);
		return b;
	}
};
// the first N bits, for the table makers that look bits up by position
template <int N>
struct ScrambleSeq { bool bit[N]; };
template <int N>
constexpr ScrambleSeq<N> scramble_seq()
{
	ScrambleSeq<N> s{};
	Scrambler g;
	for (int i = 0; i < N; i++)
		s.bit[i] = g.next() != 0;
	return s;
}

// ---- positions -----------------------------------------------------------------------------------------------------
// intra-burst interleaver over 8 N bits (interleave.c:48-61, 73-87): coded bit k travels at position intra_pos(N, k);
// interleaving writes out[intra_pos] = in[k], de-interleaving reads out[k] = in[intra_pos]
constexpr int intra_pos(int N, int k) { return N * ((5 * k) & 7) + (k >> 3); }

// TCH3 (tch3.c:60-76): position of coded bit kc among the frame's 104 bits
constexpr int tch3_pos(int kc)
{
	const int ii = kc % 24, ij = kc / 24;
	return ii < 8 ? ij + 5 * ii : ij + 4 * ii + 8;
}

}  // namespace l1c
}  // namespace gmr1
