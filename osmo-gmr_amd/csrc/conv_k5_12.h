// conv_k5_12.h -- the BCCH / CCCH layer-1 chain behind the demodulator: constant tables (trellis steps, costs, CRC
// syndromes, the demodulator's soft-bit tables), branch metrics, the 16-state K=5 rate-1/2 Viterbi decoders
// (decode4_k5_12: four bursts a wave; decode1_k5_12_lat: one burst, latency shape), survivor walk + CRC16, L2 store.
#pragma once
#include "l1_codes.h"
#include "rx4_operands.h"
#include "wave_ops.h"

namespace gmr1 {

// the trellis-step descriptors (kSteps12, StepTable, make_steps) and their per-lane packing are written down in
// rx4_operands.h, which the host reads as well
__constant__ StepTable c_steps = make_steps();
// a lane's four descriptors of a chain as one 16-byte load (the fused batch kernel's request ahead of pass 2)
__device__ const Rx4Steps4 g_steps4 = make_steps4(make_steps());

// Viterbi input cost of one soft bit, libosmocore's generic decoder: ((in -+ 127)^2) >> 9, and 0 for
// an erasure (in == 0).  Index = soft bit as uint8, + 256 when the scrambler flips it (the flipped
// value is (int8)(-v), so -128 stays -128 exactly as in gmr1_scramble_sbit, scramb.c:63-73).
// a[]: first coded bit of a step, cost replicated to the bytes of the words ov = 0..3 it belongs
// to (byte ov holds c0 for ov < 2, c1 otherwise); b[]: second coded bit (c0 for even ov, c1 for odd).
struct CostTable { uint32_t a[512], b[512]; };
static constexpr CostTable make_cost()
{
	CostTable t{};
	for (int idx = 0; idx < 512; idx++) {
		int v = (int)(int8_t)(uint8_t)(idx & 255);
		if (idx & 256)
			v = (int)(int8_t)(uint8_t)(-v);
		const int e0 = v - 127, e1 = v + 127;
		const uint32_t c0 = v ? (uint32_t)((e0 * e0) >> 9) : 0u;
		const uint32_t c1 = v ? (uint32_t)((e1 * e1) >> 9) : 0u;
		t.a[idx] = c0 | (c0 << 8) | (c1 << 16) | (c1 << 24);
		t.b[idx] = c0 | (c1 << 8) | (c0 << 16) | (c1 << 24);
	}
	return t;
}
__constant__ CostTable c_cost = make_cost();

// The same for libosmocore's accelerated decoder (osmo_conv_decode_acc, decision D1b: oracle/orc_3p_acc.c).  It MAXIMISES
// the correlation sum in * (+-1); minimising  sum over the coded bits that contradict the soft bit's sign of |in|  ranks
// every pair of paths identically ((sum |in| - correlation) / 2, an integer) and is non-negative, so the packed
// [metric | decisions] words and v_min_u32 serve both decoders.  |in| <= 127 on the fused path (the demodulator's soft
// bits); two soft bits of -128 in one step would overflow a byte lane -- k_l1 takes 16-bit lanes in this mode.
static constexpr CostTable make_cost_acc()
{
	CostTable t{};
	for (int idx = 0; idx < 512; idx++) {
		int v = (int)(int8_t)(uint8_t)(idx & 255);
		if (idx & 256)
			v = (int)(int8_t)(uint8_t)(-v);
		const uint32_t c0 = v < 0 ? (uint32_t)(-v) : 0u;
		const uint32_t c1 = v > 0 ? (uint32_t)v : 0u;
		t.a[idx] = c0 | (c0 << 8) | (c1 << 16) | (c1 << 24);
		t.b[idx] = c0 | (c1 << 8) | (c0 << 16) | (c1 << 24);
	}
	return t;
}
__constant__ CostTable c_cost_acc = make_cost_acc();
// what the accelerated decoder gives state 0 as a start: 127 * N * K in correlation units (conv_acc.c reset_decoder),
// halved like the costs
constexpr uint32_t kAccLeadK5r2 = 127u * 2u * 5u / 2u;

struct SynTable { uint16_t s[208]; };
static constexpr SynTable make_syn()
{
	// CRC16 (init 0; reference src/l1/crc.c:58-63) is linear: the
	// check word of 192 message bits is the XOR of s[k] over the set bits k.
	// s[192+i] folds the received CRC bit i (MSB first) in, so that the XOR over
	// all 208 decoded bits is zero iff the check passes.
	SynTable t{};
	for (int k = 0; k < 192; k++)
		t.s[k] = (uint16_t)l1c::crc_unit(l1c::kCrc16, k, 192);
	for (int i = 0; i < 16; i++)
		t.s[192 + i] = (uint16_t)(1u << (15 - i));
	return t;
}
__constant__ SynTable c_syn = make_syn();

// the same table laid out for the decoder's CRC stage: lane `loc` of a row owns decoded bits
// 13 loc .. 13 loc + 12; w[loc][p] = s[13 loc + 2p] | s[13 loc + 2p + 1] << 16 (two 128-bit loads per lane)
struct SynRows { uint32_t w[16][8]; };
static constexpr SynRows make_syn_rows()
{
	const SynTable t = make_syn();
	SynRows r{};
	for (int loc = 0; loc < 16; loc++)
		for (int q = 0; q < 13; q++)
			r.w[loc][q >> 1] |= (uint32_t)t.s[13 * loc + q] << (16 * (q & 1));
	return r;
}
__constant__ __attribute__((aligned(16))) SynRows c_syn_rows = make_syn_rows();

// Soft bits of a pi/4-CQPSK symbol by table (pi4cxpsk.c:452-507): the two soft bits are a function of the symbol's
// phase quantised to 1/128 symbol (dq = round(|sv - round(sv)| * 128)) -- piecewise constant with every boundary on a
// multiple of 1/256 symbol.  Cell k of the table covers phases [k, k + 1) / 1024 turns (1 turn = 4 symbols) and holds
// what the arithmetic gives at the cell's midpoint (no ties there): nearest symbol sp (Gray bits p0 p1), its neighbour
// on the side of the phase, distance dq; the bit that differs between the two gets 127 - dq, the other 127 - dq/2.
// Entry = soft bit 0 | soft bit 1 << 8.  The arithmetic form and the table differ only for phases that are exactly a
// cell boundary in binary floating point.
struct SbLut { uint16_t v[1024]; };
static constexpr SbLut make_sb_lut()
{
	SbLut t{};
	for (int k = 0; k < 1024; k++) {
		int q = 2 * k + 1;                    // cell midpoint in 1/512 symbol; a turn is 2048
		if (q > 1024)
			q -= 2048;                        // (-2, 2] symbols
		const int n = (q + 256 + 2048) / 512 - 4;   // nearest symbol, floor((q + 256) / 512)
		const int dlq = 512 * n - q;          // round(sv) - sv, odd: never zero
		const int adl = dlq < 0 ? -dlq : dlq;
		const int dq = (adl + 2) / 4;         // round(|dl| * 128): adl / 4 = m + 1/4 or m + 3/4
		const unsigned sp = (unsigned)n & 3u;
		const unsigned neg = dlq < 0 ? 1u : 0u;
		const bool f0 = ((sp ^ neg ^ 1u) & 1u) != 0;
		const int m_near = 127 - dq, m_far = 127 - (dq >> 1);
		int v0 = f0 ? m_near : m_far;
		int v1 = f0 ? m_far : m_near;
		if (sp >> 1)
			v0 = -v0;
		if ((sp ^ (sp >> 1)) & 1u)
			v1 = -v1;
		t.v[k] = (uint16_t)(((unsigned)v0 & 0xffu) | (((unsigned)v1 & 0xffu) << 8));
	}
	return t;
}
__device__ __attribute__((aligned(16))) const SbLut g_sb_lut = make_sb_lut();
constexpr int kSbLutBytes = 2048;

// The same for pi/4-CBPSK (one bit per symbol, a turn is two symbols; pi4cxpsk.c:452-507 with nbits = 1): the symbol's
// one soft bit is 127 - dq (its neighbour always differs in that bit), negative for symbol 1.  Entry = the soft bit in
// the low byte; cells and boundaries as above (dq steps at odd multiples of 1/256 symbol, cell edges at multiples of 1/512).
static constexpr SbLut make_sb_lut1()
{
	SbLut t{};
	for (int k = 0; k < 1024; k++) {
		int q = 2 * k + 1;                    // cell midpoint in 1/1024 symbol; a turn is 2048
		if (q > 1024)
			q -= 2048;                        // (-1, 1] symbols
		const int n = (q + 512 + 2048) / 1024 - 2;  // nearest symbol, floor((q + 512) / 1024)
		const int dlq = 1024 * n - q;         // round(sv) - sv, odd: never zero
		const int adl = dlq < 0 ? -dlq : dlq;
		const int dq = (adl + 4) / 8;         // round(|dl| * 128): adl / 8 is never half an integer
		const unsigned sp = (unsigned)n & 1u;
		const int v0 = sp ? -(127 - dq) : (127 - dq);
		t.v[k] = (uint16_t)((unsigned)v0 & 0xffu);
	}
	return t;
}
__device__ __attribute__((aligned(16))) const SbLut g_sb_lut1 = make_sb_lut1();

// K=5 rate-1/2 code (g0 = 1+D^3+D^4, g1 = 1+D+D^2+D^4; reference src/l1/conv.c:123-145)
__device__ __forceinline__ uint32_t out_k5_12(uint32_t s, uint32_t b)
{
	constexpr uint32_t g0 = l1c::kK5_12[0], g1 = l1c::kK5_12[1];
	uint32_t reg = (s << 1) | b;
	return ((uint32_t)(__popc(reg & g0) & 1) << 1) | (uint32_t)(__popc(reg & g1) & 1);
}
__device__ __forceinline__ uint32_t rotl4(uint32_t x, int r) { return ((x << r) | (x >> (4 - r))) & 15u; }

// ---------------------------------------------------------------------------
// branch metrics of one burst into bm[0..212): byte ov = cost of coded word ov
// (descramble + de-interleave folded into the gather via c_steps)
//   bcch.c:91-92 / ccch.c:95-96, interleave.c:73-87, scramb.c:63-73
// ---------------------------------------------------------------------------
template <bool ACC = false>
__device__ __forceinline__ void branch_metrics_k5_12(const int8_t *__restrict__ eb, int chain,
                                                     uint32_t *__restrict__ bm, int lane)
{
	const CostTable &ct = ACC ? c_cost_acc : c_cost;
	for (int k = lane; k < kSteps12; k += 64) {
		const uint32_t st = c_steps.w[chain][k];
		// the four byte sums c(a) + c(b) of a step come out of one add of two table words
		const uint32_t ia = (uint32_t)(uint8_t)eb[st & 0x3ffu] | ((st >> 2) & 0x100u);
		const uint32_t ib = (uint32_t)(uint8_t)eb[(st >> 16) & 0x3ffu] | ((st >> 18) & 0x100u);
		bm[k] = ct.a[ia] + ct.b[ib];
	}
}

// the four bursts of a fused wave at once: every lane owns steps lane + 64 it of each burst, and the
// three dependent fetches (step descriptor -> soft bits -> cost words) are each issued for all 16
// (burst, step) pairs before anything waits -- three memory round trips per wave instead of 48
// (steps(c, it): the descriptor of step lane + 64 it of chain c, 0 beyond the last step; the two forms below say where from)
template <bool ACC, class Steps>
__device__ __forceinline__ void branch_metrics4_k5_12_from(const int8_t *__restrict__ eb, int eb_stride, int row_ok,
                                                           int row_chain, uint32_t *__restrict__ bm, int lane, Steps steps)
{
	const CostTable &ct = ACC ? c_cost_acc : c_cost;
	uint32_t st[2][4];
#pragma unroll
	for (int c = 0; c < 2; c++)
#pragma unroll
		for (int it = 0; it < 4; it++)
			st[c][it] = steps(c, it);
	uint32_t ia[4][4], ib[4][4];
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const bool ch = ((row_chain >> q) & 1) != 0;
		const int8_t *e = eb + q * eb_stride;
#pragma unroll
		for (int it = 0; it < 4; it++) {
			const uint32_t s = ch ? st[1][it] : st[0][it];
			ia[q][it] = (uint32_t)(uint8_t)e[s & 0x3ffu] | ((s >> 2) & 0x100u);
			ib[q][it] = (uint32_t)(uint8_t)e[(s >> 16) & 0x3ffu] | ((s >> 18) & 0x100u);
		}
	}
	uint32_t va[4][4], vb[4][4];
#pragma unroll
	for (int q = 0; q < 4; q++)
#pragma unroll
		for (int it = 0; it < 4; it++) {
			va[q][it] = ct.a[ia[q][it]];
			vb[q][it] = ct.b[ib[q][it]];
		}
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const bool ok = ((row_ok >> q) & 1) != 0;
#pragma unroll
		for (int it = 0; it < 4; it++) {
			const int k = lane + 64 * it;
			if (k < kSteps12)
				bm[q * kSteps12 + k] = ok ? va[q][it] + vb[q][it] : 0u;
		}
	}
}

// the descriptors read from c_steps here, a memory trip of their own in front of the other two
template <bool ACC = false>
__device__ __forceinline__ void branch_metrics4_k5_12(const int8_t *__restrict__ eb, int eb_stride, int row_ok,
                                                      int row_chain, uint32_t *__restrict__ bm, int lane)
{
	branch_metrics4_k5_12_from<ACC>(eb, eb_stride, row_ok, row_chain, bm, lane, [&](int c, int it) -> uint32_t {
		const int k = lane + 64 * it;
		return k < kSteps12 ? c_steps.w[c][k] : 0u;
	});
}

// the descriptors already in registers: st0 / st1 = the lane's g_steps4 entries of chain 0 / 1, which the caller asked for
// ahead of its own waits
template <bool ACC = false>
__device__ __forceinline__ void branch_metrics4_k5_12(const int8_t *__restrict__ eb, int eb_stride, int row_ok,
                                                      int row_chain, uint32_t *__restrict__ bm, int lane,
                                                      const uint4 st0, const uint4 st1)
{
	branch_metrics4_k5_12_from<ACC>(eb, eb_stride, row_ok, row_chain, bm, lane, [&](int c, int it) -> uint32_t {
		const uint4 v = c ? st1 : st0;
		return it == 0 ? v.x : (it == 1 ? v.y : (it == 2 ? v.z : v.w));
	});
}

// ---------------------------------------------------------------------------
// 4 x (K=5, rate 1/2, 208 bits + flush) Viterbi, one burst per 16-lane row
//
// In-place butterfly: the two predecessors of a state always sit in two lanes of the row that
// differ by an xor mask, and the two successor states are written back to the same two lanes.
// The masks of the four phases are 8, 7, 2, 1 -- each ONE DPP control (row_ror:8,
// row_half_mirror, quad_perm), so the partner's metric arrives folded into the add.  With
// loc = c0*8 ^ c1*7 ^ c2*2 ^ c3*1, the predecessor state held by a lane in phase ph has bit i =
// c[(3 - i + ph) & 3]; after 4 steps the layout is back where it started.
//
// One 32-bit word per state carries everything the step needs:
//     [ path metric : 16 | decisions of the current 16-step window : 16 ]
// The metric never exceeds 212 * 252 = 53 424; unreachable states carry 0xF000 (libosmocore's
// MAX_AE plays the same role).  In step j of a window a lane that is the HIGH predecessor
// ((t >> 1) + 8) of its butterfly adds bit j (tb) to what it sends on.  Lanes exchange CANDIDATES,
// not words: each lane forms  own word + (cost << 16) + tb  twice, once with the cost of its
// transition into its own successor and once with that into the PARTNER's successor, and the
// v_min_u32 that takes the partner's candidate through DPP then (a) picks the smaller metric,
// (b) on equal metrics keeps the LOW predecessor (osmo_conv_decode: strict '>' on ascending
// states), and (c) leaves the decision in bit j of the winner's history -- three VALU
// instructions per trellis step (two v_add3_u32, v_min_u32 with DPP); the word carries no tb
// between steps, and a window ends with a plain clear of the low half.  (Pulling the partner's
// WORD through DPP instead needs its tb inside the word before it travels: a fourth instruction
// per step.)  A VGPR written by a VALU instruction must not be read through DPP by the next two
// instructions: the partner-bound candidate is formed first, and the second add plus the two cost
// prefetches (or an s_nop) stand between it and the min.  The cost byte is fetched by every lane
// straight from the branch-metric words in LDS into the HIGH half of a register
// (ds_read_u8_d16_hi; with SRAM-ECC the low half reads back as zero, which is what the add
// wants), 8 steps ahead.
//
// The decision of step k is the oldest bit of the winning predecessor = input bit u[k-4].
// Windows start at k = 4 + 16 m, so window m's 16 decisions ARE the decoded bits
// u[16 m .. 16 m + 15], and its low 4 bits name the survivor's state at the start of the
// window: the "traceback" is 13 dependent 16-bit LDS reads per burst.
// ---------------------------------------------------------------------------
constexpr uint32_t kSentinel = 0xF0000000u;

// per row location: bits 0-7 cost byte of the transition own predecessor -> own successor (2 bits per phase), 8-15 cost
// byte of own predecessor -> the PARTNER's successor, 16-31 the 16-step tb pattern (bit j set when the lane holds a HIGH
// predecessor in phase j & 3)
struct DecTable { uint32_t v[16]; };
static constexpr uint32_t dec_out(uint32_t s, uint32_t b)
{
	return l1c::conv_word(l1c::kK5_12, (s << 1) | b);
}
// the predecessor state a row location holds in phase ph (loc in the basis {8, 7, 2, 1})
static constexpr uint32_t dec_state(uint32_t loc, int ph)
{
	uint32_t c[4] = {0, 0, 0, 0};
	c[0] = (loc >> 3) & 1u;
	uint32_t x = loc & 7u;
	c[1] = (x >> 2) & 1u;
	x ^= c[1] ? 7u : 0u;
	c[2] = (x >> 1) & 1u;
	c[3] = x & 1u;
	uint32_t sp = 0;
	for (int i = 0; i < 4; i++)
		sp |= c[(3 - i + ph) & 3] << i;
	return sp;
}
static constexpr DecTable make_dec()
{
	DecTable t{};
	for (uint32_t loc = 0; loc < 16; loc++) {
		uint32_t e = 0;
		for (int ph = 0; ph < 4; ph++) {
			// the lane's successor takes input bit b, the partner's (predecessor sp ^ 8) input bit b ^ 1
			const uint32_t sp = dec_state(loc, ph);
			const uint32_t b = sp >> 3;
			e |= dec_out(sp, b) << (2 * ph);
			e |= dec_out(sp, b ^ 1u) << (8 + 2 * ph);
			for (int j = ph; j < 16; j += 4)
				e |= b << (16 + j);
		}
		t.v[loc] = e;
	}
	return t;
}
// What the partner lane (loc ^ {8, 7, 2, 1}[ph]) sends is what this lane used to add to the partner's word itself: the
// cost of the partner's predecessor -> this lane's successor.  Both generators have the D^0 and D^4 taps, so that is
// also the lane's own bits 8-15 (k_l1_acc reads them as the partner's cost into the own successor).
static constexpr bool dec_exchange_holds()
{
	const DecTable t = make_dec();
	const uint32_t mask[4] = {8u, 7u, 2u, 1u};
	for (uint32_t loc = 0; loc < 16; loc++)
		for (int ph = 0; ph < 4; ph++) {
			const uint32_t sp = dec_state(loc, ph);
			const uint32_t partner_into_mine = dec_out(sp ^ 8u, sp >> 3);
			if (dec_state(loc ^ mask[ph], ph) != (sp ^ 8u))
				return false;
			if (((t.v[loc ^ mask[ph]] >> (8 + 2 * ph)) & 3u) != partner_into_mine)
				return false;
			if (((t.v[loc] >> (8 + 2 * ph)) & 3u) != partner_into_mine)
				return false;
		}
	return true;
}
static_assert(dec_exchange_holds(), "the partner lane's bits 8-15 must name the cost of its predecessor into this lane's successor");
__constant__ DecTable c_dec = make_dec();

#define GMR1_DPP_PH0 "row_ror:8"
#define GMR1_DPP_PH1 "row_half_mirror"
#define GMR1_DPP_PH2 "quad_perm:[2,3,0,1]"
#define GMR1_DPP_PH3 "quad_perm:[1,0,3,2]"

// both outgoing candidates of the lane: S to the partner's successor, T1 to its own
#define ACS_CAND                                                                                   \
	"s_waitcnt lgkmcnt(%[wt])\n\t"                                                                  \
	"v_add3_u32 %[s], %[w], %[x], %[t]\n\t"                                                         \
	"v_add3_u32 %[t1], %[w], %[r], %[t]\n\t"
#define ACS_MIN(PH)                                                                                \
	"v_min_u32_dpp %[w], %[s], %[t1] " GMR1_DPP_PH##PH " row_mask:0xf bank_mask:0xf\n\t"
// step with the operands of position J, prefetching the cost bytes of step J + 8; TB = tb of the position
#define ACS_PF(J, PH, WAIT, TB)                                                                    \
	asm volatile(ACS_CAND                                                                          \
	             "ds_read_u8_d16_hi %[rn], %[ao] offset:%[off]\n\t"                                 \
	             "ds_read_u8_d16_hi %[xn], %[ap] offset:%[off]\n\t"                                 \
	             ACS_MIN(PH)                                                                       \
	             : [w] "+v"(w), [rn] "+v"(R[((J) + 8) & 15]), [xn] "+v"(X[((J) + 8) & 15]),        \
	               [t1] "=&v"(t1), [s] "=&v"(s)                                                      \
	             : [r] "v"(R[J]), [x] "v"(X[J]), [ao] "v"(ao[PH]), [ap] "v"(ap[PH]), [t] "v"(TB),    \
	               [off] "i"(4 * ((J) + 8)), [wt] "i"(WAIT))
// step without prefetch: the s_nop is the second wait state between the write of S and its read through DPP
#define ACS_NP(J, PH, WAIT, TB)                                                                    \
	asm volatile(ACS_CAND                                                                          \
	             "s_nop 0\n\t"                                                                      \
	             ACS_MIN(PH)                                                                       \
	             : [w] "+v"(w), [t1] "=&v"(t1), [s] "=&v"(s)                                         \
	             : [r] "v"(R[J]), [x] "v"(X[J]), [t] "v"(TB), [wt] "i"(WAIT))
// cost bytes of step K (relative to the address registers) into the operands of position J
#define ACS_LOAD(J, PH, K)                                                                         \
	asm volatile("ds_read_u8_d16_hi %[rn], %[ao] offset:%[off]\n\t"                                 \
	             "ds_read_u8_d16_hi %[xn], %[ap] offset:%[off]\n\t"                                 \
	             : [rn] "+v"(R[J]), [xn] "+v"(X[J])                                                  \
	             : [ao] "v"(ao[PH]), [ap] "v"(ap[PH]), [off] "i"(4 * (K)))

struct DecPre;
__device__ __forceinline__ void k5_12_survivors_crc(uint64_t *__restrict__ surv, uint32_t *__restrict__ ubits, int lane,
                                                    uint32_t &syn_o, const DecPre *dp = nullptr);
__device__ __forceinline__ void k5_12_survivors_crc_lat(uint64_t *__restrict__ surv, uint32_t *__restrict__ ubits, int lane,
                                                        uint32_t &syn_o, const DecPre *dp);

// bm: 4 rows x 212 words; surv: 13 x 64 halfwords of window decisions; ubits: 4 rows x 8 words
// (decoded bits, LSB first)
//
// ACC = libosmocore's accelerated decoder instead of its generic one (decision D1b, oracle/orc_3p_acc.c; costs from
// c_cost_acc): every start state is allowed, state 0 leading by 127 * N * K; the four flush steps are ordinary
// butterflies (the survivor walk still starts in state 0); no path metric is returned.  Ties between the two paths into
// a state fall to the same (lower) predecessor in both decoders.
struct DecPre {                                    // the decoder's per-lane constants, when the caller keeps them (receive loop)
	uint32_t dc;
	uint4 sy0, sy1;
#ifdef GMR1_HIP_PROFILE
	unsigned long long *stamp = nullptr;
#endif
};
#ifdef GMR1_HIP_PROFILE
#define GMR1_DSTAMP(dp, k, lane)                                             \
	do {                                                                    \
		if ((dp)->stamp && (lane) == 0)                                     \
			(dp)->stamp[k] = __builtin_readcyclecounter();                  \
	} while (0)
#else
#define GMR1_DSTAMP(dp, k, lane) do { } while (0)
#endif

template <bool ACC = false>
__device__ void decode4_k5_12(const uint32_t *__restrict__ bm, uint64_t *__restrict__ surv,
                              uint32_t *__restrict__ ubits, int lane, uint32_t &syn_o, uint32_t &final_ae,
                              const DecPre *dp = nullptr)
{
	typedef __attribute__((address_space(3))) const unsigned char lds_cbyte;
	const int row = lane >> 4;
	const uint32_t loc = (uint32_t)lane & 15u;
	// per-location constants (c_dec): cost byte of the transition into the own / the partner's successor per phase, tb pattern
	const uint32_t dc = dp ? dp->dc : c_dec.v[loc];
	const uint32_t row_base = (uint32_t)(uintptr_t)(lds_cbyte *)(bm + row * kSteps12);
	uint32_t ao[4], ap[4];      // LDS byte address of this lane's cost into its own / the partner's successor in step 0 of the phase
	bool hi[4];
#pragma unroll
	for (int ph = 0; ph < 4; ph++) {
		ao[ph] = row_base + ((dc >> (2 * ph)) & 3u);
		ap[ph] = row_base + ((dc >> (8 + 2 * ph)) & 3u);
		hi[ph] = ((dc >> (16 + ph)) & 1u) != 0;
	}
	// cost << 16 of the transition into the own / the partner's successor, per window position (low halves stay zero
	// whether or not the d16 load preserves them)
	uint32_t R[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, X[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t T[16];             // tie-break / decision bit of the position: set in HIGH-predecessor lanes
#pragma unroll
	for (int j = 0; j < 16; j++)
		T[j] = (dc >> 16) & (1u << j);
	uint32_t w = loc ? (ACC ? kAccLeadK5r2 << 16 : kSentinel) : 0u;
	uint32_t t1, s;
	uint16_t *dump = reinterpret_cast<uint16_t *>(surv) + lane;

	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	// steps 0..3: the decisions are u[-4..-1], dropped
	ACS_LOAD(0, 0, 0); ACS_LOAD(1, 1, 1); ACS_LOAD(2, 2, 2); ACS_LOAD(3, 3, 3);
	ACS_NP(0, 0, 6, T[0]); ACS_NP(1, 1, 4, T[1]); ACS_NP(2, 2, 2, T[2]); ACS_NP(3, 3, 0, T[3]);
	w &= 0xffff0000u;
#pragma unroll
	for (int ph = 0; ph < 4; ph++) {
		ao[ph] += 16;
		ap[ph] += 16;
	}
	// window pipeline: the costs of 8 steps are always in flight
	ACS_LOAD(0, 0, 0); ACS_LOAD(1, 1, 1); ACS_LOAD(2, 2, 2); ACS_LOAD(3, 3, 3);
	ACS_LOAD(4, 0, 4); ACS_LOAD(5, 1, 5); ACS_LOAD(6, 2, 6); ACS_LOAD(7, 3, 7);
#pragma unroll 1
	for (int m = 0; m < 12; m++) {
		ACS_PF(0, 0, 14, T[0]); ACS_PF(1, 1, 14, T[1]); ACS_PF(2, 2, 14, T[2]); ACS_PF(3, 3, 14, T[3]);
		ACS_PF(4, 0, 14, T[4]); ACS_PF(5, 1, 14, T[5]); ACS_PF(6, 2, 14, T[6]); ACS_PF(7, 3, 14, T[7]);
		ACS_PF(8, 0, 14, T[8]); ACS_PF(9, 1, 14, T[9]); ACS_PF(10, 2, 14, T[10]); ACS_PF(11, 3, 14, T[11]);
		ACS_PF(12, 0, 14, T[12]); ACS_PF(13, 1, 14, T[13]); ACS_PF(14, 2, 14, T[14]); ACS_PF(15, 3, 14, T[15]);
		dump[m * 64] = (uint16_t)w;
		w &= 0xffff0000u;
#pragma unroll
		for (int ph = 0; ph < 4; ph++) {
			ao[ph] += 64;
			ap[ph] += 64;
		}
	}
	// window 12: steps 196..211, the last four are the flush (b = 0 transitions only: the lanes
	// whose new state ends in 1 become unreachable)
	ACS_PF(0, 0, 14, T[0]); ACS_PF(1, 1, 14, T[1]); ACS_PF(2, 2, 14, T[2]); ACS_PF(3, 3, 14, T[3]);
	ACS_PF(4, 0, 14, T[4]); ACS_PF(5, 1, 14, T[5]); ACS_PF(6, 2, 14, T[6]); ACS_PF(7, 3, 14, T[7]);
	ACS_NP(8, 0, 14, T[8]); ACS_NP(9, 1, 12, T[9]); ACS_NP(10, 2, 10, T[10]); ACS_NP(11, 3, 8, T[11]);
	if constexpr (ACC) {
		ACS_NP(12, 0, 6, T[12]); ACS_NP(13, 1, 4, T[13]); ACS_NP(14, 2, 2, T[14]); ACS_NP(15, 3, 0, T[15]);
		(void)hi;
	} else {
		// (a lane just made unreachable sends the bare sentinel on, without a tb)
		ACS_NP(12, 0, 6, T[12]);
		w = hi[0] ? kSentinel : w;
		ACS_NP(13, 1, 4, hi[0] ? 0u : T[13]);
		w = hi[1] ? kSentinel : w;
		ACS_NP(14, 2, 2, hi[1] ? 0u : T[14]);
		w = hi[2] ? kSentinel : w;
		ACS_NP(15, 3, 0, hi[2] ? 0u : T[15]);
		w = hi[3] ? kSentinel : w;
	}
	dump[12 * 64] = (uint16_t)w;
	// state 0 ends in location 0 of the row; osmo_conv_decode_acc returns 0, not a metric
	final_ae = ACC ? 0u : w >> 16;
	k5_12_survivors_crc(surv, ubits, lane, syn_o, dp);
}

// The K=5 rate-1/2 decoder shaped for the LATENCY of one burst (the receive loop: a wave alone on its SIMD issues one
// instruction every four to five cycles whatever the dependences, so a round costs what its instruction count says).
// The batch decoder above spends 6 instructions per trellis step (wait, two adds, min with DPP, two cost-byte reads).  Here a step's operands come ready-made from a table the branch-metric phase expands once per burst:
// per step and code word two 8-byte entries (this lane the HIGH predecessor or not) -- both generators have the D^0 and D^4
// taps, so the partner's code word is the own one's complement -- holding  own cost << 16 | tie-break bit if this lane is the
// HIGH predecessor,  partner's cost << 16 | tie-break bit if the partner is.  One ds_read_b64 and three VALU per step: 5
// instructions.  212 x 64 B of LDS, which only the loop (one burst per work-group) can afford.  Arithmetic, ties and
// decisions are the batch decoder's.
static constexpr bool dec_partner_is_complement()
{
	const DecTable t = make_dec();
	for (int loc = 0; loc < 16; loc++)
		for (int ph = 0; ph < 4; ph++)
			if (((t.v[loc] >> (8 + 2 * ph)) & 3u) != (((t.v[loc] >> (2 * ph)) & 3u) ^ 3u))
				return false;
	return true;
}
static_assert(dec_partner_is_complement(), "the partner transition's code word must be the own one's complement");
typedef uint32_t lat_u32x2 __attribute__((ext_vector_type(2)));
constexpr int kLatTabBytes = kSteps12 * 64;
#define ACSL_CORE(PH)                                                                              \
	".if %[wt] >= 0\n\t"                                                                            \
	"s_waitcnt lgkmcnt(%[wt])\n\t"                                                                  \
	".endif\n\t"                                                                                    \
	"v_add_u32 %[t1], %[w], %[r]\n\t"                                                               \
	"v_add_u32_dpp %[t2], %[w], %[q] " GMR1_DPP_PH##PH " row_mask:0xf bank_mask:0xf\n\t"            \
	"v_min_u32 %[w], %[t1], %[t2]\n\t"
#define ACSL_PF(J, PH, WAIT)                                                                       \
	asm volatile(ACSL_CORE(PH)                                                                     \
	             "ds_read_b64 %[rqn], %[a] offset:%[off]\n\t"                                       \
	             : [w] "+v"(w), [rqn] "=v"(RQ[((J) + 8) & 15]), [t1] "=&v"(t1), [t2] "=&v"(t2)        \
	             : [r] "v"(RQ[J].x), [q] "v"(RQ[J].y), [a] "v"(A[PH]), [off] "i"(16 * ((J) + 8)), [wt] "i"(WAIT))
#define ACSL_NP(J, PH, WAIT)                                                                       \
	asm volatile(ACSL_CORE(PH)                                                                     \
	             : [w] "+v"(w), [t1] "=&v"(t1), [t2] "=&v"(t2)                                       \
	             : [r] "v"(RQ[J].x), [q] "v"(RQ[J].y), [wt] "i"(WAIT))
#define ACSL_LOAD(J, PH, K)                                                                        \
	asm volatile("ds_read_b64 %[rqn], %[a] offset:%[off]\n\t" : [rqn] "=v"(RQ[J]) : [a] "v"(A[PH]), [off] "i"(16 * (K)))

// one step's eight entries from its cost word (byte j = cost of code word j): cls = 2 * code word + HIGH
__device__ __forceinline__ void lat_expand_step(uint32_t *__restrict__ tab, int k, uint32_t word)
{
	const uint32_t bit = 1u << (k < 4 ? k : ((k - 4) & 15));
	const uint32_t c0 = (word << 16) & 0x00ff0000u, c1 = (word << 8) & 0x00ff0000u, c2 = word & 0x00ff0000u,
	               c3 = (word >> 8) & 0x00ff0000u;
	// code-word-major ([j][step], 16 bytes each: not HIGH {c_j, c_(3-j) | bit}, HIGH {c_j | bit, c_(3-j)}): lanes own
	// consecutive steps, so a wave's 16-byte writes are consecutive in LDS (step-major they were 64 bytes apart: eight-way
	// bank conflicts, 1 400 cycles)
	uint4 *d = reinterpret_cast<uint4 *>(tab) + k;
	d[0 * kSteps12] = make_uint4(c0, c3 | bit, c0 | bit, c3);
	d[1 * kSteps12] = make_uint4(c1, c2 | bit, c1 | bit, c2);
	d[2 * kSteps12] = make_uint4(c2, c1 | bit, c2 | bit, c1);
	d[3 * kSteps12] = make_uint4(c3, c0 | bit, c3 | bit, c0);
}

// TAIL = false: the forward pass alone -- window words to `surv`, the final metric returned; the survivor walk and the CRC
// (k5_12_survivors_crc_lat) are the caller's, on another wave (k_rx_chain_pipe)
template <bool ACC = false, bool TAIL = true>
__device__ void decode1_k5_12_lat(const uint32_t *__restrict__ tab, uint64_t *__restrict__ surv,
                                  uint32_t *__restrict__ ubits, int lane, uint32_t &syn_o, uint32_t &final_ae,
                                  const DecPre *dp)
{
	typedef __attribute__((address_space(3))) const unsigned char lds_cbyte;
	const uint32_t loc = (uint32_t)lane & 15u;
	const uint32_t dc = dp->dc;
	const uint32_t base = (uint32_t)(uintptr_t)(lds_cbyte *)tab;
	uint32_t A[4];              // LDS byte address of this lane's entry in step 0 of the phase
	bool hi[4];
#pragma unroll
	for (int ph = 0; ph < 4; ph++) {
		hi[ph] = ((dc >> (16 + ph)) & 1u) != 0;
		A[ph] = base + (uint32_t)(kSteps12 * 16) * ((dc >> (2 * ph)) & 3u) + (hi[ph] ? 8u : 0u);
	}
	lat_u32x2 RQ[16];
	uint32_t w = loc ? (ACC ? kAccLeadK5r2 << 16 : kSentinel) : 0u;
	uint32_t t1, t2;
	uint16_t *dump = reinterpret_cast<uint16_t *>(surv) + lane;

	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	// steps 0..3: the decisions are u[-4..-1], dropped
	ACSL_LOAD(0, 0, 0); ACSL_LOAD(1, 1, 1); ACSL_LOAD(2, 2, 2); ACSL_LOAD(3, 3, 3);
	ACSL_NP(0, 0, 3); ACSL_NP(1, 1, 2); ACSL_NP(2, 2, 1); ACSL_NP(3, 3, 0);
	w &= 0xffff0000u;
#pragma unroll
	for (int ph = 0; ph < 4; ph++)
		A[ph] += 4 * 16;
	// window pipeline: the operands of 8 steps are always in flight
	ACSL_LOAD(0, 0, 0); ACSL_LOAD(1, 1, 1); ACSL_LOAD(2, 2, 2); ACSL_LOAD(3, 3, 3);
	ACSL_LOAD(4, 0, 4); ACSL_LOAD(5, 1, 5); ACSL_LOAD(6, 2, 6); ACSL_LOAD(7, 3, 7);
#pragma unroll 1
	for (int m = 0; m < 12; m++) {
		// (one wait per four steps: eight loads are in flight, the four oldest must have landed)
		ACSL_PF(0, 0, 4); ACSL_PF(1, 1, -1); ACSL_PF(2, 2, -1); ACSL_PF(3, 3, -1);
		ACSL_PF(4, 0, 4); ACSL_PF(5, 1, -1); ACSL_PF(6, 2, -1); ACSL_PF(7, 3, -1);
		ACSL_PF(8, 0, 4); ACSL_PF(9, 1, -1); ACSL_PF(10, 2, -1); ACSL_PF(11, 3, -1);
		ACSL_PF(12, 0, 4); ACSL_PF(13, 1, -1); ACSL_PF(14, 2, -1); ACSL_PF(15, 3, -1);
		dump[m * 64] = (uint16_t)w;
		w &= 0xffff0000u;
#pragma unroll
		for (int ph = 0; ph < 4; ph++)
			A[ph] += 16 * 16;
	}
	// window 12: steps 196..211, the last four are the flush (generic decoder: b = 0 transitions only -- the lanes whose new
	// state ends in 1 become unreachable)
	ACSL_PF(0, 0, 4); ACSL_PF(1, 1, -1); ACSL_PF(2, 2, -1); ACSL_PF(3, 3, -1);
	ACSL_PF(4, 0, 4); ACSL_PF(5, 1, -1); ACSL_PF(6, 2, -1); ACSL_PF(7, 3, -1);
	ACSL_NP(8, 0, 4); ACSL_NP(9, 1, -1); ACSL_NP(10, 2, -1); ACSL_NP(11, 3, -1);
	if constexpr (ACC) {
		ACSL_NP(12, 0, 0); ACSL_NP(13, 1, -1); ACSL_NP(14, 2, -1); ACSL_NP(15, 3, -1);
		(void)hi;
	} else {
		ACSL_NP(12, 0, 0);
		w = hi[0] ? kSentinel : w;
		ACSL_NP(13, 1, -1);
		w = hi[1] ? kSentinel : w;
		ACSL_NP(14, 2, -1);
		w = hi[2] ? kSentinel : w;
		ACSL_NP(15, 3, -1);
		w = hi[3] ? kSentinel : w;
	}
	dump[12 * 64] = (uint16_t)w;
	final_ae = ACC ? 0u : w >> 16;
	GMR1_DSTAMP(dp, 12, lane);
	if constexpr (TAIL)
		k5_12_survivors_crc_lat(surv, ubits, lane, syn_o, dp);
	else
		syn_o = 0;
}

// Tail of the decoder shaped for the LATENCY of one burst (the receive loop: one burst per wave, nothing to overlap with):
// the 13 window words of every location are read at once and the survivor chain is walked with v_readlane on scalars --
// 13 dependent LDS round trips become one.  Row 0 only; the CRC as in k5_12_survivors_crc.
__device__ __forceinline__ void k5_12_survivors_crc_lat(uint64_t *__restrict__ surv, uint32_t *__restrict__ ubits, int lane,
                                                        uint32_t &syn_o, const DecPre *dp)
{
	const int row = lane >> 4;
	const uint32_t loc = (uint32_t)lane & 15u;
	WSYNC();
	// survivor chain of row 0: every location's 13 window words at once, then the walk on scalars
	{
		constexpr unsigned long long kLocOf =
			0x0ull | (0x8ull << 4) | (0x7ull << 8) | (0xFull << 12) | (0x2ull << 16) | (0xAull << 20) |
			(0x5ull << 24) | (0xDull << 28) | (0x1ull << 32) | (0x9ull << 36) | (0x6ull << 40) |
			(0xEull << 44) | (0x3ull << 48) | (0xBull << 52) | (0x4ull << 56) | (0xCull << 60);
		const uint16_t *d16 = reinterpret_cast<const uint16_t *>(surv) + loc;      // (rows 1-3 read row 0's words too)
		uint32_t H[13];
#pragma unroll
		for (int m = 0; m < 13; m++)
			H[m] = d16[m * 64];
		uint32_t L = 0, hv[13];
#pragma unroll
		for (int m = 12; m >= 0; m--) {
			hv[m] = (uint32_t)__builtin_amdgcn_readlane((int)H[m], (int)L);
			L = (uint32_t)(kLocOf >> (4 * (hv[m] & 15u))) & 15u;
		}
		if (lane == 0) {
#pragma unroll
			for (int m = 0; m < 13; m += 2)
				ubits[m >> 1] = hv[m] | (m == 12 ? 0u : (hv[m + 1] << 16));
		}
	}
	WSYNC();
	GMR1_DSTAMP(dp, 13, lane);
	// CRC16 over the 208 decoded bits, 13 bits per lane of the row, XOR-reduced with DPP (as in k5_12_survivors_crc)
	uint32_t syn = 0;
	{
		const uint32_t *ub = ubits + row * 8;
		const uint32_t k0 = loc * 13u;
		const uint32_t lo = ub[k0 >> 5], hi2 = ub[(k0 >> 5) + 1];
		const uint32_t cbits = __builtin_amdgcn_alignbit(hi2, lo, k0 & 31u);
		const uint32_t sy[7] = {dp->sy0.x, dp->sy0.y, dp->sy0.z, dp->sy0.w, dp->sy1.x, dp->sy1.y, dp->sy1.z};
		uint32_t acc = 0;
#pragma unroll
		for (int pq = 0; pq < 7; pq++) {
			const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)cbits, 2 * pq, 1);
			const uint32_t m1 = pq < 6 ? (uint32_t)__builtin_amdgcn_sbfe((int)cbits, 2 * pq + 1, 1) : 0u;
			acc ^= sy[pq] & ((m0 & 0xffffu) | (m1 & 0xffff0000u));
		}
		syn = (acc ^ (acc >> 16)) & 0xffffu;
		syn ^= row_xor<1>(syn);
		syn ^= row_xor<2>(syn);
		syn ^= row_xor<4>(syn);
		syn ^= row_xor<8>(syn);
	}
	syn_o = syn;
}

// second half of the decoder: survivor chain and CRC16 of the four rows (shared with the 16-bit-lane forward pass below)
__device__ __forceinline__ void k5_12_survivors_crc(uint64_t *__restrict__ surv, uint32_t *__restrict__ ubits, int lane,
                                                    uint32_t &syn_o, const DecPre *dp)
{
	const int row = lane >> 4;
	const uint32_t loc = (uint32_t)lane & 15u;
	// this lane's CRC syndrome words travel while the survivor chain is walked
	const uint4 sy0 = dp ? dp->sy0 : *reinterpret_cast<const uint4 *>(&c_syn_rows.w[loc][0]);
	const uint4 sy1 = dp ? dp->sy1 : *reinterpret_cast<const uint4 *>(&c_syn_rows.w[loc][4]);
	WSYNC();

	// survivor chain, one lane per row: window m's decisions at the survivor's location are the
	// decoded bits u[16 m ..]; their low nibble (u[16m-4 .. 16m-1] seen from window m) is the state
	// at the start of the window, bit-reversed: h0 -> state bit 3 -> basis vector 8, h1 -> 7,
	// h2 -> 2, h3 -> 1  (osmo_conv_decode_get_output, end state 0 after flush)
	if (loc == 0) {
		const uint16_t *d16 = reinterpret_cast<const uint16_t *>(surv) + row * 16;
		// location of the state whose reversed nibble is x, x = 0..15
		constexpr unsigned long long kLocOf =
			0x0ull | (0x8ull << 4) | (0x7ull << 8) | (0xFull << 12) | (0x2ull << 16) | (0xAull << 20) |
			(0x5ull << 24) | (0xDull << 28) | (0x1ull << 32) | (0x9ull << 36) | (0x6ull << 40) |
			(0xEull << 44) | (0x3ull << 48) | (0xBull << 52) | (0x4ull << 56) | (0xCull << 60);
		uint32_t L = 0;
		uint32_t prev = 0;
#pragma unroll
		for (int m = 12; m >= 0; m--) {
			const uint32_t h = d16[m * 64 + L];
			L = (uint32_t)(kLocOf >> (4 * (h & 15u))) & 15u;
			if (m & 1)
				prev = h;
			else
				ubits[row * 8 + (m >> 1)] = h | (m == 12 ? 0u : (prev << 16));
		}
	}
	WSYNC();

	// CRC16 over the 208 decoded bits, 13 bits per lane of the row, XOR-reduced with DPP
	uint32_t syn = 0;
	{
		const uint32_t *ub = ubits + row * 8;
		const uint32_t k0 = loc * 13u;
		const uint32_t lo = ub[k0 >> 5], hi2 = ub[(k0 >> 5) + 1];      // word 7 of a row is never a data word
		const uint32_t cbits = __builtin_amdgcn_alignbit(hi2, lo, k0 & 31u);
		const uint32_t sy[7] = {sy0.x, sy0.y, sy0.z, sy0.w, sy1.x, sy1.y, sy1.z};
		uint32_t acc = 0;
#pragma unroll
		for (int pq = 0; pq < 7; pq++) {
			const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)cbits, 2 * pq, 1);
			const uint32_t m1 = pq < 6 ? (uint32_t)__builtin_amdgcn_sbfe((int)cbits, 2 * pq + 1, 1) : 0u;
			acc ^= sy[pq] & ((m0 & 0xffffu) | (m1 & 0xffff0000u));
		}
		syn = (acc ^ (acc >> 16)) & 0xffffu;
		syn ^= row_xor<1>(syn);
		syn ^= row_xor<2>(syn);
		syn ^= row_xor<4>(syn);
		syn ^= row_xor<8>(syn);
	}
	syn_o = syn;
}

__device__ __forceinline__ void store_l2(uint8_t *l2, const uint32_t *ub)
{
	uint32_t *l2w = reinterpret_cast<uint32_t *>(l2);
#pragma unroll
	for (int i = 0; i < 6; i++)
		l2w[i] = ub[i];
}

#undef ACS_CAND
#undef ACS_MIN
#undef ACS_PF
#undef ACS_NP
#undef ACS_LOAD
#undef ACSL_CORE
#undef ACSL_PF
#undef ACSL_NP
#undef ACSL_LOAD
#undef GMR1_DPP_PH0
#undef GMR1_DPP_PH1
#undef GMR1_DPP_PH2
#undef GMR1_DPP_PH3

}  // namespace gmr1
