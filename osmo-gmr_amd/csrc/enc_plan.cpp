// enc_plan.cpp -- the layer-1 channel ENCODERS (reference include/osmocom/gmr1/l1/bcch.h:37, ccch.h:37, facch3.h:37-38,
// tch3.h:37-39, facch9.h:37-39, tch9.h:47-49, rach.h:37, xch_dc12.h:37) written down ONCE each as an EncPlan -- the
// position map from payload bits to burst bits (CRC tables, trellis-step windows, puncturing, interleavers, scrambler,
// multiplexing; the structure follows the reference's encoders line by line, in index space instead of on data).  The
// codes themselves -- polynomials, CRCs, puncturing masks and the puncturer, scrambler, interleaver positions -- are
// l1_codes.h's, the description the decoders' tables are made from.  Host arithmetic only: no HIP, so
// tests/c/enc_plan_host.cpp runs it on its own, under the sanitizers too.  Every bit of every burst is then computed on
// the GPU by k_encode (tx_kernels.hip, through capi_encode.cpp); there is no CPU path.

#include "enc_plan.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#include "l1_codes.h"
#include "nt9_map.h"

using namespace gmr1;

namespace {

// ---- a burst bit in index space -------------------------------------------------------------------------
struct Sym {
	int kind = 1;      // 0 coded (window t, poly slot), 1 constant 0, 2 multiplexed-in bit t
	int t = 0, poly = 0;
	int scr = 0;       // scrambler bit xor-ed in
	int ci = 0;        // keystream index + 1
	int d = 0;         // burst delay (inter-burst interleaver)
};
typedef std::vector<Sym> Bits;

Sym aux_bit(int idx)
{
	Sym s;
	s.kind = 2;
	s.t = idx;
	return s;
}

uint16_t pay_lsb(int k) { return (uint16_t)k; }                                       // osmo_pbit2ubit_ext, lsb mode
uint16_t pay_msb(int k) { return (uint16_t)((k >> 3) * 8 + 7 - (k & 7)); }            // osmo_pbit2ubit
uint16_t crc_a(int bit) { return (uint16_t)(0x4000 | bit); }
uint16_t crc_b(int bit) { return (uint16_t)(0x8000 | bit); }

struct Code {
	int N, K, len;
	bool tail_biting;
	unsigned polys[5];                 // bit i = D^i (the comments of reference src/l1/conv.c)
	std::vector<uint8_t> punct;        // per unpunctured coded bit: 1 = not sent (empty: nothing punctured)
};

struct Builder {
	EncPlan P;
	int n_poly = 0;

	Builder() { std::memset(&P, 0, sizeof(P)); P.depth = 1; }

	int poly_slot(uint32_t mask)
	{
		for (int i = 0; i < n_poly; i++)
			if (P.poly[i] == mask)
				return i;
		if (n_poly == 8)
			abort();
		P.poly[n_poly] = mask;
		return n_poly++;
	}

	// CRC of `n` payload-sourced bits (osmo_crcXXgen_set_bits, init 0 / no final xor: crc.c:36-63): the register is the
	// xor of one table entry per set bit
	void crc_table(uint16_t *tab, const l1c::Crc &c, const std::vector<uint16_t> &src)
	{
		const int n = (int)src.size();
		for (int k = 0; k < n; k++)
			tab[src[k]] ^= (uint16_t)l1c::crc_unit(c, k, n);
	}

	// extended information word of one code: [K-1 preset | info | K-1 flush zeros]; returns the offset of step 0's window
	int add_word(int K, bool tail_biting, const std::vector<uint16_t> &info)
	{
		const int base = P.n_ext, len = (int)info.size();
		if (base + (K - 1) + len + (tail_biting ? 0 : K - 1) > kEncMaxExt)
			abort();
		int o = base;
		for (int i = 0; i < K - 1; i++)
			P.ext_src[o++] = tail_biting ? info[len - (K - 1) + i] : (uint16_t)0xffff;
		for (int i = 0; i < len; i++)
			P.ext_src[o++] = info[i];
		if (!tail_biting)
			for (int i = 0; i < K - 1; i++)
				P.ext_src[o++] = 0xffff;
		P.n_ext = o;
		return base;
	}

	// osmo_conv_encode over the word at `base`: step t reads the register (state << 1 | bit), bit i = D^i = info[t - i];
	// in the extended word that is window bit K-1-i.  Output bit j of a step = poly j, MSB of next_output first.
	Bits conv(const Code &c, int base)
	{
		Bits out;
		const int steps = c.len + (c.tail_biting ? 0 : c.K - 1);
		int slots[5];
		for (int j = 0; j < c.N; j++) {
			uint32_t m = 0;
			for (int i = 0; i < c.K; i++)
				if ((c.polys[j] >> i) & 1)
					m |= 1u << (c.K - 1 - i);
			slots[j] = poly_slot(m);
		}
		for (int t = 0, idx = 0; t < steps; t++)
			for (int j = 0; j < c.N; j++, idx++) {
				if (!c.punct.empty() && c.punct[idx])
					continue;
				Sym s;
				s.kind = 0;
				s.t = base + t;
				s.poly = slots[j];
				out.push_back(s);
			}
		return out;
	}

	// bits that are sent as they are (class-2 speech bits): a window of one bit
	Bits plain(int base, int n)
	{
		Bits out;
		const int slot = poly_slot(1u);
		for (int i = 0; i < n; i++) {
			Sym s;
			s.kind = 0;
			s.t = base + i;
			s.poly = slot;
			out.push_back(s);
		}
		return out;
	}

	void finish(const Bits &e)
	{
		if ((int)e.size() > kEncMaxOut)
			abort();
		P.n_out = (int)e.size();
		for (int i = 0; i < P.n_out; i++) {
			const Sym &s = e[i];
			P.out[i] = (uint32_t)s.t | ((uint32_t)s.poly << 10) | ((uint32_t)s.kind << 13) | ((uint32_t)s.scr << 15) |
			           ((uint32_t)s.ci << 16) | ((uint32_t)s.d << 26);
		}
	}
};

// gmr1_interleave_intra (interleave.c:48-61)
Bits interleave_intra(const Bits &in, int off, int N)
{
	Bits out(8 * N);
	for (int kc = 0; kc < 8 * N; kc++)
		out[l1c::intra_pos(N, kc)] = in[off + kc];
	return out;
}

// gmr1_scramble_ubit (scramb.c:39-52, 83-93): the LFSR is restarted for every call
void scramble(Bits &b, int off, int n)
{
	l1c::Scrambler g;
	for (int i = 0; i < n; i++)
		b[off + i].scr ^= (int)g.next();
}

void cipher(Bits &b, int off, int n, int c0)
{
	for (int i = 0; i < n; i++)
		b[off + i].ci = c0 + i + 1;
}

void append(Bits &dst, const Bits &src, int off, int n) { dst.insert(dst.end(), src.begin() + off, src.begin() + off + n); }

std::vector<uint16_t> lsb_bits(int first, int n)
{
	std::vector<uint16_t> v(n);
	for (int i = 0; i < n; i++)
		v[i] = pay_lsb(first + i);
	return v;
}

// a code of l1_codes.h's polynomials (N of them) over `len` information bits
template <int N>
Code make_code(int K, int len, bool tb, const unsigned (&polys)[N])
{
	Code c;
	c.N = N; c.K = K; c.len = len; c.tail_biting = tb;
	for (int j = 0; j < N; j++)
		c.polys[j] = polys[j];
	return c;
}

// per unpunctured coded bit of `c`: 1 = not sent, `mn` repeated over the whole stream (gmr1_puncturer_generate with
// repeat 0 and no first / last block: tch3.c:48, xch_dc12.c:52)
template <int M>
void puncture_all(Code &c, const l1c::Punct<M> &mn)
{
	c.punct.assign((size_t)(c.len + (c.tail_biting ? 0 : c.K - 1)) * c.N, 0);
	l1c::punctured_bits(c.punct.data(), (int)c.punct.size(), l1c::kNoScheme, l1c::scheme(mn), l1c::kNoScheme, 0);
}

// 192 information bits + CRC16 (crc.c:58-63): BCCH, CCCH, xCH
std::vector<uint16_t> info_crc16(Builder &b, int n_bits)
{
	std::vector<uint16_t> info = lsb_bits(0, n_bits);
	b.crc_table(b.P.crc_tab, l1c::kCrc16, info);
	for (int i = 0; i < 16; i++)
		info.push_back(crc_a(15 - i));
	return info;
}

// ---- the chains --------------------------------------------------------------------------------------------
void plan_bcch_ccch(Builder &b, bool ccch)          // bcch.c:60-81, ccch.c:60-83
{
	b.P.n_in0 = 24;
	const Code c = make_code(5, 208, false, l1c::kK5_12);
	const int base = b.add_word(5, false, info_crc16(b, 192));
	const Bits coded = b.conv(c, base);                            // 424
	const Bits il = interleave_intra(coded, 0, 53);
	Bits e;
	if (ccch) e.resize(4);                                         // 4 + 4 padding zeros, scrambled with the rest
	append(e, il, 0, 424);
	if (ccch) e.resize(432);
	scramble(e, 0, (int)e.size());
	b.finish(e);
}

void plan_facch3(Builder &b)                        // facch3.c:65-116
{
	b.P.n_in0 = 10;
	b.P.n_aux0 = 32;
	b.P.n_ciph = 384;
	const Code c = make_code(5, 92, false, l1c::kK5_14);
	const int base = b.add_word(5, false, info_crc16(b, 76));
	const Bits coded = b.conv(c, base);                            // 384
	Bits cp(384);
	for (int i = 0; i < 384; i++)
		cp[(i & 3) * 96 + (i >> 2)] = coded[i];
	Bits e;
	for (int bu = 0; bu < 4; bu++) {
		Bits x = interleave_intra(cp, 96 * bu, 12);
		scramble(x, 0, 96);
		cipher(x, 0, 96, 96 * bu);
		append(e, x, 0, 22);
		for (int j = 0; j < 8; j++)
			e.push_back(aux_bit(8 * bu + j));
		append(e, x, 22, 74);
	}
	b.finish(e);
}

void plan_tch3(Builder &b, int m)                   // tch3.c:78-118 with the conv_encode arguments the right way round
{
	b.P.n_in0 = 20;                                                // frame0 | frame1
	b.P.n_aux0 = 4;
	b.P.n_ciph = 208;
	Code c = make_code(7, 48, true, l1c::kTch3);
	puncture_all(c, l1c::k5_12_P12);                               // P(1;2), punct.c:239-248
	Bits epp(208);
	for (int f = 0; f < 2; f++) {
		std::vector<uint16_t> cls1(48), cls2(32);
		for (int k = 0; k < 48; k++) cls1[k] = pay_msb(80 * f + k);
		for (int k = 0; k < 32; k++) cls2[k] = pay_msb(80 * f + 48 + k);
		const int b1 = b.add_word(7, true, cls1);
		const int b2 = b.add_word(1, false, cls2);
		Bits cb = b.conv(c, b1);                                   // 72
		const Bits raw = b.plain(b2, 32);
		append(cb, raw, 0, 32);                                    // 104
		Bits ep(104);
		for (int kc = 0; kc < 104; kc++)
			ep[l1c::tch3_pos(kc)] = cb[kc];
		for (int j = 0; j < 104; j++)
			epp[m ? 104 * f + j : 2 * j + f] = ep[j];
	}
	scramble(epp, 0, 208);
	cipher(epp, 0, 208, 0);
	Bits e;
	append(e, epp, 0, 52);
	for (int j = 0; j < 4; j++)
		e.push_back(aux_bit(j));
	append(e, epp, 52, 156);
	b.finish(e);
}

// the NT9 burst around 648 coded positions: scramble, SACCH, cipher, status (facch9.c:84-103, tch9.c:114-136)
void nt9_finish(Builder &b, Bits &x)
{
	b.P.n_aux0 = 10;
	b.P.n_aux1 = 4;
	b.P.n_ciph = 658;
	scramble(x, 0, 648);
	Bits my;
	append(my, x, 0, 52);
	for (int j = 0; j < 10; j++)
		my.push_back(aux_bit(j));
	append(my, x, 52, 596);
	cipher(my, 0, 658, 0);
	Bits e;
	append(e, my, 0, 52);
	for (int j = 0; j < 4; j++)
		e.push_back(aux_bit(10 + j));
	append(e, my, 52, 606);
	b.finish(e);
}

void plan_facch9(Builder &b)                        // facch9.c:60-104
{
	b.P.n_in0 = 38;
	const Code c = make_code(5, 316, false, l1c::kK5_12);
	const int base = b.add_word(5, false, info_crc16(b, 300));
	const Bits coded = b.conv(c, base);                            // 640
	const Bits il = interleave_intra(coded, 0, 80);
	Bits x(4);
	append(x, il, 0, 640);
	x.resize(648);
	nt9_finish(b, x);
}

void plan_tch9(Builder &b, int mode)                // tch9.c:56-79, 81-137
{
	const int len = kNt9Kinds[mode].len;
	Code c = mode == 0 ? make_code(5, len, false, l1c::kK5_15)
	       : mode == 1 ? make_code(5, len, false, l1c::kK5_13) : make_code(5, len, false, l1c::kK5_12);
	c.punct = nt9_punctured(mode);
	b.P.n_in0 = len / 8;
	b.P.depth = 3;
	const int base = b.add_word(5, false, lsb_bits(0, len));
	const Bits coded = b.conv(c, base);
	if (coded.size() != 648)
		abort();
	Bits x = interleave_intra(coded, 0, 81);
	for (int jk = 0; jk < 648; jk++)
		x[jk].d = jk % 3;                                          // gmr1_interleave_inter, N = 3 (interleave.c:128-158)
	nt9_finish(b, x);
}

void plan_rach(Builder &b)                          // rach.c:44-66, 78-136
{
	b.P.n_in0 = 18;
	b.P.n_in1 = 1;                                                 // the SB mask rides as payload byte 18
	const std::vector<uint16_t> u1 = lsb_bits(0, 16), u2 = lsb_bits(16, 123);
	b.crc_table(b.P.crc_tab, l1c::kCrc8, u1);                      // crc.c:36-44
	for (int i = 0; i < 8; i++)
		b.P.crc_tab[144 + i] ^= (uint16_t)(1u << i);               // crc bit ^= sb_mask bit, rach.c:104-105
	b.crc_table(b.P.crc_tab2, l1c::kCrc12, u2);                    // crc.c:46-54
	std::vector<uint16_t> info = u2;
	for (int i = 0; i < 12; i++) info.push_back(crc_b(11 - i));
	info.insert(info.end(), u1.begin(), u1.end());
	for (int i = 0; i < 8; i++) info.push_back(crc_a(7 - i));      // 159
	Code c = make_code(5, 159, false, l1c::kK5_14);
	c.punct.assign(163 * 4, 0);
	for (int i = 0; i < 135; i++)
		c.punct[4 * i + 2] = c.punct[4 * i + 3] = 1;
	const int base = b.add_word(5, false, info);
	const Bits coded = b.conv(c, base);                            // 382
	const Bits e1p = interleave_intra(coded, 270, 14);             // 112
	Bits e2p = interleave_intra(coded, 0, 33);                     // 264
	append(e2p, coded, 264, 6);
	Bits x;
	append(x, e1p, 0, 112);
	append(x, e2p, 0, 270);
	append(x, e1p, 0, 112);
	scramble(x, 0, 494);
	Bits e;
	append(e, x, 112, 136);
	append(e, x, 0, 112);
	append(e, x, 382, 112);
	append(e, x, 248, 134);
	b.finish(e);
}

void plan_xch(Builder &b)                           // xch_dc12.c:45-54, 64-84
{
	b.P.n_in0 = 24;
	Code c = make_code(9, 208, true, l1c::kK9_13);
	puncture_all(c, l1c::k9_13_P1213);                             // punct.c:1105-1125
	const int base = b.add_word(9, true, info_crc16(b, 192));
	const Bits coded = b.conv(c, base);                            // 432
	Bits e = interleave_intra(coded, 0, 54);
	scramble(e, 0, 432);
	b.finish(e);
}

}  // namespace

void gmr1::build_enc_plan(int id, EncPlan *out)
{
	Builder b;
	switch (id) {
	case kPlBcch: plan_bcch_ccch(b, false); break;
	case kPlCcch: plan_bcch_ccch(b, true); break;
	case kPlFacch3: plan_facch3(b); break;
	case kPlTch3M0: plan_tch3(b, 0); break;
	case kPlTch3M1: plan_tch3(b, 1); break;
	case kPlFacch9: plan_facch9(b); break;
	case kPlTch9_2k4: plan_tch9(b, 0); break;
	case kPlTch9_4k8: plan_tch9(b, 1); break;
	case kPlTch9_9k6: plan_tch9(b, 2); break;
	case kPlRach: plan_rach(b); break;
	default: plan_xch(b); break;
	}
	*out = b.P;
}
