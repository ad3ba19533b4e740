// tx_pulse_host.cpp -- the shaped modulator's pulse and index rule (osmo-gmr_amd/csrc/tx_pulse.h) on the host
// (tests/test_tx_pulse_host.py): the text the kernel k_shape runs, driven by lines on stdin, one answer line each.
//   T <pulse> <t>                                   -> the pulse at t symbols, rounded to float: "<hex bits>"
//   C <pulse> <sps> <span> <frac>                   -> a burst's coefficient table [mi * sps + p]: "<count> <hex bits> ..."
//   W <start> <span> <sps> <len> <in_len>           -> per window sample the body sample q = i sps + p, or -1 outside the body
//   S <pulse> <sps> <span> <frac> <start> <in_len> <len> <re im> x len
//                                                   -> the window without rotation and gain: "<hex re> <hex im>" x in_len
//   A <n> <len> <sps> <pulse> <span> <in_len>       -> shape_args_bad
// Doubles travel as %.17g.  The padded symbols and the table live in heap blocks of exactly their size, so a tap or a
// coefficient read outside them trips the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tx_pulse.h"

using namespace gmr1;

struct P2 { float x, y; };

static unsigned bits(float f)
{
	unsigned u;
	std::memcpy(&u, &f, 4);
	return u;
}

static float *coef_table(int pulse, int sps, int span, double frac)
{
	const int n = pulse_coefs(span, sps);
	float *cf = static_cast<float *>(std::malloc((size_t)n * sizeof(float)));
	if (!cf)
		std::exit(2);
	for (int c = 0; c < n; c++)
		cf[c] = pulse_coef(pulse, c / sps - span, c % sps, frac, sps);
	return cf;
}

int main()
{
	char kind;
	while (std::scanf(" %c", &kind) == 1) {
		if (kind == 'T') {
			int pulse;
			double t;
			if (std::scanf("%d %lf", &pulse, &t) != 2)
				return 2;
			std::printf("%08x\n", bits((float)(pulse == kPulseRrc ? rrc_pulse(t) : rc_pulse(t))));
		} else if (kind == 'C') {
			int pulse, sps, span;
			double frac;
			if (std::scanf("%d %d %d %lf", &pulse, &sps, &span, &frac) != 4)
				return 2;
			float *cf = coef_table(pulse, sps, span, frac);
			std::printf("%d", pulse_coefs(span, sps));
			for (int c = 0; c < pulse_coefs(span, sps); c++)
				std::printf(" %08x", bits(cf[c]));
			std::printf("\n");
			std::free(cf);
		} else if (kind == 'W') {
			int start, span, sps, len, in_len;
			if (std::scanf("%d %d %d %d %d", &start, &span, &sps, &len, &in_len) != 5)
				return 2;
			for (int k = 0; k < in_len; k++) {
				int i = -7, p = -7;
				const int in = shape_index(k, start, span, sps, len, shape_div_magic(sps), &i, &p);
				if (in && (p < 0 || p >= sps || i < 0 || i >= len + 2 * span))
					return 3;
				std::printf("%d ", in ? i * sps + p : -1);
			}
			std::printf("\n");
		} else if (kind == 'S') {
			int pulse, sps, span, start, in_len, len;
			double frac;
			if (std::scanf("%d %d %d %lf %d %d %d", &pulse, &sps, &span, &frac, &start, &in_len, &len) != 7)
				return 2;
			const int npad = shape_padded_len(len, span);
			P2 *sp = static_cast<P2 *>(std::calloc((size_t)npad, sizeof(P2)));
			if (!sp)
				return 2;
			for (int j = 0; j < len; j++)
				if (std::scanf("%f %f", &sp[2 * span + j].x, &sp[2 * span + j].y) != 2)
					return 2;
			float *cf = coef_table(pulse, sps, span, frac);
			for (int k = 0; k < in_len; k++) {
				int i, p;
				P2 v = {0.f, 0.f};
				if (shape_index(k, start, span, sps, len, shape_div_magic(sps), &i, &p))
					v = shape_body<P2>(sp, cf, i, p, span, sps);
				std::printf("%08x %08x ", bits(v.x), bits(v.y));
			}
			std::printf("\n");
			std::free(cf);
			std::free(sp);
		} else if (kind == 'A') {
			int n, len, sps, pulse, span, in_len;
			if (std::scanf("%d %d %d %d %d %d", &n, &len, &sps, &pulse, &span, &in_len) != 6)
				return 2;
			std::printf("%d\n", shape_args_bad(n, len, sps, pulse, span, in_len));
		} else {
			return 2;
		}
	}
	return 0;
}
