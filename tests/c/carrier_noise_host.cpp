// carrier_noise_host.cpp -- the carrier mixer's noise rule and carrier phase (osmo-gmr_amd/csrc/carrier_noise.h) on the
// host (tests/test_carrier_host.py): the text the kernel k_carrier_mix runs, driven by lines on stdin, one answer line each.
//   P <c0> <c1> <c2> <c3> <k0> <k1>     (hex)      -> Philox4x32-10: "<w0> <w1> <w2> <w3>" (hex)
//   N <seed> <id> <first> <count>       (decimal)  -> per sample n = first .. first + count: "<wa> <wb> <u1> <u2> <re> <im>",
//                                                     the sample's two words and the float bits of its uniforms and of z
//   F <cfo> <n>                         (%.17g, decimal) -> the float bits of carrier_phase(cfo, n)
// The samples of an N line go through a heap block of exactly their size, so an index outside it trips the sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "carrier_noise.h"

using namespace gmr1;

struct P2 { float x, y; };

static unsigned bits(float f)
{
	unsigned u;
	std::memcpy(&u, &f, 4);
	return u;
}

int main()
{
	char kind;
	while (std::scanf(" %c", &kind) == 1) {
		if (kind == 'P') {
			uint32_t c[4], k[2], w[4];
			if (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6)
				return 2;
			philox4x32_10(c, k, w);
			std::printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
		} else if (kind == 'N') {
			uint64_t seed;
			uint32_t id;
			int64_t first;
			int count;
			if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNd64 " %d", &seed, &id, &first, &count) != 4 || count < 0)
				return 2;
			P2 *z = static_cast<P2 *>(std::malloc((size_t)(count ? count : 1) * sizeof(P2)));
			if (!z)
				return 2;
			for (int i = 0; i < count; i++)
				z[i] = noise_sample<P2>(seed, id, first + i);
			for (int i = 0; i < count; i++) {
				const int64_t n = first + i;
				uint32_t w[4];
				noise_words(seed, id, (uint64_t)(n >> 1), w);
				const uint32_t wa = w[(n & 1) ? 2 : 0], wb = w[(n & 1) ? 3 : 1];
				std::printf("%08x %08x %08x %08x %08x %08x ", wa, wb, bits(noise_u1(wa)), bits(noise_u2(wb)), bits(z[i].x), bits(z[i].y));
			}
			std::printf("\n");
			std::free(z);
		} else if (kind == 'F') {
			double cfo;
			int64_t n;
			if (std::scanf("%lf %" SCNd64, &cfo, &n) != 2)
				return 2;
			std::printf("%08x\n", bits(carrier_phase(cfo, n)));
		} else {
			return 2;
		}
	}
	return 0;
}
