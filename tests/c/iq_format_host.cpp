// iq_format_host.cpp -- the load rule of osmo-gmr_amd/csrc/iq_format.h on the host (tests/test_chan_iq_host.py): every value
// of both integer types through iq_load, out of a heap buffer of exactly the samples' bytes whose base lies ONE SAMPLE into
// the allocation (4 bytes off for S16, 2 for S8), so that a load wider than a sample, or one that assumes more alignment,
// trips the sanitizers.  Sample k holds I = the k-th value of the type, Q = its bitwise complement: both components see
// every value.  Prints "<name> <count> <hex bits> ..." lines: bytes, scale, s16_i, s16_q, s8_i, s8_q, f32.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iq_format.h"

using namespace gmr1;

struct P2 { float x, y; };

static unsigned bits(float f)
{
	unsigned u;
	std::memcpy(&u, &f, 4);
	return u;
}

static void line(const char *name, const std::vector<float> &v)
{
	std::printf("%s %zu", name, v.size());
	for (float f : v)
		std::printf(" %08x", bits(f));
	std::printf("\n");
}

template <int FMT, typename T> static void every_value(const char *ni, const char *nq, int lo, int n)
{
	const size_t sb = (size_t)iq_sample_bytes(FMT);
	unsigned char *buf = static_cast<unsigned char *>(std::malloc((size_t)(n + 1) * sb));
	if (!buf)
		std::exit(2);
	std::memset(buf, 0x55, sb);
	T *s = reinterpret_cast<T *>(buf + sb);
	for (int k = 0; k < n; k++) {
		s[2 * k] = (T)(lo + k);
		s[2 * k + 1] = (T)~(lo + k);
	}
	std::vector<float> vi(n), vq(n);
	for (int k = 0; k < n; k++) {
		const P2 v = iq_load<FMT, P2>(buf + sb, k);
		vi[k] = v.x;
		vq[k] = v.y;
	}
	line(ni, vi);
	line(nq, vq);
	std::free(buf);
}

int main()
{
	std::printf("bytes 5 %d %d %d %d %d\n", iq_sample_bytes(kIqF32), iq_sample_bytes(kIqS16), iq_sample_bytes(kIqS8),
	            iq_sample_bytes(-1), iq_sample_bytes(3));
	line("scale", {iq_scale(kIqF32), iq_scale(kIqS16), iq_scale(kIqS8)});
	every_value<kIqS16, int16_t>("s16_i", "s16_q", -32768, 65536);
	every_value<kIqS8, int8_t>("s8_i", "s8_q", -128, 256);
	// the float format is a plain read: one sample in, as above
	const float raw[6] = {9.f, 9.f, 0.25f, -1.5f, 3.0e-39f, -0.0f};
	const P2 a = iq_load<kIqF32, P2>(raw + 2, 0), b = iq_load<kIqF32, P2>(raw + 2, 1);
	line("f32", {a.x, a.y, b.x, b.y});
	return 0;
}
