// scratch_carve_host.cpp -- the host layer's carve-up of device scratch without a device (csrc/scratch_carve.h,
// scratch_layouts.h; tests/test_scratch_carve_host.py).  "carve" checks the cursor itself and prints
// "ok"; otherwise one query per line of stdin, one answer per line:
//   sizes                                    -> the public structs the layouts size by
//   follow3 n | follow9 n | acq n peaks | audio n_calls n | acqblock A
//                                            -> every member's name and offset from a null base, then "bytes" and the total
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scratch_layouts.h"

using namespace gmr1;

#define CHECK(c)                                                                \
	do {                                                                        \
		if (!(c)) {                                                             \
			fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #c); \
			return 1;                                                           \
		}                                                                       \
	} while (0)

static int carve_check()
{
	// sizes in bytes as (elements, element size): below, at and past a line, nothing, and several lines
	static const size_t kN[] = {1, 127, 128, 129, 0, 33, 0, 1000, 5};
	static const size_t kE[] = {1, 1, 1, 1, 4, 4, 8, 2, 8};
	const int n = sizeof(kN) / sizeof(kN[0]);
	auto take = [&](Carve &c, int i) -> void * {
		switch (kE[i]) {
		case 1: return c.take<uint8_t>(kN[i]);
		case 2: return c.take<int16_t>(kN[i]);
		case 4: return c.take<int32_t>(kN[i]);
		default: return c.take<uint64_t>(kN[i]);
		}
	};
	// a null base: the pointers are the running offsets
	size_t sum = 0;
	Carve c0(nullptr);
	for (int i = 0; i < n; i++) {
		CHECK((uintptr_t)take(c0, i) == sum);
		sum += (kN[i] * kE[i] + 127) / 128 * 128;
		CHECK(c0.bytes() == sum);
	}
	CHECK(up128(0) == 0 && up128(1) == 128 && up128(128) == 128 && up128(129) == 256);
	// a real block: aligned, inside, one behind the other
	unsigned char *buf = static_cast<unsigned char *>(aligned_alloc(128, sum));
	CHECK(buf);
	Carve c1(buf);
	uintptr_t end = (uintptr_t)buf;
	for (int i = 0; i < n; i++) {
		const size_t before = c1.bytes();
		const uintptr_t p = (uintptr_t)take(c1, i);
		CHECK(p % 128 == 0);
		CHECK(p >= end && p + kN[i] * kE[i] <= (uintptr_t)buf + sum);
		end = p + kN[i] * kE[i];
		if (kN[i] == 0)
			CHECK(c1.bytes() == before);          // nothing taken, nothing moved
		if (kN[i])
			std::memset(reinterpret_cast<void *>(p), 0x5a, kN[i] * kE[i]);
	}
	CHECK(c1.bytes() == c0.bytes());
	free(buf);
	printf("ok\n");
	return 0;
}

static std::string g_line;
static void member(const char *name, const void *p) { g_line += std::string(name) + " " + std::to_string((uintptr_t)p) + " "; }
#define M(o, f) member(#f, (o).f)
#define M2(o, f) member(#f "0", (o).f[0]), member(#f "1", (o).f[1])
static void total(size_t bytes) { printf("%sbytes %zu\n", g_line.c_str(), bytes); }

int main(int argc, char **argv)
{
	if (argc > 1 && !strcmp(argv[1], "carve"))
		return carve_check();
	char buf[256], what[32];
	while (fgets(buf, sizeof(buf), stdin)) {
		long long v[5] = {0, 0, 0, 0, 0};
		if (sscanf(buf, "%31s %lld %lld %lld %lld %lld", what, &v[0], &v[1], &v[2], &v[3], &v[4]) < 1)
			continue;
		const std::string w = what;
		g_line.clear();
		if (w == "sizes") {
			printf("%zu %zu\n", sizeof(gmr1_hip_rx_audio), sizeof(gmr1_hip_fcch_acq));
		} else if (w == "follow3") {
			const FollowScratch o(nullptr, (size_t)v[0]);
			M(o, call); M(o, p); M(o, et); M(o, en); M(o, krv); M(o, drv); M(o, bt); M(o, dsid); M(o, dtoa); M(o, frv); M(o, fsid);
			M(o, ftoa); M(o, srv); M(o, feb); M(o, seb); M(o, cls); M(o, need); M(o, jeb); M(o, jfn); M(o, kss); M(o, ksf);
			M2(o, sfr); M2(o, scv); M2(o, fl); M2(o, fcrc); M2(o, fcv);
			total(o.bytes);
			if (o.bytes != tch3_follow_scratch_bytes((int)v[0])) return 1;
		} else if (w == "follow9") {
			const Follow9Scratch o(nullptr, (size_t)v[0]);
			M(o, eb); M(o, sid); M(o, rv); M(o, cls); M(o, need); M(o, src); M(o, call); M(o, ks); M(o, fl2); M(o, tl2); M(o, fcrc);
			M(o, fcv); M(o, tcv);
			total(o.bytes);
			if (o.bytes != tch9_follow_scratch_bytes((int)v[0])) return 1;
		} else if (w == "acq") {
			const AcqScratch o(nullptr, (size_t)v[0], (size_t)v[1]);
			M(o, base); M(o, len); M(o, stat); M(o, align); M(o, base_align); M(o, ferr); M(o, can3); M(o, off); M(o, peaks);
			M(o, toa1); M(o, rv1); M(o, ftoa); M(o, fe); M(o, count); M(o, ctoa); M(o, cfe); M(o, snr); M(o, live); M(o, fs);
			total(o.bytes);
		} else if (w == "audio") {
			const AudioScratch o(nullptr, (size_t)v[0], (size_t)v[1]);
			M(o, slot); M(o, sink);
			total(o.bytes);
			if (o.bytes != tch3_audio_scratch_bytes((int)v[0], (int)v[1])) return 1;
		} else if (w == "acqblock") {
			const AcqBlock o(nullptr, (size_t)v[0]);
			M(o, offset); M(o, length); M(o, results);
			member("up_bytes", reinterpret_cast<const void *>(o.up_bytes));
			total(o.bytes);
		} else {
			fprintf(stderr, "unknown query %s\n", what);
			return 2;
		}
	}
	return 0;
}
