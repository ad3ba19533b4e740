// Host check of the addresses window_touch_q reads (osmo-gmr_amd/csrc/rx_touch.h), built with -fsanitize=address,undefined:
// for every window length and every start inside a 128-byte line the touched dwords are read out of a heap block that ends
// with the window, so a read beyond it is the sanitizer's to report; the bounds and the line coverage are checked here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "rx_touch.h"

static int fail(const char *what, int in_len, int start, long v)
{
	std::printf("FAIL %s in_len %d start %d value %ld\n", what, in_len, start, v);
	return 1;
}

int main()
{
	using namespace gmr1;
	static const int lens[] = {960, 976, 1016, 1024};
	long reads = 0;
	unsigned sum = 0;
	for (int in_len : lens) {
		for (int start = 0; start < kTouchLine; start += 8) {
			const size_t bytes = (size_t)start + 8u * (size_t)in_len;        // the block ends with the window's last byte
			void *blk = nullptr;
			if (posix_memalign(&blk, kTouchLine, bytes) != 0)
				return fail("alloc", in_len, start, 0);
			unsigned char *buf = static_cast<unsigned char *>(blk);
			for (size_t i = 0; i < bytes; i++)
				buf[i] = (unsigned char)i;
			const unsigned char *win = buf + start;
			const uintptr_t first = reinterpret_cast<uintptr_t>(win), last_dword = first + 8u * (uintptr_t)in_len - 4u;
			std::set<uintptr_t> touched;
			// as the wave does it: lane l reads slot l, lane 0 slot 64 as well
			for (int lane = 0; lane < 64; lane++) {
				for (int slot = lane; slot < kTouchSlots; slot += 64) {
					if (slot >= 64 && lane != 0)
						continue;
					const int o = window_touch_offset((unsigned)(first & (kTouchLine - 1)), in_len, slot);
					if (o < 0)
						continue;
					const uintptr_t ad = first + (uintptr_t)o;
					if (ad < first)
						return fail("before the window", in_len, start, o);
					if (ad > last_dword)
						return fail("behind the last dword", in_len, start, o);
					if (ad & 3u)
						return fail("not a dword address", in_len, start, o);
					sum += *reinterpret_cast<const volatile uint32_t *>(win + o);
					reads++;
					touched.insert(ad / kTouchLine);
				}
			}
			for (uintptr_t ln = first / kTouchLine; ln <= (first + 8u * (uintptr_t)in_len - 1u) / kTouchLine; ln++)
				if (!touched.count(ln))
					return fail("line not touched", in_len, start, (long)(ln - first / kTouchLine));
			if (touched.size() != (first + 8u * (uintptr_t)in_len - 1u) / kTouchLine - first / kTouchLine + 1)
				return fail("line outside the window touched", in_len, start, (long)touched.size());
			// slots that do not exist read nothing
			if (window_touch_offset((unsigned)start, in_len, -1) >= 0 || window_touch_offset((unsigned)start, in_len, kTouchSlots) >= 0)
				return fail("slot out of range reads", in_len, start, 0);
			std::free(blk);
		}
	}
	// the successor is touched only if this wave takes it next: never for q = 3, never for g + 1 >= n_end
	for (int g0 = 0; g0 < 12; g0 += 4)
		for (int n_end = g0; n_end <= g0 + 4; n_end++)
			for (int q = 0; q < 4; q++) {
				const int g = g0 + q;
				const bool want = window_touch_wanted(q, g, n_end);
				if (want != (q < 3 && g + 1 < n_end))
					return fail("wanted", q, g, n_end);
				if (g + 1 >= n_end && want)
					return fail("touch beyond the wave's bursts", q, g, n_end);
			}
	std::printf("OK %ld reads %u\n", reads, sum);
	return 0;
}
