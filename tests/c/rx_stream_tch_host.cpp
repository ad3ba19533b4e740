// Host-side check of the arithmetic that lets the streaming receive loop follow TCH3 calls (osmo-gmr_amd/csrc/rx_stream.h,
// DESIGN.md 4.4b): the traffic window of a frame the walk admitted lies inside the samples the handle holds, for every
// sps, timeslot and BCCH correction the argument covers.  tests/test_rx_stream_tch_host.py builds and runs it.
#include <cstdio>

#include "rx_stream.h"

using namespace gmr1;

#define CHECK(x) do { if (!(x)) { std::printf("FAIL line %d, sps %d: %s\n", __LINE__, sps, #x); return 1; } } while (0)

int main()
{
	for (int sps = 1; sps <= 16; sps++) {
		const long long fl = rx_stream_frame_len(sps);
		const int in_len = rx_tch3_in_len(sps), win = sps + sps / 2;
		CHECK(in_len == 117 * sps + win);
		for (int tn = 0; tn < 32; tn++) {
			// burst_map of an NT3 burst with `win` samples of search room (rx_loop.h), restated by rx_tch3_begin
			RxLoopState c{};
			c.align = 100000;
			c.len = 1 << 30;
			int begin = 0;
			CHECK(rx_loop_burst_map(c, sps, 117, tn, win, &begin) == win >> 1);
			CHECK(begin == rx_tch3_begin(c.align, sps, tn));
			// upper test: a frame admitted at `a` (a + 2 fl <= len) whose BCCH burst then moved align by d -- at most 10 sps
			// of timing correction and an SI1 that relabels the timeslot up to 13 slots down -- still holds its window
			const long long a = 7 * fl + 13;
			for (long long d = -(31 * 39 + 10) * sps; d <= (13 * 39 + 10) * sps; d += (d < 0 ? 97 : 1))
				CHECK(rx_tch3_begin((int)(a + d), sps, tn) + in_len <= a + 2 * fl);
			// ... and the window ends where the issue of the design says: below align + (31 * 39 + 118.5) sps
			CHECK(2 * (rx_tch3_begin(0, sps, tn) + in_len) <= (2 * (31 * 39 + 118) + 1) * (long long)sps + 1);
			// lower test: a window starts no earlier than the walk's own reach before align, so once a carrier has dropped
			// samples (every walking chain's align is at least rx_stream_reach_back from the front: k_rx_stage's check, and
			// rx_stream_keep_from keeps 2 fl > reach_back) begin < 0 cannot happen in rebased coordinates
			CHECK(rx_tch3_begin(0, sps, tn) >= -(long long)rx_stream_reach_back(sps));
			CHECK(rx_tch3_begin(rx_stream_reach_back(sps), sps, tn) >= 0);
		}
		CHECK(2 * fl > rx_stream_reach_back(sps));
		// the one forward move the argument does not cover: 14 slots down at timeslot 31
		CHECK(rx_tch3_begin((int)(7 * fl + (14 * 39 + 10) * sps), sps, 31) + in_len > 7 * fl + 2 * fl);
		// a tch handle's record bound: the loop's per-chain buffer plus one TCH3 record per frame the walk can log
		for (long long len = 0; len < 50 * fl; len += 1013) {
			CHECK(rx_stream_frames_per_chain(len, sps) == len / fl + 2);
			CHECK(rx_stream_tch_rec_per_chain(len, sps) == rx_stream_rec_per_chain(len, sps) + len / fl + 2);
		}
	}
	std::printf("ok\n");
	return 0;
}
