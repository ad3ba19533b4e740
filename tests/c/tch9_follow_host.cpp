// Host-side exercise of osmo-gmr_amd/csrc/tch9_follow.h (rx_tch9's routing, which the device runs in k_tch9f_plan and
// k_tch9f_emit): plans calls read from stdin 64 frames a step from the mask of TCH9 frames, the way the kernels do from a
// ballot.  tests/test_tch9_follow_host.py compares the result with the frame by frame restatement of tests/tch9_cases.py.
//   a call, one line: active n_held base n, then n pairs rv sync_id (base: the index of its first frame)
//   prints per call one line: per frame cls need src1 src2, then the carry behind the last frame and the new n_held
#include <cstdio>
#include <vector>

#include "tch9_follow.h"

using namespace gmr1;

int main()
{
	int active, n_held, base, n;
	while (scanf("%d %d %d %d", &active, &n_held, &base, &n) == 4) {
		if (n < 0)
			return 2;
		std::vector<int> rv(n), sid(n);
		for (int k = 0; k < n; k++)
			if (scanf("%d %d", &rv[k], &sid[k]) != 2)
				return 3;
		Tch9Carry carry = tch9f_seed(n_held);
		const int k0 = base, k1 = base + n;
		for (int kb = k0; kb < k1; kb += 64) {
			int cls[64];
			unsigned long long tch = 0;
			for (int lane = 0; lane < 64; lane++) {
				const int k = kb + lane;
				cls[lane] = k < k1 ? tch9f_class(active, rv[k - base], sid[k - base]) : kT9Off;
				if (k < k1 && cls[lane] == kT9Tch)
					tch |= 1ull << lane;
			}
			for (int lane = 0; lane < 64 && kb + lane < k1; lane++) {
				const Tch9Carry s = tch9f_sources(tch, lane, kb, carry);
				printf("%d %d %d %d ", cls[lane], tch9f_need(cls[lane]), s.s1, s.s2);
			}
			carry = tch9f_sources(tch, 64, kb, carry);
		}
		printf("%d %d %d\n", carry.s1, carry.s2, tch9f_n_held(carry));
	}
	return 0;
}
