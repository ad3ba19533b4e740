// Host-side exercise of osmo-gmr_amd/csrc/tch3_follow.h (rx_tch3's per-frame state machine, which the device runs inside
// k_tch3f_walk): walks one call through per-frame results read from stdin and moves the FACCH3 soft bits as the step says,
// the way the kernel does.  tests/test_tch3_follow_host.py feeds it what tests/tch3_cases.py computed from the oracle.
//   usage: tch3_follow_host p energy_dkab_bits energy_burst_bits < frames
//   a frame: energy_bits dkab_rv det_rv btid facch_rv facch_sid speech_rv fn, then 104 soft bits
//   prints per frame: cls need flush, and at the end the state: scalars, bi_fn, 416 soft bits
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tch3_follow.h"

using namespace gmr1;

static float from_bits(unsigned long v)
{
	const uint32_t u = (uint32_t)v;
	float f;
	memcpy(&f, &u, 4);
	return f;
}

static uint32_t to_bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

int main(int argc, char **argv)
{
	if (argc < 4)
		return 2;
	Tch3Walk s{};
	int8_t ebits[416] = {0};
	s.active = 1;
	s.p = atoi(argv[1]);
	s.energy_dkab = from_bits(strtoul(argv[2], nullptr, 10));
	s.energy_burst = from_bits(strtoul(argv[3], nullptr, 10));
	for (;;) {
		unsigned long eb, fn;
		Tch3FrameIn f;
		if (scanf("%lu %d %d %d %d %d %d %lu", &eb, &f.dkab_rv, &f.det_rv, &f.btid, &f.facch_rv, &f.facch_sid, &f.speech_rv, &fn) != 8)
			break;
		f.energy = from_bits(eb);
		f.fn = (uint32_t)fn;
		int8_t burst[104];
		for (int i = 0; i < 104; i++) {
			int v;
			if (scanf("%d", &v) != 1)
				return 3;
			burst[i] = (int8_t)v;
		}
		const Tch3Act a = tch3_follow_step(s, f);
		if (a.flush == 1)
			memset(ebits, 0, sizeof(ebits));
		if (a.store)
			memcpy(&ebits[104 * a.bi], burst, 104);
		if (a.flush == 2)
			memset(ebits, 0, sizeof(ebits));
		printf("%d %d %d\n", a.cls, a.need, a.flush);
	}
	printf("end %d %d %d %d %d %d %u %u %u %u %u %u", s.active, s.p, s.ciph, s.weak_cnt, s.sync_id, s.burst_cnt,
	       to_bits(s.energy_dkab), to_bits(s.energy_burst), s.bi_fn[0], s.bi_fn[1], s.bi_fn[2], s.bi_fn[3]);
	for (int i = 0; i < 416; i++)
		printf(" %d", ebits[i]);
	printf("\n");
	return 0;
}
