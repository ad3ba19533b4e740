// Host-side table of the channelizer's and the direct mode's plans (osmo-gmr_amd/csrc/chan_plan.h): the numbers the library
// works out for a (sample rate, sps) before it touches the device, printed so that tests/test_chan_plan_host.py can hold them
// to the oracle's restatements (oracle/orc_chan.py, tests/chan_grid_cases.py) without a GPU.  By its first argument:
//   ddc       lines "rate sps" ->  "ok|refused d1 d2 num den rrc_tpf row j0 nt1 nt2 nrrc | refusal text"
//   chan      lines "rate sps n_in" -> "ok|refused n_chans ntaps n_blocks tpf j0 num den pre pre_tpf pre_j0 pre_num pre_den
//             n_mid T n_out | refusal text"   (n_mid: samples into the filterbank, T: its instants)
//   taps chan|ddc rate sps -> one line per vector, "name count bits ..." with every float32 as its bit pattern in hex
//             (a bank: x0 y0 x1 y1 ... row by row)
//   carrier rate sps f ... -> "t1 ..." (re, im pairs, carrier after carrier) and "rot ..." (doubles as bit patterns)
//   select nch idx ... -> "ok slot ..." or "refused | text"
// Floats travel as bit patterns so that the comparison sees exactly what the library would upload.  Built once more under the
// address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chan_plan.h"

using namespace gmr1;

namespace {

uint32_t bits(float f)
{
	uint32_t u;
	std::memcpy(&u, &f, sizeof(u));
	return u;
}

void show(const char *name, const std::vector<float> &v)
{
	std::printf("%s %zu", name, v.size());
	for (float f : v)
		std::printf(" %08x", bits(f));
	std::printf("\n");
}

void show(const char *name, const std::vector<F2> &v)
{
	std::printf("%s %zu", name, v.size());
	for (const F2 &f : v)
		std::printf(" %08x %08x", bits(f.x), bits(f.y));
	std::printf("\n");
}

int ddc()
{
	double rate;
	int sps;
	while (std::scanf("%lf %d", &rate, &sps) == 2) {
		DdcNumbers p;
		std::string why;
		const bool ok = plan_numbers(rate, sps, &p, &why);
		std::printf("%s %d %d %lld %lld %d %d %d %zu %zu %zu | %s\n", ok ? "ok" : "refused", p.d1, p.d2, p.rs.num, p.rs.den,
		            p.rrc_tpf, p.rs.tpf, p.rs.j0, p.taps1.size(), p.taps2.size(), p.rrc.size(), why.c_str());
	}
	return 0;
}

int chan()
{
	double rate;
	int sps;
	unsigned long long n_in;
	while (std::scanf("%lf %d %llu", &rate, &sps, &n_in) == 3) {
		ChanNumbers p;
		std::string why;
		const bool ok = plan_numbers(rate, sps, &p, &why);
		const StreamCounts c = ok ? p.counts(n_in) : StreamCounts{0, 0, 0};
		std::printf("%s %d %d %d %d %d %lld %lld %d %d %d %lld %lld %" PRIu64 " %" PRIu64 " %" PRIu64 " | %s\n", ok ? "ok" : "refused",
		            p.n_chans, p.ntaps(), p.n_blocks, p.rs.tpf, p.rs.j0, p.rs.num, p.rs.den, p.pre ? 1 : 0, p.pre_rs.tpf, p.pre_rs.j0,
		            p.pre_rs.num, p.pre_rs.den, c.a, c.b, c.out, why.c_str());
	}
	return 0;
}

int taps(const char *which, double rate, int sps)
{
	std::string why;
	if (!std::strcmp(which, "chan")) {
		ChanNumbers p;
		if (!plan_numbers(rate, sps, &p, &why))
			return 1;
		show("taps", p.taps);
		show("rrc", p.rrc);
		show("bank", p.bank);
		show("pre_taps", p.pre_taps);
		show("pre_bank", p.pre_bank);
	} else {
		DdcNumbers p;
		if (!plan_numbers(rate, sps, &p, &why))
			return 1;
		show("taps1", p.taps1);
		show("taps2", p.taps2);
		show("rrc", p.rrc);
		show("bank", p.bank);
	}
	return 0;
}

int carrier(double rate, int sps, int n, char **f)
{
	DdcNumbers p;
	std::string why;
	if (!plan_numbers(rate, sps, &p, &why))
		return 1;
	std::vector<double> freq, rot;
	for (int i = 0; i < n; i++)
		freq.push_back(std::atof(f[i]));
	std::vector<F2> t1;
	ddc_carrier_taps(p, n, freq.data(), t1, rot);
	show("t1", t1);
	std::printf("rot %zu", rot.size());
	for (double d : rot) {
		uint64_t u;
		std::memcpy(&u, &d, sizeof(u));
		std::printf(" %016" PRIx64, u);
	}
	std::printf("\n");
	return 0;
}

int select(int nch, int n, char **a)
{
	std::vector<int32_t> idx, slot;
	for (int i = 0; i < n; i++)
		idx.push_back(std::atoi(a[i]));
	std::string why;
	if (!select_channels(nch, n, idx.data(), slot, &why)) {
		std::printf("refused | %s\n", why.c_str());
		return 0;
	}
	std::printf("ok");
	for (int32_t s : slot)
		std::printf(" %d", s);
	std::printf("\n");
	return 0;
}

}  // namespace

int main(int argc, char **argv)
{
	const char *cmd = argc > 1 ? argv[1] : "";
	if (!std::strcmp(cmd, "ddc"))
		return ddc();
	if (!std::strcmp(cmd, "chan"))
		return chan();
	if (!std::strcmp(cmd, "taps") && argc == 5)
		return taps(argv[2], std::atof(argv[3]), std::atoi(argv[4]));
	if (!std::strcmp(cmd, "carrier") && argc >= 4)
		return carrier(std::atof(argv[2]), std::atoi(argv[3]), argc - 4, argv + 4);
	if (!std::strcmp(cmd, "select") && argc >= 3)
		return select(std::atoi(argv[2]), argc - 3, argv + 3);
	std::fprintf(stderr, "usage: chan_plan_host ddc|chan|taps|carrier|select ...\n");
	return 2;
}
