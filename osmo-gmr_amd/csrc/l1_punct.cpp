// l1_punct.cpp -- gmr1_puncturer_generate (reference src/l1/punct.c:48-133): host code, no GPU involved.  The walk over
// the first / main / last block is l1_codes.h's punctured_bits, the one the GPU path's maps and plans are built with.
#include <errno.h>
#include <stdlib.h>

#include <vector>

#include <osmocom/gmr1/l1/conv.h>
#include <osmocom/gmr1/l1/punct.h>

#include "l1_codes.h"

using namespace gmr1;

namespace {

// coded bits of the unpunctured stream (libosmocore's osmo_conv_get_output_length(code, 0) [3P]): one N-bit word per
// data bit, K - 1 more for a flushed code, less whatever an already attached puncture list removes
int coded_length(const struct osmo_conv_code *code)
{
	const int steps = code->len + (code->term == CONV_TERM_FLUSH ? code->K - 1 : 0);
	int n = steps * code->N;
	if (code->puncture)
		for (const int *p = code->puncture; *p >= 0; p++)
			n--;
	return n;
}

l1c::Scheme scheme(const struct gmr1_puncturer *p) { return p ? l1c::Scheme{p->L * p->N, p->mask} : l1c::kNoScheme; }

}  // namespace

extern "C" int gmr1_puncturer_generate(struct osmo_conv_code *code, const struct gmr1_puncturer *punct_pre,
                                       const struct gmr1_puncturer *punct_main, const struct gmr1_puncturer *punct_post,
                                       int repeat)
{
	if (!code || !punct_main)
		return -EINVAL;
	const int N = code->N;
	if ((punct_pre && punct_pre->N != N) || punct_main->N != N || (punct_post && punct_post->N != N))
		return -EINVAL;

	const int total = coded_length(code);
	std::vector<uint8_t> flag(total > 0 ? total : 0, 0);
	l1c::punctured_bits(flag.data(), total, scheme(punct_pre), scheme(punct_main), scheme(punct_post), repeat);
	size_t n = 0;
	for (uint8_t f : flag)
		n += f;

	int *p = static_cast<int *>(malloc((n + 1) * sizeof(int)));
	if (!p)
		return -ENOMEM;
	n = 0;
	for (int i = 0; i < total; i++)
		if (flag[i])
			p[n++] = i;
	p[n] = -1;
	code->puncture = p;
	return 0;
}
