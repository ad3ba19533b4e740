// Host-side exercise of osmo-gmr_amd/csrc/ambe_calls.h (which records of the TCH3 follower a call of the speech decoder
// owns, and which of them are speech; the device runs it in k_ambe_calls).  tests/test_tch3_voice_host.py compares the
// result with a direct restatement.
//   first line printed: ambe_calls_is_speech(type) for type = 0 .. 255, and the record layout the header states
//   then per line of stdin "n_frames n_calls first[0] .. first[n_calls]": "lo hi" of every call, on one line
#include <cstdio>
#include <vector>

#include "ambe_calls.h"

using namespace gmr1;

int main()
{
	for (unsigned type = 0; type < 256; type++)
		printf("%d ", ambe_calls_is_speech(type) ? 1 : 0);
	printf("%d %d %d %d %d\n", kAmbeRecBytes, kAmbeRecType, kAmbeRecL2, kAmbeRecFrames, kAmbeRecSpeech);
	int n_frames, n_calls;
	while (scanf("%d %d", &n_frames, &n_calls) == 2) {
		if (n_calls < 0)
			return 2;
		std::vector<int32_t> first((size_t)n_calls + 1);           // exactly as long as the entry reads: ASan sees one past
		for (int c = 0; c <= n_calls; c++)
			if (scanf("%d", &first[c]) != 1)
				return 3;
		for (int c = 0; c < n_calls; c++) {
			const AmbeSpan s = ambe_calls_span(first.data(), c, n_frames);
			printf("%d %d ", s.lo, s.hi);
		}
		printf("\n");
	}
	return 0;
}
