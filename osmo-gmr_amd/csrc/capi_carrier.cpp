// capi_carrier.cpp -- C ABI of the last step of the transmit direction: FCCH chirp windows (k_chirp, tx_kernels.hip) and the
// carrier mixer (k_carrier_mix, carrier_kernels.hip), which turns the windows the shaped modulator and the chirp entry make
// into carriers -- what everything behind the demodulator reads.  The reference has no transmitter; the contract is
// include/gmr1_hip.h's.  The host forms validate what they can see, stage through Stage and block; the _dev forms enqueue.

#include "capi_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/gmr1_hip.h"
#include "../../include/osmocom/gmr1/sdr/fcch.h"
#include "tx_pulse.h"

namespace gmr1 {

int HostWindows::check(const char *who, int n, int in_len, const uint64_t *offset, uint64_t out_len)
{
	order.assign(offset, offset + n);
	for (int b = 0; b < n; b++)
		if (offset[b] > out_len || (uint64_t)in_len > out_len - offset[b])
			return fail(-EINVAL, "%s: window %d leaves the %llu samples of out", who, b, (unsigned long long)out_len);
	std::sort(order.begin(), order.end());
	for (int b = 1; b < n; b++)
		if (order[b] - order[b - 1] < (uint64_t)in_len)
			return fail(-EINVAL, "%s: the windows at samples %llu and %llu overlap", who, (unsigned long long)order[b - 1],
			            (unsigned long long)order[b]);
	return 0;
}

float *HostWindows::stage(Stage &sg, int in_len, const uint64_t *offset, float *out, const uint64_t **d_offset)
{
	// the device copy of out covers the windows' hull; the offsets are taken relative to its first sample
	const size_t n = order.size();
	const uint64_t lo = order.front(), hull = order.back() + (uint64_t)in_len - lo;
	rel_.assign(offset, offset + n);
	for (uint64_t &o : rel_)
		o -= lo;
	*d_offset = sg.in(rel_.data(), n);
	float *d_out = sg.dev<float>((size_t)hull * 2);
	for (size_t b = 0, first = 0; b < n; b++)          // one copy back per run of windows that touch
		if (b + 1 == n || order[b + 1] - order[b] > (uint64_t)in_len) {
			sg.back(out + 2 * order[first], d_out + 2 * (order[first] - lo), (size_t)(order[b] + (uint64_t)in_len - order[first]) * 2);
			first = b + 1;
		}
	return d_out;
}

}  // namespace gmr1

using namespace gmr1;

namespace {

// ---- FCCH chirp windows ---------------------------------------------------------------------------------------------
// what both forms refuse without looking at an array
int chirp_check(const char *who, int fcch_type, int n, int sps, int in_len, const uint64_t *offset, const float *out)
{
	if (chirp_args_bad(fcch_type, n, sps, in_len))
		return fail(-EINVAL, "%s: fcch_type %d (0..2), n %d, sps %d (1..%d) or in_len %d is out of range", who, fcch_type, n, sps,
		            kShapeMaxSps, in_len);
	if (n > 0 && (!offset || !out))
		return fail(-EINVAL, "%s: offset and out are required", who);
	return 0;
}

// every pointer is device memory; the arguments have passed chirp_check
int chirp_enqueue(hipStream_t st, int fcch_type, int n, int sps, int in_len, const uint64_t *offset, const int32_t *start,
                  const float *frac, const float *cfo, const float *phase0, const float *gain, float *out)
{
	ChirpArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.len = kFcchBuiltin[fcch_type]->len; a.sps = sps; a.in_len = in_len;
	a.freq = (double)kFcchBuiltin[fcch_type]->freq;
	a.offset = offset; a.start = start; a.frac = frac; a.cfo = cfo; a.phase0 = phase0; a.gain = gain;
	a.out = reinterpret_cast<float2 *>(out);
	HIP_TRY(launch_chirp(a, st));
	return 0;
}

// ---- the mixer --------------------------------------------------------------------------------------------------------
// what both forms refuse without looking at an array.  Segments are present where seg_first is given.
int mix_check(const char *who, int n_carriers, const float *seg_iq, const int32_t *seg_first, const uint64_t *seg_src,
              const int64_t *seg_pos, const uint32_t *seg_len, uint32_t max_seg_len, const uint64_t *out_offset,
              const uint64_t *length, const float *out)
{
	if (n_carriers < 0)
		return fail(-EINVAL, "%s: n_carriers %d", who, n_carriers);
	if (n_carriers > 0 && (!out_offset || !length || !out))
		return fail(-EINVAL, "%s: out_offset, length and out are required", who);
	if (seg_first && (!seg_iq || !seg_src || !seg_pos || !seg_len))
		return fail(-EINVAL, "%s: with seg_first, seg_iq, seg_src, seg_pos and seg_len are required", who);
	if (seg_first && max_seg_len == 0)
		return fail(-EINVAL, "%s: max_seg_len is 0 with segments present", who);
	return 0;
}

}  // namespace

extern "C" {

int gmr1_hip_fcch_chirp_batch_dev(void *stream, int fcch_type, int n, int sps, int in_len,
                                  const uint64_t *offset, const int32_t *start, const float *frac, const float *cfo,
                                  const float *phase0, const float *gain, float *out, uint64_t out_len)
{
	(void)out_len;
	int r = chirp_check("fcch_chirp_batch_dev", fcch_type, n, sps, in_len, offset, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0)
		return 0;
	return chirp_enqueue((hipStream_t)stream, fcch_type, n, sps, in_len, offset, start, frac, cfo, phase0, gain, out);
}

int gmr1_hip_fcch_chirp_batch(int fcch_type, int n, int sps, int in_len,
                              const uint64_t *offset, const int32_t *start, const float *frac, const float *cfo,
                              const float *phase0, const float *gain, float *out, uint64_t out_len)
{
	const char *who = "fcch_chirp_batch";
	int r = chirp_check(who, fcch_type, n, sps, in_len, offset, out);
	if (r) return r;
	HostWindows win;
	if ((r = win.check(who, n, in_len, offset, out_len))) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0)
		return 0;
	Stage sg;
	const size_t nn = (size_t)n;
	const int32_t *d_start = sg.in(start, nn);
	const float *d_frac = sg.in(frac, nn), *d_cfo = sg.in(cfo, nn), *d_ph = sg.in(phase0, nn), *d_gain = sg.in(gain, nn);
	const uint64_t *d_off;
	float *d_out = win.stage(sg, in_len, offset, out, &d_off);
	if ((r = sg.err())) return r;
	r = chirp_enqueue(nullptr, fcch_type, n, sps, in_len, d_off, d_start, d_frac, d_cfo, d_ph, d_gain, d_out);
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_carrier_mix_dev(void *stream, int n_carriers, const float *seg_iq, const int32_t *seg_first,
                             const uint64_t *seg_src, const int64_t *seg_pos, const uint32_t *seg_len, uint32_t max_seg_len,
                             const uint64_t *out_offset, const uint64_t *length, uint64_t max_length, const int64_t *first,
                             const float *sigma, const double *cfo, const uint32_t *noise_id, uint64_t seed, float *out)
{
	int r = mix_check("carrier_mix_dev", n_carriers, seg_iq, seg_first, seg_src, seg_pos, seg_len, max_seg_len, out_offset, length, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_carriers == 0)
		return 0;
	MixArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n_carriers = n_carriers;
	a.seg_iq = reinterpret_cast<const float2 *>(seg_iq);
	a.seg_first = seg_first; a.seg_src = seg_src; a.seg_pos = reinterpret_cast<const long long *>(seg_pos); a.seg_len = seg_len;
	a.max_seg_len = max_seg_len;
	a.out_offset = out_offset; a.length = length; a.max_length = max_length;
	a.first = reinterpret_cast<const long long *>(first);
	a.sigma = sigma; a.cfo = cfo; a.noise_id = noise_id; a.seed = seed;
	a.out = reinterpret_cast<float2 *>(out);
	HIP_TRY(launch_carrier_mix(a, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_carrier_mix(int n_carriers, const float *seg_iq, uint64_t seg_iq_len, int n_seg, const int32_t *seg_first,
                         const uint64_t *seg_src, const int64_t *seg_pos, const uint32_t *seg_len, uint32_t max_seg_len,
                         const uint64_t *out_offset, const uint64_t *length, uint64_t max_length, const int64_t *first,
                         const float *sigma, const double *cfo, const uint32_t *noise_id, uint64_t seed,
                         float *out, uint64_t out_len)
{
	const char *who = "carrier_mix";
	if (n_seg < 0)
		return fail(-EINVAL, "%s: n_seg %d", who, n_seg);
	if (n_seg > 0 && !seg_first)
		return fail(-EINVAL, "%s: %d segments without seg_first", who, n_seg);
	int r = mix_check(who, n_carriers, seg_iq, n_seg > 0 ? seg_first : nullptr, seg_src, seg_pos, seg_len, max_seg_len, out_offset,
	                  length, out);
	if (r) return r;
	// the arrays are in reach here: the segment lists, the segments, the carriers in out, the noise levels
	if (seg_first) {
		if (seg_first[0] != 0 || (n_carriers > 0 && seg_first[n_carriers] != n_seg) || (n_carriers == 0 && n_seg != 0))
			return fail(-EINVAL, "%s: seg_first does not run from 0 to n_seg = %d", who, n_seg);
		for (int c = 0; c < n_carriers; c++)
			if (seg_first[c + 1] < seg_first[c])
				return fail(-EINVAL, "%s: seg_first decreases at carrier %d", who, c);
	}
	for (int c = 0; c < n_carriers && n_seg > 0; c++)
		for (int s = seg_first[c]; s < seg_first[c + 1]; s++) {
			if (seg_len[s] > max_seg_len)
				return fail(-EINVAL, "%s: segment %d has %u samples, max_seg_len is %u", who, s, seg_len[s], max_seg_len);
			if (s > seg_first[c] && seg_pos[s] < seg_pos[s - 1])
				return fail(-EINVAL, "%s: the segments of carrier %d are not sorted by pos (segment %d)", who, c, s);
			if (seg_src[s] > seg_iq_len || (uint64_t)seg_len[s] > seg_iq_len - seg_src[s])
				return fail(-EINVAL, "%s: segment %d leaves the %llu samples of seg_iq", who, s, (unsigned long long)seg_iq_len);
		}
	std::vector<std::pair<uint64_t, uint64_t>> span;          // (offset, length) of the carriers that have samples
	for (int c = 0; c < n_carriers; c++) {
		if (length[c] > max_length)
			return fail(-EINVAL, "%s: carrier %d has %llu samples, max_length is %llu", who, c, (unsigned long long)length[c],
			            (unsigned long long)max_length);
		if (out_offset[c] > out_len || length[c] > out_len - out_offset[c])
			return fail(-EINVAL, "%s: carrier %d leaves the %llu samples of out", who, c, (unsigned long long)out_len);
		if (sigma && !(sigma[c] >= 0.f && std::isfinite(sigma[c])))
			return fail(-EINVAL, "%s: sigma of carrier %d is negative or not finite", who, c);
		if (length[c])
			span.push_back({out_offset[c], length[c]});
	}
	std::sort(span.begin(), span.end());
	for (size_t i = 1; i < span.size(); i++)
		if (span[i].first - span[i - 1].first < span[i - 1].second)
			return fail(-EINVAL, "%s: the carriers at samples %llu and %llu of out overlap", who,
			            (unsigned long long)span[i - 1].first, (unsigned long long)span[i].first);
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n_carriers == 0 || span.empty())
		return 0;
	// the device copy of out covers the carriers' hull; only the carriers are copied back, so what lies between them stays
	const uint64_t lo = span.front().first, hull = span.back().first + span.back().second - lo;
	std::vector<uint64_t> rel(out_offset, out_offset + n_carriers);
	for (int c = 0; c < n_carriers; c++)
		rel[c] = length[c] ? rel[c] - lo : 0;
	Stage sg;
	const size_t nc = (size_t)n_carriers, ns = (size_t)n_seg;
	const float *d_iq = n_seg > 0 ? sg.in(seg_iq, (size_t)seg_iq_len * 2) : nullptr;
	const int32_t *d_first_seg = n_seg > 0 ? sg.in(seg_first, nc + 1) : nullptr;
	const uint64_t *d_src = n_seg > 0 ? sg.in(seg_src, ns) : nullptr;
	const int64_t *d_pos = n_seg > 0 ? sg.in(seg_pos, ns) : nullptr;
	const uint32_t *d_len = n_seg > 0 ? sg.in(seg_len, ns) : nullptr;
	const uint64_t *d_off = sg.in(rel.data(), nc), *d_length = sg.in(length, nc);
	const int64_t *d_first = sg.in(first, nc);
	const float *d_sigma = sg.in(sigma, nc);
	const double *d_cfo = sg.in(cfo, nc);
	const uint32_t *d_id = sg.in(noise_id, nc);
	float *d_out = sg.dev<float>((size_t)hull * 2);
	if ((r = sg.err())) return r;
	for (const auto &sp : span)
		sg.back(out + 2 * sp.first, d_out + 2 * (sp.first - lo), (size_t)sp.second * 2);
	r = gmr1_hip_carrier_mix_dev(nullptr, n_carriers, d_iq, d_first_seg, d_src, d_pos, d_len, max_seg_len, d_off, d_length, max_length,
	                             d_first, d_sigma, d_cfo, d_id, seed, d_out);
	if (r) return r;
	return sg.fetch();
}

}  // extern "C"
