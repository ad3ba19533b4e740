// capi_tch.cpp -- C ABI of the DKAB demodulator and the A5 keystream generator
// (reference include/osmocom/gmr1/sdr/dkab.h:39-41, include/osmocom/gmr1/l1/a5.h:37-41).

#include "capi_common.h"

#include <vector>

#include "../../include/gmr1_hip.h"
#include "../../include/osmocom/gmr1/sdr/dkab.h"
#include "../../include/osmocom/gmr1/l1/a5.h"

using namespace gmr1;

namespace {
constexpr int kDkabMaxLen = 4096;
}

extern "C" {

int gmr1_hip_dkab_demod_batch_dev(void *stream, int n, int sps, int in_len,
                                  const float *iq, const uint64_t *offset, const float *freq_shift,
                                  const int32_t *p, int8_t *ebits, float *toa, int32_t *rv)
{
	if (n < 0 || !iq || !offset || !p || !rv)
		return fail(-EINVAL, "dkab: iq/offset/p/rv are required");
	if (sps < 1 || sps > 16)
		return fail(-EINVAL, "dkab: sps=%d out of range (1..16)", sps);
	const int w = in_len - GMR1_DKAB_SYMS * sps + 1;
	if (w <= 0)
		return fail(-EINVAL, "dkab: window of %d samples is shorter than a DKAB (%d)", in_len, GMR1_DKAB_SYMS * sps);
	if (in_len > kDkabMaxLen)
		return fail(-EINVAL, "dkab: window of %d samples (<= %d supported)", in_len, kDkabMaxLen);
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	DkabArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.sps = sps; a.in_len = in_len;
	a.iq = reinterpret_cast<const float2 *>(iq);
	a.offset = offset; a.freq_shift = freq_shift; a.p = p;
	a.ebits = ebits; a.toa = toa; a.rv = rv;
	HIP_TRY(launch_dkab(a, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_dkab_demod_batch(int n, int sps, int in_len,
                              const float *iq, uint64_t iq_len, const uint64_t *offset, const float *freq_shift,
                              const int32_t *p, int8_t *ebits, float *toa, int32_t *rv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!iq || !offset || !p || !rv)
		return fail(-EINVAL, "dkab: iq/offset/p/rv are required");
	if ((r = bursts_fit(n, offset, in_len, iq_len))) return r;
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const uint64_t *d_off = sg.in(offset, (size_t)n);
	const int32_t *d_p = sg.in(p, (size_t)n);
	const float *d_fs = sg.in(freq_shift, (size_t)n);
	int32_t *d_rv = sg.out(rv, (size_t)n);
	int8_t *d_eb = sg.out_always(ebits, (size_t)n * 8);
	float *d_toa = sg.out_always(toa, (size_t)n);
	if ((r = sg.err())) return r;
	r = gmr1_hip_dkab_demod_batch_dev(nullptr, n, sps, in_len, d_iq, d_off, d_fs, d_p, d_eb, d_toa, d_rv);
	if (r) return r;
	return sg.fetch();
}

int gmr1_dkab_demod(struct osmo_cxvec *burst_in, int sps, float freq_shift, int p, sbit_t *ebits, float *toa_p)
{
	if (!burst_in || !burst_in->data || !ebits || !toa_p)
		return fail(-EINVAL, "gmr1_dkab_demod: NULL argument");
	const uint64_t off = 0;
	int32_t rv = 0, pp = p;
	float toa = 0.f;
	int8_t eb[8];
	int r = gmr1_hip_dkab_demod_batch(1, sps, burst_in->len, reinterpret_cast<const float *>(burst_in->data),
	                                  (uint64_t)burst_in->len, &off, &freq_shift, &pp, eb, &toa, &rv);
	if (r) return r;
	*toa_p = toa;
	if (rv == 0)
		std::memcpy(ebits, eb, 8);
	return rv;
}

int gmr1_hip_a5_batch_dev(void *stream, int n, int alg, int nbits,
                          const uint8_t *keys, const uint32_t *fn, uint8_t *dl, uint8_t *ul)
{
	if (n < 0 || nbits < 0 || (alg == 1 && (!keys || !fn)))
		return fail(-EINVAL, "a5: keys / fn are required for A5/1");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	A5Args a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.alg = alg; a.nbits = nbits; a.keys = keys; a.fn = fn; a.dl = dl; a.ul = ul;
	HIP_TRY(launch_a5(a, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_a5_batch(int n, int alg, int nbits, const uint8_t *keys, const uint32_t *fn, uint8_t *dl, uint8_t *ul)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0 || nbits <= 0) return 0;
	if (alg == 1 && (!keys || !fn))
		return fail(-EINVAL, "a5: keys / fn are required for A5/1");
	Stage sg;
	const size_t nb = (size_t)n * nbits;
	const uint8_t *d_k = sg.in(keys, (size_t)n * 8);
	const uint32_t *d_fn = sg.in(fn, (size_t)n);
	// the buffers start out as the caller's, so that "unsupported n" leaves them untouched
	uint8_t *d_dl = sg.inout(dl, nb);
	uint8_t *d_ul = sg.inout(ul, nb);
	if ((r = sg.err())) return r;
	r = gmr1_hip_a5_batch_dev(nullptr, n, alg, nbits, d_k, d_fn, d_dl, d_ul);
	if (r) return r;
	return sg.fetch();
}

void gmr1_a5(int n, uint8_t *key, uint32_t fn, int nbits, ubit_t *dl, ubit_t *ul)
{
	(void)gmr1_hip_a5_batch(1, n, nbits, key, &fn, reinterpret_cast<uint8_t *>(dl), reinterpret_cast<uint8_t *>(ul));
}

void gmr1_a5_1(uint8_t *key, uint32_t fn, int nbits, ubit_t *dl, ubit_t *ul)
{
	gmr1_a5(1, key, fn, nbits, dl, ul);
}

}  // extern "C"
