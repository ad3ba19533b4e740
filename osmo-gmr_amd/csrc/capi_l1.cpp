// capi_l1.cpp -- C-ABI entry points of the layer-1 decoders: BCCH and CCCH (l1_dev / l1_host, which the reference's
// one-burst decode calls in capi_one.cpp go through as well), FACCH3, TCH3.
#include "capi_common.h"

#include <osmocom/gmr1/l1/facch3.h>
#include <osmocom/gmr1/l1/tch3.h>

namespace gmr1 {

// BCCH / CCCH batch decode (chain: kChainBcch / kChainCcch); device pointers, then host pointers staged through HBM
int l1_dev(hipStream_t st, int chain, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	if (n < 0 || !ebits || !l2 || !crc || !conv)
		return fail(-EINVAL, "l1 decode: NULL argument");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	L1Args a;
	a.n = n; a.chain = chain; a.conv_acc = conv_acc(); a.ebits = ebits; a.l2 = l2; a.crc = crc; a.conv = conv;
	HIP_TRY(launch_l1(a, st));
	return 0;
}

int l1_host(int chain, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	const int neb = chain == kChainCcch ? 432 : 424;
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	Stage sg;
	const int8_t *d_eb = sg.in(ebits, (size_t)n * neb);
	uint8_t *d_l2 = sg.out(l2, (size_t)n * 24);
	int32_t *d_crc = sg.out(crc, (size_t)n);
	int32_t *d_conv = sg.out(conv, (size_t)n);
	if ((r = sg.err())) return r;
	r = l1_dev(nullptr, chain, n, d_eb, d_l2, d_crc, d_conv);
	if (r) return r;
	return sg.fetch();
}

}  // namespace gmr1

using namespace gmr1;

extern "C" {

int gmr1_hip_bcch_decode_batch_dev(void *stream, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	return l1_dev((hipStream_t)stream, kChainBcch, n, ebits, l2, crc, conv);
}

int gmr1_hip_ccch_decode_batch_dev(void *stream, int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	return l1_dev((hipStream_t)stream, kChainCcch, n, ebits, l2, crc, conv);
}

int gmr1_hip_bcch_decode_batch(int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	return l1_host(kChainBcch, n, ebits, l2, crc, conv);
}

int gmr1_hip_ccch_decode_batch(int n, const int8_t *ebits, uint8_t *l2, int32_t *crc, int32_t *conv)
{
	return l1_host(kChainCcch, n, ebits, l2, crc, conv);
}

int gmr1_hip_facch3_decode_batch_dev(void *stream, int n, const int8_t *ebits, const uint8_t *ciph,
                                     uint8_t *l2, uint8_t *bits_s, int32_t *crc, int32_t *conv)
{
	if (n < 0 || !ebits || !l2 || !crc || !conv)
		return fail(-EINVAL, "facch3 decode: NULL argument");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	Facch3Args a;
	a.n = n; a.conv_acc = conv_acc(); a.ebits = ebits; a.ciph = ciph; a.l2 = l2; a.bits_s = bits_s; a.crc = crc; a.conv = conv;
	HIP_TRY(launch_facch3(a, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_facch3_decode_batch(int n, const int8_t *ebits, const uint8_t *ciph,
                                 uint8_t *l2, uint8_t *bits_s, int32_t *crc, int32_t *conv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!ebits || !l2 || !crc || !conv)
		return fail(-EINVAL, "facch3 decode: NULL argument");
	Stage sg;
	const int8_t *d_eb = sg.in(ebits, (size_t)n * 416);
	const uint8_t *d_ci = sg.in(ciph, (size_t)n * 384);
	uint8_t *d_l2 = sg.out(l2, (size_t)n * 10);
	uint8_t *d_s = sg.out_always(bits_s, (size_t)n * 32);
	int32_t *d_crc = sg.out(crc, (size_t)n);
	int32_t *d_conv = sg.out(conv, (size_t)n);
	if ((r = sg.err())) return r;
	r = gmr1_hip_facch3_decode_batch_dev(nullptr, n, d_eb, d_ci, d_l2, d_s, d_crc, d_conv);
	if (r) return r;
	return sg.fetch();
}

int gmr1_hip_tch3_decode_batch_dev(void *stream, int n, int m, const int8_t *ebits, const uint8_t *ciph,
                                   uint8_t *frames, uint8_t *bits_s, int32_t *conv)
{
	if (n < 0 || !ebits || !frames)
		return fail(-EINVAL, "tch3 decode: NULL argument");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	Tch3Args a;
	a.n = n; a.m = m ? 1 : 0; a.conv_acc = conv_acc(); a.ebits = ebits; a.ciph = ciph; a.frames = frames; a.bits_s = bits_s; a.conv = conv;
	HIP_TRY(launch_tch3(a, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_tch3_decode_batch(int n, int m, const int8_t *ebits, const uint8_t *ciph,
                               uint8_t *frames, uint8_t *bits_s, int32_t *conv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!ebits || !frames)
		return fail(-EINVAL, "tch3 decode: NULL argument");
	Stage sg;
	const int8_t *d_eb = sg.in(ebits, (size_t)n * 212);
	const uint8_t *d_ci = sg.in(ciph, (size_t)n * 208);
	uint8_t *d_fr = sg.out(frames, (size_t)n * 20);
	uint8_t *d_s = sg.out_always(bits_s, (size_t)n * 4);
	int32_t *d_conv = sg.out_always(conv, (size_t)n * 2);
	if ((r = sg.err())) return r;
	r = gmr1_hip_tch3_decode_batch_dev(nullptr, n, m, d_eb, d_ci, d_fr, d_s, d_conv);
	if (r) return r;
	return sg.fetch();
}

// ---- reference-compatible single calls ---------------------------------------------------------
int gmr1_facch3_decode(uint8_t *l2, ubit_t *bits_s, const sbit_t *bits_e, const ubit_t *ciph, int *conv_rv)
{
	int32_t crc = 0, conv = 0;
	int r = gmr1_hip_facch3_decode_batch(1, reinterpret_cast<const int8_t *>(bits_e), ciph, l2, bits_s, &crc, &conv);
	if (r) return r;
	if (conv_rv) *conv_rv = conv;
	return crc;
}

void gmr1_tch3_decode(uint8_t *frame0, uint8_t *frame1, ubit_t *bits_s,
                      const sbit_t *bits_e, const ubit_t *ciph, int m, int *conv0_rv, int *conv1_rv)
{
	// the reference returns void: a device failure leaves the outputs zeroed and is
	// reported through gmr1_hip_last_error()
	uint8_t fr[20] = {0};
	uint8_t st[4] = {0};
	int32_t conv[2] = {0, 0};
	(void)gmr1_hip_tch3_decode_batch(1, m, reinterpret_cast<const int8_t *>(bits_e), ciph, fr, st, conv);
	std::memcpy(frame0, fr, 10);
	std::memcpy(frame1, fr + 10, 10);
	if (bits_s) std::memcpy(bits_s, st, 4);
	if (conv0_rv) *conv0_rv = conv[0];
	if (conv1_rv) *conv1_rv = conv[1];
}

}  // extern "C"
