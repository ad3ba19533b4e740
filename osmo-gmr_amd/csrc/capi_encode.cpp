// capi_encode.cpp -- C ABI of the batched layer-1 channel encoders (include/gmr1_hip.h).  A chain is an EncPlan, written
// down on the host by enc_plan.cpp and uploaded here once per chain and device; every bit of every burst is computed on the
// GPU by k_encode (tx_kernels.hip).  The reference's own single calls run through encode_host too: capi_tx_ref.cpp.

#include "capi_common.h"

#include "../../include/gmr1_hip.h"
#include "../../include/osmocom/gmr1/l1/tch9.h"
#include "dev_cache.h"

using namespace gmr1;

namespace {

struct DevPlan { EncPlan host; EncPlan *d; };
DevCache<int, DevPlan> g_plans;

// What every encode starts with, in this order: the device's state, n, the chain's plan on the current device, the arrays
// the plan asks for.  *p stays null where there is nothing to do (n == 0).
int encode_begin(int id, int n, int seq_len, const EncIo &io, const char *what, const DevPlan **p)
{
	*p = nullptr;
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n < 0)
		return fail(-EINVAL, "%s: n < 0", what);
	if (n == 0)
		return 0;
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	const DevPlan *dp;
	r = g_plans.get(dev, id, &dp, [id](DevPlan *e) {
		build_enc_plan(id, &e->host);
		return upload(&e->d, std::vector<EncPlan>(1, e->host));
	});
	if (r) return r;
	const EncPlan &h = dp->host;
	if (!io.in0 || !io.ebits || (h.n_in1 && !io.in1) || (h.n_aux0 && !io.aux0) || (h.n_aux1 && !io.aux1))
		return fail(-EINVAL, "%s: a required array is NULL", what);
	if (h.depth > 1 && (seq_len < 1 || n % seq_len))
		return fail(-EINVAL, "%s: %d bursts are not a whole number of runs of %d", what, n, seq_len);
	*p = dp;
	return 0;
}

// every pointer is device memory; the arguments have passed encode_begin
int encode_enqueue(hipStream_t st, const DevPlan &p, int n, int seq_len, const EncIo &io)
{
	EncArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.seq_len = p.host.depth > 1 ? seq_len : 1; a.plan = p.d;
	a.in0 = io.in0; a.in1 = io.in1; a.aux0 = io.aux0; a.aux1 = io.aux1; a.ciph = io.ciph; a.ebits = io.ebits;
	HIP_TRY(launch_encode(a, st));
	return 0;
}

}  // namespace

namespace gmr1 {

int encode_dev(hipStream_t st, int id, int n, int seq_len, const EncIo &io, const char *what)
{
	const DevPlan *p;
	const int r = encode_begin(id, n, seq_len, io, what, &p);
	return r || !p ? r : encode_enqueue(st, *p, n, seq_len, io);
}

// H2D -> kernel -> D2H
int encode_host(int id, int n, int seq_len, const EncIo &io, const char *what)
{
	const DevPlan *p;
	int r = encode_begin(id, n, seq_len, io, what, &p);
	if (r || !p) return r;
	const EncPlan &h = p->host;
	const size_t nn = (size_t)n;
	Stage sg;
	auto in = [&](const uint8_t *src, int per) { return per ? sg.in(src, (size_t)per * nn) : nullptr; };
	const EncIo d = {in(io.in0, h.n_in0), in(io.in1, h.n_in1), in(io.aux0, h.n_aux0), in(io.aux1, h.n_aux1), in(io.ciph, h.n_ciph),
	                 sg.out(io.ebits, (size_t)h.n_out * nn)};
	if ((r = sg.err())) return r;
	r = encode_enqueue(nullptr, *p, n, seq_len, d);
	if (r) return r;
	return sg.fetch();
}

int tch9_plan(int mode) { return mode == GMR1_TCH9_2k4 ? kPlTch9_2k4 : mode == GMR1_TCH9_4k8 ? kPlTch9_4k8 : mode == GMR1_TCH9_9k6 ? kPlTch9_9k6 : -1; }

}  // namespace gmr1

extern "C" {

int gmr1_hip_bcch_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlBcch, n, 1, {.in0 = l2, .ebits = ebits}, "bcch_encode");
}
int gmr1_hip_bcch_encode_batch(int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_host(kPlBcch, n, 1, {.in0 = l2, .ebits = ebits}, "bcch_encode");
}
int gmr1_hip_ccch_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlCcch, n, 1, {.in0 = l2, .ebits = ebits}, "ccch_encode");
}
int gmr1_hip_ccch_encode_batch(int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_host(kPlCcch, n, 1, {.in0 = l2, .ebits = ebits}, "ccch_encode");
}
int gmr1_hip_xch_dc12_encode_batch_dev(void *stream, int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlXch, n, 1, {.in0 = l2, .ebits = ebits}, "xch_dc12_encode");
}
int gmr1_hip_xch_dc12_encode_batch(int n, const uint8_t *l2, uint8_t *ebits)
{
	return encode_host(kPlXch, n, 1, {.in0 = l2, .ebits = ebits}, "xch_dc12_encode");
}
int gmr1_hip_facch3_encode_batch_dev(void *stream, int n, const uint8_t *l2, const uint8_t *bits_s, const uint8_t *ciph,
                                     uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlFacch3, n, 1, {.in0 = l2, .aux0 = bits_s, .ciph = ciph, .ebits = ebits}, "facch3_encode");
}
int gmr1_hip_facch3_encode_batch(int n, const uint8_t *l2, const uint8_t *bits_s, const uint8_t *ciph, uint8_t *ebits)
{
	return encode_host(kPlFacch3, n, 1, {.in0 = l2, .aux0 = bits_s, .ciph = ciph, .ebits = ebits}, "facch3_encode");
}
int gmr1_hip_tch3_encode_batch_dev(void *stream, int n, int m, const uint8_t *frames, const uint8_t *bits_s,
                                   const uint8_t *ciph, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, m ? kPlTch3M1 : kPlTch3M0, n, 1,
	                  {.in0 = frames, .aux0 = bits_s, .ciph = ciph, .ebits = ebits}, "tch3_encode");
}
int gmr1_hip_tch3_encode_batch(int n, int m, const uint8_t *frames, const uint8_t *bits_s, const uint8_t *ciph,
                               uint8_t *ebits)
{
	return encode_host(m ? kPlTch3M1 : kPlTch3M0, n, 1, {.in0 = frames, .aux0 = bits_s, .ciph = ciph, .ebits = ebits}, "tch3_encode");
}
int gmr1_hip_facch9_encode_batch_dev(void *stream, int n, const uint8_t *l2, const uint8_t *sacch, const uint8_t *status,
                                     const uint8_t *ciph, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlFacch9, n, 1, {.in0 = l2, .aux0 = sacch, .aux1 = status, .ciph = ciph, .ebits = ebits},
	                  "facch9_encode");
}
int gmr1_hip_facch9_encode_batch(int n, const uint8_t *l2, const uint8_t *sacch, const uint8_t *status,
                                 const uint8_t *ciph, uint8_t *ebits)
{
	return encode_host(kPlFacch9, n, 1, {.in0 = l2, .aux0 = sacch, .aux1 = status, .ciph = ciph, .ebits = ebits}, "facch9_encode");
}
int gmr1_hip_tch9_encode_batch_dev(void *stream, int mode, int n, int seq_len, const uint8_t *l2, const uint8_t *sacch,
                                   const uint8_t *status, const uint8_t *ciph, uint8_t *ebits)
{
	if (tch9_plan(mode) < 0)
		return fail(-EINVAL, "tch9_encode: mode %d unknown", mode);
	return encode_dev((hipStream_t)stream, tch9_plan(mode), n, seq_len,
	                  {.in0 = l2, .aux0 = sacch, .aux1 = status, .ciph = ciph, .ebits = ebits}, "tch9_encode");
}
int gmr1_hip_tch9_encode_batch(int mode, int n, int seq_len, const uint8_t *l2, const uint8_t *sacch,
                               const uint8_t *status, const uint8_t *ciph, uint8_t *ebits)
{
	if (tch9_plan(mode) < 0)
		return fail(-EINVAL, "tch9_encode: mode %d unknown", mode);
	return encode_host(tch9_plan(mode), n, seq_len, {.in0 = l2, .aux0 = sacch, .aux1 = status, .ciph = ciph, .ebits = ebits},
	                   "tch9_encode");
}
int gmr1_hip_rach_encode_batch_dev(void *stream, int n, const uint8_t *rach, const uint8_t *sb_mask, uint8_t *ebits)
{
	return encode_dev((hipStream_t)stream, kPlRach, n, 1, {.in0 = rach, .in1 = sb_mask, .ebits = ebits}, "rach_encode");
}
int gmr1_hip_rach_encode_batch(int n, const uint8_t *rach, const uint8_t *sb_mask, uint8_t *ebits)
{
	return encode_host(kPlRach, n, 1, {.in0 = rach, .in1 = sb_mask, .ebits = ebits}, "rach_encode");
}

// the position map of one chain as the kernel reads it (struct EncPlan, csrc/enc_plan.h); host-only, works without a GPU
int gmr1_hip_encoder_plan(int chain, void *buf, int buf_len)
{
	if (chain < 0 || chain >= kPlCount)
		return fail(-EINVAL, "gmr1_hip_encoder_plan: chain %d unknown", chain);
	if (buf) {
		if (buf_len < (int)sizeof(EncPlan))
			return fail(-EINVAL, "gmr1_hip_encoder_plan: the plan has %d bytes", (int)sizeof(EncPlan));
		build_enc_plan(chain, static_cast<EncPlan *>(buf));
	}
	return (int)sizeof(EncPlan);
}

}  // extern "C"
