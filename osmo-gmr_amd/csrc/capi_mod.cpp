// capi_mod.cpp -- C ABI of the modulators: gmr1_pi4cxpsk_mod (reference include/osmocom/gmr1/sdr/pi4cxpsk.h:115-117) and its
// batch forms, one sample per symbol (k_mod), and the shaped modulator past where the reference ends (k_shape; tx_pulse.h).
// The host writes down the per-symbol plan and the rotation phasors of a burst format; the samples are made on the GPU.

#include "capi_common.h"

#include <cmath>

#include "../../include/gmr1_hip.h"
#include "../../include/osmocom/gmr1/sdr/pi4cxpsk.h"
#include "dev_cache.h"
#include "tx_pulse.h"

using namespace gmr1;

namespace {

// per-symbol plan of one (burst format, sync sequence): -1 guard, 0..3 training symbol, 4 + k data symbol from ebits[k..]
int mod_plan(const gmr1_hip_burst_flat &f, int sync_id, std::vector<int16_t> *out)
{
	if (sync_id < 0 || sync_id >= f.n_sync)
		return -EINVAL;
	if (f.len < 1 || f.len > 4096 || (f.nbits != 1 && f.nbits != 2))
		return -EINVAL;
	out->assign(f.len, -1);
	for (int c = 0; c < f.n_sync_chunks[sync_id]; c++) {
		const gmr1_hip_chunk &cs = f.sync[sync_id][c];
		for (int i = 0; i < cs.len; i++) {
			if (cs.pos + i < 0 || cs.pos + i >= f.len)
				return -EINVAL;
			(*out)[cs.pos + i] = (int16_t)(cs.syms[i] & 3);
		}
	}
	int k = 0;
	for (int c = 0; c < f.n_data; c++)
		for (int i = 0; i < f.data[c].len; i++, k += f.nbits) {
			const int p = f.data[c].pos + i;
			if (p < 0 || p >= f.len)
				return -EINVAL;
			(*out)[p] = (int16_t)(4 + k);
		}
	return 0;
}

// osmo_cxvec_rotate: sample i times e^{j (rotation * i)}, phase and phasor in single precision
std::vector<float2> mod_rot(const gmr1_hip_burst_flat &f)
{
	std::vector<float2> rot((size_t)f.len);
	for (int i = 0; i < f.len; i++) {
		const float ph = f.rotation * (float)i;
		rot[i] = make_float2(cosf(ph), sinf(ph));
	}
	return rot;
}

int mod_dev(hipStream_t st, const gmr1_hip_burst_flat &f, int sync_id, int n, const uint8_t *ebits, float *out)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n < 0 || (n > 0 && (!ebits || !out)))
		return fail(-EINVAL, "mod: ebits / out are required");
	std::vector<int16_t> plan;
	r = mod_plan(f, sync_id, &plan);
	if (r) return fail(r, "mod: unsupported burst description or sync_id %d", sync_id);
	if (n == 0)
		return 0;
	const std::vector<float2> rot = mod_rot(f);
	Stage sg(st);
	int16_t *d_p = sg.dev<int16_t>(plan.size());
	float2 *d_r = sg.dev<float2>(rot.size());
	if ((r = sg.err())) return r;
	HIP_TRY(hipMemcpyAsync(d_p, plan.data(), plan.size() * 2, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(d_r, rot.data(), rot.size() * 8, hipMemcpyHostToDevice, st));
	ModArgs a;
	a.n = n; a.len = f.len; a.nbits = f.nbits; a.n_ebits = f.ebits; a.rotation = f.rotation;
	a.plan = d_p; a.rot = d_r; a.ebits = ebits; a.out = reinterpret_cast<float2 *>(out);
	HIP_TRY(launch_mod(a, st));
	HIP_TRY(hipStreamSynchronize(st));         // the plan buffer is released on return
	return 0;
}

int mod_host(const gmr1_hip_burst_flat &f, int sync_id, int n, const uint8_t *ebits, float *out)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n < 0 || (n > 0 && (!ebits || !out)))
		return fail(-EINVAL, "mod: ebits / out are required");
	if (n == 0)
		return 0;
	Stage sg;
	const uint8_t *d_e = sg.in(ebits, (size_t)n * f.ebits);
	float *d_o = sg.out(out, (size_t)n * f.len * 2);
	if ((r = sg.err())) return r;
	r = mod_dev(nullptr, f, sync_id, n, d_e, d_o);
	if (r) return r;
	return sg.fetch();
}

int builtin_flat(int burst_id, gmr1_hip_burst_flat *f)
{
	if (burst_id < 0 || burst_id >= GMR1_HIP_N_BURSTS)
		return fail(-EINVAL, "mod: burst id %d unknown", burst_id);
	tables_init();
	return flatten(kBuiltin[burst_id], f, kBuiltinName[burst_id]);
}

// ---- shaped modulator (k_shape; tx_pulse.h) -----------------------------------------------------------------------
// the modulator's tables of a built-in format on the current device, every sync sequence's plan: uploaded once and kept,
// so the _dev entries only enqueue
struct ModTab { int n_sync; int16_t *plan; float2 *rot; };
DevCache<int, ModTab> g_mod_tabs;

int mod_tables(int burst_id, const gmr1_hip_burst_flat &f, const ModTab **out)
{
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	return g_mod_tabs.get(dev, burst_id, out, [&f](ModTab *t) {
		std::vector<int16_t> plans, one;
		for (int s = 0; s < f.n_sync; s++) {
			const int r = mod_plan(f, s, &one);
			if (r) return fail(r, "mod_shaped: unsupported burst description");
			plans.insert(plans.end(), one.begin(), one.end());
		}
		t->n_sync = f.n_sync;
		int r = upload(&t->plan, plans);
		if (!r && (r = upload(&t->rot, mod_rot(f))))
			(void)hipFree(t->plan);
		return r;
	});
}

// where the symbols of a shaping call come from: memory (symbols) or a built-in format's burst bits (ebits)
struct ShapeSrc {
	const char *who;
	bool bits;
	int burst_id;                      // bits: the built-in format ...
	gmr1_hip_burst_flat f;             // ... and its description (shape_check fills it in)
	const float *symbols;
	const uint8_t *ebits;
	const int32_t *sync_id;
};

// what both forms refuse without looking at an array; fills in src->f and *len for a built-in format
int shape_check(ShapeSrc *src, int n, int *len, int sps, int pulse, int span, int in_len, const uint64_t *offset, const float *out)
{
	if (src->bits) {
		if (src->burst_id < 0 || src->burst_id >= GMR1_HIP_N_BURSTS)
			return fail(-EINVAL, "%s: burst id %d unknown", src->who, src->burst_id);
		const int r = builtin_flat(src->burst_id, &src->f);
		if (r) return r;
		*len = src->f.len;
	}
	if (shape_args_bad(n, *len, sps, pulse, span, in_len))
		return fail(-EINVAL, "%s: n %d, len %d (1..%d), sps %d (1..%d), pulse %d, span %d (1..%d) or in_len %d is out of range", src->who,
		            n, *len, kShapeMaxLen, sps, kShapeMaxSps, pulse, span, kShapeMaxSpan, in_len);
	if (n > 0 && (!(src->bits ? (const void *)src->ebits : (const void *)src->symbols) || !offset || !out))
		return fail(-EINVAL, "%s: %s, offset and out are required", src->who, src->bits ? "ebits" : "symbols");
	return 0;
}

// every pointer is device memory; the arguments have passed shape_check
int shape_enqueue(hipStream_t st, const ShapeSrc &src, int n, int len, int sps, int pulse, int span, int in_len,
                  const uint64_t *offset, const int32_t *start, const float *frac, const float *cfo, const float *phase0,
                  const float *gain, float *out)
{
	ShapeArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n; a.len = len; a.sps = sps; a.pulse = pulse; a.span = span; a.in_len = in_len;
	if (src.bits) {
		const ModTab *t;
		const int r = mod_tables(src.burst_id, src.f, &t);
		if (r) return r;
		a.nbits = src.f.nbits; a.n_ebits = src.f.ebits; a.n_sync = t->n_sync;
		a.plan = t->plan; a.rot = t->rot; a.ebits = src.ebits; a.sync_id = src.sync_id;
	} else {
		a.symbols = reinterpret_cast<const float2 *>(src.symbols);
	}
	a.offset = offset; a.start = start; a.frac = frac; a.cfo = cfo; a.phase0 = phase0; a.gain = gain;
	a.out = reinterpret_cast<float2 *>(out);
	HIP_TRY(launch_shape(a, st));
	return 0;
}

int shape_dev(hipStream_t st, ShapeSrc src, int n, int len, int sps, int pulse, int span, int in_len,
              const uint64_t *offset, const int32_t *start, const float *frac, const float *cfo, const float *phase0,
              const float *gain, float *out)
{
	int r = shape_check(&src, n, &len, sps, pulse, span, in_len, offset, out);
	if (r) return r;
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0)
		return 0;
	return shape_enqueue(st, src, n, len, sps, pulse, span, in_len, offset, start, frac, cfo, phase0, gain, out);
}

// host pointers.  The arrays are in reach here, so the windows are checked: inside out_len, pairwise disjoint; and every
// sync_id names a sequence of the format.  Only the windows are copied back, so what lies between them in out stays.
int shape_host(ShapeSrc src, int n, int len, int sps, int pulse, int span, int in_len,
               const uint64_t *offset, const int32_t *start, const float *frac, const float *cfo, const float *phase0,
               const float *gain, float *out, uint64_t out_len)
{
	int r = shape_check(&src, n, &len, sps, pulse, span, in_len, offset, out);
	if (r) return r;
	HostWindows win;
	if ((r = win.check(src.who, n, in_len, offset, out_len))) return r;
	for (int b = 0; b < n; b++)
		if (src.bits && src.sync_id && (src.sync_id[b] < 0 || src.sync_id[b] >= src.f.n_sync))
			return fail(-EINVAL, "%s: burst %d asks for sync sequence %d of %d", src.who, b, (int)src.sync_id[b], src.f.n_sync);
	DevState *s;
	if ((r = dev_state(&s))) return r;
	if (n == 0)
		return 0;
	Stage sg;
	const size_t nn = (size_t)n;
	ShapeSrc d = src;
	d.symbols = sg.in(src.symbols, nn * (size_t)len * 2);
	d.ebits = src.bits ? sg.in(src.ebits, nn * (size_t)src.f.ebits) : nullptr;
	d.sync_id = sg.in(src.sync_id, nn);
	const int32_t *d_start = sg.in(start, nn);
	const float *d_frac = sg.in(frac, nn), *d_cfo = sg.in(cfo, nn), *d_ph = sg.in(phase0, nn), *d_gain = sg.in(gain, nn);
	const uint64_t *d_off;
	float *d_out = win.stage(sg, in_len, offset, out, &d_off);
	if ((r = sg.err())) return r;
	r = shape_enqueue(nullptr, d, n, len, sps, pulse, span, in_len, d_off, d_start, d_frac, d_cfo, d_ph, d_gain, d_out);
	if (r) return r;
	return sg.fetch();
}

}  // namespace

extern "C" {

int gmr1_hip_mod_batch_dev(void *stream, int burst_id, int sync_id, int n, const uint8_t *ebits, float *out)
{
	gmr1_hip_burst_flat f;
	int r = builtin_flat(burst_id, &f);
	if (r) return r;
	return mod_dev((hipStream_t)stream, f, sync_id, n, ebits, out);
}
int gmr1_hip_mod_batch(int burst_id, int sync_id, int n, const uint8_t *ebits, float *out)
{
	gmr1_hip_burst_flat f;
	int r = builtin_flat(burst_id, &f);
	if (r) return r;
	return mod_host(f, sync_id, n, ebits, out);
}

int gmr1_hip_shape_batch_dev(void *stream, int n, int len, int sps, int pulse, int span, int in_len,
                             const float *symbols, const uint64_t *offset, const int32_t *start,
                             const float *frac, const float *cfo, const float *phase0, const float *gain,
                             float *out, uint64_t out_len)
{
	(void)out_len;                             // the windows are on the device: the host form checks them against it
	ShapeSrc src = {"shape_batch_dev", false, -1, {}, symbols, nullptr, nullptr};
	return shape_dev((hipStream_t)stream, src, n, len, sps, pulse, span, in_len, offset, start, frac, cfo, phase0, gain, out);
}
int gmr1_hip_shape_batch(int n, int len, int sps, int pulse, int span, int in_len,
                         const float *symbols, const uint64_t *offset, const int32_t *start,
                         const float *frac, const float *cfo, const float *phase0, const float *gain,
                         float *out, uint64_t out_len)
{
	ShapeSrc src = {"shape_batch", false, -1, {}, symbols, nullptr, nullptr};
	return shape_host(src, n, len, sps, pulse, span, in_len, offset, start, frac, cfo, phase0, gain, out, out_len);
}
int gmr1_hip_mod_shaped_batch_dev(void *stream, int burst_id, int n, int sps, int pulse, int span, int in_len,
                                  const uint8_t *ebits, const int32_t *sync_id,
                                  const uint64_t *offset, const int32_t *start,
                                  const float *frac, const float *cfo, const float *phase0, const float *gain,
                                  float *out, uint64_t out_len)
{
	(void)out_len;
	ShapeSrc src = {"mod_shaped_batch_dev", true, burst_id, {}, nullptr, ebits, sync_id};
	return shape_dev((hipStream_t)stream, src, n, 0, sps, pulse, span, in_len, offset, start, frac, cfo, phase0, gain, out);
}
int gmr1_hip_mod_shaped_batch(int burst_id, int n, int sps, int pulse, int span, int in_len,
                              const uint8_t *ebits, const int32_t *sync_id,
                              const uint64_t *offset, const int32_t *start,
                              const float *frac, const float *cfo, const float *phase0, const float *gain,
                              float *out, uint64_t out_len)
{
	ShapeSrc src = {"mod_shaped_batch", true, burst_id, {}, nullptr, ebits, sync_id};
	return shape_host(src, n, 0, sps, pulse, span, in_len, offset, start, frac, cfo, phase0, gain, out, out_len);
}

int gmr1_pi4cxpsk_mod(struct gmr1_pi4cxpsk_burst *burst_type, ubit_t *ebits, int sync_id, struct osmo_cxvec *burst_out)
{
	if (!burst_type || !ebits || !burst_out || !burst_out->data)
		return fail(-EINVAL, "gmr1_pi4cxpsk_mod: NULL argument");
	if (burst_out->max_len < burst_type->len)
		return -ENOMEM;                                            // pi4cxpsk.c:752-756
	tables_init();
	gmr1_hip_burst_flat f;
	int r = flatten(burst_type, &f, "mod");
	if (r) return fail(r, "gmr1_pi4cxpsk_mod: unsupported burst description");
	burst_out->len = burst_type->len;
	return mod_host(f, sync_id, 1, ebits, reinterpret_cast<float *>(burst_out->data));
}

}  // extern "C"
