// capi_rx_fused.cpp -- the launch set-up of the fused BCCH / CCCH receive (demodulate, then the layer-1 chain on the soft
// bits, in one kernel) that the headline batch entries here, the one-burst calls (capi_one.cpp) and the receive loop
// (capi_rx.cpp) all go through, and the polyphase-planar entries.  What the path asks of the burst tables, its window
// lengths, its staging size and its kernel choice are the rules of rx_select.h.
#include "capi_common.h"
#include "rx_select.h"

namespace gmr1 {

// what every burst of the fused BCCH / CCCH path shares, written into `a` (the caller has zeroed it and set its pointers)
int rx_fused_base_args(int sps, RxArgs *a, int min_sps)
{
	if (sps < min_sps || sps > 16)
		return fail(-EINVAL, "rx_bcch_ccch: sps=%d unsupported (%d..16)", sps, min_sps);
	a->sps = sps;
	a->conv_acc = conv_acc();
	a->in_len[0] = fused_window_len(0, sps);
	a->in_len[1] = fused_window_len(1, sps);
	a->fixed_type = -1;
	a->ebits_stride = 432;
	a->ssyms_stride = 234;
	if (a->in_len[0] > kMaxInLen)
		return fail(-EINVAL, "rx_bcch_ccch: window too long");
	for (int k = 0; k < 2; k++)
		if (!fused_format_matches(g_host_types[kFusedType[k]], k))
			return fail(-EINVAL, "rx_bcch_ccch: burst table %d does not have the training layout the kernel is built for",
			            kFusedType[k]);
	if (!fused_operands_match(g_host_types, g_host_ord4, kHostSteps4))
		return fail(-EINVAL, "rx_bcch_ccch: the packed per-lane operand tables do not say what the burst and step tables say");
	a->stage_samples = fused_stage_samples(g_host_types, sps);
	return 0;
}

int rx_fused_launch(hipStream_t stream, RxArgs a)
{
	if (a.n < 0 || !a.iq || !a.offset || !a.kind || !a.l2 || !a.crc || !a.conv || !a.rv)
		return fail(-EINVAL, "rx_bcch_ccch: iq/offset/kind/l2/crc/conv/rv are required");
	if (a.plane_stride < 0 || (a.plane_stride && (a.sps != 4 || a.energy)))
		return fail(-EINVAL, "rx_bcch_ccch: the polyphase-planar sample layout exists at 4 samples per symbol (sps=%d)", a.sps);
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	r = rx_fused_base_args(a.sps, &a, 1);
	if (r) return r;
	a.dbg_stop = dbg_stop_env();
	static const int env_impl = profile_env_int("GMR1_HIP_RX_IMPL", 0);
	a.impl = fused_impl(a.sps, a.plane_stride, env_impl);
	HIP_TRY(launch_rx(a, true, a.in_len[0], stream));
	return 0;
}

// process_bcch of n_chains chains (launch_rx_loop: k_rx_chain, k_rx4, k_rx_merge); every pointer in `la` is device memory
int rx_loop_dev_impl(hipStream_t stream, int n_chains, int sps, const float *iq, const RxLoopArgs &la)
{
	if (n_chains < 0 || !iq || !la.state || !la.rec || !la.n_rounds || !la.n_rec || !la.n_frames || la.max_rounds < 1 ||
	    la.rec_stride < 1 || (la.rec_frame && !la.rec_minen) || (la.flog && la.flog_stride < 1) || !la.rounds || !la.n_ccch || !la.fin || !la.slice_end ||
	    la.c_stride < 4 || (la.c_stride & 3) || !la.c_off || !la.c_fs || !la.c_kind || !la.c_meta || !la.c_l2 || !la.c_crc ||
	    !la.c_conv || !la.c_rv || !la.c_en)
		return fail(-EINVAL, "rx_loop: bad arguments");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	RxArgs a;
	std::memset(&a, 0, sizeof(a));
	a.iq = reinterpret_cast<const float2 *>(iq);
	r = rx_fused_base_args(sps, &a, 1);
	if (r) return r;
	HIP_TRY(launch_rx_loop(a, la, n_chains, stream));
	return 0;
}

namespace {
// the batch entries' arguments as a launch; plane_stride 0: iq is the interleaved sample array
int rx_bcch_ccch_dev_impl(hipStream_t stream, int n, int sps,
                          const float *iq, const uint64_t *offset, const uint8_t *kind,
                          const float *freq_shift,
                          uint8_t *l2, int32_t *crc, int32_t *conv,
                          float *toa, float *freq_err,
                          int8_t *ebits, float *ssyms, int32_t *rv, long long plane_stride)
{
	RxArgs a;
	std::memset(&a, 0, sizeof(a));
	a.n = n;
	a.sps = sps;
	a.plane_stride = plane_stride;
	a.iq = reinterpret_cast<const float2 *>(iq);
	a.offset = offset; a.kind = kind; a.freq_shift = freq_shift;
	a.l2 = l2; a.crc = crc; a.conv = conv; a.toa = toa; a.freq_err = freq_err;
	a.ebits = ebits; a.ssyms = ssyms; a.rv = rv;
	return rx_fused_launch(stream, a);
}
}  // namespace

}  // namespace gmr1

using namespace gmr1;

extern "C" {

int gmr1_hip_rx_bcch_ccch_batch_dev(void *stream, int n, int sps,
                                    const float *iq, const uint64_t *offset, const uint8_t *kind,
                                    const float *freq_shift,
                                    uint8_t *l2, int32_t *crc, int32_t *conv,
                                    float *toa, float *freq_err,
                                    int8_t *ebits, float *ssyms, int32_t *rv)
{
	return rx_bcch_ccch_dev_impl((hipStream_t)stream, n, sps, iq, offset, kind, freq_shift, l2, crc, conv,
	                             toa, freq_err, ebits, ssyms, rv, 0);
}

int gmr1_hip_rx_bcch_ccch_batch_planar_dev(void *stream, int n, int sps,
                                           const float *iq_planes, uint64_t plane_stride,
                                           const uint64_t *offset, const uint8_t *kind,
                                           const float *freq_shift,
                                           uint8_t *l2, int32_t *crc, int32_t *conv,
                                           float *toa, float *freq_err,
                                           int8_t *ebits, float *ssyms, int32_t *rv)
{
	if (plane_stride == 0 || plane_stride > (uint64_t)1 << 40)
		return fail(-EINVAL, "rx_bcch_ccch planar: plane_stride is required");
	return rx_bcch_ccch_dev_impl((hipStream_t)stream, n, sps, iq_planes, offset, kind, freq_shift, l2, crc, conv,
	                             toa, freq_err, ebits, ssyms, rv, (long long)plane_stride);
}

int gmr1_hip_iq_to_planar_dev(void *stream, int sps, uint64_t n_samples, const float *iq,
                              float *iq_planes, uint64_t plane_stride)
{
	if (sps < 1 || sps > 16 || !iq || !iq_planes || plane_stride < (n_samples + (uint64_t)sps - 1) / (uint64_t)sps)
		return fail(-EINVAL, "iq_to_planar: sps 1..16, both arrays, plane_stride >= ceil(n_samples / sps)");
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	HIP_TRY(launch_to_planar(reinterpret_cast<const float2 *>(iq), reinterpret_cast<float2 *>(iq_planes), n_samples, sps,
	                         (long long)plane_stride, (hipStream_t)stream));
	return 0;
}

int gmr1_hip_rx_bcch_ccch_batch(int n, int sps,
                                const float *iq, uint64_t iq_len, const uint64_t *offset, const uint8_t *kind,
                                const float *freq_shift,
                                uint8_t *l2, int32_t *crc, int32_t *conv,
                                float *toa, float *freq_err,
                                int8_t *ebits, float *ssyms, int32_t *rv)
{
	DevState *s;
	int r = dev_state(&s);
	if (r) return r;
	if (n <= 0) return 0;
	if (!iq || !offset || !kind || !l2 || !crc || !conv || !rv)
		return fail(-EINVAL, "rx_bcch_ccch: iq/offset/kind/l2/crc/conv/rv are required");
	for (int i = 0; i < n; i++) {
		const uint64_t len = (uint64_t)fused_window_len(kind[i], sps);
		if (offset[i] + len > iq_len)
			return fail(-EINVAL, "burst %d runs past the end of iq", i);
	}
	Stage sg;
	const float *d_iq = sg.in(iq, (size_t)iq_len * 2);
	const uint64_t *d_off = sg.in(offset, (size_t)n);
	const uint8_t *d_kind = sg.in(kind, (size_t)n);
	const float *d_fs = sg.in(freq_shift, (size_t)n);
	uint8_t *d_l2 = sg.out(l2, (size_t)n * 24);
	int32_t *d_crc = sg.out(crc, (size_t)n);
	int32_t *d_conv = sg.out(conv, (size_t)n);
	int32_t *d_rv = sg.out(rv, (size_t)n);
	float *d_toa = sg.out_always(toa, (size_t)n);
	float *d_fe = sg.out_always(freq_err, (size_t)n);
	int8_t *d_eb = sg.out(ebits, (size_t)n * 432);
	float *d_ss = sg.out(ssyms, (size_t)n * 234);
	if ((r = sg.err())) return r;
	r = gmr1_hip_rx_bcch_ccch_batch_dev(nullptr, n, sps, d_iq, d_off, d_kind, d_fs, d_l2, d_crc, d_conv, d_toa, d_fe,
	                                    d_eb, d_ss, d_rv);
	if (r) return r;
	return sg.fetch();
}

}  // extern "C"
