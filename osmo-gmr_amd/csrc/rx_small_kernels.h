// rx_small_kernels.h -- the small kernels of rx_kernels.hip with their launchers: burst type detection, modulation
// order, the layer-1 chain alone on soft bits from HBM, interleaved -> polyphase-planar samples.
// (part of rx_kernels.hip's translation unit, included by it inside namespace gmr1, after the k_rx4* kernels)

// ---------------------------------------------------------------------------
// burst type detection (reference src/sdr/pi4cxpsk.c:617-682 gmr1_pi4cxpsk_detect):
// normalise once with the rotation of the first candidate type, run the sync search of
// every candidate, weight the power by 1/|e_toa - toa|, keep the strongest.
// ---------------------------------------------------------------------------
template <int NPL, int SPS>
__global__ __launch_bounds__(64) void k_detect(DetectArgs a, int max_in_len)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int lane = threadIdx.x;
	const Lds L = lds_carve(lds_raw, max_in_len, a.max_lags, false);
	const int g = blockIdx.x;
	const int sps = SPS ? SPS : a.sps;
	load_normalise<NPL>(a.iq + a.offset[g], a.in_len, L, lane);
	const float fsh = a.freq_shift ? a.freq_shift[g] : 0.0f;
	const float fs = (fsh - a.rot0) / (float)sps;
	const float e_toa = a.e_toa ? a.e_toa[g] : -1.0f;
	int p_id = -1, p_sid = -1, rv = 0;
	float p_toa = 0.f, p_pwr = 0.f;
	if (a.carry) {
		// a list of more than four candidates runs as several launches: pick up where the last one stopped
		rv = a.rv[g];
		p_id = a.bt_id[g]; p_sid = a.sync_id[g]; p_toa = a.toa[g]; p_pwr = a.best_pwr[g];
	}
	for (int id = 0; id < a.n_types && rv == 0; id++) {
		float toa, pwr;
		const int sid = sync_search<SPS>(a.types[id], a.in_len, a.sps, fs, L, lane, 0, toa, pwr);
		if (sid < 0) {
			rv = sid;
			break;
		}
		if (e_toa >= 0.0f)
			pwr = (float)((double)pwr / fabs((double)(e_toa - toa)));
		if (pwr > p_pwr) {
			p_id = a.first + id; p_sid = sid; p_pwr = pwr; p_toa = toa;
		}
	}
	if (lane == 0) {
		a.rv[g] = rv;
		if (a.bt_id) a.bt_id[g] = rv ? -1 : p_id;
		if (a.sync_id) a.sync_id[g] = rv ? -1 : p_sid;
		if (a.toa) a.toa[g] = rv ? 0.f : p_toa;
		if (a.best_pwr) a.best_pwr[g] = p_pwr;
	}
}

// ---------------------------------------------------------------------------
// modulation order estimate (reference src/sdr/pi4cxpsk.c:693-729 gmr1_pi4cxpsk_mod_order):
// w = v^2 / |v|^2 on the pi/4-derotated window; BPSK if |sum w|^2 >= |sum w^2|^2 / 2, else QPSK
// ---------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(64) void k_mod_order(ModOrderArgs a, int max_in_len)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int lane = threadIdx.x;
	const Lds L = lds_carve(lds_raw, max_in_len, 0, false);
	const int g = blockIdx.x;
	load_normalise<NPL>(a.iq + a.offset[g], a.in_len, L, lane);
	WSYNC();
	const float fsh = a.freq_shift ? a.freq_shift[g] : 0.0f;
	const float fs = (fsh - (kPif / 4)) / (float)a.sps;
	float sbr = 0.f, sbi = 0.f, sqr = 0.f, sqi = 0.f;
	for (int i = lane; i < a.in_len; i += 64) {
		float2 v = L.x[i];
		if (fs != 0.0f) {
			float s, c;
			sincos_fast(fs * (float)i, s, c);
			v = cmul(v, make_float2(c, s));
		}
		const float nn = v.x * v.x + v.y * v.y;
		const float2 vv = cmul(v, v);
		const float2 w = make_float2(vv.x / nn, vv.y / nn);
		const float2 ww = cmul(w, w);
		sbr += w.x; sbi += w.y;
		sqr += ww.x; sqi += ww.y;
	}
	sbr = wave_sum(sbr); sbi = wave_sum(sbi);
	sqr = wave_sum(sqr); sqi = wave_sum(sqi);
	if (lane == 0) {
		const float pb = sbr * sbr + sbi * sbi;
		const float pq = sqr * sqr + sqi * sqi;
		a.order[g] = pb < (pq / 2.0f) ? 4 : 2;
	}
}

// ---------------------------------------------------------------------------
// The layer-1 chain under libosmocore's accelerated decoder on soft bits from OUTSIDE (they may hold -128, and two of
// those in one trellis step cost 256: one more than a byte lane of the branch-metric word takes).  Same packed-word
// butterfly, same windows, same survivor walk as decode4_k5_12<true>; the four costs of a step are 16-bit lanes of two
// words, formed here from the soft bits themselves.
// ---------------------------------------------------------------------------
template <int PH>
__device__ __forceinline__ uint32_t k5w_step(uint32_t w, const uint16_t *__restrict__ c4, uint32_t oo, uint32_t op)
{
	uint32_t p;
	if constexpr (PH == 0) p = dpp<0x128>(w);                // row_ror:8
	else if constexpr (PH == 1) p = dpp<0x141>(w);           // row_half_mirror: xor 7
	else if constexpr (PH == 2) p = dpp<0x4E>(w);            // quad_perm [2,3,0,1]
	else p = dpp<0xB1>(w);                                   // quad_perm [1,0,3,2]
	const uint32_t t1 = ((uint32_t)c4[oo] << 16) + w;
	const uint32_t t2 = ((uint32_t)c4[op] << 16) + p;
	return t1 < t2 ? t1 : t2;
}

__global__ __launch_bounds__(64) void k_l1_acc(L1Args a)
{
	__shared__ __align__(16) int8_t s_eb[4 * kEbRow];
	__shared__ __align__(16) uint2 s_bmw[4 * kSteps12];        // per step: costs of the coded words 00, 01 | 10, 11
	__shared__ __align__(16) uint64_t s_surv[kSteps12];
	__shared__ __align__(16) uint32_t s_ub[4 * 8];
	const int lane = threadIdx.x;
	const int row = lane >> 4;
	const uint32_t loc = (uint32_t)lane & 15u;
	const int g0 = blockIdx.x * 4;
	const int neb = a.chain == kChainCcch ? 432 : 424;
	const int chain = a.chain == kChainCcch ? 1 : 0;

	for (int q = 0; q < 4; q++) {
		const int g = g0 + q;
		if (g < a.n) {
			const uint32_t *src = reinterpret_cast<const uint32_t *>(a.ebits + (size_t)g * neb);
			uint32_t *dst = reinterpret_cast<uint32_t *>(s_eb + q * kEbRow);
			for (int i = lane; i < neb / 4; i += 64)
				dst[i] = src[i];
		}
	}
	WSYNC();
	for (int it = lane; it < 4 * kSteps12; it += 64) {
		const int q = it / kSteps12, k = it % kSteps12;
		uint2 v = make_uint2(0u, 0u);
		if (g0 + q < a.n) {
			const uint32_t st = c_steps.w[chain][k];
			int va = s_eb[q * kEbRow + (st & 0x3ffu)], vb = s_eb[q * kEbRow + ((st >> 16) & 0x3ffu)];
			if (st & 0x400u) va = (int8_t)(-va);                  // gmr1_scramble_sbit: -128 stays -128
			if (st & 0x4000000u) vb = (int8_t)(-vb);
			const uint32_t a0 = va < 0 ? (uint32_t)(-va) : 0u, a1 = va > 0 ? (uint32_t)va : 0u;
			const uint32_t b0 = vb < 0 ? (uint32_t)(-vb) : 0u, b1 = vb > 0 ? (uint32_t)vb : 0u;
			v = make_uint2((a0 + b0) | ((a0 + b1) << 16), (a1 + b0) | ((a1 + b1) << 16));
		}
		s_bmw[it] = v;
	}
	WSYNC();

	const uint32_t dc = c_dec.v[loc];
	uint32_t oo[4], op[4], T[16];
#pragma unroll
	for (int ph = 0; ph < 4; ph++) {
		oo[ph] = (dc >> (2 * ph)) & 3u;
		op[ph] = (dc >> (8 + 2 * ph)) & 3u;
	}
#pragma unroll
	for (int j = 0; j < 16; j++)
		T[j] = (dc >> 16) & (1u << j);
	const uint16_t *c = reinterpret_cast<const uint16_t *>(s_bmw + row * kSteps12);
	uint16_t *dump = reinterpret_cast<uint16_t *>(s_surv) + lane;
	uint32_t w = (loc ? kAccLeadK5r2 << 16 : 0u) | T[0];
	w = k5w_step<0>(w, c + 0, oo[0], op[0]) + T[1];
	w = k5w_step<1>(w, c + 4, oo[1], op[1]) + T[2];
	w = k5w_step<2>(w, c + 8, oo[2], op[2]) + T[3];
	w = k5w_step<3>(w, c + 12, oo[3], op[3]);
	w = (w & 0xffff0000u) | T[0];
#pragma unroll 1
	for (int m = 0; m < 13; m++) {
		const uint16_t *cm = c + 4 * (4 + 16 * m);
#pragma unroll
		for (int j = 0; j < 16; j += 4) {
			w = k5w_step<0>(w, cm + 4 * (j + 0), oo[0], op[0]) + T[(j + 1) & 15];
			w = k5w_step<1>(w, cm + 4 * (j + 1), oo[1], op[1]) + T[(j + 2) & 15];
			w = k5w_step<2>(w, cm + 4 * (j + 2), oo[2], op[2]) + T[(j + 3) & 15];
			w = k5w_step<3>(w, cm + 4 * (j + 3), oo[3], op[3]) + (j + 4 < 16 ? T[(j + 4) & 15] : 0u);
		}
		dump[m * 64] = (uint16_t)w;
		w = (w & 0xffff0000u) | T[0];
	}
	uint32_t syn;
	k5_12_survivors_crc(s_surv, s_ub, lane, syn);
	const int g = g0 + row;
	if (loc == 0 && g < a.n) {
		store_l2(a.l2 + (size_t)g * 24, s_ub + row * 8);
		a.crc[g] = syn ? 1 : 0;
		a.conv[g] = 0;
	}
}

__global__ __launch_bounds__(64) void k_l1(L1Args a)
{
	__shared__ __align__(16) int8_t s_eb[4 * kEbRow];
	__shared__ __align__(16) uint32_t s_bm[4 * kSteps12];
	__shared__ __align__(16) uint64_t s_surv[kSteps12];
	__shared__ __align__(16) uint32_t s_ub[4 * 8];
	const int lane = threadIdx.x;
	const int g0 = blockIdx.x * 4;
	const int neb = a.chain == kChainCcch ? 432 : 424;
	const int chain = a.chain == kChainCcch ? 1 : 0;

	// soft bits HBM -> LDS, 4 bytes per lane
	for (int q = 0; q < 4; q++) {
		const int g = g0 + q;
		if (g < a.n) {
			const uint32_t *src = reinterpret_cast<const uint32_t *>(a.ebits + (size_t)g * neb);
			uint32_t *dst = reinterpret_cast<uint32_t *>(s_eb + q * kEbRow);
			for (int i = lane; i < neb / 4; i += 64)
				dst[i] = src[i];
		}
	}
	WSYNC();
	for (int q = 0; q < 4; q++) {
		if (g0 + q < a.n) {
			branch_metrics_k5_12(s_eb + q * kEbRow, chain, s_bm + q * kSteps12, lane);
		} else {
			for (int k = lane; k < kSteps12; k += 64)
				s_bm[q * kSteps12 + k] = 0;
		}
	}
	WSYNC();
	uint32_t syn, fae;
	decode4_k5_12(s_bm, s_surv, s_ub, lane, syn, fae);
	const int row = lane >> 4;
	const int g = g0 + row;
	if ((lane & 15) == 0 && g < a.n) {
		store_l2(a.l2 + (size_t)g * 24, s_ub + row * 8);
		a.crc[g] = syn ? 1 : 0;
		a.conv[g] = (int32_t)fae;
	}
}

// Interleaved sample array -> polyphase-planar (what gmr1_hip_rx_bcch_ccch_batch_planar_dev reads): a work-group takes 256 sps
// consecutive samples; thread t of it reads samples t, t + 256, ... (coalesced) and, through LDS, writes place t of each of
// the sps planes (coalesced again).  HBM-bound by construction: every sample read once, written once.
constexpr int kPlanarTile = 256;
__global__ __launch_bounds__(256) void k_to_planar(const float2 *__restrict__ in, float2 *__restrict__ out, unsigned long long n,
                                                   int sps, long long plane_stride)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	float2 *t = reinterpret_cast<float2 *>(lds_raw);
	const unsigned long long p0 = (unsigned long long)blockIdx.x * kPlanarTile;     // first place of the tile in every plane
	const unsigned long long s0 = p0 * (unsigned long long)sps;
	for (int k = 0; k < sps; k++) {
		const unsigned long long s = s0 + (unsigned long long)(k * kPlanarTile + (int)threadIdx.x);
		t[k * kPlanarTile + threadIdx.x] = s < n ? in[s] : make_float2(0.f, 0.f);
	}
	__syncthreads();
	for (int ph = 0; ph < sps; ph++) {
		const unsigned long long s = s0 + (unsigned long long)((int)threadIdx.x * sps + ph);
		if (s < n)
			out[(long long)ph * plane_stride + (long long)(p0 + threadIdx.x)] = t[(int)threadIdx.x * sps + ph];
	}
}

hipError_t launch_to_planar(const float2 *in, float2 *out, unsigned long long n, int sps, long long plane_stride, hipStream_t stream)
{
	if (n == 0)
		return hipSuccess;
	const unsigned long long places = (n + (unsigned long long)sps - 1) / (unsigned long long)sps;
	const unsigned long long grid = (places + kPlanarTile - 1) / kPlanarTile;
	if (grid > 0x7fffffffull)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_to_planar, dim3((unsigned)grid), dim3(256), (size_t)sps * kPlanarTile * 8, stream, in, out, n, sps, plane_stride);
	return hipGetLastError();
}

hipError_t launch_detect(const DetectArgs &a, hipStream_t stream)
{
	if (a.n <= 0)
		return hipSuccess;
	if (a.in_len > kMaxInLen)
		return hipErrorInvalidValue;
	size_t off[3];
	const size_t lds = lds_layout(a.in_len, a.max_lags, false, off);
	if (a.in_len <= 1024) {
		if (a.sps == 4)
			hipLaunchKernelGGL((k_detect<16, 4>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
		else
			hipLaunchKernelGGL((k_detect<16, 0>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	} else if (a.in_len <= 2048) {
		if (a.sps == 4)
			hipLaunchKernelGGL((k_detect<32, 4>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
		else
			hipLaunchKernelGGL((k_detect<32, 0>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	} else {
		hipLaunchKernelGGL((k_detect<64, 0>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	}
	return hipGetLastError();
}

hipError_t launch_mod_order(const ModOrderArgs &a, hipStream_t stream)
{
	if (a.n <= 0)
		return hipSuccess;
	if (a.in_len > kMaxInLen)
		return hipErrorInvalidValue;
	size_t off[3];
	const size_t lds = lds_layout(a.in_len, 0, false, off);
	if (a.in_len <= 1024)
		hipLaunchKernelGGL((k_mod_order<16>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	else if (a.in_len <= 2048)
		hipLaunchKernelGGL((k_mod_order<32>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	else
		hipLaunchKernelGGL((k_mod_order<64>), dim3(a.n), dim3(64), lds, stream, a, a.in_len);
	return hipGetLastError();
}

hipError_t launch_l1(const L1Args &a, hipStream_t stream)
{
	if (a.n <= 0)
		return hipSuccess;
	if (a.conv_acc)
		hipLaunchKernelGGL(k_l1_acc, dim3((a.n + 3) / 4), dim3(64), 0, stream, a);
	else
		hipLaunchKernelGGL(k_l1, dim3((a.n + 3) / 4), dim3(64), 0, stream, a);
	return hipGetLastError();
}
