// rx_one.h -- one burst per wavefront: sync search, demod_one, and the kernel around them (k_rx).
// (part of rx_kernels.hip's translation unit, included by it inside namespace gmr1, after c_types and rx_window.h)

// sync sequence search over the normalised window in L.x with derotation step fs (rad/sample).
// Returns the winning sequence (-1: none has power), its fractional TOA and power.
template <int SPS>
__device__ int sync_search(int type, int in_len, int sps_rt, float fs, const Lds &L, int lane,
                           int dbg_stop, float &toa_o, float &pwr_o)
{
	const DevBurst &bt = c_types[type];
	const int sps = SPS ? SPS : sps_rt;
	const int nbits = bt.nbits;
	const int w = in_len - bt.len * sps + 1;
	WSYNC();
	for (int j = lane; j < w; j += 64)
		L.corr[j] = 0.f;

	// ---- sync search (pi4cxpsk.c:184-268) --------------------------------------
	float p_toa = 0.f, p_pwr = 0.f;
	int p_idx = -1;
	const int win = w < 3 ? w : 3;
	const int nsync = bt.n_sync;

	for (int sq = 0; sq < nsync; sq++) {
		const int tl = bt.sync_tl[sq];
		const int nch = bt.n_chunks[sq];

		// rotated reference: conj(ref_n) * e^{j fs sps n}; the common phase of a lag
		// drops out under |.|, so the window itself is never derotated here
		WSYNC();
		for (int n = lane; n < tl; n += 64) {
			int ch = 0, base = 0, cum = 0;
			for (int c = 0; c < nch - 1; c++) {
				cum += bt.sync[sq][c].len;
				if (n >= cum) { base = cum; ch = c + 1; }
			}
			const int nn = n - base;
			const int sym = bt.sync[sq][ch].syms[nn];
			float s, c;
			sincos_fast(fs * (float)(nn * sps), s, c);
			L.coef[n] = conj_ref_mul(nbits, sym, make_float2(c, s));
		}
		WSYNC();

		for (int j = lane; j < w; j += 64) {
			float cj = L.corr[j];
			int base = 0;
			for (int ch = 0; ch < nch; ch++) {
				const int pos = bt.sync[sq][ch].pos, len = bt.sync[sq][ch].len;
				const float2 *xp = L.x + pos * sps + j;
				const float2 *cp = L.coef + base;
				float ar = 0.f, ai = 0.f;
				for (int n = 0; n < len; n++) {
					const float2 x = xp[n * sps];
					const float2 cf = cp[n];
					ar = fmaf(cf.x, x.x, fmaf(-cf.y, x.y, ar));
					ai = fmaf(cf.x, x.y, fmaf(cf.y, x.x, ai));
				}
				base += len;
				cj += sqrtf(fmaf(ar, ar, ai * ai));
			}
			L.corr[j] = cj;
		}
		WSYNC();
		if (dbg_stop == 2) return -100;

		// ---- osmo_cxvec_peak_energy_find(corr, 3, PEAK_EARLY_LATE, &peak) ----------
		// key = (energy bits << 32) | ~index : max key = highest energy, lowest index on ties
		unsigned long long key = 0;
		for (int m = lane; m + win <= w; m += 64) {
			float e = 0.f;
			for (int k = 0; k < win; k++) {
				const float c = L.corr[m + k];
				e += c * c;
			}
			const unsigned long long kk =
				((unsigned long long)__builtin_bit_cast(uint32_t, e) << 32) | (uint32_t)(~m);
			key = kk > key ? kk : key;
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			const unsigned long long ok = __shfl_xor(key, o);
			key = ok > key ? ok : key;
		}
		int mi = (int)(~(uint32_t)key);
		if (mi < 0 || mi + win > w)
			mi = 0;
		int p = mi;
		{
			float pe = -1.f;
			for (int k = 0; k < win; k++) {
				const float c = L.corr[mi + k];
				const float e = c * c;
				if (e > pe) { pe = e; p = mi + k; }
			}
		}

		// sinc-interpolated corr at `pos` (libosmo-dsp interpolate_point, 21 taps):
		// lanes t = 0..20 of each 32-lane half hold one tap of that half's position.
		// tap weight sinc(pi (i - pos)) with i - pos = k - f  ->  -(-1)^k sin(pi f) / (pi (k - f))
		const int t = lane & 31;
		auto interp_term = [&](float pos) -> float {
			const float fl = floorf(pos);
			const int i0 = (int)fl;
			const float f = pos - fl;
			int b = i0 - 10, e = i0 + 11;
			if (b < 0) b = 0;
			if (e >= w) e = w - 1;
			const int i = i0 - 10 + t;
			const bool valid = t < 21 && i >= b && i < e;
			const float xx = kPif * ((float)i - pos);
			const float S = __builtin_amdgcn_sinf(0.5f * f);       // sin(pi f), argument in turns
			const float sg = (t & 1) ? S : -S;                     // k = t - 10 has the parity of t
			const float wgt = (xx >= 0.01f || xx <= -0.01f) ? sg * __builtin_amdgcn_rcpf(xx) : 1.0f;
			const float c = L.corr[valid ? i : 0];
			return valid ? c * wgt : 0.0f;
		};
		auto half_total = [&](float v, int half) -> float {
			v = row_sum(v);
			return lane_val(v, 32 * half) + lane_val(v, 32 * half + 16);
		};

		// Early / late bisection (incr = 1/2 ... 1/512), THREE levels per evaluation: each group of 8 lanes
		// interpolates the correlation at one candidate position and two samples later (same fractional part,
		// so the same 21 weights; lane sub holds taps k = 3 sub - 10 + {0,1,2}) -- group 0 at the current point,
		// groups 1 / 2 where the search goes if the early / late side wins, groups 3..6 one level further down.
		// The candidates are formed by the same float operations the level-by-level walk performs, so it takes
		// the same decisions; the walk itself is scalar work on two ballots.
		const int grp = lane >> 3, isub = lane & 7;
		auto interp_pair = [&](float pos, float &se, float &sl) {
			const float fl = floorf(pos);
			const int ib = (int)fl;
			const float f = pos - fl;
			const float S = __builtin_amdgcn_sinf(0.5f * f);       // sin(pi f); sin(pi (k - f)) = -(-1)^k sin(pi f)
			int be = ib - 10, ee = ib + 11, bl = ib - 8, el = ib + 13;
			if (be < 0) be = 0;
			if (bl < 0) bl = 0;
			if (ee >= w) ee = w - 1;
			if (el >= w) el = w - 1;
			float ae = 0.f, al = 0.f;
#pragma unroll
			for (int tt = 0; tt < 3; tt++) {
				const int k = 3 * isub - 10 + tt;
				const float sg = ((isub + tt) & 1) ? S : -S;
				const float xx = kPif * ((float)k - f);
				const float wgt = (xx >= 0.01f || xx <= -0.01f) ? sg * __builtin_amdgcn_rcpf(xx) : 1.0f;
				const int ie = ib + k, il = ib + 2 + k;
				const bool ve = k <= 10 && ie >= be && ie < ee;
				const bool vl = k <= 10 && il >= bl && il < el;
				const float ce = L.corr[ve ? ie : 0], cl = L.corr[vl ? il : 0];
				ae += ve ? ce * wgt : 0.0f;
				al += vl ? cl * wgt : 0.0f;
			}
			ae += row_xorf<1>(ae);
			ae += row_xorf<2>(ae);
			ae += row_xorf<4>(ae);
			al += row_xorf<1>(al);
			al += row_xorf<2>(al);
			al += row_xorf<4>(al);
			se = ae;
			sl = al;
		};
		float early = (float)p - 1.0f, incr = 0.5f;
#pragma unroll 1
		for (int it = 0; it < 3; it++) {
			const float half = incr * 0.5f, quarter = incr * 0.25f;
			float pos = early;
			if (grp == 1) {
				pos = early - incr;
			} else if (grp == 2) {
				pos = early + incr;
			} else if (grp >= 3 && grp <= 6) {
				const float a1 = grp < 5 ? early - incr : early + incr;
				pos = (grp & 1) ? a1 - half : a1 + half;           // 3: - -, 4: - +, 5: + -, 6: + +
			}
			float se, sl;
			interp_pair(pos, se, sl);
			const float ee = se * se, le = sl * sl;
			const unsigned long long m_neg = __ballot(ee > le), m_pos = __ballot(ee < le);
			auto dec = [&](int g) -> int { return ((m_neg >> (8 * g)) & 1ull) ? -1 : (((m_pos >> (8 * g)) & 1ull) ? 1 : 0); };
			const int d0 = dec(0);
			if (d0 == 0) break;
			early = d0 < 0 ? early - incr : early + incr;
			const int d1 = dec(d0 < 0 ? 1 : 2);
			if (d1 == 0) break;
			early = d1 < 0 ? early - half : early + half;
			const int d2 = dec(3 + (d0 > 0 ? 2 : 0) + (d1 > 0 ? 1 : 0));
			if (d2 == 0) break;
			early = d2 < 0 ? early - quarter : early + quarter;
			incr *= 0.125f;
		}
		const float s_toa = early + 1.0f;
		float pk = half_total(interp_term(s_toa), 0);
		pk = pk * __builtin_amdgcn_rcpf((float)tl);     // only ranked and tested against 0
		const float s_pwr = pk * pk;
		if (s_pwr > p_pwr) {
			p_pwr = s_pwr;
			p_toa = s_toa;
			p_idx = sq;
		}
	}
	toa_o = p_toa;
	pwr_o = p_pwr;
	return p_idx;
}

// One sample of the burst behind the reference's 21-tap fractional delay (pi4cxpsk.c:310-327), less the common rotation
// e^{j fl(fs j)}, which the callers add in the phase domain.  L.coef holds the taps with the rotation between neighbours in
// them, p_k e^{j fs (10 - k)} (see demod_one).  The reference de-rotates sample m by the fp32 PRODUCT fs * m before it delays
// (osmo_cxvec_sig_normalize), and hundreds of radians into a burst that product is rounded by up to 3e-5 rad, for each of the
// 21 samples under the pulse in its own way.  In a sample tens of times weaker than its neighbours that is more than 1e-4 of
// a soft-symbol step, so the roundings taken here are the reference's: eps = (fl(fs m) - fl(fs j)) - fs (m - j), a few 1e-5
// at most, enters as the factor 1 + j eps.
__device__ __forceinline__ float2 delayed_sample(const Lds &L, float fs, int j, int in_len)
{
	const float pj = fs * (float)j;
	float2 acc = make_float2(0.f, 0.f);
	for (int k = 0; k < 21; k++) {
		const int m = j + 10 - k;
		if (m >= 0 && m < in_len) {
			const float2 q = L.coef[k], x = L.x[m];
			const float eps = fmaf(-fs, (float)(10 - k), fs * (float)m - pj);
			const float tr = fmaf(q.x, x.x, -q.y * x.y), ti = fmaf(q.x, x.y, q.y * x.x);
			acc.x += fmaf(-eps, ti, tr);
			acc.y += fmaf(eps, tr, ti);
		}
	}
	return acc;
}

// ---------------------------------------------------------------------------
// demodulation of one burst by one wavefront
// returns the reference's rv (0, or -1 when no sync sequence has power)
// ---------------------------------------------------------------------------
template <int NPL, int SPS>
__device__ int demod_one(int type, const float2 *__restrict__ in, int in_len, int sps_rt,
                         float freq_shift, const Lds &L, int8_t *__restrict__ eb, int lane,
                         int dbg_stop, int &sync_id_o, float &toa_o, float &ferr_o,
                         float *__restrict__ g_ssyms)
{
	const DevBurst &bt = c_types[type];
	const int sps = SPS ? SPS : sps_rt;
	const int nbits = bt.nbits;
	const int blen = bt.len;

	float avr, avi, inv_sd;
	load_normalise_stats<NPL>(in, in_len, L, lane, avr, avi, inv_sd);
	if (dbg_stop == 1) return -100;

	// per-sample derotation step (pi4cxpsk.c:539)
	const float fs = (freq_shift - bt.rotation) / (float)sps;
	float p_toa = 0.f, p_pwr = 0.f;
	const int p_idx = sync_search<SPS>(type, in_len, sps_rt, fs, L, lane, dbg_stop, p_toa, p_pwr);
	if (p_idx == -100 || dbg_stop == 3) return -100;

	sync_id_o = p_idx;
	toa_o = p_toa;
	if (p_idx < 0) {
		ferr_o = 0.f;
		return -1;
	}
	const int sq = p_idx;
	const int nch = bt.n_chunks[sq];

	// ---- everything after the sync search works in the PHASE domain ----------------
	// The reference rotates the decimated burst three times (derotation e^{j fs n},
	// fine frequency e^{-j f i}, carrier conj(phasor)) and then takes cargf() of each
	// symbol (pi4cxpsk.c:286-297,574-581,442-460).  arg() of that product is
	//     arg(x[i sps + d]) + fs (i sps + d) - f i - arg(phasor)      (mod 2 pi)
	// so only the <= 17 sync symbols are ever rotated as complex numbers; the 234
	// symbols cost one atan2 and a few adds each.  Soft bits only depend on the phase.
	const int d = (int)roundf(p_toa);
	const int row = lane >> 4, col = lane & 15;

	// align (pi4cxpsk.c:280-348): at sps >= 4 symbol i is sample i*sps + d.  Below 4 samples per
	// symbol the reference first applies a 21-tap sinc fractional delay (osmo_cxvec_convolve,
	// CONV_NO_DELAY) when |toa - d| > 0.1.  It does so on the DEROTATED burst; with
	// g[m] = x[m] e^{j fs m} the delayed sample is e^{j fs n} sum_k (p_k e^{j fs (10-k)}) x[n+10-k], so the
	// rotation moves into 21 complex taps and the common e^{j fs n} stays in the phase domain (delayed_sample, which also
	// takes over how the reference rounds fs m).
	const float ofs_frac = p_toa - (float)d;
	const bool frac_on = (sps < 4) && (fabsf(ofs_frac) > 0.1f);
	if (frac_on) {
		WSYNC();
		if (lane < 21) {
			const float xx = kPif * ((float)(lane - 10) + ofs_frac);
			const float pv = (xx >= 0.01f || xx <= -0.01f) ? (sinf(xx) / xx) : 1.0f;
			float s, c;
			sincos_fast(fs * (float)(10 - lane), s, c);
			L.coef[lane] = make_float2(pv * c, pv * s);
		}
		WSYNC();
	}
	auto pick = [&](int j) -> float2 {
		if (j < 0 || j >= in_len)
			return make_float2(0.f, 0.f);
		if (!frac_on)
			return L.x[j];
		return delayed_sample(L, fs, j, in_len);
	};

	auto reduce_2pi = [](float a) -> float {
		const float k = rintf(a * 0.159154943091895336f);
		a = fmaf(-k, 6.2831854820251465f, a);
		return fmaf(-k, -1.7484555e-7f, a);
	};
	// conj(ref) * derotated sample of sync symbol j of chunk c (pi4cxpsk.c:386-388)
	auto sync_term = [&](int c, int j) -> float2 {
		const int idx = (bt.sync[sq][c].pos + j) * sps + d;
		float2 x = pick(idx);
		float s, cc;
		sincos_fast(fs * (float)idx, s, cc);
		x = cmul(x, make_float2(cc, s));
		return conj_ref_mul(nbits, bt.sync[sq][c].syms[j], x);
	};

	// ---- fine frequency error from the sync chunks (pi4cxpsk.c:360-406) ---------
	// one chunk per 16-lane row, one sync symbol per lane; chunk sums by DPP
	float ffe = 0.f;
	if (nch > 1) {
		float sumr[kMaxChunks], sumi[kMaxChunks];
#pragma unroll
		for (int c0 = 0; c0 < kMaxChunks; c0 += 4) {
			if (c0 < nch) {
				const int c = c0 + row;
				float tr = 0.f, ti = 0.f;
				if (c < nch) {
					const int len = bt.sync[sq][c].len;
					for (int j = col; j < len; j += 16) {
						const float2 tt = sync_term(c, j);
						tr += tt.x;
						ti += tt.y;
					}
				}
				tr = row_sum(tr);
				ti = row_sum(ti);
#pragma unroll
				for (int r = 0; r < 4; r++) {
					sumr[c0 + r] = lane_val(tr, 16 * r);
					sumi[c0 + r] = lane_val(ti, 16 * r);
				}
			}
		}
		float f = 0.f;
#pragma unroll
		for (int i = 1; i < kMaxChunks; i++) {
			if (i < nch) {
				const float ppos = (float)bt.sync[sq][i - 1].pos + (float)bt.sync[sq][i - 1].len / 2.0f;
				const float cpos = (float)bt.sync[sq][i].pos + (float)bt.sync[sq][i].len / 2.0f;
				// corr[i] * conj(corr[i-1])
				const float re = sumr[i] * sumr[i - 1] - sumi[i] * (-sumi[i - 1]);
				const float im = sumr[i] * (-sumi[i - 1]) + sumi[i] * sumr[i - 1];
				f += atan2_fast(im, re) / (cpos - ppos);
			}
		}
		f /= (float)(nch - 1);
		ffe = f;
	}
	ferr_o = ffe;
	const float rps = -ffe;            // pi4cxpsk.c:574-575
	if (dbg_stop == 4) return -100;

	// ---- carrier phase from the (frequency-corrected) sync symbols (pi4cxpsk.c:415-433)
	float tr = 0.f, ti = 0.f;
#pragma unroll
	for (int c0 = 0; c0 < kMaxChunks; c0 += 4) {
		if (c0 < nch) {
			const int c = c0 + row;
			if (c < nch) {
				const int pos = bt.sync[sq][c].pos, len = bt.sync[sq][c].len;
				for (int j = col; j < len; j += 16) {
					float2 tt = sync_term(c, j);
					if (ffe != 0.0f) {
						float s, cc;
						sincos_fast(rps * (float)(pos + j), s, cc);
						tt = cmul(tt, make_float2(cc, s));
					}
					tr += tt.x;
					ti += tt.y;
				}
			}
		}
	}
	const float phr = wave_sum(tr), phi = wave_sum(ti);
	const float psi = atan2_fast(phi, phr);      // arg(phasor); |phasor| never matters
	if (dbg_stop == 5) return -100;

	// ---- soft symbols + soft bits (pi4cxpsk.c:442-503) ------------------------------
	// one symbol per lane and piece, pieces for the longest format whatever the window: a burst of more than 256 symbols fits a
	// window of 1024 samples or fewer at 1 and 2 samples per symbol (NT9 and RACH, 351 symbols, DC12, 468); a piece beyond the
	// burst's length costs its test
	constexpr int NSYM = (kMaxLen + 63) / 64;
	static_assert(NSYM * 64 >= kMaxLen, "the soft-symbol loop covers every format's length");
	const float inv_dd = (float)(1 << nbits) / (2.0f * kPif);
	const int mask = (1 << nbits) - 1;
	// the soft symbols that go out are formed about the reference's mean (window_mean_serial): what a normalised sample
	// moves by.  (Not behind the fractional delay, which has mixed the window's samples.)
	const bool ref_mean = g_ssyms != nullptr && !frac_on;
	float2 dm = make_float2(0.f, 0.f);
	if (ref_mean) {
		const float2 m = window_mean_serial(in, in_len);
		dm = make_float2((avr - m.x) * inv_sd, (avi - m.y) * inv_sd);
	}
	auto soft_symbol = [&](float2 x, int i, int j) -> float {
		float th = atan2_fast(x.y, x.x) + reduce_2pi(fs * (float)j);
		th = reduce_2pi(fmaf(rps, (float)i, th) - psi);
		return (x.x == 0.0f && x.y == 0.0f) ? 0.0f : th * inv_dd;   // cargf(0) = 0
	};
#pragma unroll
	for (int r = 0; r < NSYM; r++) {
		if (64 * r >= blen)
			break;                                   // (wave-uniform: the pieces beyond the burst are jumped over)
		const int i = lane + 64 * r;
		if (i >= blen)
			continue;
		const int j = i * sps + d;
		const float2 x = pick(j);
		const float sv = soft_symbol(x, i, j);
		if (g_ssyms)
			g_ssyms[i] = (ref_mean && j >= 0 && j < in_len) ? soft_symbol(make_float2(x.x + dm.x, x.y + dm.y), i, j) : sv;
		const int ord = bt.ord_of_sym[i];
		if (ord >= 0) {
			const float svr2 = roundf(sv);
			const int sp = (int)svr2 & mask;
			const int ss = (svr2 > sv ? (sp - 1) : (sp + 1)) & mask;
			const int dq = (int)roundf((2.0f * fabsf(svr2 - sv)) * 64.0f);
			if (nbits == 2) {
				// symbol -> bits 0:00 1:01 2:11 3:10 (pi4cxpsk.c:95-100)
				const int p0 = sp >> 1, p1 = (sp ^ (sp >> 1)) & 1;
				const int s0 = ss >> 1, s1 = (ss ^ (ss >> 1)) & 1;
				const int v0 = 127 - ((p0 ^ s0) ? dq : (dq >> 1));
				const int v1 = 127 - ((p1 ^ s1) ? dq : (dq >> 1));
				const uint32_t pk2 = (uint32_t)(uint8_t)(int8_t)(p0 ? -v0 : v0) |
				                     ((uint32_t)(uint8_t)(int8_t)(p1 ? -v1 : v1) << 8);
				*reinterpret_cast<uint16_t *>(eb + 2 * ord) = (uint16_t)pk2;
			} else {
				const int p0 = sp & 1, s0 = ss & 1;
				const int v0 = 127 - ((p0 ^ s0) ? dq : (dq >> 1));
				eb[ord] = (int8_t)(p0 ? -v0 : v0);
			}
		}
	}
	WSYNC();
	return 0;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
template <int NPL, int SPS, bool DECODE, bool ACC = false>
__global__ __launch_bounds__(64) void k_rx(RxArgs a, int max_in_len, int max_len)
{
	extern __shared__ __align__(16) unsigned char lds_raw[];
	const int lane = threadIdx.x;
	const Lds L = lds_carve(lds_raw, max_in_len, max_len, DECODE);

	constexpr int PER = DECODE ? 4 : 1;
	int g0 = blockIdx.x * PER;
	int n_end = a.n;
	if (DECODE && a.seg_count) {
		// the receive loop's CCCH lists (see k_rx4): segments with unused slots, one time slice of each per launch
		int sg = g0 / a.seg_stride;
		int lo = 0;
		if (a.seg_first) {
			if (a.seg_groups > 0) {
				sg = (int)blockIdx.x / a.seg_groups;
				lo = (a.seg_first[sg] + 3) & ~3;
				g0 = sg * a.seg_stride + lo + ((int)blockIdx.x % a.seg_groups) * PER;
			} else {
				lo = (a.seg_first[sg] + 3) & ~3;
			}
		}
		const int base = sg * a.seg_stride;
		n_end = min(min(a.n, g0 + PER), base + min(a.seg_count[sg], a.seg_stride));
		if (g0 >= n_end || g0 < base + lo)
			return;
	}
	int row_ok = 0;       // bit q: burst q of this wave demodulated fine
	int row_chain = 0;    // bit q: burst q is CCCH

	for (int q = 0; q < PER; q++) {
		const int g = g0 + q;
		if (g >= n_end)
			break;
		int type, in_len;
		if (DECODE) {
			const int kind = a.kind[g] ? 1 : 0;
			type = kind ? GMR1_HIP_DC6 : GMR1_HIP_BCCH;
			in_len = a.in_len[kind];
			row_chain |= kind << q;
		} else {
			type = a.fixed_type;
			in_len = a.in_len[0];
		}
		type = __builtin_amdgcn_readfirstlane(type);
		in_len = __builtin_amdgcn_readfirstlane(in_len);
		const float fsh = a.freq_shift ? a.freq_shift[g] : 0.0f;
		int sid = -1;
		float toa = 0.f, fe = 0.f;
		float *gss = a.ssyms ? a.ssyms + (size_t)g * a.ssyms_stride : nullptr;
		int8_t *eb = L.eb + (DECODE ? q * kEbRow : 0);

		WSYNC();
		const int rv = demod_one<NPL, SPS>(type, a.iq + a.offset[g], in_len, a.sps, fsh, L, eb, lane,
		                                   a.dbg_stop, sid, toa, fe, gss);
		if (rv == -100)
			continue;    // profiling build-out: phase cut-off
		if (a.energy) {
			const float e = window_energy<NPL>(a.iq + a.offset[g], in_len, lane);
			if (lane == 0)
				a.energy[g] = e;
		}

		if (lane == 0) {
			a.rv[g] = rv;
			if (a.sync_id) a.sync_id[g] = sid;
			if (a.toa) a.toa[g] = rv ? 0.f : toa;
			if (a.freq_err) a.freq_err[g] = rv ? 0.f : fe;
		}
		if (a.ebits) {
			const int neb = c_types[type].ebits;
			int8_t *ge = a.ebits + (size_t)g * a.ebits_stride;
			// (demodulation only: what lies behind a row's soft bits is the caller's; the fused rows of 432 are zero there)
			for (int i = lane; i < (DECODE ? a.ebits_stride : neb); i += 64)
				ge[i] = (rv == 0 && i < neb) ? eb[i] : (int8_t)0;
		}
		if (rv && gss)
			for (int i = lane; i < c_types[type].len; i += 64)
				gss[i] = 0.f;
		if (rv == 0)
			row_ok |= 1 << q;
	}

	if (DECODE) {
		if (a.dbg_stop && a.dbg_stop < 7)
			return;
		WSYNC();     // x is dead from here on: bm / surv / ubits overlay it
		for (int q = 0; q < 4; q++) {
			if ((row_ok >> q) & 1) {
				branch_metrics_k5_12<ACC>(L.eb + q * kEbRow, (row_chain >> q) & 1, L.bm + q * kSteps12, lane);
			} else {
				for (int k = lane; k < kSteps12; k += 64)
					L.bm[q * kSteps12 + k] = 0;
			}
		}
		WSYNC();
		if (a.dbg_stop == 7)
			return;
		uint32_t syn, fae;
		decode4_k5_12<ACC>(L.bm, L.surv, L.ubits, lane, syn, fae);
		const int row = lane >> 4;
		const int g = g0 + row;
		if ((lane & 15) == 0 && g < n_end) {
			if ((row_ok >> row) & 1) {
				store_l2(a.l2 + (size_t)g * 24, L.ubits + row * 8);
				a.crc[g] = syn ? 1 : 0;
				a.conv[g] = (int32_t)fae;
			} else {
				uint32_t *l2w = reinterpret_cast<uint32_t *>(a.l2 + (size_t)g * 24);
#pragma unroll
				for (int i = 0; i < 6; i++)
					l2w[i] = 0;
				a.crc[g] = -1;
				a.conv[g] = 0;
			}
		}
	}
}
