// tx_pulse.h -- what the shaped modulator (k_shape, tx_kernels.hip; gmr1_hip_shape_batch*, gmr1_hip_mod_shaped_batch*)
// evaluates per burst and per sample, HIP-free: the two pulses and THE rule that says which burst-relative sample a
// window sample is.  Host-callable: the kernel runs this text, and tests/c/tx_pulse_host.cpp prints what it gives
// next to synth.rc_pulse / synth.rrc_pulse / synth.shape_bursts (osmo-gmr_amd/synth.py), the independent statement.
//
// A burst of L symbols s[0..L) (s = 0 elsewhere) shaped with a pulse g cut at +-span symbols has a body of
// (L + 2 span) sps samples; body sample q belongs to burst-relative time q - span sps samples and is
//   body[q] = sum_{m=-span..span} s[i - span - m] g(m + (p - frac) / sps),   i = q div sps, p = q mod sps.
// Symbol 0 of the burst lands on window sample `start`, so window sample k is body sample q = k - (start - span sps);
// outside the body the window is zero.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define GMR1_HD __host__ __device__ inline
#else
#define GMR1_HD inline
#endif

namespace gmr1 {

constexpr int kPulseRc = 0, kPulseRrc = 1;          // = GMR1_HIP_PULSE_RC / _RRC
constexpr int kShapeMaxSps = 16, kShapeMaxSpan = 8, kShapeMaxLen = 2048;
constexpr double kPulseAlpha = 0.35;
constexpr double kPulsePi = 3.141592653589793;

// numpy's sinc: sin(pi x) / (pi x), with x = 0 moved to 1e-20
GMR1_HD double pulse_sinc(double x)
{
	const double y = kPulsePi * (x == 0.0 ? 1.0e-20 : x);
	return sin(y) / y;
}

// raised cosine, t in symbols: synth.rc_pulse, operation for operation
GMR1_HD double rc_pulse(double t)
{
	const double a2t = 2.0 * kPulseAlpha * t;
	const double den = 1.0 - a2t * a2t;
	if (fabs(den) < 1e-9)                              // |t| = 1 / (2 alpha)
		return (kPulsePi / 4) * pulse_sinc(1.0 / (2 * kPulseAlpha));
	return pulse_sinc(t) * cos(kPulsePi * kPulseAlpha * t) / den;
}

// root raised cosine (unit energy per symbol at one sample per symbol): synth.rrc_pulse, operation for operation
GMR1_HD double rrc_pulse(double t)
{
	const double a = kPulseAlpha;
	if (fabs(t) < 1e-9)
		return 1.0 - a + 4.0 * a / kPulsePi;
	if (fabs(fabs(4.0 * a * t) - 1.0) < 1e-9)          // |t| = 1 / (4 alpha)
		return (a / sqrt(2.0)) * ((1 + 2 / kPulsePi) * sin(kPulsePi / (4 * a)) + (1 - 2 / kPulsePi) * cos(kPulsePi / (4 * a)));
	const double a4t = 4.0 * a * t;
	return (sin(kPulsePi * t * (1 - a)) + a4t * cos(kPulsePi * t * (1 + a))) / (kPulsePi * t * (1 - a4t * a4t));
}

// 0: no such pulse
GMR1_HD int pulse_known(int pulse) { return pulse == kPulseRc || pulse == kPulseRrc; }

// coefficient of tap m (-span..span) at sample phase p (0..sps) for a burst delayed by frac samples: evaluated in
// double, rounded to float once
GMR1_HD float pulse_coef(int pulse, int m, int p, double frac, int sps)
{
	const double t = (double)m + ((double)p - frac) / (double)sps;
	return (float)(pulse == kPulseRrc ? rrc_pulse(t) : rc_pulse(t));
}

// the coefficients of a burst, as the kernel keeps them: tap mi = m + span of phase p at [mi * sps + p]
GMR1_HD int pulse_coefs(int span, int sps) { return (2 * span + 1) * sps; }

// q div sps as the high half of one multiplication, the multiplier found once per burst: with M = floor(2^32 / sps) + 1,
// M sps = 2^32 + e, 0 < e <= sps, so floor(q M / 2^32) = floor(q / sps + q e / (sps 2^32)) = q div sps while q sps < 2^32;
// a body has at most (2048 + 16) 16 samples.  sps 1 has no such M in 32 bits and needs none (0).
GMR1_HD uint32_t shape_div_magic(int sps) { return sps > 1 ? (uint32_t)(0x100000000ull / (uint32_t)sps) + 1u : 0u; }

// window sample k of a burst of len symbols whose symbol 0 lands on window sample start (any value: the body is
// clipped at both ends of the window): 0 if k lies outside the body, else 1 and body sample q = i sps + p.
// magic: shape_div_magic(sps)
GMR1_HD int shape_index(int k, int start, int span, int sps, int len, uint32_t magic, int *i, int *p)
{
	const long long q = (long long)k - ((long long)start - (long long)span * sps);
	if (q < 0 || q >= (long long)(len + 2 * span) * sps)
		return 0;
	const uint32_t qi = sps > 1 ? (uint32_t)(((uint64_t)(uint32_t)q * magic) >> 32) : (uint32_t)q;
	*i = (int)qi;
	*p = (int)((uint32_t)q - qi * (uint32_t)sps);
	return 1;
}

// body symbol slot i draws on s[i - span - m]; with the symbols stored behind 2 span zeros (and followed by 2 span more)
// tap mi = m + span reads padded[i + 2 span - mi]: always inside the len + 4 span entries
GMR1_HD int shape_padded_len(int len, int span) { return len + 4 * span; }
GMR1_HD int shape_tap_at(int i, int span, int mi) { return i + 2 * span - mi; }

// one body sample from padded symbols (pairs of floats) and the burst's coefficients: the kernel's inner loop, one fused
// multiply-add per component and tap (said here, not left to a compiler switch: host and device round alike).
// V: a pair of floats {x, y}
template <typename V>
GMR1_HD V shape_body(const V *padded, const float *coef, int i, int p, int span, int sps)
{
	float re = 0.f, im = 0.f;
	for (int mi = 0; mi <= 2 * span; mi++) {
		const V s = padded[shape_tap_at(i, span, mi)];
		const float g = coef[mi * sps + p];
		re = __builtin_fmaf(s.x, g, re);
		im = __builtin_fmaf(s.y, g, im);
	}
	return V{re, im};
}

// ---- the FCCH dual chirp (k_chirp; gmr1_hip_fcch_chirp_batch*): synth.fcch_dual_chirp, operation for operation.
// Sample q = 0 .. len sps of a chirp of len symbols delayed by frac samples: sqrt(2) cos(freq 2 pi / len t^2) at
// t = (q - frac) / sps - len / 2 symbols, evaluated in double and rounded to float once, as the pulse coefficients are.
GMR1_HD float chirp_value(double freq, int len, int sps, long long q, double frac)
{
	const double t = ((double)q - frac) / (double)sps - (double)len / 2.0;
	return (float)(sqrt(2.0) * cos(freq * 2 * kPulsePi / (double)len * t * t));
}

// window sample k of a chirp whose sample 0 lands on window sample start: 0 if k lies outside the chirp, else 1 and q
GMR1_HD int chirp_index(int k, int start, int sps, int len, long long *q)
{
	*q = (long long)k - (long long)start;
	return *q >= 0 && *q < (long long)len * sps;
}

// what the chirp entries refuse (include/gmr1_hip.h): 0 if the arguments are in range
GMR1_HD int chirp_args_bad(int fcch_type, int n, int sps, int in_len)
{
	return fcch_type < 0 || fcch_type > 2 || n < 0 || sps < 1 || sps > kShapeMaxSps || in_len < 1;
}

// the arguments every entry refuses (include/gmr1_hip.h): 0 if they are in range
GMR1_HD int shape_args_bad(int n, int len, int sps, int pulse, int span, int in_len)
{
	return n < 0 || len < 1 || len > kShapeMaxLen || sps < 1 || sps > kShapeMaxSps || span < 1 || span > kShapeMaxSpan ||
	       !pulse_known(pulse) || in_len < 1;
}

}  // namespace gmr1
