// carrier_noise.h -- what the carrier mixer (k_carrier_mix, carrier_kernels.hip; gmr1_hip_carrier_mix*) evaluates per
// sample besides its sums, HIP-free: THE noise rule -- Philox4x32-10, words to uniforms, a pair of uniforms to a complex
// Gaussian -- and the carrier phase at an absolute sample index.  Host-callable: the kernel runs this text, and
// tests/c/carrier_noise_host.cpp prints what it gives next to tests/carrier_ref.py, the numpy restatement.
//
// The noise of carrier stream `id` at absolute sample n depends on (seed, id, n) alone: one Philox call per pair of samples,
//   key = (seed low, seed high), counter = (j low, j high, id, 0), j = n >> 1,
// words w0, w1 for sample 2 j and w2, w3 for sample 2 j + 1; with (wa, wb) the sample's two words
//   u1 = ((wa >> 8) + 1) 2^-24 in (0, 1],  u2 = (wb >> 8) 2^-24 in [0, 1),  r = sqrtf(-2 logf(u1)),
//   z = r (cospi(2 u2) + j sinpi(2 u2)):  unit variance per component.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define GMR1_HD __host__ __device__ inline
#else
#define GMR1_HD inline
#endif

namespace gmr1 {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // the multipliers of Philox4x32 ...
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // ... and what the key grows by per round

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are
// in tests/test_carrier_host.py): counter c[4], key k[2] -> w[4]
GMR1_HD void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t w[4])
{
	uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t)p1;
		c3 = (uint32_t)p0;
		c0 = n0;
		c2 = n2;
		k0 += kPhiloxW0;
		k1 += kPhiloxW1;
	}
	w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the four words of the pair of samples 2 j, 2 j + 1 of noise stream `id`
GMR1_HD void noise_words(uint64_t seed, uint32_t id, uint64_t j, uint32_t w[4])
{
	const uint32_t c[4] = {(uint32_t)j, (uint32_t)(j >> 32), id, 0u};
	const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
	philox4x32_10(c, k, w);
}

// words to uniforms: both exact in float (24 bits)
GMR1_HD float noise_u1(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }     // (0, 1]: the logarithm's argument
GMR1_HD float noise_u2(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }            // [0, 1): the angle in turns

// cos and sin of pi x: the device's sincospif; on the host (which has none) through double
GMR1_HD void noise_sincospi(float x, float *s, float *c)
{
#if defined(__HIP_DEVICE_COMPILE__)
	sincospif(x, s, c);
#else
	const double y = 3.141592653589793 * (double)x;
	*s = (float)sin(y);
	*c = (float)cos(y);
#endif
}

// a sample's two words to its complex Gaussian.  V: a pair of floats {x, y}
template <typename V>
GMR1_HD V noise_pair(uint32_t wa, uint32_t wb)
{
	const float r = sqrtf(-2.0f * logf(noise_u1(wa)));
	float s, c;
	noise_sincospi(2.0f * noise_u2(wb), &s, &c);
	return V{r * c, r * s};
}

// the whole rule for one sample (the kernel shares a Philox call between the two samples of a pair)
template <typename V>
GMR1_HD V noise_sample(uint64_t seed, uint32_t id, int64_t n)
{
	uint32_t w[4];
	noise_words(seed, id, (uint64_t)(n >> 1), w);
	return (n & 1) ? noise_pair<V>(w[2], w[3]) : noise_pair<V>(w[0], w[1]);
}

// the carrier phase cfo n at absolute sample n, in [-pi, pi], as a float: the product in double (n reaches 2^23 within
// 90 s at four samples per symbol, so a float phase would be wrong by radians), the turns taken off in double against a
// two-part 2 pi (fused, so the only rounding that grows with n is the product's: 2^-53 |cfo n|), rounded to float once
constexpr double kTwoPiHi = 6.283185307179586, kTwoPiLo = 2.4492935982947064e-16, kInvTwoPi = 0.15915494309189535;

GMR1_HD float carrier_phase(double cfo, int64_t n)
{
	const double th = cfo * (double)n;
	const double turns = rint(th * kInvTwoPi);
	return (float)__builtin_fma(-turns, kTwoPiLo, __builtin_fma(-turns, kTwoPiHi, th));
}

}  // namespace gmr1
