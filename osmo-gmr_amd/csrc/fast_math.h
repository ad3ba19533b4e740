// fast_math.h -- single-precision sin / cos / atan2 and complex products as the receive kernels use them.
#pragma once
#include "wave_ops.h"

namespace gmr1 {

static constexpr float kPif = 3.14159265358979323846f;

// ---------------------------------------------------------------------------
// math helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
	return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// sin / cos for |x| up to a few thousand radians: two-constant Cody-Waite reduction
// by pi/2 (exact to ~1e-10 thanks to fma) and the classic single-precision minimax
// polynomials on [-pi/4, pi/4]; ~1 ulp, so results track libm's to the last bit or two.
__device__ __forceinline__ void sincos_fast(float x, float &s, float &c)
{
	const float k = rintf(x * 0.636619772367581343f);
	float r = fmaf(-k, 1.57079637050628662109375f, x);
	r = fmaf(-k, -4.37113900018624283e-8f, r);
	const float z = r * r;
	float sp = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
	sp = fmaf(sp, z, -1.6666654611e-1f);
	sp = fmaf(sp * z, r, r);
	float cp = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
	cp = fmaf(cp, z, 4.166664568298827e-2f);
	cp = fmaf(cp * z, z, fmaf(-0.5f, z, 1.0f));
	const int q = (int)k;
	const float ss = (q & 1) ? cp : sp;
	const float cc = (q & 1) ? sp : cp;
	s = (q & 2) ? -ss : ss;
	c = ((q + 1) & 2) ? -cc : cc;
}

// atan2 with ~1.5e-7 absolute error: octant folding + one reciprocal + degree-9 minimax
__device__ __forceinline__ float atan2_fast(float y, float x)
{
	const float ax = fabsf(x), ay = fabsf(y);
	const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
	const bool big = mn > 0.41421356237f * mx;             // tan(pi/8)
	const float num = big ? (mn - mx) : mn;
	const float den = big ? (mn + mx) : mx;
	const float t = num * __builtin_amdgcn_rcpf(den);
	const float z = t * t;
	float p = fmaf(z, 8.05374449538e-2f, -1.38776856032e-1f);
	p = fmaf(p, z, 1.99777106478e-1f);
	p = fmaf(p, z, -3.33329491539e-1f);
	float a = fmaf(p * z, t, t);
	a += big ? 0.785398163397448309f : 0.0f;
	a = (ay > ax) ? (1.57079632679489662f - a) : a;
	a = (x < 0.0f) ? (kPif - a) : a;
	a = (mx == 0.0f) ? 0.0f : a;
	return (y < 0.0f) ? -a : a;
}

// atan2(y, x) / (2 pi), same minimax polynomial as atan2_fast with the coefficients in turns;
// atan2_turns(0, 0) = 0
__device__ __forceinline__ float atan2_turns(float y, float x)
{
	const float ax = fabsf(x), ay = fabsf(y);
	const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
	const bool big = mn > 0.41421356237f * mx;             // tan(pi/8)
	const float num = big ? (mn - mx) : mn;
	const float den = big ? (mn + mx) : mx;
	const float t = num * __builtin_amdgcn_rcpf(den);
	const float z = t * t;
	float p = fmaf(z, 1.28179325e-2f, -2.20870226e-2f);     // atan2_fast's coefficients / (2 pi)
	p = fmaf(p, z, 3.17955140e-2f);
	p = fmaf(p, z, -5.30510363e-2f);
	p = fmaf(p, z, 1.59154943e-1f);
	float a = p * t;
	a += big ? 0.125f : 0.0f;
	a = (ay > ax) ? (0.25f - a) : a;
	a = (x < 0.0f) ? (0.5f - a) : a;
	a = (mx == 0.0f) ? 0.0f : a;
	return __builtin_copysignf(a, y);
}

// conj(ref) * v for ref = modulating value of sync symbol `sym` (exact: ref is +-1 / +-j)
__device__ __forceinline__ float2 conj_ref_mul(int nbits, int sym, float2 v)
{
	if (nbits == 2) {
		// sym0: ( x, y)  sym1: ( y,-x)  sym2: (-x,-y)  sym3: (-y, x)
		const bool odd = (sym & 1) != 0;
		const float a = odd ? v.y : v.x, b = odd ? v.x : v.y;
		return make_float2((sym & 2) ? -a : a, ((sym + 1) & 2) ? -b : b);
	}
	return (sym & 1) ? make_float2(-v.x, -v.y) : v;
}

// (ar, ai) += c x as two packed FMAs: (-c.im x.im, c.im x.re) first, then c.re (x.re, x.im) -- the order of the scalar
// chains ar = fma(c.re, x.re, fma(-c.im, x.im, ar)), ai = fma(c.re, x.im, fma(c.im, x.re, ai)).  Written out with the
// operand selects and the sign on the ONE pair: the compiler builds (-c.im, c.im) and (c.re, c.re) as pairs of their own,
// four scalar registers a tap, and spills what they displace.  (s_nop: a packed result needs one wait state before its
// next use, which the compiler's own sequences carry as well.)
__device__ __forceinline__ void pk_cmac(v2f &acc, unsigned long long c, v2f x)
{
	asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]\n\ts_nop 0\n\t"
	    "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\ts_nop 0"
	    : "+v"(acc)
	    : "s"(c), "v"(x));
}

}  // namespace gmr1
