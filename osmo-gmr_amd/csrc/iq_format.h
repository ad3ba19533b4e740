// iq_format.h -- the sample formats a wideband capture may arrive in (include/gmr1_hip.h: GMR1_HIP_IQ_*) and THE rule that
// turns one stored sample into the float pair every kernel computes on.  Interleaved I, Q of the named type; an integer is
// its value x 2^-15 (S16) or 2^-7 (S8): exact in float32 (a 16-bit integer and a power of two), so -32768 and -128 are
// -1.0 and an integer capture gives bit for bit what its float twin gives.  Host-callable: the kernels of
// chan_kernels.hip read through it, and tests/c/iq_format_host.cpp walks every value of both types through it.
// A sample is loaded as ONE unit of its own size -- 4 bytes for S16, 2 for S8 -- and the pointer needs that alignment only:
// a capture may start one sample into an allocation, and a streamed push of an odd count leaves the next one there.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define GMR1_HD __host__ __device__ inline
#else
#define GMR1_HD inline
#endif

namespace gmr1 {

constexpr int kIqF32 = 0, kIqS16 = 1, kIqS8 = 2;       // = GMR1_HIP_IQ_F32 / _S16 / _S8

// bytes per complex sample; -1: no such format
GMR1_HD int iq_sample_bytes(int fmt) { return fmt == kIqF32 ? 8 : fmt == kIqS16 ? 4 : fmt == kIqS8 ? 2 : -1; }
// what a stored component is multiplied by
GMR1_HD float iq_scale(int fmt) { return fmt == kIqS16 ? 1.0f / 32768.0f : fmt == kIqS8 ? 1.0f / 128.0f : 1.0f; }

struct alignas(4) IqS16 { int16_t i, q; };
struct alignas(2) IqS8 { int8_t i, q; };

// a stored sample as V = a pair of floats {x, y} (float2 on the device) ...
template <typename V> GMR1_HD V iq_value(IqS16 v) { return V{(float)v.i * iq_scale(kIqS16), (float)v.q * iq_scale(kIqS16)}; }
template <typename V> GMR1_HD V iq_value(IqS8 v) { return V{(float)v.i * iq_scale(kIqS8), (float)v.q * iq_scale(kIqS8)}; }
// ... and sample s of the capture at p.  (The two steps are apart for the one reader that keeps its loads in flight:
// what travels is the stored sample, and the conversion sits where the value is first used.)
template <int FMT> struct IqStored;
template <> struct IqStored<kIqS16> { typedef IqS16 type; };
template <> struct IqStored<kIqS8> { typedef IqS8 type; };
template <int FMT>
GMR1_HD typename IqStored<FMT>::type iq_fetch(const void *p, long long s)
{
	return static_cast<const typename IqStored<FMT>::type *>(p)[s];
}
template <int FMT, typename V>
GMR1_HD V iq_load(const void *p, long long s)
{
	static_assert(FMT == kIqF32 || FMT == kIqS16 || FMT == kIqS8, "GMR1_HIP_IQ_*");
	if constexpr (FMT == kIqF32)
		return static_cast<const V *>(p)[s];
	else
		return iq_value<V>(iq_fetch<FMT>(p, s));
}

}  // namespace gmr1
