// wave_ops.h -- what one wavefront does across its lanes without LDS traffic (DPP, readlane) and the
// wave-scope fences and LDS flags; shared by every translation unit of the receive side.
#pragma once
#include "gmr1_dev.h"

namespace gmr1 {

#define WSYNC()                                                   \
	do {                                                          \
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");    \
		__builtin_amdgcn_wave_barrier();                          \
	} while (0)

typedef float v2f __attribute__((ext_vector_type(2)));   // (re, im) in a register pair: v_pk_add / v_pk_mul / v_pk_fma_f32

// ---------------------------------------------------------------------------
// cross-lane helpers (DPP: no LDS traffic)
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v)
{
	return __builtin_bit_cast(float, dpp<CTRL>(__builtin_bit_cast(uint32_t, v)));
}

// the partner's value in the steps 1, 2, 4, 8 of a reduction over a 16-lane row.  Callers: row_xor<4> is only valid as
// step 3 of such a reduction by a commutative operation, run in the order 1, 2, 4, 8.  Lane l ^ X for X in {8, 2, 1};
// for X = 4 lane 7 - (l & 7) of the half -- a lane of the half's OTHER quad, whose four lanes all hold that quad's value
// after steps 1 and 2 -- which is one DPP operand instead of the two moves an exact l ^ 4 takes, with the same result
// bit for bit
template <int X>
__device__ __forceinline__ uint32_t row_xor(uint32_t v)
{
	if constexpr (X == 8) return dpp<0x128>(v);                    // row_ror:8
	else if constexpr (X == 4) return dpp<0x141>(v);               // row_half_mirror
	else if constexpr (X == 2) return dpp<0x4E>(v);                // quad_perm [2,3,0,1]
	else return dpp<0xB1>(v);                                      // quad_perm [1,0,3,2]
}
template <int X>
__device__ __forceinline__ float row_xorf(float v)
{
	return __builtin_bit_cast(float, row_xor<X>(__builtin_bit_cast(uint32_t, v)));
}

// every lane gets the sum over its 16-lane row
__device__ __forceinline__ float row_sum(float v)
{
	v += row_xorf<1>(v);
	v += row_xorf<2>(v);
	v += row_xorf<4>(v);
	v += row_xorf<8>(v);
	return v;
}

__device__ __forceinline__ float lane_val(float v, int l)
{
	return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// (r0 + r16) + (r32 + r48) of the four row sums, wave-uniform.  The two cross-row steps are DPP row broadcasts: lane 15 of
// every row into the next row (row 1 then holds r16 + r0, row 3 r48 + r32), then lane 31 into rows 2 and 3 (row 3:
// (r48 + r32) + (r16 + r0)) -- the same three additions, operands swapped, so the same float; one readlane instead of four
// and no moves back from scalar registers.
__device__ __forceinline__ float wave_sum(float v)
{
	v = row_sum(v);
	v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xf, 0xf, true));   // row_bcast:15
	v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xf, 0xf, true));   // row_bcast:31 (rows 0, 1: + 0)
	return lane_val(v, 63);
}

// 64-bit max within each 16-lane row
template <int X>
__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long k)
{
	const uint32_t lo = row_xor<X>((uint32_t)k), hi = row_xor<X>((uint32_t)(k >> 32));
	const unsigned long long o = ((unsigned long long)hi << 32) | lo;
	return o > k ? o : k;
}

// (bounded: a wave that gives up does the work itself -- no hand-shake can hang the work-group)
__device__ __forceinline__ bool lds_wait_eq(const int *flag, int want)
{
	for (int i = 0; i < (1 << 16); i++) {
		if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == want)
			return true;
		__builtin_amdgcn_s_sleep(1);
	}
	return false;
}
__device__ __forceinline__ void lds_post(int *flag, int v)
{
	__hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace gmr1
