// carrier_kernels.hip -- the carrier mixer for gfx950 (gmr1_hip_carrier_mix*; past where the reference ends: it has no
// transmitter).  Windows the library already makes (k_shape, k_chirp: bursts and FCCH chirps) become carriers: continuous
// streams with the windows overlap-added at absolute sample positions, rotated by a carrier offset, over a noise floor.
//
// k_carrier_mix is a GATHER: a work-group owns a tile of kMixTile consecutive samples of one carrier and every sample is
// written exactly once, by the lane that summed it -- no atomics, no scratch, and the summation order of a sample is the
// carrier's list order whatever the launch looks like, so the result is reproducible bit for bit.  (A scatter of segments
// would need float atomics and would sum in arrival order.)
//   1. The tile's candidate segments: the carrier's segments are sorted by pos, so the first one that can reach the tile is
//      the first with pos > tile_start - max_seg_len (binary search), and the walk ends at the first with pos >= tile_end.
//      Carrier, tile and therefore every descriptor are uniform over the work-group: the search and the walk run on the
//      scalar unit (s_load of seg_pos / seg_len / seg_src), and the lanes only do the sums.
//   2. A lane owns kMixUnits 16-byte units of the output, two samples each (the unit grid is that of the ADDRESS, as in
//      k_shape: a carrier that starts on an odd sample of `out` has a single sample at either end).  A segment is read 16
//      bytes at a time where both samples lie in it and the source address is a unit's too, else 8.
//   3. cfo != 0 (per carrier, hence uniform): the phase of absolute sample n through carrier_phase (carrier_noise.h:
//      fp64 product and reduction) and the accurate sincosf.  fp64 is spent nowhere else.
//   4. sigma != 0 (uniform): one Philox4x32-10 call gives the noise of samples 2 j and 2 j + 1.  A unit whose lower sample
//      has an even absolute index is exactly one call; with an odd one (a carrier that starts on an odd absolute index or
//      an odd address: uniform again) it straddles two pairs and takes the upper half of one and the lower half of the next.
//   5. Streaming stores: nothing here is read again by this kernel.
// Carriers of different lengths: the carrier on grid.y, max_length sizing grid.x; a tile past its carrier's end returns.
//
// Bound: Philox / transcendental issue, not the 8 bytes per sample stored -- with noise alone the kernel takes twice a plain
// fill of the same bytes, what torch's own generator takes; segments and the fp64 phase add a third each (64 carriers x
// 60 s: 1.43 ms against the fill's 0.42 ms; DESIGN.md section 4.8c has the table).
#include <hip/hip_runtime.h>

#include "carrier_noise.h"
#include "gmr1_dev.h"

namespace gmr1 {

typedef float mx_v4f __attribute__((ext_vector_type(4)));
typedef float mx_v2f __attribute__((ext_vector_type(2)));

// a value every lane reads from one address that nothing writes while the kernel runs (the carriers' and the segments'
// descriptors): through the constant address space, so that the load is the scalar unit's
template <typename T>
__device__ __forceinline__ T uload(const T *p)
{
	return *(const __attribute__((address_space(4))) T *)p;
}

constexpr int kMixThreads = 256, kMixUnits = 2;
constexpr int kMixTile = kMixThreads * kMixUnits * 2;        // samples of a tile (= GMR1_HIP_CARRIER_MIX_TILE)

__global__ __launch_bounds__(kMixThreads) void k_carrier_mix(MixArgs a)
{
	const long long tile = blockIdx.x;
	for (int c = blockIdx.y; c < a.n_carriers; c += gridDim.y) {
		const long long length = (long long)uload(a.length + c);
		float2 *outc = a.out + uload(a.out_offset + c);
		const int odd = (int)((reinterpret_cast<uintptr_t>(outc) >> 3) & 1u);     // the carrier starts in the upper half of a unit
		const long long k_base = tile * kMixTile - odd;                           // the lower sample of the tile's first unit
		if (k_base >= length)
			continue;
		const long long first = a.first ? uload(a.first + c) : 0;
		long long k0[kMixUnits];
		float2 acc[kMixUnits][2];
		for (int u = 0; u < kMixUnits; u++) {
			k0[u] = k_base + 2 * (u * kMixThreads + (int)threadIdx.x);
			acc[u][0] = acc[u][1] = make_float2(0.f, 0.f);
		}

		// 1. + 2.: the overlap-add, in list order
		if (a.seg_first) {
			const long long n_lo = first + (k_base < 0 ? 0 : k_base);
			const long long n_hi = first + (k_base + kMixTile < length ? k_base + kMixTile : length);
			const int end = uload(a.seg_first + c + 1);
			int lo = uload(a.seg_first + c), hi = end;
			const long long reach = n_lo - (long long)a.max_seg_len;
			while (lo < hi) {
				const int mid = lo + ((hi - lo) >> 1);
				if (uload(a.seg_pos + mid) > reach)
					hi = mid;
				else
					lo = mid + 1;
			}
			for (int s = lo; s < end; s++) {
				const long long pos = uload(a.seg_pos + s);
				if (pos >= n_hi)
					break;
				const long long len = uload(a.seg_len + s);
				if (pos + len <= n_lo)
					continue;
				const float2 *src = a.seg_iq + uload(a.seg_src + s);
				for (int u = 0; u < kMixUnits; u++) {
					const long long k = k0[u], d = first + k - pos;
					const bool in0 = k >= 0 && k < length && d >= 0 && d < len;
					const bool in1 = k + 1 < length && d + 1 >= 0 && d + 1 < len;
					if (in0 && in1 && (reinterpret_cast<uintptr_t>(src + d) & 15u) == 0) {
						const mx_v4f v = *reinterpret_cast<const mx_v4f *>(src + d);
						acc[u][0].x += v.x; acc[u][0].y += v.y;
						acc[u][1].x += v.z; acc[u][1].y += v.w;
					} else {
						if (in0) {
							const float2 v = src[d];
							acc[u][0].x += v.x; acc[u][0].y += v.y;
						}
						if (in1) {
							const float2 v = src[d + 1];
							acc[u][1].x += v.x; acc[u][1].y += v.y;
						}
					}
				}
			}
		}

		// 3. the carrier offset
		const double cfo = a.cfo ? uload(a.cfo + c) : 0.0;
		if (cfo != 0.0) {
			for (int u = 0; u < kMixUnits; u++)
				for (int h = 0; h < 2; h++) {
					float sn, cs;
					sincosf(carrier_phase(cfo, first + k0[u] + h), &sn, &cs);
					const float2 v = acc[u][h];
					acc[u][h] = make_float2(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
				}
		}

		// 4. the noise floor
		const float sigma = a.sigma ? uload(a.sigma + c) : 0.f;
		if (sigma != 0.f) {
			const uint32_t id = a.noise_id ? uload(a.noise_id + c) : (uint32_t)c;
			const bool straddles = ((first + k_base) & 1) != 0;
			for (int u = 0; u < kMixUnits; u++) {
				const long long n0 = first + k0[u];
				uint32_t w[4];
				float2 z0, z1;
				noise_words(a.seed, id, (uint64_t)(n0 >> 1), w);
				if (!straddles) {
					z0 = noise_pair<float2>(w[0], w[1]);
					z1 = noise_pair<float2>(w[2], w[3]);
				} else {
					z0 = noise_pair<float2>(w[2], w[3]);
					noise_words(a.seed, id, (uint64_t)(n0 >> 1) + 1u, w);
					z1 = noise_pair<float2>(w[0], w[1]);
				}
				acc[u][0].x += sigma * z0.x; acc[u][0].y += sigma * z0.y;
				acc[u][1].x += sigma * z1.x; acc[u][1].y += sigma * z1.y;
			}
		}

		// 5. every sample of the carrier, nothing else
		for (int u = 0; u < kMixUnits; u++) {
			const long long k = k0[u];
			const float2 x0 = acc[u][0], x1 = acc[u][1];
			if (k >= 0 && k + 1 < length)
				__builtin_nontemporal_store((mx_v4f){x0.x, x0.y, x1.x, x1.y}, reinterpret_cast<mx_v4f *>(outc + k));
			else if (k >= 0 && k < length)
				__builtin_nontemporal_store((mx_v2f){x0.x, x0.y}, reinterpret_cast<mx_v2f *>(outc + k));
			else if (k < 0 && k + 1 < length)
				__builtin_nontemporal_store((mx_v2f){x1.x, x1.y}, reinterpret_cast<mx_v2f *>(outc + k + 1));
		}
	}
}

hipError_t launch_carrier_mix(const MixArgs &a, hipStream_t stream)
{
	if (a.n_carriers <= 0 || a.max_length == 0)
		return hipSuccess;
	// one more sample than max_length: a carrier on an odd address has its first sample alone in a unit
	const unsigned long long tiles = (a.max_length + 1 + kMixTile - 1) / kMixTile;
	if (tiles > 0x7fffffffull)
		return hipErrorInvalidValue;
	const unsigned gy = (unsigned)(a.n_carriers < 65535 ? a.n_carriers : 65535);
	hipLaunchKernelGGL(k_carrier_mix, dim3((unsigned)tiles, gy), dim3(kMixThreads), 0, stream, a);
	return hipGetLastError();
}

}  // namespace gmr1
