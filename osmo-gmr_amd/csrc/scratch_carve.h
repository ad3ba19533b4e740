// scratch_carve.h -- how the host layer cuts one block of device memory into 128-byte-aligned arrays: written once per
// block, as takes from a cursor.  On a null base the takes measure the block (the pointers are the running offsets), on
// the block itself they name its arrays.  Host only, no HIP: tests/c/scratch_carve_host.cpp walks it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gmr1 {

inline size_t up128(size_t x) { return (x + 127) & ~(size_t)127; }

// The cursor.  All arithmetic is on integers: a null base is a measurement, not a pointer anything is added to.
struct Carve {
	uintptr_t base, q;
	explicit Carve(void *block) : base((uintptr_t)block), q(base) {}
	// the next n_elems elements, rounded up to whole lines; none advances nothing
	template <class T> T *take(size_t n_elems)
	{
		T *p = reinterpret_cast<T *>(q);
		q += up128(n_elems * sizeof(T));
		return p;
	}
	size_t bytes() const { return (size_t)(q - base); }
};

}  // namespace gmr1
