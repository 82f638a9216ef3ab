// Host-side helpers shared by the evaluation units (metrics.hip, vis.hip, errmap.hip, raster.hip).  The training and forward units do
// not include this header.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rnerf {

// do [a, a + na) and [b, b + nb) share a byte?  A null pointer overlaps nothing.
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

// n rounded up to a multiple of 16: the sections of a workspace stay 16-byte aligned
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace rnerf
