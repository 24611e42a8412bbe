// Host-side precondition helpers of the small-kernel entry points (misc.hip, sam.hip): alignment and
// the overlap of operand ranges.  Plain pointer arithmetic: everything here is answered before any runtime call.
#pragma once
#include <stdint.h>

namespace lgd_contract {

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// [p, p + pb) and [q, q + qb) share a byte (a NULL operand shares none)
inline bool overlaps(const void* p, int64_t pb, const void* q, int64_t qb) {
  if (!p || !q) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

// an output that may BE an input of the same extent (every thread rewrites only what it has read itself): only a
// partial overlap is wrong
inline bool partly_overlaps(const void* out, const void* in, int64_t bytes) {
  return out != in && overlaps(out, bytes, in, bytes);
}

}  // namespace lgd_contract
