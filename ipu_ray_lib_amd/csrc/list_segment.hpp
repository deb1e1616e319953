// list_segment.hpp — the segment rule of every list fill (crossing lists, neighbour lists, box lists, contact lists), one
// definition for the kernels and the host twins: item i of a fill writes into hits[offsets[i] .. offsets[i + 1]), cut at the
// caller's `capacity`.
#pragma once

#include "ray_math.h"

namespace mi {

// The length of the segment [first, last) cut at capacity; a decreasing pair, or a start at or past capacity, is an empty one.
// A fill touches hits[first + j] for j < segment_len(...) and nothing else.
MI_HD uint64_t segment_len(uint64_t first, uint64_t last, uint64_t capacity) {
  uint64_t len = 0;
  if (last > first && first < capacity) len = (last < capacity ? last : capacity) - first;
  return len;
}

}  // namespace mi
