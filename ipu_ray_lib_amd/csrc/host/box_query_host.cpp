// box_query_host.cpp — mi_box_query_host / mi_box_offsets_host / mi_box_fill_host (include/mi_scene_host.h): the host twins of
// box_query_kernel, box_count_kernel and box_fill_kernel (box_kernels.hpp; mi_box_query* / mi_box_offsets* / mi_box_fill*). The
// compact nodes are walked in the device's order through the table the point queries' twin walks (walkTable,
// point_query_host.cpp: a node's box is min and min + (float)extent, a leaf's primitive is resolved from the scene's arrays), and
// boxes and primitives are tested by the MI_HD code of box_math.hpp that the kernels run: compares, selects and single rounded
// binary32 operations, so the results equal the device's byte for byte. The fill is "the len smallest keys, ascending" by a sort -
// keys are unique within a box, so the device's heap leaves the same bytes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "scene_types.hpp"
#include "../box_math.hpp"

namespace mi::host {

namespace {
// box_walk of box_kernels.hpp over the table: a node is entered when its box meets [lo, hi] (closed compares); accept(node index,
// contained) for each touching primitive of a reached leaf, true ends the walk.
template <class Accept>
void boxWalk(const std::vector<WalkNode>& nodes, const mi_box& bx, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
  const f3 lo = mk(bx.lo[0], bx.lo[1], bx.lo[2]), hi = mk(bx.hi[0], bx.hi[1], bx.hi[2]);
  const uint32_t end = box_query_valid(lo, hi) ? (uint32_t)nodes.size() : 0u;
  uint32_t i = 0;
  while (i < end) {
    const WalkNode& w = nodes[i];
    ++boxTests;
    if (!box_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), lo, hi)) { i = w.skip; continue; }
    if (w.kind == kInterior) { ++i; continue; }
    ++primTests;
    bool contained;
    if (box_touches_prim(w.kind, w.f, lo, hi, &contained) && accept(i, contained)) break;
    i = w.skip;
  }
}
}  // namespace

void boxQueryHost(const mi_scene_desc& d, int kind, const mi_box* boxes, void* out, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_box_query_host");
  uint64_t boxTests = 0, primTests = 0;
  for (size_t k = 0; k < n; ++k) {
    mi_box bx;
    memcpy(&bx, boxes + k, sizeof bx);
    uint32_t count = 0;
    boxWalk(nodes, bx, boxTests, primTests, [&](uint32_t, bool) { ++count; return kind == MI_BOX_ANY; });
    if (kind == MI_BOX_ANY) static_cast<uint8_t*>(out)[k] = count ? 1u : 0u;
    else memcpy(static_cast<char*>(out) + k * sizeof count, &count, sizeof count);      // (the caller's buffer need not be aligned)
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

void boxOffsetsHost(const mi_scene_desc& d, const mi_box* boxes, uint64_t* offsets, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_box_offsets_host");
  uint64_t boxTests = 0, primTests = 0, total = 0;
  if (n) memcpy(offsets, &total, sizeof total);
  for (size_t k = 0; k < n; ++k) {
    mi_box bx;
    memcpy(&bx, boxes + k, sizeof bx);
    boxWalk(nodes, bx, boxTests, primTests, [&](uint32_t, bool) { ++total; return false; });
    memcpy(reinterpret_cast<char*>(offsets) + (k + 1) * sizeof total, &total, sizeof total);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

void boxFillHost(const mi_scene_desc& d, const mi_box* boxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_box_fill_host");
  uint64_t boxTests = 0, primTests = 0;
  std::vector<mi_overlap> found;      // every touching primitive of the box; its head is copied out once sorted
  for (size_t k = 0; k < n; ++k) {
    uint64_t first, last;
    memcpy(&first, reinterpret_cast<const char*>(offsets) + k * sizeof first, sizeof first);
    memcpy(&last, reinterpret_cast<const char*>(offsets) + (k + 1) * sizeof last, sizeof last);
    uint64_t len = 0;
    if (last > first && first < capacity) len = (last < capacity ? last : capacity) - first;
    if (!len) continue;
    mi_box bx;
    memcpy(&bx, boxes + k, sizeof bx);
    found.clear();
    boxWalk(nodes, bx, boxTests, primTests, [&](uint32_t at, bool contained) {
      found.push_back(mi_overlap{nodes[at].primID, nodes[at].geomID, (uint16_t)(contained ? MI_OVERLAP_CONTAINED : 0), (uint32_t)k, 0u});
      return false;
    });
    std::sort(found.begin(), found.end(), [](const mi_overlap& a, const mi_overlap& b) { return overlap_key(a.geomID, a.primID) < overlap_key(b.geomID, b.primID); });
    const mi_overlap pad = {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, (uint32_t)k, 0u};
    found.resize((size_t)len, pad);
    memcpy(reinterpret_cast<char*>(hits) + first * sizeof(mi_overlap), found.data(), (size_t)len * sizeof(mi_overlap));
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

}  // namespace mi::host
