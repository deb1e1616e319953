// tri_query_host.cpp — mi_tri_query_host / mi_tri_offsets_host / mi_tri_fill_host (include/mi_scene_host.h): the host twins of
// tri_query_kernel, tri_count_kernel and tri_fill_kernel (contact_kernels.hpp; mi_tri_query* / mi_tri_offsets* / mi_tri_fill*). The
// compact nodes are walked in the device's order through the table the point queries' twin walks (walkTable,
// point_query_host.cpp), and boxes and primitives are tested by the MI_HD code of contact_math.hpp that the kernels run: compares,
// selects and single rounded binary32 operations, so the results equal the device's byte for byte. The fill is "the len smallest
// keys, ascending" by a sort - keys are unique within a query, so the device's heap leaves the same bytes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "scene_types.hpp"
#include "../contact_math.hpp"

namespace mi::host {

namespace {
// tri_walk of contact_kernels.hpp over the table: a node is entered when its box meets the query's bounds (closed compares);
// accept(node index) for each touching primitive of a reached leaf, true ends the walk.
template <class Accept>
void triWalk(const std::vector<WalkNode>& nodes, const mi_tri& t, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
  const f3 q0 = mk(t.a[0], t.a[1], t.a[2]), q1 = mk(t.b[0], t.b[1], t.b[2]), q2 = mk(t.c[0], t.c[1], t.c[2]);
  f3 qmn, qmx;
  tri_query_bounds(q0, q1, q2, qmn, qmx);
  const uint32_t end = tri_query_valid(q0, q1, q2) ? (uint32_t)nodes.size() : 0u;
  uint32_t i = 0;
  while (i < end) {
    const WalkNode& w = nodes[i];
    ++boxTests;
    if (!box_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), qmn, qmx)) { i = w.skip; continue; }
    if (w.kind == kInterior) { ++i; continue; }
    ++primTests;
    if (tri_touches_prim(w.kind, w.f, q0, q1, q2, qmn, qmx) && accept(i)) break;
    i = w.skip;
  }
}
}  // namespace

void triQueryHost(const mi_scene_desc& d, int kind, const mi_tri* tris, void* out, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_tri_query_host");
  uint64_t boxTests = 0, primTests = 0;
  for (size_t k = 0; k < n; ++k) {
    mi_tri t;
    memcpy(&t, tris + k, sizeof t);
    uint32_t count = 0;
    triWalk(nodes, t, boxTests, primTests, [&](uint32_t) { ++count; return kind == MI_TRI_ANY; });
    if (kind == MI_TRI_ANY) static_cast<uint8_t*>(out)[k] = count ? 1u : 0u;
    else memcpy(static_cast<char*>(out) + k * sizeof count, &count, sizeof count);      // (the caller's buffer need not be aligned)
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

void triOffsetsHost(const mi_scene_desc& d, const mi_tri* tris, uint64_t* offsets, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_tri_offsets_host");
  uint64_t boxTests = 0, primTests = 0, total = 0;
  if (n) memcpy(offsets, &total, sizeof total);
  for (size_t k = 0; k < n; ++k) {
    mi_tri t;
    memcpy(&t, tris + k, sizeof t);
    triWalk(nodes, t, boxTests, primTests, [&](uint32_t) { ++total; return false; });
    memcpy(reinterpret_cast<char*>(offsets) + (k + 1) * sizeof total, &total, sizeof total);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

void triFillHost(const mi_scene_desc& d, const mi_tri* tris, const uint64_t* offsets, mi_contact* hits, size_t capacity, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_tri_fill_host");
  uint64_t boxTests = 0, primTests = 0;
  std::vector<mi_contact> found;      // every touching primitive of the triangle; its head is copied out once sorted
  for (size_t k = 0; k < n; ++k) {
    uint64_t first, last;
    memcpy(&first, reinterpret_cast<const char*>(offsets) + k * sizeof first, sizeof first);
    memcpy(&last, reinterpret_cast<const char*>(offsets) + (k + 1) * sizeof last, sizeof last);
    uint64_t len = 0;
    if (last > first && first < capacity) len = (last < capacity ? last : capacity) - first;
    if (!len) continue;
    mi_tri t;
    memcpy(&t, tris + k, sizeof t);
    found.clear();
    triWalk(nodes, t, boxTests, primTests, [&](uint32_t at) {
      found.push_back(mi_contact{nodes[at].primID, nodes[at].geomID, (uint16_t)0, (uint32_t)k, 0u});
      return false;
    });
    std::sort(found.begin(), found.end(), [](const mi_contact& a, const mi_contact& b) { return overlap_key(a.geomID, a.primID) < overlap_key(b.geomID, b.primID); });
    const mi_contact pad = {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, (uint32_t)k, 0u};
    found.resize((size_t)len, pad);
    memcpy(reinterpret_cast<char*>(hits) + first * sizeof(mi_contact), found.data(), (size_t)len * sizeof(mi_contact));
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

}  // namespace mi::host
