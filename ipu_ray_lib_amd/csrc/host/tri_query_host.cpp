// tri_query_host.cpp — mi_tri_query_host / mi_tri_offsets_host / mi_tri_fill_host (include/mi_scene_host.h): the host twins of the
// triangle queries' kernels (contact_kernels.hpp over touch_kernels.hpp; mi_tri_query* / mi_tri_offsets* / mi_tri_fill*). The compact
// nodes are walked in the device's order (walkHost, walk_host.hpp) through their table (walkTable, walk_table.cpp), and boxes and
// primitives are tested by the MI_HD code of contact_math.hpp that the kernels run: compares, selects and single rounded binary32
// operations, so the results equal the device's byte for byte. Query, offsets and fill are the touch family's (touch_host.hpp);
// what is the triangles' own is here.
#include "touch_host.hpp"
#include "../contact_math.hpp"

namespace mi::host {

namespace {
struct TriTouch {
  using Item = mi_tri;
  using Record = mi_contact;
  static constexpr const char *kQuery = "mi_tri_query_host", *kOffsets = "mi_tri_offsets_host", *kFill = "mi_tri_fill_host";
  // tri_walk of contact_kernels.hpp over walkHost: a node is entered when its box meets the query's bounds (closed compares);
  // accept(node index, 0) for each touching primitive of a reached leaf, true ends the walk.
  template <class Accept>
  static void walk(const std::vector<WalkNode>& nodes, const mi_tri& t, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
    const f3 q0 = mk(t.a[0], t.a[1], t.a[2]), q1 = mk(t.b[0], t.b[1], t.b[2]), q2 = mk(t.c[0], t.c[1], t.c[2]);
    f3 qmn, qmx;
    tri_query_bounds(q0, q1, q2, qmn, qmx);
    walkHost(nodes, tri_query_valid(q0, q1, q2), boxTests, primTests,
      [&](const WalkNode& w) { return box_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), qmn, qmx); },
      [&](uint32_t i, const WalkNode& w) { return tri_touches_prim(w.kind, w.f, q0, q1, q2, qmn, qmx) && accept(i, 0u); });
  }
};
}  // namespace

void triQueryHost(const mi_scene_desc& d, int kind, const mi_tri* tris, void* out, size_t n, uint64_t* visits) {
  touchQueryHost<TriTouch>(d, kind, tris, out, n, visits);
}
void triOffsetsHost(const mi_scene_desc& d, const mi_tri* tris, uint64_t* offsets, size_t n, uint64_t* visits) {
  touchOffsetsHost<TriTouch>(d, tris, offsets, n, visits);
}
void triFillHost(const mi_scene_desc& d, const mi_tri* tris, const uint64_t* offsets, mi_contact* hits, size_t capacity, size_t n, uint64_t* visits) {
  touchFillHost<TriTouch>(d, tris, offsets, hits, capacity, n, visits);
}

}  // namespace mi::host
