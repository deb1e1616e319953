// frustum_query_host.cpp — mi_frustum_query_host / mi_frustum_offsets_host / mi_frustum_fill_host (include/mi_scene_host.h): the
// host twins of the frustum queries' kernels (frustum_kernels.hpp over touch_kernels.hpp; mi_frustum_query* / mi_frustum_offsets* /
// mi_frustum_fill*). The compact nodes are walked in the device's order (walkHost, walk_host.hpp) through their table (walkTable,
// walk_table.cpp), and boxes and primitives are tested by the MI_HD code of frustum_math.hpp that the kernels run: compares,
// selects and single rounded binary32 operations, so the results equal the device's byte for byte. Query, offsets and fill are the
// touch family's (touch_host.hpp); what is the frusta's own is here.
#include "touch_host.hpp"
#include "../frustum_math.hpp"

namespace mi::host {

namespace {
static_assert((int)MI_FRUSTUM_ANY == (int)MI_BOX_ANY && (int)MI_FRUSTUM_COUNT == (int)MI_BOX_COUNT, "touchQueryHost takes any touch family's kind");

FPlane planeOf(const float p[4]) {
  FPlane r;
  r.x = p[0];
  r.y = p[1];
  r.z = p[2];
  r.d = p[3];
  return r;
}
Frustum frustumOf(const mi_frustum& f) {
  Frustum q;
  q.p0 = planeOf(f.planes[0]);
  q.p1 = planeOf(f.planes[1]);
  q.p2 = planeOf(f.planes[2]);
  q.p3 = planeOf(f.planes[3]);
  q.p4 = planeOf(f.planes[4]);
  q.p5 = planeOf(f.planes[5]);
  return q;
}

struct FrustumTouch {
  using Item = mi_frustum;
  using Record = mi_overlap;
  static constexpr const char *kQuery = "mi_frustum_query_host", *kOffsets = "mi_frustum_offsets_host", *kFill = "mi_frustum_fill_host";
  // frustum_walk of frustum_kernels.hpp over walkHost: a node is entered when frustum_meets_bounds of its box holds; accept(node
  // index, MI_OVERLAP_CONTAINED or 0) for each touching primitive of a reached leaf, true ends the walk.
  template <class Accept>
  static void walk(const std::vector<WalkNode>& nodes, const mi_frustum& fr, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
    const Frustum q = frustumOf(fr);
    walkHost(nodes, frustum_query_valid(q), boxTests, primTests,
      [&](const WalkNode& w) { return frustum_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), q); },
      [&](uint32_t i, const WalkNode& w) {
        bool contained;
        return frustum_touches_prim(w.kind, w.f, q, &contained) && accept(i, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u);
      });
  }
};
}  // namespace

void frustumQueryHost(const mi_scene_desc& d, int kind, const mi_frustum* frusta, void* out, size_t n, uint64_t* visits) {
  touchQueryHost<FrustumTouch>(d, kind, frusta, out, n, visits);
}
void frustumOffsetsHost(const mi_scene_desc& d, const mi_frustum* frusta, uint64_t* offsets, size_t n, uint64_t* visits) {
  touchOffsetsHost<FrustumTouch>(d, frusta, offsets, n, visits);
}
void frustumFillHost(const mi_scene_desc& d, const mi_frustum* frusta, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n, uint64_t* visits) {
  touchFillHost<FrustumTouch>(d, frusta, offsets, hits, capacity, n, visits);
}
bool frustumMeetsBoundsHost(const mi_frustum& frustum, const float mn[3], const float mx[3]) {
  const Frustum q = frustumOf(frustum);
  return frustum_query_valid(q) && frustum_meets_bounds(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]), q);
}

}  // namespace mi::host
