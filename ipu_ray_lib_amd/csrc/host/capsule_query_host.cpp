// capsule_query_host.cpp — mi_capsule_query_host / mi_capsule_offsets_host / mi_capsule_fill_host (include/mi_scene_host.h): the
// host twins of the capsule queries' kernels (capsule_kernels.hpp over touch_kernels.hpp; mi_capsule_query* / mi_capsule_offsets* /
// mi_capsule_fill*). The compact nodes are walked in the device's order (walkHost, walk_host.hpp) through their table (walkTable,
// walk_table.cpp), and boxes and primitives are tested by the MI_HD code of capsule_math.hpp that the kernels run: compares,
// selects and single rounded binary32 operations, so the results equal the device's byte for byte. Query, offsets and fill are the
// touch family's (touch_host.hpp); what is the capsules' own is here.
#include "touch_host.hpp"
#include "../capsule_math.hpp"

namespace mi::host {

namespace {
static_assert((int)MI_CAPSULE_ANY == (int)MI_BOX_ANY && (int)MI_CAPSULE_COUNT == (int)MI_BOX_COUNT, "touchQueryHost takes any touch family's kind");

Capsule capsuleOf(const mi_capsule& c) { return capsule_make(mk(c.a[0], c.a[1], c.a[2]), mk(c.b[0], c.b[1], c.b[2]), c.radius); }
bool capsuleValid(const mi_capsule& c) { return capsule_query_valid(mk(c.a[0], c.a[1], c.a[2]), mk(c.b[0], c.b[1], c.b[2]), c.radius); }

struct CapsuleTouch {
  using Item = mi_capsule;
  using Record = mi_overlap;
  static constexpr const char *kQuery = "mi_capsule_query_host", *kOffsets = "mi_capsule_offsets_host", *kFill = "mi_capsule_fill_host";
  // capsule_walk of capsule_kernels.hpp over walkHost: a node is entered when capsule_meets_bounds of its box holds; accept(node
  // index, MI_OVERLAP_CONTAINED or 0) for each touching primitive of a reached leaf, true ends the walk.
  template <class Accept>
  static void walk(const std::vector<WalkNode>& nodes, const mi_capsule& cp, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
    const Capsule q = capsuleOf(cp);
    walkHost(nodes, capsuleValid(cp), boxTests, primTests,
      [&](const WalkNode& w) { return capsule_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), q); },
      [&](uint32_t i, const WalkNode& w) {
        bool contained;
        return capsule_touches_prim(w.kind, w.f, q, &contained) && accept(i, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u);
      });
  }
};
}  // namespace

void capsuleQueryHost(const mi_scene_desc& d, int kind, const mi_capsule* capsules, void* out, size_t n, uint64_t* visits) {
  touchQueryHost<CapsuleTouch>(d, kind, capsules, out, n, visits);
}
void capsuleOffsetsHost(const mi_scene_desc& d, const mi_capsule* capsules, uint64_t* offsets, size_t n, uint64_t* visits) {
  touchOffsetsHost<CapsuleTouch>(d, capsules, offsets, n, visits);
}
void capsuleFillHost(const mi_scene_desc& d, const mi_capsule* capsules, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n, uint64_t* visits) {
  touchFillHost<CapsuleTouch>(d, capsules, offsets, hits, capacity, n, visits);
}
bool capsuleMeetsBoundsHost(const mi_capsule& capsule, const float mn[3], const float mx[3]) {
  return capsuleValid(capsule) && capsule_meets_bounds(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]), capsuleOf(capsule));
}

}  // namespace mi::host
