// obox_query_host.cpp — mi_obox_query_host / mi_obox_offsets_host / mi_obox_fill_host (include/mi_scene_host.h): the host twins of
// the oriented-box queries' kernels (obox_kernels.hpp over touch_kernels.hpp; mi_obox_query* / mi_obox_offsets* / mi_obox_fill*). The
// compact nodes are walked in the device's order (walkHost, walk_host.hpp) through their table (walkTable, walk_table.cpp), and
// boxes and primitives are tested by the MI_HD code of obox_math.hpp that the kernels run: compares, selects and single rounded
// binary32 operations, so the results equal the device's byte for byte. Query, offsets and fill are the touch family's
// (touch_host.hpp); what is the oriented boxes' own is here.
#include "touch_host.hpp"
#include "../obox_math.hpp"

namespace mi::host {

namespace {
static_assert((int)MI_OBOX_ANY == (int)MI_BOX_ANY && (int)MI_OBOX_COUNT == (int)MI_BOX_COUNT, "touchQueryHost takes any touch family's kind");

OBox oboxOf(const mi_obox& b) {
  return obox_make(mk(b.centre[0], b.centre[1], b.centre[2]), mk(b.half[0], b.half[1], b.half[2]), b.quat[0], b.quat[1], b.quat[2], b.quat[3]);
}
bool oboxValid(const mi_obox& b) {
  return obox_query_valid(mk(b.centre[0], b.centre[1], b.centre[2]), mk(b.half[0], b.half[1], b.half[2]), b.quat[0], b.quat[1], b.quat[2], b.quat[3]);
}

struct OBoxTouch {
  using Item = mi_obox;
  using Record = mi_overlap;
  static constexpr const char *kQuery = "mi_obox_query_host", *kOffsets = "mi_obox_offsets_host", *kFill = "mi_obox_fill_host";
  // obox_walk of obox_kernels.hpp over walkHost: a node is entered when obox_meets_bounds of its box holds; accept(node index,
  // MI_OVERLAP_CONTAINED or 0) for each touching primitive of a reached leaf, true ends the walk.
  template <class Accept>
  static void walk(const std::vector<WalkNode>& nodes, const mi_obox& bx, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
    const OBox q = oboxOf(bx);
    walkHost(nodes, oboxValid(bx), boxTests, primTests,
      [&](const WalkNode& w) { return obox_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), q); },
      [&](uint32_t i, const WalkNode& w) {
        bool contained;
        return obox_touches_prim(w.kind, w.f, q, &contained) && accept(i, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u);
      });
  }
};
}  // namespace

void oboxQueryHost(const mi_scene_desc& d, int kind, const mi_obox* oboxes, void* out, size_t n, uint64_t* visits) {
  touchQueryHost<OBoxTouch>(d, kind, oboxes, out, n, visits);
}
void oboxOffsetsHost(const mi_scene_desc& d, const mi_obox* oboxes, uint64_t* offsets, size_t n, uint64_t* visits) {
  touchOffsetsHost<OBoxTouch>(d, oboxes, offsets, n, visits);
}
void oboxFillHost(const mi_scene_desc& d, const mi_obox* oboxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n, uint64_t* visits) {
  touchFillHost<OBoxTouch>(d, oboxes, offsets, hits, capacity, n, visits);
}
bool oboxMeetsBoundsHost(const mi_obox& obox, const float mn[3], const float mx[3]) {
  return oboxValid(obox) && obox_meets_bounds(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]), oboxOf(obox));
}

}  // namespace mi::host
