// box_query_host.cpp — mi_box_query_host / mi_box_offsets_host / mi_box_fill_host (include/mi_scene_host.h): the host twins of the
// box queries' kernels (box_kernels.hpp over touch_kernels.hpp; mi_box_query* / mi_box_offsets* / mi_box_fill*). The compact nodes
// are walked in the device's order (walkHost, walk_host.hpp) through their table (walkTable, walk_table.cpp), and boxes and
// primitives are tested by the MI_HD code of box_math.hpp that the kernels run: compares, selects and single rounded binary32
// operations, so the results equal the device's byte for byte. Query, offsets and fill are the touch family's (touch_host.hpp);
// what is the boxes' own is here.
#include "touch_host.hpp"

namespace mi::host {

namespace {
struct BoxTouch {
  using Item = mi_box;
  using Record = mi_overlap;
  static constexpr const char *kQuery = "mi_box_query_host", *kOffsets = "mi_box_offsets_host", *kFill = "mi_box_fill_host";
  // box_walk of box_kernels.hpp over walkHost: a node is entered when its box meets [lo, hi] (closed compares); accept(node index,
  // MI_OVERLAP_CONTAINED or 0) for each touching primitive of a reached leaf, true ends the walk.
  template <class Accept>
  static void walk(const std::vector<WalkNode>& nodes, const mi_box& bx, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
    const f3 lo = mk(bx.lo[0], bx.lo[1], bx.lo[2]), hi = mk(bx.hi[0], bx.hi[1], bx.hi[2]);
    walkHost(nodes, box_query_valid(lo, hi), boxTests, primTests,
      [&](const WalkNode& w) { return box_meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), lo, hi); },
      [&](uint32_t i, const WalkNode& w) {
        bool contained;
        return box_touches_prim(w.kind, w.f, lo, hi, &contained) && accept(i, contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u);
      });
  }
};
}  // namespace

void boxQueryHost(const mi_scene_desc& d, int kind, const mi_box* boxes, void* out, size_t n, uint64_t* visits) {
  touchQueryHost<BoxTouch>(d, kind, boxes, out, n, visits);
}
void boxOffsetsHost(const mi_scene_desc& d, const mi_box* boxes, uint64_t* offsets, size_t n, uint64_t* visits) {
  touchOffsetsHost<BoxTouch>(d, boxes, offsets, n, visits);
}
void boxFillHost(const mi_scene_desc& d, const mi_box* boxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n, uint64_t* visits) {
  touchFillHost<BoxTouch>(d, boxes, offsets, hits, capacity, n, visits);
}

}  // namespace mi::host
