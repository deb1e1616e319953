// point_query_host.cpp — mi_point_query_host (include/mi_scene_host.h): the host twin of point_query_kernel (point_kernels.hpp,
// mi_point_query / mi_point_query_device). The compact nodes are walked in the device's order (walkHost, walk_host.hpp) through
// their table (walkTable, walk_table.cpp), and boxes and primitives are evaluated by the MI_HD code of point_math.hpp that the
// kernel runs: every step is a compare / select or one rounded binary32 operation, so the results equal the device's byte for
// byte.
#include <cstring>
#include <vector>

#include "walk_host.hpp"
#include "../point_math.hpp"

namespace mi::host {

void pointQueryHost(const mi_scene_desc& d, int kind, const mi_point* points, void* out, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_point_query_host");

  uint64_t boxTests = 0, primEvals = 0;
  for (size_t k = 0; k < n; ++k) {
    mi_point pt;
    memcpy(&pt, points + k, sizeof pt);
    const f3 p = mk(pt.x, pt.y, pt.z);
    float best = pt.radius * pt.radius;
    uint32_t leaf = kInterior;
    ClosestPoint win;
    win.q = mk(0.f, 0.f, 0.f); win.v = win.w = 0.f;
    walkHost(nodes, point_query_valid(p, pt.radius), boxTests, primEvals,
      [&](const WalkNode& w) { return point_box_dist2(w.minx, w.maxx, w.miny, w.maxy, w.minz, w.maxz, p) < best; },
      [&](uint32_t i, const WalkNode& w) {
        const ClosestPoint c = closest_on_prim(w.kind, w.f, p);
        const float d2 = point_dist2(p, c.q);
        if (d2 < best) {
          leaf = i;
          if (kind == MI_POINT_WITHIN) return true;
          best = d2; win = c;
        }
        return false;
      });
    if (kind == MI_POINT_WITHIN) {
      static_cast<uint8_t*>(out)[k] = leaf != kInterior ? 1u : 0u;
      continue;
    }
    mi_point_hit h;
    memset(&h, 0, sizeof h);
    if (leaf != kInterior) {
      h.dist = sqrtf(best); h.prim_id = nodes[leaf].primID; h.geom_id = nodes[leaf].geomID; h.flags = 0;
      h.point.x = win.q.x; h.point.y = win.q.y; h.point.z = win.q.z; h.b1 = win.v; h.b2 = win.w;
    } else {
      h.dist = pt.radius; h.prim_id = MI_INVALID_PRIM; h.geom_id = MI_INVALID_GEOM; h.flags = MI_FLAG_ESCAPED;
    }
    memcpy(static_cast<char*>(out) + k * sizeof h, &h, sizeof h);      // (the caller's buffer need not be aligned)
  }
  if (visits) { visits[0] = boxTests; visits[1] = primEvals; }
}

// ---- neighbour lists: the host twins of near_count_kernel / near_fill_kernel (near_kernels.hpp, mi_near_offsets* / mi_near_fill*) ----
namespace {
// near_walk of near_kernels.hpp over walkHost: a node is entered when db < r2 && db <= bound (bound: +inf, or what accept lowered
// it to); accept(d2, node index) for each primitive of a reached leaf with d2 < r2.
template <class Accept>
void nearWalk(const std::vector<WalkNode>& nodes, const mi_point& pt, float& bound, uint64_t& boxTests, uint64_t& primEvals, const Accept& accept) {
  const f3 p = mk(pt.x, pt.y, pt.z);
  const float r2 = pt.radius * pt.radius;
  walkHost(nodes, point_query_valid(p, pt.radius), boxTests, primEvals,
    [&](const WalkNode& w) {
      const float db = point_box_dist2(w.minx, w.maxx, w.miny, w.maxy, w.minz, w.maxz, p);
      return db < r2 && db <= bound;
    },
    [&](uint32_t i, const WalkNode& w) {
      const ClosestPoint c = closest_on_prim(w.kind, w.f, p);
      const float d2 = point_dist2(p, c.q);
      if (d2 < r2) accept(d2, i);
      return false;
    });
}

// a sorts before b: dist2 as a float, then geomID, then primID
bool neighbourBefore(const mi_neighbour& a, const mi_neighbour& b) {
  if (a.dist2 < b.dist2) return true;
  if (!(a.dist2 == b.dist2)) return false;
  return a.geomID != b.geomID ? a.geomID < b.geomID : a.primID < b.primID;
}
}  // namespace

void nearOffsetsHost(const mi_scene_desc& d, const mi_point* points, uint64_t* offsets, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_near_offsets_host");
  uint64_t boxTests = 0, primEvals = 0, total = 0;
  if (n) memcpy(offsets, &total, sizeof total);      // (the caller's buffers need not be aligned)
  for (size_t k = 0; k < n; ++k) {
    mi_point pt;
    memcpy(&pt, points + k, sizeof pt);
    float bound = kInf;
    nearWalk(nodes, pt, bound, boxTests, primEvals, [&](float, uint32_t) { ++total; });
    memcpy(reinterpret_cast<char*>(offsets) + (k + 1) * sizeof total, &total, sizeof total);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primEvals; }
}

void nearFillHost(const mi_scene_desc& d, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits, size_t capacity, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_near_fill_host");
  uint64_t boxTests = 0, primEvals = 0;
  std::vector<mi_neighbour> seg;      // the point's segment, copied out once the walk is done (the caller's buffer need not be aligned)
  for (size_t k = 0; k < n; ++k) {
    uint64_t lo, hi;
    memcpy(&lo, reinterpret_cast<const char*>(offsets) + k * sizeof lo, sizeof lo);
    memcpy(&hi, reinterpret_cast<const char*>(offsets) + (k + 1) * sizeof hi, sizeof hi);
    const uint64_t len = segment_len(lo, hi, capacity);
    if (!len) continue;
    mi_point pt;
    memcpy(&pt, points + k, sizeof pt);
    seg.resize((size_t)len);
    uint64_t held = 0;
    mi_neighbour tail = {};
    float bound = kInf;
    nearWalk(nodes, pt, bound, boxTests, primEvals, [&](float d2, uint32_t at) {
      const mi_neighbour rec = {d2, nodes[at].primID, nodes[at].geomID, 0, (uint32_t)k};
      uint64_t j;
      if (held < len) {
        j = held++;
      } else {
        if (!neighbourBefore(rec, tail)) return;
        j = len - 1;
      }
      const bool last = j == len - 1;
      mi_neighbour end = rec;
      while (j > 0) {
        const mi_neighbour prev = seg[j - 1];
        if (!neighbourBefore(rec, prev)) break;
        seg[j] = prev;
        if (j == len - 1) end = prev;
        --j;
      }
      seg[j] = rec;
      if (last) { tail = end; bound = end.dist2; }
    });
    const mi_neighbour pad = {kInf, MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, (uint32_t)k};
    for (uint64_t j = held; j < len; ++j) seg[j] = pad;
    memcpy(reinterpret_cast<char*>(hits) + lo * sizeof(mi_neighbour), seg.data(), (size_t)len * sizeof(mi_neighbour));
  }
  if (visits) { visits[0] = boxTests; visits[1] = primEvals; }
}

}  // namespace mi::host
