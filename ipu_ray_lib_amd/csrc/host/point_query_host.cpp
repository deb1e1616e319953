// point_query_host.cpp — mi_point_query_host (include/mi_scene_host.h): the host twin of point_query_kernel (point_kernels.hpp,
// mi_point_query / mi_point_query_device). The compact nodes are walked in the device's order - preorder, first child first,
// a node passed goes on at the node behind its subtree -, a node's box is min and min + (float)extent (one rounded add, as the
// device record carries it), a leaf's primitive is resolved from the scene's arrays as mi_scene_create resolves it, and boxes and
// primitives are evaluated by the MI_HD code of point_math.hpp that the kernel runs: every step is a compare / select or one
// rounded binary32 operation, so the results equal the device's byte for byte.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "scene_types.hpp"
#include "../point_math.hpp"

namespace mi::host {

// The walk's table of desc's nodes; fn: the entry's name, for the message of what is refused.
std::vector<WalkNode> walkTable(const mi_scene_desc& d, const char* fn) {
  auto need = [fn](bool ok, const char* what) { if (!ok) throw std::invalid_argument(std::string(fn) + ": " + what); };
  const uint32_t N = d.num_nodes;
  need(N == 0 || d.bvh_nodes, "bvh_nodes is null");
  need(d.num_geometry == 0 || d.geometry, "geometry is null");
  need(d.num_geometry <= kMaxGeometries, kTooManyGeometries);
  need(d.num_meshes == 0 || (d.mesh_info && d.mesh_tris && d.mesh_verts), "mesh arrays are null");
  need(d.num_spheres == 0 || d.spheres, "spheres is null");
  need(d.num_discs == 0 || d.discs, "discs is null");

  // the walk's table: skip links from the back (mi_scene_create's checks of the depth-first layout), boxes, leaf records
  std::vector<WalkNode> nodes(N);
  for (uint32_t i = N; i-- > 0;) {
    const mi_bvh_node& c = d.bvh_nodes[i];
    WalkNode& w = nodes[i];
    w.minx = c.min_x; w.miny = c.min_y; w.minz = c.min_z;
    w.maxx = c.min_x + half_bits_to_float(c.dx);
    w.maxy = c.min_y + half_bits_to_float(c.dy);
    w.maxz = c.min_z + half_bits_to_float(c.dz);
    for (float& x : w.f) x = 0.f;
    w.primID = c.prim_or_second_child; w.geomID = c.geom_id;
    if (c.geom_id == MI_INVALID_GEOM) {
      const uint32_t second = c.prim_or_second_child;
      need(i + 1 < N && second > i + 1 && second < N, "BVH is not a depth-first BVH2 (bad second child index)");
      need(nodes[i + 1].skip == second, "BVH is not in depth-first order (first child's subtree must end at the second child)");
      w.skip = nodes[second].skip;
      w.kind = kInterior;
      continue;
    }
    w.skip = i + 1;
    need(c.geom_id < d.num_geometry, "leaf geomID out of range");
    const mi_geom_ref& r = d.geometry[c.geom_id];
    need(r.type <= 2 && r.index < (r.type == 0 ? d.num_meshes : r.type == 1 ? d.num_spheres : d.num_discs), "geometry index out of range");
    w.kind = r.type;
    if (r.type == 0) {
      const mi_mesh_info& m = d.mesh_info[r.index];
      need(c.prim_or_second_child < m.num_triangles && (uint64_t)m.first_index + c.prim_or_second_child < d.num_tris, "leaf primID out of range");
      const size_t base = 3 * ((size_t)m.first_index + c.prim_or_second_child);
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = d.mesh_tris[base + k];
        need((uint64_t)m.first_vertex + v < d.num_verts, "triangle vertex index out of range");
        const mi_vec3& p = d.mesh_verts[m.first_vertex + v];
        w.f[3 * k] = p.x; w.f[3 * k + 1] = p.y; w.f[3 * k + 2] = p.z;
      }
    } else if (r.type == 1) {
      const mi_sphere& s = d.spheres[r.index];
      w.f[0] = s.x; w.f[1] = s.y; w.f[2] = s.z; w.f[3] = s.radius; w.f[4] = s.radius * s.radius;
      w.primID = 0;
    } else {
      const mi_disc& c2 = d.discs[r.index];
      w.f[0] = c2.nx; w.f[1] = c2.ny; w.f[2] = c2.nz; w.f[3] = c2.cx; w.f[4] = c2.cy; w.f[5] = c2.cz; w.f[6] = c2.r * c2.r;
      w.primID = 0;
    }
  }
  need(N == 0 || nodes[0].skip == N, "BVH root does not span the node array");
  return nodes;
}

void pointQueryHost(const mi_scene_desc& d, int kind, const mi_point* points, void* out, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, "mi_point_query_host");
  const uint32_t N = d.num_nodes;

  uint64_t boxTests = 0, primEvals = 0;
  for (size_t k = 0; k < n; ++k) {
    mi_point pt;
    memcpy(&pt, points + k, sizeof pt);
    const f3 p = mk(pt.x, pt.y, pt.z);
    float best = pt.radius * pt.radius;
    uint32_t leaf = kInterior;
    ClosestPoint win;
    win.q = mk(0.f, 0.f, 0.f); win.v = win.w = 0.f;
    const uint32_t end = point_query_valid(p, pt.radius) ? N : 0u;
    uint32_t i = 0;
    while (i < end) {
      const WalkNode& w = nodes[i];
      ++boxTests;
      const bool enter = point_box_dist2(w.minx, w.maxx, w.miny, w.maxy, w.minz, w.maxz, p) < best;
      if (!enter) { i = w.skip; continue; }
      if (w.kind == kInterior) { ++i; continue; }
      ++primEvals;
      const ClosestPoint c = closest_on_prim(w.kind, w.f, p);
      const float d2 = point_dist2(p, c.q);
      if (d2 < best) {
        leaf = i;
        if (kind == MI_POINT_WITHIN) break;
        best = d2; win = c;
      }
      i = w.skip;
    }
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
// near_walk of near_kernels.hpp over the table: a node is entered when db < r2 && db <= bound (bound: +inf, or what accept lowered
// it to); accept(d2, node index) for each primitive of a reached leaf with d2 < r2.
template <class Accept>
void nearWalk(const std::vector<WalkNode>& nodes, const mi_point& pt, float& bound, uint64_t& boxTests, uint64_t& primEvals, const Accept& accept) {
  const f3 p = mk(pt.x, pt.y, pt.z);
  const float r2 = pt.radius * pt.radius;
  const uint32_t end = point_query_valid(p, pt.radius) ? (uint32_t)nodes.size() : 0u;
  uint32_t i = 0;
  while (i < end) {
    const WalkNode& w = nodes[i];
    ++boxTests;
    const float db = point_box_dist2(w.minx, w.maxx, w.miny, w.maxy, w.minz, w.maxz, p);
    const bool enter = db < r2 && db <= bound;
    if (!enter) { i = w.skip; continue; }
    if (w.kind == kInterior) { ++i; continue; }
    ++primEvals;
    const ClosestPoint c = closest_on_prim(w.kind, w.f, p);
    const float d2 = point_dist2(p, c.q);
    if (d2 < r2) accept(d2, i);
    i = w.skip;
  }
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
    uint64_t len = 0;
    if (hi > lo && lo < capacity) len = (hi < capacity ? hi : capacity) - lo;
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
