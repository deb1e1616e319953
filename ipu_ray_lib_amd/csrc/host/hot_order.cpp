// hot_order.cpp — mi_hot_nodes / mi_hot_walk (include/mi_scene_host.h): the hot-first order of K1w's private copy of the walk's
// arrays (csrc/hot_order.hpp: the functions the device library's upload runs) and a plain walk of a node array under either
// protocol, compiled for the host so that the permutation can be checked without a GPU.
#include "../hot_order.hpp"
#include "../ray_math.h"
#include "../../../include/mi_scene_host.h"

#include <cmath>

namespace {

// The device's preorder node array of a compact BVH, as the upload derives it: the box as six floats (max = min + extent, one
// rounded add), link = the node after the subtree, hit = the first child, or link with the flag for a leaf. False: not a
// depth-first BVH2.
bool preorder_nodes(const mi_bvh_node* c, uint32_t n, mi::HotNode* out) {
  std::vector<uint32_t> skip(n);
  for (uint32_t i = n; i-- > 0;) {
    if (c[i].geom_id != MI_INVALID_GEOM) { skip[i] = i + 1; continue; }
    const uint32_t second = c[i].prim_or_second_child;
    if (!(i + 1 < n && second > i + 1 && second < n) || skip[i + 1] != second) return false;
    skip[i] = skip[second];
  }
  if (n && skip[0] != n) return false;
  for (uint32_t i = 0; i < n; ++i) {
    mi::HotNode g;
    g.minx = c[i].min_x; g.miny = c[i].min_y; g.minz = c[i].min_z;
    g.maxx = c[i].min_x + mi::half_bits_to_float(c[i].dx);
    g.maxy = c[i].min_y + mi::half_bits_to_float(c[i].dy);
    g.maxz = c[i].min_z + mi::half_bits_to_float(c[i].dz);
    g.link = skip[i] << 5;
    g.hit = c[i].geom_id != MI_INVALID_GEOM ? ((skip[i] << 5) | mi::kHotLeafFlag) : ((i + 1) << 5);
    out[i] = g;
  }
  return true;
}

}  // namespace

extern "C" int mi_hot_nodes(const mi_bvh_node* compact, uint32_t num_nodes, void* preorder, uint32_t* order, void* hot, uint32_t* leaf_link) {
  if (num_nodes && (!compact || !preorder || !order || !hot || !leaf_link)) return MI_ERR_INVALID_ARG;
  if (num_nodes >= (mi::kHotLeafFlag >> 5)) return MI_ERR_INVALID_ARG;
  if (!num_nodes) return MI_OK;
  mi::HotNode* pre = static_cast<mi::HotNode*>(preorder);
  if (!preorder_nodes(compact, num_nodes, pre)) return MI_ERR_INVALID_ARG;
  mi::hot_first_order(pre, num_nodes, order);
  mi::hot_permute_nodes(pre, num_nodes, order, static_cast<mi::HotNode*>(hot), leaf_link);
  return MI_OK;
}

extern "C" int mi_hot_share(const void* preorder, uint32_t num_nodes, const uint32_t* order, double* share) {
  if (num_nodes && (!preorder || !order || !share)) return MI_ERR_INVALID_ARG;
  mi::hot_prefix_share(static_cast<const mi::HotNode*>(preorder), num_nodes, order, share);
  return MI_OK;
}

// The collapsed tree of the private copy (hot_order.hpp: hot_collapse_keep / hot_collapse_nodes, then the same order, permutation
// and share over the survivors).
extern "C" int mi_hot_collapse(const mi_bvh_node* compact, uint32_t num_nodes, double theta, void* preorder, uint8_t* keep, uint32_t* from, void* collapsed,
                               uint32_t* order, void* hot, uint32_t* leaf_link, double* share, uint32_t counts[2]) {
  if (!counts || (num_nodes && (!compact || !preorder || !keep || !from || !collapsed || !order || !hot || !leaf_link || !share))) return MI_ERR_INVALID_ARG;
  if (num_nodes >= (mi::kHotLeafFlag >> 5) || theta != theta) return MI_ERR_INVALID_ARG;
  counts[0] = counts[1] = 0u;
  if (!num_nodes) return MI_OK;
  if (theta < 0.0) theta = mi::kHotCollapseTheta;
  mi::HotNode* pre = static_cast<mi::HotNode*>(preorder);
  if (!preorder_nodes(compact, num_nodes, pre)) return MI_ERR_INVALID_ARG;
  const uint32_t m = mi::hot_collapse_keep(pre, num_nodes, theta, keep, &counts[1]);
  counts[0] = m;
  mi::HotNode* sub = static_cast<mi::HotNode*>(collapsed);
  mi::hot_collapse_nodes(pre, num_nodes, keep, sub, from);
  mi::hot_first_order(sub, m, order);
  mi::hot_permute_nodes(sub, m, order, static_cast<mi::HotNode*>(hot), leaf_link);
  mi::hot_prefix_share_any(sub, m, order, share);
  return MI_OK;
}

// The node array the plain HOT builds walk (hot_join_regions): the collapsed tree, then every node; *exact_start = the place of the second
// region's root, where a cast on the literal box test starts.
extern "C" int mi_hot_join(const void* thin, const uint32_t* thin_link, uint32_t m, const void* full, const uint32_t* full_link, uint32_t n, void* joined, uint32_t* joined_link,
                           uint32_t* exact_start) {
  if ((m && (!thin || !thin_link)) || (n && (!full || !full_link)) || ((m || n) && (!joined || !joined_link)) || !exact_start) return MI_ERR_INVALID_ARG;
  if ((uint64_t)m + n >= (mi::kHotLeafFlag >> 5)) return MI_ERR_INVALID_ARG;
  mi::hot_join_regions(static_cast<const mi::HotNode*>(thin), thin_link, m, static_cast<const mi::HotNode*>(full), full_link, n, static_cast<mi::HotNode*>(joined), joined_link);
  *exact_start = m;
  return MI_OK;
}

// Whether a cast takes the literal box test in K1w (exactSlab, trace_wavefront.hpp): a reciprocal direction component or an origin component
// that is not finite.
extern "C" int mi_hot_cast_is_literal(const float origin[3], const float direction[3]) {
  if (!origin || !direction) return 0;
  for (int a = 0; a < 3; ++a) if (!(std::fabs(1.f / direction[a]) < INFINITY) || !(std::fabs(origin[a]) < INFINITY)) return 1;
  return 0;
}

// mi_hot_walk with the ray's far end given and the box test as the kernels run it on their literal lanes (box_hit_literal_axis,
// trace_kernels.hpp: the far product scaled by kSlabScale): t_max = the cast's hit.t while these boxes are tested. Returns the number
// of entries like mi_hot_walk; *box_tests (may be null) receives the number of box tests among them.
extern "C" uint32_t mi_hot_walk_count(const void* nodes, uint32_t num_nodes, const uint32_t* leaf_link, uint32_t start, const float origin[3], const float direction[3], float t_max,
                                      uint32_t* visits, uint32_t capacity, uint32_t* box_tests, int* status) {
  if (status) *status = MI_OK;
  if (box_tests) *box_tests = 0u;
  if (!num_nodes) return 0u;
  if (!nodes || !origin || !direction || (!visits && capacity) || start >= num_nodes) { if (status) *status = MI_ERR_INVALID_ARG; return 0u; }
  const mi::HotNode* nd = static_cast<const mi::HotNode*>(nodes);
  const uint32_t end = num_nodes << 5;
  const float inv[3] = {1.f / direction[0], 1.f / direction[1], 1.f / direction[2]};
  uint32_t count = 0, tests = 0, node = start << 5;
  for (uint64_t guard = 0; node < end && guard < 4ull * num_nodes + 4ull; ++guard) {
    const mi::HotNode& g = nd[node >> 5];
    if (count < capacity) visits[count] = node >> 5;
    ++count; ++tests;
    float t0 = 0.f, t1 = t_max;
    const float lo[3] = {g.minx, g.miny, g.minz}, hi[3] = {g.maxx, g.maxy, g.maxz};
    for (int a = 0; a < 3; ++a) {
      float tmin = (lo[a] - origin[a]) * inv[a], tmax = (hi[a] - origin[a]) * inv[a];
      if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; }
      tmax *= mi::kSlabScale;
      t0 = tmin > t0 ? tmin : t0; t1 = tmax < t1 ? tmax : t1;
    }
    uint32_t next = !(t0 > t1) ? g.hit : g.link;
    if (next & mi::kHotLeafFlag) {
      next &= ~mi::kHotLeafFlag;
      uint32_t leaf;
      if (leaf_link) { leaf = next >> 5; if (leaf >= num_nodes) { if (status) *status = MI_ERR_INVALID_ARG; return count; } next = leaf_link[leaf]; }
      else leaf = (next >> 5) - 1u;
      if (count < capacity) visits[count] = leaf | mi::kHotLeafFlag;
      ++count;
    }
    if (next > end || (next & 31u)) { if (status) *status = MI_ERR_INVALID_ARG; return count; }
    node = next;
  }
  if (box_tests) *box_tests = tests;
  if (node < end && status) *status = MI_ERR_INVALID_ARG;
  return count;
}

// The stackless walk K1w makes, box tests only (no primitive ever shortens the ray: every box the ray's line segment [0, inf)
// meets is entered): visits[] takes the index of every node whose box is tested, with bit 31 set again for a leaf whose box
// is hit - the primitive test. leaf_link = null: the shared arrays' protocol (a leaf's hit successor is its link with the flag:
// the lane stands behind the leaf); otherwise the layout-free one (the flag rides on the leaf's own offset, the node that follows
// comes from leaf_link). Successors outside the array end the walk with MI_ERR_INVALID_ARG in *status.
extern "C" uint32_t mi_hot_walk(const void* nodes, uint32_t num_nodes, const uint32_t* leaf_link, const float origin[3], const float direction[3],
                                uint32_t* visits, uint32_t capacity, int* status) {
  if (status) *status = MI_OK;
  if (!num_nodes) return 0u;
  if (!nodes || !origin || !direction || (!visits && capacity)) { if (status) *status = MI_ERR_INVALID_ARG; return 0u; }
  const mi::HotNode* nd = static_cast<const mi::HotNode*>(nodes);
  const uint32_t end = num_nodes << 5;
  const float inv[3] = {1.f / direction[0], 1.f / direction[1], 1.f / direction[2]};
  uint32_t count = 0, node = 0;
  // (every step moves to a node the walk has not tested yet in a well-formed array; the bound only stops a malformed one)
  for (uint64_t guard = 0; node < end && guard < 4ull * num_nodes + 4ull; ++guard) {
    const mi::HotNode& g = nd[node >> 5];
    if (count < capacity) visits[count] = node >> 5;
    ++count;
    float t0 = 0.f, t1 = INFINITY;
    const float lo[3] = {g.minx, g.miny, g.minz}, hi[3] = {g.maxx, g.maxy, g.maxz};
    for (int a = 0; a < 3; ++a) {      // the reference's compare / select sequence (CompactBVH2Node.hpp:14-50)
      float tmin = (lo[a] - origin[a]) * inv[a], tmax = (hi[a] - origin[a]) * inv[a];
      if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; }
      t0 = tmin > t0 ? tmin : t0; t1 = tmax < t1 ? tmax : t1;
    }
    uint32_t next = !(t0 > t1) ? g.hit : g.link;
    if (next & mi::kHotLeafFlag) {
      next &= ~mi::kHotLeafFlag;
      uint32_t leaf;
      if (leaf_link) { leaf = next >> 5; if (leaf >= num_nodes) { if (status) *status = MI_ERR_INVALID_ARG; return count; } next = leaf_link[leaf]; }
      else leaf = (next >> 5) - 1u;
      if (count < capacity) visits[count] = leaf | mi::kHotLeafFlag;
      ++count;
    }
    if (next > end || (next & 31u)) { if (status) *status = MI_ERR_INVALID_ARG; return count; }
    node = next;
  }
  if (node < end && status) *status = MI_ERR_INVALID_ARG;
  return count;
}
