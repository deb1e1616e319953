// hot_order_check.cpp — a stand-alone check of csrc/hot_order.hpp and host/hot_order.cpp (its own main; built and run by
// tests/test_hot_order.py with the address and undefined-behaviour sanitizers, never part of a library): random depth-first BVH2s
// of compact nodes, their hot-first order, the private node array, and walks of both arrays for random rays, which must visit the
// same nodes and primitives in the same order; and the collapsed tree (mi_hot_collapse), whose walks must test the same primitives in the same
// order. Exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/mi_scene_host.h"
#include "../ray_math.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 32); }
float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) * (1.f / 16777216.f); }

struct Box { float lo[3], hi[3]; };

// a random tree over `prims` leaf boxes in depth-first order: first child = i + 1, second child's index in the node
uint32_t grow(std::vector<mi_bvh_node>& out, const std::vector<Box>& leaf, uint32_t first, uint32_t count, Box& box) {
  const uint32_t at = (uint32_t)out.size();
  out.push_back(mi_bvh_node{});
  if (count == 1) {
    box = leaf[first];
    out[at].prim_or_second_child = first; out[at].geom_id = 0;
  } else {
    const uint32_t left = 1 + rnd() % (count - 1);
    Box a, b;
    grow(out, leaf, first, left, a);
    const uint32_t second = grow(out, leaf, first + left, count - left, b);
    for (int k = 0; k < 3; ++k) { box.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; box.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
    out[at].prim_or_second_child = second; out[at].geom_id = MI_INVALID_GEOM;
  }
  out[at].min_x = box.lo[0]; out[at].min_y = box.lo[1]; out[at].min_z = box.lo[2];
  out[at].dx = mi::half_not_smaller(box.hi[0] - box.lo[0]);
  out[at].dy = mi::half_not_smaller(box.hi[1] - box.lo[1]);
  out[at].dz = mi::half_not_smaller(box.hi[2] - box.lo[2]);
  return at;
}

int fail(const char* what, uint32_t prims, uint32_t ray) { fprintf(stderr, "hot_order_check: %s (tree of %u primitives, ray %u)\n", what, prims, ray); return 1; }

}  // namespace

int main() {
  const uint32_t sizes[] = {0, 1, 2, 3, 7, 64, 1000};
  for (uint32_t prims : sizes) {
    std::vector<Box> leaf(prims);
    for (Box& b : leaf) for (int k = 0; k < 3; ++k) { const float c = uni(-20.f, 20.f), h = uni(0.f, 3.f); b.lo[k] = c - h; b.hi[k] = c + h; }
    std::vector<mi_bvh_node> compact;
    Box root;
    if (prims) grow(compact, leaf, 0, prims, root);
    const uint32_t n = (uint32_t)compact.size();
    std::vector<unsigned char> pre(32 * (size_t)n), hot(32 * (size_t)n);
    std::vector<uint32_t> order(n), link(n);
    if (mi_hot_nodes(compact.data(), n, pre.data(), order.data(), hot.data(), link.data()) != MI_OK) return fail("mi_hot_nodes refused a depth-first BVH2", prims, 0);
    std::vector<unsigned char> seen(n, 0);
    for (uint32_t k = 0; k < n; ++k) { if (order[k] >= n || seen[order[k]]) return fail("the order is not a bijection", prims, 0); seen[order[k]] = 1; }
    if (n && order[0] != 0) return fail("the root does not stand first", prims, 0);
    // the collapsed tree (hot_collapse_keep / hot_collapse_nodes): survivors in preorder, then the same order and permutation over them
    std::vector<unsigned char> pre2(32 * (size_t)n), thin(32 * (size_t)n), hot2(32 * (size_t)n), keep(n);
    std::vector<uint32_t> from(n), order2(n), link2(n);
    std::vector<double> share2(n);
    uint32_t counts[2] = {0, 0};
    if (mi_hot_collapse(compact.data(), n, -1.0, pre2.data(), keep.data(), from.data(), thin.data(), order2.data(), hot2.data(), link2.data(), share2.data(), counts) != MI_OK)
      return fail("mi_hot_collapse refused a depth-first BVH2", prims, 0);
    const uint32_t m = counts[0];
    if (m > n || (n && (m == 0 || !keep[0] || from[0] != 0 || order2[0] != 0))) return fail("the collapsed tree lost its root", prims, 0);
    if (n && memcmp(pre.data(), pre2.data(), pre.size()) != 0) return fail("mi_hot_collapse and mi_hot_nodes disagree on the preorder array", prims, 0);
    std::vector<unsigned char> joined(32 * ((size_t)m + n));
    std::vector<uint32_t> jlink((size_t)m + n);
    uint32_t exact = 0;
    if (mi_hot_join(hot2.data(), link2.data(), m, hot.data(), link.data(), n, joined.data(), jlink.data(), &exact) != MI_OK || exact != m) return fail("mi_hot_join failed", prims, 0);
    const uint32_t cap = 4 * n + 4;
    std::vector<uint32_t> a(cap), b(cap);
    for (uint32_t r = 0; r < 2000; ++r) {
      float o[3], d[3];
      for (int k = 0; k < 3; ++k) { o[k] = uni(-30.f, 30.f); d[k] = uni(-1.f, 1.f); }
      if (r % 7 == 0) d[rnd() % 3] = 0.f;      // (an axis-parallel ray: an infinite reciprocal, NaN slab products)
      if (r % 31 == 0) { d[0] = 0.f; d[1] = 0.f; d[2] = 1.f; }
      int sa = 0, sb = 0;
      const uint32_t ca = mi_hot_walk(pre.data(), n, nullptr, o, d, a.data(), cap, &sa);
      const uint32_t cb = mi_hot_walk(hot.data(), n, link.data(), o, d, b.data(), cap, &sb);
      if (sa != MI_OK || sb != MI_OK) return fail("a walk left the array", prims, r);
      if (ca != cb || ca > cap) return fail("the two walks differ in length", prims, r);
      for (uint32_t k = 0; k < ca; ++k)
        if (((b[k] & 0x80000000u) | order[b[k] & 0x7FFFFFFFu]) != a[k]) return fail("the two walks visit different nodes", prims, r);
      // the collapsed walk: the same leaves in the same order, with the ray's far end open and given
      const float far = (r % 3 == 0) ? uni(0.f, 60.f) : INFINITY;
      uint32_t ta = 0, tb = 0;
      const uint32_t wa = mi_hot_walk_count(pre.data(), n, nullptr, 0, o, d, far, a.data(), cap, &ta, &sa);
      // (as the device walks it: the joined array, a cast on the literal box test from the region of every node)
      const uint32_t wb = mi_hot_walk_count(joined.data(), m + n, jlink.data(), mi_hot_cast_is_literal(o, d) ? exact : 0u, o, d, far, b.data(), cap, &tb, &sb);
      if (sa != MI_OK || sb != MI_OK || wa > cap || wb > cap) return fail("a counted walk left the array", prims, r);
      uint32_t ka = 0, kb = 0;
      for (;; ++ka, ++kb) {
        while (ka < wa && !(a[ka] & 0x80000000u)) ++ka;
        while (kb < wb && !(b[kb] & 0x80000000u)) ++kb;
        if (ka >= wa || kb >= wb) break;
        const uint32_t at = b[kb] & 0x7FFFFFFFu;
        if ((at < m ? from[order2[at]] : order[at - m]) != (a[ka] & 0x7FFFFFFFu)) return fail("the collapsed walk tests another primitive", prims, r);
      }
      if ((ka < wa) != (kb < wb)) return fail("the collapsed walk tests more or fewer primitives", prims, r);
    }
  }
  // what is refused: a second child that is not behind the first child's subtree
  {
    mi_bvh_node bad[3];
    memset(bad, 0, sizeof bad);
    bad[0].geom_id = MI_INVALID_GEOM; bad[0].prim_or_second_child = 1; bad[1].geom_id = 0; bad[2].geom_id = 0;
    unsigned char pre[96], hot[96]; uint32_t order[3], link[3];
    if (mi_hot_nodes(bad, 3, pre, order, hot, link) != MI_ERR_INVALID_ARG) return fail("a malformed tree was accepted", 2, 0);
  }
  puts("hot_order_check OK");
  return 0;
}
