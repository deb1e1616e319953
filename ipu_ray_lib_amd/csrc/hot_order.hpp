// hot_order.hpp — the hot-first node order of K1w's private copy of the walk's arrays (option "hot_nodes").
//
// The stackless walk only needs each node's two successors, so a copy of the node array may stand in any order. This one
// puts the nodes a path tracer's rays visit most in front, so that a short prefix - what a workgroup can stage in LDS -
// covers most visits: the array is cut into its chains of first children (a chain starts at the root or at a second child
// and runs down the first children to a leaf: a run of consecutive preorder indices), and the chains are laid out by
// falling half-area of their first node's box, ties by preorder index; the root's chain stands first whatever its area,
// so the root stays node 0 and its first child node 1 (root_start). A visit's probability goes with the area of the
// node's parent, and a chain's head is the largest box in it.
//
// The order is a pure function of the node array (binary64 products of binary32 differences, a stable sort): the same scene
// renders through the same copy everywhere. Plain C++, shared by the device library's upload and the host library's export.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mi {

struct HotNode { float minx, maxx, miny, maxy, minz, maxz; uint32_t link, hit; };     // the layout of GNode (trace_kernels.hpp)
static_assert(sizeof(HotNode) == 32, "HotNode mirrors the 32-byte device node");
constexpr uint32_t kHotLeafFlag = 0x80000000u;

// order[k] = the preorder index of the node that stands at place k of the private array.
inline void hot_first_order(const HotNode* nodes, uint32_t n, uint32_t* order) {
  struct Chain { uint32_t head; double area; };
  std::vector<Chain> chains;
  for (uint32_t i = 0; i < n; ++i) {
    if (i != 0 && !(nodes[i - 1].hit & kHotLeafFlag)) continue;      // a first child: inside its parent's chain
    const double dx = (double)nodes[i].maxx - (double)nodes[i].minx, dy = (double)nodes[i].maxy - (double)nodes[i].miny, dz = (double)nodes[i].maxz - (double)nodes[i].minz;
    chains.push_back({i, dx * dy + dy * dz + dz * dx});
  }
  if (chains.size() > 1)
    std::stable_sort(chains.begin() + 1, chains.end(), [](const Chain& a, const Chain& b) { return a.area > b.area; });
  uint32_t k = 0;
  for (const Chain& c : chains) {
    uint32_t i = c.head;
    for (;;) { order[k++] = i; if (nodes[i].hit & kHotLeafFlag) break; ++i; }
  }
}

// The private node array for `order`, and per node the word a leaf's primitive record starts with in the private copies:
// successors stay byte offsets (place << 5, n << 5 = the walk ends). The walk of this array is layout-free: a leaf's `hit`
// successor is its OWN offset with the flag - "stop here, test the primitive of this node" - and the node that follows comes
// out of the record (leafLink[k]: the leaf's link; 0 for interior nodes).
inline void hot_permute_nodes(const HotNode* nodes, uint32_t n, const uint32_t* order, HotNode* out, uint32_t* leafLink) {
  std::vector<uint32_t> place(n + 1u);
  for (uint32_t k = 0; k < n; ++k) place[order[k]] = k;
  place[n] = n;
  for (uint32_t k = 0; k < n; ++k) {
    const HotNode& s = nodes[order[k]];
    HotNode d = s;
    d.link = place[s.link >> 5] << 5;
    if (s.hit & kHotLeafFlag) { d.hit = (k << 5) | kHotLeafFlag; leafLink[k] = d.link; }
    else { d.hit = place[s.hit >> 5] << 5; leafLink[k] = 0u; }
    out[k] = d;
  }
}

// What share of a random line's box tests falls on the first k places of the order, for every k: share[k - 1], from the
// surface-area model the builder's cost uses - a node is tested when its parent's box is hit, which a random line through the
// root's box does with a probability proportional to that box's half-area (the root: its own). A property of the tree alone.
inline void hot_prefix_share(const HotNode* nodes, uint32_t n, const uint32_t* order, double* share) {
  auto half_area = [&](uint32_t i) {
    const double dx = (double)nodes[i].maxx - (double)nodes[i].minx, dy = (double)nodes[i].maxy - (double)nodes[i].miny, dz = (double)nodes[i].maxz - (double)nodes[i].minz;
    return dx * dy + dy * dz + dz * dx;
  };
  std::vector<double> weight(n, 0.0);
  if (n) weight[0] = half_area(0);
  for (uint32_t i = 0; i < n; ++i) {
    if (nodes[i].hit & kHotLeafFlag) continue;
    const double a = half_area(i);
    weight[i + 1] = a;                                             // the first child, and the second: the node after the first one's subtree
    const uint32_t second = nodes[i + 1].link >> 5;
    if (second < n) weight[second] = a;
  }
  double sum = 0.0;
  for (uint32_t k = 0; k < n; ++k) { sum += weight[order[k]]; share[k] = sum; }
  for (uint32_t k = 0; k < n; ++k) share[k] = sum > 0.0 ? share[k] / sum : 1.0;
}

// ---- the collapsed tree ------------------------------------------------------------------------------------
// An interior node's box test only culls: which primitives a cast tests, in which order and with which hit.t depends on the leaves'
// own box tests alone, as long as a hit child implies a hit parent. The slab test is monotone in the planes (a box that lies inside
// another, all six stored floats compared, is hit only if the other is; hit.t only falls between a parent's test and its
// child's), so an interior node whose two children lie inside its stored box can be taken out of the walk: its parent's successor
// goes to its first child instead, whose own link already leads to the second. What changes is the number of box tests, nothing
// else. That holds for finite slab products only. On the literal test (a zero or denormal direction component, a non-finite origin) it
// FAILS for one nested pair, which host/slab_nesting_check.cpp finds and the box scene's walls contain: a child that is flat on an axis
// and lies on a face of a parent that is not, the origin on that plane, the direction component -0 - the child's two products are NaN
// and drop out of every compare, the parent's are NaN and -inf (or +inf and NaN) and miss. So casts on the literal test never walk the
// collapsed tree: the private arrays carry a second region behind it, every node in hot-first order (hot_join_regions), and such a
// cast starts at that region's root. The stored boxes are NOT nested as a rule (max = min + a binary16 extent, rounded per node), hence the containment test per
// node; the area rule keeps the nodes that cull: X goes when half-area(X) > theta * half-area(its nearest surviving ancestor).
//
// The survivors, in preorder, are again a preorder array of the same format - a tree of any arity: an interior node's first child
// is the next survivor, a leaf's link the next survivor, every link the first survivor at or after the old one's first-child
// descent - so hot_first_order and hot_permute_nodes run over them unchanged. Chains now continue through deleted nodes: a chain
// runs from its head (the root, or a survivor that follows a leaf) down through the surviving first children to a leaf. The root
// survives and its first surviving descendant stands at place 1 (root_start).
constexpr double kHotCollapseTheta = 0.5;      // (profiles/r13_k1w_collapse.txt: real box tests per cast at 0.5 / 0.6 / 0.75)

inline double hot_half_area(const HotNode& g) {
  const double dx = (double)g.maxx - (double)g.minx, dy = (double)g.maxy - (double)g.miny, dz = (double)g.maxz - (double)g.minz;
  return dx * dy + dy * dz + dz * dx;
}
inline bool hot_box_inside(const HotNode& c, const HotNode& p) {
  return c.minx >= p.minx && c.maxx <= p.maxx && c.miny >= p.miny && c.maxy <= p.maxy && c.minz >= p.minz && c.maxz <= p.maxz;
}

// keep[i] = 1: node i of the preorder array stays in the walk. Returns the number of survivors; *blocked (may be null) counts the
// interior nodes the area rule would delete and the containment rule keeps.
inline uint32_t hot_collapse_keep(const HotNode* nodes, uint32_t n, double theta, uint8_t* keep, uint32_t* blocked) {
  std::vector<double> above(n, 0.0);      // the half-area of the nearest surviving ancestor (parents precede children in preorder)
  uint32_t kept = 0, held = 0;
  for (uint32_t i = 0; i < n; ++i) {
    keep[i] = 1;
    if (nodes[i].hit & kHotLeafFlag) { ++kept; continue; }
    const uint32_t first = i + 1, second = nodes[first].link >> 5;
    const double a = hot_half_area(nodes[i]);
    if (i != 0 && a > theta * above[i]) {
      if (hot_box_inside(nodes[first], nodes[i]) && hot_box_inside(nodes[second], nodes[i])) keep[i] = 0; else ++held;
    }
    above[first] = above[second] = keep[i] ? a : above[i];
    kept += keep[i];
  }
  if (blocked) *blocked = held;
  return kept;
}

// The survivors as a preorder array of their own (out, from[j] = the old index of survivor j; both as long as the survivor count).
inline void hot_collapse_nodes(const HotNode* nodes, uint32_t n, const uint8_t* keep, HotNode* out, uint32_t* from) {
  std::vector<uint32_t> to(n + 1u);      // where a successor that pointed at node i points now: the first survivor down i's first children
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; ++i) { to[i] = m; if (keep[i]) from[m++] = i; }      // (the deleted nodes in front of a survivor are its chain of ancestors)
  to[n] = m;
  for (uint32_t j = 0; j < m; ++j) {
    const HotNode& s = nodes[from[j]];
    HotNode d = s;
    d.link = to[s.link >> 5] << 5;
    d.hit = (s.hit & kHotLeafFlag) ? (d.link | kHotLeafFlag) : (to[s.hit >> 5] << 5);
    out[j] = d;
  }
}

// The private node array of the plain HOT builds: the collapsed tree's m nodes (thin, thinLink: hot_permute_nodes over the survivors), then
// all n nodes (full, fullLink: the same over the whole array) with their successors moved behind them. Both regions end at (m + n) << 5.
// out and outLink hold m + n entries; the second region's root stands at place m.
inline void hot_join_regions(const HotNode* thin, const uint32_t* thinLink, uint32_t m, const HotNode* full, const uint32_t* fullLink, uint32_t n, HotNode* out, uint32_t* outLink) {
  const uint32_t endThin = m << 5, end = (m + n) << 5, base = m << 5;
  for (uint32_t k = 0; k < m; ++k) {
    HotNode d = thin[k];
    if (d.link == endThin) d.link = end;
    out[k] = d;
    outLink[k] = ((d.hit & kHotLeafFlag) && thinLink[k] == endThin) ? end : thinLink[k];
  }
  for (uint32_t k = 0; k < n; ++k) {
    HotNode d = full[k];
    d.link += base; d.hit += base;      // (a leaf's hit is its own offset with the flag: the flag stays)
    out[m + k] = d;
    outLink[m + k] = (d.hit & kHotLeafFlag) ? fullLink[k] + base : 0u;
  }
}

// hot_prefix_share for a preorder array of any arity (a node's children: the node behind it, then link by link up to its own link).
inline void hot_prefix_share_any(const HotNode* nodes, uint32_t n, const uint32_t* order, double* share) {
  std::vector<double> weight(n, 0.0);
  if (n) weight[0] = hot_half_area(nodes[0]);
  for (uint32_t i = 0; i < n; ++i) {
    if (nodes[i].hit & kHotLeafFlag) continue;
    const double a = hot_half_area(nodes[i]);
    for (uint32_t c = i + 1, end = nodes[i].link >> 5; c < end && c < n; c = nodes[c].link >> 5) weight[c] = a;
  }
  double sum = 0.0;
  for (uint32_t k = 0; k < n; ++k) { sum += weight[order[k]]; share[k] = sum; }
  for (uint32_t k = 0; k < n; ++k) share[k] = sum > 0.0 ? share[k] / sum : 1.0;
}

}  // namespace mi
