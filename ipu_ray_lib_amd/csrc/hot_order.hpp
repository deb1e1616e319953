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

}  // namespace mi
