// walk_host.hpp — the host twins' walk, written once: walk_preorder of bvh_walk.hpp over the compact nodes' table (WalkNode,
// walkTable: scene_types.hpp, walk_table.cpp). The nodes are visited in the device's order - preorder, first child first, a node
// passed goes on at the node behind its subtree - and a family passes the two lambdas its kernels pass, over the MI_HD
// arithmetic both sides compile: the visits and the results equal the device's.
#pragma once

#include <vector>

#include "scene_types.hpp"
#include "../list_segment.hpp"      // the fills' segment rule, which the twins share with the kernels

namespace mi::host {

// `valid` false: nothing is walked. enter(const WalkNode&) -> bool: whether the node's box is entered. leaf(node index, const
// WalkNode&) -> bool: called for the primitive of an entered leaf, true ends the walk. boxTests and primTests count what the
// instrumented kernels count: one per node looked at, one per call of `leaf`.
template <class Enter, class Leaf>
void walkHost(const std::vector<WalkNode>& nodes, bool valid, uint64_t& boxTests, uint64_t& primTests, const Enter& enter, const Leaf& leaf) {
  const uint32_t end = valid ? (uint32_t)nodes.size() : 0u;
  uint32_t i = 0;
  while (i < end) {
    const WalkNode& w = nodes[i];
    ++boxTests;
    if (!enter(w)) { i = w.skip; continue; }
    if (w.kind == kInterior) { ++i; continue; }
    ++primTests;
    if (leaf(i, w)) break;
    i = w.skip;
  }
}

}  // namespace mi::host
