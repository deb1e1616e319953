// touch_host.hpp — the host twins of the touch family's kernels (touch_kernels.hpp), written once: query, offsets and fill over
// caller buffers that need not be aligned. A family describes itself as on the device, by a struct Q:
//
//   Q::Item, Q::Record                          mi_box / mi_overlap, mi_tri / mi_contact, mi_obox / mi_overlap, mi_capsule / mi_overlap, mi_frustum / mi_overlap
//   Q::kQuery, Q::kOffsets, Q::kFill            the entries' names, for the message of what walkTable refuses
//   Q::walk(nodes, item, boxTests, primTests, accept)
//                                               the item's walk over walkHost (walk_host.hpp): accept(node index, flags) for each
//                                               touching primitive, `flags` what a record of it carries; true ends the walk
//
// The fill is "the len smallest keys, ascending" by a sort - keys are unique within an item, so the device's heap leaves the same
// bytes. visits: {box tests, primitive tests}, may be null.
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "walk_host.hpp"
#include "../box_math.hpp"      // overlap_key

namespace mi::host {

// kind 0 (MI_BOX_ANY, MI_TRI_ANY, MI_OBOX_ANY, MI_CAPSULE_ANY, MI_FRUSTUM_ANY): n bytes, the walk stops at the first accept; kind 1: n uint32_t counts
template <class Q>
void touchQueryHost(const mi_scene_desc& d, int kind, const typename Q::Item* items, void* out, size_t n, uint64_t* visits) {
  static_assert((int)MI_BOX_ANY == (int)MI_TRI_ANY, "any touch family's kind");
  const std::vector<WalkNode> nodes = walkTable(d, Q::kQuery);
  uint64_t boxTests = 0, primTests = 0;
  for (size_t k = 0; k < n; ++k) {
    typename Q::Item item;
    memcpy(&item, items + k, sizeof item);
    uint32_t count = 0;
    Q::walk(nodes, item, boxTests, primTests, [&](uint32_t, uint32_t) { ++count; return kind == MI_BOX_ANY; });
    if (kind == MI_BOX_ANY) static_cast<uint8_t*>(out)[k] = count ? 1u : 0u;
    else memcpy(static_cast<char*>(out) + k * sizeof count, &count, sizeof count);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

template <class Q>
void touchOffsetsHost(const mi_scene_desc& d, const typename Q::Item* items, uint64_t* offsets, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, Q::kOffsets);
  uint64_t boxTests = 0, primTests = 0, total = 0;
  if (n) memcpy(offsets, &total, sizeof total);
  for (size_t k = 0; k < n; ++k) {
    typename Q::Item item;
    memcpy(&item, items + k, sizeof item);
    Q::walk(nodes, item, boxTests, primTests, [&](uint32_t, uint32_t) { ++total; return false; });
    memcpy(reinterpret_cast<char*>(offsets) + (k + 1) * sizeof total, &total, sizeof total);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

template <class Q>
void touchFillHost(const mi_scene_desc& d, const typename Q::Item* items, const uint64_t* offsets, typename Q::Record* hits, size_t capacity, size_t n, uint64_t* visits) {
  using Rec = typename Q::Record;
  const std::vector<WalkNode> nodes = walkTable(d, Q::kFill);
  uint64_t boxTests = 0, primTests = 0;
  std::vector<Rec> found;      // every touching primitive of the item; its head is copied out once sorted
  for (size_t k = 0; k < n; ++k) {
    uint64_t first, last;
    memcpy(&first, reinterpret_cast<const char*>(offsets) + k * sizeof first, sizeof first);
    memcpy(&last, reinterpret_cast<const char*>(offsets) + (k + 1) * sizeof last, sizeof last);
    const uint64_t len = segment_len(first, last, capacity);
    if (!len) continue;
    typename Q::Item item;
    memcpy(&item, items + k, sizeof item);
    found.clear();
    Q::walk(nodes, item, boxTests, primTests, [&](uint32_t at, uint32_t flags) {
      found.push_back(Rec{nodes[at].primID, nodes[at].geomID, (uint16_t)flags, (uint32_t)k, 0u});
      return false;
    });
    std::sort(found.begin(), found.end(), [](const Rec& a, const Rec& b) { return overlap_key(a.geomID, a.primID) < overlap_key(b.geomID, b.primID); });
    const Rec pad = {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, (uint32_t)k, 0u};
    found.resize((size_t)len, pad);
    memcpy(reinterpret_cast<char*>(hits) + first * sizeof(Rec), found.data(), (size_t)len * sizeof(Rec));
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

}  // namespace mi::host
