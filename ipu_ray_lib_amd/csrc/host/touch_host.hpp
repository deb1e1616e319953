// touch_host.hpp — the host twins of the touch family's kernels (touch_kernels.hpp), written once: walk, query, offsets, fill and
// the bounds test alone, over caller buffers that need not be aligned. A family is the shape S its kernels walk with (BoxShape in
// box_math.hpp is the plainest; touch_kernels.hpp lists what a shape holds), so the twin and the device run one spelling of
// `valid`, `meets_bounds`, `touches_prim` and of how `contained` becomes a record's flags. fn: the entry's name, for the message
// of what walkTable refuses.
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

// touch_walk of touch_kernels.hpp over walkHost: a node is entered when S::meets_bounds of its box holds; accept(node index, flags)
// for each touching primitive of a reached leaf, true ends the walk.
template <class S, class Accept>
void touchWalkHost(const std::vector<WalkNode>& nodes, const typename S::Item& item, uint64_t& boxTests, uint64_t& primTests, const Accept& accept) {
  const typename S::Fields fields = S::fields(item);
  const auto& q = S::carry(fields);
  walkHost(nodes, S::valid(fields), boxTests, primTests,
    [&](const WalkNode& w) { return S::meets_bounds(mk(w.minx, w.miny, w.minz), mk(w.maxx, w.maxy, w.maxz), q); },
    [&](uint32_t i, const WalkNode& w) {
      bool contained;
      return S::touches_prim(w.kind, w.f, q, &contained) && accept(i, S::flags(contained));
    });
}

// kind S::kAny: n bytes, the walk stops at the first accept; S::kCount: n uint32_t counts
template <class S>
void touchQueryHost(const mi_scene_desc& d, const char* fn, int kind, const typename S::Item* items, void* out, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, fn);
  uint64_t boxTests = 0, primTests = 0;
  for (size_t k = 0; k < n; ++k) {
    typename S::Item item;
    memcpy(&item, items + k, sizeof item);
    uint32_t count = 0;
    touchWalkHost<S>(nodes, item, boxTests, primTests, [&](uint32_t, uint32_t) { ++count; return kind == S::kAny; });
    if (kind == S::kAny) static_cast<uint8_t*>(out)[k] = count ? 1u : 0u;
    else memcpy(static_cast<char*>(out) + k * sizeof count, &count, sizeof count);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

template <class S>
void touchOffsetsHost(const mi_scene_desc& d, const char* fn, const typename S::Item* items, uint64_t* offsets, size_t n, uint64_t* visits) {
  const std::vector<WalkNode> nodes = walkTable(d, fn);
  uint64_t boxTests = 0, primTests = 0, total = 0;
  if (n) memcpy(offsets, &total, sizeof total);
  for (size_t k = 0; k < n; ++k) {
    typename S::Item item;
    memcpy(&item, items + k, sizeof item);
    touchWalkHost<S>(nodes, item, boxTests, primTests, [&](uint32_t, uint32_t) { ++total; return false; });
    memcpy(reinterpret_cast<char*>(offsets) + (k + 1) * sizeof total, &total, sizeof total);
  }
  if (visits) { visits[0] = boxTests; visits[1] = primTests; }
}

template <class S>
void touchFillHost(const mi_scene_desc& d, const char* fn, const typename S::Item* items, const uint64_t* offsets, typename S::Record* hits, size_t capacity, size_t n,
                   uint64_t* visits) {
  using Rec = typename S::Record;
  const std::vector<WalkNode> nodes = walkTable(d, fn);
  uint64_t boxTests = 0, primTests = 0;
  std::vector<Rec> found;      // every touching primitive of the item; its head is copied out once sorted
  for (size_t k = 0; k < n; ++k) {
    uint64_t first, last;
    memcpy(&first, reinterpret_cast<const char*>(offsets) + k * sizeof first, sizeof first);
    memcpy(&last, reinterpret_cast<const char*>(offsets) + (k + 1) * sizeof last, sizeof last);
    const uint64_t len = segment_len(first, last, capacity);
    if (!len) continue;
    typename S::Item item;
    memcpy(&item, items + k, sizeof item);
    found.clear();
    touchWalkHost<S>(nodes, item, boxTests, primTests, [&](uint32_t at, uint32_t flags) {
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

// The node test alone: whether a walk of `item` would enter the box [mn, mx]. An item that is not walked enters nothing.
template <class S>
bool touchMeetsBoundsHost(const typename S::Item& item, const float mn[3], const float mx[3]) {
  const typename S::Fields fields = S::fields(item);
  return S::valid(fields) && S::meets_bounds(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]), S::carry(fields));
}

}  // namespace mi::host
