// The host side of the query families - ray queries (mi_query*), point queries (mi_point_query*), crossing counts and signs
// (mi_count_query*, mi_point_sign*), crossing lists (mi_list_*), neighbour lists (mi_near_*) and the touch families, which
// TouchFamilies below lists: one launch frame, one build selection, one argument checker, one two-slot host pipeline, and the
// extern "C" entries on top of them. Included by raylib.hip, in its translation unit, once mi_scene, LaunchSlot, guarded,
// HIP_CHECK and kMaxWorkItems are defined (group_render.hpp is included the same way). A new family supplies a kernel header, a
// launcher body inside launchFrame, its buffer rules for queryArgsBad, and its entries; a new touch family
// supplies its Q, one name in TouchFamilies and one MI_TOUCH_ENTRIES line.
#pragma once

#include <initializer_list>
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------------

// What every query launch does around its kernels: nothing for n == 0, the work-index limit (every entry has checked it: this
// is the one place a launcher repeats it), the stream's launch slot, a DeviceScene copy (queries always start at the root:
// root_start assumes tMin = 0, tMax = inf), one thread per work item in blocks of 256, and behind the kernels the slot's lastWork
// event: ~mi_scene waits for it, and so do update, rebuild and set-geometry before they overwrite a record.
// enqueue(slot, dsv, grid, block, cnt) launches the kernels on `stream`.
template <class Enqueue>
void launchFrame(mi_scene& S, const char* fn, const char* noun, size_t n, hipStream_t stream, const Enqueue& enqueue) {
  if (n == 0) return;
  if (n > kMaxWorkItems) throw ArgError(std::string(fn) + ": more " + noun + " than one launch indexes (kMaxWorkItems)");
  const uint32_t cnt = (uint32_t)n;
  LaunchSlot& slot = S.slotFor(stream);
  const DeviceScene dsv = S.ds;
  enqueue(slot, dsv, dim3((cnt + 255) / 256), dim3(256), cnt);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(slot.lastWork, stream));
}

// The build a launch takes, as a tag for a generic lambda: double_fallback first (it has no instrumented build: it takes
// precedence, as in shadow-trace renders), then fast, then full_stats, then the plain one. HAS_DOUBLE / HAS_FAST: whether the
// family has such builds at all - only the combinations named here are ever instantiated.
template <bool STATS, bool DOUBLE, bool FAST>
struct Build { static constexpr bool stats = STATS, dbl = DOUBLE, fast = FAST; };

template <bool HAS_DOUBLE, bool HAS_FAST, class Go>
void pickBuild(const SceneOptions& opt, const Go& go) {
  if constexpr (HAS_DOUBLE) { if (opt.doubleFallback) return go(Build<false, true, false>{}); }
  if constexpr (HAS_FAST) { if (opt.fast) return go(Build<false, false, true>{}); }
  if (opt.fullStats) return go(Build<true, false, false>{});
  go(Build<false, false, false>{});
}

// a run-time flag as a compile-time one: go(std::true_type{}) or go(std::false_type{})
template <class Go>
void withFlag(bool flag, const Go& go) {
  if (flag) go(std::true_type{}); else go(std::false_type{});
}

// Ray queries (mi_query_device): closest hit (MI_QUERY_CLOSEST, n mi_query_hit) or any hit (MI_QUERY_ANY, n bytes) of n
// caller-supplied rays. Option query_kernel picks the one-thread-per-ray kernel (0) or K4 (1); full_stats, double_fallback and
// fast pick the build, as for renders.
void launchQuery(mi_scene& S, int kind, const mi_ray* d_rays, void* d_out, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_query", "rays", n, stream, [&](LaunchSlot& slot, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    if (S.opt.queryKernel != 0) HIP_CHECK(hipMemsetAsync(slot.d_workCounter, 0, sizeof(uint32_t), stream));
    withFlag(kind == MI_QUERY_ANY, [&](auto any) { pickBuild<true, true>(S.opt, [&](auto b) {
      constexpr bool ANY = decltype(any)::value;
      using B = decltype(b);
      if (S.opt.queryKernel == 0) {
        hipLaunchKernelGGL((query_plain_kernel<ANY, B::stats, B::dbl, B::fast>), grid, block, 0, stream, dsv, d_rays, d_out, cnt);
        return;
      }
      // persistent grid: as many workgroups as stay resident, never more than the batch has rays for
      const auto kern = query_wave_kernel<ANY, B::stats, B::dbl, B::fast>;
      const uint32_t perUnit = S.residentBlocks(reinterpret_cast<const void*>(kern), 256, 0);
      const uint32_t wgs = (uint32_t)std::min<uint64_t>(grid.x, (uint64_t)S.cus() * perUnit);
      if (S.opt.sayGrid) fprintf(stderr, "mi_raylib: query grid %u workgroups = %u units x %u resident\n", wgs, S.cus(), perUnit);
      hipLaunchKernelGGL(kern, dim3(wgs), block, 0, stream, dsv, d_rays, d_out, cnt, slot.d_workCounter, S.opt.queryTune);
    }); });
  });
}

// Point queries (mi_point_query_device): the nearest primitive within each point's radius (MI_POINT_CLOSEST, n mi_point_hit) or
// whether there is one (MI_POINT_WITHIN, n bytes), one thread per point (point_kernels.hpp). full_stats picks the instrumented
// build; the arithmetic options and the query-kernel options do not apply.
void launchPointQuery(mi_scene& S, int kind, const mi_point* d_points, void* d_out, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_point_query", "points", n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    withFlag(kind == MI_POINT_WITHIN, [&](auto within) { pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((point_query_kernel<decltype(within)::value, decltype(b)::stats>), grid, block, 0, stream, dsv, d_points, d_out, cnt);
    }); });
  });
}

// Crossing counts (mi_count_query_device): how many surfaces each of n caller-supplied rays crosses inside its interval, one thread
// per ray (count_kernels.hpp). double_fallback and full_stats pick the build; fast, query_kernel and query_tune do not apply.
void launchCountQuery(mi_scene& S, const mi_ray* d_rays, uint32_t* d_counts, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_count_query", "rays", n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<true, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((count_query_kernel<decltype(b)::stats, decltype(b)::dbl>), grid, block, 0, stream, dsv, d_rays, d_counts, cnt);
    });
  });
}

// Inside tests and signed distance (mi_point_sign_device). MI_SIGN_DISTANCE: the point query as mi_point_query_device launches it,
// then point_sign_kernel, which walks the crossings of each point's ray along `dir` and marks the records of the points inside in
// place; MI_SIGN_INSIDE: that walk alone, writing bytes. Both on `stream`, the slot's lastWork event behind the last launch.
void launchPointSign(mi_scene& S, int kind, const mi_point* d_points, void* d_out, f3 dir, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_point_sign", "points", n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    if (kind == MI_SIGN_DISTANCE) {
      pickBuild<false, false>(S.opt, [&](auto b) {
        hipLaunchKernelGGL((point_query_kernel<false, decltype(b)::stats>), grid, block, 0, stream, dsv, d_points, d_out, cnt);
      });
      HIP_CHECK(hipGetLastError());
    }
    withFlag(kind == MI_SIGN_DISTANCE, [&](auto distance) { pickBuild<true, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((point_sign_kernel<decltype(distance)::value, decltype(b)::stats, decltype(b)::dbl>), grid, block, 0, stream, dsv, d_points, d_out, dir, cnt);
    }); });
  });
}

// The prefix sum behind a list's offsets, in place on the 64-bit counts a count walk has written to d_incl: tile sums -> their
// scan by one workgroup -> every tile's scan with its base; a batch of one tile is the last launch alone. The tile sums live in
// the stream's launch slot: allocated when a call finds too little room, never otherwise.
void scanOffsets(LaunchSlot& slot, uint64_t* d_incl, uint32_t cnt, hipStream_t stream) {
  const uint32_t tiles = (cnt + kScanTile - 1) / kScanTile;
  if (tiles > 1 && slot.scanSumsCap < tiles) {
    if (slot.d_scanSums) { HIP_CHECK(hipStreamSynchronize(stream)); (void)hipFree(slot.d_scanSums); slot.d_scanSums = nullptr; slot.scanSumsCap = 0; }
    const size_t room = std::max<size_t>(tiles, 1024);
    HIP_CHECK(hipMalloc(&slot.d_scanSums, room * sizeof(uint64_t)));
    slot.scanSumsCap = room;
  }
  if (tiles > 1) {
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, d_incl, slot.d_scanSums, cnt);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, stream, slot.d_scanSums, tiles);
  }
  hipLaunchKernelGGL(scan_apply_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, d_incl, tiles > 1 ? slot.d_scanSums : nullptr, cnt);
}

// Crossing lists, step 1 (mi_list_offsets_device): d_incl[i] = the crossings of rays 0 .. i, i.e. the caller's offsets from their
// second entry on. The count walk (list_count_kernel: count_crossings, builds picked as launchCountQuery picks them) writes the
// counts as 64 bits, scanOffsets sums them in place.
void launchListOffsets(mi_scene& S, const mi_ray* d_rays, uint64_t* d_incl, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_list_offsets", "rays", n, stream, [&](LaunchSlot& slot, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<true, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((list_count_kernel<decltype(b)::stats, decltype(b)::dbl>), grid, block, 0, stream, dsv, d_rays, d_incl, cnt);
    });
    HIP_CHECK(hipGetLastError());
    scanOffsets(slot, d_incl, cnt, stream);
  });
}

// Crossing lists, step 2 (mi_list_fill_device): list_fill_kernel, one thread per ray (list_kernels.hpp). rayBase: the index of the
// launch's first ray in the caller's numbering (the host entry's batches). Builds as launchCountQuery.
void launchListFill(mi_scene& S, const mi_ray* d_rays, const uint64_t* d_offsets, mi_crossing* d_hits, size_t capacity, uint32_t rayBase, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_list_fill", "rays", n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<true, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((list_fill_kernel<decltype(b)::stats, decltype(b)::dbl>), grid, block, 0, stream, dsv, d_rays, d_offsets, d_hits, (uint64_t)capacity, rayBase, cnt);
    });
  });
}

// Neighbour lists, step 1 (mi_near_offsets_device): d_incl[i] = the neighbours of points 0 .. i. near_count_kernel
// (near_kernels.hpp) writes the counts as 64 bits, scanOffsets sums them. full_stats picks the instrumented build; no other
// option applies.
void launchNearOffsets(mi_scene& S, const mi_point* d_points, uint64_t* d_incl, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_near_offsets", "points", n, stream, [&](LaunchSlot& slot, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL(near_count_kernel<decltype(b)::stats>, grid, block, 0, stream, dsv, d_points, d_incl, cnt);
    });
    HIP_CHECK(hipGetLastError());
    scanOffsets(slot, d_incl, cnt, stream);
  });
}

// Neighbour lists, step 2 (mi_near_fill_device): near_fill_kernel, one thread per point (near_kernels.hpp). pointBase: the index of
// the launch's first point in the caller's numbering (the host entry's batches).
void launchNearFill(mi_scene& S, const mi_point* d_points, const uint64_t* d_offsets, mi_neighbour* d_hits, size_t capacity, uint32_t pointBase, size_t n, hipStream_t stream) {
  launchFrame(S, "mi_near_fill", "points", n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL(near_fill_kernel<decltype(b)::stats>, grid, block, 0, stream, dsv, d_points, d_offsets, d_hits, (uint64_t)capacity, pointBase, cnt);
    });
  });
}

// The touch families, each by its Q (touch_kernels.hpp): the one list there is. What must hold of all of them is folded over it.
template <class... Q>
struct TouchList {
  static constexpr bool oneKindNumbering = (((int)Q::kAny == (int)MI_BOX_ANY && (int)Q::kCount == (int)MI_BOX_COUNT) && ...);
  static constexpr size_t itemBytes = std::max({sizeof(typename Q::Item)...});
};
using TouchFamilies = TouchList<BoxTouch, TriTouch, OBoxTouch, CapsuleTouch, FrustumTouch>;
static_assert(TouchFamilies::oneKindNumbering, "every touch family numbers its kinds alike: ANY = 0, COUNT = 1");

// Touch queries, Q a family of TouchFamilies; the entry's name and the items' noun for what launchFrame refuses come from Q.
// full_stats picks the instrumented build; no other option applies.
// mi_X_query_device: whether a primitive touches each item (Q::kAny: n bytes) or how many do (Q::kCount: n uint32_t), one thread
// per item (touch_query_kernel).
template <class Q>
void launchTouchQuery(mi_scene& S, int kind, const typename Q::Item* d_items, void* d_out, size_t n, hipStream_t stream) {
  launchFrame(S, Q::kQuery, Q::kNoun, n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    withFlag(kind == Q::kCount, [&](auto count) { pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((touch_query_kernel<Q, decltype(count)::value, decltype(b)::stats>), grid, block, 0, stream, dsv, d_items, d_out, cnt);
    }); });
  });
}

// Touch lists, step 1 (mi_X_offsets_device): d_incl[i] = the primitives touching items 0 .. i.
// touch_count_kernel writes the counts as 64 bits, scanOffsets sums them.
template <class Q>
void launchTouchOffsets(mi_scene& S, const typename Q::Item* d_items, uint64_t* d_incl, size_t n, hipStream_t stream) {
  launchFrame(S, Q::kOffsets, Q::kNoun, n, stream, [&](LaunchSlot& slot, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((touch_count_kernel<Q, decltype(b)::stats>), grid, block, 0, stream, dsv, d_items, d_incl, cnt);
    });
    HIP_CHECK(hipGetLastError());
    scanOffsets(slot, d_incl, cnt, stream);
  });
}

// Touch lists, step 2 (mi_X_fill_device): touch_fill_kernel, one thread per item. itemBase: the
// index of the launch's first item in the caller's numbering (the host entry's batches).
template <class Q>
void launchTouchFill(mi_scene& S, const typename Q::Item* d_items, const uint64_t* d_offsets, typename Q::Record* d_hits, size_t capacity, uint32_t itemBase, size_t n, hipStream_t stream) {
  launchFrame(S, Q::kFill, Q::kNoun, n, stream, [&](LaunchSlot&, const DeviceScene& dsv, dim3 grid, dim3 block, uint32_t cnt) {
    pickBuild<false, false>(S.opt, [&](auto b) {
      hipLaunchKernelGGL((touch_fill_kernel<Q, decltype(b)::stats>), grid, block, 0, stream, dsv, d_items, d_offsets, d_hits, (uint64_t)capacity, itemBase, cnt);
    });
  });
}

// ------------------------------------------------------------------------------------------------------
// argument rules
// ------------------------------------------------------------------------------------------------------

// One buffer of an entry: it must not be null, and must sit at a multiple of `align` bytes (1: anywhere) - else `why`. align 0:
// this entry has no such buffer.
struct BufferRule { const void* p; size_t align; const char* why; };

constexpr const char* kBuffers16 = "buffers must be 16-byte aligned";
constexpr const char* kRays16 = "rays must be 16-byte aligned";
constexpr const char* kPoints16 = "points must be 16-byte aligned";
constexpr size_t kNoLimit = ~(size_t)0;      // (a host entry: its limit is per batch, hostBatch)

// The argument rules of every query entry, in the order the entries have always applied them: the scene, the kind (kindBad: the
// message of an unknown kind, null when the kind is fine or the entry has none), the direction of an inside test (dir: null when
// the entry has none or the caller takes the default - the triangle test shears by the smallest signed component: an axis
// direction divides by zero there), then n == 0, which is no error whatever the buffers, then the buffers - none null, then
// their alignments in turn - and the limit on n. Sets the thread's error text and returns true when a rule is broken; touches
// neither the scene nor a device.
bool queryArgsBad(const char* fn, const mi_scene* scene, const char* kindBad, const float* dir, size_t n, size_t limit, const char* noun, std::initializer_list<BufferRule> buffers) {
  std::string why;
  if (!scene) why = "null scene";
  else if (kindBad) why = kindBad;
  else if (dir && !(dir[0] != 0.f && dir[1] != 0.f && dir[2] != 0.f && std::fabs(dir[0]) < kInf && std::fabs(dir[1]) < kInf && std::fabs(dir[2]) < kInf))
    why = "a direction component is zero, NaN or infinite";
  else if (n == 0) return false;
  else {
    for (const BufferRule& b : buffers) if (b.align && !b.p) why = "null buffer";
    for (const BufferRule& b : buffers) if (why.empty() && b.align && (uintptr_t)b.p % b.align) why = b.why;
    if (why.empty() && n > limit) why = std::string("more ") + noun + " than one launch indexes (kMaxWorkItems)";
  }
  if (why.empty()) return false;
  g_err = std::string(fn) + ": " + why;
  return true;
}

// The rules of each family's entries; limit: kMaxWorkItems for a device entry, kNoLimit for a host entry.
bool rayQueryBad(const char* fn, const mi_scene* scene, int kind, const void* rays, const void* out, size_t n, size_t limit) {
  return queryArgsBad(fn, scene, kind != MI_QUERY_CLOSEST && kind != MI_QUERY_ANY ? "unknown query kind" : nullptr, nullptr, n, limit, "rays",
                      {{rays, 16, kBuffers16}, {out, 16, kBuffers16}});
}
bool pointQueryBad(const char* fn, const mi_scene* scene, int kind, const void* points, const void* out, size_t n, size_t limit) {
  return queryArgsBad(fn, scene, kind != MI_POINT_CLOSEST && kind != MI_POINT_WITHIN ? "unknown query kind" : nullptr, nullptr, n, limit, "points",
                      {{points, 16, kBuffers16}, {out, kind == MI_POINT_CLOSEST ? 16u : 1u, kBuffers16}});      // (the bytes of WITHIN lie anywhere)
}
bool countQueryBad(const char* fn, const mi_scene* scene, const void* rays, const void* counts, size_t n, size_t limit) {
  return queryArgsBad(fn, scene, nullptr, nullptr, n, limit, "rays", {{rays, 16, kRays16}, {counts, 4, "counts must be 4-byte aligned"}});
}
bool pointSignBad(const char* fn, const mi_scene* scene, int kind, const void* points, const void* out, const float* dir, size_t n, size_t limit) {
  return queryArgsBad(fn, scene, kind != MI_SIGN_INSIDE && kind != MI_SIGN_DISTANCE ? "unknown sign kind" : nullptr, dir, n, limit, "points",
                      {{points, 16, kBuffers16}, {out, kind == MI_SIGN_DISTANCE ? 16u : 1u, kBuffers16}});
}
// (the entries of the lists: `in` the rays, the points or a touch family's items - inAlign bytes aligned; hits: only the fill's)
bool listQueryBad(const char* fn, const mi_scene* scene, const char* noun, const char* inWhy, const void* in, const void* offsets, const void* hits, bool fill, size_t n, size_t limit,
                  size_t inAlign = 16) {
  return queryArgsBad(fn, scene, nullptr, nullptr, n, limit, noun,
                      {{in, inAlign, inWhy}, {offsets, 8, "offsets must be 8-byte aligned"}, {hits, fill ? 16u : 0u, "hits must be 16-byte aligned"}});
}
// (a touch family's entries: the unknown kind's message, the noun, the items' alignment and its message are Q's)
template <class Q>
bool touchQueryBad(const char* fn, const mi_scene* scene, int kind, const void* items, const void* out, size_t n, size_t limit) {
  return queryArgsBad(fn, scene, kind != Q::kAny && kind != Q::kCount ? Q::kKindBad : nullptr, nullptr, n, limit, Q::kNoun,
                      {{items, Q::kAlign, Q::kAlignBad}, {out, kind == Q::kCount ? 4u : 1u, "counts must be 4-byte aligned"}});      // (the bytes of ANY lie anywhere)
}
template <class Q>
bool touchListBad(const char* fn, const mi_scene* scene, const void* items, const void* offsets, const void* hits, bool fill, size_t n, size_t limit) {
  return listQueryBad(fn, scene, Q::kNoun, Q::kAlignBad, items, offsets, hits, fill, n, limit, Q::kAlign);
}

// The direction of an inside test: the caller's three floats or the default.
constexpr float kDefaultInsideDir[3] = {1.0f, 0.70710678f, 0.57735027f};
f3 insideDir(const float* dir) {
  const float* d = dir ? dir : kDefaultInsideDir;
  return mk(d[0], d[1], d[2]);
}

// ------------------------------------------------------------------------------------------------------
// host entries: the two-slot pipeline
// ------------------------------------------------------------------------------------------------------

// The batch size of a host entry (the host stream is cut into batches of mi_scene_set_ray_batch items: the work-index limit
// applies per batch), or 0 with the error text set when one launch cannot index a batch. n > 0.
size_t hostBatch(const char* fn, const char* noun, const mi_scene* scene, size_t n) {
  const size_t batch = (scene->rayBatch && scene->rayBatch < n) ? scene->rayBatch : n;
  if (batch <= kMaxWorkItems) return batch;
  g_err = std::string(fn) + ": more " + noun + " per batch than one launch indexes (kMaxWorkItems; see mi_scene_set_ray_batch)";
  return 0;
}

// The device buffers and streams of the pipeline's slots: kept by the scene between calls, regrown when a batch is larger than
// any before. A slot holds `batch` items in - sized for the largest item of any family, today the 96-byte frustum - and `batch`
// 32-byte records out: room for any of the results, or batch + 1 offsets. kQueryItemBytes sizes these input slots and nothing else.
constexpr size_t kQueryItemBytes = std::max({sizeof(mi_ray), sizeof(mi_point), TouchFamilies::itemBytes});
static_assert(kQueryItemBytes == 96, "the pipeline's input slots hold the largest item, mi_frustum");
void ensureQuerySlots(mi_scene* scene, size_t batch, int slots) {
  for (int i = 0; i < slots; ++i) {
    if (scene->qCap[i] < batch) {
      if (scene->d_qRays[i] || scene->d_qOut[i]) HIP_CHECK(hipDeviceSynchronize());
      for (void** p : {&scene->d_qRays[i], &scene->d_qOut[i]}) { if (*p) (void)hipFree(*p); *p = nullptr; }
      scene->qCap[i] = 0;
      HIP_CHECK(hipMalloc(&scene->d_qRays[i], batch * kQueryItemBytes));
      HIP_CHECK(hipMalloc(&scene->d_qOut[i], batch * sizeof(mi_query_hit)));
      scene->qCap[i] = batch;
    }
    if (!scene->pipeStream[i]) HIP_CHECK(hipStreamCreateWithFlags(&scene->pipeStream[i], hipStreamNonBlocking));
  }
}

// n items of inSize bytes in host memory through launch(d_in, d_out, cnt, stream), outSize bytes each back: batches through two
// slots, as mi_render - upload, query and download of batch b + 1 are enqueued on the other stream while batch b runs.
template <class Launch>
void pipelinedQuery(mi_scene* scene, const void* in, size_t inSize, void* out, size_t outSize, size_t n, size_t batch, const Launch& launch) {
  HIP_CHECK(hipSetDevice(scene->device));
  const size_t numBatches = (n + batch - 1) / batch;
  const int slots = numBatches > 1 ? 2 : 1;
  try {
    ensureQuerySlots(scene, batch, slots);
    for (size_t b = 0; b < numBatches; ++b) {
      const int i = (int)(b % slots);
      hipStream_t st = scene->pipeStream[i];
      const size_t first = b * batch, cnt = std::min(batch, n - first);
      HIP_CHECK(hipMemcpyAsync(scene->d_qRays[i], static_cast<const char*>(in) + first * inSize, cnt * inSize, hipMemcpyHostToDevice, st));
      launch(scene->d_qRays[i], scene->d_qOut[i], cnt, st);
      HIP_CHECK(hipMemcpyAsync(static_cast<char*>(out) + first * outSize, scene->d_qOut[i], cnt * outSize, hipMemcpyDeviceToHost, st));
    }
    for (int i = 0; i < slots; ++i) HIP_CHECK(hipStreamSynchronize(scene->pipeStream[i]));
  } catch (...) { (void)hipDeviceSynchronize(); throw; }
}

// mi_list_offsets, mi_near_offsets and the touch families' mi_X_offsets on host buffers: every batch's prefix sum starts at 0 on
// the device; what precedes the batch is added here, batch by batch.
template <class Launch>
void offsetsHost(mi_scene* scene, const void* in, size_t inSize, uint64_t* offsets, size_t n, size_t batch, const Launch& launch) {
  offsets[0] = 0;
  pipelinedQuery(scene, in, inSize, offsets + 1, sizeof(uint64_t), n, batch, launch);
  for (size_t first = batch; first < n; first += batch) {
    const uint64_t base = offsets[first];
    const size_t cnt = std::min(batch, n - first);
    for (size_t j = 1; j <= cnt; ++j) offsets[first + j] += base;
  }
}

// mi_list_fill, mi_near_fill and the touch families' mi_X_fill on host buffers (in: items of inSize bytes; hits: 16-byte records of
// any of the kinds;
// launch(d_in, d_offsets, d_hits, capacity, base, cnt, stream) enqueues one batch's fill): the pipeline's slots - the result buffer
// carries a batch's offsets in - plus a staging buffer of records per slot. A batch's segments are packed from 0 in the staging -
// the device sees offsets of its own, cut at `capacity` here already - and copied to where the caller's offsets put them: in one
// piece when the batch's offsets ascend (neighbouring segments then touch), item by item otherwise.
template <class Rec, class Launch>
void listFillHost(mi_scene* scene, const void* in, size_t inSize, const uint64_t* offsets, Rec* hits, size_t capacity, size_t n, size_t batch, const Launch& launch) {
  static_assert(sizeof(Rec) == 16, "the staging of the list fills holds 16-byte records of either kind");
  HIP_CHECK(hipSetDevice(scene->device));
  const size_t numBatches = (n + batch - 1) / batch;
  const int slots = numBatches > 1 ? 2 : 1;
  std::vector<uint64_t> local[2];
  std::vector<Rec> bounce;
  try {
    ensureQuerySlots(scene, batch, slots);
    for (size_t b = 0; b < numBatches; ++b) {
      const int i = (int)(b % slots);
      hipStream_t st = scene->pipeStream[i];
      if (b >= (size_t)slots) HIP_CHECK(hipStreamSynchronize(st));      // local[i] and the staging are free again
      const size_t first = b * batch, cnt = std::min(batch, n - first);
      std::vector<uint64_t>& loc = local[i];
      loc.resize(cnt + 1);
      loc[0] = 0;
      bool ascending = true;
      for (size_t j = 0; j < cnt; ++j) {
        const uint64_t lo = offsets[first + j], hi = offsets[first + j + 1];
        ascending = ascending && hi >= lo;
        loc[j + 1] = loc[j] + segment_len(lo, hi, capacity);
      }
      const size_t need = (size_t)loc[cnt];
      if (scene->listHitsCap[i] < need) {
        if (scene->d_listHits[i]) { (void)hipFree(scene->d_listHits[i]); scene->d_listHits[i] = nullptr; scene->listHitsCap[i] = 0; }
        HIP_CHECK(hipMalloc(&scene->d_listHits[i], need * sizeof(Rec)));
        scene->listHitsCap[i] = need;
      }
      Rec* staged = static_cast<Rec*>(scene->d_listHits[i]);
      HIP_CHECK(hipMemcpyAsync(scene->d_qRays[i], static_cast<const char*>(in) + first * inSize, cnt * inSize, hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(scene->d_qOut[i], loc.data(), (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      launch(scene->d_qRays[i], static_cast<const uint64_t*>(scene->d_qOut[i]), staged, need, (uint32_t)first, cnt, st);
      if (!need) continue;
      if (ascending) {
        HIP_CHECK(hipMemcpyAsync(hits + offsets[first], staged, need * sizeof(Rec), hipMemcpyDeviceToHost, st));
      } else {
        bounce.resize(need);
        HIP_CHECK(hipMemcpyAsync(bounce.data(), staged, need * sizeof(Rec), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (size_t j = 0; j < cnt; ++j) if (loc[j + 1] > loc[j]) std::memcpy(hits + offsets[first + j], bounce.data() + loc[j], (size_t)(loc[j + 1] - loc[j]) * sizeof(Rec));
      }
    }
    for (int i = 0; i < slots; ++i) HIP_CHECK(hipStreamSynchronize(scene->pipeStream[i]));
  } catch (...) { (void)hipDeviceSynchronize(); throw; }
}

// A device entry behind its argument rules: the scene's device, then the launch.
template <class Launch>
int deviceEntry(mi_scene* scene, const Launch& launch) {
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    launch();
  });
}

// The six entries of a touch family Q. fn: a device entry's name (the host entries' are Q::kQuery, Q::kOffsets, Q::kFill).
template <class Q>
int touchQueryDevice(const char* fn, mi_scene* scene, int kind, const void* d_items, void* d_out, size_t n, void* hip_stream) {
  if (touchQueryBad<Q>(fn, scene, kind, d_items, d_out, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchTouchQuery<Q>(*scene, kind, static_cast<const typename Q::Item*>(d_items), d_out, n, (hipStream_t)hip_stream); });
}

template <class Q>
int touchQueryHostEntry(mi_scene* scene, int kind, const typename Q::Item* items, void* out, size_t n) {
  if (touchQueryBad<Q>(Q::kQuery, scene, kind, items, out, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch(Q::kQuery, Q::kNoun, scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    pipelinedQuery(scene, items, sizeof(typename Q::Item), out, kind == Q::kAny ? 1 : sizeof(uint32_t), n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchTouchQuery<Q>(*scene, kind, static_cast<const typename Q::Item*>(d_in), d_out, cnt, st);
    });
  });
}

template <class Q>
int touchOffsetsDevice(const char* fn, mi_scene* scene, const void* d_items, uint64_t* d_offsets, size_t n, void* hip_stream) {
  if (touchListBad<Q>(fn, scene, d_items, d_offsets, nullptr, false, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] {
    HIP_CHECK(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), (hipStream_t)hip_stream));
    launchTouchOffsets<Q>(*scene, static_cast<const typename Q::Item*>(d_items), d_offsets + 1, n, (hipStream_t)hip_stream);
  });
}

template <class Q>
int touchFillDevice(const char* fn, mi_scene* scene, const void* d_items, const uint64_t* d_offsets, typename Q::Record* d_hits, size_t capacity, size_t n, void* hip_stream) {
  if (touchListBad<Q>(fn, scene, d_items, d_offsets, d_hits, true, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchTouchFill<Q>(*scene, static_cast<const typename Q::Item*>(d_items), d_offsets, d_hits, capacity, 0u, n, (hipStream_t)hip_stream); });
}

template <class Q>
int touchOffsetsHostEntry(mi_scene* scene, const typename Q::Item* items, uint64_t* offsets, size_t n) {
  if (touchListBad<Q>(Q::kOffsets, scene, items, offsets, nullptr, false, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch(Q::kOffsets, Q::kNoun, scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    offsetsHost(scene, items, sizeof(typename Q::Item), offsets, n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchTouchOffsets<Q>(*scene, static_cast<const typename Q::Item*>(d_in), static_cast<uint64_t*>(d_out), cnt, st);
    });
  });
}

template <class Q>
int touchFillHostEntry(mi_scene* scene, const typename Q::Item* items, const uint64_t* offsets, typename Q::Record* hits, size_t capacity, size_t n) {
  if (touchListBad<Q>(Q::kFill, scene, items, offsets, hits, true, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch(Q::kFill, Q::kNoun, scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    listFillHost(scene, items, sizeof(typename Q::Item), offsets, hits, capacity, n, batch,
                 [&](const void* d_in, const uint64_t* d_off, typename Q::Record* d_hits, size_t cap, uint32_t base, size_t cnt, hipStream_t st) {
      launchTouchFill<Q>(*scene, static_cast<const typename Q::Item*>(d_in), d_off, d_hits, cap, base, cnt, st);
    });
  });
}

}  // namespace

extern "C" {

int mi_query_device(mi_scene* scene, int kind, const void* d_rays, void* d_out, size_t n, void* hip_stream) {
  if (rayQueryBad("mi_query_device", scene, kind, d_rays, d_out, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchQuery(*scene, kind, static_cast<const mi_ray*>(d_rays), d_out, n, (hipStream_t)hip_stream); });
}

int mi_query(mi_scene* scene, int kind, const mi_ray* rays, void* out, size_t n) {
  if (rayQueryBad("mi_query", scene, kind, rays, out, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_query", "rays", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    pipelinedQuery(scene, rays, sizeof(mi_ray), out, kind == MI_QUERY_ANY ? 1 : sizeof(mi_query_hit), n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchQuery(*scene, kind, static_cast<const mi_ray*>(d_in), d_out, cnt, st);
    });
  });
}

int mi_point_query_device(mi_scene* scene, int kind, const void* d_points, void* d_out, size_t n, void* hip_stream) {
  if (pointQueryBad("mi_point_query_device", scene, kind, d_points, d_out, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchPointQuery(*scene, kind, static_cast<const mi_point*>(d_points), d_out, n, (hipStream_t)hip_stream); });
}

int mi_point_query(mi_scene* scene, int kind, const mi_point* points, void* out, size_t n) {
  if (pointQueryBad("mi_point_query", scene, kind, points, out, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_point_query", "points", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    pipelinedQuery(scene, points, sizeof(mi_point), out, kind == MI_POINT_WITHIN ? 1 : sizeof(mi_point_hit), n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchPointQuery(*scene, kind, static_cast<const mi_point*>(d_in), d_out, cnt, st);
    });
  });
}

int mi_count_query_device(mi_scene* scene, const void* d_rays, uint32_t* d_counts, size_t n, void* hip_stream) {
  if (countQueryBad("mi_count_query_device", scene, d_rays, d_counts, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchCountQuery(*scene, static_cast<const mi_ray*>(d_rays), d_counts, n, (hipStream_t)hip_stream); });
}

int mi_count_query(mi_scene* scene, const mi_ray* rays, uint32_t* counts, size_t n) {
  if (countQueryBad("mi_count_query", scene, rays, counts, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_count_query", "rays", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    pipelinedQuery(scene, rays, sizeof(mi_ray), counts, sizeof(uint32_t), n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchCountQuery(*scene, static_cast<const mi_ray*>(d_in), static_cast<uint32_t*>(d_out), cnt, st);
    });
  });
}

int mi_point_sign_device(mi_scene* scene, int kind, const void* d_points, void* d_out, const float dir[3], size_t n, void* hip_stream) {
  if (pointSignBad("mi_point_sign_device", scene, kind, d_points, d_out, dir, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchPointSign(*scene, kind, static_cast<const mi_point*>(d_points), d_out, insideDir(dir), n, (hipStream_t)hip_stream); });
}

int mi_point_sign(mi_scene* scene, int kind, const mi_point* points, void* out, const float dir[3], size_t n) {
  if (pointSignBad("mi_point_sign", scene, kind, points, out, dir, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_point_sign", "points", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    pipelinedQuery(scene, points, sizeof(mi_point), out, kind == MI_SIGN_INSIDE ? 1 : sizeof(mi_point_hit), n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchPointSign(*scene, kind, static_cast<const mi_point*>(d_in), d_out, insideDir(dir), cnt, st);
    });
  });
}

int mi_list_offsets_device(mi_scene* scene, const void* d_rays, uint64_t* d_offsets, size_t n, void* hip_stream) {
  if (listQueryBad("mi_list_offsets_device", scene, "rays", kRays16, d_rays, d_offsets, nullptr, false, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] {
    HIP_CHECK(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), (hipStream_t)hip_stream));
    launchListOffsets(*scene, static_cast<const mi_ray*>(d_rays), d_offsets + 1, n, (hipStream_t)hip_stream);
  });
}

int mi_list_fill_device(mi_scene* scene, const void* d_rays, const uint64_t* d_offsets, mi_crossing* d_hits, size_t capacity, size_t n, void* hip_stream) {
  if (listQueryBad("mi_list_fill_device", scene, "rays", kRays16, d_rays, d_offsets, d_hits, true, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchListFill(*scene, static_cast<const mi_ray*>(d_rays), d_offsets, d_hits, capacity, 0u, n, (hipStream_t)hip_stream); });
}

int mi_list_offsets(mi_scene* scene, const mi_ray* rays, uint64_t* offsets, size_t n) {
  if (listQueryBad("mi_list_offsets", scene, "rays", kRays16, rays, offsets, nullptr, false, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_list_offsets", "rays", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    offsetsHost(scene, rays, sizeof(mi_ray), offsets, n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchListOffsets(*scene, static_cast<const mi_ray*>(d_in), static_cast<uint64_t*>(d_out), cnt, st);
    });
  });
}

int mi_list_fill(mi_scene* scene, const mi_ray* rays, const uint64_t* offsets, mi_crossing* hits, size_t capacity, size_t n) {
  if (listQueryBad("mi_list_fill", scene, "rays", kRays16, rays, offsets, hits, true, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_list_fill", "rays", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    listFillHost(scene, rays, sizeof(mi_ray), offsets, hits, capacity, n, batch, [&](const void* d_in, const uint64_t* d_off, mi_crossing* d_hits, size_t cap, uint32_t base, size_t cnt, hipStream_t st) {
      launchListFill(*scene, static_cast<const mi_ray*>(d_in), d_off, d_hits, cap, base, cnt, st);
    });
  });
}

int mi_near_offsets_device(mi_scene* scene, const void* d_points, uint64_t* d_offsets, size_t n, void* hip_stream) {
  if (listQueryBad("mi_near_offsets_device", scene, "points", kPoints16, d_points, d_offsets, nullptr, false, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] {
    HIP_CHECK(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), (hipStream_t)hip_stream));
    launchNearOffsets(*scene, static_cast<const mi_point*>(d_points), d_offsets + 1, n, (hipStream_t)hip_stream);
  });
}

int mi_near_fill_device(mi_scene* scene, const void* d_points, const uint64_t* d_offsets, mi_neighbour* d_hits, size_t capacity, size_t n, void* hip_stream) {
  if (listQueryBad("mi_near_fill_device", scene, "points", kPoints16, d_points, d_offsets, d_hits, true, n, kMaxWorkItems)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  return deviceEntry(scene, [&] { launchNearFill(*scene, static_cast<const mi_point*>(d_points), d_offsets, d_hits, capacity, 0u, n, (hipStream_t)hip_stream); });
}

int mi_near_offsets(mi_scene* scene, const mi_point* points, uint64_t* offsets, size_t n) {
  if (listQueryBad("mi_near_offsets", scene, "points", kPoints16, points, offsets, nullptr, false, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_near_offsets", "points", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    offsetsHost(scene, points, sizeof(mi_point), offsets, n, batch, [&](void* d_in, void* d_out, size_t cnt, hipStream_t st) {
      launchNearOffsets(*scene, static_cast<const mi_point*>(d_in), static_cast<uint64_t*>(d_out), cnt, st);
    });
  });
}

int mi_near_fill(mi_scene* scene, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits, size_t capacity, size_t n) {
  if (listQueryBad("mi_near_fill", scene, "points", kPoints16, points, offsets, hits, true, n, kNoLimit)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  const size_t batch = hostBatch("mi_near_fill", "points", scene, n);
  if (!batch) return MI_ERR_INVALID_ARG;
  return guarded([&] {
    listFillHost(scene, points, sizeof(mi_point), offsets, hits, capacity, n, batch, [&](const void* d_in, const uint64_t* d_off, mi_neighbour* d_hits, size_t cap, uint32_t base, size_t cnt, hipStream_t st) {
      launchNearFill(*scene, static_cast<const mi_point*>(d_in), d_off, d_hits, cap, base, cnt, st);
    });
  });
}

// The touch families' entries: the bodies are the templates above, a family is one line.
#define MI_TOUCH_ENTRIES(X, Q)                                                                                                                              \
  int mi_##X##_query_device(mi_scene* scene, int kind, const void* d_items, void* d_out, size_t n, void* hip_stream) {                                      \
    return touchQueryDevice<Q>("mi_" #X "_query_device", scene, kind, d_items, d_out, n, hip_stream);                                                       \
  }                                                                                                                                                         \
  int mi_##X##_query(mi_scene* scene, int kind, const Q::Item* items, void* out, size_t n) { return touchQueryHostEntry<Q>(scene, kind, items, out, n); }   \
  int mi_##X##_offsets_device(mi_scene* scene, const void* d_items, uint64_t* d_offsets, size_t n, void* hip_stream) {                                      \
    return touchOffsetsDevice<Q>("mi_" #X "_offsets_device", scene, d_items, d_offsets, n, hip_stream);                                                     \
  }                                                                                                                                                         \
  int mi_##X##_fill_device(mi_scene* scene, const void* d_items, const uint64_t* d_offsets, Q::Record* d_hits, size_t capacity, size_t n, void* hip_stream) { \
    return touchFillDevice<Q>("mi_" #X "_fill_device", scene, d_items, d_offsets, d_hits, capacity, n, hip_stream);                                         \
  }                                                                                                                                                         \
  int mi_##X##_offsets(mi_scene* scene, const Q::Item* items, uint64_t* offsets, size_t n) { return touchOffsetsHostEntry<Q>(scene, items, offsets, n); }   \
  int mi_##X##_fill(mi_scene* scene, const Q::Item* items, const uint64_t* offsets, Q::Record* hits, size_t capacity, size_t n) {                           \
    return touchFillHostEntry<Q>(scene, items, offsets, hits, capacity, n);                                                                                 \
  }
MI_TOUCH_ENTRIES(box, BoxTouch)
MI_TOUCH_ENTRIES(tri, TriTouch)
MI_TOUCH_ENTRIES(obox, OBoxTouch)
MI_TOUCH_ENTRIES(capsule, CapsuleTouch)
MI_TOUCH_ENTRIES(frustum, FrustumTouch)
#undef MI_TOUCH_ENTRIES

}  // extern "C"
