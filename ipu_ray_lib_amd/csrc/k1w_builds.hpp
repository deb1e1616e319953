// k1w_builds.hpp — the builds of K1w (trace_wavefront.hpp path_trace_wavefront_kernel<B>) by name, and the one function that selects them.
// No HIP in here: the selection is a pure host function (csrc/host/k1w_select_check.cpp walks it, built with g++).
#pragma once

#include <cstdint>

namespace mi {

enum class K1wId : uint8_t { PlainBary, PlainLean, PlainRot, SlotsBary, SlotsLean, SlotsRot, HotBary, HotRot, Stats, StatsHot, DoubleFallback, DoubleFallbackStats, Fast,
                             Spec5, SpecStats4, Weights6, Weights5, TwoTurns, TwoTurnsSlots, Waves7, Waves5, Waves5Slots, LdsPrefix, LdsPrefixStats, Waves4,
                             PathPool /* trace_pool.hpp, its own launch code */, RefusedFast /* option fast has no NIF / instrumented build */ };
constexpr const char* kK1wNames[] = {"K1wPlainBary", "K1wPlainLean", "K1wPlainRot", "K1wSlotsBary", "K1wSlotsLean", "K1wSlotsRot", "K1wHotBary", "K1wHotRot", "K1wStats", "K1wStatsHot",
                                     "K1wDoubleFallback", "K1wDoubleFallbackStats", "K1wFast", "K1wSpec5", "K1wSpecStats4", "K1wWeights6", "K1wWeights5", "K1wTwoTurns", "K1wTwoTurnsSlots",
                                     "K1wWaves7", "K1wWaves5", "K1wWaves5Slots", "K1wLdsPrefix", "K1wLdsPrefixStats", "K1wWaves4", "path pool", "refused: fast"};
constexpr const char* k1w_name(K1wId id) { return kK1wNames[(int)id]; }

// What a build is compiled with: today's defaults; a build overrides only the fields it differs in. (B is the build itself, so that the
// derived properties read ITS fields and a profiler's kernel name reads path_trace_wavefront_kernel<mi::K1wPlainRot>.)
template <class B> struct K1wBase {
  static constexpr bool stats = false;       // the instrumented build: node / leaf counters, phase occupancy, shader cycles per phase
  static constexpr bool ldsNodes = false;    // one 1024-thread workgroup per unit shares an LDS copy of a preorder prefix of the shared node array (kernel 2)
  static constexpr int block = 256, waves = 4;      // threads of a workgroup; waves per SIMD the registers are bounded for
  // spec: a lane whose walk reaches a primitive whose box it hits does not wait for the LEAF turn: it notes the primitive
  // (pend1, found at node pend1Node) and walks on as if the test were going to leave the closest hit unchanged - which
  // is what the reference's walk does in that case. When the LEAF turn has run the test, either the guess was right
  // (no closer hit: the box tests made meanwhile used the right hit distance and stand) or the lane goes back to node
  // pend1Node + 1 with the new, closer hit and repeats the walk from there, exactly as the reference continues. A second
  // primitive found while the first is still pending makes the lane wait as before. Nothing is ever skipped or reordered
  // in what a path finally takes from the walk: only work that turns out to be unnecessary is added, in lanes that
  // would have idled.
  static constexpr bool spec = false;
  // slots: 0 = plain launches only (rgb in registers / partial sums), 1 = NIF launches only (slots), 2 = decided at run time
  // from ex.slotColor. fixedTune: the scheduling weights are the compile-time defaults (kDefaultTune) instead of the
  // `tune` argument. The default-path builds (slots 0 or 1, fixedTune) carry neither the other mode's
  // code nor the ten weights in scalar registers: no scalar spills (33 before), -2.5 % frame time.
  static constexpr int slots = 2;
  static constexpr bool fixedTune = false;
  // df: the reference's ALLOW_DOUBLE_FALLBACK=1 build of the triangle test (trace_kernels.hpp). fast: the tolerance tier
  // (scene option "fast"): the box test as three pairs of FMAs on (plane, 1/d, -o/d), the triangle test contracted, no
  // literal NaN-exact fallback - results within a stated tolerance of the exact tier's, not bit-identical.
  static constexpr bool df = false, fast = false;
  static constexpr bool merge = true;        // SHADE and GEN are served by ONE turn (false: two turns, the default kernel up to round 3)
  // bary = false (round 5): for scenes WITHOUT vertex normals. The barycentrics of the closest hit only ever feed the interpolated
  // normal (Mesh.hpp:115-120); a scene without vertex normals shades with the face normal, so the three products per primitive test,
  // the three selects of the closest-hit update and three registers of the walk are dead weight there. Bit-identical by construction
  // (nothing reads them); select_k1w picks it by the scene's hasNormals.
  static constexpr bool bary = true;
  static constexpr bool rot = false;         // primitive records are read pre-rotated for the cast's shear axis (GLeafRot): 18 selects per triangle test become 6
  static constexpr bool hot = false;         // walks the scene's private, hot-first copies and stages their first nodes in dynamic LDS (scene option "hot_nodes")
  // ---- what follows from the fields ----
  static constexpr bool firstInSetup = B::slots != 0 && B::merge && !B::spec && !B::fast && !B::ldsNodes && !B::df && !B::hot;      // (see the cast set-up of the merged SHADE / GEN turn)
  static constexpr bool phInNode = !B::spec;                    // a lane's phase is read off its node word (SPEC lanes wait for a primitive test while their node walks on)
  static constexpr bool coordsFromStream = B::waves >= 7;       // seven workgroups' LDS in a unit: 21 cold words, the pixel's (row, col) fetched again by every GEN
  // lastThrough (round 20): what only the hit record of a pixel's LAST sample reads - the last hit's leaf and distance, the normal carried from
  // bounce to bounce - is not kept in LDS for every sample; a lane on its pixel's last sample writes those fields of the record as they arise
  // (trace_wavefront.hpp). 18 cold words, not 23. ldsCounts: casts and paths are not counted per turn in registers; a lane that ends a path adds its
  // bounce count and 1 to two LDS words of its wave. The six-wave plain-render builds of the default form count that way (K1wPlain*, K1wHot*,
  // K1wFast); the HOT builds among them also write the last sample through - their staged prefix grows from 316 to 793 nodes for it. The
  // 256-thread builds have no prefix to grow and measured 1.4 % SLOWER with the write-through (K1wPlainRot, K1wFast; K1wFast also spills four
  // vector registers with it): they keep their 23 words. The NIF-slot builds, the instrumented and four-wave builds, the two-turn form and
  // K1wWaves5 / K1wWaves7 keep their words and their per-turn counts: they were not measured (profiles/r20_k1w_cold_state.txt).
  static constexpr bool ldsCounts = B::slots == 0 && B::waves == 6 && B::fixedTune && B::merge && !B::stats && !B::spec && !B::ldsNodes;
  static constexpr bool lastThrough = B::hot && B::ldsCounts;
  static constexpr uint32_t coldWords = B::lastThrough ? 18u : B::waves >= 7 ? 21u : 23u;
  static constexpr bool leafFrame = !B::bary && B::slots == 0;  // a diffuse bounce loads its tangent frame from the leaf's record
  static constexpr int minBlocksPerUnit = ((B::block == 256 || B::hot) && B::waves > 4) ? B::waves : 1;       // (of __launch_bounds__)
  static constexpr bool wellFormed = !B::hot || (B::merge && !B::spec && !B::fast && !B::ldsNodes && !B::df);   // HOT is a form of the default kernel's plain-render builds
};

// The default form: SHADE and GEN in one turn, 80 VGPRs without a spill, six waves per SIMD (profiles/r04_k1w_merged_turn_ab.txt), the default
// scheduling weights compiled in, one build for plain renders and one for NIF slots. A scene WITHOUT vertex normals takes the build that
// carries no barycentrics (option "lean_hit") and reads the primitive records pre-rotated (option "leaf_rot"); both default on, both exact (every
// byte the oracle's either way), the other settings kept for A/B. With vertex normals the pre-rotated form spills seven
// registers at 80 and loses 8 % (test_scene.dae: 292 against 271 ms per 1000 spp, profiles/r05_k1w_leaf_ab.txt): not built.
template <class B> struct K1wDefaultForm : K1wBase<B> { static constexpr int waves = 6, slots = 0; static constexpr bool fixedTune = true; };
struct K1wPlainBary : K1wDefaultForm<K1wPlainBary> { static constexpr K1wId id = K1wId::PlainBary; };
struct K1wPlainLean : K1wDefaultForm<K1wPlainLean> { static constexpr K1wId id = K1wId::PlainLean; static constexpr bool bary = false; };
struct K1wPlainRot : K1wDefaultForm<K1wPlainRot> { static constexpr K1wId id = K1wId::PlainRot; static constexpr bool bary = false, rot = true; };
struct K1wSlotsBary : K1wDefaultForm<K1wSlotsBary> { static constexpr K1wId id = K1wId::SlotsBary; static constexpr int slots = 1; };
struct K1wSlotsLean : K1wDefaultForm<K1wSlotsLean> { static constexpr K1wId id = K1wId::SlotsLean; static constexpr int slots = 1; static constexpr bool bary = false; };
struct K1wSlotsRot : K1wDefaultForm<K1wSlotsRot> { static constexpr K1wId id = K1wId::SlotsRot; static constexpr int slots = 1; static constexpr bool bary = false, rot = true; };
// ... with hot nodes (Lean has none). 768 threads: two workgroups per compute unit, six waves per SIMD - the larger the workgroup, the larger the prefix its copies of the cold state leave room for (with 23 cold words 256 x 6: 68 nodes, 512 x 3: 172, 768 x 2: 316; with today's 18 words 768 x 2: 793)
struct K1wHotBary : K1wDefaultForm<K1wHotBary> { static constexpr K1wId id = K1wId::HotBary; static constexpr int block = 768; static constexpr bool hot = true; };
struct K1wHotRot : K1wDefaultForm<K1wHotRot> { static constexpr K1wId id = K1wId::HotRot; static constexpr int block = 768; static constexpr bool bary = false, rot = true, hot = true; };
struct K1wFast : K1wDefaultForm<K1wFast> { static constexpr K1wId id = K1wId::Fast; static constexpr bool fast = true; };
// the instrumented builds (four waves, run-time weights, either kind of launch); StatsHot walks the private copy of every node: its counters are the reference's visits
struct K1wStats : K1wBase<K1wStats> { static constexpr K1wId id = K1wId::Stats; static constexpr bool stats = true; };
struct K1wStatsHot : K1wBase<K1wStatsHot> { static constexpr K1wId id = K1wId::StatsHot; static constexpr bool stats = true, hot = true; };
struct K1wDoubleFallback : K1wBase<K1wDoubleFallback> { static constexpr K1wId id = K1wId::DoubleFallback; static constexpr bool df = true; };
struct K1wDoubleFallbackStats : K1wBase<K1wDoubleFallbackStats> { static constexpr K1wId id = K1wId::DoubleFallbackStats; static constexpr bool stats = true, df = true; };
// the variants library only: kernel families that were measured and not made the default
struct K1wSpec5 : K1wBase<K1wSpec5> { static constexpr K1wId id = K1wId::Spec5; static constexpr int waves = 5; static constexpr bool spec = true; };
struct K1wSpecStats4 : K1wBase<K1wSpecStats4> { static constexpr K1wId id = K1wId::SpecStats4; static constexpr bool stats = true, spec = true; };
struct K1wWeights6 : K1wBase<K1wWeights6> { static constexpr K1wId id = K1wId::Weights6; static constexpr int waves = 6; };      // run-time weights (tune sweeps, knock-in probes): scalar spills, a few per cent slower
struct K1wWeights5 : K1wBase<K1wWeights5> { static constexpr K1wId id = K1wId::Weights5; static constexpr int waves = 5; };
struct K1wTwoTurns : K1wDefaultForm<K1wTwoTurns> { static constexpr K1wId id = K1wId::TwoTurns; static constexpr int waves = 5; static constexpr bool merge = false; };
struct K1wTwoTurnsSlots : K1wDefaultForm<K1wTwoTurnsSlots> { static constexpr K1wId id = K1wId::TwoTurnsSlots; static constexpr int waves = 5, slots = 1; static constexpr bool merge = false; };
struct K1wWaves7 : K1wDefaultForm<K1wWaves7> { static constexpr K1wId id = K1wId::Waves7; static constexpr int waves = 7; };      // 72 VGPRs, 21 words of LDS per lane
struct K1wWaves5 : K1wDefaultForm<K1wWaves5> { static constexpr K1wId id = K1wId::Waves5; static constexpr int waves = 5; };      // the 96-VGPR build of today's form
struct K1wWaves5Slots : K1wDefaultForm<K1wWaves5Slots> { static constexpr K1wId id = K1wId::Waves5Slots; static constexpr int waves = 5, slots = 1; };
struct K1wLdsPrefix : K1wBase<K1wLdsPrefix> { static constexpr K1wId id = K1wId::LdsPrefix; static constexpr bool ldsNodes = true; static constexpr int block = 1024; };
struct K1wLdsPrefixStats : K1wBase<K1wLdsPrefixStats> { static constexpr K1wId id = K1wId::LdsPrefixStats; static constexpr bool stats = true, ldsNodes = true; static constexpr int block = 1024; };
struct K1wWaves4 : K1wBase<K1wWaves4> { static constexpr K1wId id = K1wId::Waves4; };      // every default: four waves, run-time weights, either kind of launch

// The builds each library can select - and so instantiates (with_k1w): the shipped one, and what the variants library adds to it.
template <class... B> struct K1wList {};
using K1wShipped = K1wList<K1wPlainBary, K1wPlainLean, K1wPlainRot, K1wSlotsBary, K1wSlotsLean, K1wSlotsRot, K1wHotBary, K1wHotRot, K1wStats, K1wStatsHot, K1wDoubleFallback, K1wDoubleFallbackStats, K1wFast>;
using K1wVariantsOnly = K1wList<K1wSpec5, K1wSpecStats4, K1wWeights6, K1wWeights5, K1wTwoTurns, K1wTwoTurnsSlots, K1wWaves7, K1wWaves5, K1wWaves5Slots, K1wLdsPrefix, K1wLdsPrefixStats, K1wWaves4>;
template <class F, class... B> constexpr bool k1w_visit(K1wList<B...>, K1wId id, F&& f) { static_assert((B::wellFormed && ...), "HOT is a form of the default kernel's plain-render builds"); return ((id == B::id && (f(B{}), true)) || ...); }
// f(build) for the build `id` names, where the library has it (false: it has not - nothing select_k1w returns for that library)
template <bool VARIANTS, class F> constexpr bool with_k1w(K1wId id, F&& f) {
  if constexpr (VARIANTS) return k1w_visit(K1wShipped{}, id, f) || k1w_visit(K1wVariantsOnly{}, id, f);
  else return k1w_visit(K1wShipped{}, id, f);
}

// What the selection reads: the launch (instrumented or not, plain render or NIF slots), the scene, its options, the library.
struct K1wChoice {
  bool variants, stats, slots;
  bool hasNormals, rotLeaves, hasNodes;      // the scene: vertex normals, pre-rotated leaf records, a BVH that is not empty
  bool hotOn;                                // option hot_nodes is not 0 and the scene's private copies stand for the shared arrays (plain renders only take them)
  bool doubleFallback, fast, specLeaf, mergeTurns, leanHit, leafRot; int kernelChoice, wavesPerSimd;      // the options of those names
  bool defaultWeights, poolFits;             // option tune is kDefaultTune; the scene's spp / bounce limits are within the path pool's
};

// The one place that says which build a launch runs. First the two options that select arithmetic, then (variants library) the other
// kernel families in the order they have always taken precedence, then the default form by the scene's kind.
inline K1wId select_k1w(const K1wChoice& c) {
  using I = K1wId;
  const bool plain = !c.slots;
  if (c.doubleFallback) return c.stats ? I::DoubleFallbackStats : I::DoubleFallback;      // the 4-wave build with the binary64 edge functions compiled in
  if (c.fast) return (!plain || c.stats) ? I::RefusedFast : I::Fast;                      // (mi_scene_set_option refuses the other combinations it has no build for)
  const int waves = c.variants ? c.wavesPerSimd : 6;      // (the shipped library has one width)
  if (c.variants) {
    if (c.kernelChoice == 3 && c.poolFits) return I::PathPool;
    if (plain && c.kernelChoice == 2 && c.hasNodes) return c.stats ? I::LdsPrefixStats : I::LdsPrefix;      // (NIF launches of kernel 2 fall through to kernel 1)
    if (c.specLeaf) return c.stats ? I::SpecStats4 : I::Spec5;
    if (!c.stats && !c.defaultWeights) return waves == 6 ? I::Weights6 : I::Weights5;
    if (!c.stats && !c.mergeTurns) return plain ? I::TwoTurns : I::TwoTurnsSlots;
    if (!c.stats && waves == 7 && plain) return I::Waves7;
    if (!c.stats && waves == 5) return plain ? I::Waves5 : I::Waves5Slots;
  }
  const bool hot = c.hotOn && plain;
  if (c.stats) return hot ? I::StatsHot : I::Stats;
  if (waves != 6) return I::Waves4;      // option waves = 4 - and 7 with NIF slots, which has no build of its own
  const bool lean = c.leanHit && !c.hasNormals, rot = lean && c.leafRot && c.rotLeaves;
  if (rot) return hot ? I::HotRot : plain ? I::PlainRot : I::SlotsRot;
  if (lean) return plain ? I::PlainLean : I::SlotsLean;
  return hot ? I::HotBary : plain ? I::PlainBary : I::SlotsBary;
}

}  // namespace mi
