// raylib.hip — C ABI (include/mi_raylib.h) over the gfx950 kernels: scene validation + upload,
// kernel launches, counters, timing. This file is the whole device library (libmi_raylib.so).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mi_raylib.h"
#include "ray_math.h"
#include "trace_kernels.hpp"
#include "trace_wavefront.hpp"
#include "hot_order.hpp"
#include "query_kernels.hpp"         // ray queries: the one-thread-per-ray kernel and K4
#include "point_kernels.hpp"         // point queries: the nearest primitive of each given point
#include "count_kernels.hpp"         // crossing counts, inside tests and signed distance
#include "list_kernels.hpp"          // crossing lists: offsets and the sorted fill
#include "near_kernels.hpp"          // neighbour lists: every primitive within a point's radius, nearest first
#include "box_kernels.hpp"           // box queries: every primitive that touches a caller's box
#include "contact_kernels.hpp"       // triangle queries: every primitive that touches a caller's triangle
#include "obox_kernels.hpp"          // oriented-box queries: every primitive that touches a caller's rotated box (these eight: launched and entered in query_drivers.hpp, included below)
#include "capsule_kernels.hpp"       // capsule queries: every primitive within a radius of a caller's segment (these eight: launched and entered in query_drivers.hpp, included below)
#include "frustum_kernels.hpp"       // frustum queries: every primitive inside or touching the region six caller-supplied planes leave (these eight: launched and entered in query_drivers.hpp, included below)
#include "refit_kernels.hpp"         // geometry updates: the BVH refit and the record rewrite (mi_scene_update / mi_scene_update_device)
#include "rebuild_kernels.hpp"       // topology rebuild of a live scene: an LBVH from its current geometry (mi_scene_rebuild)
#include "pose_kernels.hpp"          // rigid poses: the posed geometry from a rest copy and one pose per geometry (mi_scene_set_poses*)
#include "canon_kernels.hpp"         // new contents for a live scene: the canonical primitive table on the device (mi_scene_set_geometry*)
#include "cost_kernels.hpp"          // the surface-area cost of the current tree (mi_scene_bvh_cost, option auto_rebuild)
#include "bvh_cost_host.hpp"         // its host twin: a scene whose nodes are still only on the host
#include <rocprim/device/device_radix_sort.hpp>   // the rebuild's three sorts (header-only, compiled for gfx950 with the rest of this file)
// MI_RAYLIB_VARIANTS=1 (libmi_raylib_variants.so, the test build): the kernel families that were built, measured and not
// made the default - LDS-staged nodes (kernel 2), the path pool (kernel 3), the speculative walk (spec), the 4-wave and
// the runtime-weights instantiations (waves, tune), the register-resident MLP kernel K3r (nif_shape r8 / r8s) - stay
// selectable and parity-tested there. The
// shipped library carries the default path, its instrumented build, the nested-loop kernel, the two arithmetic options and K3.
#ifndef MI_RAYLIB_VARIANTS
#define MI_RAYLIB_VARIANTS 0
#endif
#if MI_RAYLIB_VARIANTS
#include "trace_pool.hpp"
#include "nif_regs_kernel.hpp"      // K3r, the register-resident MLP kernel (round 4: correct, slower than K3; nif_shape r8 / r8s)
#endif
#include "nif_kernels.hpp"
#include "nif_asm_kernel.hpp"      // K3a, the hand-scheduled register-resident MLP kernel (nif_shape a8)
#include "scene_blob.hpp"

using namespace mi;

static_assert(sizeof(mi_trace_result) == 84, "TraceResult layout");
static_assert(sizeof(mi_hit_record) == 64, "HitRecord layout");
static_assert(sizeof(mi_ray) == 32, "Ray layout");
static_assert(sizeof(mi_bvh_node) == 24, "CompactBVH2Node layout");
static_assert(sizeof(mi_material) == 36, "Material layout");
static_assert(sizeof(mi_mesh_info) == 16 && sizeof(mi_geom_ref) == 4, "MeshInfo/GeomRef layout");
static_assert(offsetof(mi_trace_result, u) == 12 && offsetof(mi_trace_result, h) == 20, "TraceResult offsets");
static_assert(offsetof(mi_hit_record, prim_id) == 32 && offsetof(mi_hit_record, normal) == 36 &&
              offsetof(mi_hit_record, throughput) == 48 && offsetof(mi_hit_record, geom_id) == 60 &&
              offsetof(mi_hit_record, flags) == 62, "HitRecord offsets");
static_assert(sizeof(mi_query_hit) == 32 && offsetof(mi_query_hit, prim_id) == 4 && offsetof(mi_query_hit, geom_id) == 8 &&
              offsetof(mi_query_hit, flags) == 10 && offsetof(mi_query_hit, normal) == 12 && offsetof(mi_query_hit, b1) == 24 &&
              offsetof(mi_query_hit, b2) == 28, "mi_query_hit layout");
static_assert(sizeof(mi_point) == 16 && offsetof(mi_point, radius) == 12, "mi_point layout");
static_assert(sizeof(mi_point_hit) == 32 && offsetof(mi_point_hit, prim_id) == 4 && offsetof(mi_point_hit, geom_id) == 8 &&
              offsetof(mi_point_hit, flags) == 10 && offsetof(mi_point_hit, point) == 12 && offsetof(mi_point_hit, b1) == 24 &&
              offsetof(mi_point_hit, b2) == 28, "mi_point_hit layout");

namespace {

thread_local std::string g_err;

struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIP_CHECK(expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      throw DeviceError(std::string(#expr) + ": " + hipGetErrorString(_e));                  \
  } while (0)

template <class F>
int guarded(F&& f) {
  try { f(); g_err.clear(); return MI_OK; }
  catch (const ArgError& e) { g_err = e.what(); return MI_ERR_INVALID_ARG; }
  catch (const DeviceError& e) { g_err = e.what(); return MI_ERR_DEVICE; }
  catch (const std::exception& e) { g_err = e.what(); return MI_ERR_DEVICE; }
  // nothing crosses the C ABI (include/ipu_utils.hpp:590-595: an error becomes a status, never a crash): whatever else a
  // callback or a library below us throws is reported like a device error
  catch (...) { g_err = "unknown exception (not derived from std::exception)"; return MI_ERR_DEVICE; }
}

template <class T>
T* upload(const std::vector<T>& v) {
  if (v.empty()) return nullptr;
  T* d = nullptr;
  HIP_CHECK(hipMalloc(&d, v.size() * sizeof(T)));
  HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

const float* hostSinTable() {
  static const uint32_t bits[92] = {MI_SIN_TABLE_BITS};
  static float tbl[92];
  static bool init = false;
  if (!init) { memcpy(tbl, bits, sizeof tbl); init = true; }
  return tbl;
}

}  // namespace

// Kernel selection and tuning of ONE scene: defaults, overridden by the MI_RAYLIB_* environment variables as they
// stand when the scene is created (read once, into the scene) and by mi_scene_set_option afterwards. Nothing here is
// process-global: creating or tuning scene B never changes what scene A launches.
// Samples a NIF render traces per launch (option nif_spl; the default, memory permitting - ensureScratch). A launch of the persistent
// kernel cannot be shorter than its longest work unit - 64 samples of one pixel, ~14 ms for a pixel on config 5's mesh - and a
// 1440^2 launch of 128 samples is only ten units per lane: config 5's trace launches took 22 ms per 128 samples that way, 15 with 256
// per launch, 11 with 512 and no less with 768 or 1 024 (profiles/r05_config5_launch_ab.txt); 512 samples are 48 B x 512 per pixel, 51 GB
// of a 1440^2 frame's 288.
constexpr uint32_t kNifSplDefault = 512, kNifSplMax = 1024;
constexpr int kHotNodesAuto = -1;                 // option "hot_nodes" = auto: on, with as many nodes as fit, where the staged prefix takes kHotAutoShare of the tree's expected box tests
constexpr double kHotAutoShare = 0.9;             // (hot_order.hpp hot_prefix_share; the box scene: 0.96 and -2.4 % frame time, test_scene.dae: 0.76 and +2 % - profiles/r06_k1w_hot_nodes_ab.txt)
constexpr uint32_t kLdsPerCU = 160 * 1024, kLdsGranule = 1280;      // gfx950 hands LDS out in 320-dword granules; the occupancy query does not round
struct SceneOptions {
  bool fullStats = false;          // MI_RAYLIB_FULL_STATS / "full_stats": instrumented kernel variants (node/leaf counters, phase occupancy)
  WaveTune tune = kDefaultTune;
  int kernelChoice = 1;            // MI_RAYLIB_KERNEL / "kernel": 0 = nested-loop kernel, 1 = wavefront (global nodes); variants build: 2 = wavefront + LDS-staged nodes, 3 = path pool (trace_pool.hpp)
#if MI_RAYLIB_VARIANTS
  PoolTune poolTune;               // MI_RAYLIB_POOL_TUNE / "pool_tune": leafAt,burst,retireAt,refillMin,shadeW,genW[,dbl,maxExtra,leafThenNode,prio]
#endif
  uint32_t cus = 0;                // "cus": compute units the launch grids are sized for (0 = what the device reports)
  std::string why;                 // why the last set() returned false
  int poolWaves = 4;               // MI_RAYLIB_POOL_WAVES / "pool_waves": waves per workgroup of the path-pool kernel, 4 | 8 | 16 (400 | 800 | 1600 slots)
  int wavesPerSimd = 6;            // MI_RAYLIB_WAVES / "waves": 6 = the 80-VGPR build of the default kernel; variants build: 5 = the 96-VGPR build, 4 = the 4-wave build
  bool mergeTurns = true;          // "merge" (variants build): 0 = SHADE and GEN as two turns, five waves - the default kernel up to round 3
  bool specLeaf = false;           // MI_RAYLIB_SPEC / "spec": lanes walk on past ONE pending primitive test (trace_wavefront.hpp, SPEC)
  bool tiles = true;               // MI_RAYLIB_NO_TILES / "tiles": walk row-structured streams in 8x8 pixel tiles
  size_t segBudgetKb = (size_t)8 * 1024 * 1024;   // MI_RAYLIB_SEG_BUDGET_KB / "seg_budget_kb": partial-sum buffer budget per launch
  uint32_t nifSamplesPerLaunch = 0;               // MI_RAYLIB_NIF_SPL / "nif_spl": 0 = default (128, memory permitting)
  bool pin = true;                 // MI_RAYLIB_PIN / "pin": page-lock the caller's stream for the duration of mi_render
  uint32_t nifShape = 7;           // MI_RAYLIB_NIF_SHAPE / "nif_shape": 7 = auto (default: K3a where its generated body covers the network, else w6), 6 = a8 (K3a, nif_asm_kernel.hpp),
                                   // 0 = w6, 1 = t6, 2 = t4 (nif_mlp_kernel's workgroup shapes); 4 = r8, 5 = r8s (K3r, nif_regs_kernel.hpp: measured slower, selectable in the variants build)
  bool leafRot = true;             // "leaf_rot": scenes without vertex normals read primitive records pre-rotated for the cast's shear axis (GLeafRot: 18 selects per triangle test become 6; -2.4 %, profiles/r05_k1w_leaf_ab.txt)
  bool leanHit = true;             // "lean_hit": scenes without vertex normals run the default kernel's build that carries no barycentrics (BARY = false)
  bool leafFrame = true;           // "leaf_frame": scenes without vertex normals: a diffuse bounce off a triangle or disc loads its tangent frame from the leaf's record (GLeafFrame, leaf_frame.hpp); 0 = computed per hit
  bool coords = true;              // "coords": (pixel, segment) atoms read the pixel coordinates from a compact copy of the stream's (u, v)
  int nifOverlap = -1;             // "nif_overlap": NIF renders trace sample batch b + 1 beside the MLP of batch b (two slot sets, second stream): 1 | 0 | auto
                                   // (-1, the default: only beside nif_mlp_kernel, whose workgroups come and go - K3a / K3b hold every register of their
                                   // unit for the whole launch, nothing runs beside them, and the second slot set is memory better spent on longer launches)
  uint32_t nifTraceWgs = 0;        // "nif_trace_wgs": a NIF render's trace launch that runs beside the previous batch's MLP gets at most this many workgroups per
                                   // compute unit (0 = all that stay resident, the default: a cap of 1 paid 3 % while the trace launch queued behind its list
                                   // counter, and costs 0.7 % since it does not: profiles/r04_nif_overlap_ab.txt, r04_nif_trace_ab.txt)
  uint32_t nifSplit = 0;           // "nif_split": compute units a NIF render's trace launches of batches 1.. get for themselves (CU-masked streams: the MLP's
                                   // workgroups take every register of their unit, so a trace launch beside them otherwise only runs in their ramps and tails;
                                   // the MLP is power-limited and loses less than the units it gives up: DESIGN.md §6). 0 = no partition
  bool nifFirstTest = false;       // "nif_first_test": a NIF render's casts take their first box test in the turn that sets them up (k1w_builds.hpp firstInSetup) instead of
                                   // in a NODE turn. Measured neutral (config 5: NODE turns 11.0 -> 3.4 per 64 casts, SHADE turns 1.2 -> 2.1 at lower occupancy, frame +-0.05 %,
                                   // profiles/r05_config5_launch_ab.txt): off by default, kept for A/B; results are the same either way
  bool nifTiming = false;          // "nif_timing": HIP events round every MLP launch of a NIF render (mi_get_nif_timing)
  bool refitTiming = false;        // "refit_timing": HIP events round the passes of mi_scene_update* (mi_get_refit_timing)
  bool rebuildTiming = false;      // "rebuild_timing": HIP events round the passes of mi_scene_rebuild (mi_get_rebuild_timing)
  uint32_t nifGenerations = kNifGenerations;   // MI_RAYLIB_NIF_GENERATIONS / "nif_generations": MLP workgroups launched per resident slot (nif_launch_mlp; measurement knob)
  bool rootStart = true;           // MI_RAYLIB_NO_ROOT_START / "root_start": a cast whose origin lies strictly inside the root's box starts at node 1
  bool sayGrid = false;            // MI_RAYLIB_SAY_GRID / "say_grid": print every persistent launch's grid to stderr (what the runtime said stays resident)
  // the two options that select ARITHMETIC (every other option leaves every result bit alone):
  bool doubleFallback = false;     // "double_fallback": the reference's ALLOW_DOUBLE_FALLBACK=1 build (CMakeLists.txt:13,34-41; Mesh.cpp:38-51), bit-exact to the oracle in that mode
  bool fast = false;               // "fast": the tolerance tier (FMA box / triangle tests; plain path-trace renders of the default kernel only)
  int queryKernel = 0;             // "query_kernel": ray queries (mi_query*) run the one-thread-per-ray kernel (0, the default: measured faster, DESIGN.md §6 "K4") or K4 (1, query_kernels.hpp)
  QueryTune queryTune = kDefaultQueryTune;   // "query_tune": K4's scheduling weights leafAt,dbl,maxExtra,burst,keep8
  int hotNodes = kHotNodesAuto;    // "hot_nodes": plain renders of the default kernel walk K1w's private, hot-first copy of the BVH and stage this many of its
                                   // first nodes in LDS (clamped to what fits beside the cold state; trace_wavefront.hpp HOT). 0 = off: the shared arrays, today's launch; auto (the default): see kHotAutoShare
  double autoRebuild = 0.0;        // "auto_rebuild": 0 = off; a ratio R > 1: an applied update whose tree's cost estimate is above R x the baseline's runs
                                   // the rebuild before it returns (refitScene). No environment variable, as for the arithmetic options: replicas must decide alike

  // Every key takes values from a stated domain; anything else leaves the option as it was and returns false
  // (mi_scene_set_option then reports MI_ERR_INVALID_ARG, as include/mi_raylib.h promises).
  static bool flag01(const char* v, bool& out) {
    if ((v[0] != '0' && v[0] != '1') || v[1] != '\0') return false;
    out = v[0] == '1';
    return true;
  }
  static bool number(const char* v, unsigned long long lo, unsigned long long hi, unsigned long long& out) {
    if (!*v) return false;
    char* end = nullptr;
    const unsigned long long q = strtoull(v, &end, 10);
    if (!end || *end != '\0' || v[0] == '-' || q < lo || q > hi) return false;
    out = q;
    return true;
  }
  // "0", or a decimal ratio above 1 (finite; digits, a point, an exponent - nothing strtod would read as hex, inf or nan)
  static bool autoRebuildValue(const char* v, double& out) {
    if (!v || !*v) return false;
    if (!strcmp(v, "0")) { out = 0.0; return true; }
    for (const char* c = v; *c; ++c) if (!((*c >= '0' && *c <= '9') || *c == '.' || *c == 'e' || *c == 'E' || *c == '+' || *c == '-')) return false;
    char* end = nullptr;
    const double r = strtod(v, &end);
    if (!end || end == v || *end != '\0' || !(r > 1.0) || !std::isfinite(r)) return false;
    out = r;
    return true;
  }
  // what option fast has a build for: kernel 1, 6 waves, one SHADE / GEN turn, default weights, no spec
  bool defaultKernelOnly() const { return kernelChoice == 1 && !specLeaf && wavesPerSimd == 6 && mergeTurns && tune == kDefaultTune; }
  bool set(const std::string& key, const char* v) {
    why = "unknown option or bad value";
    if (!v) return false;
    unsigned long long q = 0;
    // (an instrumented launch, a NIF launch and the double_fallback build have no tolerance-tier kernel: the combination is
    // refused where it is asked for instead of rendering another tier than the scene reports)
    if (key == "full_stats") {
      bool b = fullStats;
      if (!flag01(v, b)) return false;
      if (b && fast) { why = "full_stats cannot be combined with fast (the tolerance tier has no instrumented build)"; return false; }
      fullStats = b; return true;
    }
#if MI_RAYLIB_VARIANTS
    // (the tolerance tier is a build of the default kernel only: while it is set, nothing that selects another kernel is accepted -
    // the same refusal, whichever of the two options comes first)
    if (fast && (key == "kernel" || key == "waves" || key == "spec" || key == "merge" || key == "tune")) {
      SceneOptions probe = *this; probe.fast = false;
      if (!probe.set(key, v)) { why = probe.why; return false; }
      if (!probe.defaultKernelOnly()) {
        why = "fast is a build of the default kernel only (kernel 1, 6 waves, one SHADE / GEN turn, default weights, no spec): clear fast first"; return false;
      }
      return true;      // (a default value: nothing to change)
    }
    if (key == "kernel") { if (!number(v, 0, 3, q)) return false; kernelChoice = (int)q; return true; }
    if (key == "pool_waves") { if (!number(v, 4, 16, q) || (q != 4 && q != 8 && q != 16)) return false; poolWaves = (int)q; return true; }
    if (key == "pool_tune") {
      unsigned a, b, c, d, e, f, db = 4, mx = 5, ln = 1, pr = 1;
      if (sscanf(v, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%u", &a, &b, &c, &d, &e, &f, &db, &mx, &ln, &pr) < 6) return false;
      poolTune = {a, b, c ? c : 1, d ? d : 1, e, f, db ? db : 65, mx, ln, pr};
      return true;
    }
    if (key == "waves") { if (!number(v, 4, 7, q)) return false; wavesPerSimd = (int)q; return true; }
    if (key == "spec") return flag01(v, specLeaf);
    if (key == "merge") return flag01(v, mergeTurns);
#else
    if (key == "kernel") {
      if (!number(v, 0, 3, q)) return false;
      if (q > 1) { why = "kernel 2 / 3 are not compiled into this library (the variants build, -DMI_RAYLIB_VARIANTS=1, has them)"; return false; }
      kernelChoice = (int)q; return true;
    }
    if (key == "pool_waves" || key == "pool_tune" || key == "tune") { why = "not compiled into this library (the variants build, -DMI_RAYLIB_VARIANTS=1, has it)"; return false; }
    if (key == "waves") { if (!number(v, 4, 7, q)) return false; if (q != 6) { why = "the 4-, 5- and 7-wave builds are not compiled into this library (variants build)"; return false; } return true; }
    if (key == "merge") { bool b = true; if (!flag01(v, b)) return false; if (!b) { why = "the two-turn form is not compiled into this library (variants build)"; return false; } return true; }
    if (key == "spec") { bool b = false; if (!flag01(v, b)) return false; if (b) { why = "the speculative walk is not compiled into this library (variants build)"; return false; } return true; }
#endif
    if (key == "cus") { if (!number(v, 0, 4096, q)) return false; cus = (uint32_t)q; return true; }
    if (key == "tiles") return flag01(v, tiles);
    if (key == "seg_budget_kb") { if (!number(v, 1, ~0ull >> 12, q)) return false; segBudgetKb = (size_t)q; return true; }
    if (key == "nif_spl") { if (!number(v, 0, kNifSplMax, q)) return false; nifSamplesPerLaunch = (uint32_t)q; return true; }
    if (key == "pin") return flag01(v, pin);
    if (key == "nif_timing") return flag01(v, nifTiming);
    if (key == "refit_timing") return flag01(v, refitTiming);
    if (key == "rebuild_timing") return flag01(v, rebuildTiming);
    if (key == "nif_generations") { if (!number(v, 1, 4096, q)) return false; nifGenerations = (uint32_t)q; return true; }
    if (key == "root_start") return flag01(v, rootStart);
    if (key == "say_grid") return flag01(v, sayGrid);
    if (key == "nif_overlap") { if (!strcmp(v, "auto")) { nifOverlap = -1; return true; } bool on = false; if (!flag01(v, on)) return false; nifOverlap = on ? 1 : 0; return true; }
    if (key == "nif_first_test") return flag01(v, nifFirstTest);
    if (key == "nif_split") { if (!number(v, 0, 1024, q)) return false; nifSplit = (uint32_t)q; return true; }
    if (key == "nif_trace_wgs") { if (!number(v, 0, 16, q)) return false; nifTraceWgs = (uint32_t)q; return true; }
    if (key == "coords") return flag01(v, coords);
    if (key == "query_kernel") { if (!number(v, 0, 1, q)) return false; queryKernel = (int)q; return true; }
    if (key == "query_tune") {      // leafAt,dbl,maxExtra,burst,keep8
      unsigned a, b, c, dd, e;
      char tail = 0;
      if (sscanf(v, "%u,%u,%u,%u,%u%c", &a, &b, &c, &dd, &e, &tail) != 5) return false;
      if (b == 0 || dd == 0 || e > 8 || c > 64) return false;
      queryTune = {a, b, c, dd, e};
      return true;
    }
    if (key == "lean_hit") return flag01(v, leanHit);
    if (key == "auto_rebuild") { if (!autoRebuildValue(v, autoRebuild)) { why = "auto_rebuild takes 0 (off) or a decimal ratio above 1"; return false; } return true; }
    if (key == "leaf_rot") return flag01(v, leafRot);
    if (key == "leaf_frame") return flag01(v, leafFrame);
    if (key == "hot_nodes") { if (!strcmp(v, "auto")) { hotNodes = kHotNodesAuto; return true; } if (!number(v, 0, 65535, q)) return false; hotNodes = (int)q; return true; }
    if (key == "double_fallback") {
      bool b = doubleFallback;
      if (!flag01(v, b)) return false;
      if (b && fast) { why = "double_fallback cannot be combined with fast"; return false; }
      doubleFallback = b; return true;
    }
    if (key == "fast") {
      bool b = fast;
      if (!flag01(v, b)) return false;
      if (b && (fullStats || doubleFallback)) { why = "fast cannot be combined with full_stats or double_fallback"; return false; }
#if MI_RAYLIB_VARIANTS
      if (b && !defaultKernelOnly()) { why = "fast is a build of the default kernel only (kernel 1, 6 waves, one SHADE / GEN turn, default weights, no spec)"; return false; }
#endif
      fast = b; return true;
    }
    if (key == "nif_shape") {
      const std::string s(v);
      if (s == "w6") nifShape = 0; else if (s == "t6") nifShape = 1; else if (s == "t4") nifShape = 2; else if (s == "a8") nifShape = 6; else if (s == "auto") nifShape = 7; else if (s == "b4") nifShape = 8;
#if MI_RAYLIB_VARIANTS
      else if (s == "r8") nifShape = 4; else if (s == "r8s") nifShape = 5;
#else
      else if (s == "r8" || s == "r8s") { why = "K3r (nif_shape r8 / r8s) is not compiled into this library (the variants build, -DMI_RAYLIB_VARIANTS=1, has it)"; return false; }
#endif
      else return false;
      return true;
    }
#if MI_RAYLIB_VARIANTS
    if (key == "tune") {      // leafAt,shadeAt,genAt[,burst,keep8,dbl,maxExtra,leafThenNode,prio,leafP,probe]
      unsigned a, b, c, dd = 48, k8 = 3, db = 4, mx = 6, ln = 1, pr = 1, lp = 40, pb = 0;
      if (sscanf(v, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u", &a, &b, &c, &dd, &k8, &db, &mx, &ln, &pr, &lp, &pb) < 3) return false;
      if (mx > 7 || pb > 3) return false;          // the spelled-out run of box tests has eight
      tune = {a, b, c, dd, k8, db ? db : 65, mx, ln, pr, lp ? lp : 1, pb};
      return true;
    }
#endif
    return false;
  }
  void fromEnvironment() {
    static const char* const map[][2] = {{"MI_RAYLIB_FULL_STATS", "full_stats"}, {"MI_RAYLIB_KERNEL", "kernel"}, {"MI_RAYLIB_WAVES", "waves"}, {"MI_RAYLIB_SPEC", "spec"},
                                         {"MI_RAYLIB_SEG_BUDGET_KB", "seg_budget_kb"}, {"MI_RAYLIB_NIF_SPL", "nif_spl"}, {"MI_RAYLIB_PIN", "pin"},
                                         {"MI_RAYLIB_NIF_SHAPE", "nif_shape"}, {"MI_RAYLIB_TUNE", "tune"},
                                         {"MI_RAYLIB_POOL_TUNE", "pool_tune"}, {"MI_RAYLIB_POOL_WAVES", "pool_waves"}, {"MI_RAYLIB_CUS", "cus"},
                                         {"MI_RAYLIB_NIF_OVERLAP", "nif_overlap"}, {"MI_RAYLIB_COORDS", "coords"},
                                         {"MI_RAYLIB_NIF_TRACE_WGS", "nif_trace_wgs"}, {"MI_RAYLIB_NIF_SPLIT", "nif_split"}, {"MI_RAYLIB_NIF_GENERATIONS", "nif_generations"},
                                         {"MI_RAYLIB_HOT_NODES", "hot_nodes"}, {"MI_RAYLIB_LEAF_FRAME", "leaf_frame"}};
    // (an unparsable environment value is ignored: the option keeps its default. The two options that select ARITHMETIC,
    // double_fallback and fast, are deliberately not in this list: a process that says "bit-exact" must not change tier
    // because of a variable somebody exported)
    for (const auto& m : map) if (const char* e = getenv(m[0])) (void)set(m[1], e);
    if (getenv("MI_RAYLIB_NO_TILES")) tiles = false;
    if (getenv("MI_RAYLIB_NO_ROOT_START")) rootStart = false;
    if (getenv("MI_RAYLIB_SAY_GRID")) sayGrid = true;
  }
};

// What one in-flight path-trace launch owns besides the ray stream: its work counter and the partial-sum buffer of
// segmented pixels. One per HIP stream the scene has been rendered on, so launches of one scene that are enqueued on
// different streams (mi_render's two pipeline slots, or a caller's own streams through mi_render_device) never share
// them. Renders with a NIF environment additionally share the scene's slot scratch and are therefore chained with an
// event (nifDone): they may be enqueued on any streams but execute one after the other.
struct LaunchSlot {
  hipStream_t stream = nullptr;
  uint32_t* d_workCounter = nullptr;
  float* d_segPart = nullptr; size_t segPartFloats = 0;     // [segments][n][3]
  float2* d_coords = nullptr; size_t coordsCap = 0;         // the stream's pixel coordinates, compact (WaveExtras::coords)
  uint32_t* d_poolScratch = nullptr; size_t poolScratchWords = 0;   // kernel 3 (variants build): [PG_WORDS][slots of the grid]
  hipEvent_t lastWork = nullptr;                              // recorded behind everything the scene enqueued on `stream` (launchRender): what ~mi_scene waits for
  uint64_t* d_scanSums = nullptr; size_t scanSumsCap = 0;     // crossing and neighbour lists (scanOffsets): the tile sums of the prefix sum
};

struct mi_scene {
  int device = 0;
  int numCUs = 256;
  mi_scene_desc params{};            // scalar parameters only (pointers nulled)
  DeviceScene ds{};
  SceneOptions opt;
  std::vector<void*> allocations;
  unsigned long long* d_counters = nullptr;
  std::vector<LaunchSlot> slots;
  std::map<const void*, int> residentPerCU;      // workgroups of a kernel that stay resident on one compute unit (hipOccupancyMaxActiveBlocksPerMultiprocessor), asked once per kernel
  uint32_t cus() const { return opt.cus ? opt.cus : (uint32_t)numCUs; }
  // (auto: beside nif_mlp_kernel, and whenever the trace launches are given compute units of their own - option nif_split)
  bool nifOverlapOn() const { return opt.nifOverlap < 0 ? (opt.nifSplit > 0 || !((opt.nifShape >= 6 && opt.nifShape <= 8) && nif_asm_covers(nif.regs))) : opt.nifOverlap != 0; }
  // the scene as one launch sees it: option "root_start" decides whether the walk may start below the root
  // ... and option "leaf_frame" whether a scene without vertex normals shows its per-leaf frame records (null: every frame is computed)
  DeviceScene view() const { DeviceScene v = ds; if (!opt.rootStart) v.rootInterior = 0; if (!opt.leafFrame && !v.hasNormals) v.leafNormalsOrFrames = nullptr; return v; }
  // K1w's private copies of the walk's arrays in hot-first order (option "hot_nodes"; hot_order.hpp), made at create from the
  // arrays as uploaded. Everything that changes the shared arrays on the device - a refit, a rebuild, new contents - takes its
  // mutable reference to them from touchArrays(), which retires the copies: from then on the scene launches today's kernel on
  // the shared arrays (the copies are not regenerated on the device).
  // Two of them: `hot` holds every node - the instrumented build walks it and counts the reference's visits -, `thin` the collapsed tree
  // (hot_order.hpp: interior nodes whose box test decides nothing taken out of the walk), which the plain HOT builds walk, and behind it,
  // in the same arrays, every node once more: the region a cast on the literal box test starts in (exactBase; thinNodes = the collapsed
  // tree's own count, what the staged prefix and option auto go by).
  struct HotCopy { const GNode* nodes = nullptr; const GLeaf* leaves = nullptr; const GLeafRot* rot = nullptr; const float* leafNormals = nullptr; bool valid = false;
                   uint32_t numNodes = 0, thinNodes = 0, exactBase = 0;
                   std::vector<double> share; } hot, thin;      // share[k - 1]: what the first k nodes take of the tree's expected box tests (hot_prefix_share)
  DeviceScene hotView(const HotCopy& c) const { DeviceScene v = view(); v.nodes = c.nodes; v.numNodes = c.numNodes; v.exactBase = c.exactBase; v.leaves = c.leaves; v.leavesRot = c.rot; if (v.hasNormals || opt.leafFrame) v.leafNormalsOrFrames = c.leafNormals; return v; }
  DeviceScene& touchArrays() { hot.valid = false; thin.valid = false; return ds; }
  // gives a retired copy's buffers back (hipFree waits for the work that may still read them); called where an update has been applied
  void freeRetiredHot() {
    if (hot.valid || thin.valid) return;
    for (const HotCopy* c : {&hot, &thin})
      for (const void* p : {(const void*)c->nodes, (const void*)c->leaves, (const void*)c->rot, (const void*)c->leafNormals}) release(p);
    hot = HotCopy{};
    thin = HotCopy{};
  }
  bool hotRoomSaid = false;
  // the dynamic LDS (bytes, a multiple of a node) a HOT build may take per workgroup without losing a resident workgroup per compute unit
  std::map<const void*, uint32_t> hotRoomOf;
  uint32_t hotRoom(const void* kern, int threads) {
    auto it = hotRoomOf.find(kern);
    if (it != hotRoomOf.end()) return it->second;
    hipFuncAttributes fa{};
    int nb0 = 0;
    uint32_t room = 0;
    if (hipFuncGetAttributes(&fa, kern) == hipSuccess && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb0, kern, threads, 0) == hipSuccess && nb0 > 0) {
      long bytes = ((long)(kLdsPerCU / (uint32_t)nb0 / kLdsGranule * kLdsGranule) - (long)fa.sharedSizeBytes) & ~31L;
      for (; bytes >= 32; bytes -= 256) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, (size_t)bytes) == hipSuccess && nb >= nb0) break;
      }
      if (bytes >= 32) room = (uint32_t)bytes;
    }
    (void)hipGetLastError();
    if (room && hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)room) != hipSuccess) { (void)hipGetLastError(); room = 0; }
    if (!room && !hotRoomSaid) {      // (said once per scene: the renders are right either way, but not the ones the option asked for)
      hotRoomSaid = true;
      fprintf(stderr, "mi_raylib: option hot_nodes: the runtime leaves no LDS for hot nodes beside a %d-thread workgroup's own; rendering from the shared arrays\n", threads);
    }
    hotRoomOf.emplace(kern, room);
    return room;
  }
  uint32_t residentBlocks(const void* kern, int threads, size_t ldsBytes) {
    auto it = residentPerCU.find(kern);
    if (it == residentPerCU.end()) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, ldsBytes) != hipSuccess || nb <= 0) { (void)hipGetLastError(); nb = 8; }
      it = residentPerCU.emplace(kern, nb).first;
    }
    return (uint32_t)it->second;
  }
  bool poolAttrSet[2][3] = {{false, false, false}, {false, false, false}};
  bool ldsAttrSet[2] = {false, false};   // kernel 2's dynamic-LDS opt-in (plain / instrumented build), per scene and so per device: function attributes are per device
  hipEvent_t nifDone = nullptr; bool nifPending = false;
  // mi_render's pipeline: two device batch buffers and two streams, kept between calls
  mi_trace_result* d_batch[2] = {nullptr, nullptr}; size_t batchCap[2] = {0, 0};
  hipStream_t pipeStream[2] = {nullptr, nullptr};
  double traceTimeSecs = 0.0;
  float hdriRotationDegrees = 0.f;
  size_t maxNifBatch = 0;
  size_t rayBatch = 0;               // rays per mi_render batch (0 = the whole stream in one batch)
  // mi_query's pipeline: two device ray / result buffers, kept between calls (on the same two streams as mi_render's)
  void* d_qRays[2] = {nullptr, nullptr}; void* d_qOut[2] = {nullptr, nullptr}; size_t qCap[2] = {0, 0};
  NifDevice nif;
  // scratch for the per-sample NIF loop
  // NIF renders: per-(sample, pixel) slots of one launch. TWO sets, so that the trace launch of sample batch b + 1 (into the
  // other set, on the render's stream) runs beside the MLP + accumulate pass of batch b (on nifAux): the MLP fills every CU
  // but its workgroups come and go in generations, and the traversal kernel takes the gaps (launch ramps and tails).
  struct NifSlots {
    float* u = nullptr; float* v = nullptr; float* bgr = nullptr; float* color = nullptr; float* tp = nullptr;
    uint32_t* index = nullptr; uint32_t* count = nullptr;
    hipEvent_t traced = nullptr, done = nullptr; bool donePending = false;
  } nifSlots[2];
  hipStream_t nifAux = nullptr;
  hipStream_t debugStream = nullptr;      // mi_debug_launch_progress
  // option "nif_split": the same pair of streams with compute-unit masks (the first numCUs - x units / the last x; a mask's bit i is
  // unit i / XCDs of XCD i % XCDs, so any multiple of the XCD count splits every XCD alike). splitUnits = x they were made for.
  hipStream_t nifSplitMlp = nullptr, nifSplitTrace = nullptr;
  uint32_t splitUnits = 0; bool splitRefused = false;
  hipEvent_t splitFirst = nullptr;
  Rng* d_rng = nullptr; size_t scratchRays = 0;
  float* d_segTotal = nullptr;                                // sample-at-a-time NIF renders: sum of the finished segments, [n][3]
  uint32_t scratchSamples = 0;                                // samples per launch the slot buffers are sized for
  uint32_t scratchAsked = 0;                                  // the MI_RAYLIB_NIF_SPL value they were sized under (0 = default)
  bool scratchOneSet = false;                                 // two slot sets did not fit the memory budget: this render runs without the overlap
  std::vector<std::pair<hipEvent_t, hipEvent_t>> nifTimes;    // option "nif_timing": events round the MLP launches since the last mi_get_nif_timing
  // mi_scene_update: what a refit needs, kept on the HOST at create (the device holds only records derived from it), and the
  // device tables the first update builds (refitTables; a scene that is never updated allocates nothing for them)
  struct Refit {
    std::vector<mi_bvh_node> nodes;                           // the compact nodes at create: the scene's current ones until the first update or rebuild (live < 0),
                                                              // what the first update derives the tables below from; not read afterwards (the count is ds.numNodes).
                                                              // New contents (setGeometry) keep geometry and meshInfo (the poses' owners) and leave the other host vectors empty: only the counts below are read then
    bool tables = false; uint32_t levelCap = 0;               // tables: d_prims, d_order and the level starts describe the current topology (derived on the host by
                                                              // the first update, written by the device passes of every rebuild); levelCap: entries d_levelStart holds
    std::vector<uint32_t> matIds;                             // per geometry (a rebuild writes leaf records)
    std::vector<mi_geom_ref> geometry; std::vector<mi_mesh_info> meshInfo; std::vector<uint16_t> tris;
    std::vector<mi_vec3> verts; std::vector<mi_sphere> spheres; std::vector<mi_disc> discs;   // the geometry at create (-> d_verts ... at the first update)
    uint32_t numVerts = 0, numNormals = 0, numSpheres = 0, numDiscs = 0;
    bool ready = false;
    RefitPrim* d_prims = nullptr;                             // [node]: what its box is computed from
    uint32_t* d_order = nullptr;                              // node indices by height (leaves first)
    std::vector<uint32_t> levelStart; uint32_t* d_levelStart = nullptr;   // [height]: first entry of that height in d_order; [H + 1] = numNodes
    uint32_t topFirst = 0;                                    // heights topFirst .. H run in one workgroup (refit_top_kernel)
    RefitBox* d_boxes = nullptr;                              // float boxes (scratch)
    mi_bvh_node* d_cnodes[2] = {nullptr, nullptr}; int live = -1;   // compact nodes: the scene's current ones (live; -1 = nodes[]) and the scratch
    uint32_t* d_err = nullptr;                                // pass 1 / 2 error bits (1 << kBoxTooLarge, 1 << kBoxNotFinite)
    mi_vec3* d_verts = nullptr; mi_sphere* d_spheres = nullptr; mi_disc* d_discs = nullptr;   // the current geometry
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // option "refit_timing": round passes 1, 2 and 4
    double ms[3] = {0, 0, 0};                                 // the last update's {leaf, interior, write} pass times
  } refit;
  // mi_scene_rebuild: the canonical primitive table and the scratch of the passes (rebuild_kernels.hpp), built at the first
  // rebuild (rebuildTables; a scene that is never rebuilt allocates nothing for them)
  struct Rebuild {
    bool ready = false;
    uint32_t numPrims = 0;
    RebuildPrim* d_canon = nullptr;                           // [numPrims] the canonical table of the scene's contents
    uint32_t capPrims = 0;                                    // primitives the scratch below has room for (rebuildScratch: new contents reuse it while it fits)
    RefitBox* d_primBoxes = nullptr; RefitBox* d_parts = nullptr; RefitBox* d_sceneBox = nullptr;
    uint64_t* d_keys[2] = {nullptr, nullptr}; uint32_t* d_vals[2] = {nullptr, nullptr};        // the Morton sort's double buffers
    uint32_t* d_depth[2] = {nullptr, nullptr}; uint32_t* d_ids[2] = {nullptr, nullptr};        // the depth sort's
    uint2* d_child = nullptr; uint2* d_range = nullptr; uint32_t* d_parent = nullptr; uint8_t* d_swapped = nullptr; uint32_t* d_index = nullptr;
    uint32_t* d_levelStart = nullptr;                         // [kRebuildMaxDepth + 2]
    uint32_t* d_height = nullptr;                             // [2 P - 1] node heights, Karras numbering
    uint32_t* d_hvals[2] = {nullptr, nullptr};                // the height sort's values (the keys reuse d_keys: 8 P bytes hold 2 P - 1 words)
    uint32_t* d_heightStart = nullptr;                        // [kRebuildHeightSlots]
    void* d_sortTmp = nullptr; size_t sortTmpBytes = 0;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // option "rebuild_timing"
    double ms[6] = {0, 0, 0, 0, 0, 0};                        // the last rebuild's {boxes + keys, sort, hierarchy + depths, level boxes, preorder, tables + scatter}
  } rebuild;
  // mi_scene_set_poses*: the rest snapshot, the owner tables, the arrays the pose pass writes and the current poses, built at the
  // first pose call after create, an update, new contents or a bake (poseSnapshot; a scene that is never posed allocates nothing)
  struct Poses {
    bool allocated = false;                                   // the buffers below exist, sized for the scene's current counts
    bool snapshot = false;                                    // the rest arrays and the owner tables describe the rest geometry
    bool posed = false;                                       // d_poses holds the current poses (else every pose is the identity)
    mi_vec3* d_restVerts = nullptr; mi_vec3* d_restNormals = nullptr; mi_sphere* d_restSpheres = nullptr; mi_disc* d_restDiscs = nullptr;
    mi_vec3* d_outVerts = nullptr; mi_vec3* d_outNormals = nullptr; mi_sphere* d_outSpheres = nullptr; mi_disc* d_outDiscs = nullptr;
    uint16_t* d_vertOwner = nullptr; uint16_t* d_sphereOwner = nullptr; uint16_t* d_discOwner = nullptr;
    PoseFrame* d_frames = nullptr;                            // [G]
    mi_pose* d_poses = nullptr; mi_pose* d_staged = nullptr;  // [G] the current poses; the host entry's upload
    uint32_t* d_bad = nullptr;                                // {some pose is not valid, the first such pose}
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};           // option "refit_timing": round the pose pass and what follows it
    double ms[2] = {0, 0};                                    // the last pose call's {pose pass, everything after it}
    std::vector<void*> buffers() const {
      return {d_restVerts, d_restNormals, d_restSpheres, d_restDiscs, d_outVerts, d_outNormals, d_outSpheres, d_outDiscs, d_vertOwner, d_sphereOwner,
              d_discOwner, d_frames, d_poses, d_staged, d_bad};
    }
  } poses;
  // the live loop (refit every frame, rebuild when the tree has degraded): the cost pass's scratch, the policy's baseline, what happened
  struct Live {
    Cost2* d_cost = nullptr;                                  // slot 0 = {a_root, -}, slot 1 = the last level's one entry, then the levels before it, the first last
    double baseline = 0.0; bool baselineValid = false;        // the estimate the policy compares against (option auto_rebuild)
    uint64_t applied = 0, refused = 0, rebuilds = 0, autoRebuilds = 0, hostDerivations = 0, costEvals = 0, geometrySets = 0;
    uint32_t maxLeafDepth = 0;
  } live;

  ~mi_scene() {
    (void)hipSetDevice(device);
    // Nothing of this scene's may still be in flight when its buffers go: mi_render_device is asynchronous and the caller may
    // destroy the scene right behind it. The wait is for THIS scene's work only - the event every launchRender records behind
    // what it enqueued on its stream (work on nifAux is always joined back into that stream before the event) - so destroying a
    // scene does not wait for other scenes' or replicas' launches on the device. (The events are the scene's own: the caller's
    // stream may be gone by now. hipFree below synchronises on its own account in this runtime; correctness does not rest on it.)
    for (LaunchSlot& l : slots) if (l.lastWork) (void)hipEventSynchronize(l.lastWork);
    if (nifAux) (void)hipStreamSynchronize(nifAux);
    for (hipStream_t q : {nifSplitMlp, nifSplitTrace, debugStream}) if (q) (void)hipStreamSynchronize(q);
    for (void* p : allocations) (void)hipFree(p);
    if (d_rng) (void)hipFree(d_rng);
    freeNifSlots();
    for (NifSlots& q : nifSlots) { if (q.count) (void)hipFree(q.count); if (q.traced) (void)hipEventDestroy(q.traced); if (q.done) (void)hipEventDestroy(q.done); }
    if (nifAux) (void)hipStreamDestroy(nifAux);
    for (hipStream_t q : {nifSplitMlp, nifSplitTrace, debugStream}) if (q) (void)hipStreamDestroy(q);
    if (splitFirst) (void)hipEventDestroy(splitFirst);
    if (d_segTotal) (void)hipFree(d_segTotal);
    for (LaunchSlot& l : slots) { if (l.lastWork) (void)hipEventDestroy(l.lastWork); if (l.d_workCounter) (void)hipFree(l.d_workCounter); if (l.d_segPart) (void)hipFree(l.d_segPart); if (l.d_coords) (void)hipFree(l.d_coords); if (l.d_poolScratch) (void)hipFree(l.d_poolScratch); if (l.d_scanSums) (void)hipFree(l.d_scanSums); }
    for (int i = 0; i < 2; ++i) { if (d_qRays[i]) (void)hipFree(d_qRays[i]); if (d_qOut[i]) (void)hipFree(d_qOut[i]); if (d_listHits[i]) (void)hipFree(d_listHits[i]); }
    for (int i = 0; i < 2; ++i) { if (d_batch[i]) (void)hipFree(d_batch[i]); if (pipeStream[i]) (void)hipStreamDestroy(pipeStream[i]); }
    if (nifDone) (void)hipEventDestroy(nifDone);
    for (auto& e : nifTimes) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (hipEvent_t e : refit.ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : rebuild.ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : poses.ev) if (e) (void)hipEventDestroy(e);
    nif.release();
  }
  void freeNifSlots() {
    for (NifSlots& q : nifSlots) {
      for (float** p : {&q.u, &q.v, &q.bgr, &q.color, &q.tp}) { if (*p) (void)hipFree(*p); *p = nullptr; }
      if (q.index) (void)hipFree(q.index);
      q.index = nullptr;
    }
  }
  template <class T> T* keep(T* p) { if (p) allocations.push_back((void*)p); return p; }
  // gives a kept buffer up before the scene goes (new contents replace the old ones': setGeometry)
  void release(const void* p) {
    if (!p) return;
    auto it = std::find(allocations.begin(), allocations.end(), (void*)p);
    if (it == allocations.end()) return;
    allocations.erase(it);
    (void)hipFree((void*)p);
  }
  // the launch slot of a stream (created on first use; a scene is thread-compatible, not thread-safe)
  LaunchSlot& slotFor(hipStream_t stream);
  // mi_list_fill's and mi_near_fill's staging of a batch's 16-byte records, one per pipeline slot, grown on demand (last: nothing before it moves)
  void* d_listHits[2] = {nullptr, nullptr}; size_t listHitsCap[2] = {0, 0};
};

LaunchSlot& mi_scene::slotFor(hipStream_t stream) {
  for (LaunchSlot& l : slots) if (l.stream == stream) return l;
  LaunchSlot l;
  l.stream = stream;
  HIP_CHECK(hipMalloc(&l.d_workCounter, sizeof(uint32_t)));
  if (hipEventCreateWithFlags(&l.lastWork, hipEventDisableTiming) != hipSuccess) { (void)hipFree(l.d_workCounter); throw DeviceError("hipEventCreateWithFlags failed"); }
  slots.push_back(l);
  return slots.back();
}

namespace {

// Validate everything the kernels will index with, then build the device arrays.
void buildDeviceScene(mi_scene& S, const mi_scene_desc& d) {
  auto need = [](bool ok, const char* what) { if (!ok) throw ArgError(std::string("mi_scene_create: ") + what); };
  need(d.num_nodes == 0 || d.bvh_nodes, "bvh_nodes is null");
  need(d.num_nodes < (kLeafFlag >> 5), "more than 2^26 - 1 BVH nodes");
  need(d.num_geometry == 0 || d.geometry, "geometry is null");
  need(d.num_geometry <= 0xFFFF, "more than 65535 geometries (geomID is 16 bit)");
  need(d.num_mat_ids >= d.num_geometry, "All primitives must be assigned a material.");
  need(d.num_mat_ids == 0 || d.mat_ids, "mat_ids is null");
  need(d.num_materials == 0 || d.materials, "materials is null");
  need(d.num_meshes == 0 || (d.mesh_info && d.mesh_tris && d.mesh_verts), "mesh arrays are null");
  need(d.num_normals == 0 || (d.num_normals == d.num_verts && d.mesh_normals), "normals must be absent or one per vertex");
  need(d.num_spheres == 0 || d.spheres, "spheres is null");
  need(d.num_discs == 0 || d.discs, "discs is null");
  need(d.image_width > 0.f && d.image_height > 0.f, "image size must be positive");
  for (uint32_t g = 0; g < d.num_geometry; ++g) {
    const mi_geom_ref& r = d.geometry[g];
    need(r.type <= 2, "unknown geometry type");
    need(r.index < (r.type == 0 ? d.num_meshes : r.type == 1 ? d.num_spheres : d.num_discs), "geometry index out of range");
    need(d.mat_ids[g] < d.num_materials, "material index out of range");
  }
  for (uint32_t m = 0; m < d.num_meshes; ++m) {
    const mi_mesh_info& mi_ = d.mesh_info[m];
    need((uint64_t)mi_.first_index + mi_.num_triangles <= d.num_tris, "mesh triangle range out of bounds");
    need((uint64_t)mi_.first_vertex + mi_.num_vertices <= d.num_verts, "mesh vertex range out of bounds");
    for (uint32_t t = 0; t < 3 * mi_.num_triangles; ++t)
      need(d.mesh_tris[3 * (size_t)mi_.first_index + t] < mi_.num_vertices, "triangle vertex index out of range");
  }

  // Node array: box widened to six floats, link := next(i), the node that follows i's subtree in preorder (interior
  // nodes: instead of the second child's index; leaves: beside their primitive). Also checks that the array really is a
  // preorder BVH2 (first child adjacent, second child after it, every node reached).
  // (With `next` explicit the device array only has to keep "first child = i + 1". Laying the chains of first children
  // out by falling surface area puts 93 % of the box scene's node visits into the first 128 of its 8 069 nodes - in
  // preorder the first 1 024 take 38 % - and serving that prefix from LDS was measured: 4.5 % SLOWER than the L1 that
  // already holds it; the array stays in preorder.)
  const uint32_t N = d.num_nodes;
  std::vector<GNode> nodes(N);
  std::vector<uint32_t> skip(N);
  // leaves[] is indexed by NODE: a leaf node's primitive record sits at the node's own index (interior nodes leave a zero
  // record behind), so the walk never has to carry an index from the box test to the primitive test (trace_wavefront.hpp)
  std::vector<GLeaf> leaves(N);
  memset(leaves.data(), 0, leaves.size() * sizeof(GLeaf));
  std::vector<uint8_t> isLeafNode(N, 0);
  std::vector<uint32_t> geomFirstVertex(d.num_geometry, 0);
  for (uint32_t g = 0; g < d.num_geometry; ++g)
    if (d.geometry[g].type == 0) geomFirstVertex[g] = d.mesh_info[d.geometry[g].index].first_vertex;
  for (uint32_t i = N; i-- > 0;) {
    const mi_bvh_node& n = d.bvh_nodes[i];
    if (n.geom_id != MI_INVALID_GEOM) skip[i] = i + 1;
    else {
      const uint32_t second = n.prim_or_second_child;
      need(i + 1 < N && second > i + 1 && second < N, "BVH is not a depth-first BVH2 (bad second child index)");
      need(skip[i + 1] == second, "BVH is not in depth-first order (first child's subtree must end at the second child)");
      skip[i] = skip[second];
    }
  }
  need(N == 0 || skip[0] == N, "BVH root does not span the node array");
  for (uint32_t i = 0; i < N; ++i) {
    const mi_bvh_node& n = d.bvh_nodes[i];
    // the box test's fast form assumes finite slab products (trace_wavefront.hpp): a NaN / inf box is a malformed scene
    need(std::isfinite(n.min_x) && std::isfinite(n.min_y) && std::isfinite(n.min_z), "BVH node bounds are not finite");
    need((n.dx & 0x7C00u) != 0x7C00u && (n.dy & 0x7C00u) != 0x7C00u && (n.dz & 0x7C00u) != 0x7C00u, "BVH node extents are not finite");
    GNode g;
    g.minx = n.min_x; g.miny = n.min_y; g.minz = n.min_z;
    g.maxx = n.min_x + half_bits_to_float(n.dx);                  // CompactBVH2Node.cpp:8-10, one rounded add each
    g.maxy = n.min_y + half_bits_to_float(n.dy);
    g.maxz = n.min_z + half_bits_to_float(n.dz);
    g.link = skip[i] << 5;                                         // (byte offsets: trace_kernels.hpp GNode)
    g.hit = (i + 1) << 5;                                          // interior: the first child
    if (n.geom_id != MI_INVALID_GEOM) {
      need(n.geom_id < d.num_geometry, "leaf geomID out of range");
      const mi_geom_ref& r = d.geometry[n.geom_id];
      GLeaf L;
      memset(&L, 0, sizeof L);
      if (r.type == 0) {
        const mi_mesh_info& mi_ = d.mesh_info[r.index];
        need(n.prim_or_second_child < mi_.num_triangles, "leaf primID out of range");
        const size_t base = 3 * ((size_t)mi_.first_index + n.prim_or_second_child);
        for (int k = 0; k < 3; ++k) {
          const mi_vec3& p = d.mesh_verts[mi_.first_vertex + d.mesh_tris[base + k]];
          L.f[3 * k] = p.x; L.f[3 * k + 1] = p.y; L.f[3 * k + 2] = p.z;
        }
        L.type = LEAF_TRI | ((uint32_t)n.geom_id << 16); L.primID = n.prim_or_second_child; L.triBase = (uint32_t)base;
        const f3 p0 = mk(L.f[0], L.f[1], L.f[2]), p1 = mk(L.f[3], L.f[4], L.f[5]), p2 = mk(L.f[6], L.f[7], L.f[8]);
        const f3 fn = normalized(cross(p1 - p0, p2 - p0));                        // Mesh.hpp:112-114
        L.n[0] = fn.x; L.n[1] = fn.y; L.n[2] = fn.z;
      } else if (r.type == 1) {
        const mi_sphere& s = d.spheres[r.index];
        L.f[0] = s.x; L.f[1] = s.y; L.f[2] = s.z; L.f[3] = s.radius; L.f[4] = s.radius * s.radius;   // Primitives.hpp:44
        L.type = LEAF_SPHERE | ((uint32_t)n.geom_id << 16); L.primID = 0;                                                           // Primitives.cpp:45
      } else {
        const mi_disc& c = d.discs[r.index];
        L.f[0] = c.nx; L.f[1] = c.ny; L.f[2] = c.nz; L.f[3] = c.cx; L.f[4] = c.cy; L.f[5] = c.cz; L.f[6] = c.r * c.r;
        L.type = LEAF_DISC | ((uint32_t)n.geom_id << 16); L.primID = 0;
      }
      L.matIndex = d.mat_ids[n.geom_id];
      g.hit = (skip[i] << 5) | kLeafFlag;                          // leaf: stop in front of link (= i + 1)
      leaves[i] = L;
      isLeafNode[i] = 1;
    }
    nodes[i] = g;
  }

  DeviceScene& ds = S.ds;
  ds.nodes = S.keep(upload(nodes)); ds.numNodes = N;
  ds.leaves = S.keep(upload(leaves)); ds.numLeaves = (uint32_t)leaves.size();
  // K1w's private copies (mi_scene::hot): the nodes in hot-first order with their successors renumbered, the records moved along
  // - once over every node (hot), once over the survivors of the collapse (thin). at[k] = the preorder index of the node at place k.
  struct Private { mi_scene::HotCopy* copy; std::vector<uint32_t> at, link; std::vector<GNode> nodes; } priv[2] = {{&S.hot, {}, {}, {}}, {&S.thin, {}, {}, {}}};
  {
    const HotNode* pre = reinterpret_cast<const HotNode*>(nodes.data());
    std::vector<uint8_t> keepNode(N);
    const uint32_t M = hot_collapse_keep(pre, N, kHotCollapseTheta, keepNode.data(), nullptr);
    std::vector<HotNode> thinPre(M);
    std::vector<uint32_t> thinFrom(M);
    hot_collapse_nodes(pre, N, keepNode.data(), thinPre.data(), thinFrom.data());
    need(M == 0 || (thinFrom[0] == 0 && (M == 1 || (thinPre[0].hit == 32u) == !node_is_leaf(nodes[0]))), "the collapsed tree lost its root");      // (root_start: an interior root's first surviving descendant is node 1)
    for (int c = 0; c < 2; ++c) {
      const HotNode* src = c ? thinPre.data() : pre;
      const uint32_t n = c ? M : N;
      std::vector<uint32_t> order(n);
      priv[c].nodes.resize(n);
      priv[c].link.resize(n);
      hot_first_order(src, n, order.data());
      hot_permute_nodes(src, n, order.data(), reinterpret_cast<HotNode*>(priv[c].nodes.data()), priv[c].link.data());
      priv[c].copy->share.resize(n);
      if (c) hot_prefix_share_any(src, n, order.data(), S.thin.share.data()); else hot_prefix_share(src, n, order.data(), S.hot.share.data());
      priv[c].at.resize(n);
      for (uint32_t k = 0; k < n; ++k) priv[c].at[k] = c ? thinFrom[order[k]] : order[k];
      priv[c].copy->numNodes = priv[c].copy->thinNodes = n;
    }
    {
      // the plain builds' arrays: the collapsed tree, then every node (hot_join_regions); the records below follow `at` and `link`
      std::vector<GNode> joined(M + N);
      std::vector<uint32_t> joinedLink(M + N);
      hot_join_regions(reinterpret_cast<const HotNode*>(priv[1].nodes.data()), priv[1].link.data(), M, reinterpret_cast<const HotNode*>(priv[0].nodes.data()), priv[0].link.data(), N,
                       reinterpret_cast<HotNode*>(joined.data()), joinedLink.data());
      priv[1].nodes.swap(joined);
      priv[1].link.swap(joinedLink);
      priv[1].at.insert(priv[1].at.end(), priv[0].at.begin(), priv[0].at.end());
      S.thin.numNodes = M + N;
      S.thin.exactBase = M << 5;
    }
    for (Private& p : priv) p.copy->nodes = S.keep(upload(p.nodes));
    // (a leaf's record carries the node that follows it: a plain record in triBase - the walk reads it with primID's 16 bytes, nothing
    // on the device reads the triangle's index base -, a pre-rotated block in its first word, above the kind: that word loses the geomID
    // bits the shared blocks carry, which no walk reads - the hit's geomID and primID come from the plain record, whose type word stays)
    for (Private& p : priv) {
      std::vector<GLeaf> hotLeaves(p.at.size());
      for (uint32_t k = 0; k < p.at.size(); ++k) { hotLeaves[k] = leaves[p.at[k]]; if (isLeafNode[p.at[k]]) hotLeaves[k].triBase = p.link[k]; }
      p.copy->leaves = S.keep(upload(hotLeaves));
    }
  }
  {
    // the primitive-test part of every record once per shear axis (GLeafRot, trace_kernels.hpp): a triangle's vertices with their
    // components rotated so that component kz comes last - (kx, ky, kz) = (kz + 1, kz + 2, kz) mod 3, permute_kz - other records as they are
    std::vector<GLeafRot> rot(leaves.size());
    memset(rot.data(), 0, rot.size() * sizeof(GLeafRot));
    for (size_t i = 0; i < leaves.size(); ++i)
      for (uint32_t kz = 0; kz < 3; ++kz) {
        GLeafBlock& B = rot[i].b[kz];
        B.type = leaves[i].type;
        for (int q = 0; q < 9; ++q) B.f[q] = leaves[i].f[q];
        if (leaf_kind(leaves[i]) == LEAF_TRI) {
          const uint32_t kx = (kz + 1) % 3, ky = (kz + 2) % 3;
          for (int v = 0; v < 3; ++v) { B.f[3 * v] = leaves[i].f[3 * v + kx]; B.f[3 * v + 1] = leaves[i].f[3 * v + ky]; B.f[3 * v + 2] = leaves[i].f[3 * v + kz]; }
        }
      }
    ds.leavesRot = S.keep(upload(rot));
    for (Private& p : priv) {
      std::vector<GLeafRot> hotRot(p.at.size());
      for (uint32_t k = 0; k < p.at.size(); ++k) {
        hotRot[k] = rot[p.at[k]];
        if (isLeafNode[p.at[k]]) for (uint32_t kz = 0; kz < 3; ++kz) hotRot[k].b[kz].type = p.link[k] | leaf_kind(leaves[p.at[k]]);
      }
      p.copy->rot = S.keep(upload(hotRot));
    }
  }
  ds.matIDs = S.keep(upload(std::vector<uint32_t>(d.mat_ids, d.mat_ids + d.num_mat_ids)));
  ds.materials = S.keep(upload(std::vector<mi_material>(d.materials, d.materials + d.num_materials)));
  ds.numMaterials = d.num_materials;
  ds.hasNormals = d.num_normals ? 1u : 0u;
  ds.leafNormalsOrFrames = nullptr;
  S.hot.leafNormals = S.thin.leafNormals = nullptr;
  S.hot.valid = S.thin.valid = true;
  if (ds.hasNormals) {
    std::vector<float> ln(9 * leaves.size(), 0.f);
    for (size_t k = 0; k < leaves.size(); ++k) {
      const GLeaf& L = leaves[k];
      if (!isLeafNode[k] || leaf_kind(L) != LEAF_TRI) continue;
      const uint32_t fv = geomFirstVertex[leaf_geom(L)];
      for (int c = 0; c < 3; ++c) {
        const size_t at = (size_t)fv + d.mesh_tris[L.triBase + c];
        need(at < d.num_normals, "vertex normal index out of range");
        const mi_vec3& nn = d.mesh_normals[at];
        ln[9 * k + 3 * c] = nn.x; ln[9 * k + 3 * c + 1] = nn.y; ln[9 * k + 3 * c + 2] = nn.z;
      }
    }
    ds.leafNormalsOrFrames = S.keep(upload(ln));
    for (Private& p : priv) {
      std::vector<float> hotLn(9 * p.at.size());
      for (uint32_t k = 0; k < p.at.size(); ++k) memcpy(&hotLn[9 * (size_t)k], &ln[9 * (size_t)p.at[k]], 9 * sizeof(float));
      p.copy->leafNormals = S.keep(upload(hotLn));
    }
    ds.meshTris = S.keep(upload(std::vector<uint16_t>(d.mesh_tris, d.mesh_tris + 3 * (size_t)d.num_tris)));
    ds.meshNormals = S.keep(upload(std::vector<mi_vec3>(d.mesh_normals, d.mesh_normals + d.num_normals)));
    ds.geomFirstVertex = S.keep(upload(geomFirstVertex));
  } else if (N) {
    // no vertex normals: the pointer carries the per-leaf tangent frames instead (leaf_frame.hpp) - diffuse_frame of the normal SHADE reads
    // for a triangle (GLeaf::n) or disc leaf, zeros elsewhere -, in the shared order and in the private copies' (both regions of `thin`)
    std::vector<uint8_t> framed(N);
    std::vector<float> normal(3 * (size_t)N, 0.f);
    for (uint32_t i = 0; i < N; ++i) {
      const GLeaf& L = leaves[i];
      framed[i] = isLeafNode[i] && leaf_kind(L) != LEAF_SPHERE;
      if (framed[i]) memcpy(&normal[3 * (size_t)i], leaf_kind(L) == LEAF_TRI ? L.n : L.f, 3 * sizeof(float));
    }
    std::vector<GLeafFrame> fr(N);
    fill_leaf_frames(framed.data(), normal.data(), nullptr, N, fr.data());
    ds.leafNormalsOrFrames = reinterpret_cast<const float*>(S.keep(upload(fr)));
    for (Private& p : priv) {
      std::vector<GLeafFrame> hotFr(p.at.size());
      fill_leaf_frames(framed.data(), normal.data(), p.at.data(), (uint32_t)p.at.size(), hotFr.data());
      p.copy->leafNormals = reinterpret_cast<const float*>(S.keep(upload(hotFr)));
    }
  }
  ds.rootInterior = 0;
  if (N > 1) {      // (N > 1: the root is an interior node - checked above: a leaf root spans one node; option "root_start" = 0 clears the flag per launch)
    ds.rootLoX = nodes[0].minx; ds.rootHiX = nodes[0].maxx; ds.rootLoY = nodes[0].miny; ds.rootHiY = nodes[0].maxy;
    ds.rootLoZ = nodes[0].minz; ds.rootHiZ = nodes[0].maxz; ds.rootInterior = node_is_leaf(nodes[0]) ? 0u : 1u;
  }
  ds.imageWidth = d.image_width; ds.imageHeight = d.image_height;
  float s, c;
  sincos_deg_table(d.fov_radians / 2.f, hostSinTable(), s, c);   // codelets/TraceCodelets.cpp:147-149
  ds.tanTheta = s / c;
  ds.antiAliasScale = d.anti_alias_scale;
  ds.maxPathLength = d.max_path_length; ds.rouletteStartDepth = d.roulette_start_depth;
  ds.samplesPerPixel = d.samples_per_pixel;
  ds.rngSeed = d.rng_seed;
  HIP_CHECK(hipMalloc(&S.d_counters, 32 * sizeof(unsigned long long)));
  S.keep(S.d_counters);
  HIP_CHECK(hipMemset(S.d_counters, 0, 32 * sizeof(unsigned long long)));
  ds.counters = S.d_counters;

  // what a later mi_scene_update needs, on the host: the topology and the geometry as created (validated above)
  mi_scene::Refit& R = S.refit;
  R.nodes.assign(d.bvh_nodes, d.bvh_nodes + N);
  R.geometry.assign(d.geometry, d.geometry + d.num_geometry);
  R.matIds.assign(d.mat_ids, d.mat_ids + d.num_geometry);
  R.meshInfo.assign(d.mesh_info, d.mesh_info + d.num_meshes);
  R.tris.assign(d.mesh_tris, d.mesh_tris + (d.num_meshes ? 3 * (size_t)d.num_tris : 0));
  R.verts.assign(d.mesh_verts, d.mesh_verts + (d.num_meshes ? d.num_verts : 0));
  R.spheres.assign(d.spheres, d.spheres + d.num_spheres);
  R.discs.assign(d.discs, d.discs + d.num_discs);
  R.numVerts = d.num_meshes ? d.num_verts : 0; R.numNormals = d.num_normals; R.numSpheres = d.num_spheres; R.numDiscs = d.num_discs;
}

// ---- geometry updates (mi_scene_update*, refit_kernels.hpp) -------------------------------------------------------------------
// The refit's device tables, built on the first update from what buildDeviceScene kept: per node what its box is computed from,
// the nodes bucketed by height (leaf 0, interior 1 + the higher child), scratch for the float boxes, two compact arrays (the
// current one and the one a refit writes), and the current geometry.
// The allocations: the two compact arrays, the tables' arrays, the scratch, the current geometry (about 100 bytes per node).
void refitAlloc(mi_scene& S) {
  mi_scene::Refit& R = S.refit;
  if (R.ready) return;
  const uint32_t N = (uint32_t)R.nodes.size();
  if (N) {
    HIP_CHECK(hipMalloc(&R.d_prims, (size_t)N * sizeof(RefitPrim)));
    S.keep(R.d_prims);
    HIP_CHECK(hipMalloc(&R.d_order, (size_t)N * sizeof(uint32_t)));
    S.keep(R.d_order);
    HIP_CHECK(hipMalloc(&R.d_boxes, (size_t)N * sizeof(RefitBox)));
    S.keep(R.d_boxes);
  }
  R.d_cnodes[0] = S.keep(upload(R.nodes));
  R.d_cnodes[1] = S.keep(upload(R.nodes));
  HIP_CHECK(hipMalloc(&R.d_err, sizeof(uint32_t)));
  S.keep(R.d_err);
  R.d_verts = S.keep(upload(R.verts));
  R.d_spheres = S.keep(upload(R.spheres));
  R.d_discs = S.keep(upload(R.discs));
  // (the device copies are the current geometry from now on)
  R.verts = {}; R.spheres = {}; R.discs = {};
  R.ready = true;
}

// Room for `entries` level starts on the device (a rebuilt tree may be higher than the one before: room to spare, the old array
// goes with the scene).
void refitLevelRoom(mi_scene& S, mi_scene::Refit& R, uint32_t entries) {
  if (entries <= R.levelCap) return;
  R.levelCap = 2 * entries;
  HIP_CHECK(hipMalloc(&R.d_levelStart, R.levelCap * sizeof(uint32_t)));
  S.keep(R.d_levelStart);
}

// The top levels that fit one workgroup's threads go to refit_top_kernel: one launch for them, not one per level.
void refitTopFirst(mi_scene::Refit& R) {
  const uint32_t H = (uint32_t)R.levelStart.size() - 2;
  R.topFirst = H + 1;
  while (R.topFirst > 1 && R.levelStart[R.topFirst] - R.levelStart[R.topFirst - 1] <= kRefitTopThreads) --R.topFirst;
}

// The tables of a scene's FIRST update, derived on the host from the nodes it was created with. A rebuild writes the tables of its
// topology on the device (rebuildScene), so nothing is ever derived - or read back - after one.
void refitTables(mi_scene& S) {
  mi_scene::Refit& R = S.refit;
  refitAlloc(S);
  if (R.tables) return;
  ++S.live.hostDerivations;
  const uint32_t N = (uint32_t)R.nodes.size();
  std::vector<RefitPrim> prims(N);
  std::vector<uint32_t> height(N, 0);
  for (uint32_t i = N; i-- > 0;) {
    const mi_bvh_node& n = R.nodes[i];
    RefitPrim p{0u, 0u, 0u, REFIT_INTERIOR};
    if (n.geom_id == MI_INVALID_GEOM) {
      p.a = n.prim_or_second_child;
      height[i] = 1 + std::max(height[i + 1], height[p.a]);
    } else {
      const mi_geom_ref& r = R.geometry[n.geom_id];
      if (r.type == 0) {
        const mi_mesh_info& m = R.meshInfo[r.index];
        const size_t base = 3 * ((size_t)m.first_index + n.prim_or_second_child);
        p = {m.first_vertex + R.tris[base], m.first_vertex + R.tris[base + 1], m.first_vertex + R.tris[base + 2], REFIT_TRI};
      } else {
        p = {r.index, 0u, 0u, r.type == 1 ? (uint32_t)REFIT_SPHERE : (uint32_t)REFIT_DISC};
      }
    }
    prims[i] = p;
  }
  const uint32_t H = N ? height[0] : 0;
  R.levelStart.assign(H + 2, 0);
  for (uint32_t i = 0; i < N; ++i) ++R.levelStart[height[i] + 1];
  for (uint32_t h = 0; h <= H; ++h) R.levelStart[h + 1] += R.levelStart[h];
  std::vector<uint32_t> order(N), at(R.levelStart.begin(), R.levelStart.end() - 1);
  for (uint32_t i = 0; i < N; ++i) order[at[height[i]]++] = i;
  refitTopFirst(R);
  refitLevelRoom(S, R, (uint32_t)R.levelStart.size());
  HIP_CHECK(hipMemcpy(R.d_levelStart, R.levelStart.data(), R.levelStart.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (N) {
    HIP_CHECK(hipMemcpy(R.d_prims, prims.data(), (size_t)N * sizeof(RefitPrim), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(R.d_order, order.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  R.tables = true;
}

// ---- tree cost (mi_scene_bvh_cost, cost_kernels.hpp) --------------------------------------------------------------------------------
// {sum_all, sum_leaf, a_root} of the scene's current compact nodes, on `stream`, which it waits for. A scene that was never updated
// or rebuilt has its nodes on the host only: the twin runs there, on the same shape, and nothing is allocated.
void sceneCost(mi_scene& S, hipStream_t stream, double out[3]) {
  const uint32_t N = S.ds.numNodes;
  mi_scene::Live& L = S.live;
  const mi_scene::Refit& R = S.refit;
  ++L.costEvals;
  out[0] = out[1] = out[2] = 0.0;
  if (!N) return;
  if (R.live < 0) { bvh_cost_host(R.nodes.data(), N, kCostBlock, out); return; }
  // the levels' sizes, the first level first
  uint32_t sizes[8]; int levels = 0;
  uint32_t total = 0;
  for (uint32_t n = N;;) { n = cost_blocks(n, kCostBlock); sizes[levels++] = n; total += n; if (n == 1) break; }
  if (!L.d_cost) { HIP_CHECK(hipMalloc(&L.d_cost, ((size_t)total + 1) * sizeof(Cost2))); S.keep(L.d_cost); }
  // level k lies behind the levels after it: the last one (one entry) in slot 1
  auto levelAt = [&](int k) { uint32_t at = 1; for (int j = levels - 1; j > k; --j) at += sizes[j]; return L.d_cost + at; };
  hipLaunchKernelGGL(cost_term_kernel, dim3(sizes[0]), dim3(kCostBlock), 0, stream, R.d_cnodes[R.live], N, levelAt(0), &L.d_cost[0].all);
  for (int k = 1; k < levels; ++k)
    hipLaunchKernelGGL(cost_partials_kernel, dim3(sizes[k]), dim3(kCostBlock), 0, stream, levelAt(k - 1), sizes[k - 1], levelAt(k));
  HIP_CHECK(hipGetLastError());
  Cost2 back[2];
  HIP_CHECK(hipMemcpyAsync(back, L.d_cost, sizeof back, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  out[0] = back[1].all; out[1] = back[1].leaf; out[2] = back[0].all;
}

// Argument rules of the two update entries: the first three touch neither the scene nor a device.
void updateArgs(const char* fn, const mi_scene* S, const mi_geometry_update* u) {
  auto bad = [&](const char* why) { throw ArgError(std::string(fn) + ": " + why); };
  if (!S) bad("null scene");
  if (!u) bad("null update");
  if ((!u->mesh_verts && u->num_verts) || (!u->mesh_normals && u->num_normals) || (!u->spheres && u->num_spheres) || (!u->discs && u->num_discs))
    bad("a count without its array");
  const mi_scene::Refit& R = S->refit;
  if (u->mesh_verts && u->num_verts != R.numVerts) bad("num_verts differs from the scene's vertex count");
  if (u->mesh_normals && R.numNormals == 0) bad("normals given to a scene created without normals");
  if (u->mesh_normals && u->num_normals != R.numNormals) bad("num_normals differs from the scene's normal count");
  if (u->spheres && u->num_spheres != R.numSpheres) bad("num_spheres differs from the scene's sphere count");
  if (u->discs && u->num_discs != R.numDiscs) bad("num_discs differs from the scene's disc count");
}

// The update proper, on DEVICE arrays (NULL = keep), on `stream`: passes 1 - 3 (scratch only, then the read-back that decides),
// then - behind everything already enqueued on the scene - pass 4 and the copies into the current geometry. Returns when it is
// all in place; on a refused box nothing of the scene has changed.
uint32_t rebuildScene(mi_scene& S, hipStream_t stream);
// DeviceScene::leafNormalsOrFrames as the kernels that rewrite leaves[] take it: one of the two is null
float* leafNormalsOf(const DeviceScene& ds) { return ds.hasNormals ? const_cast<float*>(ds.leafNormalsOrFrames) : nullptr; }
GLeafFrame* leafFramesOf(const DeviceScene& ds) { return ds.hasNormals ? nullptr : reinterpret_cast<GLeafFrame*>(const_cast<float*>(ds.leafNormalsOrFrames)); }
void refitScene(mi_scene& S, const mi_geometry_update& u, hipStream_t stream, const char* fn = "mi_scene_update") {
  refitTables(S);
  mi_scene::Refit& R = S.refit;
  DeviceScene& ds = S.touchArrays();      // (K1w's private copies retire here: the update writes the shared arrays)
  const uint32_t N = ds.numNodes;
  RefitGeom g;
  g.verts = u.mesh_verts ? (const mi_vec3*)u.mesh_verts : R.d_verts;
  g.spheres = u.spheres ? u.spheres : R.d_spheres;
  g.discs = u.discs ? u.discs : R.d_discs;
  g.normals = u.mesh_normals;
  const int scratch = R.live == 0 ? 1 : 0;
  mi_bvh_node* cn = R.d_cnodes[scratch];
  mi_bvh_node root{};
  const bool timing = S.opt.refitTiming && N;
  if (timing && !R.ev[0]) for (hipEvent_t& e : R.ev) HIP_CHECK(hipEventCreate(&e));
  if (N) {
    HIP_CHECK(hipMemsetAsync(R.d_err, 0, sizeof(uint32_t), stream));
    const uint32_t leaves = R.levelStart[1];
    if (timing) HIP_CHECK(hipEventRecord(R.ev[0], stream));
    hipLaunchKernelGGL(refit_leaf_kernel, dim3((leaves + 255) / 256), dim3(256), 0, stream, R.d_order, leaves, R.d_prims, g, R.d_boxes, cn, R.d_err);
    if (timing) HIP_CHECK(hipEventRecord(R.ev[1], stream));
    for (uint32_t h = 1; h < R.topFirst; ++h) {
      const uint32_t cnt = R.levelStart[h + 1] - R.levelStart[h];
      hipLaunchKernelGGL(refit_level_kernel, dim3((cnt + 255) / 256), dim3(256), 0, stream, R.d_order, R.levelStart[h], cnt, R.d_prims, R.d_boxes, cn, R.d_err);
    }
    const uint32_t H = (uint32_t)R.levelStart.size() - 2;
    if (R.topFirst <= H)
      hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(kRefitTopThreads), 0, stream, R.d_order, R.d_levelStart, R.topFirst, H, R.d_prims, R.d_boxes, cn, R.d_err);
    HIP_CHECK(hipGetLastError());
    if (timing) HIP_CHECK(hipEventRecord(R.ev[2], stream));
    uint32_t err = 0;
    HIP_CHECK(hipMemcpyAsync(&err, R.d_err, sizeof err, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(&root, cn, sizeof root, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (timing) {
      float a = 0.f, b = 0.f;
      HIP_CHECK(hipEventElapsedTime(&a, R.ev[0], R.ev[1])); HIP_CHECK(hipEventElapsedTime(&b, R.ev[1], R.ev[2]));
      R.ms[0] = a; R.ms[1] = b;
    }
    // (an empty leaf box - every point NaN on an axis - also makes its parent's extent infinite: the leaf is named first)
    if (err) ++S.live.refused;
    if (err & (1u << kBoxNotFinite)) throw ArgError(std::string(fn) + ": a node box is not finite; the scene is unchanged");
    if (err) throw ArgError(std::string(fn) + ": a node extent is above 65504 (Cannot compress BVH bounds into fp16 (half)); the scene is unchanged");
  }
  // option auto_rebuild: the baseline where there is none yet - the estimate of the tree as it stands before this update, which
  // is now certain to be applied (R.live still names it)
  const double ratio = S.opt.autoRebuild;
  if (ratio > 0.0 && N && !S.live.baselineValid) {
    double c[3];
    sceneCost(S, stream, c);
    S.live.baseline = bvh_cost_estimate(c); S.live.baselineValid = true;
  }
  // from here on the scene changes: after everything already enqueued on it, on any stream
  for (LaunchSlot& l : S.slots) if (l.stream != stream) HIP_CHECK(hipStreamWaitEvent(stream, l.lastWork, 0));
  if (N) {
    if (timing) HIP_CHECK(hipEventRecord(R.ev[3], stream));
    hipLaunchKernelGGL(refit_write_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, N, R.d_prims, cn, g, const_cast<GNode*>(ds.nodes),
                       const_cast<GLeaf*>(ds.leaves), const_cast<GLeafRot*>(ds.leavesRot), leafNormalsOf(ds), leafFramesOf(ds));
    HIP_CHECK(hipGetLastError());
  }
  if (u.mesh_verts && R.numVerts) HIP_CHECK(hipMemcpyAsync(R.d_verts, u.mesh_verts, (size_t)R.numVerts * sizeof(mi_vec3), hipMemcpyDeviceToDevice, stream));
  if (u.spheres && R.numSpheres) HIP_CHECK(hipMemcpyAsync(R.d_spheres, u.spheres, (size_t)R.numSpheres * sizeof(mi_sphere), hipMemcpyDeviceToDevice, stream));
  if (u.discs && R.numDiscs) HIP_CHECK(hipMemcpyAsync(R.d_discs, u.discs, (size_t)R.numDiscs * sizeof(mi_disc), hipMemcpyDeviceToDevice, stream));
  if (u.mesh_normals && ds.meshNormals)
    HIP_CHECK(hipMemcpyAsync(const_cast<mi_vec3*>(ds.meshNormals), u.mesh_normals, (size_t)R.numNormals * sizeof(mi_vec3), hipMemcpyDeviceToDevice, stream));
  if (timing) HIP_CHECK(hipEventRecord(R.ev[1], stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  if (timing) { float w = 0.f; HIP_CHECK(hipEventElapsedTime(&w, R.ev[3], R.ev[1])); R.ms[2] = w; }
  ++S.live.applied;
  S.freeRetiredHot();
  if (!N) return;
  R.live = scratch;
  if (N > 1) {      // the root's box as buildDeviceScene sets it (root_start)
    ds.rootLoX = root.min_x; ds.rootHiX = root.min_x + half_bits_to_float(root.dx);
    ds.rootLoY = root.min_y; ds.rootHiY = root.min_y + half_bits_to_float(root.dy);
    ds.rootLoZ = root.min_z; ds.rootHiZ = root.min_z + half_bits_to_float(root.dz);
  }
  // option auto_rebuild: the refitted tree's estimate against the baseline, a binary64 compare of figures that are functions of the
  // geometry alone (the cost pass is bit-reproducible), so every replica fed the same arrays decides alike
  if (ratio > 0.0) {
    double c[3];
    sceneCost(S, stream, c);
    if (c[2] > 0.0 && bvh_cost_estimate(c) > ratio * S.live.baseline) {
      rebuildScene(S, stream);        // (the baseline becomes the rebuilt tree's estimate there)
      ++S.live.autoRebuilds;
    }
  }
}

// ---- topology rebuild (mi_scene_rebuild, rebuild_kernels.hpp) ---------------------------------------------------------------------
template <class K>
void rebuildSort(mi_scene::Rebuild& B, K* keys[2], uint32_t* vals[2], uint32_t n, unsigned endBit, hipStream_t stream, K*& keysOut, uint32_t*& valsOut) {
  rocprim::double_buffer<K> kb(keys[0], keys[1]);
  rocprim::double_buffer<uint32_t> vb(vals[0], vals[1]);
  size_t bytes = B.sortTmpBytes;
  HIP_CHECK(rocprim::radix_sort_pairs(B.d_sortTmp, bytes, kb, vb, n, 0u, endBit, stream));
  keysOut = kb.current(); valsOut = vb.current();
}
template <class K>
size_t rebuildSortBytes(uint32_t n, unsigned endBit) {
  rocprim::double_buffer<K> kb(nullptr, nullptr);
  rocprim::double_buffer<uint32_t> vb(nullptr, nullptr);
  size_t bytes = 0;
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, kb, vb, n, 0u, endBit, (hipStream_t) nullptr));
  return bytes;
}

// The passes' scratch for P primitives: every array here is written from its start by every build before it is read, so it belongs
// to no contents. Kept while it is large enough: new contents of a scene (setGeometry) reuse it, and take new arrays - the old ones
// are given up by the caller - only when they have grown. (The canonical table is not scratch: it is the contents'.)
void rebuildScratch(mi_scene& S, mi_scene::Rebuild& B, uint32_t P) {
  const size_t N = 2 * (size_t)P - 1;
  const uint32_t I = P - 1;
  const size_t sortBytes = std::max({rebuildSortBytes<uint64_t>(P, 3 * kMortonBits), rebuildSortBytes<uint32_t>(std::max(I, 1u), 8),
                                     rebuildSortBytes<uint32_t>((uint32_t)N, 8)});
  if (B.capPrims >= P && B.sortTmpBytes >= sortBytes) return;
  auto alloc = [&](auto*& p, size_t count) { HIP_CHECK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(*p))); S.keep(p); };
  alloc(B.d_primBoxes, P); alloc(B.d_parts, kRebuildParts); alloc(B.d_sceneBox, 1);
  for (int k = 0; k < 2; ++k) { alloc(B.d_keys[k], P); alloc(B.d_vals[k], P); alloc(B.d_depth[k], I); alloc(B.d_ids[k], I); }
  alloc(B.d_child, I); alloc(B.d_range, I); alloc(B.d_parent, N); alloc(B.d_swapped, I); alloc(B.d_index, N);
  alloc(B.d_levelStart, kRebuildMaxDepth + 2);
  alloc(B.d_height, N); alloc(B.d_hvals[0], N); alloc(B.d_hvals[1], N); alloc(B.d_heightStart, kRebuildHeightSlots);
  B.sortTmpBytes = sortBytes;
  HIP_CHECK(hipMalloc(&B.d_sortTmp, std::max<size_t>(B.sortTmpBytes, 16)));
  S.keep(B.d_sortTmp);
  B.capPrims = P;
}
// every buffer rebuildScratch allocates
std::vector<void*> rebuildScratchBuffers(const mi_scene::Rebuild& B) {
  return {B.d_primBoxes, B.d_parts, B.d_sceneBox, B.d_keys[0], B.d_keys[1], B.d_vals[0], B.d_vals[1], B.d_depth[0], B.d_depth[1],
          B.d_ids[0], B.d_ids[1], B.d_child, B.d_range, B.d_parent, B.d_swapped, B.d_index, B.d_levelStart, B.d_height, B.d_hvals[0],
          B.d_hvals[1], B.d_heightStart, B.d_sortTmp};
}

// The canonical primitive table (geometry 0 .. G - 1, inside a mesh triangle 0 .. T - 1) and the passes' scratch, at the first rebuild
// of a scene that still has the contents it was created with: from the host copies create kept. (New contents write the table
// on the device and leave it ready: setGeometry.)
void rebuildTables(mi_scene& S) {
  mi_scene::Rebuild& B = S.rebuild;
  if (B.ready) return;
  const mi_scene::Refit& R = S.refit;
  mi_scene_geometry d{};
  d.geometry = R.geometry.data(); d.num_geometry = (uint32_t)R.geometry.size(); d.mesh_info = R.meshInfo.data(); d.num_meshes = (uint32_t)R.meshInfo.size();
  std::vector<uint32_t> primStart(d.num_geometry + 1);
  const size_t P = canon_prim_starts(d, primStart.data()), N = R.nodes.size();
  std::vector<RebuildPrim> canon(P);
  for (uint32_t p = 0; p < (uint32_t)P; ++p)      // (the indices were checked at create)
    (void)canon_prim(p, primStart.data(), d.num_geometry, d.geometry, d.mesh_info, R.matIds.data(), R.tris.data(), canon[p]);
  if (N != (P ? 2 * P - 1 : 0)) throw ArgError("mi_scene_rebuild: the scene's BVH does not hold every primitive exactly once (one leaf per primitive is what a rebuild keeps)");
  B.numPrims = (uint32_t)P;
  if (P) {
    rebuildScratch(S, B, (uint32_t)P);
    B.d_canon = S.keep(upload(canon));
  }
  B.ready = true;
}

// The build proper on `stream`, shared by mi_scene_rebuild (R, B, ds = the scene's own: its live records are rewritten in place) and
// mi_scene_set_geometry* (R, B, ds = a set built aside for the new contents, which becomes the scene's afterwards): passes 1 - 9
// (scratch only, then the read-back that decides), then the scatter over ds's records and R's tables - in place, behind everything
// already enqueued on the scene. B.d_canon holds the P = B.numPrims > 0 canonical primitives, R the geometry, ds.numNodes = 2 P - 1.
// Returns when it is all in place, the refit's tables of the new topology included; on a refusal (an ArgError that starts with
// `fn`) nothing of ds's records or R's tables has been written. Returns the maximal leaf depth (root = 1).
uint32_t rebuildPasses(mi_scene& S, mi_scene::Refit& R, mi_scene::Rebuild& B, DeviceScene& ds, hipStream_t stream, const char* fn, bool inPlace) {
  const uint32_t N = ds.numNodes;
  const uint32_t P = B.numPrims, I = P - 1;
  RefitGeom g;
  g.verts = R.d_verts; g.spheres = R.d_spheres; g.discs = R.d_discs;
  g.normals = ds.hasNormals ? ds.meshNormals : nullptr;
  const int scratch = R.live == 0 ? 1 : 0;
  const bool timing = S.opt.rebuildTiming;
  if (timing && !B.ev[0]) for (hipEvent_t& e : B.ev) HIP_CHECK(hipEventCreate(&e));
  auto mark = [&](int k) { if (timing) HIP_CHECK(hipEventRecord(B.ev[k], stream)); };
  auto blocks = [](uint32_t n) { return dim3((n + 255) / 256); };
  RebuildTree t;
  t.numPrims = P; t.child = B.d_child; t.range = B.d_range; t.parent = B.d_parent; t.swapped = B.d_swapped; t.boxes = R.d_boxes; t.index = B.d_index;
  t.height = B.d_height;

  if (inPlace) HIP_CHECK(hipMemsetAsync(R.d_err, 0, sizeof(uint32_t), stream));      // (aside: cleared in front of the table's kernel, which raises a bit of it)
  mark(0);
  const uint32_t parts = std::min((P + 255) / 256, kRebuildParts);
  hipLaunchKernelGGL(rebuild_prim_kernel, dim3(parts), dim3(256), 0, stream, P, B.d_canon, g, B.d_primBoxes, B.d_parts, R.d_err);
  hipLaunchKernelGGL(rebuild_scene_kernel, dim3(1), dim3(kRebuildParts), 0, stream, B.d_parts, parts, B.d_sceneBox);
  hipLaunchKernelGGL(rebuild_key_kernel, blocks(P), dim3(256), 0, stream, P, B.d_primBoxes, B.d_sceneBox, B.d_keys[0], B.d_vals[0]);
  HIP_CHECK(hipGetLastError());
  mark(1);
  uint64_t* keys = nullptr; uint32_t* sorted = nullptr;
  rebuildSort<uint64_t>(B, B.d_keys, B.d_vals, P, 3 * kMortonBits, stream, keys, sorted);
  t.sorted = sorted;
  mark(2);
  hipLaunchKernelGGL(rebuild_hierarchy_kernel, blocks(P), dim3(256), 0, stream, keys, B.d_primBoxes, t);
  uint32_t levelStart[kRebuildMaxDepth + 2] = {0};
  uint32_t* order = nullptr;
  if (I) {
    hipLaunchKernelGGL(rebuild_depth_kernel, blocks(I), dim3(256), 0, stream, I, B.d_parent, B.d_depth[0], B.d_ids[0]);
    HIP_CHECK(hipGetLastError());
    uint32_t* depth = nullptr;
    rebuildSort<uint32_t>(B, B.d_depth, B.d_ids, I, 8, stream, depth, order);
    HIP_CHECK(hipMemsetAsync(B.d_levelStart, 0, sizeof levelStart, stream));
    hipLaunchKernelGGL(rebuild_levels_kernel, blocks(I), dim3(256), 0, stream, I, depth, B.d_levelStart);
    HIP_CHECK(hipGetLastError());
    // the host launches one kernel per depth: it needs to know where the depths start
    HIP_CHECK(hipMemcpyAsync(levelStart, B.d_levelStart, sizeof levelStart, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  mark(3);
  const uint32_t D = levelStart[kRebuildMaxDepth + 1];           // the deepest interior node
  if (I) {
    if (D >= kRebuildMaxDepth) throw DeviceError(std::string(fn) + ": interior depth out of range");
    // depths 0 .. top go to the one-workgroup kernel: from the root down, every level of at most kRefitTopThreads nodes
    uint32_t top = 0;
    while (top < D && levelStart[top + 2] - levelStart[top + 1] <= kRefitTopThreads) ++top;
    for (uint32_t d = D; d > top; --d) {
      const uint32_t cnt = levelStart[d + 1] - levelStart[d];
      hipLaunchKernelGGL(rebuild_level_kernel, blocks(cnt), dim3(256), 0, stream, order, levelStart[d], cnt, t, R.d_err);
    }
    hipLaunchKernelGGL(rebuild_top_kernel, dim3(1), dim3(kRefitTopThreads), 0, stream, order, B.d_levelStart, top, t, R.d_err);
    HIP_CHECK(hipGetLastError());
  }
  mark(4);
  hipLaunchKernelGGL(rebuild_preorder_kernel, blocks(N), dim3(256), 0, stream, t);
  HIP_CHECK(hipGetLastError());
  mark(5);
  // the refit's order of the new topology: the nodes by height (scratch: the Morton sort's key buffers are free by now and hold
  // 2 P words each), and where the heights start - read back with the decision below, no wait of its own
  uint32_t* hkeys[2] = {(uint32_t*)B.d_keys[0], (uint32_t*)B.d_keys[1]};
  hipLaunchKernelGGL(rebuild_heightkey_kernel, blocks(N), dim3(256), 0, stream, t, hkeys[0], B.d_hvals[0]);
  HIP_CHECK(hipGetLastError());
  uint32_t* heights = nullptr; uint32_t* byHeight = nullptr;
  rebuildSort<uint32_t>(B, hkeys, B.d_hvals, N, 8, stream, heights, byHeight);
  uint32_t heightStart[kRebuildHeightSlots] = {0};
  HIP_CHECK(hipMemsetAsync(B.d_heightStart, 0, sizeof heightStart, stream));
  hipLaunchKernelGGL(rebuild_heights_kernel, blocks(N), dim3(256), 0, stream, N, heights, B.d_heightStart);
  HIP_CHECK(hipGetLastError());
  uint32_t err = 0;
  RefitBox rootBox{};
  HIP_CHECK(hipMemcpyAsync(&err, R.d_err, sizeof err, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(&rootBox, R.d_boxes, sizeof rootBox, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipMemcpyAsync(heightStart, B.d_heightStart, sizeof heightStart, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  // (an index out of range comes first, as at create: its record named another vertex, the boxes are not the arrays')
  if (err & (1u << kTriIndexOutOfRange)) throw ArgError(std::string(fn) + ": triangle vertex index out of range; the scene is unchanged");
  if (err & (1u << kBoxNotFinite)) throw ArgError(std::string(fn) + ": a node box is not finite; the scene is unchanged");
  if (err) throw ArgError(std::string(fn) + ": a node extent is above 65504 (Cannot compress BVH bounds into fp16 (half)); the scene is unchanged");
  const uint32_t H = heightStart[kRebuildHeightSlots - 1];
  if (H > kRebuildMaxDepth || heightStart[H + 1] != N) throw DeviceError(std::string(fn) + ": node heights out of range");
  refitLevelRoom(S, R, H + 2);
  // from here on the scene changes: after everything already enqueued on it, on any stream (records built aside are nobody's yet)
  if (inPlace) for (LaunchSlot& l : S.slots) if (l.stream != stream) HIP_CHECK(hipStreamWaitEvent(stream, l.lastWork, 0));
  hipLaunchKernelGGL(rebuild_scatter_kernel, blocks(N), dim3(256), 0, stream, t, B.d_canon, g, R.d_cnodes[scratch], const_cast<GNode*>(ds.nodes),
                     const_cast<GLeaf*>(ds.leaves), const_cast<GLeafRot*>(ds.leavesRot), leafNormalsOf(ds), leafFramesOf(ds), R.d_prims);
  HIP_CHECK(hipGetLastError());
  // both compact arrays carry the topology (a refit keeps the links and geomIDs of the array it writes)
  HIP_CHECK(hipMemcpyAsync(R.d_cnodes[1 - scratch], R.d_cnodes[scratch], (size_t)N * sizeof(mi_bvh_node), hipMemcpyDeviceToDevice, stream));
  // the refit's tables of the new topology: the scatter wrote d_prims; the order and the level starts out of the scratch
  HIP_CHECK(hipMemcpyAsync(R.d_order, byHeight, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
  HIP_CHECK(hipMemcpyAsync(R.d_levelStart, B.d_heightStart, (H + 2) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
  mark(6);
  HIP_CHECK(hipStreamSynchronize(stream));
  if (timing)
    for (int k = 0; k < 6; ++k) { float w = 0.f; HIP_CHECK(hipEventElapsedTime(&w, B.ev[k], B.ev[k + 1])); B.ms[k] = w; }
  R.live = scratch;
  R.levelStart.assign(heightStart, heightStart + H + 2);
  refitTopFirst(R);
  R.tables = true;
  ds.rootInterior = 0;
  if (N > 1) {                     // the root's box as buildDeviceScene sets it (root_start)
    Box3 rb; rb.lo = mk(rootBox.lx, rootBox.ly, rootBox.lz); rb.hi = mk(rootBox.hx, rootBox.hy, rootBox.hz);
    mi_bvh_node root{};
    box_encode(rb, root.min_x, root.min_y, root.min_z, root.dx, root.dy, root.dz);
    ds.rootLoX = root.min_x; ds.rootHiX = root.min_x + half_bits_to_float(root.dx);
    ds.rootLoY = root.min_y; ds.rootHiY = root.min_y + half_bits_to_float(root.dy);
    ds.rootLoZ = root.min_z; ds.rootHiZ = root.min_z + half_bits_to_float(root.dz);
    ds.rootInterior = 1u;
  }
  return I ? D + 2 : 1u;
}

// option auto_rebuild: the baseline is the estimate of the tree right after its last rebuild or its last new contents (with the
// option off, an update that finds it on takes the tree as it then stands)
void rebuildBaseline(mi_scene& S, hipStream_t stream) {
  S.live.baselineValid = false;
  if (S.opt.autoRebuild > 0.0 && S.ds.numNodes) {
    double c[3];
    sceneCost(S, stream, c);
    S.live.baseline = bvh_cost_estimate(c); S.live.baselineValid = true;
  }
}

// mi_scene_rebuild's work (and option auto_rebuild's): the scene's own records rebuilt in place
uint32_t rebuildScene(mi_scene& S, hipStream_t stream) {
  if (!S.ds.numNodes) return 0;
  // the current geometry and the two compact arrays on the device, the float-box scratch, the error word, room for the refit's
  // tables: the update's allocations, made once (a rebuild reads nothing of the tables, and writes them below)
  refitAlloc(S);
  rebuildTables(S);
  S.live.maxLeafDepth = rebuildPasses(S, S.refit, S.rebuild, S.touchArrays(), stream, "mi_scene_rebuild", true);
  rebuildBaseline(S, stream);
  S.freeRetiredHot();
  return S.live.maxLeafDepth;
}

// ---- rigid poses (mi_scene_set_poses*, pose_kernels.hpp) ---------------------------------------------------------------------------
// The rest snapshot is no longer the scene's rest geometry and every pose is the identity again: after an update or a bake. The
// buffers stay (the counts have not changed); the next pose call copies the current geometry into them.
void poseInvalidate(mi_scene& S) { S.poses.snapshot = false; S.poses.posed = false; }

// New contents: other counts, another geometry list. The buffers go; a scene that is not posed again allocates none.
void poseDrop(mi_scene& S) {
  mi_scene::Poses& P = S.poses;
  for (void* p : P.buffers()) S.release(p);
  mi_scene::Poses fresh;
  for (int k = 0; k < 3; ++k) fresh.ev[k] = P.ev[k];
  P = fresh;
}

// The rest snapshot: the scene's current geometry copied aside on `stream`, and the owner of every vertex, sphere and disc derived
// on the host from the geometry list (pose_owners). An ownership conflict is refused before anything is allocated or copied.
void poseSnapshot(mi_scene& S, hipStream_t stream, const char* fn) {
  mi_scene::Poses& P = S.poses;
  mi_scene::Refit& R = S.refit;
  if (P.snapshot) return;
  const uint32_t G = (uint32_t)R.geometry.size();
  std::vector<uint16_t> vo, so, dso;
  const std::string conflict = pose_owners(R.geometry.data(), G, R.meshInfo.data(), (uint32_t)R.meshInfo.size(), R.numVerts, R.numSpheres, R.numDiscs, vo, so, dso);
  if (!conflict.empty()) throw ArgError(std::string(fn) + ": " + conflict + "; the scene is unchanged");
  if (!P.allocated) {
    auto alloc = [&](auto*& p, size_t count) { p = nullptr; if (count) { HIP_CHECK(hipMalloc(&p, count * sizeof(*p))); S.keep(p); } };
    alloc(P.d_restVerts, R.numVerts); alloc(P.d_outVerts, R.numVerts); alloc(P.d_vertOwner, R.numVerts);
    alloc(P.d_restNormals, R.numNormals); alloc(P.d_outNormals, R.numNormals);
    alloc(P.d_restSpheres, R.numSpheres); alloc(P.d_outSpheres, R.numSpheres); alloc(P.d_sphereOwner, R.numSpheres);
    alloc(P.d_restDiscs, R.numDiscs); alloc(P.d_outDiscs, R.numDiscs); alloc(P.d_discOwner, R.numDiscs);
    alloc(P.d_frames, G); alloc(P.d_poses, G); alloc(P.d_staged, G); alloc(P.d_bad, 2);
    P.allocated = true;
  }
  auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, stream)); };
  copy(P.d_restVerts, R.d_verts, (size_t)R.numVerts * sizeof(mi_vec3), hipMemcpyDeviceToDevice);
  copy(P.d_restNormals, S.ds.meshNormals, (size_t)R.numNormals * sizeof(mi_vec3), hipMemcpyDeviceToDevice);
  copy(P.d_restSpheres, R.d_spheres, (size_t)R.numSpheres * sizeof(mi_sphere), hipMemcpyDeviceToDevice);
  copy(P.d_restDiscs, R.d_discs, (size_t)R.numDiscs * sizeof(mi_disc), hipMemcpyDeviceToDevice);
  copy(P.d_vertOwner, vo.data(), vo.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  copy(P.d_sphereOwner, so.data(), so.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  copy(P.d_discOwner, dso.data(), dso.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  HIP_CHECK(hipStreamSynchronize(stream));      // (the owner tables are this function's own vectors)
  P.snapshot = true;
}

// Argument rules of the two pose entries: the first two touch neither the scene nor a device.
void poseArgs(const char* fn, const mi_scene* S, const void* poses, uint32_t numGeometry) {
  auto bad = [&](const char* why) { throw ArgError(std::string(fn) + ": " + why); };
  if (!S) bad("null scene");
  if (!poses && numGeometry) bad("null poses");
  if (numGeometry != S->refit.geometry.size()) bad("num_geometry differs from the scene's geometry count");
}

// The poses proper, G of them in DEVICE memory (d_poses) or in HOST memory (h_poses, staged into the scene's own array), on `stream`:
// the rest snapshot where there is none, the frame kernel (which decides validity), the pose pass into the scene's scratch arrays,
// one small read-back, then refitScene on those arrays - which copies them into the current geometry on success and moves nothing
// on refusal. `snapshotWas`: a snapshot taken for a call that is then refused is dropped again, so that a refusal leaves the rest
// geometry as undefined as it was.
void poseScene(mi_scene& S, const mi_pose* d_poses, const mi_pose* h_poses, hipStream_t stream, const char* fn) {
  mi_scene::Poses& P = S.poses;
  mi_scene::Refit& R = S.refit;
  const uint32_t G = (uint32_t)R.geometry.size();
  if (!G) return;
  refitTables(S);      // (the current geometry on the device: a scene's first update or pose uploads it)
  const bool snapshotWas = P.snapshot;
  poseSnapshot(S, stream, fn);
  try {
    if (h_poses) {
      HIP_CHECK(hipMemcpyAsync(P.d_staged, h_poses, (size_t)G * sizeof(mi_pose), hipMemcpyHostToDevice, stream));
      d_poses = P.d_staged;
    }
    const bool timing = S.opt.refitTiming;
    if (timing && !P.ev[0]) for (hipEvent_t& e : P.ev) HIP_CHECK(hipEventCreate(&e));
    const uint32_t preset[2] = {0u, 0xFFFFFFFFu};
    HIP_CHECK(hipMemcpyAsync(P.d_bad, preset, sizeof preset, hipMemcpyHostToDevice, stream));
    if (timing) HIP_CHECK(hipEventRecord(P.ev[0], stream));
    hipLaunchKernelGGL(pose_frame_kernel, dim3((G + kPoseBlock - 1) / kPoseBlock), dim3(kPoseBlock), 0, stream, reinterpret_cast<const float4*>(d_poses), G,
                       P.d_frames, P.d_bad);
    const uint64_t total = (uint64_t)R.numVerts + R.numSpheres + R.numDiscs;
    if (total) {
      const PoseRest rest{P.d_restVerts, P.d_restNormals, P.d_restSpheres, P.d_restDiscs};
      const PoseOwners owners{P.d_vertOwner, P.d_sphereOwner, P.d_discOwner};
      const PoseOut out{P.d_outVerts, P.d_outNormals, P.d_outSpheres, P.d_outDiscs};
      hipLaunchKernelGGL(pose_apply_kernel, dim3((uint32_t)((total + kPoseBlock - 1) / kPoseBlock)), dim3(kPoseBlock), 0, stream, R.numVerts, R.numSpheres,
                         R.numDiscs, rest, owners, P.d_frames, out);
    }
    HIP_CHECK(hipGetLastError());
    if (timing) HIP_CHECK(hipEventRecord(P.ev[1], stream));
    uint32_t bad[2] = {0u, 0u};
    HIP_CHECK(hipMemcpyAsync(bad, P.d_bad, sizeof bad, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (bad[0]) throw ArgError(std::string(fn) + ": pose " + std::to_string(bad[1]) + " is not valid (eight finite floats, a quaternion whose squared norm and its "
                               "reciprocal are finite and positive, scale > 0); the scene is unchanged");
    mi_geometry_update u{};
    if (R.numVerts) { u.mesh_verts = P.d_outVerts; u.num_verts = R.numVerts; }
    if (R.numNormals) { u.mesh_normals = P.d_outNormals; u.num_normals = R.numNormals; }
    if (R.numSpheres) { u.spheres = P.d_outSpheres; u.num_spheres = R.numSpheres; }
    if (R.numDiscs) { u.discs = P.d_outDiscs; u.num_discs = R.numDiscs; }
    refitScene(S, u, stream, fn);
    if (d_poses != P.d_poses) HIP_CHECK(hipMemcpyAsync(P.d_poses, d_poses, (size_t)G * sizeof(mi_pose), hipMemcpyDeviceToDevice, stream));
    if (timing) HIP_CHECK(hipEventRecord(P.ev[2], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    P.posed = true;
    if (timing) {
      float a = 0.f, b = 0.f;
      HIP_CHECK(hipEventElapsedTime(&a, P.ev[0], P.ev[1])); HIP_CHECK(hipEventElapsedTime(&b, P.ev[1], P.ev[2]));
      P.ms[0] = a; P.ms[1] = b;
    }
  } catch (...) {
    if (!snapshotWas) P.snapshot = false;
    throw;
  }
}

// ---- new contents (mi_scene_set_geometry*, canon_kernels.hpp) ---------------------------------------------------------------------
// The scene's contents replaced by the arrays of `g` (control plane on the host, data plane where `kind` says) and its BVH built from
// them: everything the contents own - geometry, records, the refit's tables - is allocated aside, the canonical table is written by
// canon_prim_kernel, rebuildPasses runs into the new set, and only after its decision the scene's pointers are swapped and the old
// set is freed, once the work the scene had enqueued before has finished. The rebuild's scratch is reused while it is large enough.
// On any failure the new set is freed and the scene is as it was. Returns the maximal leaf depth.
uint32_t setGeometry(mi_scene& S, const mi_scene_geometry& g, hipStream_t stream, hipMemcpyKind kind, const char* fn) {
  canon_check_control(g, kLeafFlag >> 5, [&](bool ok, const char* what) { if (!ok) throw ArgError(std::string(fn) + ": " + what); });
  const uint32_t G = g.num_geometry, M = g.num_meshes;
  std::vector<uint32_t> primStart(G + 1);
  const uint32_t P = canon_prim_starts(g, primStart.data());
  const uint32_t N = P ? 2 * P - 1 : 0;
  const uint32_t numVerts = M ? g.num_verts : 0, numTris = M ? g.num_tris : 0;      // (as create keeps them)
  if (!S.refit.d_err) { HIP_CHECK(hipMalloc(&S.refit.d_err, sizeof(uint32_t))); S.keep(S.refit.d_err); }
  if (S.opt.rebuildTiming && !S.rebuild.ev[0]) for (hipEvent_t& e : S.rebuild.ev) HIP_CHECK(hipEventCreate(&e));

  const size_t mark = S.allocations.size();      // what is kept from here on is the new set's: freed again on any failure
  std::vector<void*> staged;                     // the control plane's device copies: freed on every way out
  DeviceScene ds = S.ds;
  mi_scene::Refit R;
  mi_scene::Rebuild B = S.rebuild;
  uint32_t depth = 0;
  try {
    auto alloc = [&](auto*& p, size_t count) { p = nullptr; if (count) { HIP_CHECK(hipMalloc(&p, count * sizeof(*p))); S.keep(p); } };
    auto put = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind k) { if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, k, stream)); };
    auto stage = [&](auto*& p, const void* src, size_t count) {
      p = nullptr;
      if (!count) return;
      HIP_CHECK(hipMalloc(&p, count * sizeof(*p)));
      staged.push_back(p);
      put(p, src, count * sizeof(*p), hipMemcpyHostToDevice);
    };
    // the contents: materials, the geometry as the refit and the rebuild read it, what vertex-normal scenes look up
    uint32_t* matIDs; mi_material* materials; uint16_t* tris; mi_vec3* normals; uint32_t* firstVertex;
    alloc(matIDs, g.num_mat_ids); put(matIDs, g.mat_ids, (size_t)g.num_mat_ids * sizeof(uint32_t), hipMemcpyHostToDevice);
    alloc(materials, g.num_materials); put(materials, g.materials, (size_t)g.num_materials * sizeof(mi_material), hipMemcpyHostToDevice);
    alloc(R.d_verts, numVerts); put(R.d_verts, g.mesh_verts, (size_t)numVerts * sizeof(mi_vec3), kind);
    alloc(R.d_spheres, g.num_spheres); put(R.d_spheres, g.spheres, (size_t)g.num_spheres * sizeof(mi_sphere), kind);
    alloc(R.d_discs, g.num_discs); put(R.d_discs, g.discs, (size_t)g.num_discs * sizeof(mi_disc), kind);
    alloc(tris, 3 * (size_t)numTris); put(tris, g.mesh_tris, 3 * (size_t)numTris * sizeof(uint16_t), kind);
    alloc(normals, g.num_normals); put(normals, g.mesh_normals, (size_t)g.num_normals * sizeof(mi_vec3), kind);
    alloc(firstVertex, G);
    R.numVerts = numVerts; R.numNormals = g.num_normals; R.numSpheres = g.num_spheres; R.numDiscs = g.num_discs;
    R.geometry.assign(g.geometry, g.geometry + G);                     // (what mi_scene_set_poses* derives the owners from)
    R.meshInfo.assign(g.mesh_info, g.mesh_info + M);
    R.d_err = S.refit.d_err;
    for (int k = 0; k < 4; ++k) R.ev[k] = S.refit.ev[k];
    for (int k = 0; k < 3; ++k) R.ms[k] = S.refit.ms[k];
    R.ready = true;
    // the records and the refit's tables, one entry per node
    GNode* nodes; GLeaf* leaves; GLeafRot* rot; float* leafNormals;      // (the last: nine floats of vertex normals per node, or a GLeafFrame - eight - where there are none)
    alloc(nodes, N); alloc(leaves, N); alloc(rot, N); alloc(leafNormals, (g.num_normals ? 9 : sizeof(GLeafFrame) / sizeof(float)) * (size_t)N);
    alloc(R.d_prims, N); alloc(R.d_order, N); alloc(R.d_boxes, N); alloc(R.d_cnodes[0], N); alloc(R.d_cnodes[1], N);
    ds.nodes = nodes; ds.numNodes = N; ds.leaves = leaves; ds.numLeaves = N; ds.leavesRot = rot;
    ds.matIDs = matIDs; ds.materials = materials; ds.numMaterials = g.num_materials;
    ds.hasNormals = g.num_normals ? 1u : 0u; ds.leafNormalsOrFrames = leafNormals;
    ds.meshTris = tris; ds.meshNormals = normals; ds.geomFirstVertex = firstVertex;
    ds.rootInterior = 0;
    ds.rootLoX = ds.rootHiX = ds.rootLoY = ds.rootHiY = ds.rootLoZ = ds.rootHiZ = 0.f;
    B.numPrims = P; B.ready = true;
    alloc(B.d_canon, P);                         // (the table is the new contents': a refusal must leave the scene's own as it is)
    if (P) {
      rebuildScratch(S, B, P);
      uint32_t* d_primStart; mi_geom_ref* d_geometry; mi_mesh_info* d_meshInfo;
      stage(d_primStart, primStart.data(), (size_t)G + 1); stage(d_geometry, g.geometry, G); stage(d_meshInfo, g.mesh_info, M);
      HIP_CHECK(hipMemsetAsync(R.d_err, 0, sizeof(uint32_t), stream));
      hipLaunchKernelGGL(canon_prim_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, d_primStart, G, d_geometry, d_meshInfo, matIDs, tris, B.d_canon, R.d_err);
      hipLaunchKernelGGL(canon_first_vertex_kernel, dim3((G + 255) / 256), dim3(256), 0, stream, G, d_geometry, d_meshInfo, firstVertex);
      HIP_CHECK(hipGetLastError());
      depth = rebuildPasses(S, R, B, ds, stream, fn, false);
    } else {
      // an empty scene: no node, no record; the tables of no height
      if (G) {
        mi_geom_ref* d_geometry; mi_mesh_info* d_meshInfo;
        stage(d_geometry, g.geometry, G); stage(d_meshInfo, g.mesh_info, M);
        hipLaunchKernelGGL(canon_first_vertex_kernel, dim3((G + 255) / 256), dim3(256), 0, stream, G, d_geometry, d_meshInfo, firstVertex);
        HIP_CHECK(hipGetLastError());
      }
      HIP_CHECK(hipStreamSynchronize(stream));
      R.levelStart.assign(2, 0u);
      refitTopFirst(R);
      R.tables = true; R.live = 0;
    }
    // nothing old goes before the work the scene had enqueued on it, on any stream, has finished
    for (LaunchSlot& l : S.slots) HIP_CHECK(hipEventSynchronize(l.lastWork));
  } catch (...) {
    (void)hipStreamSynchronize(stream);
    for (void* p : staged) (void)hipFree(p);
    for (size_t k = mark; k < S.allocations.size(); ++k) (void)hipFree(S.allocations[k]);
    S.allocations.resize(mark);
    throw;
  }
  for (void* p : staged) (void)hipFree(p);
  // the swap: the old set's buffers, then the scene's pointers
  const DeviceScene& o = S.ds;
  const mi_scene::Refit& oR = S.refit;
  std::vector<const void*> old = {o.nodes, o.leaves, o.leavesRot, o.matIDs, o.materials, o.leafNormalsOrFrames, o.meshTris, o.meshNormals, o.geomFirstVertex,
                                  oR.d_prims, oR.d_order, oR.d_boxes, oR.d_cnodes[0], oR.d_cnodes[1], oR.d_levelStart, oR.d_verts, oR.d_spheres, oR.d_discs,
                                  S.rebuild.d_canon, S.live.d_cost,
                                  S.hot.nodes, S.hot.leaves, S.hot.rot, S.hot.leafNormals,
                                  S.thin.nodes, S.thin.leaves, S.thin.rot, S.thin.leafNormals};      // (the private copies were the old contents')
  if (B.d_primBoxes != S.rebuild.d_primBoxes) for (void* p : rebuildScratchBuffers(S.rebuild)) old.push_back(p);
  for (const void* p : old) S.release(p);
  S.hot = mi_scene::HotCopy{};
  S.thin = mi_scene::HotCopy{};
  S.touchArrays() = ds;
  S.refit = std::move(R);
  S.rebuild = B;
  S.live.d_cost = nullptr;                       // (sized for the old node count: sceneCost allocates it again)
  poseDrop(S);                                   // (the rest snapshot and the poses were the old contents')
  S.live.maxLeafDepth = depth;
  ++S.live.geometrySets;
  rebuildBaseline(S, stream);
  return depth;
}

// Slots per pixel per launch in NIF renders: 48 B each (u, v, bgr, colour, throughput, list entry), and TWO sets of them when
// the render has more than one sample batch and the overlap is on (nif_overlap). A launch holds whole segments (ray_math.h
// segment_samples); more samples per launch mean more (pixel, segment) atoms per lane and fewer launch tails: 128 by
// default, fewer when n x samples x 48 B x sets would pass the budget - 32 GiB or half of what the device has free (plus
// what this scene already holds), whichever is less (the 1440^2 frame at 128 samples and two sets takes 25.5 GB) -, never
// less than one segment; if two sets of one segment do not fit, the render runs with one (no overlap). Option "nif_spl"
// overrides the sample count (1..128, rounded up to whole segments). None of this changes a result bit (the accumulate
// pass replays the reference's order whatever the batching: test_nif_render_sample_batching_is_order_exact).
// slot-mode (NIF) launches: at most this many workgroups, each wave of which may leave kEnvChunk - 1 padded entries in the escaped-slot list
constexpr uint32_t kMaxSlotWorkgroups = 4096;

void ensureScratch(mi_scene& S, size_t n) {
  {
    const uint32_t asked = S.opt.nifSamplesPerLaunch;
    const uint32_t segLen = segment_samples(S.ds.samplesPerPixel);
    uint32_t v = (asked >= 1 && asked <= kNifSplMax) ? asked : kNifSplDefault;
    v = ((v + segLen - 1) / segLen) * segLen;
    v = std::min(v, std::max(segLen, ((S.ds.samplesPerPixel + segLen - 1) / segLen) * segLen));      // no more than the render has
    const bool haveTwo = S.nifSlots[1].u != nullptr;
    auto setsFor = [&](uint32_t vv) { return (S.nifOverlapOn() && S.ds.samplesPerPixel > vv) ? 2u : 1u; };
    constexpr uint64_t kSlotBytes = 48;
    uint64_t budget = (uint64_t)64 << 30;
    {
      size_t freeB = 0, totalB = 0;
      if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
        const uint64_t held = (uint64_t)S.scratchRays * S.scratchSamples * kSlotBytes * (haveTwo ? 2u : 1u);
        budget = std::min<uint64_t>(budget, ((uint64_t)freeB + held) / 2);
      } else (void)hipGetLastError();
    }
    if (!(asked >= 1 && asked <= kNifSplMax))
      while (v > segLen && (uint64_t)n * v * kSlotBytes * setsFor(v) > budget) v -= segLen;
    const bool oneSetOnly = setsFor(v) == 2u && (uint64_t)n * v * kSlotBytes * 2u > budget;      // two sets of the smallest launch do not fit
    // keep what is there when it still fits this stream and the request has not changed
    if (S.scratchRays >= n && S.scratchAsked == asked && S.scratchSamples >= segLen && S.scratchSamples % segLen == 0 &&
        (haveTwo || oneSetOnly || !(S.nifOverlapOn() && S.ds.samplesPerPixel > S.scratchSamples))) return;
    S.scratchAsked = asked;
    S.scratchOneSet = oneSetOnly;
    if (v != S.scratchSamples || (!haveTwo && !oneSetOnly && S.nifOverlapOn() && S.ds.samplesPerPixel > v)) { S.scratchSamples = v; S.scratchRays = 0; }     // slot buffers are sized for n x v (x two sets)
  }
  if (S.scratchRays >= n) return;
  if (S.nifPending) { HIP_CHECK(hipDeviceSynchronize()); S.nifPending = false; }      // an earlier NIF render may still read the old buffers
  if (S.d_rng) (void)hipFree(S.d_rng);
  if (S.d_segTotal) (void)hipFree(S.d_segTotal);
  S.freeNifSlots();
  S.d_rng = nullptr; S.d_segTotal = nullptr; S.scratchRays = 0;
  const size_t slots = n * S.scratchSamples;
  HIP_CHECK(hipMalloc(&S.d_rng, n * sizeof(Rng)));
  HIP_CHECK(hipMalloc(&S.d_segTotal, 3 * n * sizeof(float)));
  // the second set only where it is used: renders of more than one sample batch with the overlap on
  const int sets = (S.nifOverlapOn() && S.ds.samplesPerPixel > S.scratchSamples && !S.scratchOneSet) ? 2 : 1;
  for (int k = 0; k < sets; ++k) {
    mi_scene::NifSlots& q = S.nifSlots[k];
    HIP_CHECK(hipMalloc(&q.u, slots * sizeof(float)));
    HIP_CHECK(hipMalloc(&q.v, slots * sizeof(float)));
    HIP_CHECK(hipMalloc(&q.bgr, 3 * slots * sizeof(float)));
    HIP_CHECK(hipMalloc(&q.color, 3 * slots * sizeof(float)));
    HIP_CHECK(hipMalloc(&q.tp, 3 * slots * sizeof(float)));
    // (every wave of a slot-mode launch pads the list to a whole chunk: trace_wavefront.hpp pushEscaped, kMaxSlotWorkgroups)
    HIP_CHECK(hipMalloc(&q.index, (slots + (size_t)kMaxSlotWorkgroups * 4u * kEnvChunk) * sizeof(uint32_t)));
    if (!q.count) HIP_CHECK(hipMalloc(&q.count, sizeof(uint32_t)));
    if (!q.traced) HIP_CHECK(hipEventCreateWithFlags(&q.traced, hipEventDisableTiming));
    if (!q.done) HIP_CHECK(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
  }
  S.scratchRays = n;
}

[[maybe_unused]] constexpr uint32_t kLdsBudgetBytes = 160 * 1024 - 2048 - 23 * 1024 * 4;     // 160 KiB per CU minus the static allocations (sin table, material cache, 23 cold-state words x 1024 threads)

// Work indices are 32 bit and every wave takes them from the launch's counter in chunks of fetchChunk (64): a wave
// that finds the counter past the end still adds its chunk, so the counter may overshoot the item count by
// (waves of the grid) x fetchChunk. Launches stay below 2^32 minus that headroom (2048 workgroups x 16 waves x 64,
// rounded up), so the counter never wraps.
constexpr uint64_t kMaxWorkItems = 0xFFFFFFFFull - ((uint64_t)1 << 22);

template <bool STATS>
void launchWavefront(mi_scene& S, mi_trace_result* d_rays, uint32_t cnt, hipStream_t stream, const WaveExtras& ex = WaveExtras{}, uint32_t wgCap = 0, uint32_t unitsHere = 0) {
  LaunchSlot& slot = S.slotFor(stream);
  const uint32_t units = unitsHere ? unitsHere : S.cus();      // (a CU-masked stream: the units of its mask)
  uint32_t* workCounter = slot.d_workCounter;
  const DeviceScene dsv = S.view();
  // Streams are walked in 8x8 pixel tiles of window-width rows (a whole window, a batch of it, or one rank's
  // 8-row bands are all sequences of full rows); the walk is only a work ORDER, any stream stays correct.
  const uint32_t w = (uint32_t)S.params.window_w;
  const uint32_t tileW = (S.opt.tiles && w >= 8 && (w % 8) == 0 && cnt >= 8u * w) ? w : 0u;
  const bool plain = ex.slotColor == nullptr;      // NIF launches leave slots instead of partial sums (kernels 1 and 3 take them; kernel 2 falls through to kernel 1)
  // Pixels with more than segment_samples(spp) samples are traced as (pixel, segment) work atoms (ray_math.h); every
  // stream has its own partial-sum buffer (LaunchSlot).
  const uint32_t segLen = segment_samples(S.ds.samplesPerPixel);
  const uint32_t segments = (S.ds.samplesPerPixel + segLen - 1) / segLen;
  const bool segmented = plain && segments > 1;
  // One launch covers as many segments of every pixel as the partial-sum budget holds (8 GiB, option "seg_budget_kb";
  // the bench frame needs 0.4 GB); longer renders run as several launches whose combine passes continue
  // the running sum in segment order, so the cut never shows in the result.
  uint32_t perLaunch = segments;
  if (segmented) {
    const size_t budgetFloats = S.opt.segBudgetKb * (size_t)(1024 / sizeof(float));
    const uint64_t byBudget = std::max<uint64_t>(1, budgetFloats / ((uint64_t)3 * cnt));
    const uint64_t byIndex = std::max<uint64_t>(1, kMaxWorkItems / cnt);           // work indices are 32-bit
    perLaunch = (uint32_t)std::min<uint64_t>(segments, std::min(byBudget, byIndex));
    const size_t need = (size_t)3 * cnt * perLaunch;
    if (slot.segPartFloats < need) {
      if (slot.d_segPart) { HIP_CHECK(hipStreamSynchronize(stream)); (void)hipFree(slot.d_segPart); }
      slot.d_segPart = nullptr; slot.segPartFloats = 0;
      HIP_CHECK(hipMalloc(&slot.d_segPart, need * sizeof(float)));
      slot.segPartFloats = need;
    }
  }
  const uint32_t launches = segmented ? (segments + perLaunch - 1) / perLaunch : 1u;
  // (pixel, segment) atoms fetch a pixel's coordinates once per segment: from a compact copy, gathered here
  const float2* coords = nullptr;
  if ((segmented || !plain) && S.opt.coords) {
    if (slot.coordsCap < cnt) {
      if (slot.d_coords) { HIP_CHECK(hipStreamSynchronize(stream)); (void)hipFree(slot.d_coords); }
      slot.d_coords = nullptr; slot.coordsCap = 0;
      HIP_CHECK(hipMalloc(&slot.d_coords, (size_t)cnt * sizeof(float2)));
      slot.coordsCap = cnt;
    }
    hipLaunchKernelGGL(pixel_coords_kernel, dim3((cnt + 255) / 256), dim3(256), 0, stream, d_rays, cnt, slot.d_coords);
    coords = slot.d_coords;
  }
  // Which build of K1w (k1w_builds.hpp select_k1w), from the launch, the scene and its options. The HOT builds take plain renders while the scene's private
  // copies stand for the shared arrays (mi_scene::touchArrays): the plain ones walk the collapsed copy (mi_scene::thin), the instrumented one the copy of every node.
  K1wChoice choice{};
  choice.variants = MI_RAYLIB_VARIANTS != 0; choice.stats = STATS; choice.slots = !plain;
  choice.hasNormals = S.ds.hasNormals != 0; choice.rotLeaves = S.ds.leavesRot != nullptr; choice.hasNodes = S.ds.numNodes > 0;
  choice.hotOn = S.opt.hotNodes != 0 && (STATS ? S.hot.valid : S.thin.valid) && S.ds.numNodes > 0;
  choice.doubleFallback = S.opt.doubleFallback; choice.fast = S.opt.fast; choice.specLeaf = S.opt.specLeaf; choice.mergeTurns = S.opt.mergeTurns;
  choice.leanHit = S.opt.leanHit; choice.leafRot = S.opt.leafRot; choice.kernelChoice = S.opt.kernelChoice; choice.wavesPerSimd = S.opt.wavesPerSimd;
  choice.defaultWeights = S.opt.tune == kDefaultTune;
#if MI_RAYLIB_VARIANTS
  choice.poolFits = S.ds.samplesPerPixel <= kPoolMaxSamples && S.ds.maxPathLength <= kPoolMaxBounces;
#endif
  const K1wId picked = select_k1w(choice);
  // (the tolerance tier - never the default - has plain, un-instrumented launches only; mi_scene_set_option refuses the other combinations it has no build for)
  if (picked == K1wId::RefusedFast) throw ArgError("mi_render: the tolerance tier (option fast) has no NIF / instrumented build; clear the option for this render");
  for (uint32_t l = 0; l < launches; ++l) {
    const uint32_t segBase = l * perLaunch;
    WaveExtras exs = ex;
    exs.coords = coords;
    if (segmented) { exs.segPart = slot.d_segPart; exs.segments = std::min(perLaunch, segments - segBase); exs.segBase = segBase; }
    HIP_CHECK(hipMemsetAsync(workCounter, 0, sizeof(uint32_t), stream));
    const uint64_t items = (uint64_t)cnt * ((segmented || !plain) ? exs.segments : 1u);     // work atoms of this launch
    if (items > kMaxWorkItems) throw ArgError("mi_render: too many work items for one launch (cut the stream with mi_scene_set_ray_batch)");
    // Grid: persistent workgroups, as many as stay resident (compute units x workgroups per unit, asked of the runtime for
    // the kernel about to be launched and remembered per scene), never more than the launch has work for.
    auto grid = [&](auto kern, uint32_t threads, size_t ldsBytes) {
      uint32_t perUnit = S.residentBlocks(reinterpret_cast<const void*>(kern), (int)threads, ldsBytes);
      if (wgCap) perUnit = std::min(perUnit, wgCap);      // (NIF renders: a trace launch that runs beside the previous batch's MLP)
      uint64_t wgs = std::min<uint64_t>((items + threads - 1) / threads, (uint64_t)units * perUnit);
      if (!plain) wgs = std::min<uint64_t>(wgs, kMaxSlotWorkgroups);      // (the escaped-slot list has padding for that many)
      return (uint32_t)wgs;
    };
    auto go = [&](auto kern, const char* name) {
      if (S.opt.sayGrid) fprintf(stderr, "mi_raylib: grid %u workgroups = %u units x %u resident, build %s\n", grid(kern, 256, 0), units, S.residentBlocks(reinterpret_cast<const void*>(kern), 256, 0), name);
      hipLaunchKernelGGL(kern, dim3(grid(kern, 256, 0)), dim3(256), 0, stream, dsv, d_rays, cnt, workCounter, 0u, S.opt.tune, tileW, exs);
    };
    // Option "hot_nodes": the HOT builds stage the first nodes of the private copy they walk in dynamic LDS - as many as asked for, as the copy
    // has, and as fit without costing a resident workgroup. false = nothing launched (no node fits, or `auto` declines).
    auto goHot = [&](auto kern, uint32_t threads, const char* name) -> bool {
      const mi_scene::HotCopy& copy = STATS ? S.hot : S.thin;
      const uint32_t room = S.hotRoom(reinterpret_cast<const void*>(kern), (int)threads);
      const uint32_t count = std::min(std::min(S.opt.hotNodes < 0 ? ~0u : (uint32_t)S.opt.hotNodes, copy.thinNodes), room / (uint32_t)sizeof(GNode));
      if (!count) return false;
      if (S.opt.hotNodes < 0) {
        // auto: decided from the prefix the plain build of this scene's kind stages, whichever build is being launched (the instrumented one has room for more)
        const uint32_t plainRoom = S.ds.hasNormals ? S.hotRoom(reinterpret_cast<const void*>(path_trace_wavefront_kernel<K1wHotBary>), K1wHotBary::block)
                                                   : S.hotRoom(reinterpret_cast<const void*>(path_trace_wavefront_kernel<K1wHotRot>), K1wHotRot::block);
        const uint32_t ref = std::min(S.thin.thinNodes, plainRoom / (uint32_t)sizeof(GNode));
        if (!ref || S.thin.share[ref - 1] < kHotAutoShare) return false;
      }
      const uint32_t wgs = grid(kern, threads, room);
      if (S.opt.sayGrid) fprintf(stderr, "mi_raylib: grid %u workgroups of %u threads, %u hot nodes of %u that fit, build %s\n", wgs, threads, count, room / (uint32_t)sizeof(GNode), name);
      hipLaunchKernelGGL(kern, dim3(wgs), dim3(threads), (size_t)count * sizeof(GNode), stream, S.hotView(copy), d_rays, cnt, workCounter, count, S.opt.tune, tileW, exs);
      return true;
    };
    auto launch = [&](K1wId id) -> bool {      // false: a HOT build that launched nothing
      bool launched = true;
      const bool has = with_k1w<MI_RAYLIB_VARIANTS != 0>(id, [&](auto build) {
        using B = decltype(build);
        auto kern = path_trace_wavefront_kernel<B>;
        if constexpr (B::hot) launched = goHot(kern, B::block, k1w_name(id));
        else if constexpr (B::ldsNodes) {
          // kernel 2: one 1024-thread workgroup per CU shares one LDS copy of the first nodes of the (preorder) array
          const uint32_t ldsNodes = std::min<uint32_t>(S.ds.numNodes, kLdsBudgetBytes / (uint32_t)sizeof(GNode));
          if (!S.ldsAttrSet[B::stats ? 1 : 0]) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudgetBytes));
            S.ldsAttrSet[B::stats ? 1 : 0] = true;
          }
          const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + 1023) / 1024, S.cus());
          hipLaunchKernelGGL(kern, dim3(blocks), dim3(B::block), (size_t)ldsNodes * sizeof(GNode), stream, S.view(), d_rays, cnt, workCounter, ldsNodes, S.opt.tune, tileW, exs);
        } else go(kern, k1w_name(id));
      });
      if (!has) throw std::logic_error(std::string("mi_render: this library has no build ") + k1w_name(id));      // (nothing select_k1w returns for it: tests/test_k1w_builds.py)
      return launched;
    };
    if (picked == K1wId::PathPool) {
#if MI_RAYLIB_VARIANTS
      // path pool (trace_pool.hpp): persistent, exactly as many workgroups as stay resident; a workgroup of W waves
      // owns 100 W path slots
      const uint32_t W = (uint32_t)S.opt.poolWaves, pwg = 100u * W;
      const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + pwg - 1) / pwg, (uint64_t)S.cus() * (16u / W));
      const uint32_t stride = blocks * pwg;
      const size_t need = (size_t)PG_WORDS * stride;
      if (slot.poolScratchWords < need) {
        if (slot.d_poolScratch) { HIP_CHECK(hipStreamSynchronize(stream)); (void)hipFree(slot.d_poolScratch); }
        slot.d_poolScratch = nullptr; slot.poolScratchWords = 0;
        HIP_CHECK(hipMalloc(&slot.d_poolScratch, need * sizeof(uint32_t)));
        slot.poolScratchWords = need;
      }
      const size_t ldsBytes = pool_lds_bytes(pwg);
      auto goPool = [&](auto kern, int which) {
        if (!S.poolAttrSet[STATS ? 1 : 0][which]) {
          HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
          S.poolAttrSet[STATS ? 1 : 0][which] = true;
        }
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * W), ldsBytes, stream, S.view(), d_rays, cnt, workCounter, S.opt.poolTune, tileW, exs, slot.d_poolScratch, stride);
      };
      if (W == 4) goPool(path_trace_pool_kernel<STATS, 4, 400, 4>, 0);
      else if (W == 8) goPool(path_trace_pool_kernel<STATS, 8, 800, 4>, 1);
      else goPool(path_trace_pool_kernel<STATS, 16, 1600, 4>, 2);
#endif
    } else if (!launch(picked)) {      // a HOT build that launched nothing: what the selection says without hot nodes
      choice.hotOn = false;
      launch(select_k1w(choice));
    }
    if (segmented) hipLaunchKernelGGL(segment_combine_kernel, dim3((cnt + 255) / 256), dim3(256), 0, stream, d_rays, cnt, exs.segments, slot.d_segPart, segBase ? 1u : 0u);
  }
}

// Option "nif_split": the two CU-masked streams of a NIF render (made once per value; 0 = none, also when the runtime refuses
// masked streams - said once on stderr: the render then shares the chip between its launches as without the option).
// Returns the units the trace stream owns.
uint32_t splitStreams(mi_scene& S) {
  const uint32_t N = (uint32_t)S.numCUs;
  uint32_t x = S.opt.nifSplit;
  if (x == 0 || S.splitRefused) return 0;
  if (x > N / 2) x = N / 2;
  if (S.splitUnits == x) return x;
  for (hipStream_t* q : {&S.nifSplitMlp, &S.nifSplitTrace}) if (*q) { (void)hipStreamSynchronize(*q); (void)hipStreamDestroy(*q); *q = nullptr; }
  S.splitUnits = 0;
  std::vector<uint32_t> lo((N + 31) / 32, 0u), hi((N + 31) / 32, 0u);
  for (uint32_t i = 0; i < N; ++i) (i < N - x ? lo : hi)[i / 32] |= 1u << (i % 32);
  const hipError_t e0 = hipExtStreamCreateWithCUMask(&S.nifSplitMlp, (uint32_t)lo.size(), lo.data());
  const hipError_t e1 = e0 == hipSuccess ? hipExtStreamCreateWithCUMask(&S.nifSplitTrace, (uint32_t)hi.size(), hi.data()) : e0;
  if (e1 != hipSuccess) {
    (void)hipGetLastError();
    if (S.nifSplitMlp) { (void)hipStreamDestroy(S.nifSplitMlp); S.nifSplitMlp = nullptr; }
    S.nifSplitTrace = nullptr; S.splitRefused = true;
    fprintf(stderr, "mi_raylib: option nif_split: no compute-unit masked streams here (%s); the render's launches share the chip\n", hipGetErrorString(e1));
    return 0;
  }
  if (!S.splitFirst) HIP_CHECK(hipEventCreateWithFlags(&S.splitFirst, hipEventDisableTiming));
  S.splitUnits = x;
  return x;
}

void launchRender(mi_scene& S, int mode, mi_trace_result* d_rays, size_t n, hipStream_t stream) {
  if (n == 0) return;
  if (n > 0xFFFFFFFFull) throw ArgError("mi_render: more than 2^32-1 rays in one call");
  const uint32_t cnt = (uint32_t)n;
  const dim3 block(256), grid((cnt + 255) / 256);
  if (mode == MI_MODE_SHADOW_TRACE) {
    const f3 light = mk(18.f, 257.f, -1060.f);          // trace.cpp:247, src/IpuScene.cpp:447
    if (S.opt.doubleFallback) hipLaunchKernelGGL((shadow_trace_kernel<false, true>), grid, block, 0, stream, S.view(), d_rays, cnt, .05f, light);
    else if (S.opt.fullStats) hipLaunchKernelGGL(shadow_trace_kernel<true>, grid, block, 0, stream, S.view(), d_rays, cnt, .05f, light);
    else hipLaunchKernelGGL(shadow_trace_kernel<false>, grid, block, 0, stream, S.view(), d_rays, cnt, .05f, light);
  } else if (mode == MI_MODE_PATH_TRACE) {
    // (the ALLOW_DOUBLE_FALLBACK=1 variant is compiled into the phase-scheduled kernel and the shadow kernel: it always takes them)
    // (the phase-scheduled kernel keeps a path's bounce count in 30 bits)
    const bool nested = (S.opt.kernelChoice == 0 || S.ds.maxPathLength >= (1u << 30)) && !S.opt.doubleFallback;
    if (!S.nif.loaded() && !nested && S.ds.samplesPerPixel >= 1 && S.ds.maxPathLength >= 1) {
      // sample loop inside the kernel (src/IpuScene.cpp:441), phase-scheduled persistent form
      if (S.opt.fullStats) launchWavefront<true>(S, d_rays, cnt, stream);
      else launchWavefront<false>(S, d_rays, cnt, stream);
    } else if (!S.nif.loaded()) {
      // sample loop inside the kernel (src/IpuScene.cpp:441: vertexSampleCount = samplesPerPixel)
      if (S.opt.fullStats) hipLaunchKernelGGL(path_trace_kernel<true>, grid, block, 0, stream, S.view(), d_rays, cnt, 0u, S.ds.samplesPerPixel, (Rng*)nullptr);
      else hipLaunchKernelGGL(path_trace_kernel<false>, grid, block, 0, stream, S.view(), d_rays, cnt, 0u, S.ds.samplesPerPixel, (Rng*)nullptr);
    } else {
      // Repeat(spp){ trace 1 sample; uv pre-pass; NIF; env post-pass }  (src/IpuScene.cpp:571-583)
      // NIF renders of one scene share its slot scratch: whatever streams they are enqueued on, each waits for the
      // previous one (and a scratch re-allocation waits for the device)
      if (!S.nifDone) HIP_CHECK(hipEventCreateWithFlags(&S.nifDone, hipEventDisableTiming));
      if (S.nifPending) HIP_CHECK(hipStreamWaitEvent(stream, S.nifDone, 0));
      ensureScratch(S, n);
      const float radians = (S.hdriRotationDegrees / 360.f) * (float)(2.0 * M_PI);   // src/IpuScene.cpp:644
      const bool wave = !nested && S.ds.maxPathLength >= 1;
      if (wave) {
        // persistent phase-scheduled kernel, several samples per launch; every path leaves a slot (WaveExtras), the
        // MLP runs on the compacted escaped slots, and a per-pixel pass adds everything in the reference's order
        if ((uint64_t)cnt * S.scratchSamples > kMaxWorkItems) throw ArgError("mi_render: ray batch too large for a NIF render (cut it with mi_scene_set_ray_batch)");
        const uint32_t segLen = segment_samples(S.ds.samplesPerPixel), segShift = segment_shift(S.ds.samplesPerPixel);
        // Sample batch b: trace its slots on `stream` (set b & 1), then MLP over the compacted escaped slots + the accumulate
        // pass - on nifAux when there are two sets, so that the trace launch of batch b + 1 runs beside them. The accumulate
        // passes run in batch order on one stream and touch only rgb; the trace launch only reads the pixel coordinates and
        // writes the hit record of the same TraceResults (other dwords), so the two never meet. A set is traced into again
        // only when the MLP + accumulate that read it are done; the render's stream ends behind the last of them.
        const bool two = S.nifOverlapOn() && S.nifSlots[1].u != nullptr;
        if (two && !S.nifAux) HIP_CHECK(hipStreamCreateWithFlags(&S.nifAux, hipStreamNonBlocking));
        // Option "nif_split" = x: the trace launches of batches 1.. run on x compute units of their own and the MLP + accumulate
        // passes on the other numCUs - x (two CU-masked streams), instead of sharing the chip. Batch 0's trace launch has the
        // device to itself and stays on the render's stream, which the masked trace stream follows (an event) and which
        // follows both again when the render ends. Only the SCHEDULE changes: same kernels, same buffers, same order per buffer.
        const uint32_t splitX = (two && S.opt.cus == 0 && S.ds.samplesPerPixel > 2u * S.scratchSamples) ? splitStreams(S) : 0u;
        hipStream_t mlpStream = splitX ? S.nifSplitMlp : two ? S.nifAux : stream;
        // (the MLP keeps its grid of one workgroup per unit of the whole chip: a mask that leaves the shader engines unequal - any x that
        // is not a multiple of their number - still gets the same share of workgroups per engine from the dispatcher, and with a grid
        // of only numCUs - x some units of the fuller engines would idle. The workgroups that find no unit free start when the first
        // ones leave, and leave at once: passes are drawn, nif_asm_kernel.hpp)
        const uint32_t mlpUnits = S.cus();
        uint32_t b = 0;
        mi_scene::NifSlots* pendQ = nullptr; uint32_t pendSc = 0, pendSegBase = 0;      // (nif_split: the batch whose accumulate pass is still to be enqueued)
        auto flushAccumulate = [&](hipStream_t on) {
          if (!pendQ) return;
          HIP_CHECK(hipStreamWaitEvent(on, pendQ->done, 0));
          hipLaunchKernelGGL(nif_accumulate_kernel, grid, block, 0, on, d_rays, cnt, pendSc, segShift, pendSegBase, pendQ->color, pendQ->tp, pendQ->u, pendQ->bgr);
          pendQ = nullptr;
        };
        try {
        for (uint32_t s0 = 0; s0 < S.ds.samplesPerPixel; s0 += S.scratchSamples, ++b) {
          mi_scene::NifSlots& q = S.nifSlots[two ? (b & 1u) : 0u];
          const uint32_t sc = std::min<uint32_t>(S.scratchSamples, S.ds.samplesPerPixel - s0);
          hipStream_t ts = (splitX && b > 0) ? S.nifSplitTrace : stream;          // this batch's trace launch
          if (splitX && b == 1) { HIP_CHECK(hipEventRecord(S.splitFirst, stream)); HIP_CHECK(hipStreamWaitEvent(ts, S.splitFirst, 0)); }
          if (two && q.donePending) { HIP_CHECK(hipStreamWaitEvent(ts, q.done, 0)); q.donePending = false; }
          HIP_CHECK(hipMemsetAsync(q.count, 0, sizeof(uint32_t), ts));
          WaveExtras ex;
          ex.sampleCount = sc; ex.segments = (sc + segLen - 1) / segLen; ex.segBase = s0 / segLen;     // (pixel, segment) atoms
          ex.u = q.u; ex.v = q.v; ex.slotColor = q.color; ex.slotTp = q.tp;
          ex.index = q.index; ex.count = q.count; ex.azimuthRotation = radians;
          ex.firstInSetup = S.opt.nifFirstTest ? 1u : 0u;
          const uint32_t wgCap = (two && b > 0 && !splitX) ? S.opt.nifTraceWgs : 0u;       // batch 0 has the device to itself
          const uint32_t unitsHere = (splitX && b > 0) ? splitX : 0u;
          if (S.opt.fullStats) launchWavefront<true>(S, d_rays, cnt, ts, ex, wgCap, unitsHere);
          else launchWavefront<false>(S, d_rays, cnt, ts, ex, wgCap, unitsHere);
          if (two) { HIP_CHECK(hipEventRecord(q.traced, ts)); HIP_CHECK(hipStreamWaitEvent(mlpStream, q.traced, 0)); }
          if (splitX) flushAccumulate(ts);
          std::pair<hipEvent_t, hipEvent_t> tm{nullptr, nullptr};
          if (S.opt.nifTiming) { HIP_CHECK(hipEventCreate(&tm.first)); HIP_CHECK(hipEventCreate(&tm.second)); S.nifTimes.push_back(tm); HIP_CHECK(hipEventRecord(tm.first, mlpStream)); }
          nif_launch_mlp(S.nif, q.u, q.v, q.index, q.count, cnt * sc, q.bgr, nullptr, mlpStream, true, S.opt.nifShape, mlpUnits, S.opt.nifGenerations);
          if (tm.second) HIP_CHECK(hipEventRecord(tm.second, mlpStream));
          if (splitX) {
            // the accumulate pass of this batch goes BEHIND the next batch's trace launch on the trace stream (which idles there until
            // the MLP is done; the set is traced into again only after it, by stream order): the MLP stream runs MLPs back to back
            HIP_CHECK(hipEventRecord(q.done, mlpStream));
            pendQ = &q; pendSc = sc; pendSegBase = ex.segBase;
          } else {
            hipLaunchKernelGGL(nif_accumulate_kernel, grid, block, 0, mlpStream, d_rays, cnt, sc, segShift, ex.segBase, q.color, q.tp, q.u, q.bgr);
            if (two) { HIP_CHECK(hipEventRecord(q.done, mlpStream)); q.donePending = true; }
          }
        }
        if (splitX) {
          flushAccumulate(b > 1 ? S.nifSplitTrace : stream);
          if (b > 1) { HIP_CHECK(hipEventRecord(S.splitFirst, S.nifSplitTrace)); HIP_CHECK(hipStreamWaitEvent(stream, S.splitFirst, 0)); }
        }
        if (two) for (mi_scene::NifSlots& q : S.nifSlots) if (q.donePending) { HIP_CHECK(hipStreamWaitEvent(stream, q.done, 0)); q.donePending = false; }
        } catch (...) {
          // a launch or a HIP call failed with MLP / accumulate passes queued on nifAux: they write the caller's rgb, so the
          // error must not return while they run behind the caller's stream (mi_render_device) - wait for them here
          if (two) { (void)hipStreamSynchronize(S.nifAux); for (mi_scene::NifSlots& q : S.nifSlots) q.donePending = false; }
          if (splitX) { (void)hipStreamSynchronize(S.nifSplitTrace); (void)hipStreamSynchronize(S.nifSplitMlp); }
          throw;
        }
      } else {
        const uint32_t segLen = segment_samples(S.ds.samplesPerPixel);
        for (uint32_t s = 0; s < S.ds.samplesPerPixel; ++s) {
          // a new segment: the finished ones move to the running total, rgb restarts from zero
          if (s != 0 && s % segLen == 0) hipLaunchKernelGGL(nif_segment_roll_kernel, grid, block, 0, stream, d_rays, S.d_segTotal, cnt, s / segLen, 0u);
          if (S.opt.fullStats) hipLaunchKernelGGL(path_trace_kernel<true>, grid, block, 0, stream, S.view(), d_rays, cnt, s, 1u, S.d_rng);
          else hipLaunchKernelGGL(path_trace_kernel<false>, grid, block, 0, stream, S.view(), d_rays, cnt, s, 1u, S.d_rng);
          nif_env_pass(S.nif, d_rays, cnt, radians, S.nifSlots[0].u, S.nifSlots[0].v, S.nifSlots[0].bgr, S.maxNifBatch, stream, S.opt.nifShape, S.cus(), S.opt.nifGenerations);
        }
        if (S.ds.samplesPerPixel > segLen) hipLaunchKernelGGL(nif_segment_roll_kernel, grid, block, 0, stream, d_rays, S.d_segTotal, cnt, 0u, 1u);
      }
      HIP_CHECK(hipEventRecord(S.nifDone, stream));
      S.nifPending = true;
    }
  } else {
    throw ArgError("mi_render: unknown render mode");
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(S.slotFor(stream).lastWork, stream));      // (~mi_scene waits for it)
}

// One wave that samples the work counter of `hip_stream`'s persistent launches `n` times, `period_ticks` (100-MHz ticks) apart, into
// d_samples as pairs {s_memrealtime, counter}: how fast a launch hands its work units out over its life - the ramp at its start, the
// moment the queue runs empty, the drain behind it (tools/launch_progress.py). It runs on a stream of the scene's own beside the launch it
// watches (K1w leaves every SIMD room for it), ends after n samples whatever happens, and changes nothing it looks at.
__global__ void __launch_bounds__(64) launch_progress_kernel(const uint32_t* counter, unsigned long long* samples, uint32_t n, uint32_t periodTicks) {
  if (threadIdx.x != 0) return;
  unsigned long long next = __builtin_amdgcn_s_memrealtime();
  for (uint32_t i = 0; i < n; ++i) {
    unsigned long long now;
    uint32_t spins = 0;
    do { __builtin_amdgcn_s_sleep(32); now = __builtin_amdgcn_s_memrealtime(); } while (now < next && ++spins < (1u << 22));
    samples[2 * i] = now;
    samples[2 * i + 1] = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    next += periodTicks;
  }
}

}  // namespace

extern "C" {

const char* mi_last_error(void) { return g_err.c_str(); }

const char* mi_version(void) {
#if MI_RAYLIB_VARIANTS
  return "mi_raylib 0.1 gfx950 fp-contract=off (bit-exact to the reference CPU path) +variants";
#else
  return "mi_raylib 0.1 gfx950 fp-contract=off (bit-exact to the reference CPU path)";
#endif
}

int mi_scene_create(const mi_scene_desc* desc, mi_scene** out) {
  if (!desc || !out) { g_err = "mi_scene_create: null argument"; return MI_ERR_INVALID_ARG; }
  *out = nullptr;
  mi_scene* S = nullptr;
  const int rc = guarded([&] {
    int count = 0;
    HIP_CHECK(hipGetDeviceCount(&count));
    if (count <= 0) throw DeviceError("no HIP device available (the product path has no CPU fallback)");
    if (desc->device < 0 || desc->device >= count) throw ArgError("mi_scene_create: device ordinal out of range");
    HIP_CHECK(hipSetDevice(desc->device));
    S = new mi_scene;
    S->device = desc->device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, desc->device) == hipSuccess && cus > 0) S->numCUs = cus; }
    S->params = *desc;
    buildDeviceScene(*S, *desc);
    // the caller's arrays are not referenced after this point
    S->params.geometry = nullptr; S->params.mesh_info = nullptr; S->params.mesh_tris = nullptr; S->params.mesh_verts = nullptr;
    S->params.mesh_normals = nullptr; S->params.mat_ids = nullptr; S->params.materials = nullptr; S->params.bvh_nodes = nullptr;
    S->params.spheres = nullptr; S->params.discs = nullptr;
    S->opt.fromEnvironment();      // read once, into this scene (SceneOptions)
    S->live.maxLeafDepth = desc->max_leaf_depth;
  });
  if (rc != MI_OK) { delete S; return rc; }
  *out = S;
  return MI_OK;
}

int mi_scene_create_from_blob(const uint8_t* blob, size_t size, const mi_scene_desc* extras, mi_scene** out) {
  if (!blob || !extras || !out) { g_err = "mi_scene_create_from_blob: null argument"; return MI_ERR_INVALID_ARG; }
  *out = nullptr;
  mi_scene_desc d = *extras;                 // spheres/discs, rng seed, crop window, pathTrace, device
  std::vector<uint64_t> aligned;             // only used when the caller's bytes are not 16-byte aligned
  const int rc = guarded([&] {
    if ((uintptr_t)blob % 16) {
      aligned.resize((size + 23) / 8);
      uint8_t* a = (uint8_t*)aligned.data();
      a += (16 - (uintptr_t)a % 16) % 16;
      std::memcpy(a, blob, size);
      blob = a;
    }
    try { mi::blob::deserialiseScene(blob, size, d, 16); }          // views into the bytes; create copies them
    catch (const std::runtime_error& e) { throw ArgError(std::string("mi_scene_create_from_blob: ") + e.what()); }
  });
  if (rc != MI_OK) return rc;
  return mi_scene_create(&d, out);
}

void mi_scene_destroy(mi_scene* scene) { delete scene; }

int mi_scene_update_device(mi_scene* scene, const mi_geometry_update* device_arrays, void* hip_stream) {
  return guarded([&] {
    updateArgs("mi_scene_update_device", scene, device_arrays);
    HIP_CHECK(hipSetDevice(scene->device));
    refitScene(*scene, *device_arrays, (hipStream_t)hip_stream);
    poseInvalidate(*scene);
  });
}

int mi_scene_update(mi_scene* scene, const mi_geometry_update* host_arrays) {
  std::vector<void*> staged;
  const int rc = guarded([&] {
    updateArgs("mi_scene_update", scene, host_arrays);
    HIP_CHECK(hipSetDevice(scene->device));
    // the given arrays to the device, then the device entry's work on the null stream
    auto stage = [&](const void* p, size_t bytes) -> const void* {
      if (!p || !bytes) return p;
      void* d = nullptr;
      HIP_CHECK(hipMalloc(&d, bytes));
      staged.push_back(d);
      HIP_CHECK(hipMemcpy(d, p, bytes, hipMemcpyHostToDevice));
      return d;
    };
    mi_geometry_update u = *host_arrays;
    u.mesh_verts = (const mi_vec3*)stage(u.mesh_verts, (size_t)u.num_verts * sizeof(mi_vec3));
    u.mesh_normals = (const mi_vec3*)stage(u.mesh_normals, (size_t)u.num_normals * sizeof(mi_vec3));
    u.spheres = (const mi_sphere*)stage(u.spheres, (size_t)u.num_spheres * sizeof(mi_sphere));
    u.discs = (const mi_disc*)stage(u.discs, (size_t)u.num_discs * sizeof(mi_disc));
    refitScene(*scene, u, nullptr);
    poseInvalidate(*scene);
  });
  for (void* d : staged) (void)hipFree(d);
  return rc;
}

int mi_scene_set_poses_device(mi_scene* scene, const void* d_poses, uint32_t num_geometry, void* hip_stream) {
  return guarded([&] {
    poseArgs("mi_scene_set_poses_device", scene, d_poses, num_geometry);
    if (!num_geometry) return;
    if ((uintptr_t)d_poses % 16) throw ArgError("mi_scene_set_poses_device: poses must be 16-byte aligned");
    HIP_CHECK(hipSetDevice(scene->device));
    poseScene(*scene, (const mi_pose*)d_poses, nullptr, (hipStream_t)hip_stream, "mi_scene_set_poses_device");
  });
}

int mi_scene_set_poses(mi_scene* scene, const mi_pose* poses, uint32_t num_geometry) {
  return guarded([&] {
    poseArgs("mi_scene_set_poses", scene, poses, num_geometry);
    if (!num_geometry) return;
    // (the host can name the pose before a device is touched; the device entry's rule is the same function)
    for (uint32_t g = 0; g < num_geometry; ++g) {
      mi_pose p;
      memcpy(&p, &poses[g], sizeof p);
      if (!pose_valid(p.quat, p.translation, p.scale))
        throw ArgError("mi_scene_set_poses: pose " + std::to_string(g) + " is not valid (eight finite floats, a quaternion whose squared norm and its "
                       "reciprocal are finite and positive, scale > 0); the scene is unchanged");
    }
    HIP_CHECK(hipSetDevice(scene->device));
    // the given poses to the device, then the device entry's work on the null stream
    poseScene(*scene, nullptr, poses, nullptr, "mi_scene_set_poses");
  });
}

int mi_scene_get_poses(mi_scene* scene, mi_pose* out, uint32_t capacity, uint32_t* num_geometry) {
  if (!scene || !num_geometry) { g_err = "mi_scene_get_poses: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    const uint32_t G = (uint32_t)scene->refit.geometry.size();
    *num_geometry = G;
    if (!out || !G) return;
    if (capacity < G) throw ArgError("mi_scene_get_poses: capacity is smaller than the scene's geometry count");
    if (scene->poses.posed) {
      HIP_CHECK(hipSetDevice(scene->device));
      HIP_CHECK(hipMemcpy(out, scene->poses.d_poses, (size_t)G * sizeof(mi_pose), hipMemcpyDeviceToHost));
    } else {
      const mi_pose identity = {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 1.f};
      for (uint32_t g = 0; g < G; ++g) out[g] = identity;
    }
  });
}

int mi_scene_bake_poses(mi_scene* scene) {
  if (!scene) { g_err = "mi_scene_bake_poses: null scene"; return MI_ERR_INVALID_ARG; }
  poseInvalidate(*scene);
  g_err.clear();
  return MI_OK;
}

int mi_get_pose_timing(mi_scene* scene, double out[2]) {
  if (!scene || !out) { g_err = "mi_get_pose_timing: null argument"; return MI_ERR_INVALID_ARG; }
  for (int i = 0; i < 2; ++i) out[i] = scene->poses.ms[i];
  g_err.clear();
  return MI_OK;
}

int mi_scene_rebuild(mi_scene* scene, void* hip_stream, uint32_t* max_leaf_depth) {
  return guarded([&] {
    if (!scene) throw ArgError("mi_scene_rebuild: null scene");
    HIP_CHECK(hipSetDevice(scene->device));
    const uint32_t depth = rebuildScene(*scene, (hipStream_t)hip_stream);
    ++scene->live.rebuilds;
    if (max_leaf_depth) *max_leaf_depth = depth;
  });
}

int mi_scene_set_geometry_device(mi_scene* scene, const mi_scene_geometry* arrays, void* hip_stream, uint32_t* max_leaf_depth) {
  return guarded([&] {
    if (!scene) throw ArgError("mi_scene_set_geometry_device: null scene");
    if (!arrays) throw ArgError("mi_scene_set_geometry_device: null geometry");
    HIP_CHECK(hipSetDevice(scene->device));
    const uint32_t depth = setGeometry(*scene, *arrays, (hipStream_t)hip_stream, hipMemcpyDeviceToDevice, "mi_scene_set_geometry_device");
    if (max_leaf_depth) *max_leaf_depth = depth;
  });
}

int mi_scene_set_geometry(mi_scene* scene, const mi_scene_geometry* host_arrays, uint32_t* max_leaf_depth) {
  return guarded([&] {
    if (!scene) throw ArgError("mi_scene_set_geometry: null scene");
    if (!host_arrays) throw ArgError("mi_scene_set_geometry: null geometry");
    HIP_CHECK(hipSetDevice(scene->device));
    // the device entry's work on the null stream, the data plane uploaded straight into the buffers the scene will own
    const uint32_t depth = setGeometry(*scene, *host_arrays, nullptr, hipMemcpyHostToDevice, "mi_scene_set_geometry");
    if (max_leaf_depth) *max_leaf_depth = depth;
  });
}

int mi_scene_bvh_cost(mi_scene* scene, void* hip_stream, double out[3]) {
  if (!scene || !out) { g_err = "mi_scene_bvh_cost: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    if (scene->refit.live >= 0) HIP_CHECK(hipSetDevice(scene->device));
    sceneCost(*scene, (hipStream_t)hip_stream, out);
  });
}

int mi_get_live_stats(mi_scene* scene, uint64_t out[8]) {
  if (!scene || !out) { g_err = "mi_get_live_stats: null argument"; return MI_ERR_INVALID_ARG; }
  const mi_scene::Live& L = scene->live;
  const uint64_t v[8] = {L.applied, L.refused, L.rebuilds, L.autoRebuilds, L.hostDerivations, L.costEvals, L.maxLeafDepth, L.geometrySets};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  g_err.clear();
  return MI_OK;
}

int mi_get_rebuild_timing(mi_scene* scene, double out[6]) {
  if (!scene || !out) { g_err = "mi_get_rebuild_timing: null argument"; return MI_ERR_INVALID_ARG; }
  for (int i = 0; i < 6; ++i) out[i] = scene->rebuild.ms[i];
  g_err.clear();
  return MI_OK;
}

int mi_get_refit_timing(mi_scene* scene, double out[3]) {
  if (!scene || !out) { g_err = "mi_get_refit_timing: null argument"; return MI_ERR_INVALID_ARG; }
  for (int i = 0; i < 3; ++i) out[i] = scene->refit.ms[i];
  g_err.clear();
  return MI_OK;
}

int mi_scene_get_bvh(mi_scene* scene, mi_bvh_node* out, uint32_t capacity, uint32_t* num_nodes) {
  if (!scene || !num_nodes) { g_err = "mi_scene_get_bvh: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    const mi_scene::Refit& R = scene->refit;
    const uint32_t N = scene->ds.numNodes;
    *num_nodes = N;
    if (!out || !N) return;
    if (capacity < N) throw ArgError("mi_scene_get_bvh: capacity is smaller than the scene's node count");
    if (R.live >= 0) {
      HIP_CHECK(hipSetDevice(scene->device));
      HIP_CHECK(hipMemcpy(out, R.d_cnodes[R.live], (size_t)N * sizeof(mi_bvh_node), hipMemcpyDeviceToHost));
    } else if (N) {
      memcpy(out, R.nodes.data(), (size_t)N * sizeof(mi_bvh_node));
    }
  });
}

int mi_render_device(mi_scene* scene, int mode, void* d_rays, size_t n, void* hip_stream) {
  if (!scene || (!d_rays && n)) { g_err = "mi_render_device: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    launchRender(*scene, mode, (mi_trace_result*)d_rays, n, (hipStream_t)hip_stream);
  });
}

int mi_render(mi_scene* scene, int mode, mi_trace_result* rays, size_t n, mi_ray_callback cb, void* user) {
  if (!scene || (!rays && n)) { g_err = "mi_render: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    if (n == 0) { scene->traceTimeSecs = 0.0; return; }
    // Ray batches (src/IpuScene.cpp:110-172, 585-618): the stream is cut into batches of rayBatch rays that
    // flow through a two-slot pipeline — upload, trace and download of batch b+1 overlap the download and
    // the callback of batch b — each slot on its own HIP stream. Every pixel owns its RNG stream, so the
    // result does not depend on the batch size. The NIF path shares scratch buffers and runs one slot.
    const size_t batch = (scene->rayBatch && scene->rayBatch < n) ? scene->rayBatch : n;
    const size_t numBatches = (n + batch - 1) / batch;
    const int slots = (numBatches > 1 && !scene->nif.loaded()) ? 2 : 1;
    // The two device batch buffers and the two streams belong to the scene and are kept between calls (a preview
    // loop of short renders would otherwise pay an allocation, two stream creations and their tear-down per call).
    for (int i = 0; i < slots; ++i) {
      if (scene->batchCap[i] < batch) {
        if (scene->d_batch[i]) { HIP_CHECK(hipDeviceSynchronize()); (void)hipFree(scene->d_batch[i]); }
        scene->d_batch[i] = nullptr; scene->batchCap[i] = 0;
        HIP_CHECK(hipMalloc(&scene->d_batch[i], batch * sizeof(mi_trace_result)));
        scene->batchCap[i] = batch;
      }
      if (!scene->pipeStream[i]) HIP_CHECK(hipStreamCreateWithFlags(&scene->pipeStream[i], hipStreamNonBlocking));
    }
    mi_trace_result* const* d = scene->d_batch;
    hipStream_t const* st = scene->pipeStream;
    // The caller's stream is page-locked for the duration of the call, so the copies are real DMA transfers that
    // overlap the kernels of the other slot (pageable copies go through a staging buffer and serialise). Memory that
    // cannot be registered (or option "pin" = 0) just takes the pageable route; memory the caller has already
    // page-locked (hipHostMalloc / hipHostRegister / torch pin_memory) is used as it is.
    bool pinned = false;
    if (scene->opt.pin && n * sizeof(mi_trace_result) >= (size_t)1 << 20) {
      hipPointerAttribute_t attr{};
      const bool known = hipPointerGetAttributes(&attr, rays) == hipSuccess && attr.type == hipMemoryTypeHost;
      if (!known) {
        (void)hipGetLastError();
        pinned = hipHostRegister(rays, n * sizeof(mi_trace_result), hipHostRegisterDefault) == hipSuccess;
        if (!pinned) (void)hipGetLastError();
      }
    }
    auto cleanup = [&] { if (pinned) (void)hipHostUnregister(rays); };
    try {
      const auto t0 = std::chrono::steady_clock::now();
      auto finish = [&](size_t b) {
        HIP_CHECK(hipStreamSynchronize(st[b % slots]));
        const size_t first = b * batch, cnt = std::min(batch, n - first);
        if (cb) cb(user, b, rays + first, cnt);              // RayCallback::fetch, src/RayCallback.cpp:8-24
      };
      for (size_t b = 0; b < numBatches; ++b) {
        const int i = (int)(b % slots);
        if (b >= (size_t)slots) finish(b - slots);
        const size_t first = b * batch, cnt = std::min(batch, n - first);
        HIP_CHECK(hipMemcpyAsync(d[i], rays + first, cnt * sizeof(mi_trace_result), hipMemcpyHostToDevice, st[i]));
        launchRender(*scene, mode, d[i], cnt, st[i]);
        HIP_CHECK(hipMemcpyAsync(rays + first, d[i], cnt * sizeof(mi_trace_result), hipMemcpyDeviceToHost, st[i]));
      }
      for (size_t b = (numBatches > (size_t)slots ? numBatches - slots : 0); b < numBatches; ++b) finish(b);
      scene->traceTimeSecs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) { (void)hipDeviceSynchronize(); cleanup(); throw; }
    cleanup();
  });
}

int mi_scene_set_option(mi_scene* scene, const char* key, const char* value) {
  if (!scene || !key || !value) { g_err = "mi_scene_set_option: null argument"; return MI_ERR_INVALID_ARG; }
  // (a value auto_rebuild does not take is refused before the scene is touched)
  if (!strcmp(key, "auto_rebuild")) { double r; if (!SceneOptions::autoRebuildValue(value, r)) { g_err = std::string("mi_scene_set_option: auto_rebuild takes 0 (off) or a decimal ratio above 1: ") + key + "=" + value; return MI_ERR_INVALID_ARG; } }
  if (!scene->opt.set(key, value)) { g_err = std::string("mi_scene_set_option: ") + scene->opt.why + ": " + key + "=" + value; return MI_ERR_INVALID_ARG; }
  return MI_OK;
}

double mi_trace_time_secs(const mi_scene* scene) { return scene ? scene->traceTimeSecs : 0.0; }

int mi_get_counters(mi_scene* scene, uint64_t counts[4]) {
  if (!scene || !counts) { g_err = "mi_get_counters: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[4];
    HIP_CHECK(hipMemcpy(h, scene->d_counters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) counts[i] = h[i];
  });
}

int mi_get_phase_stats(mi_scene* scene, uint64_t stats[12]) {
  if (!scene || !stats) { g_err = "mi_get_phase_stats: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[16];
    HIP_CHECK(hipMemcpy(h, scene->d_counters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 12; ++i) stats[i] = h[4 + i];
  });
}

int mi_get_pool_stats(mi_scene* scene, uint64_t stats[8]) {      // (zeros in a library built without the path-pool kernel)
  if (!scene || !stats) { g_err = "mi_get_pool_stats: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[32];
    HIP_CHECK(hipMemcpy(h, scene->d_counters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) stats[i] = h[16 + i];
  });
}

int mi_get_hot_stats(mi_scene* scene, uint64_t stats[5]) {
  if (!scene || !stats) { g_err = "mi_get_hot_stats: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[32];
    HIP_CHECK(hipMemcpy(h, scene->d_counters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) stats[i] = h[24 + i];
  });
}

int mi_debug_launch_progress(mi_scene* scene, void* hip_stream, uint64_t* d_samples, uint32_t n, uint32_t period_ticks) {
  if (!scene || !d_samples || n == 0 || n > (1u << 20) || period_ticks == 0 || period_ticks > 100000000u) { g_err = "mi_debug_launch_progress: bad argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    LaunchSlot& slot = scene->slotFor((hipStream_t)hip_stream);
    if (!scene->debugStream) HIP_CHECK(hipStreamCreateWithFlags(&scene->debugStream, hipStreamNonBlocking));
    hipLaunchKernelGGL(launch_progress_kernel, dim3(1), dim3(64), 0, scene->debugStream, slot.d_workCounter, reinterpret_cast<unsigned long long*>(d_samples), n, period_ticks);
    HIP_CHECK(hipGetLastError());
  });
}

int mi_get_nif_timing(mi_scene* scene, double out[2]) {
  if (!scene || !out) { g_err = "mi_get_nif_timing: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    out[0] = 0.0; out[1] = (double)scene->nifTimes.size();
    for (auto& e : scene->nifTimes) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) out[0] += ms;
      (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    scene->nifTimes.clear();
  });
}

int mi_get_nif_clock(mi_scene* scene, uint64_t out[2]) {
  if (!scene || !out) { g_err = "mi_get_nif_clock: null argument"; return MI_ERR_INVALID_ARG; }
  if (!scene->nif.loaded()) { g_err = "mi_get_nif_clock: no NIF model loaded"; return MI_ERR_NO_NIF; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[2] = {0, 0};
    HIP_CHECK(hipMemcpy(h, scene->nif.d_clock, sizeof h, hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1];
  });
}

int mi_reset_counters(mi_scene* scene) {
  if (!scene) { g_err = "mi_reset_counters: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(scene->d_counters, 0, 32 * sizeof(unsigned long long)));
  });
}

int mi_scene_set_nif(mi_scene* scene, uint32_t num_layers, const float* const* kernels, const float* const* biases,
                     const uint32_t* rows, const uint32_t* cols, const uint8_t* relu,
                     uint32_t embedding_dimension, float max_value, const float mean[3], int32_t log_tonemap) {
  if (!scene || !kernels || !rows || !cols || !relu || !mean) { g_err = "mi_scene_set_nif: null argument"; return MI_ERR_INVALID_ARG; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    try { scene->nif.load(num_layers, kernels, biases, rows, cols, relu, embedding_dimension, max_value, mean, log_tonemap); }
    catch (const std::invalid_argument& e) { throw ArgError(e.what()); }
  });
}

int mi_scene_set_hdri_rotation(mi_scene* scene, float degrees) {
  if (!scene) { g_err = "null scene"; return MI_ERR_INVALID_ARG; }
  scene->hdriRotationDegrees = degrees;
  return MI_OK;
}

int mi_scene_set_max_nif_batch(mi_scene* scene, size_t rays_per_batch) {
  if (!scene) { g_err = "null scene"; return MI_ERR_INVALID_ARG; }
  scene->maxNifBatch = rays_per_batch;
  return MI_OK;
}

int mi_scene_set_ray_batch(mi_scene* scene, size_t rays_per_batch) {
  if (!scene) { g_err = "null scene"; return MI_ERR_INVALID_ARG; }
  scene->rayBatch = rays_per_batch;
  return MI_OK;
}

int mi_nif_infer_device(mi_scene* scene, const float* d_u, const float* d_v, float* d_bgr, size_t n, void* hip_stream) {
  if (!scene || ((!d_u || !d_v || !d_bgr) && n)) { g_err = "mi_nif_infer_device: null argument"; return MI_ERR_INVALID_ARG; }
  if (!scene->nif.loaded()) { g_err = "mi_nif_infer_device: no NIF model loaded"; return MI_ERR_NO_NIF; }
  return guarded([&] {
    HIP_CHECK(hipSetDevice(scene->device));
    nif_infer(scene->nif, d_u, d_v, d_bgr, n, scene->maxNifBatch, (hipStream_t)hip_stream, scene->opt.nifShape, scene->cus(), scene->opt.nifGenerations);
    HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"

#include "query_drivers.hpp"        // the five query families: launchers, argument rules, the host pipeline, their entries
#include "group_render.hpp"

#if MI_NIF_STAMPS
// diagnostic build only: reads and clears the NIF kernel's stamp sums (nif_kernels.hpp)
extern "C" int mi_debug_nif_stamps(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(mi::nif_stamps), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(mi::nif_stamps), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

