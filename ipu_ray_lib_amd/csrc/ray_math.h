// ray_math.h — the product's ray-math core, shared by the host plumbing (g++) and the gfx950
// kernels (hipcc). Every function is a single-rounding-per-operation binary32 computation: the
// library is built with -ffp-contract=off and no fast-math so that host, device and the
// reference's CPU path agree bit for bit.
//
// Reference counterparts are cited per function (paths relative to the reference checkout).
#pragma once

#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define MI_HD __host__ __device__ __forceinline__
#else
#define MI_HD inline
#endif

namespace mi {

struct f3 { float x, y, z; };

MI_HD f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
MI_HD f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
MI_HD f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
MI_HD f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
MI_HD f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
MI_HD f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
MI_HD f3 abs3(f3 a) { return mk(fabsf(a.x), fabsf(a.y), fabsf(a.z)); }
// embree_utils/geometry.hpp:135-143 — evaluation order is part of the contract
MI_HD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
MI_HD float sqnorm(f3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
MI_HD f3 normalized(f3 a) { return a * (1.f / sqrtf(sqnorm(a))); }
MI_HD f3 cross(f3 a, f3 v) { return mk(a.y * v.z - a.z * v.y, a.z * v.x - a.x * v.z, a.x * v.y - a.y * v.x); }
MI_HD float comp(f3 a, uint32_t i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

// geometry.hpp:115-125. Named maxi/maxc upstream; they select the SMALLEST component and
// every caller depends on that.
// Written as two compare / select pairs: "x < y ? (x < z ? x : z) : (y < z ? y : z)" is "m = x < y ? x : y; m < z ? m : z" -
// the SAME comparisons on the same operands in either branch (NaN behaviour included), but hipcc evaluates all three
// compares of the nested form (the triangle test takes four of these per primitive).
MI_HD uint32_t min_index(f3 v) {
  const bool xy = v.x < v.y;
  const float m = xy ? v.x : v.y;
  return (m < v.z) ? (xy ? 0u : 1u) : 2u;
}
MI_HD float min_comp(f3 v) {
  const float m = (v.x < v.y) ? v.x : v.y;
  return (m < v.z) ? m : v.z;
}
// The smallest of three absolute values as fminf (one v_min3_f32 |a|, |b|, |c| on the device, where min_comp(abs3(..)) is two compare /
// select pairs serialised on VCC). The same bits as min_comp(abs3(mk(a, b, c))) when no operand is NaN - the operands are absolute values, so
// a tie is one bit pattern; with a NaN operand fminf returns the other operand where the select chain returns the second. Only for a caller
// whose result does not depend on the value then: the triangle test's error bound (tri_math.hpp), not offset_origin or roulette_stop.
MI_HD float min_abs3(float a, float b, float c) { return fminf(fminf(fabsf(a), fabsf(b)), fabsf(c)); }

// precision_utils.hpp:18-25
constexpr float kMachineEps = 5.9604644775390625e-08f;   // 2^-24
MI_HD constexpr float gamma_n(int i) { return (kMachineEps * (float)i) / (1.f - kMachineEps * (float)i); }
constexpr float kRayEpsilon = kMachineEps * 1500.f;
constexpr float kSlabScale = 1.f + 2.f * gamma_n(3);      // CompactBVH2Node.hpp:42
constexpr float kInf = __builtin_huge_valf();

// ---- binary16 ---------------------------------------------------------------------------------
MI_HD float half_bits_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
  _Float16 v;
  __builtin_memcpy(&v, &h, 2);
  return (float)v;                                        // v_cvt_f32_f16, exact
#else
  uint32_t sign = ((uint32_t)h & 0x8000u) << 16, ex = (h >> 10) & 0x1Fu, man = h & 0x3FFu, bits;
  if (ex == 0) {
    if (man == 0) bits = sign;
    else {                                                // subnormal: renormalise
      int sh = 0;
      while (!(man & 0x400u)) { man <<= 1; ++sh; }
      bits = sign | ((uint32_t)(113 - sh) << 23) | ((man & 0x3FFu) << 13);
    }
  } else if (ex == 31) bits = sign | 0x7F800000u | (man << 13);
  else bits = sign | ((ex + 112u) << 23) | (man << 13);
  float f; memcpy(&f, &bits, 4); return f;
#endif
}

// float -> half, round to nearest even, in integer code (not the hardware conversion): the BVH builder packs nodes with it on
// the host and the refit kernels (refit_kernels.hpp) repack them on the device, and both must produce the same bits
MI_HD uint16_t float_to_half_bits(float f) {
  uint32_t x; __builtin_memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7FFFFFFFu;
  if (x >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (x > 0x7F800000u ? 0x200u : 0u));
  if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);
  if (x < 0x33000001u) return sign;
  const int e = (int)(x >> 23) - 127;
  const uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
  uint32_t q, rem, halfway;
  if (e < -14) {
    const int shift = 13 + (-14 - e);
    q = m >> shift; rem = m & ((1u << shift) - 1u); halfway = 1u << (shift - 1);
  } else {
    q = ((uint32_t)(e + 15) << 10) | ((m >> 13) & 0x3FFu); rem = m & 0x1FFFu; halfway = 0x1000u;
  }
  if (rem > halfway || (rem == halfway && (q & 1u))) ++q;
  return (uint16_t)(sign | q);
}
// precision_utils.hpp:39-47
MI_HD uint16_t half_not_smaller(float f) {
  uint16_t h = float_to_half_bits(f);
  if (half_bits_to_float(h) < f) h = (uint16_t)(h + 1);
  return h;
}

// ---- BVH node boxes ------------------------------------------------------------------------------
// One definition of a primitive's box, of the union of two boxes and of the compact node's encoding, for the host builder
// (host/bvh_sah.cpp, host/scene_builtin.cpp), the host refit (mi_refit_compact_bvh) and the device refit (refit_kernels.hpp).
// min / max are the compare / select of Bounds::grow (host/scene_types.hpp), never fminf / v_min_f32: those differ from it on
// signed zeros and NaNs. A NaN coordinate is ignored unless every point has one (the box then stays empty: +inf / -inf).
struct Box3 { f3 lo, hi; };
MI_HD Box3 box_empty() { Box3 b; b.lo = mk(kInf, kInf, kInf); b.hi = mk(-kInf, -kInf, -kInf); return b; }
MI_HD void box_grow(Box3& b, f3 p) {
  b.lo.x = p.x < b.lo.x ? p.x : b.lo.x; b.lo.y = p.y < b.lo.y ? p.y : b.lo.y; b.lo.z = p.z < b.lo.z ? p.z : b.lo.z;
  b.hi.x = p.x > b.hi.x ? p.x : b.hi.x; b.hi.y = p.y > b.hi.y ? p.y : b.hi.y; b.hi.z = p.z > b.hi.z ? p.z : b.hi.z;
}
// InnerNode::setBounds (embree_utils/node.hpp:56-70) as the builder forms it: grow(first.lo), grow(first.hi), grow(second.lo), grow(second.hi)
MI_HD Box3 box_union(const Box3& a, const Box3& b) {
  Box3 u = box_empty();
  box_grow(u, a.lo); box_grow(u, a.hi); box_grow(u, b.lo); box_grow(u, b.hi);
  return u;
}
MI_HD Box3 triangle_box(f3 p0, f3 p1, f3 p2) { Box3 b = box_empty(); box_grow(b, p0); box_grow(b, p1); box_grow(b, p2); return b; }
// sphere: centre +- radius (Primitives.hpp:53-56); disc: centre +- r (Primitives.hpp:77-81)
MI_HD Box3 ball_box(float x, float y, float z, float r) { Box3 b; b.lo = mk(x - r, y - r, z - r); b.hi = mk(x + r, y + r, z + r); return b; }

// The compact node's box (CompactBVH2Node.hpp:52-85, src/CompactBvhBuild.cpp:5-32): min as binary32, extents hi - lo rounded UP
// to binary16. Returns kBoxOk, kBoxTooLarge (an extent above 65504: the builder throws) or kBoxNotFinite (a min or an extent that
// is not finite: mi_scene_create refuses the node); the fields are written in every case.
enum : uint32_t { kBoxOk = 0, kBoxTooLarge = 1, kBoxNotFinite = 2 };
constexpr float kMaxHalf = 65504.f;
MI_HD uint32_t box_encode(const Box3& b, float& mx, float& my, float& mz, uint16_t& dx, uint16_t& dy, uint16_t& dz) {
  mx = b.lo.x; my = b.lo.y; mz = b.lo.z;
  const float ex = b.hi.x - b.lo.x, ey = b.hi.y - b.lo.y, ez = b.hi.z - b.lo.z;
  dx = half_not_smaller(ex); dy = half_not_smaller(ey); dz = half_not_smaller(ez);
  if (ex > kMaxHalf || ey > kMaxHalf || ez > kMaxHalf) return kBoxTooLarge;
  uint32_t bx, by, bz;
  __builtin_memcpy(&bx, &mx, 4); __builtin_memcpy(&by, &my, 4); __builtin_memcpy(&bz, &mz, 4);
  const bool minBad = (bx & 0x7F800000u) == 0x7F800000u || (by & 0x7F800000u) == 0x7F800000u || (bz & 0x7F800000u) == 0x7F800000u;
  const bool extBad = (dx & 0x7C00u) == 0x7C00u || (dy & 0x7C00u) == 0x7C00u || (dz & 0x7C00u) == 0x7C00u;
  return (minBad || extBad) ? kBoxNotFinite : kBoxOk;
}

// ---- LBVH: Morton keys and Karras' hierarchy -------------------------------------------------------------------------------
// One definition for the host twin (host/lbvh.cpp, mi_build_lbvh_compact) and the device rebuild (rebuild_kernels.hpp,
// mi_scene_rebuild): both must produce the same tree. Every float step is one rounded binary32 (or binary64) operation.
//
// A centroid component quantised to 21 bits inside the scene box [lo, lo + ext]: the correctly rounded quotient (c - lo) / ext,
// scaled by 2^21 (exact), truncated, clamped to [0, 2^21 - 1]. An axis of zero (or not positive, or NaN) extent maps to 0, and so
// does a quotient that is negative or NaN.
constexpr uint32_t kMortonBits = 21;
MI_HD uint32_t lbvh_quantise(float c, float lo, float ext) {
  if (!(ext > 0.f)) return 0u;
  const float t = (c - lo) / ext;
  const float s = t * 2097152.f;
  if (!(s >= 0.f)) return 0u;
  if (s >= 2097151.f) return 2097151u;
  return (uint32_t)s;
}
// bit i of v -> bit 3 i
MI_HD uint64_t morton_spread21(uint32_t v) {
  uint64_t x = v & 0x1FFFFFu;
  x = (x | (x << 32)) & 0x001F00000000FFFFull;
  x = (x | (x << 16)) & 0x001F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}
// The 63-bit key of a primitive box inside the scene box: x in the highest bit of every triple.
MI_HD uint64_t lbvh_key(const Box3& prim, const Box3& scene) {
  const f3 c = (prim.lo + prim.hi) * .5f;
  const f3 ext = scene.hi - scene.lo;
  return (morton_spread21(lbvh_quantise(c.x, scene.lo.x, ext.x)) << 2) | (morton_spread21(lbvh_quantise(c.y, scene.lo.y, ext.y)) << 1) |
         morton_spread21(lbvh_quantise(c.z, scene.lo.z, ext.z));
}
// The scene box's accumulation: lo against lo, hi against hi (compare / select), so that an empty box (+inf / -inf) is neutral - a
// reduction pads with empty boxes, and box_grow with an empty box's corners as points would not be.
MI_HD Box3 box_merge(Box3 a, const Box3& b) {
  a.lo.x = b.lo.x < a.lo.x ? b.lo.x : a.lo.x; a.lo.y = b.lo.y < a.lo.y ? b.lo.y : a.lo.y; a.lo.z = b.lo.z < a.lo.z ? b.lo.z : a.lo.z;
  a.hi.x = b.hi.x > a.hi.x ? b.hi.x : a.hi.x; a.hi.y = b.hi.y > a.hi.y ? b.hi.y : a.hi.y; a.hi.z = b.hi.z > a.hi.z ? b.hi.z : a.hi.z;
  return a;
}
// The scene box without signed zeros (x + 0 = +0 for either zero): a reduction may meet the zeros in any order.
MI_HD Box3 lbvh_scene_box(Box3 b) {
  b.lo = b.lo + mk(0.f, 0.f, 0.f); b.hi = b.hi + mk(0.f, 0.f, 0.f);
  return b;
}
MI_HD int lbvh_clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)x);
#else
  return x ? __builtin_clzll(x) : 64;
#endif
}
// delta(i, j) of the sorted keys: the length of the common prefix of key i and key j, equal keys going on with the common prefix of
// the sorted positions themselves (so that a run of equal keys becomes a balanced subtree, not a chain); -1 outside [0, n).
MI_HD int lbvh_delta(const uint64_t* keys, uint32_t n, uint32_t i, int64_t j) {
  if (j < 0 || j >= (int64_t)n) return -1;
  const uint64_t x = keys[i] ^ keys[j];
  return x ? lbvh_clz64(x) : 64 + lbvh_clz64((uint64_t)i ^ (uint64_t)j);
}
// Karras 2012, interior node i of n - 1 over n >= 2 sorted keys: the range [first, last] of sorted positions below it and the
// position `split` its two children part at - the first child covers [first, split] (the leaf `split` when first == split), the
// second [split + 1, last] (the leaf `last` when split + 1 == last). An interior child has the index of its split-side end:
// `split` for the first, split + 1 for the second.
MI_HD void lbvh_node(const uint64_t* keys, uint32_t n, uint32_t i, uint32_t& first, uint32_t& last, uint32_t& split) {
  const int d = lbvh_delta(keys, n, i, (int64_t)i + 1) - lbvh_delta(keys, n, i, (int64_t)i - 1) >= 0 ? 1 : -1;
  const int dmin = lbvh_delta(keys, n, i, (int64_t)i - d);
  int64_t lmax = 2;
  while (lbvh_delta(keys, n, i, (int64_t)i + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (lbvh_delta(keys, n, i, (int64_t)i + (l + t) * d) > dmin) l += t;
  const int64_t j = (int64_t)i + l * d;
  const int dnode = lbvh_delta(keys, n, i, j);
  int64_t s = 0;
  for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
    if (lbvh_delta(keys, n, i, (int64_t)i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int64_t g = (int64_t)i + s * d + (d < 0 ? -1 : 0);
  first = (uint32_t)(d > 0 ? (int64_t)i : j); last = (uint32_t)(d > 0 ? j : (int64_t)i); split = (uint32_t)g;
}
// The host builder's child-order rule (host/bvh_sah.cpp): the squared distance of a box's centre from the origin, the centre in
// binary32, the squares and sums in binary64. The child with the smaller value goes first.
MI_HD double box_centre_dist2(const Box3& b) {
  const f3 c = (b.lo + b.hi) * .5f;
  return (double)c.x * c.x + (double)c.y * c.y + (double)c.z * c.z;
}

// ---- BVH cost: the surface-area cost of a tree of compact nodes ---------------------------------------------------------------
// One definition for the host twin (mi_bvh_cost_compact, host/scene_api.cpp) and the device pass (cost_kernels.hpp,
// mi_scene_bvh_cost): both must return the same three doubles bit for bit, run to run.
// A node's term is half its box's surface area from its three binary16 extents, decoded exactly, in binary64, every operation
// rounded once in the order written.
MI_HD double bvh_cost_term(uint16_t dx, uint16_t dy, uint16_t dz) {
  const double ex = (double)half_bits_to_float(dx), ey = (double)half_bits_to_float(dy), ez = (double)half_bits_to_float(dz);
  return (ex * ey + ey * ez) + ez * ex;
}
// The two sums carried through the reduction: over all nodes (a box test each), over the leaves (a primitive test each).
struct Cost2 { double all, leaf; };
MI_HD Cost2 cost_add(Cost2 a, Cost2 b) { Cost2 r; r.all = a.all + b.all; r.leaf = a.leaf + b.leaf; return r; }
// The reduction's shape. Level 0 holds one Cost2 per node, in node order. A level of n entries becomes one of cost_blocks(n, W)
// entries: entry b is the sum of entries b W .. b W + W - 1 (entries past the end count as +0) through the fixed binary tree
// below - strides W / 2, W / 4, .. 1, entry i taking entry i + stride - and the levels repeat until one entry is left (at least
// once: a single node is reduced as a block of its own). Floating-point addition is not associative: this shape, not the order in
// which threads happen to run, decides every bit of the result.
// v[0 .. W) -> v[0]; W a power of two. `lane` of `lanes` workers share the work of one stride, sync() separates the strides
// (the device: the workgroup's threads and __syncthreads(); the host: one worker, nothing to wait for).
constexpr uint32_t kCostBlock = 256;
template <class Sync>
MI_HD void cost_block_reduce(Cost2* v, uint32_t W, uint32_t lane, uint32_t lanes, Sync&& sync) {
  for (uint32_t s = W >> 1; s > 0; s >>= 1) {
    for (uint32_t i = lane; i < s; i += lanes) v[i] = cost_add(v[i], v[i + s]);
    sync();
  }
}
MI_HD uint32_t cost_blocks(uint32_t n, uint32_t W) { return n / W + (n % W ? 1u : 0u); }
// The traversal-cost estimate the auto-rebuild policy compares: expected box tests and primitive tests of a random line through
// the root box, weighted by the static instruction counts of the box-test step and the triangle-test step (DESIGN.md §6,
// tools/bvh_eval.py). cost = {sum_all, sum_leaf, a_root}; a_root == 0 gives inf or NaN, which the policy never acts on.
constexpr double kCostBoxTest = 26.0, kCostPrimTest = 224.0;
MI_HD double bvh_cost_estimate(const double cost[3]) { return (kCostBoxTest * cost[0] + kCostPrimTest * cost[1]) / cost[2]; }

// ---- sincos: ext/math/sincos.cpp:236-355 (ACC5, ABSERR, MOD360, flg=0) ---------------------------
// `tbl` = 92 floats, sin(i degrees); lives in LDS on the device, static storage on the host.
MI_HD void sincos_deg_table(float x, const float* tbl, float& s, float& c) {
  x = x * (float)(180.0 / 3.14159265358979323846264338327950288);
  const bool neg = x < 0.f;
  if (neg) x = -x;
  x = x - 360.f * floorf(x / 360.f);
  int ix = (int)(x + .5f);
  const float z = x - (float)ix;
  bool sneg = false, cneg = false;
  if (ix > 180) { sneg = true; cneg = true; ix -= 180; }
  if (ix > 90) { cneg = !cneg; ix = 180 - ix; }
  float sx = tbl[ix];
  if (sneg) sx = -sx;
  float cx = tbl[90 - ix];
  if (cneg) cx = -cx;
  const float sz = 1.74531263774940077459e-2f * z;
  const float cz = 1.f - 1.52307909153324666207e-4f * z * z;
  float y = sx * cz + cx * sz;
  if (neg) y = -y;
  s = y;
  c = cx * cz - sx * sz;
}
// sincos_deg_table behind its range reduction: x in degrees, 0 <= x < 360, `neg` the sign taken off the angle.
MI_HD void sincos_deg_reduced(float x, bool neg, const float* tbl, float& s, float& c) {
  int ix = (int)(x + .5f);
  const float z = x - (float)ix;
  bool sneg = false, cneg = false;
  if (ix > 180) { sneg = true; cneg = true; ix -= 180; }
  if (ix > 90) { cneg = !cneg; ix = 180 - ix; }
  float sx = tbl[ix];
  if (sneg) sx = -sx;
  float cx = tbl[90 - ix];
  if (cneg) cx = -cx;
  const float sz = 1.74531263774940077459e-2f * z;
  const float cz = 1.f - 1.52307909153324666207e-4f * z * z;
  float y = sx * cz + cx * sz;
  if (neg) y = -y;
  s = y;
  c = cx * cz - sx * sz;
}
// Two callers know their angle's range, and there the correctly rounded x / 360 of the general form (a dozen instructions on the
// device, on the chain to a new direction) can only give one or two quotients. Both return sincos_deg_table's bits for every binary32
// angle of their domain (host/shade_consts_check.cpp runs through all of them).
// |th| <= 2.4 (the concentric map: |th| <= 3 pi / 4): |x| < 138, floorf(x / 360) is 0 and x - 360 * 0 is x. But for th = -0 (uy = +0
// over a negative ux), which is not `neg`: the general form goes on with -0 - (-0) = +0, this one with -0. The zero only reaches
// z = x - 0 and sz = k z, and both sums that take sz give the same bits for either: s = 0 * 1 + 1 * sz = +0, c = 1 * 1 - 0 * sz = 1.
MI_HD void sincos_deg_table_small(float th, const float* tbl, float& s, float& c) {
  float x = th * (float)(180.0 / 3.14159265358979323846264338327950288);
  const bool neg = x < 0.f;
  if (neg) x = -x;
  sincos_deg_reduced(x, neg, tbl, s, c);
}
// 0 <= th <= 6.2831855f (the Box-Muller angle 2 pi u, u in [0, 1]; +0, not -0): 0 <= x <= 360.00003, the quotient's floor is 1 from
// x = 360 on (360 / 360 is 1) and 0 below (the largest binary32 below 360 divides to 1 - 2^-24), and x - 360 * 1 is exact.
MI_HD void sincos_deg_table_turn(float th, const float* tbl, float& s, float& c) {
  const float x = th * (float)(180.0 / 3.14159265358979323846264338327950288);
  sincos_deg_reduced(x >= 360.f ? x - 360.f : x, false, tbl, s, c);
}

// ---- xoroshiro128** / splitmix64: include/xoshiro.hpp:18-80 ------------------------------------------
struct Rng { uint64_t s0, s1; };
// A 64-bit rotation by a constant 0 < k < 64, k != 32, on the two 32-bit halves: k >= 32 swaps the halves, then each half of the result is
// 32 bits cut out of a pair of halves - alignbit(a, b, s), the low word of (a : b) >> s. One v_alignbit_b32 per half on the device, where
// hipcc compiles (x << k) | (x >> (64 - k)) as a 64-bit shift, a 32-bit shift and an OR (host/rotl_halves_check.cpp holds the two forms
// against each other).
MI_HD uint32_t alignbit(uint32_t a, uint32_t b, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(a, b, s);
#else
  return (uint32_t)((((uint64_t)a << 32) | b) >> s);
#endif
}
MI_HD uint64_t rotl64(uint64_t x, int k) {
  const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
  const uint32_t lo = k >= 32 ? xh : xl, hi = k >= 32 ? xl : xh, s = 32u - ((uint32_t)k & 31u);
  return ((uint64_t)alignbit(hi, lo, s) << 32) | alignbit(lo, hi, s);
}
MI_HD uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
MI_HD void rng_seed(Rng& r, uint64_t seed) { r.s0 = splitmix64(seed); r.s1 = splitmix64(r.s0); }
// a * 5 and a * 9 modulo 2^64 as (a << 2) + a and (a << 3) + a: one v_lshl_add_u64 each on the device. hipcc lowers the 64-bit
// multiply to two v_mad_u64_u32 and two moves, and turns the shift-add written in C++ back into that multiply.
#if defined(__HIP_DEVICE_COMPILE__)
MI_HD uint64_t mul5_u64(uint64_t a) { uint64_t r; asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(r) : "v"(a)); return r; }
MI_HD uint64_t mul9_u64(uint64_t a) { uint64_t r; asm("v_lshl_add_u64 %0, %1, 3, %1" : "=v"(r) : "v"(a)); return r; }
#else
MI_HD uint64_t mul5_u64(uint64_t a) { return a * 5; }
MI_HD uint64_t mul9_u64(uint64_t a) { return a * 9; }
#endif
MI_HD uint64_t rng_next(Rng& r) {
  const uint64_t a = r.s0;
  uint64_t b = r.s1;
  const uint64_t out = mul9_u64(rotl64(mul5_u64(a), 7));
  b ^= a;
  r.s0 = rotl64(a, 24) ^ b ^ (b << 16);
  r.s1 = rotl64(b, 37);
  return out;
}
// xoshiro.hpp:68-80: [1,2) double minus one, narrowed with round-to-nearest (may be exactly 1.0f)
MI_HD float rng_uniform01(Rng& r) {
  const uint64_t bits = (0x3FFull << 52) | (rng_next(r) >> 12);
  double d;
  __builtin_memcpy(&d, &bits, 8);
  return (float)(d - 1.0);
}

// Saturating float -> u32 (== v_cvt_u32_f32), so host and device agree on odd pixel coords.
MI_HD uint32_t f2u_sat(float f) {
  if (!(f > 0.f)) return 0u;
  if (f >= 4294967296.f) return 0xFFFFFFFFu;
  return (uint32_t)f;
}
// Per-pixel stream: seeded from the user seed and FULL-image (row, col).
// A pixel's samples are cut into segments of segment_samples(samplesPerPixel); segment j has its own stream
// (j = 0: the plain per-pixel seed) and its own partial rgb sum, added in segment order. The work
// atom of the persistent kernel is (pixel, segment): with pixel x all-samples atoms a 1440^2 x 1000 spp frame gives
// every lane only 6 atoms, and the drain at the end of the frame cost a third of the throughput. The length is a
// function of the render's sample count alone (never of the batch, crop or GPU count): about sixteen segments per
// pixel - samplesPerPixel / 16 rounded up to a power of two - but no shorter than 4 samples (every atom costs a
// fetch, a seed and a partial sum) and no longer than 64 (atoms enough for every lane's drain to be short).
// Measured on the 1440^2 box frame: 16 spp 8.1e9 -> 10.0e9 casts/s, 64 spp 9.0e9 -> 11.5e9 against one atom per
// pixel; 1000 spp 13.1e9 with 64-sample segments against 12.8e9 with 16-sample ones.
constexpr uint32_t kSegmentSamplesMin = 4, kSegmentSamplesMax = 64, kSegmentsPerPixel = 16;
MI_HD uint32_t segment_shift(uint32_t samplesPerPixel) {
  const uint32_t want = (samplesPerPixel + kSegmentsPerPixel - 1) / kSegmentsPerPixel;          // ceil(spp / 16)
  const uint32_t shift = want <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(want - 1u);              // ceil(log2(want))
  return shift < 2u ? 2u : shift > 6u ? 6u : shift;                                               // 4 ... 64 samples
}
MI_HD uint32_t segment_samples(uint32_t samplesPerPixel) { return 1u << segment_shift(samplesPerPixel); }
MI_HD void rng_seed_pixel_segment(Rng& r, uint64_t userSeed, float row, float col, uint32_t segment) {
  const uint64_t pix = ((uint64_t)f2u_sat(row) << 32) | (uint64_t)f2u_sat(col);
  rng_seed(r, (userSeed ^ ((pix + 1ull) * 0x9e3779b97f4a7c15ull)) ^ ((uint64_t)segment * 0xd1b54a32d192ed03ull));
}
MI_HD void rng_seed_pixel(Rng& r, uint64_t userSeed, float row, float col) { rng_seed_pixel_segment(r, userSeed, row, col, 0u); }

// Deterministic ln(x), x normal and positive (pixel-jitter Box-Muller only).
MI_HD float log_det(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  int e = (int)((b >> 23) & 0xFFu) - 126;
  const uint32_t mb = (b & 0x007FFFFFu) | 0x3F000000u;
  float m;
  __builtin_memcpy(&m, &mb, 4);
  if (m < 0.707106781186547524f) { e -= 1; m = m + m - 1.0f; }
  else { m = m - 1.0f; }
  float z = m * m;
  float y = 7.0376836292e-2f;
  y = y * m + -1.1514610310e-1f;
  y = y * m + 1.1676998740e-1f;
  y = y * m + -1.2420140846e-1f;
  y = y * m + 1.4249322787e-1f;
  y = y * m + -1.6668057665e-1f;
  y = y * m + 2.0000714765e-1f;
  y = y * m + -2.4999993993e-1f;
  y = y * m + 3.3333331174e-1f;
  y = y * m * z;
  const float fe = (float)e;
  y = y + -2.12194440e-4f * fe;
  y = y + -0.5f * z;
  z = m + y;
  z = z + 0.693359375f * fe;
  return z;
}
// Two N(0,1) variates per pixel sample; stands in for the IPU's hardware f32v2grand
// (codelets/TraceCodelets.cpp:158).
MI_HD void rng_gauss2(Rng& r, const float* sinTbl, float& g0, float& g1) {
  const float ua = rng_uniform01(r);
  const float ub = rng_uniform01(r);
  float w = 1.f - ua;
  if (w < 2.98023223876953125e-08f) w = 2.98023223876953125e-08f;
  const float rad = sqrtf(-2.f * log_det(w));
  float sn, cs;
  sincos_deg_table_turn(6.283185307179586f * ub, sinTbl, sn, cs);      // (ub in [0, 1])
  g0 = rad * cs;
  g1 = rad * sn;
}

// ---- camera: Render.hpp:74-85 --------------------------------------------------------------------
MI_HD f3 pixel_to_ray_dir(float x, float y, float w, float h, float tanTheta) {
  const float aspect = w / h;
  x = (x / w) - .5f;
  y = (y / h) - .5f;
  return normalized(mk(2.f * x * aspect * tanTheta, -2.f * y * tanTheta, -1.f));
}

// ---- Render.hpp:29-33 -----------------------------------------------------------------------------
MI_HD f3 offset_origin(f3 origin, f3 dir, f3 n) {
  const float m = (1.f + min_comp(abs3(origin))) * kRayEpsilon * copysignf(1.f, dot(n, dir));
  return origin + n * m;
}

// ---- sampling / BxDFs: geometric_sampling.hpp:8-63, BxDF.hpp:11-75, geometry.hpp:147-159 -------------
MI_HD void sample_disc_concentric(float u1, float u2, const float* sinTbl, float& ox, float& oy) {
  const float ux = 2.f * u1 - 1.f, uy = 2.f * u2 - 1.f;
  if (ux == 0.f && uy == 0.f) { ox = ux; oy = uy; return; }
  const float piby4 = (float)(3.14159265358979323846264338327950288 / 4.0);
  const float piby2 = (float)(3.14159265358979323846264338327950288 / 2.0);
  // (one division behind selects: as `if (wide) uy / ux else ux / uy` the device compiles two exec regions with a division each, and
  // the outcome is random per lane, so a wave runs both - the same operations on the same operands either way)
  const bool wide = fabsf(ux) > fabsf(uy);
  const float r = wide ? ux : uy;
  const float q = piby4 * ((wide ? uy : ux) / (wide ? ux : uy));
  const float th = wide ? q : piby2 - q;
  float s, c;
  sincos_deg_table_small(th, sinTbl, s, c);      // (|q| <= pi / 4: |th| <= 3 pi / 4)
  ox = r * c; oy = r * s;
}
MI_HD f3 cosine_sample_hemisphere(float u1, float u2, const float* sinTbl) {
  float x, y;
  sample_disc_concentric(u1, u2, sinTbl, x, y);
  const float z = sqrtf(fmaxf(0.f, 1.f - x * x - y * y));
  return mk(x, y, z);
}
// The tangent frame of a diffuse bounce (the reference's orthonormal system about n): |n.x| > |n.y| ? xb = (-n.z, 0, n.x) / sqrt(n.x^2 + n.z^2)
// : xb = (0, n.z, -n.y) / sqrt(n.y^2 + n.z^2), yb = n x xb. ONE sqrt and ONE division behind selects - as two branches the device runs
// both, each with its own, in every wave whose lanes hold different normals. The operations and their operands are the branch form's:
// (-n.z) * il is not -(n.z * il) for a NaN, the zero component is a literal. A function of the normal alone: K1w reads it per leaf
// where the normal is the leaf's (leaf_frame.hpp).
MI_HD void diffuse_frame(f3 n, f3& xb, f3& yb) {
  const f3 a = abs3(n), sq = n * n;
  const bool wide = a.x > a.y;
  const float il = 1.f / sqrtf((wide ? sq.x : sq.y) + sq.z);
  const float m = (wide ? -n.z : n.z) * il;
  const float z = (wide ? n.x : -n.y) * il;
  xb = mk(wide ? m : 0.f, wide ? 0.f : m, z);
  yb = cross(n, xb);
}
MI_HD f3 diffuse_in_frame(f3 n, f3 xb, f3 yb, float u1, float u2, const float* sinTbl) {
  const f3 wi = cosine_sample_hemisphere(u1, u2, sinTbl);
  return mk(dot(mk(xb.x, yb.x, n.x), wi), dot(mk(xb.y, yb.y, n.y), wi), dot(mk(xb.z, yb.z, n.z), wi));
}
MI_HD f3 sample_diffuse(f3 n, float u1, float u2, const float* sinTbl) {
  f3 xb, yb;
  diffuse_frame(n, xb, yb);
  return diffuse_in_frame(n, xb, yb, u1, u2, sinTbl);
}
MI_HD f3 reflect_dir(f3 d, f3 n) {
  const float cosTheta = dot(d, n);
  return normalized(d - n * (cosTheta * 2.f));
}
// Schlick's approximation in its two halves: the reflectance at normal incidence, a function of the index ratio alone, and the rest
MI_HD float schlick_r0(float ri) {
  const float r0 = (1.f - ri) / (1.f + ri);
  return r0 * r0;
}
MI_HD float schlick_from_r0(float cosTheta, float r0) {
  const float base = 1.f - cosTheta;
  const float base2 = base * base;
  const float base5 = base2 * base * base2;
  return r0 + (1.f - r0) * base5;
}
MI_HD float schlick(float cosTheta, float ri) { return schlick_from_r0(cosTheta, schlick_r0(ri)); }
MI_HD f3 refract_dir(f3 dir, f3 n, float ndotr, float ri) {
  const float cosTheta = -ndotr;
  const f3 rPerp = (dir + n * cosTheta) * ri;
  const f3 rPar = n * -sqrtf(fabsf(1.f - sqnorm(rPerp)));
  return rPerp + rPar;
}
MI_HD bool dielectric(f3 dir, f3 n, float ri, float u1, f3& out) {
  if (dot(n, dir) > 0.f) n = -n; else ri = 1.f / ri;
  const float ndotr = dot(n, dir);
  const float cost1 = -ndotr;
  const float cost2 = 1.f - ri * ri * (1.f - cost1 * cost1);
  if (cost2 > 0.f && u1 > schlick(cost1, ri)) { out = refract_dir(dir, n, ndotr, ri); return true; }
  out = reflect_dir(dir, n);
  return false;
}
// What a dielectric bounce takes from its material alone: the index ratio of a ray that enters, and the reflectance at normal incidence
// of a ray that leaves (ratio ior) and of one that enters (ratio 1 / ior) - the binary32 operations dielectric() and schlick() run at
// every bounce, in their order. K1w computes them once per material, where a workgroup stages the materials (trace_wavefront.hpp).
struct DielectricConsts { float invIor, r0In, r0Out; };
MI_HD DielectricConsts dielectric_consts(float ior) {
  DielectricConsts k;
  k.invIor = 1.f / ior;
  k.r0In = schlick_r0(ior);
  k.r0Out = schlick_r0(k.invIor);
  return k;
}
// The index ratio and its r0 for a ray on either side (`inside`: dot(n, dir) > 0, it leaves the medium) - computed at the bounce as
// dielectric() and schlick() do, or selected from the material's constants: the same values.
struct DielectricComputed {};
MI_HD void dielectric_ratio(float ior, const DielectricComputed&, bool inside, float& ri, float& r0) {
  ri = inside ? ior : 1.f / ior;
  r0 = schlick_r0(ri);
}
MI_HD void dielectric_ratio(float ior, const DielectricConsts& k, bool inside, float& ri, float& r0) {
  ri = inside ? ior : k.invIor;
  r0 = inside ? k.r0In : k.r0Out;
}
// dielectric() over either source of the ratio; everything else is dielectric()'s, on the same operands (K1w's form of the bounce:
// trace_wavefront.hpp shade_specular).
template <class K>
MI_HD bool dielectric_with(f3 dir, f3 n, float ior, const K& k, float u1, f3& out) {
  const bool inside = dot(n, dir) > 0.f;
  if (inside) n = -n;
  float ri, r0;
  dielectric_ratio(ior, k, inside, ri, r0);
  const float ndotr = dot(n, dir);
  const float cost1 = -ndotr;
  const float cost2 = 1.f - ri * ri * (1.f - cost1 * cost1);
  const bool refracts = cost2 > 0.f && u1 > schlick_from_r0(cost1, r0);
  if (refracts) out = refract_dir(dir, n, ndotr, ri);
  else out = reflect_dir(dir, n);
  return refracts;
}
// dielectric() with its two divisions taken from the material's constants
MI_HD bool dielectric(f3 dir, f3 n, float ior, const DielectricConsts& k, float u1, f3& out) { return dielectric_with(dir, n, ior, k, u1, out); }
// geometric_sampling.hpp:56-63 — survival probability is the smallest throughput channel
MI_HD bool roulette_stop(float u1, f3& tp) {
  const float p = min_comp(tp);
  if (p == 0.f || u1 > p) return true;
  tp = tp * (1.f / p);
  return false;
}

// sin(i degrees) table of ext/math/sincos.cpp:139-233 as binary32 bit patterns.
#define MI_SIN_TABLE_BITS \
  0x00000000u, 0x3c8ef859u, 0x3d0ef2c6u, 0x3d565e3au, 0x3d8edc7bu, 0x3db27eb6u, 0x3dd61305u, 0x3df996a2u, \
  0x3e0e8365u, 0x3e20305bu, 0x3e31d0d4u, 0x3e43636fu, 0x3e54e6cdu, 0x3e665992u, 0x3e77ba60u, 0x3e8483eeu, \
  0x3e8d2057u, 0x3e95b1beu, 0x3e9e377au, 0x3ea6b0dfu, 0x3eaf1d44u, 0x3eb77c01u, 0x3ebfcc6fu, 0x3ec80de9u, \
  0x3ed03fc9u, 0x3ed8616cu, 0x3ee0722fu, 0x3ee87171u, 0x3ef05e94u, 0x3ef838f7u, 0x3f000000u, 0x3f03d989u, \
  0x3f07a8cau, 0x3f0b6d77u, 0x3f0f2744u, 0x3f12d5e8u, 0x3f167918u, 0x3f1a108du, 0x3f1d9bfeu, 0x3f211b24u, \
  0x3f248dbbu, 0x3f27f37cu, 0x3f2b4c25u, 0x3f2e9772u, 0x3f31d522u, 0x3f3504f3u, 0x3f3826a7u, 0x3f3b39ffu, \
  0x3f3e3ebdu, 0x3f4134a6u, 0x3f441b7du, 0x3f46f30au, 0x3f49bb13u, 0x3f4c7360u, 0x3f4f1bbdu, 0x3f51b3f3u, \
  0x3f543bceu, 0x3f56b31du, 0x3f5919aeu, 0x3f5b6f51u, 0x3f5db3d7u, 0x3f5fe714u, 0x3f6208dau, 0x3f641901u, \
  0x3f66175eu, 0x3f6803cau, 0x3f69de1du, 0x3f6ba635u, 0x3f6d5becu, 0x3f6eff20u, 0x3f708fb2u, 0x3f720d81u, \
  0x3f737871u, 0x3f74d063u, 0x3f76153fu, 0x3f7746eau, 0x3f78654du, 0x3f797051u, 0x3f7a67e2u, 0x3f7b4bebu, \
  0x3f7c1c5cu, 0x3f7cd925u, 0x3f7d8235u, 0x3f7e1781u, 0x3f7e98fdu, 0x3f7f069eu, 0x3f7f605cu, 0x3f7fa62fu, \
  0x3f7fd814u, 0x3f7ff605u, 0x3f800000u, 0x3f7ff605u

}  // namespace mi
