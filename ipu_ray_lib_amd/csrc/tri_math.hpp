// tri_math.hpp — the exact tiers' triangle test (Mesh.cpp:6-104) and the shear it runs on (Primitives.cpp:5-22). One text, compiled by
// hipcc for every kernel that walks the BVH (trace_kernels.hpp includes it) and by g++ for csrc/host/tri_verdict_check.cpp, which holds it
// against the oracle's o_intersect_triangle bit for bit: every function is a sequence of compares, selects and single binary32 (DF: binary64)
// operations in the order written - no contraction, correctly rounded division on both sides.
#pragma once

#include "ray_math.h"

namespace mi {

struct Shear { uint32_t kz; float sx, sy, sz; };

// Primitives.cpp:5-22. Pure function of the ray, so it is evaluated once per cast instead of once
// per leaf (Mesh.hpp:89); identical values.
MI_HD Shear make_shear(f3 d) {
  Shear s;
  s.kz = min_index(d);
  uint32_t kx = s.kz + 1; if (kx == 3) kx = 0;
  uint32_t ky = kx + 1; if (ky == 3) ky = 0;
  const float dx = comp(d, kx), dy = comp(d, ky), dz = comp(d, s.kz);
  s.sx = -dx / dz;
  s.sy = -dy / dz;
  s.sz = 1.f / dz;
  return s;
}

MI_HD f3 permute_kz(f3 p, uint32_t kz) {
  // (kx,ky,kz) is the cyclic rotation that puts component kz last. Written as selects: as three early returns
  // hipcc built divergent regions (exec-mask juggling, ~50 scalar instructions in dependent chains per
  // primitive test) out of what is six v_cndmask per vector.
  const bool r1 = kz == 0;   // (1, 2, 0)
  const bool r2 = kz == 1;   // (2, 0, 1)
  return mk(r1 ? p.y : (r2 ? p.z : p.x), r1 ? p.z : (r2 ? p.x : p.y), r1 ? p.x : (r2 ? p.y : p.z));
}

// Mesh.cpp:6-104, tFar = inf as passed by Mesh.hpp:92. Returns t (0 = miss). DF = the reference's compile-time variant
// ALLOW_DOUBLE_FALLBACK=1 (CMakeLists.txt:13,34-41; Mesh.cpp:38-51): when an edge function is exactly zero all three are
// recomputed from products and differences in binary64 and narrowed to binary32 (v_mul_f64 / v_add_f64 / v_cvt_f32_f64
// are IEEE operations: the same bits as the host's doubles). DF = false is the reference default.
// Written without the reference's early returns: every lane runs every operation and the verdicts are combined at the
// end. Identical values for every input, NaNs included: each early return of Mesh.cpp is a predicate that is evaluated
// here on the same operands (a lane that would have returned early computes on - with whatever its operands give, an
// infinite or NaN 1/det included - and is then told 0). With tFar = +inf (Mesh.hpp:90-92) tFar*det is -inf (det<0) or
// +inf (det>0), and "tScaled < -inf" / "tScaled > +inf" are false for every float including NaN, so those two
// comparisons of Mesh.cpp:62-66 drop out exactly. Measured against the early-return form: -1.4 % frame time (hipcc
// turns early returns into nested exec regions whose merges cost 45 register moves per test).
// The error bound's four minima (the reference's min-selecting maxc of absolute values) are min_abs3 (ray_math.h): the same
// bits unless an operand is NaN, and a NaN operand - a NaN shear product, edge function or scaled z - makes det or tScaled
// NaN, hence t, and deltaT is used in `t <= deltaT` alone, false for a NaN t whatever deltaT is.
// PRE: p0, p1, p2 and o arrive with their components already rotated for sh.kz (GLeafRot)
// POS: for a caller that accepts the returned t only when t > 0 && t < tCur with tCur <= +inf (a NaN tCur accepts nothing).
//   The three verdicts of Mesh.cpp:56-66 - det == 0, det < 0 with tScaled >= 0, det > 0 with tScaled <= 0 - are then not
//   evaluated: whenever one of them holds, t = tScaled * (1 / det) is <= 0, -0, +-inf or NaN (det = +-0: 1/det = +-inf, t is
//   +-inf or NaN; opposite signs: a product that is <= 0, or NaN for an infinite tScaled against a 1/det of zero), so the
//   function may return such a value where the full form returns 0, which that caller rejects as it rejects 0, and it
//   returns the full form's t and barycentrics for every input that caller accepts. A caller whose acceptance is anything
//   else takes the full form.
template <bool DF = false, bool PRE = false, bool POS = false>
MI_HD float intersect_triangle(f3 p0, f3 p1, f3 p2, f3 o, const Shear& sh, float& b0, float& b1, float& b2) {
  f3 p0t = PRE ? p0 - o : permute_kz(p0 - o, sh.kz), p1t = PRE ? p1 - o : permute_kz(p1 - o, sh.kz), p2t = PRE ? p2 - o : permute_kz(p2 - o, sh.kz);
  p0t.x += sh.sx * p0t.z; p0t.y += sh.sy * p0t.z;
  p1t.x += sh.sx * p1t.z; p1t.y += sh.sy * p1t.z;
  p2t.x += sh.sx * p2t.z; p2t.y += sh.sy * p2t.z;
  float e0 = p1t.x * p2t.y - p1t.y * p2t.x;
  float e1 = p2t.x * p0t.y - p2t.y * p0t.x;
  float e2 = p0t.x * p1t.y - p0t.y * p1t.x;
  if constexpr (DF) {
    if (e0 == 0.0f || e1 == 0.0f || e2 == 0.0f) {             // Mesh.cpp:40-50, operation for operation
      const double p2txp1ty = (double)p2t.x * (double)p1t.y;
      const double p2typ1tx = (double)p2t.y * (double)p1t.x;
      e0 = (float)(p2typ1tx - p2txp1ty);
      const double p0txp2ty = (double)p0t.x * (double)p2t.y;
      const double p0typ2tx = (double)p0t.y * (double)p2t.x;
      e1 = (float)(p0typ2tx - p0txp2ty);
      const double p1txp0ty = (double)p1t.x * (double)p0t.y;
      const double p1typ0tx = (double)p1t.y * (double)p0t.x;
      e2 = (float)(p1typ0tx - p1txp0ty);
    }
  }
  // (bitwise, not short-circuit: with || hipcc rebuilds the early returns as nested exec regions; -0.4 % frame time)
  bool miss = ((e0 < 0) | (e1 < 0) | (e2 < 0)) & ((e0 > 0) | (e1 > 0) | (e2 > 0));
  const float det = e0 + e1 + e2;
  if constexpr (!POS) miss = miss | (det == 0);
  p0t.z *= sh.sz; p1t.z *= sh.sz; p2t.z *= sh.sz;
  const float tScaled = e0 * p0t.z + e1 * p1t.z + e2 * p2t.z;
  if constexpr (!POS) miss = miss | ((det < 0.f) & (tScaled >= 0.f)) | ((det > 0.f) & (tScaled <= 0.f));
  const float invDet = 1 / det;
  b0 = e0 * invDet; b1 = e1 * invDet; b2 = e2 * invDet;
  const float t = tScaled * invDet;
  const float maxZt = min_abs3(p0t.z, p1t.z, p2t.z);
  const float deltaZ = gamma_n(3) * maxZt;
  const float maxXt = min_abs3(p0t.x, p1t.x, p2t.x);
  const float maxYt = min_abs3(p0t.y, p1t.y, p2t.y);
  const float deltaX = gamma_n(5) * (maxXt + maxZt);
  const float deltaY = gamma_n(5) * (maxYt + maxZt);
  const float deltaE = 2 * (gamma_n(2) * maxXt * maxYt + deltaY * maxXt + deltaX * maxYt);
  const float maxE = min_abs3(e0, e1, e2);
  const float deltaT = 3 * (gamma_n(3) * maxE * maxZt + deltaE * maxZt + deltaZ * maxE) * fabsf(invDet);
  miss = miss | (t <= deltaT);
  return miss ? 0.f : t;
}

}  // namespace mi
