// capsule_math.hpp — the arithmetic of capsule queries (mi_capsule_query* / mi_capsule_offsets* / mi_capsule_fill*,
// include/mi_raylib.h, where the contract is written): whether a caller's capsule - the segment [a, b] widened by a radius, the
// volume a ball sweeps on a straight move - touches a node's box, a triangle, a sphere's shell or a disc. One definition,
// compiled by hipcc for the kernels (capsule_kernels.hpp) and by g++ for the host twin (host/touch_host.hpp over CapsuleShape): every
// function is a sequence of compares, selects and single binary32 operations in the order written (no contraction, correctly
// rounded divide and sqrt on both sides), so the two return the same bits. The closest point of a triangle, the squared
// distance of two points and the primitives' bounds are point_math.hpp's and box_math.hpp's: nothing of them is repeated here.
//
// Everything is CLOSED, and every rejection is a strict compare that a NaN fails.
#pragma once

#include "box_math.hpp"

namespace mi {

// A query as the walk carries it, every member named: the two ends and d = b - a (9 floats; the six non-zero components of the
// lateral axes X0 = (0, d.z, -d.y), X1 = (-d.z, 0, d.x), X2 = (d.y, -d.x, 0) are d's own with a sign, so they are not held twice),
// radius, r2 = radius radius and dd = d.d (3), the world bounds (6) and the four widths R0, R1, R2, Rd (4).
struct Capsule { f3 a, b, d; float radius, r2, dd; f3 qmn, qmx; float R0, R1, R2, Rd; };

// Whether a query is walked at all: seven finite floats and radius >= 0 (-0 is legal; a == b is a ball, radius == 0 a segment).
MI_HD bool capsule_query_valid(f3 a, f3 b, float radius) {
  return fabsf(a.x) < kInf && fabsf(a.y) < kInf && fabsf(a.z) < kInf && fabsf(b.x) < kInf && fabsf(b.y) < kInf && fabsf(b.z) < kInf &&
         fabsf(radius) < kInf && radius >= 0.f;
}

// The smallest normal binary32, 2^-126: a squared length below it has lost bits, or all of them.
constexpr float kCapsuleMinNormal = 1.17549435e-38f;

// The width of the capsule on an axis of squared length ll: radius sqrtf(ll), and +inf - an axis that separates nothing - where ll
// lies below the smallest normal binary32 (a == b, or a segment so short that its square underflows: radius sqrtf(ll) would be 0
// or short of its bits while the products X_k dh_k are not, and would part the ball from boxes that it reaches).
MI_HD float capsule_axis_width(float radius, float ll) { return ll >= kCapsuleMinNormal ? radius * sqrtf(ll) : kInf; }

// The whole query from its seven floats. R_i = capsule_axis_width(radius, X_i.X_i), the squares of the two non-zero components
// added in the order of their index: X0: d.z d.z + d.y d.y, X1: d.z d.z + d.x d.x, X2: d.y d.y + d.x d.x. Rd likewise from dd.
MI_HD Capsule capsule_make(f3 a, f3 b, float radius) {
  Capsule q;
  q.a = a;
  q.b = b;
  q.d = b - a;
  q.radius = radius;
  q.r2 = radius * radius;
  q.dd = dot(q.d, q.d);
  q.qmn = mk(sel_min(a.x, b.x) - radius, sel_min(a.y, b.y) - radius, sel_min(a.z, b.z) - radius);
  q.qmx = mk(sel_max(a.x, b.x) + radius, sel_max(a.y, b.y) + radius, sel_max(a.z, b.z) + radius);
  const float xx = q.d.x * q.d.x, yy = q.d.y * q.d.y, zz = q.d.z * q.d.z;
  q.R0 = capsule_axis_width(radius, zz + yy);
  q.R1 = capsule_axis_width(radius, zz + xx);
  q.R2 = capsule_axis_width(radius, yy + xx);
  q.Rd = capsule_axis_width(radius, q.dd);
  return q;
}

// One lateral axis: its two non-zero components p (at the lower index) and s, against the offsets of the bounds on those two
// world axes. Relative to a the segment projects onto 0 and the ball widens that to +-R. Bitwise |: nothing to branch around.
MI_HD bool capsule_lateral_separates(float p, float s, float R, float dlp, float dhp, float dls, float dhs) {
  const bool pp = p > 0.f, ps = s > 0.f;
  const float up = (pp ? p * dhp : p * dlp) + (ps ? s * dhs : s * dls);
  const float dn = (pp ? p * dlp : p * dhp) + (ps ? s * dls : s * dhs);
  return (dn > R) | (up < -R);
}

// The bounds [mn, mx] against the query: the six closed compares against the world bounds, the three lateral axes cross(d, e_k)
// and the axis d itself, on which the segment projects onto [0, dd] and the ball widens that by Rd. A node's box is entered on it;
// unchanged, it is the first step of every primitive test, on the primitive's own bounds. Every operation is monotone in mn
// (falling) and mx (rising) as computed - fl(a - c), fl(x a) for a fixed x and fl(a + b) are - so bounds that contain other bounds
// pass whenever those pass: a primitive whose bounds pass has every ancestor's box pass. Written with & and |:
// the result selects between nd.hit and nd.link.
MI_HD bool capsule_meets_bounds(f3 mn, f3 mx, const Capsule& q) {
  const bool meets = (mn.x <= q.qmx.x) & (mx.x >= q.qmn.x) & (mn.y <= q.qmx.y) & (mx.y >= q.qmn.y) & (mn.z <= q.qmx.z) & (mx.z >= q.qmn.z);
  const f3 dl = mn - q.a, dh = mx - q.a;
  const bool s0 = capsule_lateral_separates(q.d.z, -q.d.y, q.R0, dl.y, dh.y, dl.z, dh.z);
  const bool s1 = capsule_lateral_separates(-q.d.z, q.d.x, q.R1, dl.x, dh.x, dl.z, dh.z);
  const bool s2 = capsule_lateral_separates(q.d.y, -q.d.x, q.R2, dl.x, dh.x, dl.y, dh.y);
  const bool px = q.d.x > 0.f, py = q.d.y > 0.f, pz = q.d.z > 0.f;
  const float up = ((px ? q.d.x * dh.x : q.d.x * dl.x) + (py ? q.d.y * dh.y : q.d.y * dl.y)) + (pz ? q.d.z * dh.z : q.d.z * dl.z);
  const float dn = ((px ? q.d.x * dl.x : q.d.x * dh.x) + (py ? q.d.y * dl.y : q.d.y * dh.y)) + (pz ? q.d.z * dl.z : q.d.z * dh.z);
  const bool sd = (dn > q.dd + q.Rd) | (up < -q.Rd);
  return meets & !s0 & !s1 & !s2 & !sd;
}

// The squared distance of p from the segment: t = dot(p - a, d); t <= 0: the end a; t >= dd: the end b; else the point
// a + d (t / dd). A NaN t fails both compares and gives a NaN distance, which rejects nothing.
MI_HD float capsule_point_seg_dist2(const Capsule& q, f3 p) {
  const float t = dot(p - q.a, q.d);
  if (t <= 0.f) return point_dist2(p, q.a);
  if (t >= q.dd) return point_dist2(p, q.b);
  return point_dist2(p, q.a + q.d * (t / q.dd));
}

MI_HD float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// The squared distance of the segments [p1, p1 + d1] (aa = d1.d1) and [p2, q2]: Ericson, Real-Time Collision Detection §5.1.9,
// without its epsilon. d2 = q2 - p2, r = p1 - p2, e = d2.d2, f = d2.r; both lengths <= 0: r.r. aa <= 0: s = 0, t = clamp(f / e).
// Else c = d1.r; e <= 0: t = 0, s = clamp(-c / aa). Else b = d1.d2, denom = aa e - b b, s = denom != 0 ? clamp((b f - c e) /
// denom) : 0, t = (b s + f) / e; t < 0: t = 0, s = clamp(-c / aa); t > 1: t = 1, s = clamp((b - c) / aa). The result is
// dot(c1 - c2, c1 - c2), c1 = p1 + d1 s, c2 = p2 + d2 t. clamp(x) = x < 0 ? 0 : x > 1 ? 1 : x: a NaN stays a NaN.
MI_HD float seg_seg_dist2(f3 p1, f3 d1, float aa, f3 p2, f3 q2) {
  const f3 d2 = q2 - p2, r = p1 - p2;
  const float e = dot(d2, d2), f = dot(d2, r);
  if (aa <= 0.f && e <= 0.f) return dot(r, r);
  float s, t;
  if (aa <= 0.f) {
    s = 0.f;
    t = clamp01(f / e);
  } else {
    const float c = dot(d1, r);
    if (e <= 0.f) {
      t = 0.f;
      s = clamp01(-c / aa);
    } else {
      const float b = dot(d1, d2);
      const float denom = aa * e - b * b;
      s = denom != 0.f ? clamp01((b * f - c * e) / denom) : 0.f;
      t = (b * s + f) / e;
      if (t < 0.f) {
        t = 0.f;
        s = clamp01(-c / aa);
      } else if (t > 1.f) {
        t = 1.f;
        s = clamp01((b - c) / aa);
      }
    }
  }
  const f3 c1 = p1 + d1 * s, c2 = p2 + d2 * t;
  const f3 v = c1 - c2;
  return dot(v, v);
}

// tri_point_dist2 of the contract, the squared distance of p from the triangle: closest_on_triangle and point_dist2 as they stand
// (contact_math.hpp has the same under that name; this file sits over point_math.hpp and box_math.hpp alone).
MI_HD float capsule_tri_point_dist2(f3 A, f3 B, f3 C, f3 p) { return point_dist2(p, closest_on_triangle(A, B, C, p).q); }

// The segment crosses the triangle's face: the ends not strictly on one side of the plane and not both in it, and the three
// scalar triple products of d with the vertices as seen from a of one sign (zero goes with either).
MI_HD bool capsule_pierces_triangle(const Capsule& q, f3 A, f3 B, f3 C) {
  const f3 n = cross(B - A, C - A);
  const float sa = dot(n, q.a - A), sb = dot(n, q.b - A);
  const bool sides = !((sa > 0.f) & (sb > 0.f)) & !((sa < 0.f) & (sb < 0.f)) & !((sa == 0.f) & (sb == 0.f));
  const f3 u0 = A - q.a, u1 = B - q.a, u2 = C - q.a;
  const float w0 = dot(q.d, cross(u0, u1)), w1 = dot(q.d, cross(u1, u2)), w2 = dot(q.d, cross(u2, u0));
  return sides & (((w0 >= 0.f) & (w1 >= 0.f) & (w2 >= 0.f)) | ((w0 <= 0.f) & (w1 <= 0.f) & (w2 <= 0.f)));
}

// Triangle (A, B, C), its bounds already met: an end of the segment within the radius (a, then b), the segment within the radius
// of an edge (AB, BC, CA), or the segment through the face. The sub-tests run as early-outs in this order.
MI_HD bool capsule_touches_triangle(const Capsule& q, f3 A, f3 B, f3 C) {
  if (!(capsule_tri_point_dist2(A, B, C, q.a) > q.r2)) return true;
  if (!(capsule_tri_point_dist2(A, B, C, q.b) > q.r2)) return true;
  if (!(seg_seg_dist2(q.a, q.d, q.dd, A, B) > q.r2)) return true;
  if (!(seg_seg_dist2(q.a, q.d, q.dd, B, C) > q.r2)) return true;
  if (!(seg_seg_dist2(q.a, q.d, q.dd, C, A) > q.r2)) return true;
  return capsule_pierces_triangle(q, A, B, C);
}

// The primitive of a leaf record (kind and f as box_touches_prim takes them): capsule_meets_bounds on the primitive's own
// bounds, then the test of its kind. *contained means something only for a touching primitive: a triangle's three vertices
// within the radius of the segment (exact: the capsule is convex); a sphere or a disc whose farthest point from the segment,
// sqrtf(dmin2) + its radius, is (a disc: sufficient, never set wrongly).
MI_HD bool capsule_touches_prim(uint32_t kind, const float* f, const Capsule& q, bool* contained) {
  f3 mn, mx;
  *contained = false;
  if (kind == 0u) {
    const f3 A = mk(f[0], f[1], f[2]), B = mk(f[3], f[4], f[5]), C = mk(f[6], f[7], f[8]);
    triangle_bounds(A, B, C, mn, mx);
    if (!capsule_meets_bounds(mn, mx, q)) return false;
    if (!capsule_touches_triangle(q, A, B, C)) return false;
    *contained = capsule_point_seg_dist2(q, A) <= q.r2 && capsule_point_seg_dist2(q, B) <= q.r2 && capsule_point_seg_dist2(q, C) <= q.r2;
    return true;
  }
  if (kind == 1u) {
    // Sphere (centre c, radius R): the shell is reached from outside - dmin2 <= (R + radius)^2 - and from inside: a capsule
    // wholly inside the ball, its farthest end nearer than R - radius, touches nothing.
    const f3 c = mk(f[0], f[1], f[2]);
    const float R = f[3];
    sphere_bounds(c, R, mn, mx);
    if (!capsule_meets_bounds(mn, mx, q)) return false;
    const float dmin2 = capsule_point_seg_dist2(q, c);
    const float dmax2 = sel_max(point_dist2(q.a, c), point_dist2(q.b, c));
    const float s = R + q.radius, m = R - q.radius;
    if (!(!(dmin2 > s * s) && !(m > 0.f && dmax2 < m * m))) return false;
    *contained = sqrtf(dmin2) + R <= q.radius;
    return true;
  }
  // Disc (normal n taken as given, centre c, r2 = the squared radius as the leaf record holds it, r' = sqrtf(r2)). CONSERVATIVE:
  // its tight bounds, the plane's slab widened by rn = radius sqrtf(n.n), and the ball of r' about c.
  const f3 n = mk(f[0], f[1], f[2]), c = mk(f[3], f[4], f[5]);
  disc_bounds(n, c, f[6], mn, mx);
  if (!capsule_meets_bounds(mn, mx, q)) return false;
  const float sa = dot(n, q.a - c), sb = dot(n, q.b - c), rn = q.radius * sqrtf(dot(n, n));
  if (!(!(sa > rn && sb > rn) && !(sa < -rn && sb < -rn))) return false;
  const float rp = sqrtf(f[6]), s = rp + q.radius;
  const float dmin2 = capsule_point_seg_dist2(q, c);
  if (dmin2 > s * s) return false;
  *contained = sqrtf(dmin2) + rp <= q.radius;
  return true;
}

// The capsules as a touch family (touch_kernels.hpp).
struct CapsuleShape {
  using Item = mi_capsule;
  using Record = mi_overlap;
  struct Fields { f3 a, b; float radius; };
  using Carried = Capsule;
  static constexpr int kAny = MI_CAPSULE_ANY, kCount = MI_CAPSULE_COUNT;
  static constexpr size_t kAlign = 16;
  static constexpr const char *kNoun = "capsules", *kKindBad = "unknown capsule kind", *kAlignBad = "capsules must be 16-byte aligned";
  static MI_HD Fields fields(const mi_capsule& c) { return {mk(c.a[0], c.a[1], c.a[2]), mk(c.b[0], c.b[1], c.b[2]), c.radius}; }
  static MI_HD bool valid(const Fields& c) { return capsule_query_valid(c.a, c.b, c.radius); }
  static MI_HD Carried carry(const Fields& c) { return capsule_make(c.a, c.b, c.radius); }
  static MI_HD bool meets_bounds(f3 mn, f3 mx, const Carried& q) { return capsule_meets_bounds(mn, mx, q); }
  static MI_HD bool touches_prim(uint32_t kind, const float* f, const Carried& q, bool* contained) { return capsule_touches_prim(kind, f, q, contained); }
  static MI_HD uint32_t flags(bool contained) { return overlap_flags(contained); }
};

}  // namespace mi
