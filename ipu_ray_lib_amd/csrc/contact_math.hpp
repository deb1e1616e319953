// contact_math.hpp — the arithmetic of triangle queries (mi_tri_query* / mi_tri_offsets* / mi_tri_fill*, include/mi_raylib.h, where
// the contract is written): whether a caller's triangle (q0, q1, q2) touches a scene triangle, a sphere's shell or a disc. One
// definition, compiled by hipcc for the kernels (contact_kernels.hpp) and by g++ for the host twin (host/touch_host.hpp over TriShape):
// compares, selects and single binary32 operations in the order written (no contraction, correctly rounded sqrt and divide on both
// sides), so the two return the same bits. dot and cross are ray_math.h's; minima and maxima are sel_min / sel_max (box_math.hpp).
//
// Everything is CLOSED: contact counts. Every separation is a strict compare that a NaN fails, so a NaN never separates and a
// query so large that its arithmetic overflows errs towards listing. Every test starts with the primitive's own bounds - those the
// box queries define (triangle_bounds, sphere_bounds, disc_bounds) - against the query's bounds [qmn, qmx].
#pragma once

#include "box_math.hpp"

namespace mi {

// Whether a triangle query is walked at all: nine finite coordinates. A collapsed triangle (a segment, a point) is legal.
MI_HD bool tri_query_valid(f3 q0, f3 q1, f3 q2) {
  return fabsf(q0.x) < kInf && fabsf(q0.y) < kInf && fabsf(q0.z) < kInf && fabsf(q1.x) < kInf && fabsf(q1.y) < kInf && fabsf(q1.z) < kInf &&
         fabsf(q2.x) < kInf && fabsf(q2.y) < kInf && fabsf(q2.z) < kInf;
}

// One axis x of the separating-axis test, everything relative to q0: the scene triangle's moved vertices u0, u1, u2 and the
// query's v0 = 0, v1, v2 are projected, pT_i = dot(x, u_i), pQ_0 = 0, pQ_j = dot(x, v_j); x separates exactly when every pT lies
// strictly above every pQ or every pT strictly below every pQ - nine pairs each way, each a compare that a NaN fails. A zero axis
// projects everything to 0 and separates nothing.
MI_HD bool tri_axis_separates(f3 x, f3 u0, f3 u1, f3 u2, f3 v1, f3 v2) {
  const float t0 = dot(x, u0), t1 = dot(x, u1), t2 = dot(x, u2);
  const float s0 = 0.f, s1 = dot(x, v1), s2 = dot(x, v2);
  const bool above = t0 > s0 && t0 > s1 && t0 > s2 && t1 > s0 && t1 > s1 && t1 > s2 && t2 > s0 && t2 > s1 && t2 > s2;
  const bool below = t0 < s0 && t0 < s1 && t0 < s2 && t1 < s0 && t1 < s1 && t1 < s2 && t2 < s0 && t2 < s1 && t2 < s2;
  return above || below;
}

// Scene triangle (a, b, c) against the query: its bounds, then 17 axes in this order - the query's normal nQ, the triangle's
// normal nT, the nine cross(e_i, f_j) (i outer, j inner), cross(nT, e_i), cross(nQ, f_j). The last six decide coplanar pairs, where
// the first eleven are zero or normal to the common plane. The vertices are moved by q0 first (u = a - q0, ...): the products then
// carry the size of the pair's separation and not of its coordinates, which is what keeps a far-away pair's projections apart.
// Spelled out axis by axis: e_i, f_j and the moved vertices are named values, nothing is indexed.
MI_HD bool tri_touches_triangle(f3 a, f3 b, f3 c, f3 q0, f3 q1, f3 q2, f3 qmn, f3 qmx) {
  f3 mn, mx;
  triangle_bounds(a, b, c, mn, mx);
  if (!box_meets_bounds(mn, mx, qmn, qmx)) return false;
  const f3 u0 = a - q0, u1 = b - q0, u2 = c - q0;
  const f3 v1 = q1 - q0, v2 = q2 - q0;
  const f3 e0 = u1 - u0, e1 = u2 - u1, e2 = u0 - u2;
  const f3 f0 = v1, f1 = v2 - v1, f2 = mk(-v2.x, -v2.y, -v2.z);
  const f3 nT = cross(e0, e1), nQ = cross(f0, f1);
  if (tri_axis_separates(nQ, u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(nT, u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e0, f0), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e0, f1), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e0, f2), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e1, f0), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e1, f1), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e1, f2), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e2, f0), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e2, f1), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(e2, f2), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(nT, e0), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(nT, e1), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(nT, e2), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(nQ, f0), u0, u1, u2, v1, v2)) return false;
  if (tri_axis_separates(cross(nQ, f1), u0, u1, u2, v1, v2)) return false;
  return !tri_axis_separates(cross(nQ, f2), u0, u1, u2, v1, v2);
}

// The squared distance of p from the query triangle: the point queries' closest point (point_math.hpp), as it stands.
MI_HD float tri_point_dist2(f3 q0, f3 q1, f3 q2, f3 p) { return point_dist2(p, closest_on_triangle(q0, q1, q2, p).q); }

// Sphere (centre c, radius, r2 = the squared radius as the leaf record holds it): queries see SURFACES, so the triangle touches
// the sphere when it reaches the shell from outside and from inside - its nearest point no farther than the radius, its farthest
// point, which is a vertex, no nearer: !(dmin2 > r2) && !(dmax2 < r2).
MI_HD bool tri_touches_sphere(f3 c, float radius, float r2, f3 q0, f3 q1, f3 q2, f3 qmn, f3 qmx) {
  f3 mn, mx;
  sphere_bounds(c, radius, mn, mx);
  if (!box_meets_bounds(mn, mx, qmn, qmx)) return false;
  const float dmin2 = tri_point_dist2(q0, q1, q2, c);
  const float dmax2 = sel_max(sel_max(point_dist2(q0, c), point_dist2(q1, c)), point_dist2(q2, c));
  return !(dmin2 > r2) && !(dmax2 < r2);
}

// Disc (normal n taken as given, centre c, r2). CONSERVATIVE, as for boxes: three necessary conditions, all of which must hold -
// the disc's tight bounds meet the query's; the triangle meets the disc's plane: s_i = dot(n, q_i - c) neither all > 0 nor all < 0;
// the triangle meets the ball of the disc's radius about its centre: !(dmin2 of c > r2). No touching disc is missed (up to the
// rounding of these operations); a triangle that passes the rim may be listed without touching.
MI_HD bool tri_touches_disc(f3 n, f3 c, float r2, f3 q0, f3 q1, f3 q2, f3 qmn, f3 qmx) {
  f3 mn, mx;
  disc_bounds(n, c, r2, mn, mx);
  if (!box_meets_bounds(mn, mx, qmn, qmx)) return false;
  const float s0 = dot(n, q0 - c), s1 = dot(n, q1 - c), s2 = dot(n, q2 - c);
  if ((s0 > 0.f && s1 > 0.f && s2 > 0.f) || (s0 < 0.f && s1 < 0.f && s2 < 0.f)) return false;
  return !(tri_point_dist2(q0, q1, q2, c) > r2);
}

// The query's bounds: the per-axis select-min and select-max of its vertices (triangle_bounds: compares only).
MI_HD void tri_query_bounds(f3 q0, f3 q1, f3 q2, f3& qmn, f3& qmx) { triangle_bounds(q0, q1, q2, qmn, qmx); }

// The primitive in the first 40 bytes of a leaf record, as box_touches_prim reads it: kind = LEAF_* (0 triangle, 1 sphere, 2 disc),
// f = tri: a, b, c | sphere: centre, radius, radius2 | disc: n, centre, r2.
MI_HD bool tri_touches_prim(uint32_t kind, const float* f, f3 q0, f3 q1, f3 q2, f3 qmn, f3 qmx) {
  if (kind == 0u) return tri_touches_triangle(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), mk(f[6], f[7], f[8]), q0, q1, q2, qmn, qmx);
  if (kind == 1u) return tri_touches_sphere(mk(f[0], f[1], f[2]), f[3], f[4], q0, q1, q2, qmn, qmx);
  return tri_touches_disc(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), f[6], q0, q1, q2, qmn, qmx);
}

// The triangles as a touch family (touch_kernels.hpp): the walk carries the vertices and their bounds, a contact
// record has no flags, and a batch is a float32 [n, 3, 3] array - 4-byte aligned.
struct TriShape {
  using Item = mi_tri;
  using Record = mi_contact;
  struct Fields { f3 q0, q1, q2; };
  struct Carried { f3 q0, q1, q2, qmn, qmx; };
  static constexpr int kAny = MI_TRI_ANY, kCount = MI_TRI_COUNT;
  static constexpr size_t kAlign = 4;
  static constexpr const char *kNoun = "triangles", *kKindBad = "unknown triangle kind", *kAlignBad = "triangles must be 4-byte aligned";
  static MI_HD Fields fields(const mi_tri& t) { return {mk(t.a[0], t.a[1], t.a[2]), mk(t.b[0], t.b[1], t.b[2]), mk(t.c[0], t.c[1], t.c[2])}; }
  static MI_HD bool valid(const Fields& t) { return tri_query_valid(t.q0, t.q1, t.q2); }
  static MI_HD Carried carry(const Fields& t) {
    Carried q = {t.q0, t.q1, t.q2, {}, {}};
    tri_query_bounds(q.q0, q.q1, q.q2, q.qmn, q.qmx);
    return q;
  }
  static MI_HD bool meets_bounds(f3 mn, f3 mx, const Carried& q) { return box_meets_bounds(mn, mx, q.qmn, q.qmx); }
  static MI_HD bool touches_prim(uint32_t kind, const float* f, const Carried& q, bool* contained) {
    *contained = false;
    return tri_touches_prim(kind, f, q.q0, q.q1, q.q2, q.qmn, q.qmx);
  }
  static MI_HD uint32_t flags(bool) { return 0u; }
};

}  // namespace mi
