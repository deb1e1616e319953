// frustum_math.hpp — the arithmetic of frustum queries (mi_frustum_query* / mi_frustum_offsets* / mi_frustum_fill*,
// include/mi_raylib.h, where the contract is written): whether the region that six caller-supplied planes leave - a camera's view
// volume, a screen tile's sub-frustum, a half-space, a slab - touches a node's box, a triangle, a sphere or a disc. One
// definition, compiled by hipcc for the kernels (frustum_kernels.hpp) and by g++ for the host twin
// (host/touch_host.hpp over FrustumShape): every function is a sequence of compares, selects and single binary32 operations in the order
// written (no contraction, correctly rounded divide and sqrt on both sides), so the two return the same bits. The primitives'
// bounds are box_math.hpp's: nothing of them is repeated here.
//
// Everything is CLOSED. The region has no finite world bounds: the planes are all there is, at the nodes and at the leaves. The
// planes live in named members and every loop over planes, edges and pairs of planes is written out: nothing is indexed.
#pragma once

#include "box_math.hpp"

namespace mi {

// One plane n.p + d >= 0, the normal pointing inward and not necessarily unit. Four zeros: absent, it holds everywhere.
struct FPlane { float x, y, z, d; };

// A query as the walk carries it: the six planes, 24 floats, every member named.
struct Frustum { FPlane p0, p1, p2, p3, p4, p5; };

MI_HD bool frustum_plane_finite(const FPlane& p) {
  const float ax = fabsf(p.x), ay = fabsf(p.y), az = fabsf(p.z), ad = fabsf(p.d);
  return (ax < kInf) & (ay < kInf) & (az < kInf) & (ad < kInf);
}

// Whether a query is walked at all: 24 finite floats. A zero normal with d < 0 and contradictory planes are valid; they list
// nothing by the arithmetic below.
MI_HD bool frustum_query_valid(const Frustum& q) {
  const bool v0 = frustum_plane_finite(q.p0), v1 = frustum_plane_finite(q.p1), v2 = frustum_plane_finite(q.p2), v3 = frustum_plane_finite(q.p3),
             v4 = frustum_plane_finite(q.p4), v5 = frustum_plane_finite(q.p5);
  return v0 & v1 & v2 & v3 & v4 & v5;
}

// s = n.V + d = ((n.x V.x + n.y V.y) + n.z V.z) + d
MI_HD float frustum_plane_at(const FPlane& p, f3 v) { return ((p.x * v.x + p.y * v.y) + p.z * v.z) + p.d; }

// The corner of the bounds farthest along n lies behind the plane: t_k = n_k > 0 ? n_k mx_k : n_k mn_k, up = ((t0 + t1) + t2) + d,
// up < 0. A NaN separates nothing.
MI_HD bool frustum_plane_separates(const FPlane& p, f3 mn, f3 mx) {
  const float t0 = p.x > 0.f ? p.x * mx.x : p.x * mn.x;
  const float t1 = p.y > 0.f ? p.y * mx.y : p.y * mn.y;
  const float t2 = p.z > 0.f ? p.z * mx.z : p.z * mn.z;
  return ((t0 + t1) + t2) + p.d < 0.f;
}

// The bounds [mn, mx] against the region: no plane has the whole of them behind it. A node's box is entered on it; unchanged, it
// is the first step of every primitive test, on the primitive's own bounds. Every operation is monotone in mn (falling) and mx
// (rising) as computed - fl(x a) for a fixed x and fl(a + b) are - so bounds that contain other bounds pass whenever those pass
// (DESIGN.md §37). Written with |: the result selects between nd.hit and nd.link.
MI_HD bool frustum_meets_bounds(f3 mn, f3 mx, const Frustum& q) {
  const bool s0 = frustum_plane_separates(q.p0, mn, mx), s1 = frustum_plane_separates(q.p1, mn, mx), s2 = frustum_plane_separates(q.p2, mn, mx),
             s3 = frustum_plane_separates(q.p3, mn, mx), s4 = frustum_plane_separates(q.p4, mn, mx), s5 = frustum_plane_separates(q.p5, mn, mx);
  return !(s0 | s1 | s2 | s3 | s4 | s5);
}

// The six plane values of one point, and whether it lies in the region (all six >= 0).
struct FSix { float s0, s1, s2, s3, s4, s5; };
MI_HD FSix frustum_six(const Frustum& q, f3 v) {
  FSix s;
  s.s0 = frustum_plane_at(q.p0, v);
  s.s1 = frustum_plane_at(q.p1, v);
  s.s2 = frustum_plane_at(q.p2, v);
  s.s3 = frustum_plane_at(q.p3, v);
  s.s4 = frustum_plane_at(q.p4, v);
  s.s5 = frustum_plane_at(q.p5, v);
  return s;
}
MI_HD bool frustum_six_inside(const FSix& s) { return (s.s0 >= 0.f) & (s.s1 >= 0.f) & (s.s2 >= 0.f) & (s.s3 >= 0.f) & (s.s4 >= 0.f) & (s.s5 >= 0.f); }

// One plane's cut of the edge's parameter interval [t0, t1], from the plane's values sa and sb at the two ends: both negative,
// the edge misses; the first negative, t0 = sel_max(t0, sa / (sa - sb)); otherwise the second negative, t1 = sel_min(t1, sa /
// (sa - sb)). Scalar state only.
MI_HD void frustum_clip_plane(float sa, float sb, float& t0, float& t1, bool& miss) {
  const bool na = sa < 0.f, nb = sb < 0.f;
  miss |= na & nb;
  if (na != nb) {
    const float t = sa / (sa - sb);
    if (na) t0 = sel_max(t0, t);
    else t1 = sel_min(t1, t);
  }
}

// The edge whose ends have the plane values a and b passes through the region: [0, 1] cut by the six planes is not empty.
MI_HD bool frustum_edge_touches(const FSix& a, const FSix& b) {
  float t0 = 0.f, t1 = 1.f;
  bool miss = false;
  frustum_clip_plane(a.s0, b.s0, t0, t1, miss);
  frustum_clip_plane(a.s1, b.s1, t0, t1, miss);
  frustum_clip_plane(a.s2, b.s2, t0, t1, miss);
  frustum_clip_plane(a.s3, b.s3, t0, t1, miss);
  frustum_clip_plane(a.s4, b.s4, t0, t1, miss);
  frustum_clip_plane(a.s5, b.s5, t0, t1, miss);
  return !miss & (t0 <= t1);
}

// The point x where the planes pi and pj meet the triangle's plane (normal m = (B - A) x (C - A), mA = m.A): c = n_i x n_j,
// det = c.m, skipped unless det != 0; u = n_j x m, w = m x n_i, x_k = (((-d_i) u_k - d_j w_k) + mA c_k) / det. The triangle is
// touched there when x satisfies the other four planes and lies in the triangle: m.((B - A) x (x - A)), m.((C - B) x (x - B)) and
// m.((A - C) x (x - C)) all >= 0. A NaN fails the compares.
MI_HD bool frustum_corner_in_face(const FPlane& pi, const FPlane& pj, const FPlane& pa, const FPlane& pb, const FPlane& pc, const FPlane& pd, f3 A, f3 B, f3 C,
                                  f3 m, float mA) {
  const f3 ni = mk(pi.x, pi.y, pi.z), nj = mk(pj.x, pj.y, pj.z);
  const f3 c = cross(ni, nj);
  const float det = dot(c, m);
  if (!(det != 0.f)) return false;
  const f3 u = cross(nj, m), w = cross(m, ni);
  const float ndi = -pi.d;
  const f3 x = mk(((ndi * u.x - pj.d * w.x) + mA * c.x) / det, ((ndi * u.y - pj.d * w.y) + mA * c.y) / det, ((ndi * u.z - pj.d * w.z) + mA * c.z) / det);
  const float xa = frustum_plane_at(pa, x), xb = frustum_plane_at(pb, x), xc = frustum_plane_at(pc, x), xd = frustum_plane_at(pd, x);
  const bool in_planes = (xa >= 0.f) & (xb >= 0.f) & (xc >= 0.f) & (xd >= 0.f);
  const float e0 = dot(m, cross(B - A, x - A)), e1 = dot(m, cross(C - B, x - B)), e2 = dot(m, cross(A - C, x - C));
  return in_planes & (e0 >= 0.f) & (e1 >= 0.f) & (e2 >= 0.f);
}

// The region passes through the face: some corner of its cross-section with the triangle's plane - where two of the six planes
// meet that plane - lies in the region and in the triangle. The 15 pairs i < j in order.
MI_HD bool frustum_through_face(const Frustum& q, f3 A, f3 B, f3 C) {
  const f3 m = cross(B - A, C - A);
  const float mA = dot(m, A);
  if (frustum_corner_in_face(q.p0, q.p1, q.p2, q.p3, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p0, q.p2, q.p1, q.p3, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p0, q.p3, q.p1, q.p2, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p0, q.p4, q.p1, q.p2, q.p3, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p0, q.p5, q.p1, q.p2, q.p3, q.p4, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p1, q.p2, q.p0, q.p3, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p1, q.p3, q.p0, q.p2, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p1, q.p4, q.p0, q.p2, q.p3, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p1, q.p5, q.p0, q.p2, q.p3, q.p4, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p2, q.p3, q.p0, q.p1, q.p4, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p2, q.p4, q.p0, q.p1, q.p3, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p2, q.p5, q.p0, q.p1, q.p3, q.p4, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p3, q.p4, q.p0, q.p1, q.p2, q.p5, A, B, C, m, mA)) return true;
  if (frustum_corner_in_face(q.p3, q.p5, q.p0, q.p1, q.p2, q.p4, A, B, C, m, mA)) return true;
  return frustum_corner_in_face(q.p4, q.p5, q.p0, q.p1, q.p2, q.p3, A, B, C, m, mA);
}

// Triangle (A, B, C), its bounds already met. The 18 plane values serve the first two stages: a vertex in the region (all three:
// *contained, exact since the region is convex); an edge through the region (AB, BC, CA); the region through the face. The stages
// run as early-outs in this order.
MI_HD bool frustum_touches_triangle(const Frustum& q, f3 A, f3 B, f3 C, bool* contained) {
  const FSix sa = frustum_six(q, A), sb = frustum_six(q, B), sc = frustum_six(q, C);
  const bool ia = frustum_six_inside(sa), ib = frustum_six_inside(sb), ic = frustum_six_inside(sc);
  *contained = ia & ib & ic;
  if (ia | ib | ic) return true;
  if (frustum_edge_touches(sa, sb)) return true;
  if (frustum_edge_touches(sb, sc)) return true;
  if (frustum_edge_touches(sc, sa)) return true;
  return frustum_through_face(q, A, B, C);
}

// One plane against the ball (c, R2 = its squared radius): s = n.c + d, nn = n.n. The whole ball lies behind the plane when
// s < 0 && s s > R2 nn; the whole ball lies in front of it (the plane included) when s >= 0 && s s >= R2 nn.
MI_HD void frustum_plane_ball(const FPlane& p, f3 c, float R2, bool& rejects, bool& holds) {
  const float s = frustum_plane_at(p, c), nn = dot(mk(p.x, p.y, p.z), mk(p.x, p.y, p.z));
  const float ss = s * s, rn = R2 * nn;
  rejects |= (s < 0.f) & (ss > rn);
  holds &= (s >= 0.f) & (ss >= rn);
}

// CONSERVATIVE: the ball is rejected only when some plane has the whole of it behind it. *contained: every plane has the whole
// ball in front of it - exact for a ball.
MI_HD bool frustum_touches_ball(const Frustum& q, f3 c, float R2, bool* contained) {
  bool rejects = false, holds = true;
  frustum_plane_ball(q.p0, c, R2, rejects, holds);
  frustum_plane_ball(q.p1, c, R2, rejects, holds);
  frustum_plane_ball(q.p2, c, R2, rejects, holds);
  frustum_plane_ball(q.p3, c, R2, rejects, holds);
  frustum_plane_ball(q.p4, c, R2, rejects, holds);
  frustum_plane_ball(q.p5, c, R2, rejects, holds);
  *contained = holds;
  return !rejects;
}

// The primitive of a leaf record (kind and f as box_touches_prim takes them): frustum_meets_bounds on the primitive's own bounds,
// then the test of its kind. *contained means something only for a touching primitive. A sphere (centre, radius R) is the ball of
// R2 = R R; a disc (n, centre, r2 as the leaf record holds it) its tight bounds, then the ball of r2 about its centre.
MI_HD bool frustum_touches_prim(uint32_t kind, const float* f, const Frustum& q, bool* contained) {
  f3 mn, mx;
  *contained = false;
  if (kind == 0u) {
    const f3 A = mk(f[0], f[1], f[2]), B = mk(f[3], f[4], f[5]), C = mk(f[6], f[7], f[8]);
    triangle_bounds(A, B, C, mn, mx);
    if (!frustum_meets_bounds(mn, mx, q)) return false;
    return frustum_touches_triangle(q, A, B, C, contained);
  }
  if (kind == 1u) {
    const f3 c = mk(f[0], f[1], f[2]);
    const float R = f[3];
    sphere_bounds(c, R, mn, mx);
    if (!frustum_meets_bounds(mn, mx, q)) return false;
    return frustum_touches_ball(q, c, R * R, contained);
  }
  const f3 n = mk(f[0], f[1], f[2]), c = mk(f[3], f[4], f[5]);
  disc_bounds(n, c, f[6], mn, mx);
  if (!frustum_meets_bounds(mn, mx, q)) return false;
  return frustum_touches_ball(q, c, f[6], contained);
}

// The frusta as a touch family (touch_kernels.hpp): the six planes are what the walk carries, as given.
struct FrustumShape {
  using Item = mi_frustum;
  using Record = mi_overlap;
  using Fields = Frustum;
  using Carried = Frustum;
  static constexpr int kAny = MI_FRUSTUM_ANY, kCount = MI_FRUSTUM_COUNT;
  static constexpr size_t kAlign = 16;
  static constexpr const char *kNoun = "frusta", *kKindBad = "unknown frustum kind", *kAlignBad = "frusta must be 16-byte aligned";
  static MI_HD FPlane plane(const float p[4]) { return {p[0], p[1], p[2], p[3]}; }
  static MI_HD Fields fields(const mi_frustum& f) {
    return {plane(f.planes[0]), plane(f.planes[1]), plane(f.planes[2]), plane(f.planes[3]), plane(f.planes[4]), plane(f.planes[5])};
  }
  static MI_HD bool valid(const Fields& q) { return frustum_query_valid(q); }
  static MI_HD const Carried& carry(const Fields& q) { return q; }
  static MI_HD bool meets_bounds(f3 mn, f3 mx, const Carried& q) { return frustum_meets_bounds(mn, mx, q); }
  static MI_HD bool touches_prim(uint32_t kind, const float* f, const Carried& q, bool* contained) { return frustum_touches_prim(kind, f, q, contained); }
  static MI_HD uint32_t flags(bool contained) { return overlap_flags(contained); }
};

}  // namespace mi
