// point_math.hpp — the arithmetic of point queries (mi_point_query / mi_point_query_device, include/mi_raylib.h): the squared
// distance of a point from a node's box and the closest point of a triangle, a sphere and a disc. One definition, compiled by
// hipcc for point_query_kernel (point_kernels.hpp) and by g++ for the host twin (host/point_query_host.cpp): every function is a
// sequence of single binary32 operations in the order written (no contraction, correctly rounded divide and sqrt on both sides),
// so the two return the same bits. A dot product is (x x' + y y') + z z' (ray_math.h dot).
#pragma once

#include "ray_math.h"

namespace mi {

// Squared distance of p from the box [min, max]: per axis the excess max(min - p, p - max, 0), then (ex ex + ey ey) + ez ez.
// A finite p and a finite box give no NaN: an excess that overflows is +inf, and +inf is never below a bound.
MI_HD float point_box_dist2(float minx, float maxx, float miny, float maxy, float minz, float maxz, f3 p) {
  const float ex = fmaxf(fmaxf(minx - p.x, p.x - maxx), 0.f);
  const float ey = fmaxf(fmaxf(miny - p.y, p.y - maxy), 0.f);
  const float ez = fmaxf(fmaxf(minz - p.z, p.z - maxz), 0.f);
  return (ex * ex + ey * ey) + ez * ez;
}

MI_HD float point_dist2(f3 p, f3 q) { const f3 d = p - q; return dot(d, d); }

// A closest point and, for a triangle, its barycentrics v, w (q = a + ab v + ac w); 0 for the other primitives.
struct ClosestPoint { f3 q; float v, w; };

// Ericson, Real-Time Collision Detection §5.1.5: the Voronoi region of p decides - a vertex (A, B, C), an edge (AB, AC, BC) or
// the face -, the regions tested in that book's order. All six projections and the three edge functions are formed first (their
// values do not depend on the region), the region picks ONE quotient - AB: d1 / (d1 - d3), AC: d2 / (d2 - d6), BC: (d4 - d3) /
// ((d4 - d3) + (d5 - d6)), face: 1 / ((va + vb) + vc) - and the barycentrics follow from it, so that the lanes of a wave share
// one division whatever regions they are in. A triangle collapsed to a point has ab = ac = 0 and falls in region A; a collapsed
// triangle that reaches the face region divides by zero and its NaN distance is never accepted. Nothing is special-cased.
MI_HD ClosestPoint closest_on_triangle(f3 a, f3 b, f3 c, f3 p) {
  const f3 ab = b - a, ac = c - a;
  const f3 ap = p - a, bp = p - b, cp = p - c;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool rA = d1 <= 0.f && d2 <= 0.f;
  const bool rB = !rA && d3 >= 0.f && d4 <= d3;
  const bool rAB = !(rA || rB) && vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
  const bool rC = !(rA || rB || rAB) && d6 >= 0.f && d5 <= d6;
  const bool rAC = !(rA || rB || rAB || rC) && vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
  const bool rBC = !(rA || rB || rAB || rC || rAC) && va <= 0.f && e43 >= 0.f && e56 >= 0.f;
  const bool vertex = rA || rB || rC;
  const float num = rAB ? d1 : rAC ? d2 : rBC ? e43 : 1.f;
  const float den = vertex ? 1.f : rAB ? d1 - d3 : rAC ? d2 - d6 : rBC ? e43 + e56 : (va + vb) + vc;
  const float r = num / den;
  ClosestPoint cpt;
  cpt.v = rA ? 0.f : rB ? 1.f : rAB ? r : (rC || rAC) ? 0.f : rBC ? 1.f - r : vb * r;
  cpt.w = (rA || rB || rAB) ? 0.f : rC ? 1.f : (rAC || rBC) ? r : vc * r;
  cpt.q = (a + ab * cpt.v) + ac * cpt.w;
  return cpt;
}

// The closest point of a sphere's SURFACE: the centre moved by the radius towards p; from the centre itself, towards +x.
MI_HD ClosestPoint closest_on_sphere(f3 c, float radius, f3 p) {
  const f3 v = p - c;
  const float len = sqrtf(dot(v, v));
  ClosestPoint cpt;
  cpt.q = len > 0.f ? c + v * (radius / len) : mk(c.x + radius, c.y, c.z);
  cpt.v = cpt.w = 0.f;
  return cpt;
}

// The closest point of a disc (centre c, normal n taken as given, squared radius r2): p projected into the disc's plane, pulled
// back to the rim when the projection lies outside it.
MI_HD ClosestPoint closest_on_disc(f3 n, f3 c, float r2, f3 p) {
  const f3 v = p - c;
  const float h = dot(v, n);
  const f3 q0 = p - n * h;
  const f3 u = q0 - c;
  const float uu = dot(u, u);
  ClosestPoint cpt;
  cpt.q = uu <= r2 ? q0 : c + u * (sqrtf(r2) / sqrtf(uu));
  cpt.v = cpt.w = 0.f;
  return cpt;
}

// The closest point of the primitive in the first 40 bytes of a leaf record (trace_kernels.hpp GLeaf): kind = LEAF_* (0 triangle,
// 1 sphere, 2 disc), f = tri: a, b, c | sphere: centre, radius | disc: n, centre, r2.
MI_HD ClosestPoint closest_on_prim(uint32_t kind, const float* f, f3 p) {
  if (kind == 0u) return closest_on_triangle(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), mk(f[6], f[7], f[8]), p);
  if (kind == 1u) return closest_on_sphere(mk(f[0], f[1], f[2]), f[3], p);
  return closest_on_disc(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), f[6], p);
}

// Whether a query is walked at all: a finite point and a radius that is neither NaN nor negative (+inf is legal).
MI_HD bool point_query_valid(f3 p, float radius) {
  return fabsf(p.x) < kInf && fabsf(p.y) < kInf && fabsf(p.z) < kInf && radius >= 0.f;
}

}  // namespace mi
