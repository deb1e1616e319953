// box_math.hpp — the arithmetic of box queries (mi_box_query* / mi_box_offsets* / mi_box_fill*, include/mi_raylib.h, where the
// contract is written): whether a caller's axis-aligned box [lo, hi] touches a node's box, a triangle, a sphere's shell or a
// disc. One definition, compiled by hipcc for the kernels (box_kernels.hpp) and by g++ for the host twin
// (host/touch_host.hpp over BoxShape): every function is a sequence of compares, selects and single binary32 operations in the order
// written (no contraction, correctly rounded sqrt and divide on both sides), so the two return the same bits. A dot product is
// (x x' + y y') + z z' (ray_math.h dot). Minima and maxima are compare / select pairs, never fminf / fmaxf: what a NaN does
// is then written here and not left to a library.
//
// Everything is CLOSED: contact counts. Every separation is a strict compare that a NaN fails, so a NaN never separates and a
// box so large that its arithmetic overflows errs towards listing.
#pragma once

#include "point_math.hpp"
#include "../../include/mi_raylib.h"

namespace mi {

// Whether a box query is walked at all: six finite coordinates and lo <= hi on every axis (lo == hi is legal: a plane, a line,
// a point).
MI_HD bool box_query_valid(f3 lo, f3 hi) {
  return fabsf(lo.x) < kInf && fabsf(lo.y) < kInf && fabsf(lo.z) < kInf && fabsf(hi.x) < kInf && fabsf(hi.y) < kInf && fabsf(hi.z) < kInf &&
         lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
}

// The bounds [mn, mx] against the box: closed compares, no arithmetic. A node's box is entered on it; a primitive's own bounds
// precede its test.
MI_HD bool box_meets_bounds(f3 mn, f3 mx, f3 lo, f3 hi) {
  return mn.x <= hi.x && mx.x >= lo.x && mn.y <= hi.y && mx.y >= lo.y && mn.z <= hi.z && mx.z >= lo.z;
}
// The bounds lie inside the box, faces included (MI_OVERLAP_CONTAINED).
MI_HD bool box_holds_bounds(f3 mn, f3 mx, f3 lo, f3 hi) {
  return mn.x >= lo.x && mx.x <= hi.x && mn.y >= lo.y && mx.y <= hi.y && mn.z >= lo.z && mx.z <= hi.z;
}

MI_HD float sel_min(float a, float b) { return a < b ? a : b; }
MI_HD float sel_max(float a, float b) { return a > b ? a : b; }
MI_HD bool point_in_box(f3 p, f3 lo, f3 hi) { return p.x >= lo.x && p.x <= hi.x && p.y >= lo.y && p.y <= hi.y && p.z >= lo.z && p.z <= hi.z; }

// "min > r || max < -r" of three projections, as two conjunctions: a NaN among p0, p1, p2, r separates nothing.
MI_HD bool sat_separates(float p0, float p1, float p2, float r) {
  const float nr = -r;
  return (p0 > r && p1 > r && p2 > r) || (p0 < nr && p1 < nr && p2 < nr);
}

// The three axes e x X, e x Y, e x Z of one edge e against the moved vertices v0, v1, v2 and the half extents h
// (Akenine-Moller, Fast 3D Triangle-Box Overlap Testing): the projection of v on
//   X x e = (0, -e.z, e.y): e.y v.z - e.z v.y, radius h.y |e.z| + h.z |e.y|
//   Y x e = (e.z, 0, -e.x): e.z v.x - e.x v.z, radius h.x |e.z| + h.z |e.x|
//   Z x e = (-e.y, e.x, 0): e.x v.y - e.y v.x, radius h.x |e.y| + h.y |e.x|
// All three vertices are projected (two projections agree up to rounding; none is assumed to).
MI_HD bool sat_edge_separates(f3 e, f3 v0, f3 v1, f3 v2, f3 h) {
  const f3 a = abs3(e);
  if (sat_separates(e.y * v0.z - e.z * v0.y, e.y * v1.z - e.z * v1.y, e.y * v2.z - e.z * v2.y, h.y * a.z + h.z * a.y)) return true;
  if (sat_separates(e.z * v0.x - e.x * v0.z, e.z * v1.x - e.x * v1.z, e.z * v2.x - e.x * v2.z, h.x * a.z + h.z * a.x)) return true;
  return sat_separates(e.x * v0.y - e.y * v0.x, e.x * v1.y - e.y * v1.x, e.x * v2.y - e.y * v2.x, h.x * a.y + h.y * a.x);
}

// The bounds of the three kinds of primitive (triangle_bounds, sphere_bounds, disc_bounds below, each before the test that defines
// it): the triangle queries (contact_math.hpp) test a primitive's bounds by the same functions.
//
// Triangle (a, b, c). Its bounds are the per-axis minimum and maximum of the vertices (compares only): the box's three axes
// and CONTAINED are decided by them, exactly. Then: a vertex in the box accepts at once (compares only); otherwise the
// separating-axis test in centre / half-extent form - cb = 0.5 lo + 0.5 hi, h = 0.5 hi - 0.5 lo, v0 = a - cb, v1 = b - cb,
// v2 = c - cb, e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2 -, the nine edge axes edge by edge (e0, e1, e2), then the plane:
// n = cross(e0, e1), s = n.v0, r = (h.x |n.x| + h.y |n.y|) + h.z |n.z|, separated when s > r || s < -r. A collapsed
// triangle has zero axes, which separate nothing: what its bounds and the remaining axes say stands.
MI_HD void triangle_bounds(f3 a, f3 b, f3 c, f3& mn, f3& mx) {
  mn = mk(sel_min(sel_min(a.x, b.x), c.x), sel_min(sel_min(a.y, b.y), c.y), sel_min(sel_min(a.z, b.z), c.z));
  mx = mk(sel_max(sel_max(a.x, b.x), c.x), sel_max(sel_max(a.y, b.y), c.y), sel_max(sel_max(a.z, b.z), c.z));
}
MI_HD bool box_touches_triangle(f3 a, f3 b, f3 c, f3 lo, f3 hi, bool* contained) {
  f3 mn, mx;
  triangle_bounds(a, b, c, mn, mx);
  *contained = box_holds_bounds(mn, mx, lo, hi);
  if (!box_meets_bounds(mn, mx, lo, hi)) return false;
  if (point_in_box(a, lo, hi) || point_in_box(b, lo, hi) || point_in_box(c, lo, hi)) return true;
  const f3 cb = lo * 0.5f + hi * 0.5f, h = hi * 0.5f - lo * 0.5f;
  const f3 v0 = a - cb, v1 = b - cb, v2 = c - cb;
  const f3 e0 = v1 - v0, e1 = v2 - v1;
  if (sat_edge_separates(e0, v0, v1, v2, h)) return false;
  if (sat_edge_separates(e1, v0, v1, v2, h)) return false;
  if (sat_edge_separates(v0 - v2, v0, v1, v2, h)) return false;
  const f3 n = cross(e0, e1);
  const f3 an = abs3(n);
  const float s = dot(n, v0), r = (h.x * an.x + h.y * an.y) + h.z * an.z;
  return !(s > r || s < -r);
}

// Sphere (centre c, radius, r2 = the squared radius as the leaf record holds it): queries see SURFACES, so the box touches
// the sphere when it reaches the shell from outside and from inside - dmin2 <= r2 && dmax2 >= r2, dmin2 = point_box_dist2 of
// the centre, dmax2 = the squared distance of the farthest corner: per axis f = max(|c - lo|, |hi - c|), (fx fx + fy fy) +
// fz fz. Written as !(dmin2 > r2) && !(dmax2 < r2). The bounds are c - radius and c + radius, one rounded operation each.
MI_HD void sphere_bounds(f3 c, float radius, f3& mn, f3& mx) {
  mn = mk(c.x - radius, c.y - radius, c.z - radius);
  mx = mk(c.x + radius, c.y + radius, c.z + radius);
}
MI_HD bool box_touches_sphere(f3 c, float radius, float r2, f3 lo, f3 hi, bool* contained) {
  f3 mn, mx;
  sphere_bounds(c, radius, mn, mx);
  *contained = box_holds_bounds(mn, mx, lo, hi);
  if (!box_meets_bounds(mn, mx, lo, hi)) return false;
  const float dmin2 = point_box_dist2(lo.x, hi.x, lo.y, hi.y, lo.z, hi.z, c);
  const float fx = sel_max(fabsf(c.x - lo.x), fabsf(hi.x - c.x));
  const float fy = sel_max(fabsf(c.y - lo.y), fabsf(hi.y - c.y));
  const float fz = sel_max(fabsf(c.z - lo.z), fabsf(hi.z - c.z));
  const float dmax2 = (fx * fx + fy * fy) + fz * fz;
  return !(dmin2 > r2) && !(dmax2 < r2);
}

// Disc (normal n taken as given, centre c, r2 = the squared radius as the leaf record holds it). CONSERVATIVE: three
// necessary conditions, all of which must hold -
//   the box meets the disc's tight bounds: r = sqrtf(r2), nn = n.n, per axis t = 1 - n_i n_i / nn, clamped (t > 0 ? t : 0, which
//     also takes a NaN to 0), half extent r sqrtf(t), bounds c -+ it; these bounds also decide CONTAINED;
//   the box meets the disc's plane: cb = 0.5 lo + 0.5 hi, h = 0.5 hi - 0.5 lo, s = n.(cb - c), rr = (h.x |n.x| + h.y |n.y|) + h.z |n.z|,
//     !(|s| > rr);
//   the box meets the ball of the disc's radius about its centre: !(point_box_dist2 of c > r2).
// No touching disc is missed (up to the rounding of the operations above). A box that passes the disc's rim within its own
// size may list it although it does not touch: the three conditions can hold together where the plane's part inside the box
// lies just outside the rim.
MI_HD void disc_bounds(f3 n, f3 c, float r2, f3& mn, f3& mx) {
  const float r = sqrtf(r2), nn = dot(n, n);
  const float tx = 1.f - n.x * n.x / nn, ty = 1.f - n.y * n.y / nn, tz = 1.f - n.z * n.z / nn;
  const f3 ext = mk(r * sqrtf(tx > 0.f ? tx : 0.f), r * sqrtf(ty > 0.f ? ty : 0.f), r * sqrtf(tz > 0.f ? tz : 0.f));
  mn = c - ext;
  mx = c + ext;
}
MI_HD bool box_touches_disc(f3 n, f3 c, float r2, f3 lo, f3 hi, bool* contained) {
  f3 mn, mx;
  disc_bounds(n, c, r2, mn, mx);
  *contained = box_holds_bounds(mn, mx, lo, hi);
  if (!box_meets_bounds(mn, mx, lo, hi)) return false;
  const f3 cb = lo * 0.5f + hi * 0.5f, h = hi * 0.5f - lo * 0.5f;
  const f3 an = abs3(n);
  const float s = dot(n, cb - c), rr = (h.x * an.x + h.y * an.y) + h.z * an.z;
  if (fabsf(s) > rr) return false;
  return !(point_box_dist2(lo.x, hi.x, lo.y, hi.y, lo.z, hi.z, c) > r2);
}

// The primitive in the first 40 bytes of a leaf record (trace_kernels.hpp GLeaf): kind = LEAF_* (0 triangle, 1 sphere, 2 disc),
// f = tri: a, b, c | sphere: centre, radius, radius2 | disc: n, centre, r2. *contained is written whatever is returned and
// means something only for a touching primitive.
MI_HD bool box_touches_prim(uint32_t kind, const float* f, f3 lo, f3 hi, bool* contained) {
  if (kind == 0u) return box_touches_triangle(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), mk(f[6], f[7], f[8]), lo, hi, contained);
  if (kind == 1u) return box_touches_sphere(mk(f[0], f[1], f[2]), f[3], f[4], lo, hi, contained);
  return box_touches_disc(mk(f[0], f[1], f[2]), mk(f[3], f[4], f[5]), f[6], lo, hi, contained);
}

// The sort key of an overlap record: geomID, then primID. Unique within a box.
MI_HD uint64_t overlap_key(uint32_t geomID, uint32_t primID) { return ((uint64_t)geomID << 32) | primID; }

// What a record of a touching primitive carries when its family reports containment.
MI_HD uint32_t overlap_flags(bool contained) { return contained ? (uint32_t)MI_OVERLAP_CONTAINED : 0u; }

// The boxes as a touch family (the shape every family supplies is described in touch_kernels.hpp).
struct BoxShape {
  using Item = mi_box;
  using Record = mi_overlap;
  struct Fields { f3 lo, hi; };
  using Carried = Fields;
  static constexpr int kAny = MI_BOX_ANY, kCount = MI_BOX_COUNT;
  static constexpr size_t kAlign = 16;
  static constexpr const char *kNoun = "boxes", *kKindBad = "unknown box kind", *kAlignBad = "boxes must be 16-byte aligned";
  static MI_HD Fields fields(const mi_box& b) { return {mk(b.lo[0], b.lo[1], b.lo[2]), mk(b.hi[0], b.hi[1], b.hi[2])}; }
  static MI_HD bool valid(const Fields& b) { return box_query_valid(b.lo, b.hi); }
  static MI_HD const Carried& carry(const Fields& b) { return b; }
  static MI_HD bool meets_bounds(f3 mn, f3 mx, const Carried& q) { return box_meets_bounds(mn, mx, q.lo, q.hi); }
  static MI_HD bool touches_prim(uint32_t kind, const float* f, const Carried& q, bool* contained) { return box_touches_prim(kind, f, q.lo, q.hi, contained); }
  static MI_HD uint32_t flags(bool contained) { return overlap_flags(contained); }
};

}  // namespace mi
