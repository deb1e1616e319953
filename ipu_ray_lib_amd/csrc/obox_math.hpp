// obox_math.hpp — the arithmetic of oriented-box queries (mi_obox_query* / mi_obox_offsets* / mi_obox_fill*, include/mi_raylib.h,
// where the contract is written): whether a caller's rotated box - centre, half extents, a quaternion that need not be unit -
// touches a node's box, a triangle, a sphere's shell or a disc. One definition, compiled by hipcc for the kernels
// (obox_kernels.hpp) and by g++ for the host twin (host/touch_host.hpp over OBoxShape): every function is a sequence of compares, selects
// and single binary32 operations in the order written (no contraction, correctly rounded divide on both sides), so the two
// return the same bits. The primitive tests are box_math.hpp's, called in the box's own frame: nothing of them is repeated here.
//
// Everything is CLOSED, and every separation is a strict compare that a NaN fails.
#pragma once

#include "box_math.hpp"

namespace mi {

// A query as the walk carries it: the centre and half extents (6 floats), the frame's rows U, V, W (9) and the world bounds (6).
struct OBox { f3 c, h, U, V, W, qmn, qmx; };

// qq = ((x x + y y) + z z) + w w and s = 2.f / qq, the scale that makes the frame orthogonal for any non-zero quaternion
MI_HD float obox_quat_scale(float x, float y, float z, float w, float* qq) {
  *qq = ((x * x + y * y) + z * z) + w * w;
  return 2.f / *qq;
}

// Whether a query is walked at all: ten finite floats, half >= 0 on every axis (0 is legal: a rectangle, a segment, a point),
// qq > 0 and a finite s.
MI_HD bool obox_query_valid(f3 c, f3 h, float x, float y, float z, float w) {
  float qq;
  const float s = obox_quat_scale(x, y, z, w, &qq);
  return fabsf(c.x) < kInf && fabsf(c.y) < kInf && fabsf(c.z) < kInf && fabsf(h.x) < kInf && fabsf(h.y) < kInf && fabsf(h.z) < kInf &&
         fabsf(x) < kInf && fabsf(y) < kInf && fabsf(z) < kInf && fabsf(w) < kInf && h.x >= 0.f && h.y >= 0.f && h.z >= 0.f && qq > 0.f &&
         fabsf(s) < kInf;
}

// The frame of the quaternion (x, y, z, w): a point p has the local coordinates (dot(U, d), dot(V, d), dot(W, d)), d = p - centre.
MI_HD void obox_frame(float x, float y, float z, float w, f3& U, f3& V, f3& W) {
  float qq;
  const float s = obox_quat_scale(x, y, z, w, &qq);
  const float xs = x * s, ys = y * s, zs = z * s;
  const float wx = w * xs, wy = w * ys, wz = w * zs;
  const float xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
  U = mk(1.f - (yy + zz), xy + wz, xz - wy);
  V = mk(xy - wz, 1.f - (xx + zz), yz + wx);
  W = mk(xz + wy, yz - wx, 1.f - (xx + yy));
}

// The query's world bounds: per world axis ext = (|U| half.x + |V| half.y) + |W| half.z, qmn = centre - ext, qmx = centre + ext.
MI_HD void obox_world_bounds(OBox& q) {
  const f3 ext = mk((fabsf(q.U.x) * q.h.x + fabsf(q.V.x) * q.h.y) + fabsf(q.W.x) * q.h.z,
                    (fabsf(q.U.y) * q.h.x + fabsf(q.V.y) * q.h.y) + fabsf(q.W.y) * q.h.z,
                    (fabsf(q.U.z) * q.h.x + fabsf(q.V.z) * q.h.y) + fabsf(q.W.z) * q.h.z);
  q.qmn = q.c - ext;
  q.qmx = q.c + ext;
}

// The whole query from its ten floats (frame and bounds of an invalid query are never read: it is not walked)
MI_HD OBox obox_make(f3 c, f3 h, float x, float y, float z, float w) {
  OBox q;
  q.c = c;
  q.h = h;
  obox_frame(x, y, z, w, q.U, q.V, q.W);
  obox_world_bounds(q);
  return q;
}

// One axis A of the frame, half extent hA, against the bounds moved to the centre (dl = mn - centre, dh = mx - centre): the
// largest and the smallest projection of the bounds on A, corner picked per component by A's sign. Separated when the smallest
// lies above hA or the largest below -hA. Bitwise |: both compares are always made, nothing to branch around.
MI_HD bool obox_slab_separates(f3 A, float hA, f3 dl, f3 dh) {
  const bool px = A.x > 0.f, py = A.y > 0.f, pz = A.z > 0.f;
  const float up = ((px ? A.x * dh.x : A.x * dl.x) + (py ? A.y * dh.y : A.y * dl.y)) + (pz ? A.z * dh.z : A.z * dl.z);
  const float dn = ((px ? A.x * dl.x : A.x * dh.x) + (py ? A.y * dl.y : A.y * dh.y)) + (pz ? A.z * dl.z : A.z * dh.z);
  return (dn > hA) | (up < -hA);
}

// The bounds [mn, mx] against the query: box_meets_bounds against the world bounds, then the three slabs of the box's own frame.
// A node's box is entered on it; unchanged, it is the first step of every primitive test, on the primitive's own bounds. Every
// operation is monotone in mn (falling) and mx (rising) as computed - fl(a - c), fl(x a) for a fixed x and fl(a + b) are - so a
// box that contains another passes whenever that one does: a primitive whose bounds pass has every ancestor's box pass
// (DESIGN.md §34).
MI_HD bool obox_meets_bounds(f3 mn, f3 mx, const OBox& q) {
  const bool meets = box_meets_bounds(mn, mx, q.qmn, q.qmx);
  const f3 dl = mn - q.c, dh = mx - q.c;
  const bool su = obox_slab_separates(q.U, q.h.x, dl, dh), sv = obox_slab_separates(q.V, q.h.y, dl, dh), sw = obox_slab_separates(q.W, q.h.z, dl, dh);
  return meets & !su & !sv & !sw;
}

// A point and a direction in the box's frame
MI_HD f3 obox_local_dir(const OBox& q, f3 d) { return mk(dot(q.U, d), dot(q.V, d), dot(q.W, d)); }
MI_HD f3 obox_local_point(const OBox& q, f3 p) { return obox_local_dir(q, p - q.c); }

// The primitive of a leaf record (kind and f as box_touches_prim takes them): obox_meets_bounds on the primitive's own bounds,
// then the box family's test in the box's frame on [-half, half] - a triangle's vertices, a sphere's centre, a disc's centre and
// normal moved there. In that test cb = 0.5 (-half) + 0.5 half is an exact zero and h is half. *contained is what that call
// reports - exact for a triangle (all three moved vertices in the box), the sphere's and disc's bounds about the moved centre -
// and means something only for a touching primitive.
MI_HD bool obox_touches_prim(uint32_t kind, const float* f, const OBox& q, bool* contained) {
  const f3 lo = -q.h, hi = q.h;
  f3 mn, mx;
  *contained = false;
  if (kind == 0u) {
    const f3 a = mk(f[0], f[1], f[2]), b = mk(f[3], f[4], f[5]), c = mk(f[6], f[7], f[8]);
    triangle_bounds(a, b, c, mn, mx);
    if (!obox_meets_bounds(mn, mx, q)) return false;
    return box_touches_triangle(obox_local_point(q, a), obox_local_point(q, b), obox_local_point(q, c), lo, hi, contained);
  }
  if (kind == 1u) {
    const f3 c = mk(f[0], f[1], f[2]);
    sphere_bounds(c, f[3], mn, mx);
    if (!obox_meets_bounds(mn, mx, q)) return false;
    return box_touches_sphere(obox_local_point(q, c), f[3], f[4], lo, hi, contained);
  }
  const f3 n = mk(f[0], f[1], f[2]), c = mk(f[3], f[4], f[5]);
  disc_bounds(n, c, f[6], mn, mx);
  if (!obox_meets_bounds(mn, mx, q)) return false;
  return box_touches_disc(obox_local_dir(q, n), obox_local_point(q, c), f[6], lo, hi, contained);
}

// The oriented boxes as a touch family (touch_kernels.hpp).
struct OBoxShape {
  using Item = mi_obox;
  using Record = mi_overlap;
  struct Fields { f3 c, h; float x, y, z, w; };      // centre, half extents, the quaternion as given
  using Carried = OBox;
  static constexpr int kAny = MI_OBOX_ANY, kCount = MI_OBOX_COUNT;
  static constexpr size_t kAlign = 16;
  static constexpr const char *kNoun = "oriented boxes", *kKindBad = "unknown oriented-box kind", *kAlignBad = "oriented boxes must be 16-byte aligned";
  static MI_HD Fields fields(const mi_obox& b) {
    return {mk(b.centre[0], b.centre[1], b.centre[2]), mk(b.half[0], b.half[1], b.half[2]), b.quat[0], b.quat[1], b.quat[2], b.quat[3]};
  }
  static MI_HD bool valid(const Fields& b) { return obox_query_valid(b.c, b.h, b.x, b.y, b.z, b.w); }
  static MI_HD Carried carry(const Fields& b) { return obox_make(b.c, b.h, b.x, b.y, b.z, b.w); }
  static MI_HD bool meets_bounds(f3 mn, f3 mx, const Carried& q) { return obox_meets_bounds(mn, mx, q); }
  static MI_HD bool touches_prim(uint32_t kind, const float* f, const Carried& q, bool* contained) { return obox_touches_prim(kind, f, q, contained); }
  static MI_HD uint32_t flags(bool contained) { return overlap_flags(contained); }
};

}  // namespace mi
