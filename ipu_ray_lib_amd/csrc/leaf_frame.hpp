// leaf_frame.hpp — the per-leaf tangent frame of a diffuse bounce (scene option "leaf_frame").
//
// sample_diffuse builds an orthonormal system (xb, yb) about the hit's normal before it draws the new direction: a compare, a sum,
// a correctly rounded sqrt and division, five products and a cross product (diffuse_frame, ray_math.h). In a scene WITHOUT vertex
// normals the normal of a triangle hit is the leaf's face normal (GLeaf::n) and a disc's its plane normal, both constants of the
// primitive - so the frame is one too, and K1w's SHADE turn loads it (two 16-byte loads off the hit's leaf index, issued with the
// leaf record's own) instead of computing it. Only a sphere's frame depends on the hit point: sphere leaves and interior nodes
// carry zeros, and a sphere lane computes the frame as before. The record is written wherever GLeaf::n is: at upload on the host
// (fill_leaf_frames, also run by the host library's mi_leaf_frames so that the records can be checked without a GPU) and by the
// device kernels that rewrite leaves[] (refit, rebuild, new geometry), always as diffuse_frame of the normal just stored - the same
// binary32 operations the kernel would run per hit, so every path stays bit-identical.
#pragma once

#include "ray_math.h"

#include <cstdint>

namespace mi {

// 32 bytes per NODE, indexed like leaves[]: {xb.x, xb.y, xb.z, 0, yb.x, yb.y, yb.z, 0}
struct __attribute__((aligned(16))) GLeafFrame { float xb[3]; float pad0; float yb[3]; float pad1; };
static_assert(sizeof(GLeafFrame) == 32, "GLeafFrame must stay 32 bytes");

MI_HD GLeafFrame leaf_frame_zero() { GLeafFrame r; r.xb[0] = r.xb[1] = r.xb[2] = r.pad0 = r.yb[0] = r.yb[1] = r.yb[2] = r.pad1 = 0.f; return r; }
MI_HD GLeafFrame leaf_frame_of(f3 n) {
  f3 xb, yb;
  diffuse_frame(n, xb, yb);
  GLeafFrame r;
  r.xb[0] = xb.x; r.xb[1] = xb.y; r.xb[2] = xb.z; r.pad0 = 0.f;
  r.yb[0] = yb.x; r.yb[1] = yb.y; r.yb[2] = yb.z; r.pad1 = 0.f;
  return r;
}

// out[k] = the record of node at[k] (at = null: node k): the frame of normal[3 * node ..] where framed[node] (a triangle or disc leaf),
// zeros elsewhere.
inline void fill_leaf_frames(const uint8_t* framed, const float* normal, const uint32_t* at, uint32_t count, GLeafFrame* out) {
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t i = at ? at[k] : k;
    out[k] = framed[i] ? leaf_frame_of(mk(normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2])) : leaf_frame_zero();
  }
}

}  // namespace mi
