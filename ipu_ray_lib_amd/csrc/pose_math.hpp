// pose_math.hpp — the arithmetic of rigid poses (mi_scene_set_poses*, include/mi_raylib.h, where the contract is written): whether
// a pose is valid, whether it is the identity, and what it makes of a point, a direction, a sphere and a disc. One definition,
// compiled by hipcc for the kernels (pose_kernels.hpp) and by g++ for the host twin (host/pose_host.cpp): every function is a
// sequence of compares and single binary32 operations in the order written (no contraction, correctly rounded divide on both sides),
// so the two return the same bits. The frame is obox_math.hpp's obox_frame, unchanged: a body and its mi_obox turn alike.
// The second half is host code only: which geometry owns which vertex, sphere and disc (pose_owners), shared by the driver
// (raylib.hip) and the twin.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "obox_math.hpp"
#include "../../include/mi_raylib.h"

namespace mi {

// A pose as the pass reads it: the frame's columns U, V, W (a point p turns into U p.x + V p.y + W p.z), the translation, the
// scale, and whether the pose is the identity (then the rest bytes are copied, not computed). 64 bytes: four 16-byte loads.
struct alignas(16) PoseFrame {
  float U[3], V[3], W[3], t[3];
  float scale;
  uint32_t identity;
  uint32_t pad[2];
};
static_assert(sizeof(PoseFrame) == 64, "a pose's frame is four 16-byte loads");

// Eight finite floats, qq > 0, a finite 2 / qq (obox_query_valid's rule for the quaternion) and scale > 0.
MI_HD bool pose_valid(const float q[4], const float t[3], float scale) {
  float qq;
  const float s = obox_quat_scale(q[0], q[1], q[2], q[3], &qq);
  return fabsf(q[0]) < kInf && fabsf(q[1]) < kInf && fabsf(q[2]) < kInf && fabsf(q[3]) < kInf && fabsf(t[0]) < kInf && fabsf(t[1]) < kInf &&
         fabsf(t[2]) < kInf && fabsf(scale) < kInf && qq > 0.f && fabsf(s) < kInf && scale > 0.f;
}

// Float compares: -0 counts as zero.
MI_HD bool pose_is_identity(const float q[4], const float t[3], float scale) {
  return q[0] == 0.f && q[1] == 0.f && q[2] == 0.f && q[3] == 1.f && t[0] == 0.f && t[1] == 0.f && t[2] == 0.f && scale == 1.f;
}

MI_HD PoseFrame pose_frame(const float q[4], const float t[3], float scale) {
  PoseFrame F;
  f3 U, V, W;
  obox_frame(q[0], q[1], q[2], q[3], U, V, W);
  F.U[0] = U.x; F.U[1] = U.y; F.U[2] = U.z;
  F.V[0] = V.x; F.V[1] = V.y; F.V[2] = V.z;
  F.W[0] = W.x; F.W[1] = W.y; F.W[2] = W.z;
  F.t[0] = t[0]; F.t[1] = t[1]; F.t[2] = t[2];
  F.scale = scale;
  F.identity = pose_is_identity(q, t, scale) ? 1u : 0u;
  F.pad[0] = F.pad[1] = 0u;
  return F;
}

// A direction: r_k = (U_k p.x + V_k p.y) + W_k p.z - no scale, no translation, not renormalised.
MI_HD f3 pose_dir(const PoseFrame& F, f3 p) {
  return mk((F.U[0] * p.x + F.V[0] * p.y) + F.W[0] * p.z, (F.U[1] * p.x + F.V[1] * p.y) + F.W[1] * p.z, (F.U[2] * p.x + F.V[2] * p.y) + F.W[2] * p.z);
}

// A point: p'_k = scale r_k + t_k.
MI_HD f3 pose_point(const PoseFrame& F, f3 p) {
  const f3 r = pose_dir(F, p);
  return mk(F.scale * r.x + F.t[0], F.scale * r.y + F.t[1], F.scale * r.z + F.t[2]);
}

MI_HD mi_vec3 pose_vertex(const PoseFrame& F, mi_vec3 v) {
  if (F.identity) return v;
  const f3 p = pose_point(F, mk(v.x, v.y, v.z));
  mi_vec3 r; r.x = p.x; r.y = p.y; r.z = p.z;
  return r;
}

MI_HD mi_vec3 pose_normal(const PoseFrame& F, mi_vec3 v) {
  if (F.identity) return v;
  const f3 p = pose_dir(F, mk(v.x, v.y, v.z));
  mi_vec3 r; r.x = p.x; r.y = p.y; r.z = p.z;
  return r;
}

// A sphere: the centre is a point, radius' = scale radius.
MI_HD mi_sphere pose_sphere(const PoseFrame& F, mi_sphere s) {
  if (F.identity) return s;
  const f3 c = pose_point(F, mk(s.x, s.y, s.z));
  mi_sphere r; r.x = c.x; r.y = c.y; r.z = c.z; r.radius = F.scale * s.radius;
  return r;
}

// A disc: the centre is a point, the normal a direction, r' = scale r.
MI_HD mi_disc pose_disc(const PoseFrame& F, mi_disc d) {
  if (F.identity) return d;
  const f3 n = pose_dir(F, mk(d.nx, d.ny, d.nz)), c = pose_point(F, mk(d.cx, d.cy, d.cz));
  mi_disc r; r.nx = n.x; r.ny = n.y; r.nz = n.z; r.r = F.scale * d.r; r.cx = c.x; r.cy = c.y; r.cz = c.z;
  return r;
}

// ---- host only: ownership -------------------------------------------------------------------------------------------------------
constexpr uint16_t kPoseUnowned = 0xFFFFu;      // (at most 65 535 geometries: ids 0 .. 0xFFFE)

// The owner of every vertex, sphere and disc: the geometry whose mesh's range [first_vertex, first_vertex + num_vertices) holds
// the vertex, the geometry that references the sphere or disc; kPoseUnowned where there is none. Returns the empty string, or what
// is refused: one mesh, sphere or disc referenced by two geometry entries, two referenced meshes whose vertex ranges intersect -
// the message names the pair. References out of range are not followed (mi_scene_create has refused them).
inline std::string pose_owners(const mi_geom_ref* geometry, uint32_t G, const mi_mesh_info* meshInfo, uint32_t M, uint32_t numVerts,
                               uint32_t numSpheres, uint32_t numDiscs, std::vector<uint16_t>& vertOwner, std::vector<uint16_t>& sphereOwner,
                               std::vector<uint16_t>& discOwner) {
  vertOwner.assign(numVerts, kPoseUnowned);
  sphereOwner.assign(numSpheres, kPoseUnowned);
  discOwner.assign(numDiscs, kPoseUnowned);
  std::vector<uint16_t> meshOwner(M, kPoseUnowned);
  static const char* const kKind[3] = {"mesh", "sphere", "disc"};
  for (uint32_t g = 0; g < G && g < kPoseUnowned; ++g) {
    const mi_geom_ref& r = geometry[g];
    if (r.type > 2) continue;
    std::vector<uint16_t>& owner = r.type == 0 ? meshOwner : (r.type == 1 ? sphereOwner : discOwner);
    if (r.index >= owner.size()) continue;
    if (owner[r.index] != kPoseUnowned)
      return "geometries " + std::to_string(owner[r.index]) + " and " + std::to_string(g) + " both reference " + kKind[r.type] + " " + std::to_string(r.index);
    owner[r.index] = (uint16_t)g;
    if (r.type != 0) continue;
    const mi_mesh_info& m = meshInfo[r.index];
    const uint64_t end = std::min<uint64_t>((uint64_t)m.first_vertex + m.num_vertices, numVerts);
    for (uint64_t v = m.first_vertex; v < end; ++v) {
      if (vertOwner[v] != kPoseUnowned)
        return "the vertex ranges of geometries " + std::to_string(vertOwner[v]) + " and " + std::to_string(g) + " intersect (vertex " + std::to_string(v) + ")";
      vertOwner[v] = (uint16_t)g;
    }
  }
  return std::string();
}

}  // namespace mi
