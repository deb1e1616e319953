// pose_kernels.hpp — gfx950 kernels of mi_scene_set_poses / mi_scene_set_poses_device: the posed geometry of a live scene from its
// rest copy and one 32-byte pose per geometry. The driver is poseScene in raylib.hip, which hands the arrays written here to
// refitScene; DESIGN.md §35 has the numbers.
//
//   1 pose_frame_kernel   one thread per geometry: the pose as two 16-byte loads, its validity (an invalid pose sets the flag
//                         and leaves its index in the second word), and its PoseFrame - obox_frame made once per geometry
//   2 pose_apply_kernel   one thread per vertex (the vertex and, where the scene has them, its normal), then per sphere, then per
//                         disc: the owner (uint16), the owner's frame (four 16-byte loads, wave-uniform over long runs of one
//                         body's vertices), the rest record, the posed record. Unowned records and identity poses copy the rest bytes.
//
// Lane i reads the 12 bytes at i x 12: a wave's vertex load covers 768 consecutive bytes, every byte of every line fetched is used
// (cdna_hip_programming.md, Guideline 2); the pass moves 12 + 12 bytes per vertex (and as many per normal) plus 2 for the owner.
// No LDS, no scratch, no per-lane arrays. Everything is pose_math.hpp's, which the host twin compiles too.
#pragma once

#include <hip/hip_runtime.h>

#include "pose_math.hpp"

namespace mi {

constexpr uint32_t kPoseBlock = 256;

struct PoseRest { const mi_vec3* verts; const mi_vec3* normals; const mi_sphere* spheres; const mi_disc* discs; };
struct PoseOwners { const uint16_t* verts; const uint16_t* spheres; const uint16_t* discs; };
struct PoseOut { mi_vec3* verts; mi_vec3* normals; mi_sphere* spheres; mi_disc* discs; };

// bad[0]: 1 when some pose is not valid; bad[1]: the smallest index of such a pose (preset to 0xFFFFFFFF).
__global__ __launch_bounds__(kPoseBlock) void pose_frame_kernel(const float4* __restrict__ poses, uint32_t G, PoseFrame* __restrict__ frames,
                                                                uint32_t* __restrict__ bad) {
  const uint32_t g = blockIdx.x * kPoseBlock + threadIdx.x;
  if (g >= G) return;
  const float4 a = poses[2 * (size_t)g], b = poses[2 * (size_t)g + 1];
  const float q[4] = {a.x, a.y, a.z, a.w}, t[3] = {b.x, b.y, b.z};
  if (!pose_valid(q, t, b.w)) {
    atomicOr(&bad[0], 1u);
    atomicMin(&bad[1], g);
  }
  frames[g] = pose_frame(q, t, b.w);
}

__global__ __launch_bounds__(kPoseBlock) void pose_apply_kernel(uint32_t V, uint32_t S, uint32_t D, PoseRest rest, PoseOwners owners,
                                                                const PoseFrame* __restrict__ frames, PoseOut out) {
  const uint64_t i = (uint64_t)blockIdx.x * kPoseBlock + threadIdx.x;
  if (i < V) {
    const uint16_t o = owners.verts[i];
    mi_vec3 v = rest.verts[i];
    if (rest.normals) {
      mi_vec3 n = rest.normals[i];
      if (o != kPoseUnowned) { const PoseFrame F = frames[o]; v = pose_vertex(F, v); n = pose_normal(F, n); }
      out.normals[i] = n;
    } else if (o != kPoseUnowned) {
      v = pose_vertex(frames[o], v);
    }
    out.verts[i] = v;
    return;
  }
  const uint64_t s = i - V;
  if (s < S) {
    const uint16_t o = owners.spheres[s];
    mi_sphere sp = rest.spheres[s];
    if (o != kPoseUnowned) sp = pose_sphere(frames[o], sp);
    out.spheres[s] = sp;
    return;
  }
  const uint64_t d = s - S;
  if (d < D) {
    const uint16_t o = owners.discs[d];
    mi_disc dc = rest.discs[d];
    if (o != kPoseUnowned) dc = pose_disc(frames[o], dc);
    out.discs[d] = dc;
  }
}

}  // namespace mi
