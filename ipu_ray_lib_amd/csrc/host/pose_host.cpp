// pose_host.cpp — mi_pose_geometry_host (include/mi_scene_host.h): the host twin of the pose pass of mi_scene_set_poses*
// (pose_kernels.hpp). The owners are derived by the function the driver calls (pose_owners) and every record is moved by the MI_HD
// code of pose_math.hpp that the kernels run - compares and single rounded binary32 operations - so the arrays equal the device's
// byte for byte. The refusals are the entry's: an invalid pose, an ownership conflict.
#include <stdexcept>

#include "scene_types.hpp"
#include "../pose_math.hpp"

namespace mi::host {

void poseGeometryHost(const mi_scene_desc& d, const mi_pose* poses, uint32_t numGeometry, mi_vec3* vertsOut, mi_vec3* normalsOut, mi_sphere* spheresOut,
                      mi_disc* discsOut) {
  const char* fn = "mi_pose_geometry_host";
  auto bad = [&](const std::string& why) { throw std::invalid_argument(std::string(fn) + ": " + why); };
  if (numGeometry != d.num_geometry) bad("num_geometry differs from the scene's geometry count");
  const uint32_t V = d.num_meshes ? d.num_verts : 0;      // (as mi_scene_create keeps them)
  if (d.num_normals && d.num_normals != V) bad("normals must be absent or one per vertex");
  if ((V && !vertsOut) || (d.num_normals && !normalsOut) || (d.num_spheres && !spheresOut) || (d.num_discs && !discsOut)) bad("null buffer");
  if ((d.num_geometry && !d.geometry) || (d.num_meshes && !d.mesh_info) || (V && !d.mesh_verts) || (d.num_normals && !d.mesh_normals) ||
      (d.num_spheres && !d.spheres) || (d.num_discs && !d.discs))
    bad("a count without its array");
  for (uint32_t g = 0; g < d.num_geometry; ++g) {
    const mi_geom_ref& r = d.geometry[g];
    const uint32_t limit = r.type == 0 ? d.num_meshes : (r.type == 1 ? d.num_spheres : d.num_discs);
    if (r.type > 2 || r.index >= limit) bad("geometry " + std::to_string(g) + " references nothing of the scene");
    if (r.type == 0 && (uint64_t)d.mesh_info[r.index].first_vertex + d.mesh_info[r.index].num_vertices > V) bad("a mesh's vertex range is out of bounds");
  }
  std::vector<PoseFrame> frames(numGeometry);
  for (uint32_t g = 0; g < numGeometry; ++g) {
    mi_pose p;
    memcpy(&p, &poses[g], sizeof p);
    if (!pose_valid(p.quat, p.translation, p.scale))
      bad("pose " + std::to_string(g) + " is not valid (eight finite floats, a quaternion whose squared norm and its reciprocal are finite and positive, scale > 0)");
    frames[g] = pose_frame(p.quat, p.translation, p.scale);
  }
  std::vector<uint16_t> vo, so, dso;
  const std::string conflict = pose_owners(d.geometry, d.num_geometry, d.mesh_info, d.num_meshes, V, d.num_spheres, d.num_discs, vo, so, dso);
  if (!conflict.empty()) bad(conflict);
  for (uint32_t i = 0; i < V; ++i) {
    vertsOut[i] = vo[i] == kPoseUnowned ? d.mesh_verts[i] : pose_vertex(frames[vo[i]], d.mesh_verts[i]);
    if (d.num_normals) normalsOut[i] = vo[i] == kPoseUnowned ? d.mesh_normals[i] : pose_normal(frames[vo[i]], d.mesh_normals[i]);
  }
  for (uint32_t i = 0; i < d.num_spheres; ++i) spheresOut[i] = so[i] == kPoseUnowned ? d.spheres[i] : pose_sphere(frames[so[i]], d.spheres[i]);
  for (uint32_t i = 0; i < d.num_discs; ++i) discsOut[i] = dso[i] == kPoseUnowned ? d.discs[i] : pose_disc(frames[dso[i]], d.discs[i]);
}

}  // namespace mi::host
