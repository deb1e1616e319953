/* sanitize_pose.c - the host twin of rigid poses (mi_pose_geometry_host, include/mi_scene_host.h) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, from a stand-alone program: tools/sanitize_pose.sh builds the host library's sources and this file
 * with -fsanitize=address,undefined into one executable and runs it. CPU only; nothing is loaded into python.
 * It poses the built-in scenes - random orientations with quaternions that are not unit, scales from 1/8 to 8, the identity - into
 * buffers of exactly the scene's counts, checks what must hold whatever the scene (an identity pose keeps every
 * byte, posing twice from rest gives the same bytes), and runs every refusal: each kind of invalid pose, a wrong count, a null
 * buffer, a mesh range moved onto its neighbour's, a geometry referenced twice, an empty description with wild pointers. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_scene_host.h"

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static float rnd(void) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((g_state >> 40) & 0xFFFFFF) / 16777216.0f;
}

static const mi_pose kIdentity = {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 1.f};

static int expect_refused(int rc, const char* what) {
  if (rc == MI_ERR_INVALID_ARG && strstr(mi_host_last_error(), "mi_pose_geometry_host")) return 0;
  fprintf(stderr, "not refused: %s (rc %d, \"%s\")\n", what, rc, mi_host_last_error());
  return 1;
}

static int run_scene(const char* name, const char* mesh) {
  mi_host_scene* hs = NULL;
  mi_scene_desc d;
  if (mi_host_scene_builtin(name, mesh, &hs) != MI_OK || mi_host_scene_fill_desc(hs, &d) != MI_OK) {
    fprintf(stderr, "%s: %s\n", name, mi_host_last_error());
    return 1;
  }
  const uint32_t G = d.num_geometry, V = d.num_meshes ? d.num_verts : 0;
  /* buffers of exactly the scene's counts: a record written or read behind one of them is a report */
  char* rawp = malloc((size_t)G * sizeof(mi_pose));
  char* rawv[2] = {malloc((size_t)V * sizeof(mi_vec3)), malloc((size_t)V * sizeof(mi_vec3))};
  char* rawn = malloc((size_t)d.num_normals * sizeof(mi_vec3));
  char* raws = malloc((size_t)d.num_spheres * sizeof(mi_sphere));
  char* rawd = malloc((size_t)d.num_discs * sizeof(mi_disc));
  mi_pose* poses = (mi_pose*)rawp;
  mi_vec3* verts[2] = {(mi_vec3*)rawv[0], (mi_vec3*)rawv[1]};
  mi_vec3* normals = (mi_vec3*)rawn;
  mi_sphere* spheres = (mi_sphere*)raws;
  mi_disc* discs = (mi_disc*)rawd;
  int bad = 0;
  for (uint32_t g = 0; g < G; ++g) {
    mi_pose p;
    const float norm = (g % 5 == 0) ? 1000.f : (g % 7 == 0 ? 1e-3f : 1.f);      /* the quaternion need not be unit */
    for (int k = 0; k < 4; ++k) p.quat[k] = (rnd() * 2.f - 1.f) * norm;
    for (int k = 0; k < 3; ++k) p.translation[k] = (rnd() * 2.f - 1.f) * 100.f;
    p.scale = ldexpf(1.f + rnd(), (int)(g % 6) - 3);
    if (g % 4 == 3) p = kIdentity;
    memcpy(rawp + (size_t)g * sizeof p, &p, sizeof p);
  }
  /* twice from rest: the same bytes */
  for (int k = 0; k < 2; ++k)
    if (mi_pose_geometry_host(&d, poses, G, verts[k], normals, spheres, discs) != MI_OK) {
      fprintf(stderr, "%s: %s\n", name, mi_host_last_error());
      bad = 1;
    }
  if (!bad && V && memcmp(verts[0], verts[1], (size_t)V * sizeof(mi_vec3)) != 0) { fprintf(stderr, "%s: posing twice from rest differs\n", name); bad = 1; }
  /* identities: every byte kept */
  for (uint32_t g = 0; g < G; ++g) memcpy(rawp + (size_t)g * sizeof(mi_pose), &kIdentity, sizeof kIdentity);
  if (mi_pose_geometry_host(&d, poses, G, verts[0], normals, spheres, discs) != MI_OK) { fprintf(stderr, "%s: %s\n", name, mi_host_last_error()); bad = 1; }
  if (!bad && ((V && memcmp(verts[0], d.mesh_verts, (size_t)V * sizeof(mi_vec3))) ||
               (d.num_normals && memcmp(normals, d.mesh_normals, (size_t)d.num_normals * sizeof(mi_vec3))) ||
               (d.num_spheres && memcmp(spheres, d.spheres, (size_t)d.num_spheres * sizeof(mi_sphere))) ||
               (d.num_discs && memcmp(discs, d.discs, (size_t)d.num_discs * sizeof(mi_disc))))) {
    fprintf(stderr, "%s: the identity changed a byte\n", name);
    bad = 1;
  }
  /* every kind of invalid pose, on the last geometry */
  if (G) {
    const float nan_ = NAN, inf_ = INFINITY;
    const mi_pose invalid[8] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 1.f},   {{nan_, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 1.f},
                                {{inf_, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 1.f},  {{0.f, 0.f, 0.f, 1.f}, {0.f, nan_, 0.f}, 1.f},
                                {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, 0.f},   {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, -2.f},
                                {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, inf_},  {{1e-20f, 0.f, 0.f, 1e-20f}, {0.f, 0.f, 0.f}, 1.f}};
    for (int k = 0; k < 8; ++k) {
      memcpy(rawp + (size_t)(G - 1) * sizeof(mi_pose), &invalid[k], sizeof(mi_pose));
      bad |= expect_refused(mi_pose_geometry_host(&d, poses, G, verts[0], normals, spheres, discs), "an invalid pose");
    }
    memcpy(rawp + (size_t)(G - 1) * sizeof(mi_pose), &kIdentity, sizeof kIdentity);
    bad |= expect_refused(mi_pose_geometry_host(&d, poses, G - 1, verts[0], normals, spheres, discs), "a wrong count");
    bad |= expect_refused(mi_pose_geometry_host(&d, NULL, G, verts[0], normals, spheres, discs), "null poses");
    if (V) bad |= expect_refused(mi_pose_geometry_host(&d, poses, G, NULL, normals, spheres, discs), "a null buffer");
    /* a geometry referenced twice */
    if (G > 1) {
      mi_geom_ref* geometry = malloc((size_t)G * sizeof(mi_geom_ref));
      memcpy(geometry, d.geometry, (size_t)G * sizeof(mi_geom_ref));
      geometry[G - 1] = geometry[0];
      mi_scene_desc e = d;
      e.geometry = geometry;
      bad |= expect_refused(mi_pose_geometry_host(&e, poses, G, verts[0], normals, spheres, discs), "a geometry referenced twice");
      free(geometry);
    }
    /* a mesh's range moved onto its neighbour's */
    if (d.num_meshes > 1 && d.mesh_info[1].first_vertex > 0) {
      mi_mesh_info* info = malloc((size_t)d.num_meshes * sizeof(mi_mesh_info));
      memcpy(info, d.mesh_info, (size_t)d.num_meshes * sizeof(mi_mesh_info));
      info[1].first_vertex -= 1;
      mi_scene_desc e = d;
      e.mesh_info = info;
      bad |= expect_refused(mi_pose_geometry_host(&e, poses, G, verts[0], normals, spheres, discs), "intersecting vertex ranges");
      free(info);
    }
  }
  printf("%-8s %u geometries, %u vertices, %u normals, %u spheres, %u discs: %s\n", name, G, V, d.num_normals, d.num_spheres, d.num_discs, bad ? "FAILED" : "ok");
  free(rawp); free(rawv[0]); free(rawv[1]); free(rawn); free(raws); free(rawd);
  mi_host_scene_destroy(hs);
  return bad;
}

int main(int argc, char** argv) {
  const char* mesh = argc > 1 ? argv[1] : "assets/monkey_bust.glb";
  int bad = 0;
  bad |= run_scene("box", mesh);
  bad |= run_scene("spheres", mesh);
  bad |= run_scene("monkey", mesh);
  /* an empty description: zero geometries read no pointer */
  mi_scene_desc none;
  memset(&none, 0, sizeof none);
  if (mi_pose_geometry_host(&none, (const mi_pose*)(uintptr_t)0xDEAD0000u, 0, NULL, NULL, NULL, NULL) != MI_OK) { fprintf(stderr, "the empty scene: %s\n", mi_host_last_error()); bad = 1; }
  bad |= expect_refused(mi_pose_geometry_host(NULL, NULL, 0, NULL, NULL, NULL, NULL), "a null description");
  printf(bad ? "sanitize_pose: FAILED\n" : "sanitize_pose: clean\n");
  return bad;
}
