/* sanitize_point_query.c - the host twin of point queries (mi_point_query_host, include/mi_scene_host.h) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, from a stand-alone program: tools/sanitize_point_query.sh builds the host library's sources and this
 * file with -fsanitize=address,undefined into one executable and runs it. CPU only; nothing is loaded into python.
 * It queries the built-in scenes with points inside, outside and on their boxes, with every radius edge, unaligned buffers, an
 * empty scene and no points, and checks what must hold whatever the scene: WITHIN == CLOSEST found, a found distance below the
 * radius, "nothing found" records as the contract writes them. */
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

static int run_scene(const char* name, const char* mesh, size_t n) {
  mi_host_scene* hs = NULL;
  mi_scene_desc d;
  if (mi_host_scene_builtin(name, mesh, &hs) != MI_OK || mi_host_scene_fill_desc(hs, &d) != MI_OK) {
    fprintf(stderr, "%s: %s\n", name, mi_host_last_error());
    return 1;
  }
  /* buffers at odd addresses: the twin asks no alignment */
  char* rawp = malloc(n * sizeof(mi_point) + 1);
  char* rawo = malloc(n * sizeof(mi_point_hit) + 1);
  unsigned char* in = malloc(n);
  mi_point* pts = (mi_point*)(rawp + 1);
  void* out = rawo + 1;
  const float lo[3] = {d.bvh_nodes[0].min_x, d.bvh_nodes[0].min_y, d.bvh_nodes[0].min_z};
  const float radii[6] = {INFINITY, 1.0f, 0.0f, -1.0f, NAN, 100.0f};
  for (size_t i = 0; i < n; ++i) {
    mi_point p;
    p.x = lo[0] + (rnd() * 3.f - 1.f) * 600.f; p.y = lo[1] + (rnd() * 3.f - 1.f) * 600.f; p.z = lo[2] + (rnd() * 3.f - 1.f) * 600.f;
    p.radius = radii[i % 6];
    if (i % 97 == 0) p.x = NAN;
    if (i % 101 == 0) p.y = INFINITY;
    memcpy(pts + i, &p, sizeof p);
  }
  uint64_t vc[2], vw[2];
  int bad = 0;
  if (mi_point_query_host(&d, MI_POINT_CLOSEST, pts, out, n, vc) != MI_OK || mi_point_query_host(&d, MI_POINT_WITHIN, pts, in, n, vw) != MI_OK) {
    fprintf(stderr, "%s: %s\n", name, mi_host_last_error());
    return 1;
  }
  size_t found = 0;
  for (size_t i = 0; i < n; ++i) {
    mi_point_hit h; mi_point p;
    memcpy(&h, (char*)out + i * sizeof h, sizeof h);
    memcpy(&p, pts + i, sizeof p);
    const int f = h.prim_id != MI_INVALID_PRIM;
    found += (size_t)f;
    if (f != (int)in[i]) ++bad;
    if (f && !(h.dist < p.radius && h.flags == 0 && h.geom_id < d.num_geometry)) ++bad;
    if (!f && !(memcmp(&h.dist, &p.radius, 4) == 0 && h.geom_id == MI_INVALID_GEOM && h.flags == MI_FLAG_ESCAPED && h.b1 == 0.f && h.point.x == 0.f)) ++bad;
  }
  printf("%s: %zu points, %zu found, %llu box tests, %llu primitive evaluations (WITHIN: %llu, %llu), %d bad\n", name, n, found,
         (unsigned long long)vc[0], (unsigned long long)vc[1], (unsigned long long)vw[0], (unsigned long long)vw[1], bad);
  /* no points; visits not asked for */
  if (mi_point_query_host(&d, MI_POINT_CLOSEST, NULL, NULL, 0, NULL) != MI_OK) ++bad;
  if (mi_point_query_host(&d, MI_POINT_WITHIN, pts, in, n, NULL) != MI_OK) ++bad;
  /* refusals */
  if (mi_point_query_host(NULL, 0, pts, out, n, NULL) != MI_ERR_INVALID_ARG || mi_point_query_host(&d, 2, pts, out, n, NULL) != MI_ERR_INVALID_ARG ||
      mi_point_query_host(&d, 0, NULL, out, n, NULL) != MI_ERR_INVALID_ARG) ++bad;
  /* nodes cut short: not a depth-first BVH2 any more, refused before anything is read past the end */
  if (d.num_nodes > 2) {
    mi_scene_desc cut = d;
    cut.num_nodes = d.num_nodes - 1;
    if (mi_point_query_host(&cut, 0, pts, out, 1, NULL) != MI_ERR_INVALID_ARG) ++bad;
  }
  free(rawp); free(rawo); free(in);
  mi_host_scene_destroy(hs);
  return bad;
}

int main(int argc, char** argv) {
  const char* mesh = argc > 1 ? argv[1] : "assets/monkey_bust.glb";
  int bad = run_scene("spheres", mesh, 20000) + run_scene("box-simple", mesh, 20000) + run_scene("box", mesh, 20000);
  /* an empty scene */
  mi_scene_desc empty;
  memset(&empty, 0, sizeof empty);
  mi_point p = {1.f, 2.f, 3.f, INFINITY};
  mi_point_hit h;
  unsigned char in = 7;
  uint64_t v[2] = {9, 9};
  if (mi_point_query_host(&empty, MI_POINT_CLOSEST, &p, &h, 1, v) != MI_OK || h.prim_id != MI_INVALID_PRIM || !isinf(h.dist) || v[0] || v[1]) ++bad;
  if (mi_point_query_host(&empty, MI_POINT_WITHIN, &p, &in, 1, NULL) != MI_OK || in != 0) ++bad;
  printf(bad ? "FAILED: %d\n" : "sanitize_point_query OK\n", bad);
  return bad ? 1 : 0;
}
