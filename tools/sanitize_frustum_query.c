/* sanitize_frustum_query.c - the host twins of frustum queries (mi_frustum_query_host, mi_frustum_offsets_host, mi_frustum_fill_host,
 * include/mi_scene_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program:
 * tools/sanitize_frustum_query.sh builds the host library's sources and this file with -fsanitize=address,undefined into one
 * executable and runs it. CPU only; nothing is loaded into python.
 * It queries the built-in scenes with regions of one to six planes through and beside their root boxes - half-spaces, slabs,
 * wedges, closed boxes, normals from 1e-20 to 1e15 -, with every kind of invalid query (a NaN, an infinity) and the legal edges
 * (six absent planes, a zero normal with d < 0 and with d = -0, contradictory planes, offsets of 1e19), unaligned buffers,
 * caller-made and decreasing offsets, a capacity that cuts segments, an empty scene and no frusta, and checks what must hold
 * whatever the scene: ANY == (COUNT > 0), the offsets are the counts' running total, a segment's keys ascend strictly, nothing is
 * written at or past the capacity. */
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
  /* buffers at odd addresses: the twins ask no alignment */
  char* rawb = malloc(n * sizeof(mi_frustum) + 1);
  char* rawc = malloc(n * sizeof(uint32_t) + 1);
  char* rawo = malloc((n + 1) * sizeof(uint64_t) + 1);
  unsigned char* any = malloc(n);
  mi_frustum* frs = (mi_frustum*)(rawb + 1);
  void* counts = rawc + 1;
  uint64_t* offsets = (uint64_t*)(rawo + 1);
  const float lo[3] = {d.bvh_nodes[0].min_x, d.bvh_nodes[0].min_y, d.bvh_nodes[0].min_z};
  const float scales[6] = {1.0f, 1e-20f, 1e15f, 0.001f, 1024.0f, 3.0f};
  for (size_t i = 0; i < n; ++i) {
    mi_frustum f;
    memset(&f, 0, sizeof f);
    const int present = 1 + (int)(i % 6);
    for (int k = 0; k < present; ++k) {
      /* a plane through a point near the root box, the normal towards the box's corner or away from it */
      float p[3], nn[3];
      for (int a = 0; a < 3; ++a) {
        p[a] = lo[a] + (rnd() * 3.f - 1.f) * 600.f;
        nn[a] = (rnd() * 2.f - 1.f) * scales[(i / 6) % 6];
      }
      if (k % 3 == 1) nn[(int)(rnd() * 3.f) % 3] = 0.f;
      f.planes[k][0] = nn[0]; f.planes[k][1] = nn[1]; f.planes[k][2] = nn[2];
      f.planes[k][3] = -(nn[0] * p[0] + nn[1] * p[1] + nn[2] * p[2]);
    }
    if (i % 97 == 0) f.planes[0][0] = NAN;
    if (i % 101 == 0) f.planes[2][3] = INFINITY;
    if (i % 103 == 0) { f.planes[5][0] = f.planes[5][1] = f.planes[5][2] = 0.f; f.planes[5][3] = -1.f; }      /* empty by a zero normal */
    if (i % 107 == 0) { f.planes[5][0] = f.planes[5][1] = f.planes[5][2] = 0.f; f.planes[5][3] = -0.f; }
    if (i % 109 == 0) memset(&f, 0, sizeof f);                                                                /* the whole scene */
    if (i % 113 == 0) { f.planes[0][0] = 1.f; f.planes[0][3] = -(lo[0] + 1.f); f.planes[1][0] = -1.f; f.planes[1][3] = lo[0] - 1.f; }      /* contradictory */
    if (i % 127 == 0) { f.planes[0][0] = 1.f; f.planes[0][1] = f.planes[0][2] = 0.f; f.planes[0][3] = 1e19f; }
    if (i % 131 == 0) f.planes[4][1] = -INFINITY;
    memcpy(frs + i, &f, sizeof f);
  }
  uint64_t va[2], vc[2], vo[2], vf[2];
  int bad = 0;
  if (mi_frustum_query_host(&d, MI_FRUSTUM_ANY, frs, any, n, va) != MI_OK || mi_frustum_query_host(&d, MI_FRUSTUM_COUNT, frs, counts, n, vc) != MI_OK ||
      mi_frustum_offsets_host(&d, frs, offsets, n, vo) != MI_OK) {
    fprintf(stderr, "%s: %s\n", name, mi_host_last_error());
    return 1;
  }
  uint64_t total = 0, first;
  memcpy(&first, offsets, sizeof first);
  if (first != 0) ++bad;
  for (size_t i = 0; i < n; ++i) {
    uint32_t c; uint64_t o;
    memcpy(&c, (char*)counts + i * sizeof c, sizeof c);
    memcpy(&o, (char*)offsets + (i + 1) * sizeof o, sizeof o);
    total += c;
    if (o != total || (c > 0) != (any[i] != 0)) ++bad;
  }
  if (vo[0] != vc[0] || vo[1] != vc[1] || va[0] > vc[0]) ++bad;
  /* the full fill, then a capacity that cuts it in the middle, into exactly sized buffers: a write past them is the sanitizer's */
  for (int pass = 0; pass < 2; ++pass) {
    const size_t capacity = (size_t)(pass ? total / 2 : total);
    char* rawh = malloc(capacity * sizeof(mi_overlap) + 1);
    mi_overlap* hits = (mi_overlap*)(rawh + 1);
    if (mi_frustum_fill_host(&d, frs, offsets, hits, capacity, n, vf) != MI_OK) ++bad;
    if (!pass && (vf[0] > vo[0] || vf[1] > vo[1])) ++bad;
    uint64_t prev_key = 0; uint32_t prev_box = 0xFFFFFFFFu;
    for (size_t j = 0; j < capacity; ++j) {
      mi_overlap r;
      memcpy(&r, (char*)hits + j * sizeof r, sizeof r);
      const uint64_t key = ((uint64_t)r.geomID << 32) | r.primID;
      if (r.geomID >= d.num_geometry || (r.flags != 0 && r.flags != MI_OVERLAP_CONTAINED) || r.reserved != 0 || r.box >= n) ++bad;
      if (r.box == prev_box && key <= prev_key) ++bad;
      prev_key = key; prev_box = r.box;
    }
    free(rawh);
  }
  /* caller-made offsets: K = 3 per frustum, then the same pairs reversed (decreasing: nothing is written, nothing walked) */
  uint64_t* koff = malloc((n + 1) * sizeof(uint64_t));
  mi_overlap* khits = malloc(3 * n * sizeof(mi_overlap));
  for (size_t i = 0; i <= n; ++i) koff[i] = 3 * i;
  if (mi_frustum_fill_host(&d, frs, koff, khits, 3 * n, n, NULL) != MI_OK) ++bad;
  for (size_t i = 0; i < n; ++i) {
    uint32_t c;
    memcpy(&c, (char*)counts + i * sizeof c, sizeof c);
    for (uint32_t j = 0; j < 3; ++j) {
      const mi_overlap r = khits[3 * i + j];
      if (r.box != i || (j < c) != (r.primID != MI_INVALID_PRIM || r.geomID != MI_INVALID_GEOM) || (j >= c && r.flags != MI_FLAG_ESCAPED)) ++bad;
    }
  }
  for (size_t i = 0; i <= n; ++i) koff[i] = 3 * (n - i);
  if (mi_frustum_fill_host(&d, frs, koff, khits, 3 * n, n, vf) != MI_OK || vf[0] || vf[1]) ++bad;
  free(koff); free(khits);
  printf("%s: %zu frusta, %llu overlaps, %llu box tests, %llu primitive tests (ANY: %llu, %llu), %d bad\n", name, n, (unsigned long long)total,
         (unsigned long long)vc[0], (unsigned long long)vc[1], (unsigned long long)va[0], (unsigned long long)va[1], bad);
  /* no frusta; visits not asked for */
  if (mi_frustum_query_host(&d, MI_FRUSTUM_ANY, NULL, NULL, 0, NULL) != MI_OK || mi_frustum_offsets_host(&d, NULL, NULL, 0, NULL) != MI_OK ||
      mi_frustum_fill_host(&d, NULL, NULL, NULL, 0, 0, NULL) != MI_OK) ++bad;
  /* refusals */
  if (mi_frustum_query_host(NULL, 0, frs, any, n, NULL) != MI_ERR_INVALID_ARG || mi_frustum_query_host(&d, 2, frs, any, n, NULL) != MI_ERR_INVALID_ARG ||
      mi_frustum_query_host(&d, 0, NULL, any, n, NULL) != MI_ERR_INVALID_ARG || mi_frustum_offsets_host(&d, frs, NULL, n, NULL) != MI_ERR_INVALID_ARG) ++bad;
  /* nodes cut short: not a depth-first BVH2 any more, refused before anything is read past the end */
  if (d.num_nodes > 2) {
    mi_scene_desc cut = d;
    cut.num_nodes = d.num_nodes - 1;
    if (mi_frustum_query_host(&cut, 0, frs, any, 1, NULL) != MI_ERR_INVALID_ARG) ++bad;
  }
  free(rawb); free(rawc); free(rawo); free(any);
  mi_host_scene_destroy(hs);
  return bad;
}

int main(int argc, char** argv) {
  const char* mesh = argc > 1 ? argv[1] : "assets/monkey_bust.glb";
  int bad = run_scene("spheres", mesh, 5000) + run_scene("box-simple", mesh, 5000) + run_scene("box", mesh, 5000);
  /* an empty scene */
  mi_scene_desc empty;
  memset(&empty, 0, sizeof empty);
  mi_frustum b;
  memset(&b, 0, sizeof b);
  b.planes[0][0] = 1.f; b.planes[0][3] = 1.f;      /* x >= -1 */
  unsigned char any = 7;
  uint64_t off[2] = {9, 9}, v[2] = {9, 9};
  mi_overlap pad[2];
  const uint64_t two[2] = {0, 2};
  if (mi_frustum_query_host(&empty, MI_FRUSTUM_ANY, &b, &any, 1, v) != MI_OK || any != 0 || v[0] || v[1]) ++bad;
  if (mi_frustum_offsets_host(&empty, &b, off, 1, NULL) != MI_OK || off[0] || off[1]) ++bad;
  if (mi_frustum_fill_host(&empty, &b, two, pad, 2, 1, NULL) != MI_OK || pad[1].primID != MI_INVALID_PRIM || pad[1].flags != MI_FLAG_ESCAPED) ++bad;
  /* the bounds test on its own: a null pointer and a query that is not valid give 0 */
  const float mn[3] = {-0.5f, -0.5f, -0.5f}, mx[3] = {0.5f, 0.5f, 0.5f};
  mi_frustum zero = b;
  zero.planes[3][2] = NAN;
  if (mi_frustum_meets_bounds_host(&b, mn, mx) != 1 || mi_frustum_meets_bounds_host(NULL, mn, mx) != 0 || mi_frustum_meets_bounds_host(&zero, mn, mx) != 0) ++bad;
  printf(bad ? "FAILED: %d\n" : "sanitize_frustum_query OK\n", bad);
  return bad ? 1 : 0;
}
