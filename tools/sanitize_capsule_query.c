/* sanitize_capsule_query.c - the host twins of capsule queries (mi_capsule_query_host, mi_capsule_offsets_host, mi_capsule_fill_host,
 * include/mi_scene_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer, from a stand-alone program:
 * tools/sanitize_capsule_query.sh builds the host library's sources and this file with -fsanitize=address,undefined into one
 * executable and runs it. CPU only; nothing is loaded into python.
 * It queries the built-in scenes with capsules inside, outside and across their root boxes, of every length and radius from a point
 * to the whole scene, in every direction, with every kind of invalid query (a NaN, an infinity, a negative radius) and the legal
 * edges (a == b, radius 0 and -0, a length whose square underflows, coordinates whose products overflow), unaligned buffers,
 * caller-made and decreasing offsets, a capacity that cuts segments, an empty scene and no capsules, and checks what must hold whatever the scene: ANY == (COUNT > 0), the offsets are the counts' running total, a
 * segment's keys ascend strictly, nothing is written at or past the capacity. */
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
  char* rawb = malloc(n * sizeof(mi_capsule) + 1);
  char* rawc = malloc(n * sizeof(uint32_t) + 1);
  char* rawo = malloc((n + 1) * sizeof(uint64_t) + 1);
  unsigned char* any = malloc(n);
  mi_capsule* caps = (mi_capsule*)(rawb + 1);
  void* counts = rawc + 1;
  uint64_t* offsets = (uint64_t*)(rawo + 1);
  const float lo[3] = {d.bvh_nodes[0].min_x, d.bvh_nodes[0].min_y, d.bvh_nodes[0].min_z};
  const float sizes[6] = {0.0f, 1.0f, 10.0f, 60.0f, 300.0f, 5000.0f};
  for (size_t i = 0; i < n; ++i) {
    mi_capsule c;
    memset(&c, 0, sizeof c);
    const float len = sizes[(i / 6) % 6];
    for (int k = 0; k < 3; ++k) {
      c.a[k] = lo[k] + (rnd() * 3.f - 1.f) * 600.f;
      c.b[k] = c.a[k] + (rnd() * 2.f - 1.f) * len;
    }
    c.radius = sizes[i % 6] * (0.5f + 0.5f * rnd());
    if (i % 97 == 0) c.a[0] = NAN;
    if (i % 101 == 0) c.b[1] = INFINITY;
    if (i % 103 == 0) c.radius = -1.f;
    if (i % 107 == 0) c.radius = -0.f;
    if (i % 109 == 0) { c.a[0] = 0.f; c.b[0] = 1e-30f; c.b[1] = c.a[1]; c.b[2] = c.a[2]; }      /* dd underflows */
    if (i % 113 == 0) c.radius = NAN;
    if (i % 127 == 0) { c.a[0] = -1e19f; c.b[0] = 1e19f; }                                         /* products overflow */
    if (i % 131 == 0) c.radius = INFINITY;
    memcpy(caps + i, &c, sizeof c);
  }
  uint64_t va[2], vc[2], vo[2], vf[2];
  int bad = 0;
  if (mi_capsule_query_host(&d, MI_CAPSULE_ANY, caps, any, n, va) != MI_OK || mi_capsule_query_host(&d, MI_CAPSULE_COUNT, caps, counts, n, vc) != MI_OK ||
      mi_capsule_offsets_host(&d, caps, offsets, n, vo) != MI_OK) {
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
    if (mi_capsule_fill_host(&d, caps, offsets, hits, capacity, n, vf) != MI_OK) ++bad;
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
  /* caller-made offsets: K = 3 per capsule, then the same pairs reversed (decreasing: nothing is written, nothing walked) */
  uint64_t* koff = malloc((n + 1) * sizeof(uint64_t));
  mi_overlap* khits = malloc(3 * n * sizeof(mi_overlap));
  for (size_t i = 0; i <= n; ++i) koff[i] = 3 * i;
  if (mi_capsule_fill_host(&d, caps, koff, khits, 3 * n, n, NULL) != MI_OK) ++bad;
  for (size_t i = 0; i < n; ++i) {
    uint32_t c;
    memcpy(&c, (char*)counts + i * sizeof c, sizeof c);
    for (uint32_t j = 0; j < 3; ++j) {
      const mi_overlap r = khits[3 * i + j];
      if (r.box != i || (j < c) != (r.primID != MI_INVALID_PRIM || r.geomID != MI_INVALID_GEOM) || (j >= c && r.flags != MI_FLAG_ESCAPED)) ++bad;
    }
  }
  for (size_t i = 0; i <= n; ++i) koff[i] = 3 * (n - i);
  if (mi_capsule_fill_host(&d, caps, koff, khits, 3 * n, n, vf) != MI_OK || vf[0] || vf[1]) ++bad;
  free(koff); free(khits);
  printf("%s: %zu capsules, %llu overlaps, %llu box tests, %llu primitive tests (ANY: %llu, %llu), %d bad\n", name, n, (unsigned long long)total,
         (unsigned long long)vc[0], (unsigned long long)vc[1], (unsigned long long)va[0], (unsigned long long)va[1], bad);
  /* no capsules; visits not asked for */
  if (mi_capsule_query_host(&d, MI_CAPSULE_ANY, NULL, NULL, 0, NULL) != MI_OK || mi_capsule_offsets_host(&d, NULL, NULL, 0, NULL) != MI_OK ||
      mi_capsule_fill_host(&d, NULL, NULL, NULL, 0, 0, NULL) != MI_OK) ++bad;
  /* refusals */
  if (mi_capsule_query_host(NULL, 0, caps, any, n, NULL) != MI_ERR_INVALID_ARG || mi_capsule_query_host(&d, 2, caps, any, n, NULL) != MI_ERR_INVALID_ARG ||
      mi_capsule_query_host(&d, 0, NULL, any, n, NULL) != MI_ERR_INVALID_ARG || mi_capsule_offsets_host(&d, caps, NULL, n, NULL) != MI_ERR_INVALID_ARG) ++bad;
  /* nodes cut short: not a depth-first BVH2 any more, refused before anything is read past the end */
  if (d.num_nodes > 2) {
    mi_scene_desc cut = d;
    cut.num_nodes = d.num_nodes - 1;
    if (mi_capsule_query_host(&cut, 0, caps, any, 1, NULL) != MI_ERR_INVALID_ARG) ++bad;
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
  mi_capsule b = {{0.f, 0.f, 0.f}, 1.f, {1.f, 1.f, 1.f}, 0};
  unsigned char any = 7;
  uint64_t off[2] = {9, 9}, v[2] = {9, 9};
  mi_overlap pad[2];
  const uint64_t two[2] = {0, 2};
  if (mi_capsule_query_host(&empty, MI_CAPSULE_ANY, &b, &any, 1, v) != MI_OK || any != 0 || v[0] || v[1]) ++bad;
  if (mi_capsule_offsets_host(&empty, &b, off, 1, NULL) != MI_OK || off[0] || off[1]) ++bad;
  if (mi_capsule_fill_host(&empty, &b, two, pad, 2, 1, NULL) != MI_OK || pad[1].primID != MI_INVALID_PRIM || pad[1].flags != MI_FLAG_ESCAPED) ++bad;
  /* the bounds test on its own: a null pointer and a query that is not valid give 0 */
  const float mn[3] = {-0.5f, -0.5f, -0.5f}, mx[3] = {0.5f, 0.5f, 0.5f};
  mi_capsule zero = b;
  zero.radius = -1.f;
  if (mi_capsule_meets_bounds_host(&b, mn, mx) != 1 || mi_capsule_meets_bounds_host(NULL, mn, mx) != 0 || mi_capsule_meets_bounds_host(&zero, mn, mx) != 0) ++bad;
  printf(bad ? "FAILED: %d\n" : "sanitize_capsule_query OK\n", bad);
  return bad ? 1 : 0;
}
