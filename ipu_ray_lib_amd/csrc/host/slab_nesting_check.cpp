// slab_nesting_check.cpp — a stand-alone check (its own main; built and run by tests/test_hot_collapse.py, never part of a library)
// of what a collapsed walk (csrc/hot_order.hpp) would need from the box test on the lanes that run it literally - a zero or denormal
// direction component, a non-finite origin, where "the slab arithmetic is monotone" says nothing: for a box inside another box,
// CHILD HIT => PARENT HIT under the reference's compare / select sequence (CompactBVH2Node.hpp:14-50 as box_hit_literal_axis of
// trace_kernels.hpp writes it: ordered compares that a NaN fails, the far product scaled by kSlabScale). Origins and directions
// run per axis over +-0, denormals, +-inf, NaN and values on and beside the planes, all three axes crossed, against nested box
// pairs (shared faces, flat children inside and ON a face, equal boxes), with hit.t = inf and a finite hit.t.
//
// The implication does NOT hold: a child that is flat on an axis and lies on a face of a parent that is not flat there is hit while
// the parent is missed, with the origin on that plane and the direction component -0 (the child's two products are NaN and drop out
// of every compare; the parent's are NaN and -inf, or +inf and NaN). That is why casts on the literal test never walk the collapsed
// tree (hot_join_regions). Exit status 0 = counter-examples were found, and EVERY one of them has such an axis, a direction component
// whose reciprocal is -inf on it and the origin on the child's plane: nothing else breaks the implication.
#include <cmath>
#include <cstdio>
#include <limits>

#include "../ray_math.h"

namespace {

struct Interval { float lo, hi; };
struct Nested { Interval child, parent; };

bool box_hit_literal(const Interval b[3], const float o[3], const float inv[3], float tCur) {
  float t0 = 0.f, t1 = tCur;
  for (int a = 0; a < 3; ++a) {
    float tmin = (b[a].lo - o[a]) * inv[a], tmax = (b[a].hi - o[a]) * inv[a];
    if (tmin > tmax) { const float s = tmin; tmin = tmax; tmax = s; }
    tmax *= mi::kSlabScale;
    t0 = tmin > t0 ? tmin : t0;
    t1 = tmax < t1 ? tmax : t1;
  }
  return !(t0 > t1);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float tiny = std::numeric_limits<float>::denorm_min();       // its reciprocal is +inf
  const float sub = 1.1754942e-38f;                                  // the largest denormal: a finite reciprocal
  // planes at -1, 0, 0.5, 1, 2: origins on them, beside them, inside, outside (-1 is outside most children), and the specials
  const float origins[] = {0.f, -0.f, tiny, -tiny, 2.f, 1.f, std::nextafterf(1.f, 2.f), 0.25f, -1.f, inf, -inf, nan};
  const float dirs[] = {0.f, -0.f, tiny, -tiny, sub, -sub, 1.f, -1.f, 0.3f, inf, -inf, nan};
  const Nested per_axis[] = {
      {{0.f, 1.f}, {-1.f, 2.f}},      // strictly inside
      {{0.f, 1.f}, {0.f, 1.f}},       // equal
      {{0.f, 0.5f}, {-1.f, 1.f}},
      {{1.f, 1.f}, {0.f, 2.f}},       // a flat child on the plane 1
      {{0.f, 0.f}, {0.f, 0.f}},       // flat, both, on the plane 0
      {{-1.f, 0.f}, {-1.f, 2.f}},     // a shared lower face
      {{0.5f, 2.f}, {-1.f, 2.f}},     // a shared upper face
      {{0.f, 0.f}, {0.f, 2.f}},       // a flat child ON the lower face
      {{2.f, 2.f}, {-1.f, 2.f}},      // a flat child ON the upper face
  };
  const int patterns[][3] = {{0, 0, 0}, {3, 3, 3}, {4, 4, 4}, {5, 5, 5}, {6, 6, 6}, {0, 3, 5}, {3, 5, 0}, {4, 1, 6}, {2, 6, 4}, {7, 0, 0}, {0, 8, 0}, {0, 2, 7}, {8, 5, 6}, {7, 8, 3}};
  const float fars[] = {inf, 0.75f};
  const int NO = sizeof origins / sizeof origins[0], ND = sizeof dirs / sizeof dirs[0];
  unsigned long long tests = 0, both = 0, broken = 0;
  for (const auto& pat : patterns) {
    Interval child[3], parent[3];
    for (int a = 0; a < 3; ++a) { child[a] = per_axis[pat[a]].child; parent[a] = per_axis[pat[a]].parent; }
    for (int ox = 0; ox < NO; ++ox) for (int oy = 0; oy < NO; ++oy) for (int oz = 0; oz < NO; ++oz) {
      const float o[3] = {origins[ox], origins[oy], origins[oz]};
      for (int dx = 0; dx < ND; ++dx) for (int dy = 0; dy < ND; ++dy) for (int dz = 0; dz < ND; ++dz) {
        const float inv[3] = {1.f / dirs[dx], 1.f / dirs[dy], 1.f / dirs[dz]};
        for (float far : fars) {
          ++tests;
          if (!box_hit_literal(child, o, inv, far)) continue;
          ++both;
          if (!box_hit_literal(parent, o, inv, far)) {
            ++broken;
            bool known = false;      // a flat child on a face of a parent that is not flat, the origin on it, a reciprocal of -inf
            for (int a = 0; a < 3; ++a)
              known = known || (child[a].lo == child[a].hi && parent[a].lo < parent[a].hi && (child[a].lo == parent[a].lo || child[a].lo == parent[a].hi) &&
                                o[a] == child[a].lo && inv[a] == -inf);
            if (!known) {
              fprintf(stderr, "slab_nesting_check: child hit, parent missed, and no flat child on a face: boxes {%d %d %d}, origin (%g %g %g), direction (%g %g %g), hit.t %g\n",
                      pat[0], pat[1], pat[2], o[0], o[1], o[2], dirs[dx], dirs[dy], dirs[dz], far);
              return 1;
            }
          }
        }
      }
    }
  }
  if (!broken) { fprintf(stderr, "slab_nesting_check: no counter-example found: the enumeration has lost the flat child on a face\n"); return 1; }
  printf("slab_nesting_check OK: %llu box pairs tested, %llu with the child hit, %llu of them with the parent missed - each a flat child on a face\n", tests, both, broken);
  return 0;
}
