// cross_host.cpp — mi_sphere_crossings_host and mi_sphere_roots_host (include/mi_scene_host.h): sphere_crossings and sphere_roots of
// cross_math.hpp, the one piece of the
// crossing-count arithmetic (mi_count_query / mi_point_sign) that has no reference counterpart, compiled for the host from the
// definition the kernels run, so that it can be checked without a GPU.
#include "../cross_math.hpp"
#include "../../../include/mi_scene_host.h"

extern "C" uint32_t mi_sphere_crossings_host(const float centre[3], float radius2, const float origin[3], const float direction[3],
                                             float t_min, float t_max) {
  if (!centre || !origin || !direction) return 0u;
  return mi::sphere_crossings(mi::mk(centre[0], centre[1], centre[2]), radius2, mi::mk(origin[0], origin[1], origin[2]),
                              mi::mk(direction[0], direction[1], direction[2]), t_min, t_max);
}

extern "C" uint32_t mi_sphere_roots_host(const float centre[3], float radius2, const float origin[3], const float direction[3],
                                         float t_min, float t_max, float t[2]) {
  if (!centre || !origin || !direction || !t) return 0u;
  return mi::sphere_roots(mi::mk(centre[0], centre[1], centre[2]), radius2, mi::mk(origin[0], origin[1], origin[2]),
                          mi::mk(direction[0], direction[1], direction[2]), t_min, t_max, t);
}
