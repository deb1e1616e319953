// bvh_cost_host.hpp — the surface-area cost of a tree of compact nodes on the host: the twin of the device pass
// (cost_kernels.hpp). Terms, the reduction's shape and the block width are the MI_HD code of ray_math.h that the kernels run, so
// the three doubles equal the device's bit for bit. Used by mi_bvh_cost_compact (host/scene_api.cpp) and by
// mi_scene_bvh_cost for a scene whose nodes are still only on the host (raylib.hip).
#pragma once

#include <vector>

#include "../../include/mi_raylib.h"
#include "ray_math.h"

namespace mi {

// out = {sum_all, sum_leaf, a_root}; W = the block width (a power of two, at least 2; kCostBlock is what the device runs)
inline void bvh_cost_host(const mi_bvh_node* nodes, uint32_t n, uint32_t W, double out[3]) {
  out[0] = out[1] = out[2] = 0.0;
  if (!n) return;
  std::vector<Cost2> level(n), block(W);
  for (uint32_t i = 0; i < n; ++i) {
    const double a = bvh_cost_term(nodes[i].dx, nodes[i].dy, nodes[i].dz);
    level[i].all = a;
    level[i].leaf = nodes[i].geom_id != MI_INVALID_GEOM ? a : 0.0;
  }
  out[2] = level[0].all;
  do {
    const uint32_t count = (uint32_t)level.size(), blocks = cost_blocks(count, W);
    std::vector<Cost2> next(blocks);
    for (uint32_t b = 0; b < blocks; ++b) {
      for (uint32_t k = 0; k < W; ++k) {
        const uint64_t i = (uint64_t)b * W + k;
        block[k] = i < count ? level[i] : Cost2{0.0, 0.0};
      }
      cost_block_reduce(block.data(), W, 0u, 1u, [] {});
      next[b] = block[0];
    }
    level.swap(next);
  } while (level.size() > 1);
  out[0] = level[0].all; out[1] = level[0].leaf;
}

}  // namespace mi
