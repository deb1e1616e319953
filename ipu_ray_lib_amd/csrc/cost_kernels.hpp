// cost_kernels.hpp — gfx950 kernels of mi_scene_bvh_cost and of the auto-rebuild policy: the surface-area cost of a scene's
// current compact nodes, summed on the device. The driver is sceneCost in raylib.hip, the host twin bvh_cost_host
// (bvh_cost_host.hpp, mi_bvh_cost_compact); DESIGN.md §18 has the definition, the reduction's shape and the numbers.
//
// Exactness. The term, the pairwise add and the reduction's shape are the MI_HD code of ray_math.h the twin runs. Floating-point
// addition is not associative, so nothing here adds in an order that scheduling decides: no atomics, one workgroup per block of
// kCostBlock consecutive entries, the fixed tree of cost_block_reduce inside it, one store per workgroup, and the next level in
// the next launch. The three doubles equal the twin's bit for bit, run to run and device to device.
//
// Passes, all on the caller's stream, kernel boundaries giving visibility between them:
//   1 cost_term_kernel      one thread per node: its term, reduced per workgroup into partials[blockIdx.x]; node 0's term -> root
//   2 cost_partials_kernel  one thread per partial of the level before, reduced the same way; launched until one entry is left
//   3 (host) one read-back of 32 bytes: a_root and {sum_all, sum_leaf}
// A bandwidth pass over the 24-byte nodes (8 of them read: the extents and the geomID); every index is checked against its count.
#pragma once

#include <hip/hip_runtime.h>

#include "ray_math.h"
#include "../../include/mi_raylib.h"

namespace mi {

__device__ __forceinline__ void cost_reduce_and_store(Cost2* sh, Cost2 mine, Cost2* out) {
  sh[threadIdx.x] = mine;
  __syncthreads();
  cost_block_reduce(sh, kCostBlock, threadIdx.x, kCostBlock, [] { __syncthreads(); });
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// pass 1: gridDim.x = cost_blocks(n, kCostBlock)
__global__ void __launch_bounds__(kCostBlock) cost_term_kernel(const mi_bvh_node* nodes, uint32_t n, Cost2* partials, double* root) {
  __shared__ Cost2 sh[kCostBlock];
  const uint32_t i = blockIdx.x * kCostBlock + threadIdx.x;
  Cost2 v; v.all = 0.0; v.leaf = 0.0;
  if (i < n) {
    const mi_bvh_node c = nodes[i];
    const double a = bvh_cost_term(c.dx, c.dy, c.dz);
    v.all = a;
    v.leaf = c.geom_id != MI_INVALID_GEOM ? a : 0.0;
    if (i == 0) *root = a;
  }
  cost_reduce_and_store(sh, v, partials);
}

// pass 2: gridDim.x = cost_blocks(n, kCostBlock); in and out are different levels of the partials buffer
__global__ void __launch_bounds__(kCostBlock) cost_partials_kernel(const Cost2* in, uint32_t n, Cost2* out) {
  __shared__ Cost2 sh[kCostBlock];
  const uint32_t i = blockIdx.x * kCostBlock + threadIdx.x;
  Cost2 v; v.all = 0.0; v.leaf = 0.0;
  if (i < n) v = in[i];
  cost_reduce_and_store(sh, v, out);
}

}  // namespace mi
