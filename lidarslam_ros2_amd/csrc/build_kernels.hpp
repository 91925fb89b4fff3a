// The key kernel shared by the target-side builders (grid_build.hip) and the voxel filter (cloud_codec.hip): each translation unit
// compiles its own copy (internal linkage).  The voxel arithmetic itself lives in voxel_device.hpp.
#pragma once
#include "voxel_device.hpp"

namespace lsr {
namespace {

// key = linear leaf index exactly as VoxelGridCovariance computes it (voxel_device.hpp: leaf_key)
__global__ __launch_bounds__(256) void leaf_key_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, int n, float inv_leaf, int mb0, int mb1,
                                                       int mb2, int mul1, int mul2, unsigned int sentinel,
                                                       unsigned int* __restrict__ key,
                                                       uint4* __restrict__ fill_a, size_t n_a, int* __restrict__ fill_b, size_t n_b,
                                                       int* __restrict__ zero_word) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  // the all-ones fills of the sort-based builder (NaN leaf records of empty cells, cell_slot = -1) and its counter ride along:
  // three memset launches less
  for (size_t k = (size_t)i; k < n_a; k += (size_t)gridDim.x * blockDim.x) fill_a[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (size_t k = (size_t)i; k < n_b; k += (size_t)gridDim.x * blockDim.x) fill_b[k] = -1;
  if (i == 0 && zero_word) *zero_word = 0;
  if (i >= n) return;
  key[i] = leaf_key<int>(x[i], y[i], z[i], inv_leaf, mb0, mb1, mb2, mul1, mul2, sentinel);   // (the sort numbers the values itself)
}

}  // namespace
}  // namespace lsr
