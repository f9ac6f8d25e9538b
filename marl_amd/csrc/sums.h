// Deterministic two-stage sums of the loss kernels (mixers.hip, policy.hip): every workgroup of 256 threads leaves NV partial sums
// in a workspace row, one single-workgroup launch adds the rows in a fixed order.  No float atomics: two calls give the same bits.
#pragma once
#include "common.h"

namespace {

constexpr int SUMS_TPB = 256;

template <int NV>
__device__ __forceinline__ void block_partials(float (&v)[NV], float* ws) {
  __shared__ float sh[NV][SUMS_TPB / 64];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0) sh[i][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    float s = 0.f;
    for (int w = 0; w < SUMS_TPB / 64; ++w) s += sh[threadIdx.x][w];
    ws[(long)blockIdx.x * NV + threadIdx.x] = s;
  }
}

// the fixed-order tree of the finish pass, called by every thread of ONE workgroup of SUMS_TPB: column i of nblocks workspace rows
// of nv partials - a strided sum per thread, then the LDS halving; every thread gets the total
__device__ __forceinline__ float block_tree_sum(const float* ws, int nblocks, int nv, int i) {
  __shared__ float sh[SUMS_TPB];
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += SUMS_TPB) s += ws[(long)b * nv + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = SUMS_TPB / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const float tot = sh[0];
  __syncthreads();                     // sh is free for the next column
  return tot;
}

__global__ void finish_sums_kernel(const float* ws, int nblocks, int nv, float* out) {
  for (int i = 0; i < nv; ++i) {
    const float tot = block_tree_sum(ws, nblocks, nv, i);
    if (threadIdx.x == 0) out[i] = tot;
  }
}

}  // namespace
