// What the head kernels (rtw_head.hip, world_head.hip, maic_head.hip) share: one wave owns a 16-row tile held in LDS and
// multiplies it with weights read through L2 on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).
//
// K-permutation (mfma16x4 in common.h): a chunk of 16 k values is four MFMA steps; at step i lane quarter q = lane >> 4
// supplies k0 + 4q + i for BOTH operands.  The sum over k does not care about the order, and each lane's four operands are
// 16 contiguous bytes of its X row and of its W row.  The result is the usual D layout: register r of lane l holds row
// drow(r), column n0 + (l & 15).
#pragma once
#include "common.h"

namespace head_tile {

__host__ __device__ inline long pad64(long n) { return (n + 63) / 64 * 64; }
__host__ __device__ inline int round4(int n) { return (n + 3) / 4 * 4; }

// row of D register r for this lane; its column is n0 + (lane & 15)
__device__ __forceinline__ int drow(int r) { return 4 * (threadIdx.x >> 4) + r; }

// acc[16 x 16 column tile n0] += X[16 x K] * W[n0.., coff + k]^T.  X in LDS (row pitch ldx), W row-major with row stride
// ldw; rows n >= nvalid of W read as 0.  KGUARD: k >= K reads as 0 (any K; X zero-padded to a multiple of 16 columns or
// not).  Without it K % 16 == 0 is the caller's promise, and the loop carries no per-element test - with K a constant the
// guarded form does not fold to this one, so the flavour is a compile-time choice.
template <bool KGUARD>
__device__ __forceinline__ f32x4 tile_gemm(f32x4 acc, const float* X, int ldx, int K, const float* __restrict__ W, long ldw,
                                           int coff, int n0, int nvalid) {
  const int l = threadIdx.x, m = l & 15, q4 = (l >> 4) * 4;
  const int n = n0 + m;
  const bool nok = n < nvalid;
  const float* wr = W + (long)(nok ? n : 0) * ldw + coff;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int k = k0 + q4;
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool kok = !KGUARD || k + i < K;
      a[i] = kok ? X[m * ldx + k + i] : 0.0f;
      b[i] = (kok && nok) ? __ldg(wr + k + i) : 0.0f;
    }
    acc = mfma16x4(a, b, acc);
  }
  return acc;
}

// acc[16 x 16 column tile n0] += X[16 x K] W: W row-major (K rows of ldw floats, columns n < nvalid) - the input gradient of
// a Linear layer whose weight is W.  k >= K reads as 0.
__device__ __forceinline__ f32x4 tile_gemm_t(f32x4 acc, const float* X, int ldx, int K, const float* __restrict__ W, long ldw,
                                             int n0, int nvalid) {
  const int l = threadIdx.x, m = l & 15, q4 = (l >> 4) * 4;
  const int n = n0 + m;
  const bool nok = n < nvalid;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int k = k0 + q4;
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool kok = k + i < K;
      a[i] = kok ? X[m * ldx + k + i] : 0.0f;
      b[i] = (kok && nok) ? __ldg(W + (long)(k + i) * ldw + n) : 0.0f;
    }
    acc = mfma16x4(a, b, acc);
  }
  return acc;
}

// sh[16][ld] <- rows row0 .. row0 + 15 of h (rows of 64 floats); tile rows r with !valid(r) are zeros and are not read
template <class V>
__device__ __forceinline__ void load_h(float* sh, int ld, const float* h, long row0, V valid) {
  for (int idx = threadIdx.x; idx < 16 * 64; idx += 64) {
    const int r = idx / 64, c = idx % 64;
    sh[r * ld + c] = valid(r) ? h[(row0 + r) * 64 + c] : 0.0f;
  }
}

}  // namespace head_tile
