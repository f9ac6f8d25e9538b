// What the MAIC message head's forward (maic_head.hip) and backward (maic_head_bwd.hip) share: the fixed sizes of the head,
// the tile decomposition (one wave owns G = 16 / N whole environments) and the small device helpers.
#pragma once
#include "head_tile.h"
#include "../../include/marl_hip.h"

namespace maic {

constexpr int MC_H = 64;             // rnn_hidden_dim
constexpr int MC_NH = 64;            // nn_hidden_size
constexpr int MC_L = 8;              // latent_dim
constexpr int MC_D = 32;             // attention_dim
constexpr int MC_NMAX = 16;
constexpr int MC_AMAX = 32;
constexpr int MC_LDH = MC_H + 4;
constexpr int MC_LDL = MC_NMAX * MC_L + 4;
constexpr int MC_LDK = MC_D + 4;
constexpr int MC_LDQ = MC_L + 4;     // kq: L products + key . bq
constexpr int MC_LDA = MC_NMAX + 1;
constexpr int MC_M0 = MC_H + MC_L;   // row length of msg_net.0
constexpr int MC_RED = 16;           // slices of the statistics merge
constexpr float MC_QSCALE = 0.17677669529663687f;   // 1 / sqrt(attention_dim)

__host__ __device__ inline int mc_envs_per_tile(int N) { return N >= 16 ? 1 : 16 / N; }

// every dense product here starts from zero, has K = 64 and a zero-padded X: the unguarded flavour
__device__ __forceinline__ f32x4 mc_gemm(const float* X, int ldx, int K, const float* __restrict__ W, long ldw, int n0,
                                         int nvalid) {
  return head_tile::tile_gemm<false>(f32x4{0, 0, 0, 0}, X, ldx, K, W, ldw, 0, n0, nvalid);
}

__device__ __forceinline__ float leaky(float t) { return t > 0.0f ? t : 0.01f * t; }

// (n, mean, m2) <- merge with (nb, mb, m2b)
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  if (nb == 0.0f) return;
  const float nt = n + nb, d = mb - mean;
  mean += d * (nb / nt);
  m2 += m2b + d * d * (n * nb / nt);
  n = nt;
}

inline bool maic_weights_ok(const marl_maic_weights_t* w) {
  const void* ps[] = {w->e0_w, w->e0_b, w->bn_w, w->bn_b, w->bn_rm, w->bn_rv, w->e3_w, w->e3_b, w->m0_w, w->m0_b,
                      w->m2_w, w->m2_b, w->k_w, w->k_b, w->q_w, w->q_b};
  for (const void* q : ps)
    if (!q) return false;
  return true;
}

}  // namespace maic
