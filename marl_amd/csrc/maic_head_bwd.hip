// Backward of the MAIC message head (csrc/maic_head.hip; autograd of reference network/MAIC.py:58-87) on gfx950, for a sparse
// gradient on return_q: one (action a_j, value v_j) pair per row j - what the TD loss leaves after the gather, and what BPTT
// already takes for the identity path q -> return_q.  This file produces the head's own contribution to dh and the head's
// weight gradients; inference_net gets none (it only feeds the MI loss).
//
// With senders i and receivers j of one environment (notation of maic_head.hip):
//   d msg[i][j] = alpha[i][j] v_j on action a_j only, so
//   d hid[i][j] = alpha[i][j] v_j msg_net.2[a_j, :]                     d pre[i][j] = d hid[i][j] LeakyReLU'(pre[i][j])
//   d alpha[i][j] = v_j (msg_net.2[a_j, :] . hid[i][j] + b2[a_j])       (test mode: 0 where the gate zeroed alpha)
//   d msg_net.2[a_j, :] += v_j S_j with S_j = sum_i alpha[i][j] hid[i][j] - the forward's own S - and d b2[a_j] += v_j sum_i alpha[i][j]
//   d U_j = sum_i d pre[i][j]   (U_j = msg_net.0[:, :64] h_j + b: the h_repeat quirk puts the RECEIVER's h there)
//   d lat[i][j] = msg_net.0[:, 64:]^T d pre[i][j] + d logit[i][j] (Wq^T key_i) / sqrt(D)
//   d logit[i][.] = softmax backward of d alpha[i][.] (diagonal: a constant, no gradient)
//   d key_i = (Wq G_i + bq g_i) / sqrt(D), d Wq = sum_i key_i (x) G_i / sqrt(D), d bq = sum_i key_i g_i / sqrt(D)
//     with G_i = sum_j d logit[i][j] lat[i][j], g_i = sum_j d logit[i][j]
//   lat = mu + sqrt(v) eps, v = max(exp(lv), var_floor): d mu = d lat, d lv = d lat eps sqrt(v) / 2 where exp(lv) >= var_floor, else 0
//   d z = embed_net.3^T [d mu | d lv], d bn = d z LeakyReLU'(bn); BatchNorm backward (batch mode: the column sums of d bn and
//   d bn xhat over ALL rows of the call), d y -> embed_net.0.
//
// One wave owns the 16-row tile of G = 16 / N whole environments, as in the forward, and RECOMPUTES every intermediate from
// h, eps and the weights; nothing of N x N size is stored.  All cross-agent coupling is inside the tile.  Launches:
//   1, 2 (batch mode) the batch statistics of y = embed_net.0 h again - Chan merge in the forward's order - WITHOUT moving the
//        running statistics; eval mode: one small launch that writes the affine map of the running statistics
//   3    the pair kernel: forward recompute, the chain above down to d bn; row planes S, DU, d par, z, d key, d bn, xhat and the
//        dense d msg_net.2 rows; dh = msg_net.0[:, :64]^T DU + w_key^T d key; one partial per tile for what is no row product:
//        d msg_net.0[:, 64:], d b2, d w_query, d bq and the two BatchNorm column sums
//   4    the partials summed in a fixed order (slices of tiles, then the slices in sequence) and added into the gradients
//   5    d y from d bn (BatchNorm backward), dh += embed_net.0^T d y
//   6..  five marl_linear_wgrad reductions over the row planes: embed_net.0, embed_net.3, msg_net.0[:, :64], msg_net.2, w_key
// No float atomics anywhere: two calls give the same bits.  Everything is fp32.
#include "maic_common.h"

namespace {

using namespace maic;
using head_tile::drow;
using head_tile::tile_gemm_t;

// one tile's partial sums (floats): d msg_net.0[:, 64:] (64 x 8), d b2 (32), d w_query (32 x 8), d bq (32), sum d bn, sum d bn xhat
constexpr int PO_V = 0, PO_B2 = 512, PO_QW = 544, PO_QB = 800, PO_S1 = 832, PO_S2 = 896, PO_USED = 960, PO_STRIDE = 1024;
constexpr int MB_SLICES = MC_RED;    // slices of the partial merge, as many as the statistics merge has

struct BwdArgs {
  marl_maic_weights_t w;
  marl_maic_grads_t g;
  const float* h;                    // (R, 64)
  const float* eps;                  // (R, N L) or null (test mode)
  const int* u_act;                  // (R)
  const float* dq_val;               // (R)
  const float* extra;                // (R, 2 N L) or null: a further gradient on the post-clamp [mean | var] planes
  float* dh;                         // (R, 64)
  float *spart, *ss, *bnsum;         // statistics partials (mean | M2 per tile), scale | shift | mean | rstd, the two column sums
  float *S, *DU, *z, *dbn, *xh, *dy; // (R, 64) planes
  float *dkey, *dpar, *dm2;          // (R, 32), (R, 2 N L), (R, lda)
  float *part, *part2;               // per-tile partials, per-slice partials
  long R;
  int bs, N, A, G, test_mode, lda;
  float var_floor, bn_eps;
};

__device__ __forceinline__ int tile_rows(const BwdArgs& p, long row0) {
  const long left = p.R - row0;
  const int rw = p.G * p.N;
  return left < rw ? (int)left : rw;
}

// ---- launch 1 (batch mode): the tile's (mean, M2) per column of y = embed_net.0 h, as the forward's first launch
__global__ __launch_bounds__(64) void maic_bwd_stats_kernel(BwdArgs p) {
  __shared__ float sh_h[16 * MC_LDH], sh_y[16 * MC_LDH];
  const long row0 = (long)blockIdx.x * p.G * p.N;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  __syncthreads();
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const f32x4 acc = mc_gemm(sh_h, MC_LDH, MC_H, p.w.e0_w, MC_H, n0, MC_NH);
    const int c = n0 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_y[drow(r) * MC_LDH + c] = acc[r] + p.w.e0_b[c];
  }
  __syncthreads();
  float s = 0.0f;
  for (int r = 0; r < nv; ++r) s += sh_y[r * MC_LDH + l];
  const float mean = s / (float)nv;
  float m2 = 0.0f;
  for (int r = 0; r < nv; ++r) {
    const float d = sh_y[r * MC_LDH + l] - mean;
    m2 = fmaf(d, d, m2);
  }
  p.spart[(long)blockIdx.x * 128 + l] = mean;
  p.spart[(long)blockIdx.x * 128 + 64 + l] = m2;
}

// ---- launch 2: ss = scale | shift | mean | rstd per column.  batch: the merged statistics of launch 1 (the forward's order);
// otherwise the running statistics.  Nothing of the module's state is written.
__global__ __launch_bounds__(64 * MC_RED) void maic_bwd_bn_kernel(BwdArgs p, int nblk, int batch) {
  __shared__ float sh_n[MC_RED][64], sh_m[MC_RED][64], sh_v[MC_RED][64];
  const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
  float n = 0.0f, mean = 0.0f, m2 = 0.0f;
  if (batch) {
    const int rw = p.G * p.N;
    for (int b = s; b < nblk; b += MC_RED) {
      const long left = p.R - (long)b * rw;
      const float nb = (float)(left < rw ? left : rw);
      chan_merge(n, mean, m2, nb, p.spart[(long)b * 128 + c], p.spart[(long)b * 128 + 64 + c]);
    }
  }
  sh_n[s][c] = n; sh_m[s][c] = mean; sh_v[s][c] = m2;
  __syncthreads();
  if (s != 0) return;
  float var;
  if (batch) {
    for (int k = 1; k < MC_RED; ++k) chan_merge(n, mean, m2, sh_n[k][c], sh_m[k][c], sh_v[k][c]);
    var = m2 / n;
  } else {
    mean = p.w.bn_rm[c];
    var = p.w.bn_rv[c];
  }
  const float sd = sqrtf(var + p.bn_eps);
  const float scale = p.w.bn_w[c] / sd;
  p.ss[c] = scale;
  p.ss[64 + c] = p.w.bn_b[c] - mean * scale;
  p.ss[128 + c] = mean;
  p.ss[192 + c] = 1.0f / sd;
}

// ---- launch 3: the pair kernel
__global__ __launch_bounds__(64) void maic_bwd_pair_kernel(BwdArgs p) {
  __shared__ float sh_h[16 * MC_LDH];      // h; from the slot loop on: hid of the slot
  __shared__ float sh_z[16 * MC_LDH], sh_u[16 * MC_LDH];
  __shared__ float sh_dp[16 * MC_LDH];     // d pre of the slot; at the end: d bn
  __shared__ float sh_S[16 * MC_LDH];      // S; at the end: d bn xhat
  __shared__ float sh_DU[16 * MC_LDH];
  __shared__ float sh_lat[16 * MC_LDL], sh_dlat[16 * MC_LDL];
  __shared__ float sh_sd[16 * MC_LDL];     // d lat -> d lv factor eps sqrt(v) / 2 (0 under the clamp); then d lv itself
  __shared__ float sh_k[16 * MC_LDK], sh_dk[16 * MC_LDK];
  __shared__ float sh_kq[16 * MC_LDQ], sh_dkq[16 * MC_LDQ];
  __shared__ float sh_al[16 * MC_LDA];     // alpha after the gate
  __shared__ float sh_au[16 * MC_LDA];     // alpha before it
  __shared__ float sh_dot[16 * MC_LDA];    // d alpha, then d logit
  __shared__ float sh_val[16];
  __shared__ int sh_act[16];
  const marl_maic_weights_t& w = p.w;
  const int N = p.N, A = p.A, NL = p.N * MC_L, RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  float* part = p.part + (long)blockIdx.x * PO_STRIDE;
  if (l < 16) {
    int a = 0;
    float v = 0.0f;
    if (l < nv) {
      a = p.u_act[row0 + l];
      v = p.dq_val[row0 + l];
      if (a < 0 || a >= A) { a = 0; v = 0.0f; }
    }
    sh_act[l] = a;
    sh_val[l] = v;
  }
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  for (int idx = l; idx < 16 * MC_LDH; idx += 64) { sh_S[idx] = 0.0f; sh_DU[idx] = 0.0f; }
  for (int idx = l; idx < 16 * MC_LDL; idx += 64) { sh_dlat[idx] = 0.0f; sh_sd[idx] = 0.0f; }
  __syncthreads();
  // ---- forward again: z (and xhat), U, key
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const int c = n0 + m;
    f32x4 y = mc_gemm(sh_h, MC_LDH, MC_H, w.e0_w, MC_H, n0, MC_NH);
    const float scale = p.ss[c], shift = p.ss[64 + c], mean = p.ss[128 + c], rstd = p.ss[192 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = drow(r);
      const float yv = y[r] + w.e0_b[c];
      const float zv = leaky(fmaf(yv, scale, shift));
      sh_z[row * MC_LDH + c] = zv;
      if (row < nv) {
        p.z[(row0 + row) * MC_NH + c] = zv;
        p.xh[(row0 + row) * MC_NH + c] = (yv - mean) * rstd;
      }
    }
    const f32x4 u = mc_gemm(sh_h, MC_LDH, MC_H, w.m0_w, MC_M0, n0, MC_NH);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_u[drow(r) * MC_LDH + c] = u[r] + w.m0_b[c];
  }
  for (int n0 = 0; n0 < MC_D; n0 += 16) {
    const f32x4 k = mc_gemm(sh_h, MC_LDH, MC_H, w.k_w, MC_H, n0, MC_D);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_k[drow(r) * MC_LDK + n0 + m] = k[r] + w.k_b[n0 + m];
  }
  __syncthreads();
  // ---- latent, and the factor that turns d lat into d lv
  for (int n0 = 0; n0 < NL; n0 += 16) {
    const int c = n0 + m;
    const f32x4 mu = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w, MC_NH, n0, NL);
    f32x4 lat, sd = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) lat[r] = c < NL ? mu[r] + w.e3_b[c] : 0.0f;
    if (!p.test_mode || p.extra) {
      const f32x4 lv = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w + (long)NL * MC_NH, MC_NH, n0, NL);
      if (c < NL) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (drow(r) < nv) {
            const float ex = expf(lv[r] + w.e3_b[NL + c]);
            if (!p.test_mode) {
              const float sv = sqrtf(fmaxf(ex, p.var_floor));
              const float e = p.eps[(row0 + drow(r)) * NL + c];
              lat[r] = fmaf(sv, e, lat[r]);
              sd[r] = ex >= p.var_floor ? 0.5f * sv * e : 0.0f;
            }
            // d var -> d lv factor of the extra gradient (0 under the clamp), parked where d lv goes at the end
            if (p.extra) p.dpar[(row0 + drow(r)) * 2 * NL + NL + c] = ex >= p.var_floor ? ex : 0.0f;
          }
        }
      }
    }
    if (c < NL) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sh_lat[drow(r) * MC_LDL + c] = lat[r];
        sh_sd[drow(r) * MC_LDL + c] = sd[r];
      }
    }
  }
  for (int idx = l; idx < 16 * (MC_L + 1); idx += 64) {
    const int r = idx / (MC_L + 1), k = idx % (MC_L + 1);
    float s = 0.0f;
    for (int d = 0; d < MC_D; ++d) s = fmaf(sh_k[r * MC_LDK + d], k < MC_L ? w.q_w[d * MC_L + k] : w.q_b[d], s);
    sh_kq[r * MC_LDQ + k] = s;
  }
  __syncthreads();
  for (int idx = l; idx < 16 * N; idx += 64) {
    const int r = idx / N, j = idx % N;
    float s = sh_kq[r * MC_LDQ + MC_L];
#pragma unroll
    for (int k = 0; k < MC_L; ++k) s = fmaf(sh_kq[r * MC_LDQ + k], sh_lat[r * MC_LDL + j * MC_L + k], s);
    s *= MC_QSCALE;
    sh_au[r * MC_LDA + j] = (j == r % N) ? -1e9f : s;
  }
  __syncthreads();
  if (l < 16) {
    const int r = l;
    if (r < nv) {
      float mx = -3.0e38f;
      for (int j = 0; j < N; ++j) mx = fmaxf(mx, sh_au[r * MC_LDA + j]);
      float sum = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float e = expf(sh_au[r * MC_LDA + j] - mx);
        sh_au[r * MC_LDA + j] = e;
        sum += e;
      }
      const float thr = 0.25f / (float)N;
      for (int j = 0; j < N; ++j) {
        const float a = sh_au[r * MC_LDA + j] / sum;
        sh_au[r * MC_LDA + j] = a;
        sh_al[r * MC_LDA + j] = (p.test_mode && a < thr) ? 0.0f : a;
      }
    } else {
      for (int j = 0; j < N; ++j) { sh_au[r * MC_LDA + j] = 0.0f; sh_al[r * MC_LDA + j] = 0.0f; }
    }
  }
  __syncthreads();
  // ---- the pairs, slot by slot: lane n owns hidden unit n of msg_net.0 for the 16 senders of the tile
  float vk[MC_L], dV[MC_L];
#pragma unroll
  for (int k = 0; k < MC_L; ++k) {
    vk[k] = w.m0_w[(long)l * MC_M0 + MC_H + k];
    dV[k] = 0.0f;
  }
  for (int j = 0; j < N; ++j) {
    int e0 = 0, cnt = 0;                   // first row of the sender's environment
    for (int r = 0; r < 16; ++r) {
      if (cnt == N) { e0 += N; cnt = 0; }
      ++cnt;
      const int rj = r < RW ? e0 + j : 0;  // row of the receiver
      float lat[MC_L];
      float pre = sh_u[rj * MC_LDH + l];
#pragma unroll
      for (int k = 0; k < MC_L; ++k) {
        lat[k] = sh_lat[r * MC_LDL + j * MC_L + k];
        pre = fmaf(vk[k], lat[k], pre);
      }
      const float hid = leaky(pre);
      const float ag = sh_al[r * MC_LDA + j];            // 0 for rows that do not exist
      const float dp = ag * sh_val[rj] * w.m2_w[(long)sh_act[rj] * MC_NH + l] * (pre > 0.0f ? 1.0f : 0.01f);
      sh_h[r * MC_LDH + l] = hid;
      sh_dp[r * MC_LDH + l] = dp;
      sh_S[rj * MC_LDH + l] = fmaf(ag, hid, sh_S[rj * MC_LDH + l]);
      sh_DU[rj * MC_LDH + l] += dp;
#pragma unroll
      for (int k = 0; k < MC_L; ++k) dV[k] = fmaf(dp, lat[k], dV[k]);
    }
    __syncthreads();
    if (l < 16) {                          // d alpha[r][j] = v_j msg[r][j][a_j]
      const int r = l;
      const int rj = r < RW ? (r / N) * N + j : 0;
      const float* w2 = w.m2_w + (long)sh_act[rj] * MC_NH;
      float s = w.m2_b[sh_act[rj]];
      for (int n = 0; n < MC_NH; ++n) s = fmaf(w2[n], sh_h[r * MC_LDH + n], s);
      sh_dot[r * MC_LDA + j] = s * sh_val[rj];
    }
    {                                      // d lat[r][j] = msg_net.0[:, 64:]^T d pre[r][j]
      const f32x4 acc = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dp, MC_LDH, MC_NH, w.m0_w + MC_H, MC_M0, 0, MC_L);
      if (m < MC_L) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sh_dlat[drow(i) * MC_LDL + j * MC_L + m] = acc[i];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < MC_L; ++k) part[PO_V + l * MC_L + k] = dV[k];
  // ---- row planes of the msg_net reductions; d b2
  for (int idx = l; idx < 16 * MC_NH; idx += 64) {
    const int r = idx / MC_NH, c = idx % MC_NH;
    if (r < nv) {
      p.S[(row0 + r) * MC_NH + c] = sh_S[r * MC_LDH + c];
      p.DU[(row0 + r) * MC_NH + c] = sh_DU[r * MC_LDH + c];
    }
  }
  for (int idx = l; idx < 16 * p.lda; idx += 64) {
    const int r = idx / p.lda, c = idx % p.lda;
    if (r < nv) p.dm2[(row0 + r) * p.lda + c] = (c == sh_act[r]) ? sh_val[r] : 0.0f;
  }
  if (l < MC_AMAX) {
    float s = 0.0f;
    for (int r = 0; r < nv; ++r) {
      if (sh_act[r] != l) continue;
      const int e0 = (r / N) * N, j = r % N;
      float as = 0.0f;
      for (int i = 0; i < N; ++i) as += sh_al[(e0 + i) * MC_LDA + j];
      s = fmaf(sh_val[r], as, s);
    }
    part[PO_B2 + l] = s;
  }
  // ---- softmax backward
  if (l < 16) {
    const int r = l;
    const float thr = 0.25f / (float)N;
    float inner = 0.0f;
    for (int j = 0; j < N; ++j) {
      const float a = sh_au[r * MC_LDA + j];
      const float da = (p.test_mode && a < thr) ? 0.0f : sh_dot[r * MC_LDA + j];
      sh_dot[r * MC_LDA + j] = da;
      inner = fmaf(a, da, inner);
    }
    for (int j = 0; j < N; ++j) {
      const float dl = sh_au[r * MC_LDA + j] * (sh_dot[r * MC_LDA + j] - inner);
      sh_dot[r * MC_LDA + j] = (r < nv && j != r % N) ? dl : 0.0f;
    }
  }
  __syncthreads();
  // ---- d lat += the attention path; d kq
  for (int idx = l; idx < 16 * NL; idx += 64) {
    const int r = idx / NL, c = idx % NL;
    sh_dlat[r * MC_LDL + c] = fmaf(MC_QSCALE * sh_dot[r * MC_LDA + c / MC_L], sh_kq[r * MC_LDQ + c % MC_L], sh_dlat[r * MC_LDL + c]);
  }
  for (int idx = l; idx < 16 * (MC_L + 1); idx += 64) {
    const int r = idx / (MC_L + 1), k = idx % (MC_L + 1);
    float s = 0.0f;
    for (int j = 0; j < N; ++j) s = fmaf(sh_dot[r * MC_LDA + j], k < MC_L ? sh_lat[r * MC_LDL + j * MC_L + k] : 1.0f, s);
    sh_dkq[r * MC_LDQ + k] = MC_QSCALE * s;
  }
  __syncthreads();
  // ---- d key, d w_query, d bq; d par = [d mu | d lv]
  for (int idx = l; idx < 16 * MC_D; idx += 64) {
    const int r = idx / MC_D, d = idx % MC_D;
    float s = sh_dkq[r * MC_LDQ + MC_L] * w.q_b[d];
#pragma unroll
    for (int k = 0; k < MC_L; ++k) s = fmaf(sh_dkq[r * MC_LDQ + k], w.q_w[d * MC_L + k], s);
    sh_dk[r * MC_LDK + d] = s;
    if (r < nv) p.dkey[(row0 + r) * MC_D + d] = s;
  }
  for (int idx = l; idx < MC_D * MC_L; idx += 64) {
    const int d = idx / MC_L, k = idx % MC_L;
    float s = 0.0f;
    for (int r = 0; r < 16; ++r) s = fmaf(sh_k[r * MC_LDK + d], sh_dkq[r * MC_LDQ + k], s);
    part[PO_QW + idx] = s;
  }
  if (l < MC_D) {
    float s = 0.0f;
    for (int r = 0; r < 16; ++r) s = fmaf(sh_k[r * MC_LDK + l], sh_dkq[r * MC_LDQ + MC_L], s);
    part[PO_QB + l] = s;
  }
  for (int idx = l; idx < 16 * NL; idx += 64) {
    const int r = idx / NL, c = idx % NL;
    float dmu = sh_dlat[r * MC_LDL + c];
    float dlv = dmu * sh_sd[r * MC_LDL + c];
    if (p.extra && r < nv) {               // the extra planes join before the clamp gate: one embed_net backward for both
      const long g = (row0 + r) * 2 * NL + c;
      dlv = fmaf(p.extra[g + NL], p.dpar[g + NL], dlv);
      dmu += p.extra[g];
      sh_dlat[r * MC_LDL + c] = dmu;
    }
    sh_sd[r * MC_LDL + c] = dlv;
    if (r < nv) {
      p.dpar[(row0 + r) * 2 * NL + c] = dmu;
      p.dpar[(row0 + r) * 2 * NL + NL + c] = dlv;
    }
  }
  __syncthreads();
  // ---- d bn = (embed_net.3^T d par) LeakyReLU'(bn); dh = msg_net.0[:, :64]^T DU + w_key^T d key
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const int c = n0 + m;
    f32x4 dz = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dlat, MC_LDL, NL, w.e3_w, MC_NH, n0, MC_NH);
    if (!p.test_mode || p.extra) dz = tile_gemm_t(dz, sh_sd, MC_LDL, NL, w.e3_w + (long)NL * MC_NH, MC_NH, n0, MC_NH);
    f32x4 dh = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_DU, MC_LDH, MC_NH, w.m0_w, MC_M0, n0, MC_H);
    dh = tile_gemm_t(dh, sh_dk, MC_LDK, MC_D, w.k_w, MC_H, n0, MC_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = drow(r);
      const float dbn = dz[r] * (sh_z[row * MC_LDH + c] > 0.0f ? 1.0f : 0.01f);
      float xh = 0.0f;
      if (row < nv) {
        xh = p.xh[(row0 + row) * MC_NH + c];         // this thread's own store above
        p.dbn[(row0 + row) * MC_NH + c] = dbn;
        p.dh[(row0 + row) * MC_H + c] = dh[r];
      }
      sh_dp[row * MC_LDH + c] = dbn;
      sh_S[row * MC_LDH + c] = dbn * xh;
    }
  }
  __syncthreads();
  float s1 = 0.0f, s2 = 0.0f;
  for (int r = 0; r < nv; ++r) {
    s1 += sh_dp[r * MC_LDH + l];
    s2 += sh_S[r * MC_LDH + l];
  }
  part[PO_S1 + l] = s1;
  part[PO_S2 + l] = s2;
}

// ---- launch 4a (more than MB_SLICES tiles): slice s sums the partials of tiles s, s + MB_SLICES, ..
__global__ __launch_bounds__(256) void maic_bwd_slice_kernel(const float* __restrict__ in, int n, float* out) {
  const int s = blockIdx.x;
  for (int c = threadIdx.x; c < PO_USED; c += 256) {
    float a = 0.0f;
    for (int b = s; b < n; b += MB_SLICES) a += in[(long)b * PO_STRIDE + c];
    out[(long)s * PO_STRIDE + c] = a;
  }
}

// ---- launch 4b: rows 0 .. n-1 of `in` summed in sequence and added into the gradients; the BatchNorm sums also go to bnsum
__global__ __launch_bounds__(1024) void maic_bwd_apply_kernel(BwdArgs p, const float* __restrict__ in, int n) {
  const int c = threadIdx.x;
  if (c >= PO_USED) return;
  float a = 0.0f;
  for (int b = 0; b < n; ++b) a += in[(long)b * PO_STRIDE + c];
  if (c < PO_B2) {
    p.g.m0_w[(long)(c / MC_L) * MC_M0 + MC_H + c % MC_L] += a;
  } else if (c < PO_QW) {
    if (c - PO_B2 < p.A) p.g.m2_b[c - PO_B2] += a;
  } else if (c < PO_QB) {
    p.g.q_w[c - PO_QW] += a;
  } else if (c < PO_S1) {
    p.g.q_b[c - PO_QB] += a;
  } else if (c < PO_S2) {
    p.g.bn_b[c - PO_S1] += a;
    p.bnsum[c - PO_S1] = a;
  } else {
    p.g.bn_w[c - PO_S2] += a;
    p.bnsum[64 + c - PO_S2] = a;
  }
}

// ---- launch 5: d y = scale (d bn - mean(d bn) - xhat mean(d bn xhat)) in batch mode, scale d bn otherwise; dh += embed_net.0^T d y
__global__ __launch_bounds__(64) void maic_bwd_embed_kernel(BwdArgs p, int batch) {
  __shared__ float sh_dy[16 * MC_LDH];
  const int RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  const float invR = 1.0f / (float)p.R;
  for (int idx = l; idx < 16 * MC_NH; idx += 64) {
    const int r = idx / MC_NH, c = idx % MC_NH;
    float v = 0.0f;
    if (r < nv) {
      const long g = (row0 + r) * MC_NH + c;
      float d = p.dbn[g];
      if (batch) d = d - p.bnsum[c] * invR - p.xh[g] * (p.bnsum[64 + c] * invR);
      v = p.ss[c] * d;
      p.dy[g] = v;
    }
    sh_dy[r * MC_LDH + c] = v;
  }
  __syncthreads();
  for (int n0 = 0; n0 < MC_H; n0 += 16) {
    const f32x4 acc = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dy, MC_LDH, MC_NH, p.w.e0_w, MC_H, n0, MC_H);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (drow(r) < nv) p.dh[(row0 + drow(r)) * MC_H + n0 + m] += acc[r];
  }
}

bool maic_grads_ok(const marl_maic_grads_t* g) {
  float* ps[] = {g->e0_w, g->e0_b, g->bn_w, g->bn_b, g->e3_w, g->e3_b, g->m0_w, g->m0_b, g->m2_w, g->m2_b, g->k_w, g->k_b,
                 g->q_w, g->q_b};
  for (float* q : ps)
    if (!q) return false;
  return true;
}

struct BwdLayout {
  long S, DU, z, dbn, xh, dy, dkey, dpar, dm2, spart, ss, bnsum, part, part2, wg, total;     // float offsets
  int nblk, lda;
};

BwdLayout bwd_layout(int bs, int N, int A) {
  BwdLayout L;
  const long R = (long)bs * N;
  const int G = mc_envs_per_tile(N);
  L.nblk = (bs + G - 1) / G;
  L.lda = head_tile::round4(A);
  const long p64 = head_tile::pad64(R * MC_NH);
  L.S = 0; L.DU = p64; L.z = 2 * p64; L.dbn = 3 * p64; L.xh = 4 * p64; L.dy = 5 * p64;
  L.dkey = 6 * p64;
  L.dpar = L.dkey + head_tile::pad64(R * MC_D);
  L.dm2 = L.dpar + head_tile::pad64(R * 2 * N * MC_L);
  L.spart = L.dm2 + head_tile::pad64(R * L.lda);
  L.ss = L.spart + (long)L.nblk * 128;
  L.bnsum = L.ss + 256;
  L.part = L.bnsum + 128;
  L.part2 = L.part + (long)L.nblk * PO_STRIDE;
  L.wg = L.part2 + (long)MB_SLICES * PO_STRIDE;
  size_t wg = 0;
  const int M = R > 0x7fffffff ? 0x7fffffff : (int)R;
  const size_t cand[] = {marl_linear_wgrad_workspace(M, MC_NH, MC_H, 1), marl_linear_wgrad_workspace(M, 2 * N * MC_L, MC_NH, 1),
                         marl_linear_wgrad_workspace(M, A, MC_NH, 1), marl_linear_wgrad_workspace(M, MC_D, MC_H, 1)};
  for (size_t c : cand) wg = c > wg ? c : wg;
  L.total = L.wg + (long)((wg + 3) / 4);
  return L;
}

marl_src_t dense_src(const float* x, long ld, int k) {
  marl_src_t s{};
  s.p0 = x; s.ld0 = ld; s.k0 = k;
  return s;
}

}  // namespace

extern "C" size_t marl_maic_bwd_workspace(int bs, int N, int A) {
  if (bs < 0 || N < 1 || N > MC_NMAX || A < 1 || A > MC_AMAX) return 0;
  return (size_t)bwd_layout(bs, N, A).total * sizeof(float);
}

extern "C" int marl_maic_head_bwd(const marl_maic_weights_t* w, const marl_maic_grads_t* g, const float* h, const float* eps,
                                  const int* u_act, const float* dq_val, float* dh, float* ws, size_t ws_bytes, int bs, int N,
                                  int A, int test_mode, int bn_batch, float var_floor, float bn_eps, void* stream) {
  return marl_maic_head_bwd_ex(w, g, h, eps, u_act, dq_val, nullptr, dh, ws, ws_bytes, bs, N, A, test_mode, bn_batch, var_floor,
                               bn_eps, stream);
}

extern "C" int marl_maic_head_bwd_ex(const marl_maic_weights_t* w, const marl_maic_grads_t* g, const float* h, const float* eps,
                                     const int* u_act, const float* dq_val, const float* dpar_extra, float* dh, float* ws,
                                     size_t ws_bytes, int bs, int N, int A, int test_mode, int bn_batch, float var_floor,
                                     float bn_eps, void* stream) {
  if (!w || !maic_weights_ok(w) || !g || !maic_grads_ok(g) || !h || !u_act || !dq_val || !dh || !ws || bs < 0 ||
      !marl_maic_supported(N, 1, A, MC_H, MC_NH, MC_L, MC_D))
    return (int)hipErrorInvalidValue;
  if (!test_mode && !eps) return (int)hipErrorInvalidValue;
  const long R = (long)bs * N;
  if (R == 0) return 0;
  if (R > 0x7fffffffL || (bn_batch && R < 2) || ws_bytes < marl_maic_bwd_workspace(bs, N, A)) return (int)hipErrorInvalidValue;
  const BwdLayout L = bwd_layout(bs, N, A);
  BwdArgs a{};
  a.w = *w; a.g = *g;
  a.h = h; a.eps = test_mode ? nullptr : eps; a.u_act = u_act; a.dq_val = dq_val; a.extra = dpar_extra; a.dh = dh;
  a.spart = ws + L.spart; a.ss = ws + L.ss; a.bnsum = ws + L.bnsum;
  a.S = ws + L.S; a.DU = ws + L.DU; a.z = ws + L.z; a.dbn = ws + L.dbn; a.xh = ws + L.xh; a.dy = ws + L.dy;
  a.dkey = ws + L.dkey; a.dpar = ws + L.dpar; a.dm2 = ws + L.dm2;
  a.part = ws + L.part; a.part2 = ws + L.part2;
  a.R = R; a.bs = bs; a.N = N; a.A = A; a.G = mc_envs_per_tile(N); a.test_mode = test_mode ? 1 : 0; a.lda = L.lda;
  a.var_floor = var_floor; a.bn_eps = bn_eps;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nblk);
  const int batch = bn_batch ? 1 : 0;
  if (batch) {
    hipLaunchKernelGGL(maic_bwd_stats_kernel, grid, dim3(64), 0, s, a);
    MARL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(maic_bwd_bn_kernel, dim3(1), dim3(64 * MC_RED), 0, s, a, L.nblk, batch);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maic_bwd_pair_kernel, grid, dim3(64), 0, s, a);
  MARL_CHECK_LAUNCH();
  if (L.nblk > MB_SLICES) {
    hipLaunchKernelGGL(maic_bwd_slice_kernel, dim3(MB_SLICES), dim3(256), 0, s, (const float*)a.part, L.nblk, a.part2);
    MARL_CHECK_LAUNCH();
    hipLaunchKernelGGL(maic_bwd_apply_kernel, dim3(1), dim3(1024), 0, s, a, (const float*)a.part2, MB_SLICES);
  } else {
    hipLaunchKernelGGL(maic_bwd_apply_kernel, dim3(1), dim3(1024), 0, s, a, (const float*)a.part, L.nblk);
  }
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maic_bwd_embed_kernel, grid, dim3(64), 0, s, a, batch);
  MARL_CHECK_LAUNCH();
  float* wg = ws + L.wg;
  const size_t wg_bytes = ws_bytes - (size_t)L.wg * sizeof(float);
  const int M = (int)R, NP = 2 * N * MC_L;
  marl_src_t xh = dense_src(h, MC_H, MC_H), xz = dense_src(a.z, MC_NH, MC_NH), xs = dense_src(a.S, MC_NH, MC_NH);
  int e;
  // embed_net.0: dW += d y^T h ; embed_net.3: dW += d par^T z
  if ((e = marl_linear_wgrad(a.dy, MC_NH, nullptr, 0, &xh, g->e0_w, MC_H, g->e0_b, M, MC_NH, MC_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  if ((e = marl_linear_wgrad(a.dpar, NP, nullptr, 0, &xz, g->e3_w, MC_NH, g->e3_b, M, NP, MC_NH, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  // msg_net.0[:, :64]: dW += DU^T h (the latent columns came from the partials) ; msg_net.2: dW += d msg^T S (its bias too)
  if ((e = marl_linear_wgrad(a.DU, MC_NH, nullptr, 0, &xh, g->m0_w, MC_M0, g->m0_b, M, MC_NH, MC_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  if ((e = marl_linear_wgrad(a.dm2, a.lda, nullptr, 0, &xs, g->m2_w, MC_NH, nullptr, M, A, MC_NH, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  // w_key: dW += d key^T h
  if ((e = marl_linear_wgrad(a.dkey, MC_D, nullptr, 0, &xh, g->k_w, MC_H, g->k_b, M, MC_D, MC_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  return 0;
}
