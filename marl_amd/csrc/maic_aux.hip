// The MAIC agent's two auxiliary losses (reference network/MAIC.py:88-123) on gfx950, values and gradients in one call - the
// values are only ever wanted with their gradients.  Notation of maic_head.hip: senders i, receivers j of one environment,
// pair row (b*N + i)*N + j.
//
//   MI (calculate_action_mi_loss): g1 = Normal(mean[i][j], sqrt(var[i][j])) from embed_net (var = max(exp(.), var_floor)),
//     a_j = argmax return_q[j] (lowest index on a tie, no mask, not differentiated), u[i][j] = W0[:, :64] h_i + W0[:, 64 + a_j] + b0,
//     out[i][j] = inference_net.3 LeakyReLU(BatchNorm(u[i][j])) - BatchNorm over ALL bs*N*N pair rows, diagonal included -,
//     g2 = Normal(out[:8], sqrt(max(exp(out[8:]), var_floor))), mi = mi_w * mean_pairs sum_L KL(g1 || g2),
//     KL = log(s2 / s1) + (v1 + (m1 - m2)^2) / (2 v2) - 1/2.
//   Entropy: key = w_key h_i, query = w_query lat[i][j] (h and lat as constants), alpha = softmax_j(key . query) - no 1/sqrt(D), no
//     diagonal mask -, ent = ent_w * mean_rows -sum_j a' log2 a' with a' = max(alpha, 1e-4).
//
// The first layer of inference_net is NOT done pair by pair: P = W0[:, :64] h + b0 is one 16-row MFMA product per tile and the
// action part a column lookup; BatchNorm and what follows are per pair (slot by slot, lane n owns hidden unit n, as the head's
// pair loop).  One wave owns the 16-row tile of G = 16 / N whole environments.  Launches:
//   1, 2  the statistics of BOTH BatchNorms (embed_net.1 over the rows, inference_net.1 over the pairs): per-tile (mean, M2), Chan
//         merge in a fixed order.  Only here do inference_net.1's running statistics move (batch mode, mi_w > 0 - the reference
//         evaluates inference_net only then); embed_net.1's buffers are never written.  Eval mode: launch 2 alone writes the
//         affine maps of the running statistics.
//   3     the loss kernel: both losses, d(mean, var) of the MI term (the plane marl_maic_head_bwd_ex adds to its own), d out per
//         pair (16 floats), the entropy term's d key rows; one partial per tile: d inference_net.3, the two BatchNorm column sums,
//         d w_query, the two loss sums
//   4     the partials summed in a fixed order (slices of tiles, then the slices in sequence) and added into the gradients / losses
//   5     the BatchNorm backward of inference_net.1 with the merged column sums, d P = sum_j d u[.][j] rows, dh = W0[:, :64]^T d P;
//         one partial per tile: d W0[:, 64:] (per action)
//   6     those partials, as 4
//   7, 8  marl_linear_wgrad: inference_net.0[:, :64] (and its bias) from d P, w_key from d key
// No float atomics: two calls give the same bits.  Everything is fp32.
#include "maic_common.h"

namespace {

using namespace maic;
using head_tile::drow;
using head_tile::tile_gemm_t;

constexpr int MC_O = 2 * MC_L;       // outputs of inference_net.3
constexpr int MC_LDO = MC_O + 4;
constexpr float ALPHA_FLOOR = 1e-4f;
// one tile's partial sums (floats): d inference_net.3 (16 x 64), its bias (16), sum d bn, sum d bn xhat, d w_query (32 x 8), d bq (32),
// the KL sum, the entropy sum; d inference_net.0[:, 64 + a] as [a][n]
constexpr int PO_W3 = 0, PO_B3 = 1024, PO_S1 = 1040, PO_S2 = 1104, PO_QW = 1168, PO_QB = 1424, PO_MI = 1456, PO_ENT = 1457,
              PO_WA = 1472, PO_STRIDE = PO_WA + MC_AMAX * MC_NH;
constexpr int MB_SLICES = MC_RED;
constexpr int SP = 256;              // statistics partial of a tile: embed mean | M2 | inference mean | M2

struct AuxArgs {
  marl_maic_weights_t w;
  marl_maic_infer_t iw;
  marl_maic_grads_t g;               // only w_key and w_query receive a gradient
  marl_maic_infer_grads_t ig;
  const float *h, *eps, *q;          // (R, 64), (R, N L) or null (test mode), (R, A)
  const float* den;                  // gradient pre-scale den[0] * dscale (null: dscale alone)
  float *mi_out, *ent_out;
  float *dpar, *dh;                  // (R, 2 N L), (R, 64)
  float *spart, *ss, *bnsum;         // statistics partials, scale | shift | mean | rstd of both BatchNorms, the two column sums
  float *dout, *dP, *dkey;           // (R N, 16), (R, 64), (R, 32)
  float *part, *part2;
  long R;
  int bs, N, A, G, test_mode, move_stats;
  float mi_w, ent_w, dscale, var_floor, bn_eps, bn_mom;
};

__device__ __forceinline__ int tile_rows(const AuxArgs& p, long row0) {
  const long left = p.R - row0;
  const int rw = p.G * p.N;
  return left < rw ? (int)left : rw;
}

// greedy action of each row of the tile by return_q: the lowest index wins a tie; rows that do not exist read as action 0
__device__ __forceinline__ void load_actions(const AuxArgs& p, long row0, int nv, int* sh_act) {
  const int l = threadIdx.x;
  if (l >= 16) return;
  int a = 0;
  if (l < nv) {
    const float* q = p.q + (row0 + l) * p.A;
    float best = q[0];
    for (int c = 1; c < p.A; ++c)
      if (q[c] > best) { best = q[c]; a = c; }
  }
  sh_act[l] = a;
}

// sh_wa[a][n] = inference_net.0[n, 64 + a]
__device__ __forceinline__ void stage_wa(const AuxArgs& p, float* sh_wa) {
  for (int idx = threadIdx.x; idx < p.A * MC_NH; idx += 64)
    sh_wa[idx] = p.iw.i0_w[(long)(idx % MC_NH) * (MC_H + p.A) + MC_H + idx / MC_NH];
}

// sh_P = inference_net.0[:, :64] h + b0 for the 16 rows of the tile
__device__ __forceinline__ void infer_rows(const AuxArgs& p, const float* sh_h, float* sh_P) {
  const int m = threadIdx.x & 15;
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const f32x4 acc = mc_gemm(sh_h, MC_LDH, MC_H, p.iw.i0_w, MC_H + p.A, n0, MC_NH);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_P[drow(r) * MC_LDH + n0 + m] = acc[r] + p.iw.i0_b[n0 + m];
  }
}

// row of the receiver of slot j for sender row r (first row of r's environment + j); rows past the tile's environments: 0
__device__ __forceinline__ int recv_row(int r, int j, int N, int RW) { return r < RW ? (r / N) * N + j : 0; }

// ---- launch 1 (batch mode): the tile's (mean, M2) per column of y = embed_net.0 h over its rows and of u over its pairs
__global__ __launch_bounds__(64) void aux_stats_kernel(AuxArgs p) {
  __shared__ float sh_h[16 * MC_LDH], sh_y[16 * MC_LDH], sh_wa[MC_AMAX * MC_NH];
  __shared__ int sh_act[16];
  const int N = p.N, RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  float* out = p.spart + (long)blockIdx.x * SP;
  load_actions(p, row0, nv, sh_act);
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  stage_wa(p, sh_wa);
  __syncthreads();
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const f32x4 acc = mc_gemm(sh_h, MC_LDH, MC_H, p.w.e0_w, MC_H, n0, MC_NH);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_y[drow(r) * MC_LDH + n0 + m] = acc[r] + p.w.e0_b[n0 + m];
  }
  __syncthreads();
  {
    float s = 0.0f;
    for (int r = 0; r < nv; ++r) s += sh_y[r * MC_LDH + l];
    const float mean = s / (float)nv;
    float m2 = 0.0f;
    for (int r = 0; r < nv; ++r) {
      const float d = sh_y[r * MC_LDH + l] - mean;
      m2 = fmaf(d, d, m2);
    }
    out[l] = mean;
    out[64 + l] = m2;
  }
  __syncthreads();
  infer_rows(p, sh_h, sh_y);
  __syncthreads();
  float s = 0.0f;
  for (int r = 0; r < nv; ++r)
    for (int j = 0; j < N; ++j) s += sh_y[r * MC_LDH + l] + sh_wa[sh_act[recv_row(r, j, N, RW)] * MC_NH + l];
  const float mean = s / (float)(nv * N);
  float m2 = 0.0f;
  for (int r = 0; r < nv; ++r)
    for (int j = 0; j < N; ++j) {
      const float d = sh_y[r * MC_LDH + l] + sh_wa[sh_act[recv_row(r, j, N, RW)] * MC_NH + l] - mean;
      m2 = fmaf(d, d, m2);
    }
  out[128 + l] = mean;
  out[192 + l] = m2;
}

// ---- launch 2: ss[net] = scale | shift | mean | rstd per column, net 0 = embed_net.1, net 1 = inference_net.1.  batch: the merged
// statistics of launch 1, and inference_net.1's running statistics move (move_stats); otherwise the running statistics
__global__ __launch_bounds__(64 * MC_RED) void aux_bn_kernel(AuxArgs p, int nblk, int batch) {
  __shared__ float sh_n[MC_RED][64], sh_m[MC_RED][64], sh_v[MC_RED][64];
  const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
  for (int net = 0; net < 2; ++net) {
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    if (batch) {
      const int rw = p.G * p.N;
      for (int b = s; b < nblk; b += MC_RED) {
        const long left = p.R - (long)b * rw;
        const float rows = (float)(left < rw ? left : rw);
        const float* sp = p.spart + (long)b * SP + net * 128;
        chan_merge(n, mean, m2, net ? rows * (float)p.N : rows, sp[c], sp[64 + c]);
      }
    }
    sh_n[s][c] = n; sh_m[s][c] = mean; sh_v[s][c] = m2;
    __syncthreads();
    if (s == 0) {
      float* rm = net ? p.iw.ibn_rm : p.w.bn_rm;
      float* rv = net ? p.iw.ibn_rv : p.w.bn_rv;
      float var;
      if (batch) {
        for (int k = 1; k < MC_RED; ++k) chan_merge(n, mean, m2, sh_n[k][c], sh_m[k][c], sh_v[k][c]);
        var = m2 / n;
        if (net && p.move_stats) {
          rm[c] = (1.0f - p.bn_mom) * rm[c] + p.bn_mom * mean;
          rv[c] = (1.0f - p.bn_mom) * rv[c] + p.bn_mom * (m2 / (n - 1.0f));
          if (c == 0 && p.iw.ibn_nbt) p.iw.ibn_nbt[0] += 1;
        }
      } else {
        mean = rm[c];
        var = rv[c];
      }
      const float sd = sqrtf(var + p.bn_eps);
      const float scale = (net ? p.iw.ibn_w : p.w.bn_w)[c] / sd;
      float* ss = p.ss + net * 256;
      ss[c] = scale;
      ss[64 + c] = (net ? p.iw.ibn_b : p.w.bn_b)[c] - mean * scale;
      ss[128 + c] = mean;
      ss[192 + c] = 1.0f / sd;
    }
    __syncthreads();
  }
}

// the slot's inference hidden layer for lane n = hidden unit n and the 16 sender rows: sh_a1 = LeakyReLU(bn), sh_xh = xhat
__device__ __forceinline__ void infer_slot(const AuxArgs& p, int j, const float* sh_P, const float* sh_wa, const int* sh_act,
                                           float* sh_a1, float* sh_xh) {
  const int l = threadIdx.x, N = p.N, RW = p.G * p.N;
  const float* ss = p.ss + 256;
  const float scale = ss[l], shift = ss[64 + l], mean = ss[128 + l], rstd = ss[192 + l];
  for (int r = 0; r < 16; ++r) {
    const float u = sh_P[r * MC_LDH + l] + sh_wa[sh_act[recv_row(r, j, N, RW)] * MC_NH + l];
    sh_a1[r * MC_LDH + l] = leaky(fmaf(u, scale, shift));
    sh_xh[r * MC_LDH + l] = (u - mean) * rstd;
  }
}

// ---- launch 3: the loss kernel
__global__ __launch_bounds__(64) void aux_loss_kernel(AuxArgs p) {
  __shared__ float sh_h[16 * MC_LDH];      // h; from the slot loop on: a1 of the slot
  __shared__ float sh_z[16 * MC_LDH];      // z of embed_net; from the slot loop on: xhat of the slot
  __shared__ float sh_P[16 * MC_LDH];
  __shared__ float sh_mean[16 * MC_LDL], sh_var[16 * MC_LDL], sh_lat[16 * MC_LDL];
  __shared__ float sh_wa[MC_AMAX * MC_NH];
  __shared__ float sh_out[16 * MC_LDO], sh_dout[16 * MC_LDO];
  __shared__ float sh_k[16 * MC_LDK], sh_kq[16 * MC_LDQ], sh_dkq[16 * MC_LDQ];
  __shared__ float sh_al[16 * MC_LDA], sh_dl[16 * MC_LDA];
  __shared__ float sh_red[2 * 4 * 64];
  __shared__ float sh_ent[16];
  __shared__ int sh_act[16];
  const marl_maic_weights_t& w = p.w;
  const int N = p.N, NL = p.N * MC_L, RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  float* part = p.part + (long)blockIdx.x * PO_STRIDE;
  const float gs = (p.den ? p.den[0] : 1.0f) * p.dscale;
  const float cm = p.mi_w / ((float)p.R * (float)N) * gs, ce = p.ent_w / (float)p.R * gs;
  load_actions(p, row0, nv, sh_act);
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  stage_wa(p, sh_wa);
  __syncthreads();
  // ---- z of embed_net, P of inference_net, key
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const int c = n0 + m;
    const f32x4 y = mc_gemm(sh_h, MC_LDH, MC_H, w.e0_w, MC_H, n0, MC_NH);
    const float scale = p.ss[c], shift = p.ss[64 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_z[drow(r) * MC_LDH + c] = leaky(fmaf(y[r] + w.e0_b[c], scale, shift));
  }
  infer_rows(p, sh_h, sh_P);
  for (int n0 = 0; n0 < MC_D; n0 += 16) {
    const f32x4 k = mc_gemm(sh_h, MC_LDH, MC_H, w.k_w, MC_H, n0, MC_D);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_k[drow(r) * MC_LDK + n0 + m] = k[r] + w.k_b[n0 + m];
  }
  __syncthreads();
  // ---- mean | var | latent (rows that do not exist: a unit Gaussian, never used)
  for (int n0 = 0; n0 < NL; n0 += 16) {
    const int c = n0 + m;
    const f32x4 mu = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w, MC_NH, n0, NL);
    const f32x4 lv = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w + (long)NL * MC_NH, MC_NH, n0, NL);
    if (c < NL) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = drow(r);
        float mean = 0.0f, var = 1.0f, lat = 0.0f;
        if (row < nv) {
          mean = mu[r] + w.e3_b[c];
          var = fmaxf(expf(lv[r] + w.e3_b[NL + c]), p.var_floor);
          lat = p.test_mode ? mean : fmaf(sqrtf(var), p.eps[(row0 + row) * NL + c], mean);
        }
        sh_mean[row * MC_LDL + c] = mean;
        sh_var[row * MC_LDL + c] = var;
        sh_lat[row * MC_LDL + c] = lat;
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
  // ---- the entropy term: its own logits (no scale, no diagonal mask), softmax, clamp; d logit
  if (l < 16) {
    const int r = l;
    float ent = 0.0f;
    if (r < nv) {
      float mx = -3.0e38f;
      for (int j = 0; j < N; ++j) {
        float s = sh_kq[r * MC_LDQ + MC_L];
#pragma unroll
        for (int k = 0; k < MC_L; ++k) s = fmaf(sh_kq[r * MC_LDQ + k], sh_lat[r * MC_LDL + j * MC_L + k], s);
        sh_al[r * MC_LDA + j] = s;
        mx = fmaxf(mx, s);
      }
      float sum = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float e = expf(sh_al[r * MC_LDA + j] - mx);
        sh_al[r * MC_LDA + j] = e;
        sum += e;
      }
      float inner = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float a = sh_al[r * MC_LDA + j] / sum;
        const float lg = log2f(fmaxf(a, ALPHA_FLOOR));
        ent = fmaf(-fmaxf(a, ALPHA_FLOOR), lg, ent);
        const float da = a >= ALPHA_FLOOR ? -(lg + 1.4426950408889634f) : 0.0f;
        sh_al[r * MC_LDA + j] = a;
        sh_dl[r * MC_LDA + j] = da;
        inner = fmaf(a, da, inner);
      }
      for (int j = 0; j < N; ++j) sh_dl[r * MC_LDA + j] = ce * sh_al[r * MC_LDA + j] * (sh_dl[r * MC_LDA + j] - inner);
    } else {
      for (int j = 0; j < N; ++j) sh_dl[r * MC_LDA + j] = 0.0f;
    }
    sh_ent[r] = ent;
  }
  __syncthreads();
  for (int idx = l; idx < 16 * (MC_L + 1); idx += 64) {
    const int r = idx / (MC_L + 1), k = idx % (MC_L + 1);
    float s = 0.0f;
    for (int j = 0; j < N; ++j) s = fmaf(sh_dl[r * MC_LDA + j], k < MC_L ? sh_lat[r * MC_LDL + j * MC_L + k] : 1.0f, s);
    sh_dkq[r * MC_LDQ + k] = s;
  }
  __syncthreads();
  for (int idx = l; idx < 16 * MC_D; idx += 64) {
    const int r = idx / MC_D, d = idx % MC_D;
    float s = sh_dkq[r * MC_LDQ + MC_L] * w.q_b[d];
#pragma unroll
    for (int k = 0; k < MC_L; ++k) s = fmaf(sh_dkq[r * MC_LDQ + k], w.q_w[d * MC_L + k], s);
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
  __syncthreads();
  // ---- the pairs, slot by slot
  float dW3[MC_O], db3 = 0.0f, kl = 0.0f, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
  for (int o = 0; o < MC_O; ++o) dW3[o] = 0.0f;
  for (int j = 0; j < N; ++j) {
    infer_slot(p, j, sh_P, sh_wa, sh_act, sh_h, sh_z);
    __syncthreads();
    {
      const f32x4 acc = mc_gemm(sh_h, MC_LDH, MC_NH, p.iw.i3_w, MC_NH, 0, MC_O);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_out[drow(r) * MC_LDO + m] = acc[r] + p.iw.i3_b[m];
    }
    __syncthreads();
    for (int idx = l; idx < 16 * MC_L; idx += 64) {
      const int r = idx / MC_L, k = idx % MC_L;
      float dm2 = 0.0f, dlv2 = 0.0f;
      if (r < nv) {
        const float m1 = sh_mean[r * MC_LDL + j * MC_L + k], v1 = sh_var[r * MC_LDL + j * MC_L + k];
        const float ex = expf(sh_out[r * MC_LDO + MC_L + k]);
        const float v2 = fmaxf(ex, p.var_floor), d = m1 - sh_out[r * MC_LDO + k];
        const float q = fmaf(d, d, v1), iv2 = 1.0f / v2;
        kl += 0.5f * (logf(v2) - logf(v1)) + 0.5f * q * iv2 - 0.5f;
        const float dm1 = cm * d * iv2;
        dm2 = -dm1;
        dlv2 = ex >= p.var_floor ? cm * 0.5f * iv2 * (1.0f - q * iv2) * ex : 0.0f;
        const long g = (row0 + r) * 2 * NL + j * MC_L + k;
        p.dpar[g] = dm1;
        p.dpar[g + NL] = cm * 0.5f * (iv2 - 1.0f / v1);
        float* dout = p.dout + ((row0 + r) * N + j) * MC_O;
        dout[k] = dm2;
        dout[MC_L + k] = dlv2;
      }
      sh_dout[r * MC_LDO + k] = dm2;
      sh_dout[r * MC_LDO + MC_L + k] = dlv2;
    }
    __syncthreads();
    // d inference_net.3 (lane n: column n), its bias (lanes < 16)
#pragma unroll
    for (int o = 0; o < MC_O; ++o)
      for (int r = 0; r < 16; ++r) dW3[o] = fmaf(sh_dout[r * MC_LDO + o], sh_h[r * MC_LDH + l], dW3[o]);
    if (l < MC_O)
      for (int r = 0; r < 16; ++r) db3 += sh_dout[r * MC_LDO + l];
    // d bn = (inference_net.3^T d out) LeakyReLU'(bn): its two column sums
    for (int n0 = 0; n0 < MC_NH; n0 += 16) {
      const f32x4 da = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dout, MC_LDO, MC_O, p.iw.i3_w, MC_NH, n0, MC_NH);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = drow(r) * MC_LDH + n0 + m;
        const float dbn = da[r] * (sh_h[at] > 0.0f ? 1.0f : 0.01f);
        s1[n0 >> 4] += dbn;
        s2[n0 >> 4] = fmaf(dbn, sh_z[at], s2[n0 >> 4]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int o = 0; o < MC_O; ++o) part[PO_W3 + o * MC_NH + l] = dW3[o];
  if (l < MC_O) part[PO_B3 + l] = db3;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    sh_red[(l >> 4) * 64 + b * 16 + m] = s1[b];
    sh_red[256 + (l >> 4) * 64 + b * 16 + m] = s2[b];
  }
  __syncthreads();
  part[PO_S1 + l] = (sh_red[l] + sh_red[64 + l]) + (sh_red[128 + l] + sh_red[192 + l]);
  part[PO_S2 + l] = (sh_red[256 + l] + sh_red[320 + l]) + (sh_red[384 + l] + sh_red[448 + l]);
  __syncthreads();
  sh_red[l] = kl;
  __syncthreads();
  if (l == 0) {
    float s = 0.0f;
    for (int i = 0; i < 64; ++i) s += sh_red[i];
    part[PO_MI] = s;
    float e = 0.0f;
    for (int r = 0; r < 16; ++r) e += sh_ent[r];
    part[PO_ENT] = e;
  }
}

// ---- launch 5: BatchNorm backward of inference_net.1, d P rows, dh, d inference_net.0[:, 64:]
__global__ __launch_bounds__(64) void aux_infer_bwd_kernel(AuxArgs p, int batch) {
  __shared__ float sh_h[16 * MC_LDH];      // h; from the slot loop on: a1 of the slot
  __shared__ float sh_P[16 * MC_LDH];
  __shared__ float sh_xh[16 * MC_LDH];     // xhat of the slot, then d u of the slot
  __shared__ float sh_dP[16 * MC_LDH];
  __shared__ float sh_wa[MC_AMAX * MC_NH], sh_dwa[MC_AMAX * MC_NH];
  __shared__ float sh_dout[16 * MC_LDO];
  __shared__ int sh_act[16];
  const int N = p.N, A = p.A, RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15;
  float* part = p.part + (long)blockIdx.x * PO_STRIDE;
  const float invP = 1.0f / ((float)p.R * (float)N);
  load_actions(p, row0, nv, sh_act);
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  stage_wa(p, sh_wa);
  for (int idx = l; idx < 16 * MC_LDH; idx += 64) sh_dP[idx] = 0.0f;
  for (int idx = l; idx < MC_AMAX * MC_NH; idx += 64) sh_dwa[idx] = 0.0f;
  __syncthreads();
  infer_rows(p, sh_h, sh_P);
  __syncthreads();
  for (int j = 0; j < N; ++j) {
    infer_slot(p, j, sh_P, sh_wa, sh_act, sh_h, sh_xh);
    for (int idx = l; idx < 16 * MC_O; idx += 64) {
      const int r = idx / MC_O, o = idx % MC_O;
      sh_dout[r * MC_LDO + o] = r < nv ? p.dout[((row0 + r) * N + j) * MC_O + o] : 0.0f;
    }
    __syncthreads();
    for (int n0 = 0; n0 < MC_NH; n0 += 16) {
      const int c = n0 + m;
      const f32x4 da = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dout, MC_LDO, MC_O, p.iw.i3_w, MC_NH, n0, MC_NH);
      const float scale = p.ss[256 + c], b1 = p.bnsum[c] * invP, b2 = p.bnsum[64 + c] * invP;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = drow(r), at = row * MC_LDH + c;
        float d = da[r] * (sh_h[at] > 0.0f ? 1.0f : 0.01f);
        if (batch) d = d - b1 - sh_xh[at] * b2;
        sh_xh[at] = row < nv ? scale * d : 0.0f;          // this thread's own xhat: d u from here on
      }
    }
    __syncthreads();
    for (int r = 0; r < 16; ++r) {
      const float du = sh_xh[r * MC_LDH + l];
      sh_dP[r * MC_LDH + l] += du;
      sh_dwa[sh_act[recv_row(r, j, N, RW)] * MC_NH + l] += du;
    }
    __syncthreads();
  }
  for (int n0 = 0; n0 < MC_H; n0 += 16) {
    const f32x4 dh = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_dP, MC_LDH, MC_NH, p.iw.i0_w, MC_H + A, n0, MC_H);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (drow(r) < nv) p.dh[(row0 + drow(r)) * MC_H + n0 + m] = dh[r];
  }
  for (int idx = l; idx < 16 * MC_NH; idx += 64) {
    const int r = idx / MC_NH, c = idx % MC_NH;
    if (r < nv) p.dP[(row0 + r) * MC_NH + c] = sh_dP[r * MC_LDH + c];
  }
  for (int idx = l; idx < A * MC_NH; idx += 64) part[PO_WA + idx] = sh_dwa[idx];
}

// ---- launches 4a / 6a (more than MB_SLICES tiles): slice s sums columns [c0, c1) of the partials of tiles s, s + MB_SLICES, ..
__global__ __launch_bounds__(256) void aux_slice_kernel(const float* __restrict__ in, int n, float* out, int c0, int c1) {
  const int s = blockIdx.x;
  for (int c = c0 + threadIdx.x; c < c1; c += 256) {
    float a = 0.0f;
    for (int b = s; b < n; b += MB_SLICES) a += in[(long)b * PO_STRIDE + c];
    out[(long)s * PO_STRIDE + c] = a;
  }
}

// ---- launches 4b / 6b: columns [c0, c1) of rows 0 .. n-1 of `in` summed in sequence and added into the gradients and the losses
__global__ __launch_bounds__(256) void aux_apply_kernel(AuxArgs p, const float* __restrict__ in, int n, int c0, int c1) {
  const int c = c0 + blockIdx.x * 256 + threadIdx.x;
  if (c >= c1) return;
  float a = 0.0f;
  for (int b = 0; b < n; ++b) a += in[(long)b * PO_STRIDE + c];
  if (c < PO_B3) {
    p.ig.i3_w[c - PO_W3] += a;
  } else if (c < PO_S1) {
    p.ig.i3_b[c - PO_B3] += a;
  } else if (c < PO_S2) {
    p.ig.ibn_b[c - PO_S1] += a;
    p.bnsum[c - PO_S1] = a;
  } else if (c < PO_QW) {
    p.ig.ibn_w[c - PO_S2] += a;
    p.bnsum[64 + c - PO_S2] = a;
  } else if (c < PO_QB) {
    p.g.q_w[c - PO_QW] += a;
  } else if (c < PO_MI) {
    p.g.q_b[c - PO_QB] += a;
  } else if (c == PO_MI) {
    p.mi_out[0] += p.mi_w * (a / ((float)p.R * (float)p.N));
  } else if (c == PO_ENT) {
    p.ent_out[0] += p.ent_w * (a / (float)p.R);
  } else if (c >= PO_WA) {
    const int act = (c - PO_WA) / MC_NH, nn = (c - PO_WA) % MC_NH;
    if (act < p.A) p.ig.i0_w[(long)nn * (MC_H + p.A) + MC_H + act] += a;
  }
}

struct AuxLayout {
  long dout, dP, dkey, spart, ss, bnsum, part, part2, wg, total;     // float offsets
  int nblk;
};

AuxLayout aux_layout(int bs, int N, int A) {
  AuxLayout L;
  const long R = (long)bs * N;
  const int G = mc_envs_per_tile(N);
  L.nblk = (bs + G - 1) / G;
  L.dout = 0;
  L.dP = head_tile::pad64(R * N * MC_O);
  L.dkey = L.dP + head_tile::pad64(R * MC_NH);
  L.spart = L.dkey + head_tile::pad64(R * MC_D);
  L.ss = L.spart + (long)L.nblk * SP;
  L.bnsum = L.ss + 512;
  L.part = L.bnsum + 128;
  L.part2 = L.part + (long)L.nblk * PO_STRIDE;
  L.wg = L.part2 + (long)MB_SLICES * PO_STRIDE;
  const int M = R > 0x7fffffff ? 0x7fffffff : (int)R;
  const size_t c0 = marl_linear_wgrad_workspace(M, MC_NH, MC_H, 1), c1 = marl_linear_wgrad_workspace(M, MC_D, MC_H, 1);
  const size_t wg = c0 > c1 ? c0 : c1;
  L.total = L.wg + (long)((wg + 3) / 4);
  (void)A;
  return L;
}

bool infer_ok(const marl_maic_infer_t* w, const marl_maic_infer_grads_t* g) {
  const void* ps[] = {w->i0_w, w->i0_b, w->ibn_w, w->ibn_b, w->ibn_rm, w->ibn_rv, w->i3_w, w->i3_b,
                      g->i0_w, g->i0_b, g->ibn_w, g->ibn_b, g->i3_w, g->i3_b};
  for (const void* q : ps)
    if (!q) return false;
  return true;
}

// the partial columns [c0, c1) of all tiles, merged in a fixed order and applied
int merge_partials(const AuxArgs& a, int nblk, int c0, int c1, hipStream_t s) {
  const dim3 grid((unsigned)((c1 - c0 + 255) / 256));
  if (nblk > MB_SLICES) {
    hipLaunchKernelGGL(aux_slice_kernel, dim3(MB_SLICES), dim3(256), 0, s, (const float*)a.part, nblk, a.part2, c0, c1);
    MARL_CHECK_LAUNCH();
    hipLaunchKernelGGL(aux_apply_kernel, grid, dim3(256), 0, s, a, (const float*)a.part2, MB_SLICES, c0, c1);
  } else {
    hipLaunchKernelGGL(aux_apply_kernel, grid, dim3(256), 0, s, a, (const float*)a.part, nblk, c0, c1);
  }
  MARL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t marl_maic_aux_workspace(int bs, int N, int A) {
  if (bs < 0 || N < 1 || N > MC_NMAX || A < 1 || A > MC_AMAX) return 0;
  return (size_t)aux_layout(bs, N, A).total * sizeof(float);
}

extern "C" int marl_maic_aux(const marl_maic_weights_t* w, const marl_maic_infer_t* iw, const marl_maic_grads_t* g,
                             const marl_maic_infer_grads_t* ig, const float* h, const float* eps, const float* return_q,
                             float mi_weight, float entropy_weight, const float* den, float dscale, float* mi_out,
                             float* ent_out, float* dpar, float* dh, float* ws, size_t ws_bytes, int bs, int N, int A,
                             int test_mode, int bn_batch, float var_floor, float bn_eps, float bn_momentum, void* stream) {
  if (!w || !maic_weights_ok(w) || !iw || !ig || !infer_ok(iw, ig) || !g || !g->k_w || !g->k_b || !g->q_w || !g->q_b || !h ||
      !return_q || !mi_out || !ent_out || !dpar || !dh || !ws || bs < 0 || !marl_maic_supported(N, 1, A, MC_H, MC_NH, MC_L, MC_D))
    return (int)hipErrorInvalidValue;
  if (!test_mode && !eps) return (int)hipErrorInvalidValue;
  const long R = (long)bs * N;
  if (R == 0) return 0;
  if (R * N > 0x7fffffffL || (bn_batch && R < 2) || ws_bytes < marl_maic_aux_workspace(bs, N, A)) return (int)hipErrorInvalidValue;
  const AuxLayout L = aux_layout(bs, N, A);
  AuxArgs a{};
  a.w = *w; a.iw = *iw; a.g = *g; a.ig = *ig;
  a.h = h; a.eps = test_mode ? nullptr : eps; a.q = return_q; a.den = den;
  a.mi_out = mi_out; a.ent_out = ent_out; a.dpar = dpar; a.dh = dh;
  a.spart = ws + L.spart; a.ss = ws + L.ss; a.bnsum = ws + L.bnsum;
  a.dout = ws + L.dout; a.dP = ws + L.dP; a.dkey = ws + L.dkey; a.part = ws + L.part; a.part2 = ws + L.part2;
  a.R = R; a.bs = bs; a.N = N; a.A = A; a.G = mc_envs_per_tile(N); a.test_mode = test_mode ? 1 : 0;
  a.move_stats = (bn_batch && mi_weight > 0.0f) ? 1 : 0;
  a.mi_w = mi_weight; a.ent_w = entropy_weight; a.dscale = dscale;
  a.var_floor = var_floor; a.bn_eps = bn_eps; a.bn_mom = bn_momentum;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nblk);
  const int batch = bn_batch ? 1 : 0;
  if (batch) {
    hipLaunchKernelGGL(aux_stats_kernel, grid, dim3(64), 0, s, a);
    MARL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(aux_bn_kernel, dim3(1), dim3(64 * MC_RED), 0, s, a, L.nblk, batch);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(aux_loss_kernel, grid, dim3(64), 0, s, a);
  MARL_CHECK_LAUNCH();
  int e;
  if ((e = merge_partials(a, L.nblk, 0, PO_ENT + 1, s))) return e;
  hipLaunchKernelGGL(aux_infer_bwd_kernel, grid, dim3(64), 0, s, a, batch);
  MARL_CHECK_LAUNCH();
  if ((e = merge_partials(a, L.nblk, PO_WA, PO_WA + A * MC_NH, s))) return e;
  float* wg = ws + L.wg;
  const size_t wg_bytes = ws_bytes - (size_t)L.wg * sizeof(float);
  marl_src_t xh{};
  xh.p0 = h; xh.ld0 = MC_H; xh.k0 = MC_H;
  // inference_net.0[:, :64]: dW += d P^T h (the action columns came from the partials) ; w_key: dW += d key^T h
  if ((e = marl_linear_wgrad(a.dP, MC_NH, nullptr, 0, &xh, ig->i0_w, MC_H + A, ig->i0_b, (int)R, MC_NH, MC_H, 0, nullptr, wg,
                             wg_bytes, stream))) return e;
  if ((e = marl_linear_wgrad(a.dkey, MC_D, nullptr, 0, &xh, g->k_w, MC_H, g->k_b, (int)R, MC_D, MC_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  return 0;
}
