// MAIC message head (reference network/MAIC.py:52-94, MAICAgent.forward after fc2) on gfx950: the forward.  Its backward is
// maic_head_bwd.hip.
//
// Per environment of N agents (row = b * N + agent, h = the GRU output of the row):
//   y = embed_net.0 h;  z = LeakyReLU(BatchNorm(y));  p = embed_net.3 z            (2 N L columns: means | log-variances)
//   latent[i][j] (L) = mean, or mean + sqrt(max(exp(logvar), var_floor)) * eps in sampled mode     (agent i's latent for slot j)
//   msg[i][j] = msg_net.2 LeakyReLU(msg_net.0 cat(h_j, latent[i][j]))       (MAIC.py:70-72: h_repeat puts h of agent j there)
//   alpha[i][.] = softmax_j(w_key(h_i) . w_query(latent[i][j]) / sqrt(D)), diagonal -1e9; test mode: alpha < 0.25 / N -> 0
//   q[j] += sum_i alpha[i][j] msg[i][j]                                                             (MAIC.py:85, dim 1)
//
// One wave owns a tile of G = 16 / N whole environments (G N <= 16 rows), so the softmax over j and the sum over i stay inside
// the workgroup.  What makes the pair work cheap:
//   * msg_net.0 is linear in cat(h_j, latent_ij): U_j = W[:, :64] h_j + b once per row (MFMA), the L-wide part per pair.
//   * msg_net.2 is linear and alpha is a scalar per pair: q_j += W2 (sum_i alpha_ij T_ij) + b2 sum_i alpha_ij with
//     T_ij = LeakyReLU(U_j + W[:, 64:] latent_ij), so the A-wide product runs once per row, not once per pair.
//   * for a fixed slot j the 16 x 64 tile T_.j is one K = 8 MFMA product over the tile's rows, and its accumulator registers are
//     exactly the B operand of the K-permuted 16 x 16 x 16 step (register i <-> row 4 q + i), so sum_i alpha_ij T_ij is a second
//     MFMA with the gated alphas scattered into the A operand - no LDS round trip, no cross-lane sum.
//   * key . (Wq latent + bq) = (Wq^T key) . latent + key . bq: eight numbers per row instead of a D-wide query per pair.
// Dense products are fp32 MFMA (v_mfma_f32_16x16x4_f32) with the weights read through L2: the tile product of
// csrc/head_tile.h.
//
// BatchNorm: eval mode is an affine map folded per column in the one launch.  Batch-statistics mode (a module in training
// mode) needs the column statistics of y over ALL rows first: launch 1 writes y and one (mean, M2) pair per workgroup and
// column, launch 2 (one workgroup) merges them in a fixed order (Chan's pairwise update: no E[y^2] - mean^2 cancellation, no
// float atomics, the same bits on every run), writes scale / shift and updates running_mean / running_var /
// num_batches_tracked, launch 3 is the head reading y back.
#include "synth_env.h"
#include "maic_common.h"

namespace {

using namespace maic;
using head_tile::drow;

constexpr unsigned ST_MAIC_EPS = 8;  // hash stream of the sampled latents' noise (synth_env.h streams end at ST_PICK = 7)

struct MaicArgs {
  marl_maic_weights_t w;
  const float* h;                    // (R, 64)
  float* q;                          // (R, A), updated in place
  const float* eps;                  // (R, N L) or null (test mode)
  float *mean_out, *var_out, *lat_out, *alpha_out, *msg_out;   // optional
  float *y, *part, *ss;              // batch statistics: (R, 64) pre-activations, per-workgroup (mean | M2), scale | shift
  long R;
  int bs, N, A, G, test_mode;
  float var_floor, bn_eps, bn_mom;
};

// rows of this workgroup's tile that exist
__device__ __forceinline__ int tile_rows(const MaicArgs& p, long row0) {
  const long left = p.R - row0;
  const int rw = p.G * p.N;
  return left < rw ? (int)left : rw;
}

// ---- batch statistics, launch 1: y = embed_net.0 h of the tile and the tile's (mean, M2) per column
__global__ __launch_bounds__(64) void maic_embed_stats_kernel(MaicArgs p) {
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
    for (int r = 0; r < 4; ++r) {
      const int row = drow(r);
      const float v = acc[r] + p.w.e0_b[c];
      sh_y[row * MC_LDH + c] = v;
      if (row < nv) p.y[(row0 + row) * MC_NH + c] = v;
    }
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
  p.part[(long)blockIdx.x * 128 + l] = mean;
  p.part[(long)blockIdx.x * 128 + 64 + l] = m2;
}

// ---- launch 2: merge the nblk partials (slice s takes blocks s, s + 16, ..; then slices 0..15 in order), write the affine map
// of the batch statistics and update the running statistics as torch's BatchNorm1d does in training mode
__global__ __launch_bounds__(64 * MC_RED) void maic_bn_reduce_kernel(MaicArgs p, int nblk) {
  __shared__ float sh_n[MC_RED][64], sh_m[MC_RED][64], sh_v[MC_RED][64];
  const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int rw = p.G * p.N;
  float n = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int b = s; b < nblk; b += MC_RED) {
    const long left = p.R - (long)b * rw;
    const float nb = (float)(left < rw ? left : rw);
    chan_merge(n, mean, m2, nb, p.part[(long)b * 128 + c], p.part[(long)b * 128 + 64 + c]);
  }
  sh_n[s][c] = n; sh_m[s][c] = mean; sh_v[s][c] = m2;
  __syncthreads();
  if (s != 0) return;
  for (int k = 1; k < MC_RED; ++k) chan_merge(n, mean, m2, sh_n[k][c], sh_m[k][c], sh_v[k][c]);
  const float var = m2 / n;                                   // biased: the normalisation
  const float scale = p.w.bn_w[c] / sqrtf(var + p.bn_eps);
  p.ss[c] = scale;
  p.ss[64 + c] = p.w.bn_b[c] - mean * scale;
  p.w.bn_rm[c] = (1.0f - p.bn_mom) * p.w.bn_rm[c] + p.bn_mom * mean;
  p.w.bn_rv[c] = (1.0f - p.bn_mom) * p.w.bn_rv[c] + p.bn_mom * (m2 / (n - 1.0f));     // unbiased: the running estimate
  if (c == 0 && p.w.bn_nbt) p.w.bn_nbt[0] += 1;
}

// ---- the head.  BATCH: y and scale | shift come from launches 1 and 2; otherwise y is computed here and BatchNorm is the
// affine map of the running statistics.
template <bool BATCH>
__global__ __launch_bounds__(64) void maic_head_kernel(MaicArgs p) {
  __shared__ float sh_h[16 * MC_LDH], sh_z[16 * MC_LDH], sh_u[16 * MC_LDH], sh_lat[16 * MC_LDL];
  __shared__ float sh_k[16 * MC_LDK], sh_kq[16 * MC_LDQ], sh_al[16 * MC_LDA], sh_as[16];
  const marl_maic_weights_t& w = p.w;
  const int N = p.N, A = p.A, NL = p.N * MC_L, RW = p.G * p.N;
  const long row0 = (long)blockIdx.x * RW;
  const int nv = tile_rows(p, row0);
  const int l = threadIdx.x, m = l & 15, qd = l >> 4;
  head_tile::load_h(sh_h, MC_LDH, p.h, row0, [&](int r) { return r < nv; });
  __syncthreads();
  // ---- z = LeakyReLU(BatchNorm(embed_net.0 h)); U = msg_net.0[:, :64] h + b; key = w_key h + b
  for (int n0 = 0; n0 < MC_NH; n0 += 16) {
    const int c = n0 + m;
    f32x4 y;
    float scale, shift;
    if (BATCH) {
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = drow(r) < nv ? p.y[(row0 + drow(r)) * MC_NH + c] : 0.0f;
      scale = p.ss[c];
      shift = p.ss[64 + c];
    } else {
      y = mc_gemm(sh_h, MC_LDH, MC_H, w.e0_w, MC_H, n0, MC_NH);
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] += w.e0_b[c];
      scale = w.bn_w[c] / sqrtf(w.bn_rv[c] + p.bn_eps);
      shift = w.bn_b[c] - w.bn_rm[c] * scale;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_z[drow(r) * MC_LDH + c] = leaky(fmaf(y[r], scale, shift));
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
  // ---- latent: the means (columns < N L of embed_net.3), plus sqrt(var) eps in sampled mode (columns N L ..)
  for (int n0 = 0; n0 < NL; n0 += 16) {
    const int c = n0 + m;
    const f32x4 mu = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w, MC_NH, n0, NL);
    f32x4 lat;
#pragma unroll
    for (int r = 0; r < 4; ++r) lat[r] = c < NL ? mu[r] + w.e3_b[c] : 0.0f;
    if (p.mean_out && c < NL) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (drow(r) < nv) p.mean_out[(row0 + drow(r)) * NL + c] = lat[r];
    }
    if (!p.test_mode || p.var_out) {
      const f32x4 lv = mc_gemm(sh_z, MC_LDH, MC_NH, w.e3_w + (long)NL * MC_NH, MC_NH, n0, NL);
      if (c < NL) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long g = row0 + drow(r);
          if (drow(r) < nv) {
            const float var = fmaxf(expf(lv[r] + w.e3_b[NL + c]), p.var_floor);
            if (p.var_out) p.var_out[g * NL + c] = var;
            if (!p.test_mode) lat[r] = fmaf(sqrtf(var), p.eps[g * NL + c], lat[r]);
          }
        }
      }
    }
    if (c < NL) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sh_lat[drow(r) * MC_LDL + c] = lat[r];
        if (p.lat_out && drow(r) < nv) p.lat_out[(row0 + drow(r)) * NL + c] = lat[r];
      }
    }
  }
  // ---- kq[r][k] = sum_d key[r][d] Wq[d][k] (k < L), kq[r][L] = key[r] . bq
  for (int idx = l; idx < 16 * (MC_L + 1); idx += 64) {
    const int r = idx / (MC_L + 1), k = idx % (MC_L + 1);
    float s = 0.0f;
    for (int d = 0; d < MC_D; ++d) s = fmaf(sh_k[r * MC_LDK + d], k < MC_L ? w.q_w[d * MC_L + k] : w.q_b[d], s);
    sh_kq[r * MC_LDQ + k] = s;
  }
  __syncthreads();
  // ---- logits of row r = (env, i) for every slot j
  for (int idx = l; idx < 16 * N; idx += 64) {
    const int r = idx / N, j = idx % N;
    float s = sh_kq[r * MC_LDQ + MC_L];
#pragma unroll
    for (int k = 0; k < MC_L; ++k) s = fmaf(sh_kq[r * MC_LDQ + k], sh_lat[r * MC_LDL + j * MC_L + k], s);
    s *= MC_QSCALE;
    sh_al[r * MC_LDA + j] = (j == r % N) ? -1e9f : s;          // row0 is a multiple of N: r % N is the agent
  }
  __syncthreads();
  if (l < 16) {
    const int r = l;
    if (r < nv) {
      float mx = -3.0e38f;
      for (int j = 0; j < N; ++j) mx = fmaxf(mx, sh_al[r * MC_LDA + j]);
      float sum = 0.0f;
      for (int j = 0; j < N; ++j) {
        const float e = expf(sh_al[r * MC_LDA + j] - mx);
        sh_al[r * MC_LDA + j] = e;
        sum += e;
      }
      const float thr = 0.25f / (float)N;
      for (int j = 0; j < N; ++j) {
        float a = sh_al[r * MC_LDA + j] / sum;
        if (p.test_mode && a < thr) a = 0.0f;
        sh_al[r * MC_LDA + j] = a;
        if (p.alpha_out) p.alpha_out[(row0 + r) * N + j] = a;
      }
    } else {
      for (int j = 0; j < N; ++j) sh_al[r * MC_LDA + j] = 0.0f;
    }
  }
  __syncthreads();
  // weight of msg_net.2's bias in row (env, j): sum_i alpha[i][j]
  if (l < 16) {
    float s = 0.0f;
    if (l < RW) {
      const int e0 = (l / N) * N, j = l % N;
      for (int i = 0; i < N; ++i) s += sh_al[(e0 + i) * MC_LDA + j];
    }
    sh_as[l] = s;
  }
  // ---- S[(env, j)] = sum_i alpha[i][j] LeakyReLU(U_j + V latent[i][j]), slot by slot
  f32x4 S[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) S[ct] = f32x4{0, 0, 0, 0};
  for (int j = 0; j < N; ++j) {
    // K = 8 as two MFMA steps: at step i lane quarter q supplies k = 2q + i for both operands
    const float x0 = sh_lat[m * MC_LDL + j * MC_L + 2 * qd], x1 = sh_lat[m * MC_LDL + j * MC_L + 2 * qd + 1];
    f32x4 al;        // A operand of the sum: output row m takes alpha[r][j] of the rows r = 4q + i of its own environment
    int rj[4];       // row of agent j in the environment of row 4q + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * qd + i;
      rj[i] = r < RW ? (r / N) * N + j : 0;
      al[i] = (r < RW && m == rj[i]) ? sh_al[r * MC_LDA + j] : 0.0f;
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int n = ct * 16 + m;
      const float* v = w.m0_w + (long)n * MC_M0 + MC_H + 2 * qd;
      f32x4 t = mfma16(x0, __ldg(v), f32x4{0, 0, 0, 0});
      t = mfma16(x1, __ldg(v + 1), t);
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = leaky(t[i] + sh_u[rj[i] * MC_LDH + n]);
      S[ct] = mfma16x4(al, t, S[ct]);
      if (p.msg_out) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sh_z[drow(i) * MC_LDH + n] = t[i];
      }
    }
    if (p.msg_out) {       // tests only: the A-wide product per pair
      __syncthreads();
      for (int n0 = 0; n0 < A; n0 += 16) {
        const f32x4 acc = mc_gemm(sh_z, MC_LDH, MC_NH, w.m2_w, MC_NH, n0, A);
        const int c = n0 + m;
        if (c < A) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (drow(r) < nv) p.msg_out[((row0 + drow(r)) * N + j) * A + c] = acc[r] + w.m2_b[c];
        }
      }
      __syncthreads();
    }
  }
  // ---- q[(env, j)] += msg_net.2 S + b2 sum_i alpha[i][j]
  __syncthreads();
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sh_h[drow(i) * MC_LDH + ct * 16 + m] = S[ct][i];
  }
  __syncthreads();
  for (int n0 = 0; n0 < A; n0 += 16) {
    const f32x4 acc = mc_gemm(sh_h, MC_LDH, MC_NH, w.m2_w, MC_NH, n0, A);
    const int c = n0 + m;
    if (c < A) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (drow(r) < nv) p.q[(row0 + drow(r)) * A + c] += fmaf(w.m2_b[c], sh_as[drow(r)], acc[r]);
    }
  }
}

// eps[(e, n), c] ~ N(0, 1): Box-Muller over two draws of the counter hash keyed by (rseed, env, global step, (n, c))
__global__ __launch_bounds__(256) void maic_noise_kernel(unsigned rseed, unsigned env0, unsigned tg, float* eps, int E, int per_env) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)E * per_env) return;
  const unsigned e = (unsigned)(idx / per_env), k = (unsigned)(idx % per_env);
  const unsigned pre = hprefix(rseed, ST_MAIC_EPS, env0 + e, tg);
  const float u1 = u01(hfin(pre, 2u * k)), u2 = u01(hfin(pre, 2u * k + 1u));
  eps[idx] = sqrtf(-2.0f * logf(1.0f - u1)) * cosf(6.283185307179586f * u2);
}

struct WsLayout {
  long y, part, ss, total;      // float offsets
  int nblk;
};

WsLayout ws_layout(int bs, int N) {
  WsLayout L;
  const int G = mc_envs_per_tile(N);
  L.nblk = (bs + G - 1) / G;
  L.y = 0;
  L.part = head_tile::pad64((long)bs * N * MC_NH);
  L.ss = L.part + (long)L.nblk * 128;
  L.total = L.ss + 128;
  return L;
}

}  // namespace

extern "C" int marl_maic_supported(int N, int O, int A, int H, int NH, int L, int D) {
  return H == MC_H && NH == MC_NH && L == MC_L && D == MC_D && N >= 1 && N <= MC_NMAX && A >= 1 && A <= MC_AMAX && O >= 1;
}

extern "C" size_t marl_maic_workspace(int bs, int N) {
  if (bs < 0 || N < 1 || N > MC_NMAX) return 0;
  return (size_t)ws_layout(bs, N).total * sizeof(float);
}

extern "C" int marl_maic_head_fwd(const marl_maic_weights_t* w, const float* h, float* q, const float* eps, float* mean_out,
                                  float* var_out, float* lat_out, float* alpha_out, float* msg_out, float* ws,
                                  size_t ws_bytes, int bs, int N, int A, int test_mode, int bn_batch, float var_floor,
                                  float bn_eps, float bn_momentum, void* stream) {
  if (!w || !maic_weights_ok(w) || !h || !q || bs < 0 || !marl_maic_supported(N, 1, A, MC_H, MC_NH, MC_L, MC_D))
    return (int)hipErrorInvalidValue;
  if (!test_mode && !eps) return (int)hipErrorInvalidValue;
  const long R = (long)bs * N;
  if (R == 0) return 0;
  if (R > 0x7fffffffL) return (int)hipErrorInvalidValue;
  if (bn_batch && (R < 2 || !ws || ws_bytes < marl_maic_workspace(bs, N))) return (int)hipErrorInvalidValue;
  const WsLayout L = ws_layout(bs, N);
  MaicArgs a{};
  a.w = *w;
  a.h = h; a.q = q; a.eps = test_mode ? nullptr : eps;
  a.mean_out = mean_out; a.var_out = var_out; a.lat_out = lat_out; a.alpha_out = alpha_out; a.msg_out = msg_out;
  if (bn_batch) { a.y = ws + L.y; a.part = ws + L.part; a.ss = ws + L.ss; }
  a.R = R; a.bs = bs; a.N = N; a.A = A; a.G = mc_envs_per_tile(N); a.test_mode = test_mode ? 1 : 0;
  a.var_floor = var_floor; a.bn_eps = bn_eps; a.bn_mom = bn_momentum;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)L.nblk);
  if (bn_batch) {
    hipLaunchKernelGGL(maic_embed_stats_kernel, grid, dim3(64), 0, s, a);
    MARL_CHECK_LAUNCH();
    hipLaunchKernelGGL(maic_bn_reduce_kernel, dim3(1), dim3(64 * MC_RED), 0, s, a, L.nblk);
    MARL_CHECK_LAUNCH();
    hipLaunchKernelGGL(maic_head_kernel<true>, grid, dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL(maic_head_kernel<false>, grid, dim3(64), 0, s, a);
  }
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_maic_noise(unsigned rseed, int env0, unsigned tg, float* eps, int E, int N, void* stream) {
  if (!eps || E < 0 || N < 1 || N > MC_NMAX) return (int)hipErrorInvalidValue;
  const int per_env = N * N * MC_L;
  const long n = (long)E * per_env;
  if (n == 0) return 0;
  hipLaunchKernelGGL(maic_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rseed,
                     (unsigned)env0, tg, eps, E, per_env);
  MARL_CHECK_LAUNCH();
  return 0;
}
