// World-model head (reference network/world_model.py:7-41 WorldModel, :44-75 Agent.forward's q += r) on gfx950, with its
// prediction loss (algorithm/q_learner_state.py:175-181) and the backward pass of both.
//
// One wave per 16-row tile (one row = agent n of one (episode, step), or of one environment in a rollout step):
//   z = relu(W1 h + b1), e = relu(W2 z + b2)           hidden_embd (Linear, ReLU, Linear) + the ReLU of WorldModel.forward
//   r = Wr e + br  (A)   -> q += r                     world_model.py:71
//   o_hat = Wo e + bo (O), tau = Wt e + bt (2)          tau never reaches a loss; computed on request only
// Dense products run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32) over the tile with the weights read through L2
// (W1, W2: 16 KB each, Wr / Wo: A / O rows of 256 B - 99 KB at 2s3z, 129 KB at MMM2): the tile product of csrc/head_tile.h.
//
// Train mode adds sum (o_hat - o_next)^2 of the tile into one partial per workgroup; a one-workgroup kernel sums the partials in
// a fixed order and adds the total into the loss slot - no float atomics, the same bits on every run.
//
// Backward: the tile recomputes z, e and o_hat from hs (one extra pass over hs instead of saving 128 floats per row in the
// forward), then
//   dr = the sparse (dq_idx, dq_val) pair of the row (q = fc2(h) + r: dr = dq), d_o = dscale * den * (o_hat - o_next)
//   dE = Wr^T dr + Wo^T d_o,  dZ = W2^T (dE * [e > 0]),  dhs = W1^T (dZ * [z > 0])
// and stores z, e, dZ, dE, dR (dense), d_o for the weight gradients: four marl_linear_wgrad reductions (partial slabs, fixed-order
// reduce) accumulate them into the caller's gradient buffer.  Traffic per row: hs read twice (fwd + bwd) and once more by the
// W1 reduction; 4 x 64 + A + O floats written and read back once by the reductions.
#include "head_tile.h"
#include "../../include/marl_hip.h"

namespace {

using head_tile::drow;
using head_tile::tile_gemm;    // K-guarded here: O is any width
using head_tile::tile_gemm_t;

constexpr int WM_H = 64;            // rnn_hidden_dim
constexpr int WM_LDH = WM_H + 4;
constexpr int WM_NMAX = 16;
constexpr int WM_AMAX = 32;
constexpr int WM_OMAX = 256;

struct WorldArgs {
  marl_world_weights_t w;
  const float* h;                    // (R, 64)
  float* q;                          // (R, A) or null: q += r
  float *r_out, *ohat_out, *tau_out; // optional (R, A) / (R, O) / (R, 2)
  const float* obs; long obs_bs; int obs_t0; const int* ep_len; const int* ep_map;   // o_next addressing (train / bwd)
  float* partial;                    // train: one loss partial per workgroup
  // backward
  const int* dq_idx; const float* dq_val; const float* den; float dscale;
  float* dhs;                        // (R, 64)
  float *zs, *es, *dz, *de, *dr, *dov;  // (R,64) x 4, (R, lda), (R, ldo)
  int lda, ldo;
  long R; int T, N, O, A;
};

// o_next of row g, column c (c < O): the unroll's addressing (marl_agent_unroll_fwd), steps t >= ep_len read as zeros
__device__ __forceinline__ float onext_at(const WorldArgs& p, long g, int c) {
  const long tn = (long)p.T * p.N;
  const long b = g / tn;
  const int t = (int)((g / p.N) % p.T), n = (int)(g % p.N);
  if (p.ep_len && t >= p.ep_len[b]) return 0.0f;
  const long eb = p.ep_map ? (long)p.ep_map[b] : b;
  return p.obs[((eb * p.obs_bs) + (long)(t + p.obs_t0) * p.N + n) * (long)p.O + c];
}

// h of the tile -> sh_h, z -> sh_z, e -> sh_e (rows past R are zeros); optionally stores z and e
__device__ __forceinline__ void embed(const WorldArgs& p, long row0, float* sh_h, float* sh_z, float* sh_e, bool store) {
  const int l = threadIdx.x, m = l & 15;
  head_tile::load_h(sh_h, WM_LDH, p.h, row0, [&](int r) { return row0 + r < p.R; });
  __syncthreads();
  for (int n0 = 0; n0 < WM_H; n0 += 16) {
    const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_h, WM_LDH, WM_H, p.w.h0_w, WM_H, 0, n0, WM_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = fmaxf(acc[r] + p.w.h0_b[n0 + m], 0.0f);
      sh_z[drow(r) * WM_LDH + n0 + m] = v;
      if (store && row0 + drow(r) < p.R) p.zs[(row0 + drow(r)) * WM_H + n0 + m] = v;
    }
  }
  __syncthreads();
  for (int n0 = 0; n0 < WM_H; n0 += 16) {
    const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_z, WM_LDH, WM_H, p.w.h2_w, WM_H, 0, n0, WM_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = fmaxf(acc[r] + p.w.h2_b[n0 + m], 0.0f);
      sh_e[drow(r) * WM_LDH + n0 + m] = v;
      if (store && row0 + drow(r) < p.R) p.es[(row0 + drow(r)) * WM_H + n0 + m] = v;
    }
  }
  __syncthreads();
}

template <bool TRAIN>
__global__ __launch_bounds__(64) void world_fwd_kernel(WorldArgs p) {
  __shared__ float sh_h[16 * WM_LDH], sh_z[16 * WM_LDH], sh_e[16 * WM_LDH];
  const long row0 = (long)blockIdx.x * 16;
  const int l = threadIdx.x, m = l & 15;
  embed(p, row0, sh_h, sh_z, sh_e, false);
  const marl_world_weights_t& w = p.w;
  // ---- r: q += r
  for (int n0 = 0; n0 < p.A; n0 += 16) {
    const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_e, WM_LDH, WM_H, w.r_w, WM_H, 0, n0, p.A);
    const int c = n0 + m;
    if (c < p.A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long g = row0 + drow(r);
        if (g < p.R) {
          const float v = acc[r] + w.r_b[c];
          if (p.q) p.q[g * p.A + c] += v;
          if (p.r_out) p.r_out[g * p.A + c] = v;
        }
      }
    }
  }
  // ---- o_hat (train: the squared error against o_next)
  float lsum = 0.0f;
  if (TRAIN || p.ohat_out) {
    for (int n0 = 0; n0 < p.O; n0 += 16) {
      const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_e, WM_LDH, WM_H, w.o_w, WM_H, 0, n0, p.O);
      const int c = n0 + m;
      if (c < p.O) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long g = row0 + drow(r);
          if (g < p.R) {
            const float v = acc[r] + w.o_b[c];
            if (p.ohat_out) p.ohat_out[g * p.O + c] = v;
            if (TRAIN) {
              const float d = v - onext_at(p, g, c);
              lsum = fmaf(d, d, lsum);
            }
          }
        }
      }
    }
  }
  // ---- tau (terminate_out), on request
  if (p.tau_out) {
    const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_e, WM_LDH, WM_H, w.t_w, WM_H, 0, 0, 2);
    if (m < 2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long g = row0 + drow(r);
        if (g < p.R) p.tau_out[g * 2 + m] = acc[r] + w.t_b[m];
      }
    }
  }
  if (TRAIN) {
    // fixed butterfly over the wave: every lane ends with the same sum, in the same order on every run
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
    if (l == 0) p.partial[blockIdx.x] = lsum;
  }
}

// loss[0] += sum of n partials: strided per-thread sums, then a fixed tree over the workgroup
__global__ __launch_bounds__(256) void world_loss_reduce_kernel(const float* __restrict__ partial, long n, float* loss) {
  __shared__ float sh[256];
  float s = 0.0f;
  for (long i = threadIdx.x; i < n; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] += sh[0];
}

__global__ __launch_bounds__(64) void world_bwd_kernel(WorldArgs p) {
  __shared__ float sh_h[16 * WM_LDH], sh_z[16 * WM_LDH], sh_e[16 * WM_LDH], sh_g[16 * WM_LDH];
  __shared__ float sh_do[16 * (WM_OMAX + 4)];
  __shared__ int sh_ai[16];
  __shared__ float sh_av[16];
  const long row0 = (long)blockIdx.x * 16;
  const int l = threadIdx.x, m = l & 15;
  const int O = p.O, A = p.A, ldo = WM_OMAX + 4;
  const marl_world_weights_t& w = p.w;
  if (l < 16) {
    const long g = row0 + l;
    int a = -1;
    float v = 0.0f;
    if (g < p.R && p.dq_idx) {
      a = p.dq_idx[g];
      v = p.dq_val[g];
      if (a < 0 || a >= A) a = -1;
    }
    sh_ai[l] = a;
    sh_av[l] = v;
  }
  embed(p, row0, sh_h, sh_z, sh_e, true);
  const float scale = p.dscale * (p.den ? p.den[0] : 1.0f);
  // ---- dR (dense copy of the sparse pair) and d_o = scale * (o_hat - o_next)
  for (int idx = l; idx < 16 * p.lda; idx += 64) {
    const int r = idx / p.lda, c = idx % p.lda;
    if (row0 + r < p.R) p.dr[(row0 + r) * p.lda + c] = (c == sh_ai[r]) ? sh_av[r] : 0.0f;
  }
  const int OP = (O + 15) / 16 * 16;
  for (int n0 = 0; n0 < OP; n0 += 16) {
    const f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_e, WM_LDH, WM_H, w.o_w, WM_H, 0, n0, O);
    const int c = n0 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long g = row0 + drow(r);
      float d = 0.0f;
      if (c < O && g < p.R) {
        d = scale * (acc[r] + w.o_b[c] - onext_at(p, g, c));
        p.dov[g * p.ldo + c] = d;
      } else if (c < p.ldo && g < p.R) {
        p.dov[g * p.ldo + c] = 0.0f;
      }
      sh_do[drow(r) * ldo + c] = d;
    }
  }
  __syncthreads();
  // ---- dE = Wo^T d_o + dq * Wr[a, :]; gate with e > 0 into sh_g
  for (int n0 = 0; n0 < WM_H; n0 += 16) {
    const f32x4 acc = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_do, ldo, O, w.o_w, WM_H, n0, WM_H);
    const int c = n0 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = drow(r);
      const long g = row0 + row;
      const int a = sh_ai[row];
      const float v = acc[r] + (a >= 0 ? sh_av[row] * w.r_w[(long)a * WM_H + c] : 0.0f);
      if (g < p.R) p.de[g * WM_H + c] = v;
      sh_g[row * WM_LDH + c] = sh_e[row * WM_LDH + c] > 0.0f ? v : 0.0f;
    }
  }
  __syncthreads();
  // ---- dZ = W2^T dE_pre; gate with z > 0 into sh_h (h is no longer needed)
  for (int n0 = 0; n0 < WM_H; n0 += 16) {
    const f32x4 acc = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_g, WM_LDH, WM_H, w.h2_w, WM_H, n0, WM_H);
    const int c = n0 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = drow(r);
      const long g = row0 + row;
      if (g < p.R) p.dz[g * WM_H + c] = acc[r];
      sh_h[row * WM_LDH + c] = sh_z[row * WM_LDH + c] > 0.0f ? acc[r] : 0.0f;
    }
  }
  __syncthreads();
  // ---- dhs = W1^T dZ_pre
  for (int n0 = 0; n0 < WM_H; n0 += 16) {
    const f32x4 acc = tile_gemm_t(f32x4{0, 0, 0, 0}, sh_h, WM_LDH, WM_H, w.h0_w, WM_H, n0, WM_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long g = row0 + drow(r);
      if (g < p.R) p.dhs[g * WM_H + n0 + m] = acc[r];
    }
  }
}

bool world_weights_ok(const marl_world_weights_t* w) {
  const float* ps[] = {w->h0_w, w->h0_b, w->h2_w, w->h2_b, w->r_w, w->r_b, w->o_w, w->o_b, w->t_w, w->t_b};
  for (const float* q : ps)
    if (!q) return false;
  return true;
}

bool world_grads_ok(const marl_world_grads_t* g) {
  float* ps[] = {g->h0_w, g->h0_b, g->h2_w, g->h2_b, g->r_w, g->r_b, g->o_w, g->o_b};
  for (float* q : ps)
    if (!q) return false;
  return true;
}

struct BwdLayout {
  long zs, es, dz, de, dr, dov, wg, total;     // float offsets into the workspace
};

BwdLayout bwd_layout(long R, int O, int A) {
  BwdLayout L;
  const long p64 = head_tile::pad64(R * WM_H);
  L.zs = 0; L.es = p64; L.dz = 2 * p64; L.de = 3 * p64; L.dr = 4 * p64;
  L.dov = L.dr + head_tile::pad64(R * head_tile::round4(A));
  L.wg = L.dov + head_tile::pad64(R * head_tile::round4(O));
  size_t wg = 0;
  const int M = R > 0x7fffffff ? 0x7fffffff : (int)R;
  const size_t cand[] = {marl_linear_wgrad_workspace(M, WM_H, WM_H, 1), marl_linear_wgrad_workspace(M, A, WM_H, 1),
                         marl_linear_wgrad_workspace(M, O, WM_H, 1)};
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

extern "C" int marl_world_supported(int N, int O, int A, int H) {
  return H == WM_H && N >= 1 && N <= WM_NMAX && A >= 1 && A <= WM_AMAX && O >= 1 && O <= WM_OMAX;
}

extern "C" size_t marl_world_fwd_workspace(int B, int T, int N) {
  const long R = (long)B * T * N;
  return (size_t)((R + 15) / 16) * sizeof(float);
}

extern "C" size_t marl_world_bwd_workspace(int B, int T, int N, int O, int A) {
  return (size_t)bwd_layout((long)B * T * N, O, A).total * sizeof(float);
}

extern "C" int marl_world_head_fwd(const marl_world_weights_t* w, const float* h, float* q, float* r_out, float* ohat_out,
                                   float* tau_out, const float* obs, long obs_bs, int obs_t0, const int* ep_len,
                                   const int* ep_map, float* loss, float* ws, size_t ws_bytes, int B, int T, int N, int O,
                                   int A, void* stream) {
  if (!w || !world_weights_ok(w) || !h || B < 0 || T < 1 || !marl_world_supported(N, O, A, WM_H))
    return (int)hipErrorInvalidValue;
  const bool train = loss != nullptr;
  if (train && (!obs || !ws || ws_bytes < marl_world_fwd_workspace(B, T, N))) return (int)hipErrorInvalidValue;
  WorldArgs a{};
  a.w = *w;
  a.h = h; a.q = q; a.r_out = r_out; a.ohat_out = ohat_out; a.tau_out = tau_out;
  a.obs = obs; a.obs_bs = obs_bs; a.obs_t0 = obs_t0; a.ep_len = ep_len; a.ep_map = ep_map;
  a.partial = ws;
  a.R = (long)B * T * N; a.T = T; a.N = N; a.O = O; a.A = A;
  const long blocks = (a.R + 15) / 16;
  if (blocks == 0) return 0;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (train) hipLaunchKernelGGL(world_fwd_kernel<true>, dim3((unsigned)blocks), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(world_fwd_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, s, a);
  MARL_CHECK_LAUNCH();
  if (train) {
    hipLaunchKernelGGL(world_loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, blocks, loss);
    MARL_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int marl_world_head_bwd(const marl_world_weights_t* w, const marl_world_grads_t* gr, const float* hs,
                                   const int* dq_idx, const float* dq_val, const float* obs, long obs_bs, int obs_t0,
                                   const int* ep_len, const int* ep_map, const float* den, float dscale, float* dhs,
                                   float* ws, size_t ws_bytes, int B, int T, int N, int O, int A, void* stream) {
  if (!w || !world_weights_ok(w) || !gr || !world_grads_ok(gr) || !hs || !obs || !dhs || !ws || (dq_idx && !dq_val) ||
      B < 0 || T < 1 || !marl_world_supported(N, O, A, WM_H))
    return (int)hipErrorInvalidValue;
  const long R = (long)B * T * N;
  if (R == 0) return 0;
  if (R > 0x7fffffffL || ws_bytes < marl_world_bwd_workspace(B, T, N, O, A)) return (int)hipErrorInvalidValue;
  const BwdLayout L = bwd_layout(R, O, A);
  WorldArgs a{};
  a.w = *w;
  a.h = hs;
  a.obs = obs; a.obs_bs = obs_bs; a.obs_t0 = obs_t0; a.ep_len = ep_len; a.ep_map = ep_map;
  a.dq_idx = dq_idx; a.dq_val = dq_val; a.den = den; a.dscale = dscale;
  a.dhs = dhs;
  a.zs = ws + L.zs; a.es = ws + L.es; a.dz = ws + L.dz; a.de = ws + L.de; a.dr = ws + L.dr; a.dov = ws + L.dov;
  a.lda = head_tile::round4(A); a.ldo = head_tile::round4(O);
  a.R = R; a.T = T; a.N = N; a.O = O; a.A = A;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(world_bwd_kernel, dim3((unsigned)((R + 15) / 16)), dim3(64), 0, s, a);
  MARL_CHECK_LAUNCH();
  float* wg = ws + L.wg;
  const size_t wg_bytes = ws_bytes - (size_t)L.wg * sizeof(float);
  const int M = (int)R;
  int e;
  // hidden_embd.0: dW1 += (dZ [z > 0])^T h ; hidden_embd.2: dW2 += (dE [e > 0])^T z
  marl_src_t xh = dense_src(hs, WM_H, WM_H), xz = dense_src(a.zs, WM_H, WM_H), xe = dense_src(a.es, WM_H, WM_H);
  if ((e = marl_linear_wgrad(a.dz, WM_H, a.zs, WM_H, &xh, gr->h0_w, WM_H, gr->h0_b, M, WM_H, WM_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  if ((e = marl_linear_wgrad(a.de, WM_H, a.es, WM_H, &xz, gr->h2_w, WM_H, gr->h2_b, M, WM_H, WM_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  // r_out: dWr += dR^T e ; o_out: dWo += d_o^T e   (terminate_out: no gradient)
  if ((e = marl_linear_wgrad(a.dr, a.lda, nullptr, 0, &xe, gr->r_w, WM_H, gr->r_b, M, A, WM_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  if ((e = marl_linear_wgrad(a.dov, a.ldo, nullptr, 0, &xe, gr->o_w, WM_H, gr->o_b, M, O, WM_H, 0, nullptr, wg, wg_bytes,
                             stream))) return e;
  return 0;
}
