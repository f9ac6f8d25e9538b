// RTW reflection head (reference network/RTW.py:70-119 act mode, :121-203 given mode) on gfx950.
//
// One wave per tile of whole environments: EPT = 16 / N environments, R = EPT * N <= 16 rows (one row = agent i of one
// environment, or of one (episode, t) in given mode).  Keeping an environment inside one tile puts every teammate's row
// (its availability, taken action and - given mode - its GRU output) in the same wave's LDS.
//
// Dense products run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32) over the 16-row tile, with the weights read through
// L2 (140 KB at 2s3z, 280 KB at MMM2: more than a workgroup's LDS, and every phase reads each weight once per tile).
// The tile product and its K-permutation are csrc/head_tile.h.
// One-hot blocks are never multiplied: each becomes a gathered weight column added to the pre-activation
// (T0[:, 64 + j], W0[:, O + j A + a_j], Wk[:, a_j], V0[:, 64 + a_j]).  The value net's second layer is applied once to
// g = sum_j p_j relu(V0 [h ; m_j] + b) (plus bv2 * sum_j p_j) instead of to each v_j.  Argmax and softmax are on the VALU.
#include "head_tile.h"
#include "../../include/marl_hip.h"

namespace {

using head_tile::drow;
using head_tile::tile_gemm;    // K-guarded here: O is any width

constexpr int RTW_H = 64;          // rnn_hidden_dim = hidden_dim = attn_dim
constexpr int RTW_LDH = RTW_H + 4;
constexpr int RTW_NMAX = 16;
constexpr int RTW_AMAX = 32;
constexpr int RTW_OMAX = 256;

struct RtwArgs {
  marl_rtw_weights_t w;
  const float* h;          // (G*N, 64): act mode the GRU output of each row; given mode the hs plane
  const float* obs; long obs_bs; int obs_t0;
  const float* onext; long on_bs; int on_t0;      // given mode
  const float* avail; long av_bs; int av_t0;      // act mode
  const int* u; long u_bs; int u_t0;              // given mode
  float* q;                // (G*N, A), q += q_r
  int* a_out;              // act mode, optional (G*N, N)
  float* ohat_out;         // act mode, optional (G*N, O)
  int G, T, N, O, A;
};

__host__ __device__ inline int rtw_op(int O) { return (O + 15) / 16 * 16; }

template <bool GIVEN, bool NOT_SELF>
__global__ __launch_bounds__(64) void rtw_head_kernel(RtwArgs p) {
  extern __shared__ float smem[];
  const int N = p.N, O = p.O, A = p.A, OP = rtw_op(O), ldo = OP + 4;
  const int EPT = RTW_NMAX / N, R = EPT * N;
  const int g0 = blockIdx.x * EPT;
  const int l = threadIdx.x, m = l & 15;
  float* sh_h = smem;                       // [16][LDH]  h
  float* sh_P = sh_h + 16 * RTW_LDH;        // [16][LDH]  teammate pre-activation, then value pre-activation
  float* sh_x = sh_P + 16 * RTW_LDH;        // [16][LDH]  teammate / world hidden, query, then g
  float* sh_o = sh_x + 16 * RTW_LDH;        // [16][ldo]  o
  float* sh_on = sh_o + 16 * ldo;           // [16][ldo]  o_hat (act) or o_next (given)
  float* sh_t = sh_on + 16 * ldo;           // [16][AMAX+1] teammate logits
  float* sh_p = sh_t + 16 * (RTW_AMAX + 1); // [16][NMAX] attention weights
  float* sh_ps = sh_p + 16 * RTW_NMAX;      // [16] sum_j p_j
  int* sh_a = (int*)(sh_ps + 16);           // [16][NMAX] a_j (act) / u_j (given); -1 = masked one-hot block

  // ---- load the tile: h, o (and o_next); rows past the tile / past G are zeros and never stored.  Every load here addresses
  // a row as (environment g, agent r % N), h included: head_tile::load_h has the other heads' flat row addressing
  for (int idx = l; idx < 16 * RTW_H; idx += 64) {
    const int r = idx / RTW_H, c = idx % RTW_H, g = g0 + r / N;
    sh_h[r * RTW_LDH + c] = (r < R && g < p.G) ? p.h[((long)g * N + r % N) * RTW_H + c] : 0.0f;
  }
  for (int idx = l; idx < 16 * OP; idx += 64) {
    const int r = idx / OP, c = idx % OP, g = g0 + r / N;
    const bool ok = r < R && g < p.G && c < O;
    const long b = ok ? g / p.T : 0, t = ok ? g % p.T : 0;
    sh_o[r * ldo + c] = ok ? p.obs[((b * p.obs_bs) + (t + p.obs_t0) * N + r % N) * (long)O + c] : 0.0f;
    if (GIVEN) sh_on[r * ldo + c] = ok ? p.onext[((b * p.on_bs) + (t + p.on_t0) * N + r % N) * (long)O + c] : 0.0f;
  }
  if (GIVEN) {
    for (int idx = l; idx < 16 * RTW_NMAX; idx += 64) {
      const int r = idx / RTW_NMAX, j = idx % RTW_NMAX, g = g0 + r / N;
      int a = -1;
      if (r < R && g < p.G && j < N && !(NOT_SELF && j == r % N)) {
        const long b = g / p.T, t = g % p.T;
        a = p.u[b * p.u_bs + (t + p.u_t0) * N + j];
        a = a < 0 ? 0 : (a >= p.A ? p.A - 1 : a);   // padded steps carry action 0 (rollout.py:122-133 pads u with zeros)
      }
      sh_a[idx] = a;
    }
  }
  __syncthreads();

  const marl_rtw_weights_t& w = p.w;
  if (!GIVEN) {
    // ---- teammate net: P = h T0[:, :64]^T + b0 (shared by every j)
    const int ldt0 = RTW_H + N;
    for (int n0 = 0; n0 < RTW_H; n0 += 16) {
      f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_h, RTW_LDH, RTW_H, w.t0_w, ldt0, 0, n0, RTW_H);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_P[drow(r) * RTW_LDH + n0 + m] = acc[r] + w.t0_b[n0 + m];
    }
    __syncthreads();
    for (int j = 0; j < N; ++j) {
      // x_j = relu(P + T0[:, 64 + j]); the self row's input is zeroed when not_self_model: relu(b0)
      for (int idx = l; idx < 16 * RTW_H; idx += 64) {
        const int r = idx / RTW_H, c = idx % RTW_H;
        const float v = (NOT_SELF && j == r % N) ? w.t0_b[c] : sh_P[r * RTW_LDH + c] + w.t0_w[(long)c * ldt0 + RTW_H + j];
        sh_x[r * RTW_LDH + c] = fmaxf(v, 0.0f);
      }
      __syncthreads();
      for (int n0 = 0; n0 < A; n0 += 16) {
        f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_x, RTW_LDH, RTW_H, w.t2_w, RTW_H, 0, n0, A);
        if (n0 + m < A) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sh_t[drow(r) * (RTW_AMAX + 1) + n0 + m] = acc[r] + w.t2_b[n0 + m];
        }
      }
      __syncthreads();
      // first-index argmax with unavailable actions of agent j at -1e9 (RTW.py:94-95)
      if (l < 16) {
        const int r = l, g = g0 + r / N;
        int best = 0;
        if (r < R && g < p.G) {
          const long b = g / p.T, t = g % p.T;
          const float* av = p.avail + ((b * p.av_bs) + (t + p.av_t0) * N + j) * (long)A;
          float bv = 0.0f;
          for (int a = 0; a < A; ++a) {
            const float v = av[a] == 0.0f ? -1e9f : sh_t[r * (RTW_AMAX + 1) + a];
            if (a == 0 || v > bv) { bv = v; best = a; }
          }
          if (p.a_out) p.a_out[((long)g * N + r % N) * N + j] = best;
        }
        sh_a[r * RTW_NMAX + j] = (NOT_SELF && j == r % N) ? -1 : best;
      }
      __syncthreads();
    }
    // ---- world net: o_hat = W2 relu(W0 [o ; m_0 .. m_{N-1}] + b0) + b2
    const int ldw0 = O + N * A;
    for (int n0 = 0; n0 < RTW_H; n0 += 16) {
      f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_o, ldo, O, w.w0_w, ldw0, 0, n0, RTW_H);
      const int c = n0 + m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = drow(r);
        float v = acc[r] + w.w0_b[c];
        for (int j = 0; j < N; ++j) {
          const int a = sh_a[row * RTW_NMAX + j];
          if (a >= 0) v += w.w0_w[(long)c * ldw0 + O + j * A + a];
        }
        sh_x[row * RTW_LDH + c] = fmaxf(v, 0.0f);
      }
    }
    __syncthreads();
    for (int n0 = 0; n0 < OP; n0 += 16) {
      f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_x, RTW_LDH, RTW_H, w.w2_w, RTW_H, 0, n0, O);
      const int c = n0 + m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = drow(r), g = g0 + row / N;
        const float v = c < O ? acc[r] + w.w2_b[c] : 0.0f;
        sh_on[row * ldo + c] = v;
        if (p.ohat_out && c < O && row < R && g < p.G) p.ohat_out[((long)g * N + row % N) * O + c] = v;
      }
    }
    __syncthreads();
  }

  // ---- query = Wq [o ; o_next or o_hat] + bq, scaled by 1 / sqrt(attn_dim) = 1/8 as the score uses it (RTW.py:111)
  for (int n0 = 0; n0 < RTW_H; n0 += 16) {
    f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_o, ldo, O, w.wq_w, 2 * O, 0, n0, RTW_H);
    acc = tile_gemm<true>(acc, sh_on, ldo, O, w.wq_w, 2 * O, O, n0, RTW_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_x[drow(r) * RTW_LDH + n0 + m] = (acc[r] + w.wq_b[n0 + m]) / 8.0f;
  }
  // ---- value pre-activation V0[:, :64] h + bv0 of every row of the tile
  for (int n0 = 0; n0 < RTW_H; n0 += 16) {
    f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_h, RTW_LDH, RTW_H, w.v0_w, RTW_H + A, 0, n0, RTW_H);
#pragma unroll
    for (int r = 0; r < 4; ++r) sh_P[drow(r) * RTW_LDH + n0 + m] = acc[r] + w.v0_b[n0 + m];
  }
  __syncthreads();
  // ---- scores s_j = query . (Wk[:, a_j] + bk), self at -1e9 (RTW.py:113-114, :188-190); softmax over j
  for (int idx = l; idx < 16 * N; idx += 64) {
    const int r = idx / N, j = idx % N;
    const int a = sh_a[r * RTW_NMAX + j];
    float s = 0.0f;
    for (int c = 0; c < RTW_H; ++c) {
      const float key = w.wk_b[c] + (a >= 0 ? w.wk_w[(long)c * A + a] : 0.0f);
      s = fmaf(sh_x[r * RTW_LDH + c], key, s);
    }
    sh_p[r * RTW_NMAX + j] = (NOT_SELF && j == r % N) ? -1e9f : s;
  }
  __syncthreads();
  if (l < 16) {
    float mx = -INFINITY, sum = 0.0f;
    for (int j = 0; j < N; ++j) mx = fmaxf(mx, sh_p[l * RTW_NMAX + j]);
    for (int j = 0; j < N; ++j) {
      const float e = expf(sh_p[l * RTW_NMAX + j] - mx);
      sh_p[l * RTW_NMAX + j] = e;
      sum += e;
    }
    float ps = 0.0f;
    for (int j = 0; j < N; ++j) {
      const float pj = sh_p[l * RTW_NMAX + j] / sum;
      sh_p[l * RTW_NMAX + j] = pj;
      ps += pj;
    }
    sh_ps[l] = ps;
  }
  __syncthreads();
  // ---- g = sum_j p_j relu(Vpre[row of v_j] + V0[:, 64 + a_j]); act mode v_j uses h_i, given mode h_j (RTW.py:122)
  const int ldv0 = RTW_H + A;
  for (int idx = l; idx < 16 * RTW_H; idx += 64) {
    const int r = idx / RTW_H, c = idx % RTW_H;
    float gsum = 0.0f;
    for (int j = 0; j < N; ++j) {
      const int a = sh_a[r * RTW_NMAX + j];
      const int vrow = GIVEN ? (r / N) * N + j : r;
      const float pre = sh_P[vrow * RTW_LDH + c] + (a >= 0 ? w.v0_w[(long)c * ldv0 + RTW_H + a] : 0.0f);
      gsum = fmaf(sh_p[r * RTW_NMAX + j], fmaxf(pre, 0.0f), gsum);
    }
    sh_x[r * RTW_LDH + c] = gsum;
  }
  __syncthreads();
  // ---- q += V2 g + bv2 * sum_j p_j
  for (int n0 = 0; n0 < A; n0 += 16) {
    f32x4 acc = tile_gemm<true>(f32x4{0, 0, 0, 0}, sh_x, RTW_LDH, RTW_H, w.v2_w, RTW_H, 0, n0, A);
    const int c = n0 + m;
    if (c < A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = drow(r), g = g0 + row / N;
        if (row < R && g < p.G) {
          float* qp = p.q + ((long)g * N + row % N) * A + c;
          *qp = *qp + acc[r] + w.v2_b[c] * sh_ps[row];
        }
      }
    }
  }
}

size_t rtw_lds_bytes(int O) {
  const int ldo = rtw_op(O) + 4;
  return sizeof(float) * (3 * 16 * RTW_LDH + 2 * 16 * ldo + 16 * (RTW_AMAX + 1) + 16 * RTW_NMAX + 16) + sizeof(int) * 16 * RTW_NMAX;
}

template <bool GIVEN, bool NS>
int rtw_launch(const RtwArgs& a, void* stream) {
  const int EPT = RTW_NMAX / a.N;
  const int blocks = (a.G + EPT - 1) / EPT;
  if (blocks == 0) return 0;
  hipLaunchKernelGGL((rtw_head_kernel<GIVEN, NS>), dim3(blocks), dim3(64), rtw_lds_bytes(a.O), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

bool rtw_weights_ok(const marl_rtw_weights_t* w) {
  const float* ps[] = {w->t0_w, w->t0_b, w->t2_w, w->t2_b, w->w0_w, w->w0_b, w->w2_w, w->w2_b,
                       w->wq_w, w->wq_b, w->wk_w, w->wk_b, w->v0_w, w->v0_b, w->v2_w, w->v2_b};
  for (const float* q : ps)
    if (!q) return false;
  return true;
}

}  // namespace

extern "C" int marl_rtw_supported(int N, int O, int A, int H, int hidden_dim, int attn_dim) {
  return H == RTW_H && hidden_dim == RTW_H && attn_dim == RTW_H && N >= 1 && N <= RTW_NMAX && A >= 1 && A <= RTW_AMAX &&
         O >= 1 && O <= RTW_OMAX;
}

extern "C" int marl_rtw_head_act(const marl_rtw_weights_t* w, const float* h, const float* obs, long obs_bs, int obs_t0,
                                 const float* avail, long av_bs, int av_t0, float* q, int* a_out, float* ohat_out, int E,
                                 int N, int O, int A, int not_self_model, void* stream) {
  if (!w || !rtw_weights_ok(w) || !h || !obs || !avail || !q || E < 0 || !marl_rtw_supported(N, O, A, 64, 64, 64))
    return (int)hipErrorInvalidValue;
  RtwArgs a{};
  a.w = *w;
  a.h = h; a.obs = obs; a.obs_bs = obs_bs; a.obs_t0 = obs_t0;
  a.avail = avail; a.av_bs = av_bs; a.av_t0 = av_t0;
  a.q = q; a.a_out = a_out; a.ohat_out = ohat_out;
  a.G = E; a.T = 1; a.N = N; a.O = O; a.A = A;
  return not_self_model ? rtw_launch<false, true>(a, stream) : rtw_launch<false, false>(a, stream);
}

extern "C" int marl_rtw_head_given(const marl_rtw_weights_t* w, const float* hs, const float* obs, long obs_bs, int obs_t0,
                                   const float* obs_next, long on_bs, int on_t0, const int* u, long u_bs, int u_t0, float* q,
                                   int B, int T, int N, int O, int A, int not_self_model, void* stream) {
  if (!w || !rtw_weights_ok(w) || !hs || !obs || !obs_next || !u || !q || B < 0 || T < 1 ||
      !marl_rtw_supported(N, O, A, 64, 64, 64))
    return (int)hipErrorInvalidValue;
  RtwArgs a{};
  a.w = *w;
  a.h = hs; a.obs = obs; a.obs_bs = obs_bs; a.obs_t0 = obs_t0;
  a.onext = obs_next; a.on_bs = on_bs; a.on_t0 = on_t0;
  a.u = u; a.u_bs = u_bs; a.u_t0 = u_t0;
  a.q = q;
  a.G = B * T; a.T = T; a.N = N; a.O = O; a.A = A;
  return not_self_model ? rtw_launch<true, true>(a, stream) : rtw_launch<true, false>(a, stream);
}
