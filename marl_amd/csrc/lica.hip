// LICA's mixing critic (Zhou et al. 2020), the row kernels: a hypernetwork mixer whose input is the agents' action distributions.
// Per row, with x in R^K (K = N A, agent-major) and hy = [ W1 (K E, k-major) | b1 (E) | wf (E) | b2 (1) ]:
//   pre_e = b1_e + sum_k x_k W1[k, e],  h_e = relu(pre_e),  Q = sum_e h_e wf_e + b2            (no abs(): the critic is not monotonic)
// Backward, g = dL/dQ, dpre_e = g wf_e [pre_e > 0] (pre is recomputed):
//   dW1[k, e] = x_k dpre_e,  db1 = dpre,  dwf_e = g h_e,  dx_k = sum_e W1[k, e] dpre_e;  db2 = g is the caller's.
// The input is dense x (rows, K) or the taken actions u (rows N): with u only the N taken rows of W1 are read, the one-hot vector is
// never built, and dW1 gets dpre in the taken blocks and exact zeros in the others.
//
// Lane mapping.  Every row has a K x E matrix of its own (7 KB at 2s3z, up to 128 KB in the support corner), so there is no matrix
// shape shared across rows and W1 is streamed through registers, never staged.  A workgroup owns a tile of TR consecutive rows; a
// lane owns (row, four consecutive e): the EQ = ceil(E / 4) lanes of a row read one 4 E-byte line of W1 per k, 16 bytes a lane
// (single floats when E, ldh or the base leave no 16-byte pitch), and walk k = 0 .. K - 1 with the four sums in registers - every
// sum adds its products in k order.  The small operands go through LDS tiles with odd pitches: x (or u), the 2 E + 1 tail of hy,
// the products h_e wf_e (one lane per row adds them in e order: Q, the TD loss, g), dpre.  dW1 leaves from the same lanes the way
// W1 came in.  dx runs a second mapping, one lane per (row, k): the lane reads its 4 E-byte line of W1 in 16-byte pieces against
// dpre in LDS and adds in e order.  TR is the largest tile with TR EQ <= 256 lanes, TR <= 64 rows and 76 KB of LDS: 32 rows at
// E = 32 (30 at K = 512), 16 at E = 64.  marl_lica_plan reports it.
//
// The three entry points are one kernel template, fp contraction off for the whole file (but the TD loss's expressions, which are
// contracted as mixers.hip's): the loss-folded launch gives the bits of mix_fwd -> marl_td_loss -> mix_bwd.  Its two sums are taken
// by a small pass over the Q it wrote, with marl_td_loss's own partition of the rows: a sum per row tile could not have its bits.
#include "common.h"
#include "sums.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

#pragma clang fp contract(off)

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;
constexpr int MAXN = 16, MAXA = 32, MAXE = 64;         // the support range
constexpr int MAX_TILE = 64;                           // rows per tile at most
constexpr size_t LDS_CAP = 76 * 1024;                  // two workgroups in a CU's 160 KB

enum { MODE_FWD = 0, MODE_BWD = 1, MODE_LOSS = 2 };

// LDS image of a tile, floats: x or u [TR][XP] | tail of hy [TR][TP] | h wf [TR][EP] | dpre [TR][EP] | g [TR] | live [TR]
struct Tile { int TR, EQ, XP, TP, EP; size_t lds; };
inline Tile tile_of(int N, int A, int E) {
  Tile t;
  t.EQ = (E + 3) / 4;
  t.XP = (N * A) | 1;
  t.TP = (2 * E + 1) | 1;
  t.EP = E | 1;
  const size_t row = (size_t)(t.XP + t.TP + 2 * t.EP + 2) * sizeof(float);
  long tr = (long)(LDS_CAP / row);
  if (tr > MAX_TILE) tr = MAX_TILE;
  if (tr > TPB / t.EQ) tr = TPB / t.EQ;
  t.TR = (int)(tr < 1 ? 1 : tr);
  t.lds = row * t.TR;
  return t;
}

struct LiArgs {
  const float* hy; long ldh;                 // (rows, ldh): [W1 (K E) | b1 (E) | wf (E) | b2 (1)]
  const float* x;                            // (rows, K) or NULL
  const int* u;                              // (rows N) or NULL
  const float* g_in;                         // MODE_BWD: dL/dQ (rows)
  const float *q_tgt, *r, *term, *padded;    // MODE_LOSS
  float gamma;
  float* q;                                  // (rows); unused in MODE_BWD
  float* dhy; long lddh;                     // (rows, lddh): [dW1 (K E) | db1 (E) | dwf (E)] or NULL
  float* dx;                                 // (rows, K) or NULL
  float* dq_tot;                             // MODE_LOSS: (rows)
  long rows;
  int N, A, E, TR, EQ, XP, TP, EP;
};

// four consecutive floats (cnt < 4 only without vec: the short last piece of an odd E)
template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* p, int cnt) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) v[j] = p[j];
  return v;
}
template <bool VEC>
__device__ __forceinline__ void st4(float* p, const f32x4& v, int cnt) {
  if (VEC) { *reinterpret_cast<f32x4*>(p) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt) p[j] = v[j];
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(TPB) void lica_kernel(LiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float li_smem[];
  const int N = a.N, A = a.A, E = a.E, TR = a.TR, EQ = a.EQ, XP = a.XP, TP = a.TP, EP = a.EP;
  const int K = N * A, KE = K * E, TL = 2 * E + 1;
  float* Xs = li_smem;
  int* Us = reinterpret_cast<int*>(li_smem);           // the taken actions lie where x would
  float* Ts = Xs + (size_t)TR * XP;
  float* Pr = Ts + (size_t)TR * TP;
  float* Dp = Pr + (size_t)TR * EP;
  float* Gs = Dp + (size_t)TR * EP;
  int* Lv = reinterpret_cast<int*>(Gs + TR);
  const int tid = threadIdx.x;
  const int rl = tid / EQ, e0 = 4 * (tid - rl * EQ);
  const int cnt = E - e0 < 4 ? E - e0 : 4;
  for (long r0 = (long)blockIdx.x * TR; r0 < a.rows; r0 += (long)gridDim.x * TR) {
    const int nr = (int)(a.rows - r0 < TR ? a.rows - r0 : TR);
    // ---- stage the small operands
    if (a.u) {
      for (int i = tid; i < nr * N; i += TPB) { const int row = i / N; Us[row * XP + (i - row * N)] = a.u[r0 * N + i]; }
    } else {
      for (int i = tid; i < nr * K; i += TPB) { const int row = i / K; Xs[row * XP + (i - row * K)] = a.x[r0 * K + i]; }
    }
    for (int i = tid; i < nr * TL; i += TPB) {
      const int row = i / TL, c = i - row * TL;
      Ts[row * TP + c] = a.hy[(r0 + row) * a.ldh + KE + c];
    }
    __syncthreads();
    // ---- (row, four e): pre, and the products h wf
    const bool act = rl < nr;
    float pre[4] = {0.f, 0.f, 0.f, 0.f};
    if (act) {
      const float* W = a.hy + (r0 + rl) * a.ldh + e0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) pre[j] = Ts[rl * TP + e0 + j];
      if (a.u) {
        for (int i = 0; i < N; ++i) {
          const int uu = Us[rl * XP + i];
          if ((unsigned)uu < (unsigned)A) {              // x_k = 1 on the taken action: 1 w = w
            const f32x4 w = ld4<VEC>(W + (long)(i * A + uu) * E, cnt);
#pragma unroll
            for (int j = 0; j < 4; ++j) pre[j] += w[j];
          }
        }
      } else {
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
          const float xk = Xs[rl * XP + k];
          const f32x4 w = ld4<VEC>(W + (long)k * E, cnt);
#pragma unroll
          for (int j = 0; j < 4; ++j) pre[j] += xk * w[j];
        }
      }
      if (MODE != MODE_BWD) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) Pr[rl * EP + e0 + j] = (pre[j] > 0.f ? pre[j] : 0.f) * Ts[rl * TP + E + e0 + j];
      }
    }
    __syncthreads();
    // ---- row: Q, and the gradient on it
    if (tid < nr) {
      const long r = r0 + tid;
      float g = 0.f;
      int live = 1;
      if (MODE != MODE_BWD) {
        float qv = 0.f;
        for (int e = 0; e < E; ++e) qv += Pr[tid * EP + e];
        qv += Ts[tid * TP + 2 * E];
        if (a.q) a.q[r] = qv;
        if (MODE == MODE_LOSS) {                 // td_loss_kernel's expressions (mixers.hip), contracted as that file's are
#pragma clang fp contract(fast)
          const float mask = 1.f - a.padded[r];
          live = mask != 0.f;
          if (live) {
            const float target = a.r[r] + a.gamma * a.q_tgt[r] * (1.f - a.term[r]);
            const float td = target - qv;
            const float mtd = mask * td;
            g = -2.f * mask * mtd;
          }                                      // a padded row: its Q, r and target enter nothing; g = 0
          a.dq_tot[r] = g;
        }
      } else {
        g = a.g_in[r];
      }
      if (MODE != MODE_FWD) { Gs[tid] = g; Lv[tid] = live; }
    }
    if (MODE != MODE_FWD) {
      __syncthreads();
      // ---- (row, four e): dpre, and the row of dhy
      if (act) {
        const float g = Gs[rl];
        const bool live = Lv[rl] != 0;
        f32x4 dp = {0.f, 0.f, 0.f, 0.f}, dwf = {0.f, 0.f, 0.f, 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt && live && pre[j] > 0.f) {
            dp[j] = g * Ts[rl * TP + E + e0 + j];
            dwf[j] = g * pre[j];
          }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) Dp[rl * EP + e0 + j] = dp[j];
        if (a.dhy) {
          float* D = a.dhy + (r0 + rl) * a.lddh + e0;
          if (a.u) {
            for (int i = 0; i < N; ++i) {
              const int uu = Us[rl * XP + i];
              for (int c = 0; c < A; ++c) st4<VEC>(D + (long)(i * A + c) * E, c == uu ? dp : zero, cnt);
            }
          } else {
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
              const float xk = Xs[rl * XP + k];
              const f32x4 v = {xk * dp[0], xk * dp[1], xk * dp[2], xk * dp[3]};
              st4<VEC>(D + (long)k * E, v, cnt);
            }
          }
          st4<VEC>(D + KE, dp, cnt);
          st4<VEC>(D + KE + E, dwf, cnt);
        }
      }
      if (a.dx) {
        __syncthreads();
        // ---- (row, k): dx_k = sum_e W1[k, e] dpre_e, in e order
        for (int it = tid; it < nr * K; it += TPB) {
          const int row = it / K, k = it - row * K;
          const float* W = a.hy + (r0 + row) * a.ldh + (long)k * E;
          const float* d = Dp + row * EP;
          float s = 0.f;
          for (int e = 0; e < E; e += 4) {
            const int c = E - e < 4 ? E - e : 4;
            const f32x4 w = ld4<VEC>(W + e, c);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < c) s += w[j] * d[e + j];
          }
          a.dx[(r0 + row) * K + k] = s;
        }
      }
    }
    __syncthreads();                             // the tile is free for the next round
  }
}

// The two loss sums, after the row launch: td_loss_kernel's loop (mixers.hip) over the Q just written - the same rows per thread,
// the same expressions, the same partials - so that out2 has marl_td_loss's bits; a padded row adds nothing and is not looked at
__global__ __launch_bounds__(TPB) void lica_td_sums_kernel(const float* q, const float* q_tgt, const float* r, const float* term,
                                                           const float* padded, float gamma, float* ws, long rows) {
#pragma clang fp contract(fast)
  float acc[2] = {0.f, 0.f};
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < rows; i += (long)gridDim.x * TPB) {
    const float mask = 1.f - padded[i];
    if (mask == 0.f) continue;
    const float target = r[i] + gamma * q_tgt[i] * (1.f - term[i]);
    const float td = target - q[i];
    const float mtd = mask * td;
    acc[0] += mtd * mtd;
    acc[1] += mask;
  }
  block_partials<2>(acc, ws);
}

inline bool shape_ok(int N, int A, int E) { return N >= 1 && N <= MAXN && A >= 1 && A <= MAXA && E >= 1 && E <= MAXE; }
inline int grid_of(long rows, int TR) {
  const long t = (rows + TR - 1) / TR;
  return (int)(t > rt::PARTIAL_ROWS ? rt::PARTIAL_ROWS : t);        // the loss workspace holds this many rows of partials
}
inline bool float_base(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <int MODE>
int launch(LiArgs& a, hipStream_t stream) {
  if (!shape_ok(a.N, a.A, a.E) || a.rows >= (1L << 31)) return (int)hipErrorInvalidValue;
  const long KE = (long)a.N * a.A * a.E;
  if (!a.hy || !float_base(a.hy) || a.ldh < KE + 2 * a.E + 1 || (a.x != nullptr) == (a.u != nullptr))
    return (int)hipErrorInvalidValue;
  if (MODE != MODE_FWD && ((!a.dhy && !a.dx) || (a.dhy && (a.lddh < KE + 2 * a.E || !float_base(a.dhy)))))
    return (int)hipErrorInvalidValue;
  const Tile t = tile_of(a.N, a.A, a.E);
  a.TR = t.TR; a.EQ = t.EQ; a.XP = t.XP; a.TP = t.TP; a.EP = t.EP;
  // 16-byte accesses to hy and dhy where the bases, the leading dimensions and E allow them, single floats otherwise
  const bool vec = a.E % 4 == 0 && aligned16(a.hy) && a.ldh % 4 == 0 && (!a.dhy || (aligned16(a.dhy) && a.lddh % 4 == 0));
  const void* fn = vec ? (const void*)lica_kernel<MODE, true> : (const void*)lica_kernel<MODE, false>;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {(void*)&a};
  e = hipLaunchKernel(fn, dim3((unsigned)grid_of(a.rows, t.TR)), dim3(TPB), kargs, t.lds, stream);
  if (e != hipSuccess) return (int)e;
  MARL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int marl_lica_supported(int N, int A, int E) { return shape_ok(N, A, E) ? 1 : 0; }

extern "C" int marl_lica_plan(long rows, int N, int A, int E, int* plan) {
  if (!plan || !shape_ok(N, A, E) || rows >= (1L << 31)) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 4; ++i) plan[i] = 0;
  if (rows <= 0) return 0;
  const Tile t = tile_of(N, A, E);
  plan[0] = t.TR;
  plan[1] = grid_of(rows, t.TR);
  plan[2] = (int)t.lds;
  const long tiles = (rows + t.TR - 1) / t.TR;
  plan[3] = (int)((tiles + plan[1] - 1) / plan[1]);
  return 0;
}

extern "C" int marl_lica_mix_fwd(const float* hy, long ldh, const float* x, const int* u, float* q, long rows, int N, int A, int E,
                                 void* stream) {
  if (rows <= 0) return 0;
  if (!q) return (int)hipErrorInvalidValue;
  LiArgs a = {};
  a.hy = hy; a.ldh = ldh; a.x = x; a.u = u; a.q = q; a.rows = rows; a.N = N; a.A = A; a.E = E;
  return launch<MODE_FWD>(a, (hipStream_t)stream);
}

extern "C" int marl_lica_mix_bwd(const float* hy, long ldh, const float* x, const int* u, const float* dq, float* dhy, long lddh,
                                 float* dx, long rows, int N, int A, int E, void* stream) {
  if (rows <= 0) return 0;
  if (!dq) return (int)hipErrorInvalidValue;
  LiArgs a = {};
  a.hy = hy; a.ldh = ldh; a.x = x; a.u = u; a.g_in = dq; a.dhy = dhy; a.lddh = lddh; a.dx = dx;
  a.rows = rows; a.N = N; a.A = A; a.E = E;
  return launch<MODE_BWD>(a, (hipStream_t)stream);
}

extern "C" int marl_lica_loss_bwd(const float* hy, long ldh, const int* u, const float* q_tgt, const float* r, const float* term,
                                  const float* padded, float gamma, float* q, float* dhy, long lddh, float* dq_tot, float* out2,
                                  float* ws, long rows, int N, int A, int E, void* stream) {
  if (rows <= 0) return 0;
  if (!u || !q_tgt || !r || !term || !padded || !q || !dhy || !dq_tot || !out2 || !ws) return (int)hipErrorInvalidValue;
  LiArgs a = {};
  a.hy = hy; a.ldh = ldh; a.u = u; a.q_tgt = q_tgt; a.r = r; a.term = term; a.padded = padded; a.gamma = gamma;
  a.q = q; a.dhy = dhy; a.lddh = lddh; a.dq_tot = dq_tot;
  a.rows = rows; a.N = N; a.A = A; a.E = E;
  const int rc = launch<MODE_LOSS>(a, (hipStream_t)stream);
  if (rc) return rc;
  const int nb = rt::partial_blocks(rows);
  hipLaunchKernelGGL(lica_td_sums_kernel, dim3(nb), dim3(TPB), 0, (hipStream_t)stream, (const float*)q, q_tgt, r, term, padded, gamma,
                     ws, rows);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 2, out2);
  MARL_CHECK_LAUNCH();
  return 0;
}
