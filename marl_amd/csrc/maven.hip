// MAVEN (Mahajan et al., NeurIPS 2019), the three device parts of this project's own definition (include/marl_hip.h):
//   the episode noise draw, the noise-conditioned agent head  q' = q + (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n]  and its
//   backward, and the mutual-information pass: a discriminator over [softmax of the masked q' rows | state] of every step, its cross
//   entropy against the episode's noise index, and the whole backward down to the dense gradient on q' - one row launch.
//
// Head.  The rows of one (episode b, agent n) over t share one A x 64 matrix, so a work item is (b, n, 16 consecutive t): one wave
// holds the 16 h rows in LDS and multiplies them with the matrix on the fp32 matrix cores (mfma16x4, the K-permutation of
// head_tile.h).  A rollout step is the same kernel with T = 1 (one live row per tile).  An episode whose noise index is outside
// [0, K) is skipped whole: its q rows are not touched (forward), its dhs rows are zeros and it adds to no table gradient (backward).
//
// Head backward.  g = scatter(dq_idx, dq_val) + dq_dense is written out dense (BPTT's dq: fc2's gradient) and staged per tile;
// dhs = g (noise_w[k] + id_w[n]) and P(b, n) = sum_t g_t h_t^T are MFMA products, the second contracted over t.  A workgroup (one
// wave) owns a slab of the workspace - [d noise_w | d id_w | d noise_b | d id_b] - and walks the episodes b = slab, slab + slabs, ..
// in order, adding P(b, n) into its id_w[n] block and sum_n P(b, n) into its noise_w[k_b] block: the same lane adds to the same
// address every time.  A second kernel adds the slabs in slab order into the gradient views.  No float atomics anywhere.
//
// MI pass.  A workgroup of four waves owns tiles of 16 steps.  Per tile: x = [p | s] is built in LDS (never in HBM) from q', the
// availability and the state rows read in place through the episode map; wave w owns columns 16 w .. 16 w + 15 of the D = 64 hidden
// units.  h1, the logits, dlogits, dh1, dW1 (read-modify-write of the workgroup's slab, 16 x 16 accumulator tiles seeded from it),
// dW2 / db1 / db2 (registers across the tiles, stored once), dx over the probability columns and the softmax backward follow, with
// the W1 operands read through L2.  Everything is scaled by lambda_mi (1 - padded); padded steps, rows beyond the batch and steps of
// an episode with an out-of-range noise index read nothing and give exact zeros.
#include "common.h"
#include "sums.h"
#include "synth_env.h"
#include "../../include/marl_hip.h"

// loops with runtime bounds stay as written: unrolled and vectorised copies of them cost the MI kernel its scalar registers
#define SCALAR_LOOP _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")

namespace {

constexpr unsigned ST_MAVEN = 24;                      // the counter hash's stream of the episode noise (0..9 and 16..19 are taken)
constexpr int HD = 64;                                 // rnn_hidden_dim, and the discriminator's width D
constexpr int MAXN = 16, MAXA = 32, MAXK = 32;         // the support range
constexpr int HP = HD + 4;                             // LDS pitch of 64-wide tiles
constexpr int GP = MAXA + 4;                           // LDS pitch of action- / noise-wide tiles
constexpr int MAX_SLABS = 256;
constexpr size_t HEAD_WS_CAP = 64u << 20;              // the head backward's slabs take at most this many bytes
constexpr size_t MI_LDS_CAP = 96 * 1024;
constexpr int MI_TPB = SUMS_TPB;

inline int round16(int n) { return (n + 15) / 16 * 16; }
inline bool head_shape_ok(int N, int A, int K) { return N >= 1 && N <= MAXN && A >= 1 && A <= MAXA && K >= 1 && K <= MAXK; }

// ---------------------------------------------------------------- noise
__global__ __launch_bounds__(256) void maven_noise_kernel(unsigned seed, int env0, unsigned tg0, int K, int* noise, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < E) noise[e] = (int)(hkey(seed, ST_MAVEN, (unsigned)(env0 + e), tg0, 0u) % (unsigned)K);
}

// ---------------------------------------------------------------- head
struct HeadArgs {
  const float *noise_w, *id_w, *noise_b, *id_b;
  float *g_noise_w, *g_id_w, *g_noise_b, *g_id_b;
  const float* hs;
  const int* noise;
  float* q;
  const int* dq_idx;
  const float *dq_val, *dq_dense;
  float *dq_out, *dhs, *ws;
  long slab_len, items;
  int B, T, N, A, K, tt;
};

// Hs[16][HP] <- the h rows of steps t0 .. t0 + nr - 1 of (b, n); rows beyond nr are zeros
__device__ __forceinline__ void load_h_tile(float* Hs, const float* hs, int b, int n, int t0, int nr, int T, int N) {
  SCALAR_LOOP
  for (int idx = threadIdx.x; idx < 16 * (HD / 4); idx += 64) {
    const int r = idx / (HD / 4), c = (idx % (HD / 4)) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < nr) v = *reinterpret_cast<const f32x4*>(hs + (((long)b * T + t0 + r) * N + n) * HD + c);
    *reinterpret_cast<f32x4*>(Hs + r * HP + c) = v;
  }
}

__global__ __launch_bounds__(64) void maven_head_fwd_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float Hs[16 * HP];
  const int l = threadIdx.x, m = l & 15, q4 = (l >> 4) * 4;
  const int T = a.T, N = a.N, A = a.A;
  SCALAR_LOOP
  for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
    const int tile = (int)(it % a.tt);
    const long bn = it / a.tt;
    const int n = (int)(bn % N), b = (int)(bn / N);
    const int k = a.noise[b];
    if (k < 0 || k >= a.K) continue;                   // the same for the whole wave
    const int t0 = tile * 16, nr = T - t0 < 16 ? T - t0 : 16;
    load_h_tile(Hs, a.hs, b, n, t0, nr, T, N);
    __syncthreads();
    const float* Wk = a.noise_w + (long)k * A * HD;
    const float* Wn = a.id_w + (long)n * A * HD;
    SCALAR_LOOP
    for (int a0 = 0; a0 < A; a0 += 16) {
      const int col = a0 + m;
      const bool cok = col < A;
      const float* wk = Wk + (long)(cok ? col : 0) * HD;
      const float* wn = Wn + (long)(cok ? col : 0) * HD;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < HD; k0 += 16) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(Hs + m * HP + k0 + q4);
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (cok) w = *reinterpret_cast<const f32x4*>(wk + k0 + q4) + *reinterpret_cast<const f32x4*>(wn + k0 + q4);
        acc = mfma16x4(x, w, acc);
      }
      if (cok) {
        const float bias = a.noise_b[k * A + col] + a.id_b[n * A + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = q4 + r;
          if (row < nr) a.q[(((long)b * T + t0 + row) * N + n) * A + col] += acc[r] + bias;
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void maven_head_bwd_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float Hs[16 * HP];
  __shared__ __attribute__((aligned(16))) float Gs[16 * GP];
  const int l = threadIdx.x, m = l & 15, q4 = (l >> 4) * 4;
  const int T = a.T, N = a.N, A = a.A, K = a.K;
  float* sl = a.ws + (long)blockIdx.x * a.slab_len;
  SCALAR_LOOP
  for (long i = l; i < a.slab_len; i += 64) sl[i] = 0.f;
  __syncthreads();
  // the slab: [d noise_w (K A 64) | d id_w (N A 64) | d noise_b (K A) | d id_b (N A)]
  SCALAR_LOOP
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int k = a.noise[b];
    const bool kok = k >= 0 && k < K;
    const float* Wk = a.noise_w + (long)(kok ? k : 0) * A * HD;
    f32x4 Pk[2][4];
#pragma unroll
    for (int ai = 0; ai < 2; ++ai)
#pragma unroll
      for (int hj = 0; hj < 4; ++hj) Pk[ai][hj] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bk = 0.f;
    SCALAR_LOOP
    for (int n = 0; n < N; ++n) {
      const float* Wn = a.id_w + (long)n * A * HD;
      f32x4 P[2][4];
#pragma unroll
      for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int hj = 0; hj < 4; ++hj) P[ai][hj] = (f32x4){0.f, 0.f, 0.f, 0.f};
      float bnv = 0.f;
      SCALAR_LOOP
      for (int t0 = 0; t0 < T; t0 += 16) {
        const int nr = T - t0 < 16 ? T - t0 : 16;
        // g of the tile: staged, and written out dense
        SCALAR_LOOP
        for (int idx = l; idx < 16 * GP; idx += 64) {
          const int r = idx / GP, c = idx - r * GP;
          float v = 0.f;
          if (r < nr && c < A) {
            const long row = ((long)b * T + t0 + r) * N + n;
            if (a.dq_dense) v = a.dq_dense[row * A + c];
            if (a.dq_idx && a.dq_idx[row] == c) v += a.dq_val[row];
            a.dq_out[row * A + c] = v;
          }
          Gs[idx] = v;
        }
        if (kok) load_h_tile(Hs, a.hs, b, n, t0, nr, T, N);
        __syncthreads();
        if (kok) {
          // dhs (16 x 64) = g (16 x A) (noise_w[k] + id_w[n]) (A x 64)
#pragma unroll
          for (int h0 = 0; h0 < HD; h0 += 16) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            SCALAR_LOOP
            for (int k0 = 0; k0 < A; k0 += 16) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(Gs + m * GP + k0 + q4);
              f32x4 w = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int kk = k0 + q4 + i;
                if (kk < A) w[i] = Wk[(long)kk * HD + h0 + m] + Wn[(long)kk * HD + h0 + m];
              }
              acc = mfma16x4(x, w, acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = q4 + r;
              if (row < nr) a.dhs[(((long)b * T + t0 + row) * N + n) * HD + h0 + m] = acc[r];
            }
          }
          // P (A x 64) += g^T h, contracted over the tile's steps
#pragma unroll
          for (int ai = 0; ai < 2; ++ai) {
            if (ai * 16 < A) {
              f32x4 x;
#pragma unroll
              for (int i = 0; i < 4; ++i) x[i] = Gs[(q4 + i) * GP + ai * 16 + m];
#pragma unroll
              for (int hj = 0; hj < 4; ++hj) {
                f32x4 w;
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = Hs[(q4 + i) * HP + hj * 16 + m];
                P[ai][hj] = mfma16x4(x, w, P[ai][hj]);
              }
            }
          }
          if (l < A)
            SCALAR_LOOP
            for (int r = 0; r < 16; ++r) bnv += Gs[r * GP + l];
        } else {
          SCALAR_LOOP
          for (int idx = l; idx < nr * HD; idx += 64) {
            const int r = idx / HD, c = idx - r * HD;
            a.dhs[(((long)b * T + t0 + r) * N + n) * HD + c] = 0.f;
          }
        }
        __syncthreads();
      }
      if (kok) {
        float* dst = sl + ((long)K + n) * A * HD;
#pragma unroll
        for (int ai = 0; ai < 2; ++ai)
#pragma unroll
          for (int hj = 0; hj < 4; ++hj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int arow = ai * 16 + q4 + r;
              if (arow < A) dst[arow * HD + hj * 16 + m] += P[ai][hj][r];
            }
            Pk[ai][hj] += P[ai][hj];
          }
        if (l < A) sl[(long)(K + N) * A * HD + (K + n) * A + l] += bnv;
        bk += bnv;
      }
    }
    if (kok) {
      float* dst = sl + (long)k * A * HD;
#pragma unroll
      for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int hj = 0; hj < 4; ++hj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int arow = ai * 16 + q4 + r;
            if (arow < A) dst[arow * HD + hj * 16 + m] += Pk[ai][hj][r];
          }
      if (l < A) sl[(long)(K + N) * A * HD + k * A + l] += bk;
    }
  }
}

// g_j[i] += the sum over the slabs, in slab order, of element i of a slab laid out as [g0 (n0) | g1 (n1) | g2 (n2) | g3 (n3)]
__global__ __launch_bounds__(256) void maven_reduce_kernel(const float* ws, long slab_len, int slabs, float* g0, long n0, float* g1,
                                                           long n1, float* g2, long n2, float* g3, long n3) {
  SCALAR_LOOP
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < slab_len; i += (long)gridDim.x * 256) {
    const float s = slab_sum(ws + i, slab_len, 0, 1, slabs);
    long j = i;
    if (j < n0) { g0[j] += s; continue; }
    j -= n0;
    if (j < n1) { g1[j] += s; continue; }
    j -= n1;
    if (j < n2) { g2[j] += s; continue; }
    j -= n2;
    if (j < n3) g3[j] += s;
  }
}

inline long head_slab_len(int N, int A, int K) { return (long)(K + N) * A * HD + (long)(K + N) * A; }
inline int head_slabs(int B, int N, int A, int K) {
  long s = (long)(HEAD_WS_CAP / (head_slab_len(N, A, K) * sizeof(float)));
  if (s > MAX_SLABS) s = MAX_SLABS;
  if (s > B) s = B;
  return (int)(s < 1 ? 1 : s);
}
inline int reduce_blocks(long n) {
  const long b = (n + 255) / 256;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

// ---------------------------------------------------------------- MI pass
struct MiTile { int XW, XK, XP, NA, QP; size_t lds; };
// LDS image, floats: h1 [16][HP] | dh1 [16][HP] | logits / dlogits [16][GP] | m [16] | k_b [16] | t [16] | episode [16] (64-bit) |
// x [16][XP] | dx [16][QP]
inline MiTile mi_tile(int N, int A, int S) {
  MiTile t;
  t.NA = N * A;
  t.XW = t.NA + S;
  t.XK = round16(t.XW);
  t.XP = t.XK + 4;
  t.QP = round16(t.NA) + 4;
  t.lds = ((size_t)16 * (t.XP + t.QP + 2 * HP + GP) + 16 * 3 + 32) * sizeof(float);
  return t;
}
inline bool mi_shape_ok(int N, int A, int K, int S, int D) {
  return head_shape_ok(N, A, K) && D == HD && S >= 1 && S <= (1 << 20) && mi_tile(N, A, S).lds <= MI_LDS_CAP;
}
inline long mi_slab_len(int N, int A, int K, int S) { return (long)HD * (N * A + S) + HD + (long)K * HD + K; }
inline int mi_grid(long rows) {
  const long t = (rows + 15) / 16;
  return (int)(t > MAX_SLABS ? MAX_SLABS : (t < 1 ? 1 : t));
}

struct MiArgs {
  const float *w1, *b1, *w2, *b2;
  const float* q;
  const float* avail; int avail_bs;
  const float* state; int state_ld, state_bs;
  const int *ep_map, *noise;
  const float* padded;
  float lambda;
  float *dq_dense, *ce, *ws;
  int slab_len, rows, T, N, A, S, K, XW, XK, XP, QP;
};

__global__ __launch_bounds__(MI_TPB) void maven_mi_kernel(MiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mv_smem[];
  const int T = a.T, N = a.N, A = a.A, K = a.K, XW = a.XW, XK = a.XK, XP = a.XP, QP = a.QP;
  const int NA = N * A;
  __builtin_assume(N >= 1 && N <= MAXN);               // the launcher's checks: no guard in front of the loops over them
  __builtin_assume(A >= 1 && A <= MAXA);
  __builtin_assume(K >= 1 && K <= MAXK);
  __builtin_assume(XW > NA && XK >= XW);
  // the tiles of a fixed size first: their offsets are constants
  float* H1 = mv_smem;
  float* DH = H1 + 16 * HP;
  float* LG = DH + 16 * HP;
  float* RM = LG + 16 * GP;
  int* RK = reinterpret_cast<int*>(RM + 16);
  int* RT = RK + 16;
  long* RE = reinterpret_cast<long*>(RT + 16);
  float* X = reinterpret_cast<float*>(RE + 16);
  float* DX = X + 16 * XP;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, m = l & 15, q4 = (l >> 4) * 4;
  const int d0 = 16 * w;
  float* sl = a.ws + 2 * MAX_SLABS + (long)blockIdx.x * a.slab_len;      // [dW1 (64 XW) | db1 (64) | dW2 (K 64) | db2 (K)]
  SCALAR_LOOP
  for (int i = tid; i < a.slab_len; i += MI_TPB) sl[i] = 0.f;
  f32x4 dW2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float dbv = 0.f;                                     // db1[tid] (tid < 64), db2[tid - 64] (64 <= tid < 64 + K)
  float acc2[2] = {0.f, 0.f};
  __syncthreads();
  SCALAR_LOOP
  for (int r0 = blockIdx.x * 16; r0 < a.rows; r0 += gridDim.x * 16) {       // rows < 2^31 / N: no overflow
    const int nr = a.rows - r0 < 16 ? a.rows - r0 : 16;
    // ---- the rows of the tile: live or not, noise index, step, episode in the store
    if (tid < 16) {
      float mm = 0.f;
      int kb = -1, t = 0;
      long e = 0;
      if (tid < nr) {
        const int i = r0 + tid;
        const int b = i / T;
        t = i - b * T;
        kb = a.noise[b];
        const float msk = 1.f - a.padded[i];
        if (msk != 0.f && kb >= 0 && kb < K) {
          mm = msk;
          e = a.ep_map ? (long)a.ep_map[b] : b;
        }
      }
      RM[tid] = mm; RK[tid] = kb; RT[tid] = t; RE[tid] = e;
    }
    __syncthreads();
    // ---- x = [softmax of the masked rows | state | zeros up to XK]
    SCALAR_LOOP
    for (int pr = tid; pr < 16 * N; pr += MI_TPB) {
      const int r = pr / N, n = pr - r * N;
      float* xp = X + r * XP + n * A;
      if (RM[r] == 0.f) {
        SCALAR_LOOP
        for (int c = 0; c < A; ++c) xp[c] = 0.f;
        continue;
      }
      const float* qr = a.q + ((long)(r0 + r) * N + n) * A;
      const float* av = a.avail + RE[r] * a.avail_bs + ((long)RT[r] * N + n) * A;
      float mx = 0.f;
      bool any = false;
      SCALAR_LOOP
      for (int c = 0; c < A; ++c)
        if (av[c] != 0.f) { mx = (!any || qr[c] > mx) ? qr[c] : mx; any = true; }
      float sum = 0.f;
      SCALAR_LOOP
      for (int c = 0; c < A; ++c) {
        const float v = av[c] != 0.f ? expf(qr[c] - mx) : 0.f;
        xp[c] = v;
        sum += v;
      }
      SCALAR_LOOP
      for (int c = 0; c < A; ++c) xp[c] = any ? xp[c] / sum : 0.f;
    }
    SCALAR_LOOP
    for (int idx = tid; idx < 16 * GP; idx += MI_TPB) LG[idx] = 0.f;      // the columns k >= K stay zeros
    {
      const int SW = XK - NA;
      SCALAR_LOOP
      for (int idx = tid; idx < 16 * SW; idx += MI_TPB) {
        const int r = idx / SW, c = idx - r * SW;
        float v = 0.f;
        if (RM[r] != 0.f && c < a.S) v = a.state[(RE[r] * a.state_bs + RT[r]) * (long)a.state_ld + c];
        X[r * XP + NA + c] = v;
      }
    }
    __syncthreads();
    // ---- h1 = relu(W1 x + b1): wave w owns hidden units d0 .. d0 + 15
    {
      const float* wr = a.w1 + (d0 + m) * XW;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      SCALAR_LOOP
      for (int k0 = 0; k0 < XK; k0 += 16) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + m * XP + k0 + q4);
        f32x4 ww;
#pragma unroll
        for (int i = 0; i < 4; ++i) ww[i] = k0 + q4 + i < XW ? __ldg(wr + k0 + q4 + i) : 0.f;
        acc = mfma16x4(x, ww, acc);
      }
      const float bias = a.b1[d0 + m];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[r] + bias;
        H1[(q4 + r) * HP + d0 + m] = v > 0.f ? v : 0.f;
      }
    }
    __syncthreads();
    // ---- logits = W2 h1 + b2
    if (d0 < K) {
      const int col = d0 + m;
      const bool cok = col < K;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < HD; k0 += 16) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(H1 + m * HP + k0 + q4);
        f32x4 ww = {0.f, 0.f, 0.f, 0.f};
        if (cok) ww = *reinterpret_cast<const f32x4*>(a.w2 + col * HD + k0 + q4);
        acc = mfma16x4(x, ww, acc);
      }
      if (cok) {
        const float bias = a.b2[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) LG[(q4 + r) * GP + col] = acc[r] + bias;
      }
    }
    __syncthreads();
    // ---- row: ce, the hit, and dlogits = lambda m (softmax - one-hot) in the place of the logits
    if (tid < 16) {
      float* row = LG + tid * GP;
      const float mm = RM[tid];
      if (mm != 0.f) {
        const int kb = RK[tid];
        float mx = row[0];
        int arg = 0;
        SCALAR_LOOP
        for (int k = 1; k < K; ++k)
          if (row[k] > mx) { mx = row[k]; arg = k; }
        float sum = 0.f;
        SCALAR_LOOP
        for (int k = 0; k < K; ++k) sum += expf(row[k] - mx);
        const float lse = mx + logf(sum);
        const float ce = lse - row[kb];
        acc2[0] += mm * ce;
        acc2[1] += arg == kb ? mm : 0.f;
        a.ce[r0 + tid] = ce;
        const float sc = a.lambda * mm;
        SCALAR_LOOP
        for (int k = 0; k < K; ++k) row[k] = sc * (expf(row[k] - lse) - (k == kb ? 1.f : 0.f));
      } else {
        if (tid < nr) a.ce[r0 + tid] = 0.f;
        SCALAR_LOOP
        for (int k = 0; k < K; ++k) row[k] = 0.f;
      }
    }
    __syncthreads();
    // ---- dW2 (registers), db2, and dh1 = (W2^T dlogits) [h1 > 0]
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (kt * 16 < K) {
        f32x4 x, hh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[i] = LG[(q4 + i) * GP + kt * 16 + m];
          hh[i] = H1[(q4 + i) * HP + d0 + m];
        }
        dW2[kt] = mfma16x4(x, hh, dW2[kt]);
      }
    }
    if (tid >= 64 && tid < 64 + K)
      SCALAR_LOOP
      for (int r = 0; r < 16; ++r) dbv += LG[r * GP + tid - 64];
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      SCALAR_LOOP
      for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(LG + m * GP + k0 + q4);
        f32x4 ww;
#pragma unroll
        for (int i = 0; i < 4; ++i) ww[i] = k0 + q4 + i < K ? a.w2[(k0 + q4 + i) * HD + d0 + m] : 0.f;
        acc = mfma16x4(x, ww, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) DH[(q4 + r) * HP + d0 + m] = H1[(q4 + r) * HP + d0 + m] > 0.f ? acc[r] : 0.f;
    }
    __syncthreads();
    // ---- db1, dW1 into the slab, dx over the probability columns
    if (tid < 64)
      SCALAR_LOOP
      for (int r = 0; r < 16; ++r) dbv += DH[r * HP + tid];
    {
      f32x4 dh;
#pragma unroll
      for (int i = 0; i < 4; ++i) dh[i] = DH[(q4 + i) * HP + d0 + m];
      SCALAR_LOOP
      for (int j0 = 0; j0 < XW; j0 += 16) {
        const bool jok = j0 + m < XW;
        f32x4 xx, acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) xx[i] = X[(q4 + i) * XP + j0 + m];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = jok ? sl[(d0 + q4 + r) * XW + j0 + m] : 0.f;
        acc = mfma16x4(dh, xx, acc);
        if (jok) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sl[(d0 + q4 + r) * XW + j0 + m] = acc[r];
        }
      }
    }
    SCALAR_LOOP
    for (int j0 = 16 * w; j0 < NA; j0 += 64) {
      const bool jok = j0 + m < NA;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < HD; k0 += 16) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(DH + m * HP + k0 + q4);
        f32x4 ww;
#pragma unroll
        for (int i = 0; i < 4; ++i) ww[i] = jok ? __ldg(a.w1 + (k0 + q4 + i) * XW + j0 + m) : 0.f;
        acc = mfma16x4(x, ww, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) DX[(q4 + r) * QP + j0 + m] = acc[r];
    }
    __syncthreads();
    // ---- softmax backward into dq_dense: exact zeros at padded steps and unavailable actions
    SCALAR_LOOP
    for (int pr = tid; pr < nr * N; pr += MI_TPB) {
      const int r = pr / N, n = pr - r * N;
      float* out = a.dq_dense + ((long)(r0 + r) * N + n) * A;
      if (RM[r] == 0.f) {
        SCALAR_LOOP
        for (int c = 0; c < A; ++c) out[c] = 0.f;
        continue;
      }
      const float* p = X + r * XP + n * A;
      const float* d = DX + r * QP + n * A;
      float dot = 0.f;
      SCALAR_LOOP
      for (int c = 0; c < A; ++c) dot += p[c] * d[c];
      SCALAR_LOOP
      for (int c = 0; c < A; ++c) out[c] = p[c] != 0.f ? p[c] * (d[c] - dot) : 0.f;
    }
    __syncthreads();
  }
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kt * 16 + q4 + r;
      if (k < K) sl[(long)HD * XW + HD + (long)k * HD + d0 + m] = dW2[kt][r];
    }
  if (tid < 64) sl[(long)HD * XW + tid] = dbv;
  else if (tid < 64 + K) sl[(long)HD * XW + HD + (long)K * HD + tid - 64] = dbv;
  block_partials<2>(acc2, a.ws);
}

__global__ __launch_bounds__(SUMS_TPB) void maven_stats_kernel(const float* ws, int nblocks, float* out2) {
  SCALAR_LOOP
  for (int i = 0; i < 2; ++i) {
    const float tot = block_tree_sum(ws, nblocks, 2, i);
    if (threadIdx.x == 0) out2[i] += tot;
  }
}

inline bool float_base(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int marl_maven_supported(int N, int A, int K, int S, int D) { return mi_shape_ok(N, A, K, S, D) ? 1 : 0; }

extern "C" size_t marl_maven_bwd_workspace(int B, int N, int A, int K) {
  if (!head_shape_ok(N, A, K) || B <= 0) return 0;
  return (size_t)head_slabs(B, N, A, K) * head_slab_len(N, A, K) * sizeof(float);
}

extern "C" size_t marl_maven_mi_workspace(long rows, int N, int A, int K, int S) {
  if (!mi_shape_ok(N, A, K, S, HD) || rows <= 0) return 0;
  return ((size_t)2 * MAX_SLABS + (size_t)mi_grid(rows) * mi_slab_len(N, A, K, S)) * sizeof(float);
}

extern "C" int marl_maven_plan(int B, int T, int N, int A, int K, int S, int* plan) {
  if (!plan || !mi_shape_ok(N, A, K, S, HD) || B < 0 || T < 0 || (long)B * T * N >= (1L << 31)) return (int)hipErrorInvalidValue;
  SCALAR_LOOP
  for (int i = 0; i < 8; ++i) plan[i] = 0;
  if (B == 0 || T == 0) return 0;
  const long rows = (long)B * T;
  const MiTile t = mi_tile(N, A, S);
  plan[0] = (T + 15) / 16;
  const long items = (long)B * N * plan[0];
  plan[1] = (int)(items > 65535 ? 65535 : items);
  plan[2] = head_slabs(B, N, A, K);
  plan[3] = (int)((rows + 15) / 16);
  plan[4] = mi_grid(rows);
  plan[5] = (int)t.lds;
  plan[6] = (int)((plan[3] + plan[4] - 1) / plan[4]);
  plan[7] = t.XP;
  return 0;
}

extern "C" int marl_maven_noise(unsigned rseed, int env0, unsigned tg0, int K, int* noise, int E, void* stream) {
  if (K < 1 || K > MAXK || (E > 0 && !noise)) return (int)hipErrorInvalidValue;
  if (E <= 0) return 0;
  hipLaunchKernelGGL(maven_noise_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rseed, env0, tg0, K, noise, E);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_maven_head_fwd(const marl_maven_weights_t* w, const float* hs, const int* noise, float* q, int B, int T, int N, int A,
                                   int K, void* stream) {
  if (!head_shape_ok(N, A, K) || B < 0 || T < 0 || (long)B * T * N >= (1L << 31)) return (int)hipErrorInvalidValue;
  if (B == 0 || T == 0) return 0;
  if (!w || !w->noise_w || !w->id_w || !w->noise_b || !w->id_b || !hs || !noise || !q || !aligned16(w->noise_w) || !aligned16(w->id_w) ||
      !aligned16(hs) || !float_base(w->noise_b) || !float_base(w->id_b) || !float_base(q) || !float_base(noise))
    return (int)hipErrorInvalidValue;
  HeadArgs a = {};
  a.noise_w = w->noise_w; a.id_w = w->id_w; a.noise_b = w->noise_b; a.id_b = w->id_b;
  a.hs = hs; a.noise = noise; a.q = q; a.B = B; a.T = T; a.N = N; a.A = A; a.K = K;
  a.tt = (T + 15) / 16;
  a.items = (long)B * N * a.tt;
  const unsigned grid = (unsigned)(a.items > 65535 ? 65535 : a.items);
  hipLaunchKernelGGL(maven_head_fwd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_maven_head_bwd(const marl_maven_weights_t* w, const marl_maven_grads_t* g, const float* hs, const int* noise,
                                   const int* dq_idx, const float* dq_val, const float* dq_dense, float* dq_out, float* dhs, float* ws,
                                   size_t ws_bytes, int B, int T, int N, int A, int K, void* stream) {
  if (!head_shape_ok(N, A, K) || B < 0 || T < 0 || (long)B * T * N >= (1L << 31)) return (int)hipErrorInvalidValue;
  if (B == 0 || T == 0) return 0;
  if (!w || !w->noise_w || !w->id_w || !g || !g->noise_w || !g->id_w || !g->noise_b || !g->id_b || !hs || !noise || !dq_out || !dhs ||
      !ws || (dq_idx != nullptr) != (dq_val != nullptr) || !aligned16(hs) || !aligned16(w->noise_w) || !aligned16(w->id_w) ||
      !float_base(noise) || !float_base(dq_idx) || !float_base(dq_val) || !float_base(dq_dense) || !float_base(dq_out) ||
      !float_base(dhs) || !float_base(g->noise_w) || !float_base(g->id_w) || !float_base(g->noise_b) || !float_base(g->id_b) ||
      !float_base(ws) || ws_bytes < marl_maven_bwd_workspace(B, N, A, K))
    return (int)hipErrorInvalidValue;
  HeadArgs a = {};
  a.noise_w = w->noise_w; a.id_w = w->id_w;
  a.hs = hs; a.noise = noise; a.dq_idx = dq_idx; a.dq_val = dq_val; a.dq_dense = dq_dense; a.dq_out = dq_out; a.dhs = dhs; a.ws = ws;
  a.B = B; a.T = T; a.N = N; a.A = A; a.K = K;
  a.slab_len = head_slab_len(N, A, K);
  const int slabs = head_slabs(B, N, A, K);
  hipLaunchKernelGGL(maven_head_bwd_kernel, dim3((unsigned)slabs), dim3(64), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maven_reduce_kernel, dim3((unsigned)reduce_blocks(a.slab_len)), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                     a.slab_len, slabs, g->noise_w, (long)K * A * HD, g->id_w, (long)N * A * HD, g->noise_b, (long)K * A, g->id_b,
                     (long)N * A);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_maven_mi(const marl_maven_disc_t* d, const marl_maven_disc_grads_t* g, const float* q, const float* avail,
                             long avail_bs, const float* state, long state_ld, long state_bs, const int* ep_map, const int* noise,
                             const float* padded, float lambda_mi, float* dq_dense, float* ce, float* stats2, float* ws, size_t ws_bytes,
                             int B, int T, int N, int A, int S, int K, void* stream) {
  if (!mi_shape_ok(N, A, K, S, HD) || B < 0 || T < 0 || (long)B * T * N >= (1L << 31)) return (int)hipErrorInvalidValue;
  if (B == 0 || T == 0) return 0;
  const long rows = (long)B * T;
  if (!d || !d->w1 || !d->b1 || !d->w2 || !d->b2 || !g || !g->w1 || !g->b1 || !g->w2 || !g->b2 || !q || !avail || !state || !noise ||
      !padded || !dq_dense || !ce || !stats2 || !ws || !aligned16(d->w2) || !float_base(d->w1) || !float_base(state) || !float_base(avail) ||
      !float_base(ws) || state_ld < S || avail_bs < 0 || state_bs < 0 || !(lambda_mi >= 0.f) || avail_bs >= (1L << 31) || state_bs >= (1L << 31) || state_ld >= (1L << 31) ||
      rows > (1L << 31) - (16L << 16) || ws_bytes < marl_maven_mi_workspace(rows, N, A, K, S))
    return (int)hipErrorInvalidValue;
  const MiTile t = mi_tile(N, A, S);
  MiArgs a = {};
  a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2;
  a.q = q; a.avail = avail; a.avail_bs = (int)avail_bs; a.state = state; a.state_ld = (int)state_ld; a.state_bs = (int)state_bs;
  a.ep_map = ep_map; a.noise = noise; a.padded = padded; a.lambda = lambda_mi; a.dq_dense = dq_dense; a.ce = ce;
  a.ws = ws;
  a.slab_len = (int)mi_slab_len(N, A, K, S); a.rows = (int)rows;
  a.T = T; a.N = N; a.A = A; a.S = S; a.K = K; a.XW = t.XW; a.XK = t.XK; a.XP = t.XP; a.QP = t.QP;
  const int grid = mi_grid(rows);
  const void* fn = (const void*)maven_mi_kernel;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {(void*)&a};
  e = hipLaunchKernel(fn, dim3((unsigned)grid), dim3(MI_TPB), kargs, t.lds, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maven_stats_kernel, dim3(1), dim3(SUMS_TPB), 0, (hipStream_t)stream, (const float*)ws, grid, stats2);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maven_reduce_kernel, dim3((unsigned)reduce_blocks(a.slab_len)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)(ws + 2 * MAX_SLABS), a.slab_len, grid, g->w1, (long)HD * t.XW, g->b1, (long)HD, g->w2, (long)K * HD, g->b2,
                     (long)K);
  MARL_CHECK_LAUNCH();
  return 0;
}
