// COMA's counterfactual critic (include/marl_hip.h has the definitions).  A row r = (b T + t) N + i is agent i at step t of episode b.
// The critic's first layer over the virtual input [s | o_i | one-hot(u_j), own block zeroed | one-hot(u_j at t-1) | one-hot(i)] is
// never materialised: the state and observation blocks are two marl_linear calls on column blocks of fc1.weight, the 2 N A + N
// one-hot columns are gathered here from a K-major copy Wt (C = 2 N A + N rows of D floats: actions j-major, last actions, ids), so
// that every gather is one contiguous run of D floats.
//
// Lane mappings (D4 = D / 4 float4 columns, 32 at D = 128):
//   fc1_fwd / the gate pass of fc1_bwd: a lane is (step g of the 256 / D4 steps of its workgroup, float4 column c).  It forms the
//     step's shared sum pre_s + sum_j Wu[j, u_j] + [t > 0] sum_j Wl[j, u_j(t-1)] once, in registers, then walks the step's N agent
//     rows: agent i takes the sum minus its own column Wu[i, u_i] plus Wid[i].  2 N gathers per step instead of 2 N per row; a
//     half-wave reads / writes one whole row (512 bytes) per access.  No LDS, no barrier.
//   the scatter of fc1_bwd: a workgroup per (agent j, slab of steps); lane d owns column d of D.  It walks the slab's steps in
//     order and adds (dsum - dpre_j) into row u_j of an A x D table in LDS, dsum into row u_j(t-1) of a second one and dpre_j into
//     a register (the id column): no two lanes ever touch the same word, so there is no barrier and no atomic.  The tables go to a
//     workspace; one more launch adds the slabs in order into fc1.weight.grad's columns (lane = (column, d), d fastest).
//   q_taken: one lane per output element.
//   loss_bwd: row_tile.h's staging with three tiles (logits, availability, Q); dlogits and dQ are written over the logits and Q
//     tiles and stored back.  From A = 19 the twelve tiles of a workgroup pass 56 KiB and the row-per-lane form runs.
// fp32, fixed-order sums, no float atomics: two calls give the same bits.  An action index outside [0, A) is an all-zero one-hot.
#include "sums.h"
#include "policy_rows.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;
constexpr int SLAB_STEPS_MIN = 8;     // steps per slab of the scatter at least; 256 slabs at most
constexpr int SLABS_MAX = 256;

__device__ __forceinline__ bool in_range(int k, int A) { return (unsigned)k < (unsigned)A; }

__global__ void coma_onehot_cols_kernel(const float* W, long ldw, int col0, float* Wt, int C, int D) {
  const long total = (long)C * D;
  for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long)gridDim.x * TPB) {
    const int c = (int)(e / D), d = (int)(e - (long)c * D);
    Wt[e] = W[(long)d * ldw + col0 + c];
  }
}

__global__ __launch_bounds__(TPB) void coma_fc1_fwd_kernel(const f32x4* pre_s, const f32x4* Wt, const int* u, f32x4* h1, long BT,
                                                           int T, int N, int A, int D4, int SPB) {
  const int g = threadIdx.x / D4, c = threadIdx.x - g * D4;
  const long bt = (long)blockIdx.x * SPB + g;
  if (g >= SPB || bt >= BT) return;
  const int t = (int)(bt % T);
  const int* uc = u + bt * N;
  f32x4 acc = pre_s[bt * D4 + c];
  for (int j = 0; j < N; ++j) {
    const int k = uc[j];
    if (in_range(k, A)) acc += Wt[((long)j * A + k) * D4 + c];
  }
  if (t > 0) {
    const int* ul = uc - N;
    for (int j = 0; j < N; ++j) {
      const int k = ul[j];
      if (in_range(k, A)) acc += Wt[((long)(N + j) * A + k) * D4 + c];
    }
  }
  const f32x4* Wid = Wt + (long)2 * N * A * D4;
  for (int i = 0; i < N; ++i) {
    const long r = bt * N + i;
    const int k = uc[i];
    f32x4 rest = acc;
    if (in_range(k, A)) rest -= Wt[((long)i * A + k) * D4 + c];
    f32x4 v = h1[r * D4 + c] + rest + Wid[(long)i * D4 + c];
#pragma unroll
    for (int x = 0; x < 4; ++x) v[x] = fmaxf(v[x], 0.f);
    h1[r * D4 + c] = v;
  }
}

// dpre = dh1 (h1 > 0), dsum = its sum over a step's agents in agent order
__global__ __launch_bounds__(TPB) void coma_fc1_gate_kernel(const f32x4* dh1, const f32x4* h1, f32x4* dpre, f32x4* dsum, long BT,
                                                            int N, int D4, int SPB) {
  const int g = threadIdx.x / D4, c = threadIdx.x - g * D4;
  const long bt = (long)blockIdx.x * SPB + g;
  if (g >= SPB || bt >= BT) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < N; ++i) {
    const long e = (bt * N + i) * D4 + c;
    const f32x4 h = h1[e];
    f32x4 d = dh1[e];
#pragma unroll
    for (int x = 0; x < 4; ++x) d[x] = h[x] > 0.f ? d[x] : 0.f;
    dpre[e] = d;
    acc += d;
  }
  dsum[bt * D4 + c] = acc;
}

// ws[slab][j][row][d]: rows 0 .. A-1 the action columns of agent j, A .. 2A-1 its last-action columns, 2A its id column
__global__ void coma_fc1_scatter_kernel(const float* dpre, const float* dsum, const int* u, float* ws, long BT, int T, int N, int A,
                                        int D, long slab_steps) {
  extern __shared__ float tab[];                       // (2 A, D)
  const int j = blockIdx.x, d = threadIdx.x;
  if (d >= D) return;
  for (int k = 0; k < 2 * A; ++k) tab[k * D + d] = 0.f;
  float idacc = 0.f;
  const long b0 = (long)blockIdx.y * slab_steps;
  const long b1 = b0 + slab_steps < BT ? b0 + slab_steps : BT;
  for (long bt = b0; bt < b1; ++bt) {
    const float ds = dsum[bt * D + d];
    const float dp = dpre[(bt * N + j) * D + d];
    const int k = u[bt * N + j];
    if (in_range(k, A)) tab[k * D + d] += ds - dp;
    if (bt % T != 0) {
      const int kl = u[(bt - 1) * N + j];
      if (in_range(kl, A)) tab[(A + kl) * D + d] += ds;
    }
    idacc += dp;
  }
  float* o = ws + ((long)blockIdx.y * N + j) * (2 * A + 1) * D;
  for (int k = 0; k < 2 * A; ++k) o[(long)k * D + d] = tab[k * D + d];
  o[(long)2 * A * D + d] = idacc;
}

// dW[d][col0 + c] += sum over the slabs, in slab order
__global__ void coma_fc1_slabs_kernel(const float* ws, float* dW, long lddw, int col0, int slabs, int N, int A, int D) {
  const int C = 2 * N * A + N;
  const long total = (long)C * D;
  for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long)gridDim.x * TPB) {
    const int c = (int)(e / D), d = (int)(e - (long)c * D);
    int j, row;
    if (c < N * A) { j = c / A; row = c - j * A; }
    else if (c < 2 * N * A) { const int cc = c - N * A; j = cc / A; row = A + cc - j * A; }
    else { j = c - 2 * N * A; row = 2 * A; }
    float s = 0.f;
    for (int sl = 0; sl < slabs; ++sl) s += ws[(((long)sl * N + j) * (2 * A + 1) + row) * D + d];
    dW[(long)d * lddw + col0 + c] += s;
  }
}

__global__ void coma_q_taken_kernel(const float* q, const int* u, float* out, int shift, int B, int T, int N, int A) {
  const long total = (long)B * N * T;
  for (long e = (long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long)gridDim.x * TPB) {
    const int t = (int)(e % T);
    const long bn = e / T;
    const int i = (int)(bn % N);
    const long b = bn / N;
    const int ts = t + shift;
    float v = 0.f;
    if (ts >= 0 && ts < T) {
      const long r = (b * T + ts) * N + i;
      const int k = u[r];
      if (in_range(k, A)) v = q[r * A + k];
    }
    out[e] = v;
  }
}

struct ComaArgs {
  const float *logits, *avail, *q;   // (rows, A)
  const int* u;                      // (rows)
  const float *G, *padded;           // (B, N, T); (B T)
  float eps, beta;
  float *dlogits, *dq;               // (rows, A)
  float *logp, *ent, *adv, *qt;      // (rows)
  float* ws;
  long rows;
  int T, N, A, vec;
};

// one row of both losses: acc = { m (G - Q_u)^2, m, - m Adv log pi_u - beta m H, m H }
__device__ __forceinline__ void coma_row(const ComaArgs& p, long r, const float* z, const float* a, const float* q, float* outz,
                                         float* outq, float (&acc)[4]) {
  const int A = p.A;
  const long bt = r / p.N;
  const float m = 1.f - p.padded[bt];
  float lp = 0.f, H = 0.f, adv = 0.f, qu = 0.f;
  bool live = false;
  if (m != 0.f) {                                        // a padded step's logits and Q are never looked at
    const int u = p.u[r];
    const RowPolicy pol = row_policy(z, a, A, p.eps);
    if (pol.n > 0 && u >= 0 && u < A && a[u] != 0.f) {
      live = true;
      qu = q[u];
      float base = qu;                                   // one available action: pi = 1 there, Adv = 0
      if (pol.n > 1) {
        const float inv = 1.f / pol.D;
        base = 0.f;
        for (int k = 0; k < A; ++k)
          if (a[k] != 0.f) base += (pol.cw * row_e(pol, z[k]) + pol.ew) * inv * q[k];
      }
      adv = qu - base;
      const int i = (int)(r - bt * p.N);
      const long b = bt / p.T;
      const int t = (int)(bt - b * p.T);
      const float td = p.G[(b * p.N + i) * p.T + t] - qu;
      row_logp_ent_grad_of(pol, z, a, outz, A, u, -m * adv, p.beta * m, lp, H);
      for (int k = 0; k < A; ++k) outq[k] = 0.f;
      outq[u] = -2.f * m * td;
      acc[0] += m * td * td;
      acc[2] += -m * adv * lp;
      if (p.beta != 0.f) acc[2] -= p.beta * m * H;
      acc[3] += m * H;
    }
  }
  if (!live)
    for (int k = 0; k < A; ++k) { outz[k] = 0.f; outq[k] = 0.f; }
  p.logp[r] = lp; p.ent[r] = H; p.adv[r] = adv; p.qt[r] = qu;
  acc[1] += m;
}

__global__ __launch_bounds__(TPB) void coma_loss_tiled_kernel(ComaArgs p) {
  extern __shared__ __attribute__((aligned(16))) float ct_smem[];
  const int lane = threadIdx.x & 63;
  const int A = p.A;
  const int TS = rt::tile_floats(A);
  float* Sz = rt::wave_tiles(ct_smem, 3, A);
  float* Sa = Sz + TS;
  float* Sq = Sa + TS;
  float acc[4] = {};
  const long tiles = rt::tiles(p.rows);
  for (long tile = rt::first_tile(); tile < tiles; tile += rt::tile_step()) {
    const long r0 = tile * rt::ROWS;
    const int n = rt::tile_len(p.rows, r0, A);
    rt::copy<3>({Sz, Sa, Sq}, {p.logits + r0 * A, p.avail + r0 * A, p.q + r0 * A}, n, p.vec);
    rt::lds_done_fenced();
    const long r = r0 + lane;
    if (r < p.rows) coma_row(p, r, Sz + lane * A, Sa + lane * A, Sq + lane * A, Sz + lane * A, Sq + lane * A, acc);
    rt::lds_done_fenced();
    rt::copy<2>({p.dlogits + r0 * A, p.dq + r0 * A}, {Sz, Sq}, n, p.vec);
    rt::lds_done_fenced();                                // the tiles are read out before the next trip overwrites them
  }
  block_partials<4>(acc, p.ws);
}

__global__ __launch_bounds__(TPB) void coma_loss_rows_kernel(ComaArgs p) {
  float acc[4] = {};
  for (long r = (long)blockIdx.x * TPB + threadIdx.x; r < p.rows; r += (long)gridDim.x * TPB)
    coma_row(p, r, p.logits + r * p.A, p.avail + r * p.A, p.q + r * p.A, p.dlogits + r * p.A, p.dq + r * p.A, acc);
  block_partials<4>(acc, p.ws);
}

// the four sums in block order, then critic = { s0, s1 }, actor = { s2, s1, s3 }
__global__ void coma_finish_kernel(const float* ws, int nblocks, float* out_c2, float* out_a3) {
  float tot[4];
  for (int i = 0; i < 4; ++i) tot[i] = block_tree_sum(ws, nblocks, 4, i);
  if (threadIdx.x == 0) {
    out_c2[0] = tot[0]; out_c2[1] = tot[1];
    out_a3[0] = tot[2]; out_a3[1] = tot[1]; out_a3[2] = tot[3];
  }
}

inline unsigned blocks_for(long total) {
  long b = (total + TPB - 1) / TPB;
  return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
inline int fc1_slabs(long BT) {
  long s = (BT + SLAB_STEPS_MIN - 1) / SLAB_STEPS_MIN;
  return (int)(s > SLABS_MAX ? SLABS_MAX : (s < 1 ? 1 : s));
}
// D: whole float4 columns, at most one workgroup wide
inline bool dim_ok(int D) { return D > 0 && D % 4 == 0 && D <= 1024; }

}  // namespace

extern "C" int marl_coma_onehot_cols(const float* W, long ldw, int col0, float* Wt, int C, int D, void* stream) {
  if (C <= 0 || D <= 0) return 0;
  if (!W || !Wt || col0 < 0 || ldw < (long)col0 + C) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(coma_onehot_cols_kernel, dim3(blocks_for((long)C * D)), dim3(TPB), 0, (hipStream_t)stream, W, ldw, col0, Wt, C,
                     D);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_coma_fc1_fwd(const float* pre_s, const float* Wt, const int* u, float* h1, int B, int T, int N, int A, int D,
                                 void* stream) {
  if (B <= 0 || T <= 0 || N <= 0 || A <= 0 || D <= 0) return 0;
  if (!pre_s || !Wt || !u || !h1 || !dim_ok(D) || !aligned16(pre_s) || !aligned16(Wt) || !aligned16(h1)) return (int)hipErrorInvalidValue;
  const long BT = (long)B * T;
  const int D4 = D / 4, SPB = TPB / D4;
  hipLaunchKernelGGL(coma_fc1_fwd_kernel, dim3((unsigned)((BT + SPB - 1) / SPB)), dim3(TPB), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(pre_s), reinterpret_cast<const f32x4*>(Wt), u, reinterpret_cast<f32x4*>(h1), BT,
                     T, N, A, D4, SPB);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t marl_coma_fc1_bwd_workspace(int B, int T, int N, int A, int D) {
  if (B <= 0 || T <= 0 || N <= 0 || A <= 0 || D <= 0) return 0;
  return (size_t)fc1_slabs((long)B * T) * N * (2 * A + 1) * D * sizeof(float);
}

extern "C" int marl_coma_fc1_bwd(const float* dh1, const float* h1, const int* u, float* dpre, float* dsum, float* dW, long lddw,
                                 int col0, float* ws, size_t ws_bytes, int B, int T, int N, int A, int D, void* stream) {
  if (B <= 0 || T <= 0 || N <= 0 || A <= 0 || D <= 0) return 0;
  const int C = 2 * N * A + N;
  const size_t lds = (size_t)2 * A * D * sizeof(float);
  if (!dh1 || !h1 || !u || !dpre || !dsum || !dW || !ws || !dim_ok(D) || !aligned16(dh1) || !aligned16(h1) || !aligned16(dpre) || !aligned16(dsum) ||
      col0 < 0 || lddw < (long)col0 + C || lds > 64 * 1024 || ws_bytes < marl_coma_fc1_bwd_workspace(B, T, N, A, D))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const long BT = (long)B * T;
  const int D4 = D / 4, SPB = TPB / D4;
  hipLaunchKernelGGL(coma_fc1_gate_kernel, dim3((unsigned)((BT + SPB - 1) / SPB)), dim3(TPB), 0, s,
                     reinterpret_cast<const f32x4*>(dh1), reinterpret_cast<const f32x4*>(h1), reinterpret_cast<f32x4*>(dpre),
                     reinterpret_cast<f32x4*>(dsum), BT, N, D4, SPB);
  MARL_CHECK_LAUNCH();
  const int slabs = fc1_slabs(BT);
  const long slab_steps = (BT + slabs - 1) / slabs;
  hipLaunchKernelGGL(coma_fc1_scatter_kernel, dim3((unsigned)N, (unsigned)slabs), dim3((unsigned)((D + 63) / 64 * 64)), lds, s,
                     (const float*)dpre, (const float*)dsum, u, ws, BT, T, N, A, D, slab_steps);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(coma_fc1_slabs_kernel, dim3(blocks_for((long)C * D)), dim3(TPB), 0, s, (const float*)ws, dW, lddw, col0, slabs,
                     N, A, D);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_coma_q_taken(const float* q, const int* u, float* out, int shift, int B, int T, int N, int A, void* stream) {
  if (B <= 0 || T <= 0 || N <= 0 || A <= 0) return 0;
  if (!q || !u || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(coma_q_taken_kernel, dim3(blocks_for((long)B * N * T)), dim3(TPB), 0, (hipStream_t)stream, q, u, out, shift, B,
                     T, N, A);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_coma_loss_bwd(const float* logits, const float* avail, const float* q, const int* u, const float* G,
                                  const float* padded, float eps, float beta, float* dlogits, float* dq, float* logp, float* ent,
                                  float* adv, float* q_taken, float* out_c2, float* out_a3, float* ws, int B, int T, int N, int A,
                                  void* stream) {
  if (B <= 0 || T <= 0 || N <= 0 || A <= 0) return 0;
  if (!logits || !avail || !q || !u || !G || !padded || !dlogits || !dq || !logp || !ent || !adv || !q_taken || !out_c2 || !out_a3 ||
      !ws || dlogits == avail || dq == avail || dq == logits || dlogits == q || dlogits == dq || !(beta >= 0.f))
    return (int)hipErrorInvalidValue;
  ComaArgs p = {};
  p.logits = logits; p.avail = avail; p.q = q; p.u = u; p.G = G; p.padded = padded; p.eps = eps; p.beta = beta;
  p.dlogits = dlogits; p.dq = dq; p.logp = logp; p.ent = ent; p.adv = adv; p.qt = q_taken; p.ws = ws;
  p.rows = (long)B * T * N; p.T = T; p.N = N; p.A = A;
  hipStream_t s = (hipStream_t)stream;
  int nb;
  const rt::Plan pl = rt::plan(p.rows, A, 3, 56 * 1024, rt::PARTIAL_ROWS, {logits, avail, q, dlogits, dq});   // (block_partials keeps a few floats of its own)
  if (pl.tiled) {
    nb = pl.blocks;
    p.vec = pl.vec;
    hipLaunchKernelGGL(coma_loss_tiled_kernel, dim3((unsigned)nb), dim3(TPB), pl.lds_bytes, s, p);
  } else {
    nb = rt::partial_blocks(p.rows);
    hipLaunchKernelGGL(coma_loss_rows_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, p);
  }
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(coma_finish_kernel, dim3(1), dim3(TPB), 0, s, (const float*)ws, nb, out_c2, out_a3);
  MARL_CHECK_LAUNCH();
  return 0;
}
