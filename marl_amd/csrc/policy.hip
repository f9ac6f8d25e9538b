// Stochastic policy head of the policy-gradient learners (central-V, REINFORCE, MAPPO; include/marl_hip.h has the definition).
// A row is one agent at one step: logits z (A, the agent's fc2 output), availability a in {0,1}^A, exploration rate eps:
//   p = softmax(z),  n = sum a,  pt_k = a_k ((1 - eps) p_k + eps / n),  pi_k = pt_k / sum_j pt_j.
// The kernels shift by mx = the largest AVAILABLE logit (any shift gives the same p): with e_k = exp(min(z_k - mx, 80)),
// S = sum e, Sa = sum a e, w_k = (1 - eps) e_k + eps S / n and D = (1 - eps) Sa + eps S the policy is pi_k = a_k w_k / D, where
// Sa >= 1 keeps D away from 0 and the clamp keeps S finite when an unavailable logit towers over the available ones.
// Gradient of log pi_u by z_i (through pt and the renormalisation; delta_ui - pi_i at eps = 0):
//   g_i = (1 - eps) [ e_u (delta_ui - e_i / S) / w_u  -  e_i (a_i - Sa / S) / D ].
//
// Lane mapping of the two batch kernels (probs, loss_bwd): row_tile.h's staging with two tiles, logits and availability; every lane
// writes its result over its row of the logits tile, and the wave stores that tile back.  From A = 29 the tiles of four waves pass
// 56 KiB and the row-per-lane kernel runs instead.
// marl_policy_probs_bwd (LICA: the transpose-Jacobian of pi applied to dL/dpi, policy_rows.h: row_probs_bwd) stages a third tile,
// the gradient, and takes the row-per-lane form from A = 19.
// The sampler runs once per lock-step over E N rows (25 600 at most in the measured set-ups): one lane per row, like select_kernel.
#include <type_traits>
#include "synth_env.h"
#include "sums.h"
#include "policy_rows.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;

struct PolicyArgs {
  const float *logits, *avail;       // (rows, A)
  const int* u;                      // (rows)            loss only
  const float *G, *v, *padded;       // (rows / N)        loss only
  float eps, beta;                   // beta: weight of the entropy bonus (loss_bwd_ex)
  float *out, *logp, *ent, *ws;      // (rows, A): pi or dlogits; (rows); (rows) or NULL (loss_bwd_ex); partial sums
  long rows;
  int N, A, vec;
};
// ppo_loss_bwd: G holds adv and v is unused.  Its two scalars ride behind PolicyArgs in a type of their own, so that the kernel
// argument of the other instantiations is the struct it was (and their code with it)
struct PpoArgs : PolicyArgs {
  const float* logp_old;             // (rows) or NULL
  float clip;                        // c in (0, 1)
};
template <bool PPO> using ArgsOf = std::conditional_t<PPO, PpoArgs, PolicyArgs>;

// one row of the loss: m = 1 - padded, Adv = G - v of the row's (episode, step); out = -m Adv d log pi_u / dz
__device__ __forceinline__ void loss_row(const PolicyArgs& p, long r, const float* z, const float* a, float* out, float (&acc)[2]) {
  const long bt = r / p.N;
  const float m = 1.f - p.padded[bt];
  float adv = 0.f;
  if (m != 0.f) adv = p.G[bt] - p.v[bt];                 // a padded step's G and v are never looked at
  float lp = 0.f;
  if (m == 0.f) {
    for (int k = 0; k < p.A; ++k) out[k] = 0.f;          // a padded step: exact zeros, its logits are never looked at
  } else if (row_logp_grad(z, a, out, p.A, p.eps, p.u[r], -m * adv, lp)) {
    acc[0] += -m * adv * lp;
  }
  p.logp[r] = lp;
  acc[1] += m;
}

// loss_row without a baseline (v NULL: Adv = G) and with the entropy bonus: out = -m Adv d log pi_u / dz - beta m dH / dz,
// acc = { -m Adv log pi_u - beta m H, m, m H }
__device__ __forceinline__ void loss_row_ex(const PolicyArgs& p, long r, const float* z, const float* a, float* out, float (&acc)[3]) {
  const long bt = r / p.N;
  const float m = 1.f - p.padded[bt];
  float adv = 0.f;
  if (m != 0.f) adv = p.v ? p.G[bt] - p.v[bt] : p.G[bt];
  float lp = 0.f, H = 0.f;
  if (m == 0.f) {
    for (int k = 0; k < p.A; ++k) out[k] = 0.f;
  } else if (row_logp_ent_grad(z, a, out, p.A, p.eps, p.u[r], -m * adv, p.beta * m, lp, H)) {
    acc[0] += -m * adv * lp;
    if (p.beta != 0.f) acc[0] -= p.beta * m * H;
    acc[2] += m * H;
  }
  p.logp[r] = lp;
  if (p.ent) p.ent[r] = H;
  acc[1] += m;
}

// loss_row_ex's row under the clipped surrogate: Adv = adv[bt], rho = exp(log pi_u - logp_old) (1 exactly without logp_old, and on a
// row with one available action), s = rho Adv, k = clamp(rho, 1 - c, 1 + c) Adv, clipped = k < s.  log pi_u comes from the row
// scalars (one exp and two logs beside row_policy's walk), so that the gradient walk already knows its scale:
// out = -(clipped ? 0 : m Adv rho) d log pi_u / dz - beta m dH / dz,  acc = { -m min(s, k) - beta m H, m, m H, m [clipped] }
__device__ __forceinline__ void loss_row_ppo(const PpoArgs& p, long r, const float* z, const float* a, float* out, float (&acc)[4]) {
  const long bt = r / p.N;
  const float m = 1.f - p.padded[bt];
  float lp = 0.f, H = 0.f;
  if (m == 0.f) {
    for (int k = 0; k < p.A; ++k) out[k] = 0.f;          // a padded step: its logits, adv and logp_old are never looked at
  } else {
    const float adv = p.G[bt];
    const int u = p.u[r];
    const RowPolicy rp = row_policy(z, a, p.A, p.eps);
    float rho = 1.f;
    if (p.logp_old && rp.n > 1 && u >= 0 && u < p.A && a[u] != 0.f) {
      const float wu = rp.cw * row_e(rp, z[u]) + rp.ew;
      rho = expf(fminf(logf(wu) - logf(rp.D) - p.logp_old[r], EXP_CLAMP));
    }
    const float s = rho * adv, k = fminf(fmaxf(rho, 1.f - p.clip), 1.f + p.clip) * adv;
    const bool clipped = k < s;
    if (row_logp_ent_grad_of<true>(rp, z, a, out, p.A, u, clipped ? 0.f : -m * adv * rho, p.beta * m, lp, H)) {
      acc[0] += -m * fminf(s, k);
      if (p.beta != 0.f) acc[0] -= p.beta * m * H;
      acc[2] += m * H;
      if (clipped) acc[3] += m;
    }
  }
  p.logp[r] = lp;
  if (p.ent) p.ent[r] = H;
  acc[1] += m;
}

// EX (with LOSS): loss_row_ex and its three partial sums; PPO (with LOSS and EX): loss_row_ppo and its four
template <bool LOSS, bool EX = false, bool PPO = false>
__global__ __launch_bounds__(TPB) void policy_tiled_kernel(ArgsOf<PPO> p) {
  extern __shared__ __attribute__((aligned(16))) float pt_smem[];
  const int lane = threadIdx.x & 63;
  const int A = p.A;
  float* Sz = rt::wave_tiles(pt_smem, 2, A);
  float* Sa = Sz + rt::tile_floats(A);
  float acc[PPO ? 4 : EX ? 3 : 2] = {};
  const long tiles = rt::tiles(p.rows);
  for (long tile = rt::first_tile(); tile < tiles; tile += rt::tile_step()) {
    const long r0 = tile * rt::ROWS;
    const int n = rt::tile_len(p.rows, r0, A);
    rt::copy<2>({Sz, Sa}, {p.logits + r0 * A, p.avail + r0 * A}, n, p.vec);
    rt::lds_done_fenced();
    const long r = r0 + lane;
    if (r < p.rows) {
      if constexpr (PPO) loss_row_ppo(p, r, Sz + lane * A, Sa + lane * A, Sz + lane * A, acc);
      else if constexpr (EX) loss_row_ex(p, r, Sz + lane * A, Sa + lane * A, Sz + lane * A, acc);
      else if constexpr (LOSS) loss_row(p, r, Sz + lane * A, Sa + lane * A, Sz + lane * A, acc);
      else row_probs(Sz + lane * A, Sa + lane * A, Sz + lane * A, A, p.eps);
    }
    rt::lds_done_fenced();
    rt::copy(p.out + r0 * A, Sz, n, p.vec);
    rt::lds_done_fenced();                                // the tile is read out before the next trip overwrites it
  }
  if (LOSS) block_partials<PPO ? 4 : EX ? 3 : 2>(acc, p.ws);
}

// row-per-lane form for action counts whose tiles do not fit: same arithmetic in the same order
template <bool LOSS, bool EX = false, bool PPO = false>
__global__ __launch_bounds__(TPB) void policy_rows_kernel(ArgsOf<PPO> p) {
  float acc[PPO ? 4 : EX ? 3 : 2] = {};
  for (long r = (long)blockIdx.x * TPB + threadIdx.x; r < p.rows; r += (long)gridDim.x * TPB) {
    const float* z = p.logits + r * p.A;
    const float* a = p.avail + r * p.A;
    float* out = p.out + r * p.A;
    if constexpr (PPO) loss_row_ppo(p, r, z, a, out, acc);
    else if constexpr (EX) loss_row_ex(p, r, z, a, out, acc);
    else if constexpr (LOSS) loss_row(p, r, z, a, out, acc);
    else row_probs(z, a, out, p.A, p.eps);
  }
  if (LOSS) block_partials<PPO ? 4 : EX ? 3 : 2>(acc, p.ws);
}

template <bool LOSS, bool EX = false, bool PPO = false>
int launch_policy(ArgsOf<PPO> p, hipStream_t s, int& nb) {
  const rt::Plan pl = rt::plan(p.rows, p.A, 2, 56 * 1024, rt::PARTIAL_ROWS, {p.logits, p.avail, p.out});   // (block_partials keeps a few floats of its own)
  if (pl.tiled) {
    nb = pl.blocks;
    p.vec = pl.vec;
    hipLaunchKernelGGL((policy_tiled_kernel<LOSS, EX, PPO>), dim3((unsigned)nb), dim3(TPB), pl.lds_bytes, s, p);
  } else {
    nb = rt::partial_blocks(p.rows);
    hipLaunchKernelGGL((policy_rows_kernel<LOSS, EX, PPO>), dim3((unsigned)nb), dim3(TPB), 0, s, p);
  }
  MARL_CHECK_LAUNCH();
  return 0;
}

// marl_policy_probs_bwd (LICA's actor pass): gpi is a third row operand, so the tiled form stages three tiles (it fits up to A = 18)
struct ProbsBwdArgs {
  const float *logits, *avail, *gpi;     // (rows, A)
  const float *q_pi, *padded;            // (rows / N); q_pi may be NULL
  float eps, beta;
  float *out, *ent, *ws;                 // (rows, A); (rows) or NULL; partial sums
  long rows;
  int N, A, vec;
};

// one agent row: out = J^T gpi - beta m dH/dz, acc = { -m q_pi - beta m H, m, m H }; a padded step: exact zeros, nothing of it looked at
__device__ __forceinline__ void probs_bwd_row(const ProbsBwdArgs& p, long r, const float* z, const float* a, const float* g, float* out,
                                              float (&acc)[3]) {
  const long bt = r / p.N;
  const float m = 1.f - p.padded[bt];
  float H = 0.f;
  if (m == 0.f) {
    for (int k = 0; k < p.A; ++k) out[k] = 0.f;
  } else {
    if (p.q_pi) acc[0] -= m * p.q_pi[bt];
    if (row_probs_bwd(row_policy(z, a, p.A, p.eps), z, a, g, out, p.A, p.eps, p.beta * m, H)) {
      if (p.beta != 0.f) acc[0] -= p.beta * m * H;
      acc[2] += m * H;
    }
  }
  if (p.ent) p.ent[r] = H;
  acc[1] += m;
}

__global__ __launch_bounds__(TPB) void probs_bwd_tiled_kernel(ProbsBwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float pb_smem[];
  const int lane = threadIdx.x & 63;
  const int A = p.A;
  float* Sz = rt::wave_tiles(pb_smem, 3, A);
  float* Sa = Sz + rt::tile_floats(A);
  float* Sg = Sa + rt::tile_floats(A);
  float acc[3] = {};
  const long tiles = rt::tiles(p.rows);
  for (long tile = rt::first_tile(); tile < tiles; tile += rt::tile_step()) {
    const long r0 = tile * rt::ROWS;
    const int n = rt::tile_len(p.rows, r0, A);
    rt::copy<3>({Sz, Sa, Sg}, {p.logits + r0 * A, p.avail + r0 * A, p.gpi + r0 * A}, n, p.vec);
    rt::lds_done_fenced();
    const long r = r0 + lane;
    if (r < p.rows) probs_bwd_row(p, r, Sz + lane * A, Sa + lane * A, Sg + lane * A, Sz + lane * A, acc);
    rt::lds_done_fenced();
    rt::copy(p.out + r0 * A, Sz, n, p.vec);
    rt::lds_done_fenced();                                // the tile is read out before the next trip overwrites it
  }
  block_partials<3>(acc, p.ws);
}

// row-per-lane form for action counts whose tiles do not fit: same arithmetic in the same order
__global__ __launch_bounds__(TPB) void probs_bwd_rows_kernel(ProbsBwdArgs p) {
  float acc[3] = {};
  for (long r = (long)blockIdx.x * TPB + threadIdx.x; r < p.rows; r += (long)gridDim.x * TPB)
    probs_bwd_row(p, r, p.logits + r * p.A, p.avail + r * p.A, p.gpi + r * p.A, p.out + r * p.A, acc);
  block_partials<3>(acc, p.ws);
}

// marl_select_actions' argument shape; the draw is the ST_SAMPLE stream's
__global__ void policy_sample_kernel(const float* logits, const float* avail, long avail_es, const int* alive, float eps,
                                     unsigned rseed, int env0, const int* tg, int tg0, int* act_out, long act_es, int E,
                                     int N, int A) {
  const long total = (long)E * N;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
    const int e = (int)(i / N), n = (int)(i - (long)e * N);
    int* out = act_out + e * act_es + n;
    if (alive && !alive[e]) { *out = -1; continue; }
    const float* z = logits + i * A;
    const float* av = avail + e * avail_es + (long)n * A;
    const RowPolicy p = row_policy(z, av, A, eps);
    const unsigned tgl = (unsigned)(tg ? tg[e] : tg0);
    const float u = u01(hkey(rseed, ST_SAMPLE, (unsigned)(env0 + e), tgl, (unsigned)n));
    *out = row_sample(p, z, av, A, u);
  }
}

}  // namespace

extern "C" int marl_policy_sample(const float* logits, const float* avail, long avail_es, const int* alive, float eps,
                                  unsigned rseed, int env0, const int* tg, int tg0, int* act_out, long act_es, int E, int N,
                                  int A, void* stream) {
  const long total = (long)E * N;
  if (total <= 0 || A <= 0) return 0;
  if (!logits || !avail || !act_out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(policy_sample_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, logits,
                     avail, avail_es, alive, eps, rseed, env0, tg, tg0, act_out, act_es, E, N, A);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_policy_probs(const float* logits, const float* avail, float eps, float* pi, long rows, int A, void* stream) {
  if (rows <= 0 || A <= 0) return 0;
  if (!logits || !avail || !pi || pi == avail) return (int)hipErrorInvalidValue;
  PolicyArgs p = {};
  p.logits = logits; p.avail = avail; p.eps = eps; p.out = pi; p.rows = rows; p.N = 1; p.A = A;
  int nb;
  return launch_policy<false>(p, (hipStream_t)stream, nb);
}

extern "C" int marl_policy_loss_bwd(const float* logits, const float* avail, const int* u, const float* G, const float* v,
                                    const float* padded, float eps, float* dlogits, float* logp, float* out2, float* ws,
                                    long rows, int N, int A, void* stream) {
  if (rows <= 0 || A <= 0) return 0;
  if (!logits || !avail || !u || !G || !v || !padded || !dlogits || !logp || !out2 || !ws || N <= 0 || rows % N != 0 ||
      dlogits == avail)
    return (int)hipErrorInvalidValue;
  PolicyArgs p = {};
  p.logits = logits; p.avail = avail; p.u = u; p.G = G; p.v = v; p.padded = padded; p.eps = eps;
  p.out = dlogits; p.logp = logp; p.ws = ws; p.rows = rows; p.N = N; p.A = A;
  int nb;
  const int rc = launch_policy<true>(p, (hipStream_t)stream, nb);
  if (rc) return rc;
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 2, out2);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_policy_loss_bwd_ex(const float* logits, const float* avail, const int* u, const float* G, const float* v,
                                       const float* padded, float eps, float beta, float* dlogits, float* logp, float* ent,
                                       float* out3, float* ws, long rows, int N, int A, void* stream) {
  if (rows <= 0 || A <= 0) return 0;
  if (!logits || !avail || !u || !G || !padded || !dlogits || !logp || !out3 || !ws || N <= 0 || rows % N != 0 ||
      dlogits == avail || !(beta >= 0.f))
    return (int)hipErrorInvalidValue;
  PolicyArgs p = {};
  p.logits = logits; p.avail = avail; p.u = u; p.G = G; p.v = v; p.padded = padded; p.eps = eps; p.beta = beta;
  p.out = dlogits; p.logp = logp; p.ent = ent; p.ws = ws; p.rows = rows; p.N = N; p.A = A;
  int nb;
  const int rc = launch_policy<true, true>(p, (hipStream_t)stream, nb);
  if (rc) return rc;
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 3, out3);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_ppo_loss_bwd(const float* logits, const float* avail, const int* u, const float* adv, const float* logp_old,
                                 const float* padded, float eps, float beta, float clip, float* dlogits, float* logp, float* ent,
                                 float* out4, float* ws, long rows, int N, int A, void* stream) {
  if (rows <= 0 || A <= 0) return 0;
  if (!logits || !avail || !u || !adv || !padded || !dlogits || !logp || !out4 || !ws || N <= 0 || rows % N != 0 ||
      dlogits == avail || !(beta >= 0.f) || !(clip > 0.f && clip < 1.f))
    return (int)hipErrorInvalidValue;
  PpoArgs p = {};
  p.logits = logits; p.avail = avail; p.u = u; p.G = adv; p.logp_old = logp_old; p.padded = padded; p.eps = eps; p.beta = beta;
  p.clip = clip; p.out = dlogits; p.logp = logp; p.ent = ent; p.ws = ws; p.rows = rows; p.N = N; p.A = A;
  int nb;
  const int rc = launch_policy<true, true, true>(p, (hipStream_t)stream, nb);
  if (rc) return rc;
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 4, out4);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_policy_probs_bwd(const float* logits, const float* avail, const float* gpi, const float* q_pi, const float* padded,
                                     float eps, float beta, float* dlogits, float* ent, float* out3, float* ws, long rows, int N,
                                     int A, void* stream) {
  if (rows <= 0 || A <= 0) return 0;
  if (!logits || !avail || !gpi || !padded || !dlogits || !out3 || !ws || N <= 0 || rows % N != 0 || dlogits == avail ||
      !(beta >= 0.f))
    return (int)hipErrorInvalidValue;
  ProbsBwdArgs p = {};
  p.logits = logits; p.avail = avail; p.gpi = gpi; p.q_pi = q_pi; p.padded = padded; p.eps = eps; p.beta = beta;
  p.out = dlogits; p.ent = ent; p.ws = ws; p.rows = rows; p.N = N; p.A = A;
  const rt::Plan pl = rt::plan(rows, A, 3, 56 * 1024, rt::PARTIAL_ROWS, {logits, avail, gpi, dlogits});
  int nb;
  if (pl.tiled) {
    nb = pl.blocks;
    p.vec = pl.vec;
    hipLaunchKernelGGL(probs_bwd_tiled_kernel, dim3((unsigned)nb), dim3(TPB), pl.lds_bytes, (hipStream_t)stream, p);
  } else {
    nb = rt::partial_blocks(rows);
    hipLaunchKernelGGL(probs_bwd_rows_kernel, dim3((unsigned)nb), dim3(TPB), 0, (hipStream_t)stream, p);
  }
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 3, out3);
  MARL_CHECK_LAUNCH();
  return 0;
}
