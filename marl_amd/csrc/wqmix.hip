// Weighted QMIX (Rashid et al., NeurIPS 2020; include/marl_hip.h has the definition): the learner-specific parts of an update as
// two plain row passes.
//
// marl_wqmix_select, ONE pass over the agent rows r = (b, t, i), R = B T N.  Per live row (m = 1 - padded[b, t] != 0):
//   q_taken = q[r, u],  qc_taken = qc[r, u]                                      (u outside [0, A): both 0)
//   u_next = first-index argmax of q_en[r, :] masked with avail_next,  qc_next = qc_tgt[r, u_next] masked the same way
//   u_greedy = first-index argmax of q[r, :] masked with avail,  qc_greedy = qc[r, u_greedy]   (optional: CW's)
// A row with m = 0 writes exact zeros and -1 and none of its row operands or its u enters a computation.
// Lane mapping: row_tile.h's, as iql.hip - a wave stages 64 rows of the next-step operands (q_en, qc_tgt, avail_next), selects,
// then stages the current-step operands (q, qc, avail) over the same tiles and selects again.  The taken action's two values are one
// float per row each and are read from global memory before the staging, so that those loads fly beside it.  The staged form runs
// while three (without any availability: two) tiles per wave fit iql.hip's budget - up to A = 21 (31) -, beyond that the same lanes
// scan their rows in global memory: same comparisons, same bits.
//
// marl_wqmix_loss, one pass over the B T rows: marl_td_loss's partition of the rows and its expressions for the target and td, the
// weight on the kernel's own target, both gradients and four sums through sums.h.  No float atomics: two calls give the same bits.
#include "sums.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;
constexpr size_t WQ_LDS_MAX = 64 * 1024 - 64;   // iql.hip's tile budget
constexpr int WQ_MAX_N = 16, WQ_MAX_A = 32;

struct SelArgs {
  const float *q, *qc, *avail;                  // the current step's rows (avail NULL: everything available)
  const float *q_en, *qc_tgt, *avail_next;      // the next step's
  const int* u;
  const float* padded;
  float mask_val;
  float *q_taken, *qc_taken, *qc_greedy, *qc_next;
  int *u_greedy, *u_next;
  long rows;
  int N, A, vec;
  FastDiv fdN;
};

template <bool STAGED>
__global__ __launch_bounds__(TPB) void wqmix_select_kernel(SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) float wq_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A;
  const bool greedy = a.u_greedy != nullptr || a.qc_greedy != nullptr;
  const int nops = 2 + ((a.avail_next || (greedy && a.avail)) ? 1 : 0);
  const int TS = rt::tile_floats(A);
  float* S0 = wq_smem + (size_t)wave * nops * TS;          // the selecting Qs, then the selected ones, then the availability
  float* S1 = S0 + TS;
  float* S2 = S1 + TS;                                     // (only touched when nops = 3)
  const long tiles = rt::tiles(a.rows);
  for (long tile = rt::first_tile(); tile < tiles; tile += rt::tile_step()) {
    const long r0 = tile * rt::ROWS;
    const long row = r0 + lane;
    const bool in = row < a.rows;
    bool live = false;
    float qt = 0.f, qct = 0.f, qcg = 0.f, qcn = 0.f;
    int ug = -1, un = -1;
    if (in) {
      const unsigned bt = fastdiv((unsigned)row, a.fdN);   // (b, t) = row / N
      live = (1.f - a.padded[bt]) != 0.f;
      if (live) {
        const int ua = a.u[row];
        if ((unsigned)ua < (unsigned)A) { qt = a.q[row * A + ua]; qct = a.qc[row * A + ua]; }
      }
    }
    const int n = rt::tile_len(a.rows, r0, A);
    // the next step: u_next by the continuation's Qs, the target central agent's Q there
    if (STAGED) {
      rt::copy(S0, a.q_en + r0 * A, n, a.vec);
      rt::copy(S1, a.qc_tgt + r0 * A, n, a.vec);
      if (a.avail_next) rt::copy(S2, a.avail_next + r0 * A, n, a.vec);
      rt::lds_done();
    }
    if (live) {
      const float* sel = STAGED ? S0 + lane * A : a.q_en + row * A;
      const float* val = STAGED ? S1 + lane * A : a.qc_tgt + row * A;
      const float* av = !a.avail_next ? nullptr : (STAGED ? S2 + lane * A : a.avail_next + row * A);
      float best;
      un = rt::masked_argmax_row(sel, av, a.mask_val, A, &best);
      qcn = (av && av[un] == 0.f) ? a.mask_val : val[un];
    }
    // the current step (CW): u_greedy by the eval agent's Qs, the central agent's Q there
    if (greedy) {
      if (STAGED) {
        rt::lds_done_fenced();                             // the rows above are read before the tiles are written again
        rt::copy(S0, a.q + r0 * A, n, a.vec);
        rt::copy(S1, a.qc + r0 * A, n, a.vec);
        if (a.avail) rt::copy(S2, a.avail + r0 * A, n, a.vec);
        rt::lds_done();
      }
      if (live) {
        const float* sel = STAGED ? S0 + lane * A : a.q + row * A;
        const float* val = STAGED ? S1 + lane * A : a.qc + row * A;
        const float* av = !a.avail ? nullptr : (STAGED ? S2 + lane * A : a.avail + row * A);
        float best;
        ug = rt::masked_argmax_row(sel, av, a.mask_val, A, &best);
        qcg = val[ug];
      }
    }
    if (STAGED) rt::lds_done_fenced();                     // .. and before the next tile's
    if (in) {
      a.q_taken[row] = qt;
      a.qc_taken[row] = qct;
      a.u_next[row] = un;
      a.qc_next[row] = qcn;
      if (a.u_greedy) a.u_greedy[row] = ug;
      if (a.qc_greedy) a.qc_greedy[row] = qcg;
    }
  }
}

struct LossArgs {
  const float *q_tot, *qc, *qc_g, *qn, *r, *term, *padded;   // qc_g NULL: OW
  const int *u, *ug;                                         // (rows, N), CW only
  float gamma, alpha;
  float *dq_tot, *dqc, *w, *ws;
  long rows;
  int N;
};

// marl_td_loss's loop (mixers.hip: td_loss_kernel) with the weight and the second regression; a padded row is skipped, which adds
// what td_loss_kernel's 0 * td adds on finite inputs: nothing
__global__ __launch_bounds__(TPB) void wqmix_loss_kernel(LossArgs a) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < a.rows; i += (long)gridDim.x * TPB) {
    const float mask = 1.f - a.padded[i];
    float dq = 0.f, dc = 0.f, w = 0.f;
    if (mask != 0.f) {
      const float target = a.r[i] + a.gamma * a.qn[i] * (1.f - a.term[i]);
      const float td = target - a.q_tot[i];
      const float mtd = mask * td;
      const float tdc = target - a.qc[i];
      const float mtdc = mask * tdc;
      bool one;
      if (a.qc_g) {                                        // CW: the joint action is the greedy one, or the target says it is better
        one = target > a.qc_g[i];
        if (!one) {
          one = true;
          for (int n = 0; n < a.N; ++n) one = one && a.u[i * a.N + n] == a.ug[i * a.N + n];
        }
      } else {                                             // OW: Q_tot underestimates
        one = td > 0.f;
      }
      w = one ? 1.f : a.alpha;
      const float wmtd = w * mtd;
      acc[0] += wmtd * mtd;
      acc[1] += mask;
      acc[2] += mtdc * mtdc;
      acc[3] += w == 1.f ? mask : 0.f;
      dq = -2.f * mask * mtd * w;
      dc = -2.f * mask * mtdc;
    }
    a.dq_tot[i] = dq;
    a.dqc[i] = dc;
    if (a.w) a.w[i] = w;
  }
  block_partials<4>(acc, a.ws);
}

inline bool wq_overlap(const void* out, size_t out_bytes, const void* in, size_t in_bytes) {
  if (!out || !in) return false;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out), i = reinterpret_cast<uintptr_t>(in);
  return o < i + in_bytes && i < o + out_bytes;
}

// an output may not overlap an input, nor another output
template <int NO, int NI>
inline bool wq_any_overlap(const void* const (&outs)[NO], const size_t (&outb)[NO], const void* const (&ins)[NI],
                           const size_t (&inb)[NI]) {
  for (int o = 0; o < NO; ++o) {
    for (int i = 0; i < NI; ++i)
      if (wq_overlap(outs[o], outb[o], ins[i], inb[i])) return true;
    for (int p = 0; p < o; ++p)
      if (wq_overlap(outs[o], outb[o], outs[p], outb[p])) return true;
  }
  return false;
}

}  // namespace

extern "C" int marl_wqmix_supported(int N, int A) { return N >= 1 && N <= WQ_MAX_N && A >= 1 && A <= WQ_MAX_A; }

extern "C" int marl_wqmix_select(const float* q, const float* qc, const int* u, const float* avail, const float* q_en,
                                 const float* qc_tgt, const float* avail_next, const float* padded, float mask_val,
                                 float* q_taken, float* qc_taken, int* u_greedy, float* qc_greedy, int* u_next, float* qc_next,
                                 int B, int T, int N, int A, void* stream) {
  if (!marl_wqmix_supported(N, A)) return (int)hipErrorInvalidValue;
  if (B <= 0 || T <= 0) return 0;
  if (!q || !qc || !u || !q_en || !qc_tgt || !padded || !q_taken || !qc_taken || !u_next || !qc_next)
    return (int)hipErrorInvalidValue;
  const long rows = (long)B * T * N;
  if (rows >= (1L << 31)) return (int)hipErrorInvalidValue;      // 32-bit row arithmetic in the kernel
  const size_t fr = (size_t)rows * sizeof(float), fa = fr * A, fbt = (size_t)B * T * sizeof(float);
  const void* const outs[] = {q_taken, qc_taken, u_greedy, qc_greedy, u_next, qc_next};
  const size_t outb[] = {fr, fr, fr, fr, fr, fr};
  const void* const ins[] = {q, qc, u, avail, q_en, qc_tgt, avail_next, padded};
  const size_t inb[] = {fa, fa, fr, fa, fa, fa, fa, fbt};
  if (wq_any_overlap(outs, outb, ins, inb)) return (int)hipErrorInvalidValue;
  SelArgs a = {};
  a.q = q; a.qc = qc; a.avail = avail; a.q_en = q_en; a.qc_tgt = qc_tgt; a.avail_next = avail_next; a.u = u; a.padded = padded;
  a.mask_val = mask_val;
  a.q_taken = q_taken; a.qc_taken = qc_taken; a.qc_greedy = qc_greedy; a.qc_next = qc_next; a.u_greedy = u_greedy; a.u_next = u_next;
  a.rows = rows; a.N = N; a.A = A;
  a.fdN = make_fastdiv((unsigned)N);
  const bool greedy = u_greedy || qc_greedy;
  const int nops = 2 + ((avail_next || (greedy && avail)) ? 1 : 0);
  const rt::Plan pl = rt::plan(rows, A, nops, WQ_LDS_MAX, rt::PARTIAL_ROWS, {q, qc, avail, q_en, qc_tgt, avail_next});
  a.vec = pl.vec;
  if (pl.tiled)
    hipLaunchKernelGGL(wqmix_select_kernel<true>, dim3((unsigned)pl.blocks), dim3(TPB), pl.lds_bytes, (hipStream_t)stream, a);
  else                                 // the row-per-lane twin keeps the tile loop, and so the grid
    hipLaunchKernelGGL(wqmix_select_kernel<false>, dim3((unsigned)pl.blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_wqmix_loss(const float* q_tot, const float* qc, const float* qc_g, const float* qc_next_tot, const float* r,
                               const float* term, const float* padded, float gamma, const int* u, const int* u_greedy, float alpha,
                               float* dq_tot, float* dqc, float* w, float* out4, float* ws, long rows, int N, void* stream) {
  if (N < 1 || N > WQ_MAX_N || !(alpha >= 0.f && alpha <= 1.f)) return (int)hipErrorInvalidValue;
  if (rows <= 0) return 0;
  if (!q_tot || !qc || !qc_next_tot || !r || !term || !padded || !dq_tot || !dqc || !out4 || !ws) return (int)hipErrorInvalidValue;
  if (qc_g && (!u || !u_greedy)) return (int)hipErrorInvalidValue;
  if (rows >= (1L << 31)) return (int)hipErrorInvalidValue;
  const size_t fr = (size_t)rows * sizeof(float), fn = fr * N;
  const void* const outs[] = {dq_tot, dqc, w, out4, ws};
  const size_t outb[] = {fr, fr, fr, 4 * sizeof(float), marl_loss_workspace(rows)};
  const void* const ins[] = {q_tot, qc, qc_g, qc_next_tot, r, term, padded, qc_g ? u : nullptr, qc_g ? u_greedy : nullptr};
  const size_t inb[] = {fr, fr, fr, fr, fr, fr, fr, fn, fn};
  if (wq_any_overlap(outs, outb, ins, inb)) return (int)hipErrorInvalidValue;
  LossArgs a = {};
  a.q_tot = q_tot; a.qc = qc; a.qc_g = qc_g; a.qn = qc_next_tot; a.r = r; a.term = term; a.padded = padded;
  a.u = u; a.ug = u_greedy; a.gamma = gamma; a.alpha = alpha;
  a.dq_tot = dq_tot; a.dqc = dqc; a.w = w; a.ws = ws; a.rows = rows; a.N = N;
  const int nb = rt::partial_blocks(rows);
  hipLaunchKernelGGL(wqmix_loss_kernel, dim3(nb), dim3(TPB), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, nb, 4, out4);
  MARL_CHECK_LAUNCH();
  return 0;
}
