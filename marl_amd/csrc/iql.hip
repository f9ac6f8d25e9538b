// Independent Q-learning: the learner-specific tail of an update as ONE pass over the agent rows r = (b, t, i), R = B T N
// (include/marl_hip.h has the definition).  Per live row (m = 1 - padded[b, t] != 0):
//   q_taken = q[r, u[r]];   q_next = q_tgt[r, a*], a* the first-index argmax of the masked q_sel[r, :] (q_sel NULL: of q_tgt itself,
//   which is the masked max), the value masked the same way;   y = r[b,t] + gamma (1 - term[b,t]) q_next   (or ret[b, i, t]);
//   td = y - q_taken;   dq_val = - 2 m td;   partial sums { m td^2, m }.
// A row with m = 0 writes exact zeros and none of its row operands enters a computation.
//
// Lane mapping: row_tile.h's - the row operands of the selection (q_sel, q_tgt, avail_next) are what the pass moves, and only those
// given are staged, one after the other.  The taken action's Q is one float per row and is read from global memory directly, with
// the row's other scalars, before the staging so that those loads fly beside it.  The staged form runs while its tiles fit 64 KiB
// less the sums' 64 static bytes: up to A = 21 with three operands (the switch of marl_q_double_select), up to A = 31 with two
// (q_sel or avail_next NULL), any A <= 63 with one; beyond that the same lanes scan their rows in global memory.  The ret mode
// reads no row operand but the gather and never stages.
//
// Sums: sums.h - every workgroup leaves { sum m td^2, sum m } in the workspace, one single-workgroup launch adds the rows in a
// fixed order.  No float atomics: two calls give the same bits.
#include "sums.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;
constexpr size_t IQ_LDS_MAX = 64 * 1024 - 64;   // 64 KiB less the static words of block_partials

struct IqlArgs {
  const float* q; const int* u;
  const float *q_sel, *q_tgt, *avail;    // q_tgt NULL: no selection (the target is ret)
  const float *ret, *r, *term, *padded;
  float gamma, mask_val;
  float *dq_val, *q_taken, *q_next, *q_next_bnt, *ws;   // ws NULL: selection only, no loss
  long rows;
  int T, N, A, vec;
  FastDiv fdN, fdT;
};

// the lane's row of the (staged or global) operands: first-index argmax of the masked sel, the masked val there
__device__ __forceinline__ float iql_select_row(const float* sel, const float* val, const float* av, float mask_val, int A) {
  float best;
  const int arg = rt::masked_argmax_row(sel, av, mask_val, A, &best);
  return (av && av[arg] == 0.f) ? mask_val : val[arg];
}

template <bool STAGED>
__global__ __launch_bounds__(TPB) void iql_rows_kernel(IqlArgs a) {
  extern __shared__ __attribute__((aligned(16))) float iq_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A;
  const bool select = a.q_tgt != nullptr;
  const int nops = (a.q_sel ? 1 : 0) + 1 + (a.avail ? 1 : 0);
  const int TS = rt::tile_floats(A);
  // rt::wave_tiles written out: through the helper the compiler orders this kernel's prologue another way, and the staged form then
  // measures 1.2 % slower at A = 14 and 18 with the same loop body (DESIGN, the section on row_tile.h)
  float* Sv = iq_smem + (size_t)wave * nops * TS;          // q_tgt, then q_sel, then avail - those that are given
  float* Sq = a.q_sel ? Sv + TS : Sv;
  float* Sa = a.avail ? Sv + (a.q_sel ? 2 : 1) * TS : nullptr;
  float acc[2] = {0.f, 0.f};
  const long tiles = rt::tiles(a.rows);
  for (long tile = rt::first_tile(); tile < tiles; tile += rt::tile_step()) {
    const long r0 = tile * rt::ROWS;
    // the row's own scalars first: their loads fly while the tiles are staged (the taken action's Q hangs on u, the target on both)
    const long row = r0 + lane;
    const bool in = row < a.rows;
    long bnt = 0;
    float m = 0.f, qt = 0.f, rr = 0.f, tm = 0.f, yr = 0.f;
    if (in) {
      const unsigned bt = fastdiv((unsigned)row, a.fdN);  // (b, t) = row / N
      const unsigned i = (unsigned)row - bt * (unsigned)a.N;
      const unsigned b = fastdiv(bt, a.fdT);
      const unsigned t = bt - b * (unsigned)a.T;
      bnt = ((long)b * a.N + i) * a.T + t;                // the row's place in (B, N, T) layout
      m = 1.f - a.padded[bt];
      const int ua = a.u[row];
      if (m != 0.f) {
        if ((unsigned)ua < (unsigned)A) qt = a.q[row * A + ua];
        if (!select) yr = a.ret[bnt];
        else if (a.ws) { rr = a.r[bt]; tm = a.term[bt]; }
      }
    }
    if (STAGED) {
      const int n = rt::tile_len(a.rows, r0, A);
      rt::copy(Sv, a.q_tgt + r0 * A, n, a.vec);
      if (a.q_sel) rt::copy(Sq, a.q_sel + r0 * A, n, a.vec);
      if (a.avail) rt::copy(Sa, a.avail + r0 * A, n, a.vec);
      rt::lds_done();
    }
    if (in) {
      float qn = 0.f, dq = 0.f;
      if (m != 0.f) {
        float y = yr;
        if (select) {
          if (STAGED) {
            qn = iql_select_row(Sq + lane * A, Sv + lane * A, Sa ? Sa + lane * A : nullptr, a.mask_val, A);
          } else {
            const float* gv = a.q_tgt + row * A;
            qn = iql_select_row(a.q_sel ? a.q_sel + row * A : gv, gv, a.avail ? a.avail + row * A : nullptr, a.mask_val, A);
          }
          y = rr + a.gamma * qn * (1.f - tm);
        }
        if (a.ws) {
          const float td = y - qt;
          acc[0] += m * td * td;
          acc[1] += m;
          dq = -2.f * m * td;
        }
      }
      if (a.dq_val) a.dq_val[row] = dq;
      if (a.q_taken) a.q_taken[row] = qt;
      if (a.q_next) a.q_next[row] = qn;
      if (a.q_next_bnt) a.q_next_bnt[bnt] = qn;
    }
  }
  if (a.ws) block_partials<2>(acc, a.ws);
}

inline bool iql_overlap(const void* out, size_t out_bytes, const void* in, size_t in_bytes) {
  if (!out || !in) return false;
  const uintptr_t o = reinterpret_cast<uintptr_t>(out), i = reinterpret_cast<uintptr_t>(in);
  return o < i + in_bytes && i < o + out_bytes;
}

// launches the row pass (and the fixed-order finish when it carries a loss)
int iql_launch(IqlArgs a, float* out2, int B, int T, int N, int A, hipStream_t s) {
  const long rows = (long)B * T * N;
  if (rows >= (1L << 31)) return (int)hipErrorInvalidValue;      // 32-bit row arithmetic in the kernel
  a.rows = rows; a.T = T; a.N = N; a.A = A;
  a.fdN = make_fastdiv((unsigned)N); a.fdT = make_fastdiv((unsigned)T);
  const bool select = a.q_tgt != nullptr;
  // every output against every input it is not: an output may not overlap an input, nor another output
  const size_t fr = (size_t)rows * sizeof(float), fa = fr * A, fbt = (size_t)B * T * sizeof(float);
  const void* outs[] = {a.dq_val, a.q_taken, a.q_next, a.q_next_bnt, out2, a.ws};
  const size_t outb[] = {fr, fr, fr, fr, 2 * sizeof(float), marl_loss_workspace(rows)};
  const void* ins[] = {a.q, a.u, a.q_sel, a.q_tgt, a.avail, a.ret, a.r, a.term, a.padded};
  const size_t inb[] = {fa, fr, fa, fa, fa, fr, fbt, fbt, fbt};
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 9; ++i)
      if (iql_overlap(outs[o], outb[o], ins[i], inb[i])) return (int)hipErrorInvalidValue;
    for (int p = 0; p < o; ++p)
      if (iql_overlap(outs[o], outb[o], outs[p], outb[p])) return (int)hipErrorInvalidValue;
  }
  const int nops = (a.q_sel ? 1 : 0) + 1 + (a.avail ? 1 : 0);
  const rt::Plan pl = rt::plan(rows, A, nops, IQ_LDS_MAX, rt::PARTIAL_ROWS, {a.q_sel, a.q_tgt, a.avail});
  a.vec = pl.vec;
  if (select && pl.tiled)
    hipLaunchKernelGGL(iql_rows_kernel<true>, dim3((unsigned)pl.blocks), dim3(TPB), pl.lds_bytes, s, a);
  else                                 // the row-per-lane twin keeps the tile loop, and so the grid
    hipLaunchKernelGGL(iql_rows_kernel<false>, dim3((unsigned)pl.blocks), dim3(TPB), 0, s, a);
  MARL_CHECK_LAUNCH();
  if (a.ws) {
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, s, (const float*)a.ws, pl.blocks, 2, out2);
    MARL_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int marl_iql_loss_bwd(const float* q, const int* u, const float* q_sel, const float* q_tgt, const float* avail_next,
                                 const float* ret, const float* r, const float* term, const float* padded, float gamma,
                                 float mask_val, float* dq_val, float* q_taken, float* q_next, float* out2, float* ws, int B, int T,
                                 int N, int A, void* stream) {
  if (A < 1 || N < 1) return (int)hipErrorInvalidValue;
  if (B <= 0 || T <= 0) return 0;
  if (!q || !u || !padded || !dq_val || !out2 || !ws) return (int)hipErrorInvalidValue;
  if (!ret && (!q_tgt || !r || !term)) return (int)hipErrorInvalidValue;
  IqlArgs a = {};
  a.q = q; a.u = u; a.padded = padded; a.gamma = gamma; a.mask_val = mask_val;
  a.dq_val = dq_val; a.q_taken = q_taken; a.ws = ws;
  if (ret) {
    a.ret = ret;                         // (B, N, T); q_sel, q_tgt, avail_next, r and term are not read, q_next is not written
  } else {
    a.q_sel = q_sel; a.q_tgt = q_tgt; a.avail = avail_next; a.r = r; a.term = term; a.q_next = q_next;
  }
  return iql_launch(a, out2, B, T, N, A, (hipStream_t)stream);
}

extern "C" int marl_iql_select(const float* q, const int* u, const float* q_sel, const float* q_tgt, const float* avail_next,
                               const float* padded, float mask_val, float* q_taken, float* q_next_bnt, int B, int T, int N, int A,
                               void* stream) {
  if (A < 1 || N < 1) return (int)hipErrorInvalidValue;
  if (B <= 0 || T <= 0) return 0;
  if (!q || !u || !q_tgt || !padded || !q_next_bnt) return (int)hipErrorInvalidValue;
  IqlArgs a = {};
  a.q = q; a.u = u; a.q_sel = q_sel; a.q_tgt = q_tgt; a.avail = avail_next; a.padded = padded; a.mask_val = mask_val;
  a.q_taken = q_taken; a.q_next_bnt = q_next_bnt;
  return iql_launch(a, nullptr, B, T, N, A, (hipStream_t)stream);
}
