// Qatten mixer (Yang et al. 2020), the row kernel: multi-head attention over the per-agent unit features of a state row gives the
// mixing weights.  Per row, with u_i = s[i U : (i + 1) U] (read in place from the state rows the callers hold), H heads:
//   l_{h,i} = scale (p_h . u_i),  lam_{h,.} = softmax_i(l_{h,.}),  y_h = sum_i lam_{h,i} q_i,  q_tot = sum_h |w_raw_h| y_h + c.
// p_h = Wk_h^T e_h is the key layer applied to the QUERY side (e_h . (Wk_h u_i) = (Wk_h^T e_h) . u_i): the N keys of a row are never
// built, the kernel has no weight of its own and no cross-row reduction but the two loss sums.  The backward recomputes lam; nothing
// H N wide is kept between forward and backward:
//   a_i = sum_h |w_raw_h| lam_{h,i},  dq_i = g a_i,  dw_raw_h = g y_h sign(w_raw_h),  dl_{h,i} = g |w_raw_h| lam_{h,i} (q_i - y_h),
//   dp_h = scale sum_i dl_{h,i} u_i,  dc = g.
//
// Tile plan.  One lane on one row against global memory reads 480 - 1288-byte rows at a lane stride of a row (the lesson above
// qplex_mix_fwd_tiled_kernel in mixers.hip), so a workgroup owns a tile of TR consecutive rows and stages them through LDS: a row's
// N U state floats and its H U + H + 1 floats of hy are copied as they lie, consecutive lanes on consecutive 16-byte pieces - single
// floats up to the row's first 16-byte boundary, 16 bytes per lane after it, single floats at the tail; the boundary is found per row,
// because a 1288-byte state row pitch (S = 322) leaves odd rows 8-byte aligned only - and the outputs leave the same way.  The LDS row pitches are odd, so the lanes of a wave, which walk
// different rows, spread over the banks.  The arithmetic runs out of LDS with one lane per (row, head): a lane holds the N logits of
// its head in registers, never the row's H N.  TR is the largest tile with TR H <= 256 lanes, TR <= 64 rows and at most 76 KB of
// LDS (two workgroups per CU): 64 rows at 2s3z (N 5, U 24, H 4), 37 at MMM2 (N 10, U 32, H 4), 11 in the support corner
// (N 16, U 64, H 8).  marl_qatten_plan reports it.
//
// The three entry points are one kernel template: the same row arithmetic in the same order, with fp contraction off for the whole
// file, so the loss-folded launch gives the bits of mix_fwd -> marl_td_loss -> mix_bwd.
#include "common.h"
#include "sums.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

#pragma clang fp contract(off)

namespace {
namespace rt = row_tile;

constexpr int TPB = SUMS_TPB;
constexpr int MAXN = 16, MAXU = 64, MAXH = 8;          // the support range
constexpr int MAX_TILE = 64;                           // rows per tile at most
constexpr size_t LDS_CAP = 76 * 1024;                  // two workgroups in a CU's 160 KB

enum { MODE_FWD = 0, MODE_BWD = 1, MODE_LOSS = 2 };

// LDS image of a tile, floats: state row offsets [TR] (64-bit) | states [TR][SP] | hy rows [TR][HP] (p, w_raw, c in; dp, dw_raw out, in place) | q [TR][N] |
// |w| lam [TR][H][N] | y [TR][H] | dq [TR][N] | g [TR]
struct Tile { int TR, SP, HP; size_t lds; };
inline Tile tile_of(int N, int U, int H) {
  Tile t;
  t.SP = (N * U) | 1;
  t.HP = (H * U + H + 1) | 1;
  const size_t row = (size_t)(2 + t.SP + t.HP + N + H * N + H + N + 1) * sizeof(float);
  long tr = (long)(LDS_CAP / row);
  if (tr > MAX_TILE) tr = MAX_TILE;
  if (tr > TPB / H) tr = TPB / H;
  t.TR = (int)(tr < 1 ? 1 : tr);
  t.lds = row * t.TR;
  return t;
}

struct QaArgs {
  ConcatSrc s;
  const float* hy; long ldh;                 // (rows, ldh): [p (H U) | w_raw (H) | c (1)]
  const float* q;                            // (rows, N)
  float scale;
  const float* g_in;                         // MODE_BWD: dL/dq_tot (rows)
  const float *q_tgt, *r, *term, *padded;    // MODE_LOSS
  float gamma;
  float* q_tot;                              // (rows); optional in MODE_LOSS, unused in MODE_BWD
  float* dq;                                 // (rows, N)
  float* dhy; long lddh;                     // (rows, lddh): [dp (H U) | dw_raw (H)]
  float* dq_tot;                             // MODE_LOSS: (rows)
  float* ws;                                 // MODE_LOSS: loss workspace
  long rows;
  int N, U, H, TR, SP, HP;
};

// Tile copies.  A row of n floats is cut into chunks: chunk 0 the floats before the row's first 16-byte boundary (none to three),
// chunk j >= 1 the four floats from there on, the last one short.  The workgroup walks the (row, chunk) items of the tile in row
// order - consecutive lanes take consecutive 16-byte pieces of a row - and every lane issues the loads of four items before it stores
// the first: a copy that waits for each row in turn runs at one memory latency per row.
struct Chunk { int lo, cnt; bool vec; };              // floats [lo, lo + cnt) of the row; vec: one aligned 16-byte access
__device__ __forceinline__ Chunk chunk_of(const float* g, int n, int j) {
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3);
  head = head < n ? head : n;
  Chunk c;
  c.lo = j ? head + 4 * (j - 1) : 0;
  c.cnt = j ? (n - c.lo < 4 ? n - c.lo : 4) : head;
  if (c.cnt < 0) c.cnt = 0;
  c.vec = j && c.cnt == 4;
  return c;
}
__device__ __forceinline__ int chunks_of(int n) { return 1 + (n + 3) / 4; }

// rows rl < nr of n floats, global (base + off_of(rl); a negative offset reads as zeros) -> LDS rows of `pitch` floats
template <class F>
__device__ __forceinline__ void tile_in(float* lds, int pitch, const float* base, F off_of, int n, int nr) {
  const int CH = chunks_of(n), items = nr * CH;
  for (int it0 = threadIdx.x; it0 < items; it0 += 4 * TPB) {
    f32x4 v[4];
    Chunk c[4];
    int at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + u * TPB;
      c[u].cnt = 0; c[u].lo = 0; c[u].vec = false; at[u] = 0;
      v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (it < items) {
        const int rl = it / CH, j = it - rl * CH;
        const long off = off_of(rl);
        const float* g = base + (off < 0 ? 0 : off);
        c[u] = chunk_of(g, n, j);
        at[u] = rl * pitch + c[u].lo;
        if (off >= 0) {
          if (c[u].vec) v[u] = *reinterpret_cast<const f32x4*>(g + c[u].lo);
          else
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < c[u].cnt) v[u][e] = g[c[u].lo + e];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < c[u].cnt) lds[at[u] + e] = v[u][e];
  }
}
// LDS rows of `pitch` floats -> rows rl < nr of n floats at g0 + rl * ld
__device__ __forceinline__ void tile_out(float* g0, long ld, const float* lds, int pitch, int n, int nr) {
  const int CH = chunks_of(n), items = nr * CH;
  for (int it = threadIdx.x; it < items; it += TPB) {
    const int rl = it / CH, j = it - rl * CH;
    float* g = g0 + rl * ld;
    const Chunk c = chunk_of(g, n, j);
    const float* d = lds + rl * pitch + c.lo;
    if (c.vec) *reinterpret_cast<f32x4*>(g + c.lo) = (f32x4){d[0], d[1], d[2], d[3]};
    else
      for (int e = 0; e < c.cnt; ++e) g[c.lo + e] = d[e];
  }
}

// head h of a row: the softmax weights lam[0..N) (registers) and y_h.  p, u, q: LDS
__device__ __forceinline__ float head_fwd(const float* p, const float* u, const float* q, float scale, int N, int U, float (&lam)[MAXN]) {
#pragma unroll
  for (int i = 0; i < MAXN; ++i) lam[i] = 0.f;
  // every logit sums its products in the order k = 0 .. U - 1; the N sums advance side by side, so a trip's N + 1 LDS reads are
  // in flight together
#pragma unroll 4
  for (int k = 0; k < U; ++k) {
    const float pk = p[k];
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
      if (i < N) lam[i] += pk * u[i * U + k];
  }
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < MAXN; ++i)
    if (i < N) {
      lam[i] = scale * lam[i];
      mx = (i == 0 || lam[i] > mx) ? lam[i] : mx;
    }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXN; ++i)
    if (i < N) { lam[i] = expf(lam[i] - mx); sum += lam[i]; }      // the largest logit gives exp(0) = 1: sum >= 1
  float y = 0.f;
#pragma unroll
  for (int i = 0; i < MAXN; ++i)
    if (i < N) { lam[i] = lam[i] / sum; y += lam[i] * q[i]; }
  return y;
}

// head h of a row, backward: dp_h over p_h (in place) and dw_raw_h; lam, y from head_fwd
__device__ __forceinline__ float head_bwd(float* p, const float* u, const float* q, float scale, int N, int U, float g, float w, float y,
                                          float (&lam)[MAXN]) {
  const float ga = g * fabsf(w);
#pragma unroll
  for (int i = 0; i < MAXN; ++i)
    if (i < N) lam[i] = ga * lam[i] * (q[i] - y);          // dl_{h,i}
#pragma unroll 4
  for (int k = 0; k < U; ++k) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < MAXN; ++i)
      if (i < N) d += lam[i] * u[i * U + k];
    p[k] = scale * d;
  }
  return g * y * (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f));
}

template <int MODE>
__global__ __launch_bounds__(TPB) void qatten_kernel(QaArgs a) {
  extern __shared__ __attribute__((aligned(16))) float qa_smem[];
  const int N = a.N, U = a.U, H = a.H, TR = a.TR, SP = a.SP, HP = a.HP;
  const int NU = N * U, HU = H * U;
  long* Ro = reinterpret_cast<long*>(qa_smem);         // [TR] element offsets of the state rows (-1: the row reads as zeros)
  float* Ss = qa_smem + 2 * TR;
  float* Hs = Ss + (size_t)TR * SP;
  float* Qs = Hs + (size_t)TR * HP;
  float* WL = Qs + TR * N;
  float* Ys = WL + TR * H * N;
  float* Dq = Ys + TR * H;
  float* Gs = Dq + TR * N;
  const int tid = threadIdx.x;
  float acc[2] = {0.f, 0.f};
  for (long r0 = (long)blockIdx.x * TR; r0 < a.rows; r0 += (long)gridDim.x * TR) {
    const int nr = (int)(a.rows - r0 < TR ? a.rows - r0 : TR);
    // ---- stage the tile
    for (int rl = tid; rl < nr; rl += TPB) {
      const ConcatRow cr = concat_row(a.s, r0 + rl);
      Ro[rl] = cr.ok0 ? cr.r0 * a.s.ld0 : -1;
    }
    __syncthreads();
    tile_in(Ss, SP, a.s.p0, [&](int rl) { return Ro[rl]; }, NU, nr);
    tile_in(Hs, HP, a.hy + r0 * a.ldh, [&](int rl) { return rl * a.ldh; }, HU + H + 1, nr);
    for (int e = tid; e < nr * N; e += TPB) Qs[e] = a.q[r0 * N + e];
    __syncthreads();
    // ---- (row, head): softmax weights and y_h
    const bool act = tid < nr * H;
    const int rl = tid / H, h = tid - rl * H;
    float lam[MAXN];
    float y = 0.f, w = 0.f;
    if (act) {
      y = head_fwd(Hs + rl * HP + h * U, Ss + rl * SP, Qs + rl * N, a.scale, N, U, lam);
      w = Hs[rl * HP + HU + h];
      Ys[tid] = y;
      if (MODE != MODE_FWD) {
        const float aw = fabsf(w);
#pragma unroll
        for (int i = 0; i < MAXN; ++i)
          if (i < N) WL[tid * N + i] = aw * lam[i];
      }
    }
    __syncthreads();
    // ---- row: q_tot, and the gradient on it
    if (tid < nr) {
      const long r = r0 + tid;
      float g = 0.f;
      if (MODE != MODE_BWD) {
        float qt = 0.f;
        for (int hh = 0; hh < H; ++hh) qt += fabsf(Hs[tid * HP + HU + hh]) * Ys[tid * H + hh];
        qt += Hs[tid * HP + HU + H];
        if (a.q_tot) a.q_tot[r] = qt;
        if (MODE == MODE_LOSS) {                 // td_loss_kernel's expressions (mixers.hip), contracted as that file's are
#pragma clang fp contract(fast)
          const float mask = 1.f - a.padded[r];
          const float target = a.r[r] + a.gamma * a.q_tgt[r] * (1.f - a.term[r]);
          const float td = target - qt;
          const float mtd = mask * td;
          acc[0] += mtd * mtd;
          acc[1] += mask;
          g = -2.f * mask * mtd;
          a.dq_tot[r] = g;
        }
      } else {
        g = a.g_in[r];
      }
      if (MODE != MODE_FWD) Gs[tid] = g;
    }
    if (MODE != MODE_FWD) {
      __syncthreads();
      // ---- (row, head): dp_h, dw_raw_h;  (row, agent): dq_i
      if (act) Hs[rl * HP + HU + h] = head_bwd(Hs + rl * HP + h * U, Ss + rl * SP, Qs + rl * N, a.scale, N, U, Gs[rl], w, y, lam);
      for (int e = tid; e < nr * N; e += TPB) {
        const int row = e / N, i = e - row * N;
        float ai = 0.f;
        for (int hh = 0; hh < H; ++hh) ai += WL[(row * H + hh) * N + i];
        Dq[e] = Gs[row] * ai;
      }
      __syncthreads();
      tile_out(a.dhy + r0 * a.lddh, a.lddh, Hs, HP, HU + H, nr);
      for (int e = tid; e < nr * N; e += TPB) a.dq[r0 * N + e] = Dq[e];
    }
    __syncthreads();                             // the tile is free for the next round
  }
  if (MODE == MODE_LOSS) block_partials<2>(acc, a.ws);
}

inline bool shape_ok(int N, int U, int H) { return N >= 1 && N <= MAXN && U >= 1 && U <= MAXU && H >= 1 && H <= MAXH; }
// segment 0 alone, wide enough for the N unit blocks; the row remap and the episode map are honoured
inline bool src_ok(const marl_src_t* s, int N, int U) {
  return s && s->p0 && s->k0 >= N * U && s->ld0 >= N * U && !s->k1 && !s->nhot && !s->nid && !s->m0 && s->rpe0 >= 0 &&
         (!s->emap0 || s->rpe0 > 0) && (reinterpret_cast<uintptr_t>(s->p0) & 3) == 0;
}
inline ConcatSrc state_src(const marl_src_t* s) {
  ConcatSrc c = {};
  c.p0 = s->p0; c.ld0 = s->ld0; c.k0 = s->k0;
  c.rpe0 = s->rpe0; c.bs0 = s->bs0; c.off0 = s->off0;
  c.fd0 = make_fastdiv((unsigned)(s->rpe0 > 0 ? s->rpe0 : 1));
  c.fdi = make_fastdiv(1); c.fdn = make_fastdiv(1);
  c.emap0 = s->emap0;
  return c;
}
inline int grid_of(long rows, int TR) {
  const long t = (rows + TR - 1) / TR;
  return (int)(t > rt::PARTIAL_ROWS ? rt::PARTIAL_ROWS : t);        // the loss workspace holds this many rows of partials
}

template <int MODE>
int launch(QaArgs& a, const marl_src_t* s, hipStream_t stream) {
  if (!shape_ok(a.N, a.U, a.H) || !src_ok(s, a.N, a.U) || a.rows >= (1L << 31) || !a.hy || !a.q || a.ldh < a.H * a.U + a.H + 1)
    return (int)hipErrorInvalidValue;
  if (MODE != MODE_FWD && (!a.dq || !a.dhy || a.lddh < a.H * a.U + a.H)) return (int)hipErrorInvalidValue;
  const Tile t = tile_of(a.N, a.U, a.H);
  a.s = state_src(s);
  a.TR = t.TR; a.SP = t.SP; a.HP = t.HP;
  const void* fn = (const void*)qatten_kernel<MODE>;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {(void*)&a};
  e = hipLaunchKernel(fn, dim3((unsigned)grid_of(a.rows, t.TR)), dim3(TPB), kargs, t.lds, stream);
  if (e != hipSuccess) return (int)e;
  MARL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int marl_qatten_supported(const marl_src_t* s, int N, int U, int H) { return shape_ok(N, U, H) && src_ok(s, N, U) ? 1 : 0; }

extern "C" int marl_qatten_plan(long rows, int N, int U, int H, int* plan) {
  if (!shape_ok(N, U, H) || rows >= (1L << 31)) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 4; ++i) plan[i] = 0;
  if (rows <= 0) return 0;
  const Tile t = tile_of(N, U, H);
  plan[0] = t.TR;
  plan[1] = grid_of(rows, t.TR);
  plan[2] = (int)t.lds;
  const long tiles = (rows + t.TR - 1) / t.TR;
  plan[3] = (int)((tiles + plan[1] - 1) / plan[1]);
  return 0;
}

extern "C" int marl_qatten_mix_fwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale, float* q_tot,
                                   long rows, int N, int U, int H, void* stream) {
  if (rows <= 0) return 0;
  if (!q_tot) return (int)hipErrorInvalidValue;
  QaArgs a = {};
  a.hy = hy; a.ldh = ldh; a.q = q; a.scale = scale; a.q_tot = q_tot; a.rows = rows; a.N = N; a.U = U; a.H = H;
  return launch<MODE_FWD>(a, s, (hipStream_t)stream);
}

extern "C" int marl_qatten_mix_bwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale, const float* dq_tot,
                                   float* dq, float* dhy, long lddh, long rows, int N, int U, int H, void* stream) {
  if (rows <= 0) return 0;
  if (!dq_tot) return (int)hipErrorInvalidValue;
  QaArgs a = {};
  a.hy = hy; a.ldh = ldh; a.q = q; a.scale = scale; a.g_in = dq_tot; a.dq = dq; a.dhy = dhy; a.lddh = lddh;
  a.rows = rows; a.N = N; a.U = U; a.H = H;
  return launch<MODE_BWD>(a, s, (hipStream_t)stream);
}

extern "C" int marl_qatten_loss_bwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale,
                                    const float* q_tot_tgt, const float* r, const float* term, const float* padded, float gamma,
                                    float* q_tot, float* dq, float* dhy, long lddh, float* dq_tot, float* out2, float* ws, long rows,
                                    int N, int U, int H, void* stream) {
  if (rows <= 0) return 0;
  if (!q_tot_tgt || !r || !term || !padded || !dq_tot || !out2 || !ws) return (int)hipErrorInvalidValue;
  QaArgs a = {};
  a.hy = hy; a.ldh = ldh; a.q = q; a.scale = scale; a.q_tgt = q_tot_tgt; a.r = r; a.term = term; a.padded = padded; a.gamma = gamma;
  a.q_tot = q_tot; a.dq = dq; a.dhy = dhy; a.lddh = lddh; a.dq_tot = dq_tot; a.ws = ws;
  a.rows = rows; a.N = N; a.U = U; a.H = H;
  const int rc = launch<MODE_LOSS>(a, s, (hipStream_t)stream);
  if (rc) return rc;
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const float*)ws, grid_of(rows, a.TR), 2, out2);
  MARL_CHECK_LAUNCH();
  return 0;
}
