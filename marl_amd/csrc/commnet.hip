// CommNet communication head on gfx950 (the project's own definition, include/marl_hip.h): K rounds of f_comm = GRUCell(64, 64)
// over the hidden states of ONE environment-step, then the decoding layer.  With g^(-1) = h (the N agent rows of a group):
//   g^(0) = f_comm(0, h)                                            round 0: the input side is b_ih alone, no product
//   g^(j) = f_comm(c^(j), g^(j-1)),  c_i = (sum_l g_l - g_i) / N    the divisor is N, not N - 1; nothing is masked
//   logits = decoding(g^(K-1))
//
// Both kernels: 256 threads = four waves; a workgroup walks 16-row tiles in a grid-stride loop.  A tile holds 16 / N WHOLE groups
// (rows 0 .. (16 / N) N - 1; the rest of the tile is zero rows that are never written), so every sum over a group's agents is a sum
// over rows of one LDS tile and nothing couples two groups.  Wave w owns the hidden columns 16 w .. 16 w + 15 of all three gates;
// lane l = 16 q + m supplies row m of the A operand and column 16 w + m of the B operand of v_mfma_f32_16x16x4_f32 (the
// K-permutation of common.h: step i of a 16-chunk takes k = 4 q + i), and holds rows 4 q + r (r = 0 .. 3), column 16 w + m of the
// result.  The B fragments of W_ih and W_hh (2 x 3 gates x 4 chunks x 4 floats = 96 registers per lane) and of the decoding weight
// are loaded once per workgroup and stay in registers across the rounds and the tiles.
//
// c is formed in LDS: one pass over the tile's 16 x 64 elements, each the column sum over its group's rows minus the row's own
// value, times 1 / N - the (N, N, H) tensor of the published repeat / mask / mean form never exists.
//
// Backward: the g planes of all rounds are recomputed from hs into LDS (K + 1 planes), the gates of a round once more inside its
// reverse step - nothing but hs is read from memory, nothing is kept by the forward.  Reverse step j: the pointwise GRU backward gives
// dgi, dgh (16 x 192 each, LDS); dW_ih += dgi^T c, dW_hh += dgh^T g^(j-1) as MFMA products over the tile's 16 rows into per-workgroup
// register accumulators (wave w: the 12 gate tiles of its 16 columns); dc = dgi W_ih and dgh W_hh with transposed fragments read
// through L2; dg^(j-1) = dg^(j) z + dgh W_hh + (column sum of dc over the group - own dc) / N.  A workgroup writes ONE slab of
// partial weight gradients when its tiles are done; a second kernel adds the slabs in slab order into the destinations
// (marl_wgrad_slabs' idiom): no float atomics, the same bits on every call.
#include "common.h"
#include "../../include/marl_hip.h"

// No implicit contraction in this file: a row's value must not depend on where in a tile it sits, and the compiler may fuse the four
// unrolled instances of a lane's pointwise code differently; the fused operations below are written out.
#pragma clang fp contract(off)
#include "group_tile.h"    // the whole-group tile, the W_hh fragments, the GRU point and its backward (H, LD, G3, LDG)

namespace {

using namespace group_tile;

constexpr int CN_NMAX = 16;
constexpr int CN_AMAX = 32;
constexpr int CN_LDA = CN_AMAX + 4;
constexpr int CN_KMAX = 4;
constexpr int CN_FWD_WG = 512;             // workgroups of the forward (persistent over the tiles)
constexpr int CN_BWD_WG = 256;             // workgroups = slabs of the backward
// one slab: dW_ih | dW_hh | dW_dec (32 rows) | db_ih | db_hh | db_dec
constexpr int CN_S_IH = 0, CN_S_HH = G3 * H, CN_S_DEC = 2 * G3 * H, CN_S_BIH = CN_S_DEC + CN_AMAX * H;
constexpr int CN_S_BHH = CN_S_BIH + G3, CN_S_BDEC = CN_S_BHH + G3, CN_SLAB = CN_S_BDEC + CN_AMAX;

struct CommArgs {
  marl_commnet_weights_t w;
  const float* hs;        // (G, N, 64)
  float* logits;          // (G, N, A)
  const float* dlogits;   // (G, N, A)
  float* dhs;             // (G, N, 64)
  float* slabs;           // gridDim.x x CN_SLAB
  long G, tiles;
  int N, A, K, gpw;       // gpw = 16 / N groups per tile
  float invN;
};

// forward-form B fragments of f_comm for column col = 16 w + m: the W_hh half (group_tile.h) and W_ih in the same form
struct CnW : HH {
  f32x4 ih[3][4];
  float bi[3];
};

__device__ __forceinline__ void cn_load_w(CnW& W, const marl_commnet_weights_t& w, int col, int q) {
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const long row = (long)(g * H + col) * H;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        W.ih[g][c][i] = w.w_ih[row + 16 * c + 4 * q + i];
        W.hh[g][c][i] = w.w_hh[row + 16 * c + 4 * q + i];
      }
    W.bi[g] = w.b_ih[g * H + col];
    W.bh[g] = w.b_hh[g * H + col];
  }
}

// (column sum of X over the rows of element (r, c)'s group - X[r][c]) / N
__device__ __forceinline__ float cn_others(const float* X, int N, float invN, int r, int c) {
  const int r0 = r / N * N;
  float s = 0.0f;
  for (int l = 0; l < N; ++l)
    if (r0 + l < 16) s += X[(r0 + l) * LD + c];
  return (s - X[r * LD + c]) * invN;
}

// C[16][LD] <- the communication input of every row of X
__device__ __forceinline__ void cn_comm(const float* X, float* C, int N, float invN) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = threadIdx.x + 256 * k, r = idx >> 6, c = idx & 63;
    C[r * LD + c] = cn_others(X, N, invN, r, c);
  }
}

// One f_comm cell for this lane's four elements (rows 4 q + r, column col): input C (has_in false: the zero input of round 0), hidden Gp.
// The GRU point runs on the hardware exponential.
__device__ __forceinline__ void cn_cell(const CnW& W, bool has_in, const float* C, const float* Gp, int m, int q, int col, Cell& o) {
  f32x4 ai[3], ah[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) ai[g] = ah[g] = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 x = lds4(Gp, LD, m, 16 * c + 4 * q);
    mfma16x4_il3(x, W.hh[0][c], ah[0], x, W.hh[1][c], ah[1], x, W.hh[2][c], ah[2]);
  }
  if (has_in) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 x = lds4(C, LD, m, 16 * c + 4 * q);
      mfma16x4_il3(x, W.ih[0][c], ai[0], x, W.ih[1][c], ai[1], x, W.ih[2][c], ai[2]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o.hp[r] = Gp[(4 * q + r) * LD + col];
    o.hn[r] = ah[2][r] + W.bh[2];
    gru_point<true>((ai[0][r] + W.bi[0]) + (ah[0][r] + W.bh[0]), (ai[1][r] + W.bi[1]) + (ah[1][r] + W.bh[1]), ai[2][r] + W.bi[2], o.hn[r],
                 o.hp[r], o.r[r], o.z[r], o.n[r], o.h[r]);
  }
}

__global__ __launch_bounds__(256) void commnet_fwd_kernel(CommArgs p) {
  __shared__ __attribute__((aligned(16))) float sh_g[2][16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_c[16 * LD];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, m = l & 15, q = l >> 4, col = 16 * w + m;
  CnW W;
  cn_load_w(W, p.w, col, q);
  // decoding: waves 0 and 1 hold the fragments of action tile w (rows >= A are zeros)
  f32x4 dec[4];
  const int act = 16 * w + m;
  const bool dec_wave = 16 * w < p.A;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) dec[c][i] = (w < 2 && act < p.A) ? p.w.dec_w[(long)act * H + 16 * c + 4 * q + i] : 0.0f;
  const float dec_b = (w < 2 && act < p.A) ? p.w.dec_b[act] : 0.0f;

  for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    load_tile(p.gpw * p.N, p.gpw, p.N, p.G, tile, p.hs, sh_g[0]);
    __syncthreads();
    int cur = 0;
    for (int j = 0; j < p.K; ++j) {
      if (j > 0) {
        cn_comm(sh_g[cur], sh_c, p.N, p.invN);
        __syncthreads();
      }
      Cell o;
      cn_cell(W, j > 0, sh_c, sh_g[cur], m, q, col, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_g[cur ^ 1][(4 * q + r) * LD + col] = o.h[r];
      __syncthreads();
      cur ^= 1;
    }
    if (dec_wave) {
      f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = mfma16x4(lds4(sh_g[cur], LD, m, 16 * c + 4 * q), dec[c], acc);
      if (act < p.A) {
        const long row0 = tile * p.gpw * p.N;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (row_ok(p.gpw * p.N, p.gpw, p.N, p.G, tile, 4 * q + r)) p.logits[(row0 + 4 * q + r) * p.A + act] = acc[r] + dec_b;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void commnet_bwd_kernel(CommArgs p) {
  __shared__ __attribute__((aligned(16))) float sh_gs[CN_KMAX + 1][16 * LD];    // g^(-1) = h, g^(0) .. g^(K-1)
  __shared__ __attribute__((aligned(16))) float sh_c[16 * LD], sh_dg[16 * LD], sh_dc[16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_dgi[16 * LDG], sh_dgh[16 * LDG];
  __shared__ __attribute__((aligned(16))) float sh_dl[16 * CN_LDA];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, m = l & 15, q = l >> 4, col = 16 * w + m;
  const int A = p.A, K = p.K;
  CnW W;
  cn_load_w(W, p.w, col, q);
  // transposed fragment of the decoding weight: [chunk][i] = W_dec[16 chunk + 4 q + i][col] (f_comm's: group_tile's wt, through L2)
  f32x4 tdec[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = 16 * c + 4 * q + i;
      tdec[c][i] = a < A ? p.w.dec_w[(long)a * H + col] : 0.0f;
    }
  // this workgroup's partial weight gradients: tile t of a matrix = gate rows 16 t + 4 q + r, column col
  f32x4 gih[12], ghh[12], gdec[2];
#pragma unroll
  for (int t = 0; t < 12; ++t) gih[t] = ghh[t] = f32x4{0, 0, 0, 0};
  gdec[0] = gdec[1] = f32x4{0, 0, 0, 0};
  float gbih = 0.0f, gbhh = 0.0f, gbdec = 0.0f;    // thread tid < 192: gate row tid; tid < 32: action tid

  for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long row0 = tile * p.gpw * p.N;
    load_tile(p.gpw * p.N, p.gpw, p.N, p.G, tile, p.hs, sh_gs[0]);
    for (int idx = tid; idx < 16 * CN_AMAX; idx += 256) {
      const int r = idx >> 5, a = idx & 31;
      sh_dl[r * CN_LDA + a] = (a < A && row_ok(p.gpw * p.N, p.gpw, p.N, p.G, tile, r)) ? p.dlogits[(row0 + r) * A + a] : 0.0f;
    }
    __syncthreads();
    // ---- the forward planes
    for (int j = 0; j < K; ++j) {
      if (j > 0) {
        cn_comm(sh_gs[j], sh_c, p.N, p.invN);
        __syncthreads();
      }
      Cell o;
      cn_cell(W, j > 0, sh_c, sh_gs[j], m, q, col, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_gs[j + 1][(4 * q + r) * LD + col] = o.h[r];
      __syncthreads();
    }
    // ---- decoding: dg^(K-1) = dlogits W_dec, dW_dec += dlogits^T g^(K-1), db_dec += column sums
    {
      f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 2; ++c) acc = mfma16x4(lds4(sh_dl, CN_LDA, m, 16 * c + 4 * q), tdec[c], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_dg[(4 * q + r) * LD + col] = acc[r];
      f32x4 b;
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = sh_gs[K][(4 * q + i) * LD + col];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = sh_dl[(4 * q + i) * CN_LDA + 16 * t + m];
        gdec[t] = mfma16x4(a, b, gdec[t]);
      }
      if (tid < CN_AMAX)
        for (int r = 0; r < 16; ++r) gbdec += sh_dl[r * CN_LDA + tid];
    }
    __syncthreads();
    // ---- the rounds in reverse
    for (int j = K - 1; j >= 0; --j) {
      const float* gp = sh_gs[j];
      if (j > 0) {
        cn_comm(gp, sh_c, p.N, p.invN);
        __syncthreads();
      }
      Cell o;
      cn_cell(W, j > 0, sh_c, gp, m, q, col, o);
      float direct[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q + r;
        const GateGrad g = gru_point_bwd(o, r, sh_dg[row * LD + col]);
        direct[r] = g.direct;
        sh_dgi[row * LDG + col] = g.dr;
        sh_dgi[row * LDG + H + col] = g.dz;
        sh_dgi[row * LDG + 2 * H + col] = g.dn;
        sh_dgh[row * LDG + col] = g.dr;
        sh_dgh[row * LDG + H + col] = g.dz;
        sh_dgh[row * LDG + 2 * H + col] = g.dn * o.r[r];
      }
      __syncthreads();
      // weight gradients over the tile's 16 rows (k = row): A = dgi^T / dgh^T, B = c / g^(j-1)
      {
        f32x4 bc, bg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bc[i] = j > 0 ? sh_c[(4 * q + i) * LD + col] : 0.0f;
          bg[i] = gp[(4 * q + i) * LD + col];
        }
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          f32x4 ai, ah;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            ai[i] = sh_dgi[(4 * q + i) * LDG + 16 * t + m];
            ah[i] = sh_dgh[(4 * q + i) * LDG + 16 * t + m];
          }
          mfma16x4_il2(ai, bc, gih[t], ah, bg, ghh[t]);
        }
        if (tid < G3)
          for (int r = 0; r < 16; ++r) {
            gbih += sh_dgi[r * LDG + tid];
            gbhh += sh_dgh[r * LDG + tid];
          }
      }
      // dgh W_hh (and dc = dgi W_ih when the round has an input)
      f32x4 ahh = f32x4{0, 0, 0, 0}, aih = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 12; ++c) ahh = mfma16x4(lds4(sh_dgh, LDG, m, 16 * c + 4 * q), wt(p.w.w_hh, H, c, q, col), ahh);
      if (j > 0) {
#pragma unroll
        for (int c = 0; c < 12; ++c) aih = mfma16x4(lds4(sh_dgi, LDG, m, 16 * c + 4 * q), wt(p.w.w_ih, H, c, q, col), aih);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sh_dg[(4 * q + r) * LD + col] = direct[r] + ahh[r];
          sh_dc[(4 * q + r) * LD + col] = aih[r];
        }
        __syncthreads();
        // every other agent of the group receives dc / N
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int idx = tid + 256 * k, r = idx >> 6, c = idx & 63;
          sh_dg[r * LD + c] += cn_others(sh_dc, p.N, p.invN, r, c);
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (row_ok(p.gpw * p.N, p.gpw, p.N, p.G, tile, 4 * q + r)) p.dhs[(row0 + 4 * q + r) * H + col] = direct[r] + ahh[r];
        __syncthreads();
      }
    }
  }
  // ---- this workgroup's slab
  float* s = p.slabs + (long)blockIdx.x * CN_SLAB;
#pragma unroll
  for (int t = 0; t < 12; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[CN_S_IH + (16 * t + 4 * q + r) * H + col] = gih[t][r];
      s[CN_S_HH + (16 * t + 4 * q + r) * H + col] = ghh[t][r];
    }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[CN_S_DEC + (16 * t + 4 * q + r) * H + col] = gdec[t][r];
  if (tid < G3) {
    s[CN_S_BIH + tid] = gbih;
    s[CN_S_BHH + tid] = gbhh;
  }
  if (tid < CN_AMAX) s[CN_S_BDEC + tid] = gbdec;
}

// destination += the slabs' sum, slab 0 first
__global__ __launch_bounds__(256) void commnet_slab_reduce_kernel(const float* __restrict__ slabs, int n, marl_commnet_grads_t g, int A) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= CN_SLAB) return;
  float* dst;
  if (e < CN_S_HH) dst = g.w_ih + e;
  else if (e < CN_S_DEC) dst = g.w_hh + (e - CN_S_HH);
  else if (e < CN_S_BIH) dst = (e - CN_S_DEC) < A * H ? g.dec_w + (e - CN_S_DEC) : nullptr;
  else if (e < CN_S_BHH) dst = g.b_ih + (e - CN_S_BIH);
  else if (e < CN_S_BDEC) dst = g.b_hh + (e - CN_S_BHH);
  else dst = (e - CN_S_BDEC) < A ? g.dec_b + (e - CN_S_BDEC) : nullptr;
  if (!dst) return;
  *dst += slab_sum(slabs + e, CN_SLAB, 0, 1, n);
}

// ---- the encoder's sigmoid: e = sigmoid(x) in place; dxp = de e (1 - e).  float4 over the 16-byte aligned middle, single floats
// in front of it and behind it: a view that starts 4 bytes later computes the same value for every element.
__device__ __forceinline__ float cn_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

__global__ __launch_bounds__(256) void commnet_sigmoid_fwd_kernel(float* x, long n, int head) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long nv = (n - head) / 4;
  if (i < nv) {
    float4* v = reinterpret_cast<float4*>(x + head) + i;
    float4 a = *v;
    a.x = cn_sigmoid(a.x); a.y = cn_sigmoid(a.y); a.z = cn_sigmoid(a.z); a.w = cn_sigmoid(a.w);
    *v = a;
  }
  if (i < head) x[i] = cn_sigmoid(x[i]);
  const long tail = head + 4 * nv + i;
  if (i < 4 && tail < n) x[tail] = cn_sigmoid(x[tail]);
}

__global__ __launch_bounds__(256) void commnet_sigmoid_bwd_kernel(const float* de, const float* e, float* dxp, long n, int head) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long nv = (n - head) / 4;
  if (i < nv) {
    const float4 d = reinterpret_cast<const float4*>(de + head)[i], s = reinterpret_cast<const float4*>(e + head)[i];
    float4 o;
    o.x = d.x * s.x * (1.0f - s.x); o.y = d.y * s.y * (1.0f - s.y); o.z = d.z * s.z * (1.0f - s.z); o.w = d.w * s.w * (1.0f - s.w);
    reinterpret_cast<float4*>(dxp + head)[i] = o;
  }
  if (i < head) dxp[i] = de[i] * e[i] * (1.0f - e[i]);
  const long tail = head + 4 * nv + i;
  if (i < 4 && tail < n) dxp[tail] = de[tail] * e[tail] * (1.0f - e[tail]);
}

// elementwise, any alignment: the operands of the backward do not share one
__global__ __launch_bounds__(256) void commnet_sigmoid_bwd_scalar_kernel(const float* de, const float* e, float* dxp, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dxp[i] = de[i] * e[i] * (1.0f - e[i]);
}

// floats in front of the first 16-byte boundary (pointers are 4-byte aligned)
int cn_head(const void* p, long n) {
  const long h = (long)((16 - ((uintptr_t)p & 15)) & 15) / 4;
  return (int)(h < n ? h : n);
}

bool cn_weights_ok(const marl_commnet_weights_t* w) {
  return w && w->w_ih && w->w_hh && w->b_ih && w->b_hh && w->dec_w && w->dec_b;
}

bool cn_grads_ok(const marl_commnet_grads_t* g) {
  return g && g->w_ih && g->w_hh && g->b_ih && g->b_hh && g->dec_w && g->dec_b;
}

CommArgs cn_args(const marl_commnet_weights_t* w, long G, int N, int A, int K) {
  CommArgs a{};
  a.w = *w;
  a.G = G; a.N = N; a.A = A; a.K = K;
  a.gpw = 16 / N;
  a.tiles = tiles(G, N);
  a.invN = 1.0f / (float)N;
  return a;
}

}  // namespace

extern "C" int marl_commnet_supported(int N, int A, int K) {
  return N >= 1 && N <= CN_NMAX && A >= 1 && A <= CN_AMAX && K >= 1 && K <= CN_KMAX;
}

extern "C" int marl_commnet_groups_per_workgroup(int N) { return (N >= 1 && N <= CN_NMAX) ? 16 / N : 0; }

extern "C" int marl_commnet_head_fwd(const marl_commnet_weights_t* w, const float* hs, float* logits, long G, int N, int A, int K,
                                     void* stream) {
  if (!cn_weights_ok(w) || G < 0 || !marl_commnet_supported(N, A, K)) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (!hs || !logits || G > 0x7fffffffL / 16) return (int)hipErrorInvalidValue;
  CommArgs a = cn_args(w, G, N, A, K);
  a.hs = hs; a.logits = logits;
  const unsigned grid = (unsigned)(a.tiles < CN_FWD_WG ? a.tiles : CN_FWD_WG);
  hipLaunchKernelGGL(commnet_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t marl_commnet_bwd_workspace(long G, int N, int A, int K) {
  if (G <= 0 || !marl_commnet_supported(N, A, K)) return 0;
  const long tiles = group_tile::tiles(G, N);
  return (size_t)(tiles < CN_BWD_WG ? tiles : CN_BWD_WG) * CN_SLAB * sizeof(float);
}

extern "C" int marl_commnet_head_bwd(const marl_commnet_weights_t* w, const marl_commnet_grads_t* g, const float* hs,
                                     const float* dlogits, float* dhs, float* ws, size_t ws_bytes, long G, int N, int A, int K,
                                     void* stream) {
  if (!cn_weights_ok(w) || !cn_grads_ok(g) || G < 0 || !marl_commnet_supported(N, A, K)) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (!hs || !dlogits || !dhs || G > 0x7fffffffL / 16 || !ws || ws_bytes < marl_commnet_bwd_workspace(G, N, A, K))
    return (int)hipErrorInvalidValue;
  CommArgs a = cn_args(w, G, N, A, K);
  a.hs = hs; a.dlogits = dlogits; a.dhs = dhs; a.slabs = ws;
  const int grid = (int)(a.tiles < CN_BWD_WG ? a.tiles : CN_BWD_WG);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(commnet_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(commnet_slab_reduce_kernel, dim3((CN_SLAB + 255) / 256), dim3(256), 0, s, (const float*)ws, grid, *g, A);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_commnet_sigmoid_fwd(float* x, long n, void* stream) {
  if (n < 0 || (n > 0 && !x)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int head = cn_head(x, n);
  const long work = (n - head) / 4 > 4 ? (n - head) / 4 : 4;
  const long blocks = (work + 255) / 256;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(commnet_sigmoid_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, head);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_commnet_sigmoid_bwd(const float* de, const float* e, float* dxp, long n, void* stream) {
  if (n < 0 || (n > 0 && (!de || !e || !dxp))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const bool same = ((uintptr_t)de & 15) == ((uintptr_t)dxp & 15) && ((uintptr_t)e & 15) == ((uintptr_t)dxp & 15);
  if (!same) {
    const long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(commnet_sigmoid_bwd_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, s, de, e, dxp, n);
    MARL_CHECK_LAUNCH();
    return 0;
  }
  const int head = cn_head(dxp, n);
  const long work = (n - head) / 4 > 4 ? (n - head) / 4 : 4;
  const long blocks = (work + 255) / 256;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(commnet_sigmoid_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, de, e, dxp, n, head);
  MARL_CHECK_LAUNCH();
  return 0;
}
