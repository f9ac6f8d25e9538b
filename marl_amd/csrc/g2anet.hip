// G2ANet attention head on gfx950 (the project's own definition, include/marl_hip.h): over the hidden states of ONE environment-step
// (a group of N agent rows), with the partners of agent i in agent order j_0 < .. < j_{N-2}, all j != i:
//   hard:  f_{i,p} = GRU_fwd([h_i | h_{j_p}], f_{i,p-1}),  b_{i,p} = GRU_rev([h_i | h_{j_p}], b_{i,p+1}),  zero initial states
//          y = hard_encoding([f | b]),  w_{i,p} = sigmoid((y_1 - y_0 + l_{i,p}) / tau)          (w = 1 with hard off)
//   soft:  a_{i,.} = softmax_p(q_i . k_{j_p} / sqrt(32)),  x_i = sum_p a_{i,p} w_{i,p} relu(v(h_{j_p}))
//   logits_i = decoding([h_i | x_i])
// The (N-1) x 128 input of the bidirectional GRU is never built: W_ih [h_i | h_j] = W_ih[:, :64] h_i + W_ih[:, 64:] h_j, so per
// direction a row's P = W_ih[:, :64] h + b_ih and Q = W_ih[:, 64:] h are computed once and position p takes P_i + Q_{j_p}.
//
// All kernels: 256 threads = four waves; a workgroup walks 16-row tiles in a grid-stride loop; a tile holds 16 / N WHOLE groups (the
// rest of the tile is zero rows that are never written), so a partner's row is a row of the same LDS tile.  Wave w owns the hidden
// columns 16 w .. 16 w + 15 of all three gates; lane l = 16 q + m supplies row m of the A operand and column 16 w + m of the B
// operand of v_mfma_f32_16x16x4_f32 (the K-permutation of common.h) and holds rows 4 q + r, column 16 w + m of the result.  The
// W_hh fragments stay in registers across the positions and the tiles; the W_ih fragments are read through L2 once per tile.
//
// Forward: P / Q planes of both directions in LDS, the two chains interleaved (step s: position s forward, N - 2 - s in reverse), each
// state's dot product with hard_encoding's row difference taken as soon as it exists - only y_1 - y_0 matters.
//
// Backward (everything recomputed from hs and the noise): the forward kernel once more for the plane w (G, N, N-1); the soft kernel
// (decoding, attention, q / k / v: dhs is written, w is replaced by ds = d(y_1 - y_0)); one hard kernel per direction (the chain's states
// into LDS planes, then the chain in reverse; dP summed in registers, dQ by a fixed-order LDS pass; dhs += dP W_ih[:, :64] +
// dQ W_ih[:, 64:]).  Weight gradients: register accumulators per workgroup, ONE slab per workgroup and kernel, added in slab order
// by a reduce kernel (marl_wgrad_slabs' idiom): no float atomics, the same bits on every call.
#include "common.h"
#include "synth_env.h"
#include "../../include/marl_hip.h"

// No implicit contraction in this file (as commnet.hip): a row's value must not depend on where in a tile it sits.
#pragma clang fp contract(off)
#include "group_tile.h"    // the whole-group tile, the W_hh fragments, the GRU point and its backward (H, LD, G3, LDG: P, Q, dQ)

namespace {

using namespace group_tile;

constexpr int GA_D = 32;                   // attention_dim
constexpr int GA_LDG4 = 4 * H + 4;      // the gate-gradient plane: dr | dz | dn | dn r
constexpr int GA_LDQ = 3 * GA_D + 4;       // q | k | v
constexpr int GA_LDD = GA_D + 4;           // x, dx, dlogits
constexpr int GA_NMIN = 2, GA_NMAX = 10, GA_PMAX = GA_NMAX - 1, GA_AMAX = 32;
constexpr int GA_FWD_WG = 512;             // workgroups of the forward (persistent over the tiles)
constexpr int GA_BWD_WG = 256;             // workgroups = slabs of a backward kernel
// the soft kernel's slab: dW_dec[:, :64] (32 rows) | dW_dec[:, 64:] | dW_q | dW_k | dW_v | db_dec | db_v | sum of ds
constexpr int GA_S2_DH = 0, GA_S2_DX = GA_AMAX * H, GA_S2_Q = GA_S2_DX + GA_AMAX * GA_D, GA_S2_BD = GA_S2_Q + 3 * GA_D * H;
constexpr int GA_S2_BV = GA_S2_BD + GA_AMAX, GA_S2_HE = GA_S2_BV + GA_D, GA_SLAB2 = GA_S2_HE + 1;
// a hard kernel's slab: dW_ih (192, 128) | dW_hh (192, 64) | db_ih | db_hh | four row-quarter partials of sum ds state (4 x 64)
constexpr int GA_S3_IH = 0, GA_S3_HH = G3 * 2 * H, GA_S3_BIH = GA_S3_HH + G3 * H, GA_S3_BHH = GA_S3_BIH + G3;
constexpr int GA_S3_HE = GA_S3_BHH + G3, GA_SLAB3 = GA_S3_HE + 4 * H;
constexpr int GA_SLAB = GA_SLAB3 > GA_SLAB2 ? GA_SLAB3 : GA_SLAB2;

struct GaArgs {
  marl_g2anet_weights_t w;
  const float* hs;        // (G, N, 64)
  const float* noise;     // (G, N, N-1) or null
  float* logits;          // (G, N, A); null: the forward kernel stops at w
  float* wplane;          // (G, N, N-1): w out of the forward kernel, w in / ds out of the soft kernel, ds into the hard kernels
  const float* dlogits;   // (G, N, A)
  float* dhs;             // (G, N, 64)
  float* slabs;           // gridDim.x x GA_SLAB2 / GA_SLAB3
  long G, tiles;
  int N, A, gpw, nrows;   // gpw = 16 / N groups per tile, nrows = gpw N
  int hard, dir;
  float tau;
};

__device__ __forceinline__ const float* ga_w_ih(const marl_g2anet_weights_t& w, int d) { return d ? w.gr_w_ih : w.gf_w_ih; }
__device__ __forceinline__ const float* ga_w_hh(const marl_g2anet_weights_t& w, int d) { return d ? w.gr_w_hh : w.gf_w_hh; }
__device__ __forceinline__ const float* ga_b_ih(const marl_g2anet_weights_t& w, int d) { return d ? w.gr_b_ih : w.gf_b_ih; }
__device__ __forceinline__ const float* ga_b_hh(const marl_g2anet_weights_t& w, int d) { return d ? w.gr_b_hh : w.gf_b_hh; }

// the tile row of partner p of tile row `row` (a row outside the tile's whole groups: itself - its values are never written)
__device__ __forceinline__ int ga_partner(int row, int p, int N, int nrows) {
  if (row >= nrows) return row;
  const int a = row % N;
  return row - a + (p < a ? p : p + 1);
}

// the position at which row `i` (agent ai) meets partner agent aj of its group
__device__ __forceinline__ int ga_pos(int ai, int aj) { return aj < ai ? aj : aj - 1; }

// P[16][LDG] = h W_ih[:, :64]^T + b_ih and Q = h W_ih[:, 64:]^T of one direction (W_ih (192, 128), fragments through L2)
__device__ __forceinline__ void ga_pq(const float* __restrict__ w_ih, const float* __restrict__ b_ih, const float* sh_h, float* P, float* Q,
                                      int m, int q, int col) {
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    f32x4 ap = f32x4{0, 0, 0, 0}, aq = f32x4{0, 0, 0, 0};
    const float* wr = w_ih + (long)(g * H + col) * (2 * H);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 x = lds4(sh_h, LD, m, 16 * c + 4 * q);
      f32x4 bp, bq;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bp[i] = __ldg(wr + 16 * c + 4 * q + i);
        bq[i] = __ldg(wr + H + 16 * c + 4 * q + i);
      }
      mfma16x4_il2(x, bp, ap, x, bq, aq);
    }
    const float b = b_ih[g * H + col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P[(4 * q + r) * LDG + g * H + col] = ap[r] + b;
      Q[(4 * q + r) * LDG + g * H + col] = aq[r];
    }
  }
}

// One chain step at position p for this lane's four elements (rows 4 q + r, column col): input side P_row + Q_partner, hidden `prev`
// (has_prev false: the zero state, no product).  The GRU point runs on expf, not the hardware exponential behind __expf: the states'
// error reaches w multiplied by 1 / tau = 100, and with __expf a case with two pairs inside the sigmoid's transition missed the
// float64 bound on hard_encoding.bias (3.8e-5 against 3.3e-5)
__device__ __forceinline__ void ga_cell(const HH& W, const float* P, const float* Q, const float* prev, bool has_prev, int p, int N,
                                        int nrows, int m, int q, int col, Cell& o) {
  f32x4 ah[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) ah[g] = f32x4{0, 0, 0, 0};
  if (has_prev) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 x = lds4(prev, LD, m, 16 * c + 4 * q);
      mfma16x4_il3(x, W.hh[0][c], ah[0], x, W.hh[1][c], ah[1], x, W.hh[2][c], ah[2]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * q + r, jr = ga_partner(row, p, N, nrows);
    const float* Pr = P + row * LDG + col;
    const float* Qr = Q + jr * LDG + col;
    o.hp[r] = has_prev ? prev[row * LD + col] : 0.0f;
    o.hn[r] = ah[2][r] + W.bh[2];
    gru_point<false>((Pr[0] + Qr[0]) + (ah[0][r] + W.bh[0]), (Pr[H] + Qr[H]) + (ah[1][r] + W.bh[1]), Pr[2 * H] + Qr[2 * H],
                 o.hn[r], o.hp[r], o.r[r], o.z[r], o.n[r], o.h[r]);
  }
}

// sum over the 16 lanes of a row (tid >> 4 = row), the same order for every row
__device__ __forceinline__ float ga_row16_sum(float v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

// q | k | relu(v) of the tile's rows into sh_qkv[16][GA_LDQ]: six 16-column tiles, wave w takes tiles w and w + 4
struct GaQKV { f32x4 f[2][4]; float b[2]; };

__device__ __forceinline__ void ga_load_qkv(GaQKV& W, const marl_g2anet_weights_t& w, int wv, int m, int q) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int tt = wv + 4 * s;
    const float* M = tt < 2 ? w.q_w : tt < 4 ? w.k_w : w.v_w;
    const long row = (long)(16 * (tt & 1) + m) * H;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) W.f[s][c][i] = tt < 6 ? M[row + 16 * c + 4 * q + i] : 0.0f;
    W.b[s] = (tt >= 4 && tt < 6) ? w.v_b[16 * (tt & 1) + m] : 0.0f;
  }
}

__device__ __forceinline__ void ga_qkv(const GaQKV& W, const float* sh_h, float* sh_qkv, int wv, int m, int q) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int tt = wv + 4 * s;
    if (tt < 6) {
      f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = mfma16x4(lds4(sh_h, LD, m, 16 * c + 4 * q), W.f[s][c], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[r] + W.b[s];
        sh_qkv[(4 * q + r) * GA_LDQ + 16 * tt + m] = (tt >= 4 && v < 0.0f) ? 0.0f : v;
      }
    }
  }
}

// q_row . k_partner / sqrt(32)
__device__ __forceinline__ float ga_score(const float* sh_qkv, int row, int jr) {
  float s = 0.0f;
#pragma unroll 8
  for (int c = 0; c < GA_D; ++c) s += sh_qkv[row * GA_LDQ + c] * sh_qkv[jr * GA_LDQ + GA_D + c];
  return s * 0.17677669529663687f;
}

// a_{row,pp} of the softmax over the row's N - 1 scores
__device__ __forceinline__ float ga_softmax_at(const float* e, int np, int pp) {
  float mx = e[0];
  for (int k = 1; k < np; ++k) mx = fmaxf(mx, e[k]);
  float sum = 0.0f;
  for (int k = 0; k < np; ++k) sum += __expf(e[k] - mx);
  return __expf(e[pp] - mx) / sum;
}

__global__ __launch_bounds__(256) void g2anet_fwd_kernel(GaArgs p) {
  __shared__ __attribute__((aligned(16))) float sh_h[16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_pq[4][16 * LDG];        // P, Q forward; P, Q reverse
  __shared__ __attribute__((aligned(16))) float sh_st[2][2][16 * LD];      // [direction][buffer]
  __shared__ __attribute__((aligned(16))) float sh_qkv[16 * GA_LDQ];
  __shared__ __attribute__((aligned(16))) float sh_x[16 * GA_LDD];
  __shared__ float sh_s[2][16 * GA_PMAX], sh_e[16 * GA_PMAX], sh_cf[16 * GA_PMAX];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, m = l & 15, q = l >> 4, col = 16 * w + m;
  const int N = p.N, A = p.A, np = N - 1;
  const bool soft = p.logits != nullptr;
  HH Wf, Wb;
  float dvf[4], dvb[4], dbias = 0.0f;
  if (p.hard) {
    load_hh(Wf, p.w.gf_w_hh, p.w.gf_b_hh, col, q);
    load_hh(Wb, p.w.gr_w_hh, p.w.gr_b_hh, col, q);
    // hard_encoding's row difference over this thread's four columns of the dot pass (row tid >> 4, columns 4 (tid & 15) ..)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * (tid & 15) + i;
      dvf[i] = p.w.he_w[2 * H + c] - p.w.he_w[c];
      dvb[i] = p.w.he_w[3 * H + c] - p.w.he_w[H + c];
    }
    dbias = p.w.he_b[1] - p.w.he_b[0];
  }
  GaQKV Wq;
  f32x4 dec[6];
  const int act = 16 * w + m;
  const bool dec_wave = soft && 16 * w < A;
  float dec_b = 0.0f;
  if (soft) {
    ga_load_qkv(Wq, p.w, w, m, q);
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) dec[c][i] = (w < 2 && act < A) ? p.w.dec_w[(long)act * (H + GA_D) + 16 * c + 4 * q + i] : 0.0f;
    dec_b = (w < 2 && act < A) ? p.w.dec_b[act] : 0.0f;
  }

  for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long row0 = tile * p.nrows;
    load_tile(p.nrows, p.gpw, p.N, p.G, tile, p.hs, sh_h);
    __syncthreads();
    if (p.hard) {
      ga_pq(p.w.gf_w_ih, p.w.gf_b_ih, sh_h, sh_pq[0], sh_pq[1], m, q, col);
      ga_pq(p.w.gr_w_ih, p.w.gr_b_ih, sh_h, sh_pq[2], sh_pq[3], m, q, col);
    }
    if (soft) ga_qkv(Wq, sh_h, sh_qkv, w, m, q);
    __syncthreads();
    if (p.hard) {
      int cur = 0;
      for (int s = 0; s < np; ++s) {
        const int pf = s, pb = np - 1 - s;
        Cell o;
        ga_cell(Wf, sh_pq[0], sh_pq[1], sh_st[0][cur], s > 0, pf, N, p.nrows, m, q, col, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh_st[0][cur ^ 1][(4 * q + r) * LD + col] = o.h[r];
        ga_cell(Wb, sh_pq[2], sh_pq[3], sh_st[1][cur], s > 0, pb, N, p.nrows, m, q, col, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh_st[1][cur ^ 1][(4 * q + r) * LD + col] = o.h[r];
        __syncthreads();
        cur ^= 1;
        {
          const int row = tid >> 4, c0 = 4 * (tid & 15);
          float sf = 0.0f, sb = 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sf += dvf[i] * sh_st[0][cur][row * LD + c0 + i];
            sb += dvb[i] * sh_st[1][cur][row * LD + c0 + i];
          }
          sf = ga_row16_sum(sf);
          sb = ga_row16_sum(sb);
          if ((tid & 15) == 0) {
            sh_s[0][row * GA_PMAX + pf] = sf;
            sh_s[1][row * GA_PMAX + pb] = sb;
          }
        }
      }
      __syncthreads();
    }
    // w of every pair (and its score)
    if (tid < 16 * np) {
      const int row = tid / np, pp = tid - row * np;
      const bool ok = row_ok(p.nrows, p.gpw, p.N, p.G, tile, row);
      float wv = 1.0f;
      if (p.hard) {
        const float ln = (p.noise && ok) ? p.noise[(row0 + row) * np + pp] : 0.0f;
        const float y = (sh_s[0][row * GA_PMAX + pp] + sh_s[1][row * GA_PMAX + pp]) + dbias + ln;
        wv = 1.0f / (1.0f + expf(-(y / p.tau)));
        if (p.wplane && ok) p.wplane[(row0 + row) * np + pp] = wv;
      }
      sh_cf[row * GA_PMAX + pp] = wv;
      if (soft) sh_e[row * GA_PMAX + pp] = ga_score(sh_qkv, row, ga_partner(row, pp, N, p.nrows));
    }
    if (soft) {
      __syncthreads();
      if (tid < 16 * np) {      // a w, in the place of the thread's own w
        const int row = tid / np, pp = tid - row * np;
        sh_cf[row * GA_PMAX + pp] *= ga_softmax_at(sh_e + row * GA_PMAX, np, pp);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int idx = tid + 256 * k, row = idx >> 5, c = idx & 31;
        float x = 0.0f;
        for (int pp = 0; pp < np; ++pp)
          x += sh_cf[row * GA_PMAX + pp] * sh_qkv[ga_partner(row, pp, N, p.nrows) * GA_LDQ + 2 * GA_D + c];
        sh_x[row * GA_LDD + c] = x;
      }
      __syncthreads();
      if (dec_wave) {
        f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = mfma16x4(lds4(sh_h, LD, m, 16 * c + 4 * q), dec[c], acc);
#pragma unroll
        for (int c = 0; c < 2; ++c) acc = mfma16x4(lds4(sh_x, GA_LDD, m, 16 * c + 4 * q), dec[4 + c], acc);
        if (act < A) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (row_ok(p.nrows, p.gpw, p.N, p.G, tile, 4 * q + r)) p.logits[(row0 + 4 * q + r) * A + act] = acc[r] + dec_b;
        }
      }
    }
    __syncthreads();
  }
}

// ---- the soft kernel: decoding, attention and q / k / v in reverse.  dhs is WRITTEN; with hard on, the plane's w becomes ds.
__global__ __launch_bounds__(256) void g2anet_soft_bwd_kernel(GaArgs p) {
  __shared__ __attribute__((aligned(16))) float sh_h[16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_qkv[16 * GA_LDQ], sh_dqkv[16 * GA_LDQ];
  __shared__ __attribute__((aligned(16))) float sh_x[16 * GA_LDD], sh_dx[16 * GA_LDD], sh_dl[16 * GA_LDD];
  __shared__ float sh_w[16 * GA_PMAX], sh_e[16 * GA_PMAX], sh_t[16 * GA_PMAX], sh_cf[16 * GA_PMAX], sh_de[16 * GA_PMAX];
  __shared__ float sh_red[256];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, m = l & 15, q = l >> 4, col = 16 * w + m;
  const int N = p.N, A = p.A, np = N - 1, LW = H + GA_D;
  GaQKV Wq;
  ga_load_qkv(Wq, p.w, w, m, q);
  // transposed fragments: decoding's h block and x block ([chunk][i] = W_dec[16 chunk + 4 q + i][col or 64 + 16 w + m]), and
  // [W_q; W_k; W_v] (96, 64): [chunk][i] = W[16 chunk + 4 q + i][col]
  f32x4 tdh[2], tdx[2], tqkv[6];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = 16 * c + 4 * q + i;
      tdh[c][i] = a < A ? p.w.dec_w[(long)a * LW + col] : 0.0f;
      tdx[c][i] = (a < A && w < 2) ? p.w.dec_w[(long)a * LW + H + 16 * w + m] : 0.0f;
    }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const float* M = c < 2 ? p.w.q_w : c < 4 ? p.w.k_w : p.w.v_w;
#pragma unroll
    for (int i = 0; i < 4; ++i) tqkv[c][i] = M[(long)(16 * (c & 1) + 4 * q + i) * H + col];
  }
  // partial weight gradients: rows 16 t + 4 q + r of a matrix, column col (the x block of decoding: column 16 w + m, waves 0 and 1)
  f32x4 gdh[2], gdx[2], gqkv[3][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    gdh[t] = gdx[t] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) gqkv[k][t] = f32x4{0, 0, 0, 0};
  }
  float gbd = 0.0f, gbv = 0.0f, ghe = 0.0f;     // tid < 32: action / v column tid; tid < 16 (N - 1): this pair's ds

  for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long row0 = tile * p.nrows;
    load_tile(p.nrows, p.gpw, p.N, p.G, tile, p.hs, sh_h);
    for (int idx = tid; idx < 16 * GA_AMAX; idx += 256) {
      const int r = idx >> 5, a = idx & 31;
      sh_dl[r * GA_LDD + a] = (a < A && row_ok(p.nrows, p.gpw, p.N, p.G, tile, r)) ? p.dlogits[(row0 + r) * A + a] : 0.0f;
    }
    if (tid < 16 * np) {
      const int row = tid / np, pp = tid - row * np;
      sh_w[row * GA_PMAX + pp] = !p.hard ? 1.0f : row_ok(p.nrows, p.gpw, p.N, p.G, tile, row) ? p.wplane[(row0 + row) * np + pp] : 0.0f;
    }
    __syncthreads();
    ga_qkv(Wq, sh_h, sh_qkv, w, m, q);
    // dx = dlogits W_dec[:, 64:] (waves 0, 1) and the direct part of dh = dlogits W_dec[:, :64]
    f32x4 dh = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 2; ++c) dh = mfma16x4(lds4(sh_dl, GA_LDD, m, 16 * c + 4 * q), tdh[c], dh);
    if (w < 2) {
      f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 2; ++c) acc = mfma16x4(lds4(sh_dl, GA_LDD, m, 16 * c + 4 * q), tdx[c], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_dx[(4 * q + r) * GA_LDD + 16 * w + m] = acc[r];
    }
    __syncthreads();
    if (tid < 16 * np) {
      const int row = tid / np, pp = tid - row * np, jr = ga_partner(row, pp, N, p.nrows);
      sh_e[row * GA_PMAX + pp] = ga_score(sh_qkv, row, jr);
      float t = 0.0f;
#pragma unroll 8
      for (int c = 0; c < GA_D; ++c) t += sh_dx[row * GA_LDD + c] * sh_qkv[jr * GA_LDQ + 2 * GA_D + c];
      sh_t[row * GA_PMAX + pp] = t;
    }
    __syncthreads();
    if (tid < 16 * np) {
      const int row = tid / np, pp = tid - row * np;
      const float* e = sh_e + row * GA_PMAX;
      const float* tt = sh_t + row * GA_PMAX;
      const float* ww = sh_w + row * GA_PMAX;
      float mx = e[0];
      for (int k = 1; k < np; ++k) mx = fmaxf(mx, e[k]);
      float sum = 0.0f, dot = 0.0f;
      for (int k = 0; k < np; ++k) sum += __expf(e[k] - mx);
      for (int k = 0; k < np; ++k) dot += (__expf(e[k] - mx) / sum) * (ww[k] * tt[k]);
      const float a = __expf(e[pp] - mx) / sum, wv = ww[pp];
      sh_cf[row * GA_PMAX + pp] = a * wv;
      sh_de[row * GA_PMAX + pp] = a * (wv * tt[pp] - dot) * 0.17677669529663687f;
      if (p.hard && row_ok(p.nrows, p.gpw, p.N, p.G, tile, row)) {
        const float ds = ((a * tt[pp]) * (wv * (1.0f - wv))) / p.tau;
        p.wplane[(row0 + row) * np + pp] = ds;
        ghe += ds;
      }
    }
    __syncthreads();
    // x, dq of the row; dk and dv of the row as a partner: from every other row of its group, in agent order
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int idx = tid + 256 * k, row = idx >> 5, c = idx & 31;
      float x = 0.0f, dq = 0.0f, dk = 0.0f, dv = 0.0f;
      if (row < p.nrows) {
        const int a = row % N, r0 = row - a;
        for (int pp = 0; pp < np; ++pp) {
          const int jr = r0 + (pp < a ? pp : pp + 1);
          x += sh_cf[row * GA_PMAX + pp] * sh_qkv[jr * GA_LDQ + 2 * GA_D + c];
          dq += sh_de[row * GA_PMAX + pp] * sh_qkv[jr * GA_LDQ + GA_D + c];
        }
        for (int ai = 0; ai < N; ++ai)
          if (ai != a) {
            const int i = r0 + ai, pi = ga_pos(ai, a);
            dk += sh_de[i * GA_PMAX + pi] * sh_qkv[i * GA_LDQ + c];
            dv += sh_cf[i * GA_PMAX + pi] * sh_dx[i * GA_LDD + c];
          }
        if (!(sh_qkv[row * GA_LDQ + 2 * GA_D + c] > 0.0f)) dv = 0.0f;
      }
      sh_x[row * GA_LDD + c] = x;
      sh_dqkv[row * GA_LDQ + c] = dq;
      sh_dqkv[row * GA_LDQ + GA_D + c] = dk;
      sh_dqkv[row * GA_LDQ + 2 * GA_D + c] = dv;
    }
    __syncthreads();
    {
      f32x4 bh, bx;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bh[i] = sh_h[(4 * q + i) * LD + col];
        bx[i] = w < 2 ? sh_x[(4 * q + i) * GA_LDD + 16 * w + m] : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = sh_dl[(4 * q + i) * GA_LDD + 16 * t + m];
        gdh[t] = mfma16x4(a, bh, gdh[t]);
        if (w < 2) gdx[t] = mfma16x4(a, bx, gdx[t]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          f32x4 ak;
#pragma unroll
          for (int i = 0; i < 4; ++i) ak[i] = sh_dqkv[(4 * q + i) * GA_LDQ + GA_D * k + 16 * t + m];
          gqkv[k][t] = mfma16x4(ak, bh, gqkv[k][t]);
        }
      }
      if (tid < GA_AMAX)
        for (int r = 0; r < 16; ++r) {
          gbd += sh_dl[r * GA_LDD + tid];
          gbv += sh_dqkv[r * GA_LDQ + 2 * GA_D + tid];
        }
#pragma unroll
      for (int c = 0; c < 6; ++c) dh = mfma16x4(lds4(sh_dqkv, GA_LDQ, m, 16 * c + 4 * q), tqkv[c], dh);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row_ok(p.nrows, p.gpw, p.N, p.G, tile, 4 * q + r)) p.dhs[(row0 + 4 * q + r) * H + col] = dh[r];
    }
    __syncthreads();
  }
  // ---- this workgroup's slab
  float* s = p.slabs + (long)blockIdx.x * GA_SLAB2;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * q + r;
      s[GA_S2_DH + row * H + col] = gdh[t][r];
      if (w < 2) s[GA_S2_DX + row * GA_D + 16 * w + m] = gdx[t][r];
#pragma unroll
      for (int k = 0; k < 3; ++k) s[GA_S2_Q + (k * GA_D + row) * H + col] = gqkv[k][t][r];
    }
  if (tid < GA_AMAX) {
    s[GA_S2_BD + tid] = gbd;
    s[GA_S2_BV + tid] = gbv;
  }
  sh_red[tid] = ghe;
  __syncthreads();
  if (tid == 0) {
    float v = 0.0f;
    for (int k = 0; k < 16 * GA_PMAX; ++k) v += sh_red[k];
    s[GA_S2_HE] = v;
  }
}

__global__ __launch_bounds__(256) void g2anet_soft_reduce_kernel(const float* __restrict__ slabs, int n, marl_g2anet_grads_t g, int A, int hard) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= GA_SLAB2) return;
  const float v = slab_sum(slabs + e, GA_SLAB2, 0, 1, n);
  const int LW = H + GA_D;
  if (e < GA_S2_DX) {
    const int a = e / H, c = e % H;
    if (a < A) g.dec_w[a * LW + c] += v;
  } else if (e < GA_S2_Q) {
    const int a = (e - GA_S2_DX) / GA_D, c = (e - GA_S2_DX) % GA_D;
    if (a < A) g.dec_w[a * LW + H + c] += v;
  } else if (e < GA_S2_BD) {
    const int k = (e - GA_S2_Q) / (GA_D * H), i = (e - GA_S2_Q) % (GA_D * H);
    float* dst = k == 0 ? g.q_w : k == 1 ? g.k_w : g.v_w;
    dst[i] += v;
  } else if (e < GA_S2_BV) {
    if (e - GA_S2_BD < A) g.dec_b[e - GA_S2_BD] += v;
  } else if (e < GA_S2_HE) {
    g.v_b[e - GA_S2_BV] += v;
  } else if (hard) {
    g.he_b[1] += v;
    g.he_b[0] -= v;
  }
}

// ---- the hard kernel of direction p.dir: chain step s sits at position s (forward) or N - 2 - s (reverse)
__global__ __launch_bounds__(256) void g2anet_hard_bwd_kernel(GaArgs p) {
  __shared__ __attribute__((aligned(16))) float sh_h[16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_P[16 * LDG], sh_Q[16 * LDG], sh_dQ[16 * LDG];
  __shared__ __attribute__((aligned(16))) float sh_st[GA_PMAX][16 * LD];
  __shared__ __attribute__((aligned(16))) float sh_dg[16 * GA_LDG4];          // dr | dz | dn | dn r; at the tile's end dP in the first three
  __shared__ float sh_ds[16 * GA_PMAX];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, m = l & 15, q = l >> 4, col = 16 * w + m;
  const int N = p.N, np = N - 1, d = p.dir;
  const float* w_ih = ga_w_ih(p.w, d);
  const float* w_hh = ga_w_hh(p.w, d);
  HH W;
  load_hh(W, w_hh, ga_b_hh(p.w, d), col, q);
  const float dv = p.w.he_w[2 * H + d * H + col] - p.w.he_w[d * H + col];
  f32x4 gihp[12], gihq[12], ghh[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) gihp[t] = gihq[t] = ghh[t] = f32x4{0, 0, 0, 0};
  float gbih = 0.0f, gbhh = 0.0f, ghe = 0.0f;   // tid < 192: gate row tid; every thread: state column tid & 63 over rows 4 (tid >> 6) ..
  const int hhcol = tid < 2 * H ? tid : tid + H;      // gate row tid of the hidden side in the gate-gradient plane

  for (long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long row0 = tile * p.nrows;
    load_tile(p.nrows, p.gpw, p.N, p.G, tile, p.hs, sh_h);
    if (tid < 16 * np) {
      const int row = tid / np, pp = tid - row * np;
      sh_ds[row * GA_PMAX + pp] = row_ok(p.nrows, p.gpw, p.N, p.G, tile, row) ? p.wplane[(row0 + row) * np + pp] : 0.0f;
    }
    for (int idx = tid; idx < 16 * LDG; idx += 256) sh_dQ[idx] = 0.0f;
    __syncthreads();
    ga_pq(w_ih, ga_b_ih(p.w, d), sh_h, sh_P, sh_Q, m, q, col);
    __syncthreads();
    // ---- the chain's states
    for (int s = 0; s < np; ++s) {
      Cell o;
      ga_cell(W, sh_P, sh_Q, sh_st[s > 0 ? s - 1 : 0], s > 0, d ? np - 1 - s : s, N, p.nrows, m, q, col, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_st[s][(4 * q + r) * LD + col] = o.h[r];
      __syncthreads();
    }
    // ---- hard_encoding's half of this direction: sum of ds state
    {
      const int c = tid & 63, r4 = 4 * (tid >> 6);
      for (int s = 0; s < np; ++s) {
        const int pp = d ? np - 1 - s : s;
#pragma unroll
        for (int r = 0; r < 4; ++r) ghe += sh_ds[(r4 + r) * GA_PMAX + pp] * sh_st[s][(r4 + r) * LD + c];
      }
    }
    // ---- the chain in reverse
    float D[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dP[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) dP[g][r] = 0.0f;
    for (int s = np - 1; s >= 0; --s) {
      const int pp = d ? np - 1 - s : s;
      const float* prev = sh_st[s > 0 ? s - 1 : 0];
      Cell o;
      ga_cell(W, sh_P, sh_Q, prev, s > 0, pp, N, p.nrows, m, q, col, o);
      float direct[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q + r;
        const GateGrad g = gru_point_bwd(o, r, D[r] + sh_ds[row * GA_PMAX + pp] * dv);
        direct[r] = g.direct;
        sh_dg[row * GA_LDG4 + col] = g.dr;
        sh_dg[row * GA_LDG4 + H + col] = g.dz;
        sh_dg[row * GA_LDG4 + 2 * H + col] = g.dn;
        sh_dg[row * GA_LDG4 + 3 * H + col] = g.dn * o.r[r];
        dP[0][r] += g.dr;
        dP[1][r] += g.dz;
        dP[2][r] += g.dn;
      }
      __syncthreads();
      if (tid < G3)
        for (int r = 0; r < 16; ++r) gbhh += sh_dg[r * GA_LDG4 + hhcol];
      // dQ: at position pp agent pp of a group is the partner of the agents behind it, agent pp + 1 of those up to pp
      for (int idx = tid; idx < 16 * G3; idx += 256) {
        const int row = idx / G3, gc = idx - row * G3;
        if (row < p.nrows) {
          const int a = row % N, r0 = row - a;
          float sum = 0.0f;
          if (a == pp) {
            for (int ai = pp + 1; ai < N; ++ai) sum += sh_dg[(r0 + ai) * GA_LDG4 + gc];
            sh_dQ[row * LDG + gc] += sum;
          } else if (a == pp + 1) {
            for (int ai = 0; ai <= pp; ++ai) sum += sh_dg[(r0 + ai) * GA_LDG4 + gc];
            sh_dQ[row * LDG + gc] += sum;
          }
        }
      }
      if (s > 0) {
        // dW_hh += dgh^T state (k = the tile's rows), and the gradient on the previous state = dgh W_hh + dh z
        f32x4 bg;
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = prev[(4 * q + i) * LD + col];
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          f32x4 a;
#pragma unroll
          for (int i = 0; i < 4; ++i) a[i] = sh_dg[(4 * q + i) * GA_LDG4 + 16 * t + m + (t < 8 ? 0 : H)];
          ghh[t] = mfma16x4(a, bg, ghh[t]);
        }
        f32x4 ahh = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 12; ++c)
          ahh = mfma16x4(lds4(sh_dg, GA_LDG4, m, 16 * c + 4 * q + (c < 8 ? 0 : H)), wt(w_hh, H, c, q, col), ahh);
#pragma unroll
        for (int r = 0; r < 4; ++r) D[r] = direct[r] + ahh[r];
      }
      __syncthreads();
    }
    // ---- the input side: dP (summed over the positions) and dQ against h
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) sh_dg[(4 * q + r) * GA_LDG4 + g * H + col] = dP[g][r];
    __syncthreads();
    {
      f32x4 bh;
#pragma unroll
      for (int i = 0; i < 4; ++i) bh[i] = sh_h[(4 * q + i) * LD + col];
#pragma unroll
      for (int t = 0; t < 12; ++t) {
        f32x4 ap, aq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ap[i] = sh_dg[(4 * q + i) * GA_LDG4 + 16 * t + m];
          aq[i] = sh_dQ[(4 * q + i) * LDG + 16 * t + m];
        }
        mfma16x4_il2(ap, bh, gihp[t], aq, bh, gihq[t]);
      }
      if (tid < G3)
        for (int r = 0; r < 16; ++r) gbih += sh_dg[r * GA_LDG4 + tid];
      f32x4 ap = f32x4{0, 0, 0, 0}, aq = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 12; ++c)
        mfma16x4_il2(lds4(sh_dg, GA_LDG4, m, 16 * c + 4 * q), wt(w_ih, 2 * H, c, q, col), ap,
                     lds4(sh_dQ, LDG, m, 16 * c + 4 * q), wt(w_ih + H, 2 * H, c, q, col), aq);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row_ok(p.nrows, p.gpw, p.N, p.G, tile, 4 * q + r)) p.dhs[(row0 + 4 * q + r) * H + col] += ap[r] + aq[r];
    }
    __syncthreads();
  }
  // ---- this workgroup's slab
  float* s = p.slabs + (long)blockIdx.x * GA_SLAB3;
#pragma unroll
  for (int t = 0; t < 12; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * q + r;
      s[GA_S3_IH + row * (2 * H) + col] = gihp[t][r];
      s[GA_S3_IH + row * (2 * H) + H + col] = gihq[t][r];
      s[GA_S3_HH + row * H + col] = ghh[t][r];
    }
  if (tid < G3) {
    s[GA_S3_BIH + tid] = gbih;
    s[GA_S3_BHH + tid] = gbhh;
  }
  s[GA_S3_HE + tid] = ghe;
}

__global__ __launch_bounds__(256) void g2anet_hard_reduce_kernel(const float* __restrict__ slabs, int n, marl_g2anet_grads_t g, int dir) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= GA_S3_HE + H) return;
  if (e >= GA_S3_HE) {
    // hard_encoding.weight (2, 128): row 1 receives the sum, row 0 its negative (dy_1 = - dy_0)
    const int c = e - GA_S3_HE;
    float v = 0.0f;
    for (int k = 0; k < 4; ++k) v = slab_acc(v, slabs + GA_S3_HE + k * H + c, GA_SLAB3, 0, 1, n);
    g.he_w[2 * H + dir * H + c] += v;
    g.he_w[dir * H + c] -= v;
    return;
  }
  float* dst;
  if (e < GA_S3_HH) dst = (dir ? g.gr_w_ih : g.gf_w_ih) + e;
  else if (e < GA_S3_BIH) dst = (dir ? g.gr_w_hh : g.gf_w_hh) + (e - GA_S3_HH);
  else if (e < GA_S3_BHH) dst = (dir ? g.gr_b_ih : g.gf_b_ih) + (e - GA_S3_BIH);
  else dst = (dir ? g.gr_b_hh : g.gf_b_hh) + (e - GA_S3_BHH);
  *dst += slab_sum(slabs + e, GA_SLAB3, 0, 1, n);
}

// l = ln(u) - ln(1 - u), u = (k + 0.5) / 2^24 for the 24-bit draw k: ln(2 k + 1) - ln(2^25 - 1 - 2 k), both arguments exact integers
__global__ __launch_bounds__(256) void g2anet_noise_kernel(unsigned seed, int env0, unsigned tg0, float* noise, long total, int T, int N) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int per = N * (N - 1);
  const long et = idx / per;
  const unsigned i = (unsigned)(idx - et * per);
  const int e = (int)(et / T), t = (int)(et - (long)e * T);
  const unsigned k = hkey(seed, ST_GUMBEL, (unsigned)(env0 + e), tg0 + (unsigned)t, i) >> 8;
  noise[idx] = (float)(log((double)(2u * k + 1u)) - log((double)(33554431u - 2u * k)));
}

bool ga_weights_ok(const marl_g2anet_weights_t* w) {
  return w && w->gf_w_ih && w->gf_w_hh && w->gf_b_ih && w->gf_b_hh && w->gr_w_ih && w->gr_w_hh && w->gr_b_ih && w->gr_b_hh && w->he_w &&
         w->he_b && w->q_w && w->k_w && w->v_w && w->v_b && w->dec_w && w->dec_b;
}

bool ga_grads_ok(const marl_g2anet_grads_t* g) {
  return g && g->gf_w_ih && g->gf_w_hh && g->gf_b_ih && g->gf_b_hh && g->gr_w_ih && g->gr_w_hh && g->gr_b_ih && g->gr_b_hh && g->he_w &&
         g->he_b && g->q_w && g->k_w && g->v_w && g->v_b && g->dec_w && g->dec_b;
}

// floats of the plane w / ds in front of the slabs, rounded up to 64
long ga_plane_floats(long G, int N) { return (G * N * (N - 1) + 63) / 64 * 64; }

GaArgs ga_args(const marl_g2anet_weights_t* w, long G, int N, int A, int hard, float tau) {
  GaArgs a{};
  a.w = *w;
  a.G = G; a.N = N; a.A = A; a.hard = hard ? 1 : 0; a.tau = tau;
  a.gpw = 16 / N;
  a.nrows = a.gpw * N;
  a.tiles = tiles(G, N);
  return a;
}

}  // namespace

extern "C" int marl_g2anet_supported(int N, int A, int hard) {
  return N >= GA_NMIN && N <= GA_NMAX && A >= 1 && A <= GA_AMAX && (hard == 0 || hard == 1);
}

extern "C" int marl_g2anet_groups_per_workgroup(int N) { return (N >= GA_NMIN && N <= GA_NMAX) ? 16 / N : 0; }

extern "C" int marl_g2anet_head_fwd(const marl_g2anet_weights_t* w, const float* hs, const float* noise, float* logits, long G, int N,
                                    int A, int hard, float tau, void* stream) {
  if (!ga_weights_ok(w) || G < 0 || !marl_g2anet_supported(N, A, hard) || (hard && !(tau > 0.0f))) return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (!hs || !logits || G > 0x7fffffffL / 16) return (int)hipErrorInvalidValue;
  GaArgs a = ga_args(w, G, N, A, hard, tau);
  a.hs = hs; a.noise = noise; a.logits = logits;
  const unsigned grid = (unsigned)(a.tiles < GA_FWD_WG ? a.tiles : GA_FWD_WG);
  hipLaunchKernelGGL(g2anet_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t marl_g2anet_bwd_workspace(long G, int N, int A, int hard) {
  if (G <= 0 || !marl_g2anet_supported(N, A, hard)) return 0;
  const long tiles = group_tile::tiles(G, N);
  return (size_t)(ga_plane_floats(G, N) + (tiles < GA_BWD_WG ? tiles : GA_BWD_WG) * (long)GA_SLAB) * sizeof(float);
}

extern "C" int marl_g2anet_head_bwd(const marl_g2anet_weights_t* w, const marl_g2anet_grads_t* g, const float* hs, const float* noise,
                                    const float* dlogits, float* dhs, float* ws, size_t ws_bytes, long G, int N, int A, int hard,
                                    float tau, void* stream) {
  if (!ga_weights_ok(w) || !ga_grads_ok(g) || G < 0 || !marl_g2anet_supported(N, A, hard) || (hard && !(tau > 0.0f)))
    return (int)hipErrorInvalidValue;
  if (G == 0) return 0;
  if (!hs || !dlogits || !dhs || G > 0x7fffffffL / 16 || !ws || ws_bytes < marl_g2anet_bwd_workspace(G, N, A, hard))
    return (int)hipErrorInvalidValue;
  GaArgs a = ga_args(w, G, N, A, hard, tau);
  a.hs = hs; a.noise = noise; a.dlogits = dlogits; a.dhs = dhs;
  a.wplane = ws;
  a.slabs = ws + ga_plane_floats(G, N);
  const int grid = (int)(a.tiles < GA_BWD_WG ? a.tiles : GA_BWD_WG);
  hipStream_t s = (hipStream_t)stream;
  if (hard) {      // the plane w: the forward kernel, stopped in front of the soft part
    const unsigned fgrid = (unsigned)(a.tiles < GA_FWD_WG ? a.tiles : GA_FWD_WG);
    hipLaunchKernelGGL(g2anet_fwd_kernel, dim3(fgrid), dim3(256), 0, s, a);
    MARL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(g2anet_soft_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(g2anet_soft_reduce_kernel, dim3((GA_SLAB2 + 255) / 256), dim3(256), 0, s, (const float*)a.slabs, grid, *g, A, a.hard);
  MARL_CHECK_LAUNCH();
  for (int d = 0; hard && d < 2; ++d) {
    a.dir = d;
    hipLaunchKernelGGL(g2anet_hard_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
    MARL_CHECK_LAUNCH();
    hipLaunchKernelGGL(g2anet_hard_reduce_kernel, dim3((GA_S3_HE + H + 255) / 256), dim3(256), 0, s, (const float*)a.slabs, grid, *g, d);
    MARL_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int marl_g2anet_noise(unsigned seed, int env0, unsigned tg0, float* noise, int E, int T, int N, void* stream) {
  if (E < 0 || T < 0 || N < GA_NMIN || N > GA_NMAX) return (int)hipErrorInvalidValue;
  const long total = (long)E * T * N * (N - 1);
  if (total == 0) return 0;
  if (!noise) return (int)hipErrorInvalidValue;
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(g2anet_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, seed, env0, tg0, noise, total, T, N);
  MARL_CHECK_LAUNCH();
  return 0;
}
