// What the group heads (commnet.hip, g2anet.hip) share: 256 threads = four waves walk 16-row tiles that hold 16 / N WHOLE groups of
// N agent rows (rows 0 .. (16 / N) N - 1; the rest of the tile is zero rows that are never written), so a group's other rows are rows
// of the same LDS tile.  Wave w owns the hidden columns 16 w .. 16 w + 15 of all three gates of a GRUCell(., 64); lane l = 16 q + m
// supplies row m of the A operand and column col = 16 w + m of the B operand of v_mfma_f32_16x16x4_f32 (the K-permutation of
// common.h: step i of a 16-chunk takes k = 4 q + i) and holds rows 4 q + r (r = 0 .. 3), column col of the result.
#pragma once
#include "common.h"

// No implicit contraction (as the two files): a row's value must not depend on where in a tile it sits; every fused operation below
// is written out.
#pragma clang fp contract(off)

namespace group_tile {

constexpr int H = 64;
constexpr int LD = H + 4;              // row pitch of the 16 x 64 planes: 4 rows apart = 16 banks apart
constexpr int G3 = 3 * H;
constexpr int LDG = G3 + 4;            // row pitch of the 16 x 192 planes

__device__ __forceinline__ f32x4 lds4(const float* X, int ld, int row, int k) {
  return *reinterpret_cast<const f32x4*>(X + row * ld + k);
}

// tiles of G groups at gpw = 16 / N groups per tile
inline long tiles(long G, int N) {
  const int gpw = 16 / N;
  return (G + gpw - 1) / gpw;
}

// row r of tile t is global row t nrows + r (nrows = gpw N), valid while it belongs to a whole group < G
__device__ __forceinline__ bool row_ok(int nrows, int gpw, int N, long G, long tile, int r) {
  return r < nrows && tile * gpw + r / N < G;
}

// dst[16][LD] <- the tile's rows of src (rows of 64 floats), zeros on the rows that are not valid
__device__ __forceinline__ void load_tile(int nrows, int gpw, int N, long G, long tile, const float* src, float* dst) {
  const long row0 = tile * nrows;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = threadIdx.x + 256 * k, r = idx >> 6, c = idx & 63;
    dst[r * LD + c] = row_ok(nrows, gpw, N, G, tile, r) ? src[(row0 + r) * H + c] : 0.0f;
  }
}

// transposed B fragment of a row-major weight with row pitch ld, read through L2: [i] = W[16 chunk + 4 q + i][col].  The index is
// formed in 32 bits: rows x ld must stay under 2^31 (here at most 192 x 128)
__device__ __forceinline__ f32x4 wt(const float* __restrict__ W, int ld, int c, int q, int col) {
  f32x4 b;
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = __ldg(W + (16 * c + 4 * q + i) * ld + col);
  return b;
}

// forward-form B fragments of a (192, 64) W_hh for column col: [gate][chunk][i] = W[gate * 64 + col][16 chunk + 4 q + i]
struct HH {
  f32x4 hh[3][4];
  float bh[3];
};

__device__ __forceinline__ void load_hh(HH& W, const float* __restrict__ w_hh, const float* __restrict__ b_hh, int col, int q) {
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const long row = (long)(g * H + col) * H;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) W.hh[g][c][i] = w_hh[row + 16 * c + 4 * q + i];
    W.bh[g] = b_hh[g * H + col];
  }
}

// one GRU cell for this lane's four elements (rows 4 q + r, column col), the gates as torch's GRUCell names them; hn is the hidden
// side of the candidate, bias included, hp the previous state
struct Cell { float r[4], z[4], n[4], hn[4], hp[4], h[4]; };

// torch's GRUCell point: r, z = sigmoid, n = tanh(in + r hn), h = (1 - z) n + z hp = n + z (hp - n); every fused operation explicit.
// HW_EXP: the hardware exponential behind __expf, otherwise expf
template <bool HW_EXP>
__device__ __forceinline__ void gru_point(float ar, float az, float ain, float ahn, float hp, float& r, float& z, float& n, float& h) {
  r = __builtin_amdgcn_rcpf(1.0f + (HW_EXP ? __expf(-ar) : expf(-ar)));
  z = __builtin_amdgcn_rcpf(1.0f + (HW_EXP ? __expf(-az) : expf(-az)));
  const float x = 2.0f * __builtin_fmaf(r, ahn, ain);
  const float e = HW_EXP ? __expf(x) : expf(x);
  n = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  h = __builtin_fmaf(z, hp - n, n);
}

// the pointwise GRU backward of element r of a cell for the gradient dh on its new state: the gate gradients dr | dz | dn and
// direct = dh z, the part of dh that reaches the previous state past the gates.  The hidden side's dn r is taken where it is stored:
// formed here it moved a multiply ahead of three LDS stores in g2anet_hard_bwd_kernel (a wider s_waitcnt, 0.2 % on the backward)
struct GateGrad { float dr, dz, dn, direct; };

__device__ __forceinline__ GateGrad gru_point_bwd(const Cell& o, int r, float dh) {
  GateGrad g;
  g.dn = dh * (1.0f - o.z[r]) * (1.0f - o.n[r] * o.n[r]);
  g.dz = dh * (o.hp[r] - o.n[r]) * o.z[r] * (1.0f - o.z[r]);
  g.dr = g.dn * o.hn[r] * o.r[r] * (1.0f - o.r[r]);
  g.direct = dh * o.z[r];
  return g;
}

}  // namespace group_tile
