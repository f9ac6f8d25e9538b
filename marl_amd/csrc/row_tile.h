// What the row-staging select and loss kernels (mixers.hip: q_masked_max / q_double_select, policy.hip, coma.hip, iql.hip) share.
// Rows are A consecutive floats (44 bytes at A = 11): one lane per row against global memory wastes most of every 64-byte request.
// So a wave owns a tile of ROWS consecutive rows, copies each row operand into LDS as it lies - one contiguous run of ROWS * A
// floats, 16 bytes per lane where the bases allow (r0 * A * 4 is a multiple of 16, the host checks the bases), a scalar tail after -
// and every lane then walks its own row there (lane stride A dwords: conflict-free for odd A, two-way for A = 14 or 18).  Where the
// kernel writes rows, the tile is stored back the same way.  A tile is private to its wave: the wave waits on its own LDS traffic
// only, there is no workgroup barrier.  Action counts whose tiles pass the launcher's LDS cap run a row-per-lane twin on global
// pointers; the row code is one function called by both, so the twin does the same arithmetic in the same order.
#pragma once
#include <initializer_list>
#include "sums.h"

namespace row_tile {

constexpr int ROWS = 64;               // rows per wave tile (one lane per row)
constexpr int WAVES = SUMS_TPB / 64;   // waves, and so tiles in flight, per workgroup: the loss kernels launch sums.h's 256 threads
static_assert(WAVES == 4, "the LDS caps of the launchers are worked out for four waves");
constexpr int PARTIAL_ROWS = 1024;     // the loss workspace (marl_loss_workspace) holds 1024 rows of four partials: the grid cap of
                                       // every kernel that ends in block_partials; one pass of a tiled one covers 262 144 rows

__host__ __device__ inline int tile_floats(int A) { return (ROWS * A + 3) & ~3; }      // pitch of an operand tile: 16-byte multiple
__host__ __device__ inline long tiles(long rows) { return (rows + ROWS - 1) / ROWS; }

// this wave's k operand tiles (tile j at + j * tile_floats(A)) in the workgroup's dynamic LDS
__device__ __forceinline__ float* wave_tiles(float* smem, int k, int A) { return smem + (size_t)(threadIdx.x >> 6) * k * tile_floats(A); }
// tile loop of a wave:  for (long tile = first_tile(); tile < tiles(rows); tile += tile_step())  { r0 = tile * ROWS; .. }
__device__ __forceinline__ long first_tile() { return (long)blockIdx.x * WAVES + (threadIdx.x >> 6); }
__device__ __forceinline__ long tile_step() { return (long)gridDim.x * WAVES; }
// floats of the tile that starts at row r0 (the last tile may be short)
__device__ __forceinline__ int tile_len(long rows, long r0, int A) { return (int)((rows - r0 < ROWS ? rows - r0 : ROWS) * A); }

// the wave copies n floats of each of K operands, global -> LDS or back; element e of all K moves in one loop trip.
// ONES: the last source may be NULL and its tile is then filled with 1.0 (mixers.hip: no availability given = every action
// available).  Only that one is tested: a test in front of every load would serialise them
template <int K, bool ONES = false>
__device__ __forceinline__ void copy(float* const (&dst)[K], const float* const (&src)[K], int n, int vec) {
  const int lane = threadIdx.x & 63;
  const int n4 = vec ? n >> 2 : 0;                      // (bases not 16-byte aligned: plain element copy)
  for (int e = lane; e < n4; e += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      reinterpret_cast<f32x4*>(dst[k])[e] =
          (ONES && k == K - 1 && !src[k]) ? (f32x4){1.f, 1.f, 1.f, 1.f} : reinterpret_cast<const f32x4*>(src[k])[e];
  }
  for (int e = 4 * n4 + lane; e < n; e += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) dst[k][e] = (ONES && k == K - 1 && !src[k]) ? 1.f : src[k][e];
  }
}
// one operand
__device__ __forceinline__ void copy(float* dst, const float* src, int n, int vec) {
  float* const d[1] = {dst};
  const float* const s[1] = {src};
  copy<1>(d, s, n, vec);
}

// this wave's LDS traffic is done (lgkmcnt(0)): tiles are not shared across waves.  The fenced form also pins the compiler's order
__device__ __forceinline__ void lds_done() { __builtin_amdgcn_s_waitcnt(0xC07F); }
__device__ __forceinline__ void lds_done_fenced() { lds_done(); __builtin_amdgcn_wave_barrier(); }

// first-index argmax of one row of sel (LDS or global) over its available actions: an unavailable action counts as mask_val.
// Returns the index, *best its (masked) value.  What is read at the index, and how that is masked, is the caller's
__device__ __forceinline__ int masked_argmax_row(const float* sel, const float* avail, float mask_val, int A, float* best) {
  float b = 0.f; int arg = 0;
  for (int a = 0; a < A; ++a) {
    float v = sel[a];
    if (avail && avail[a] == 0.f) v = mask_val;
    if (a == 0 || v > b) { b = v; arg = a; }              // strict >: first index wins ties (torch)
  }
  *best = b;
  return arg;
}

// Launch plan of a tiled kernel with `operands` staged tiles per wave.  tiled: they fit lds_cap (else the row-per-lane twin);
// blocks: one wave per tile, at most grid_cap workgroups; vec: every base is 16-byte aligned (NULL counts as aligned)
struct Plan { bool tiled; int blocks; size_t lds_bytes; int vec; };
inline Plan plan(long rows, int A, int operands, size_t lds_cap, int grid_cap, std::initializer_list<const void*> bases) {
  Plan p;
  p.lds_bytes = (size_t)WAVES * operands * tile_floats(A) * sizeof(float);
  p.tiled = p.lds_bytes <= lds_cap;
  const long b = (tiles(rows) + WAVES - 1) / WAVES;
  p.blocks = (int)(b > grid_cap ? grid_cap : b);
  p.vec = 1;
  for (const void* q : bases) p.vec &= aligned16(q);
  return p;
}
// grid of a row-per-lane kernel (SUMS_TPB lanes per workgroup) that ends in block_partials
inline int partial_blocks(long rows) {
  const long b = (rows + SUMS_TPB - 1) / SUMS_TPB;
  return (int)(b > PARTIAL_ROWS ? PARTIAL_ROWS : (b < 1 ? 1 : b));
}

}  // namespace row_tile
