// Advantage standardisation of the PPO learner (include/marl_hip.h has the definition): over x (rows) and padded (rows), with
// m = 1 - padded and M = sum m,
//   mean = sum m x / M,   var = sum m (x - mean)^2 / M,   out = m (x - mean) / (sqrt(var) + 1e-5).
// The mean and the variance are each a pass of their own (E[x^2] - mean^2 cancels in fp32 once |mean| passes the spread), the
// third pass writes out.  Every sum goes through sums.h: block partials in the workspace, one single-workgroup launch that adds
// them in a fixed order - two calls give the same bits.  The raw sums wait in the workspace's last four floats (the partials use
// at most its first half), so nothing reads stats3 and the third pass may write it.  rows is B*T (491 520 at the full size): plain
// grid-stride loops, one float per lane.
#include "sums.h"
#include "row_tile.h"
#include "../../include/marl_hip.h"

namespace {

constexpr int TPB = SUMS_TPB;
constexpr int PS_RAW = row_tile::PARTIAL_ROWS * 4 - 4;   // { sum m x, M, sum m (x - mean)^2 } behind the partials
constexpr float PS_EPS = 1e-5f;

__device__ __forceinline__ float ps_mean(const float* raw) { return raw[1] > 0.f ? raw[0] / raw[1] : 0.f; }

// partials { sum m x, sum m }; a padded row's x is never looked at
__global__ __launch_bounds__(TPB) void ps_sum_kernel(const float* __restrict__ x, const float* __restrict__ padded, float* ws, long rows) {
  float acc[2] = {};
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < rows; i += (long)gridDim.x * TPB) {
    const float m = 1.f - padded[i];
    if (m != 0.f) acc[0] += m * x[i];
    acc[1] += m;
  }
  block_partials<2>(acc, ws);
}

// partials { sum m (x - mean)^2 }
__global__ __launch_bounds__(TPB) void ps_var_kernel(const float* __restrict__ x, const float* __restrict__ padded, float* ws, long rows) {
  const float mean = ps_mean(ws + PS_RAW);
  float acc[1] = {};
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < rows; i += (long)gridDim.x * TPB) {
    const float m = 1.f - padded[i];
    if (m != 0.f) {
      const float d = x[i] - mean;
      acc[0] += m * d * d;
    }
  }
  block_partials<1>(acc, ws);
}

// out may be x: every lane reads its own x[i] before it writes out[i]
__global__ __launch_bounds__(TPB) void ps_write_kernel(const float* x, const float* __restrict__ padded, const float* __restrict__ ws,
                                                       float* out, float* __restrict__ stats3, long rows) {
  const float* raw = ws + PS_RAW;
  const float M = raw[1], mean = ps_mean(raw);
  const float var = M > 0.f ? raw[2] / M : 0.f;
  const float inv = 1.f / (sqrtf(var) + PS_EPS);
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < rows; i += (long)gridDim.x * TPB) {
    const float m = 1.f - padded[i];
    out[i] = m != 0.f ? m * (x[i] - mean) * inv : 0.f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { stats3[0] = mean; stats3[1] = var; stats3[2] = M; }
}

}  // namespace

extern "C" int marl_masked_standardize(const float* x, const float* padded, float* out, float* stats3, float* ws, long rows,
                                       void* stream) {
  if (rows <= 0) return 0;
  if (!x || !padded || !out || !stats3 || !ws || out == padded) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int nb = row_tile::partial_blocks(rows);
  hipLaunchKernelGGL(ps_sum_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, x, padded, ws, rows);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, s, (const float*)ws, nb, 2, ws + PS_RAW);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(ps_var_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, x, padded, ws, rows);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(TPB), 0, s, (const float*)ws, nb, 1, ws + PS_RAW + 2);
  MARL_CHECK_LAUNCH();
  hipLaunchKernelGGL(ps_write_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, x, padded, (const float*)ws, out, stats3, rows);
  MARL_CHECK_LAUNCH();
  return 0;
}
