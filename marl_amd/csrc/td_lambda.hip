// TD(lambda) returns of the Q learners (reference utils/rl_utils.py:4-14, build_td_lambda_targets, with the terminal flag masked
// by the padding - include/marl_hip.h has the definition).  Per episode, with q[t] the target network's value at the NEXT state
// of step t, m = 1 - padded, a = lambda gamma:
//   done = sum_t m[t] term[t],   G[T] = q[T-1] (1 - done),
//   G[t] = a G[t+1] + c[t],      c[t] = m[t] (r[t] + (1 - lambda) gamma q[t] (1 - term[t])),   t = T-1 .. 0.
// One wave per episode, lanes along t: every global access is a coalesced row segment.  The row is walked in chunks of 64 steps
// from the last one down; inside a chunk the recursion is a weighted suffix scan over the wave, x[l] = sum_{d >= 0} a^d c[l + d],
// six shuffle steps with the powers a^1, a^2, .. a^32 (formed once, by repeated squaring), and what lies behind the chunk enters
// as a^(valid - l) G[t0 + valid]; lane 0 then holds the carry of the chunk in front.  A partial last chunk (and T < 64) is the
// same code: lanes past the row contribute 0.  Fixed order of operations, no atomics, no LDS: two calls give the same bits.
#include "common.h"
#include "../../include/marl_hip.h"

namespace {

constexpr int TL_TPB = 256;          // four waves = four episodes per workgroup pass
constexpr int TL_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(TL_TPB) void td_lambda_kernel(const float* __restrict__ q, const float* __restrict__ r,
                                                           const float* __restrict__ term, const float* __restrict__ padded,
                                                           float gamma, float lambda, float* __restrict__ ret, int B, int T) {
  const int lane = threadIdx.x & 63;
  const long wave_id = ((long)blockIdx.x * TL_TPB + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * TL_TPB) >> 6;
  const float a = lambda * gamma, k1 = (1.f - lambda) * gamma;
  float ap[7];                       // a^(2^k): the scan's weights, and the factors of the carry's a^(valid - lane)
  ap[0] = a;
#pragma unroll
  for (int k = 1; k < 7; ++k) ap[k] = ap[k - 1] * ap[k - 1];
  const int nchunks = (T + 63) >> 6;
  for (long b = wave_id; b < B; b += nwaves) {
    const long row = b * (long)T;
    // pass 1: did the episode terminate inside the window (real rows only: padded rows carry term = 1)
    float done = 0.f;
    for (int t = lane; t < T; t += 64) done += (1.f - padded[row + t]) * term[row + t];
    done = wave_sum(done);
    // G[T]: the bootstrap behind the window, only for an episode cut before it terminated
    float carry = done == 1.f ? 0.f : q[row + T - 1] * (1.f - done);
    // pass 2
    for (int c = nchunks - 1; c >= 0; --c) {
      const int t0 = c << 6;
      const int valid = T - t0 < 64 ? T - t0 : 64;
      const bool active = lane < valid;
      float x = 0.f;
      if (active) {
        const long i = row + t0 + lane;
        const float m = 1.f - padded[i];
        if (m != 0.f) x = m * fmaf(k1 * q[i], 1.f - term[i], r[i]);     // a padded row is an exact +0, whatever r and q hold
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int d = 1 << k;
        const float y = __shfl_down(x, d, 64);
        if (lane + d < 64) x = fmaf(ap[k], y, x);
      }
      // a^(valid - lane), exponent in 1 .. 64, from its binary digits
      const int e = valid - lane;
      float pw = 1.f;
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (e & (1 << k)) pw *= ap[k];
      x = fmaf(pw, carry, x);
      if (active) ret[row + t0 + lane] = x;
      carry = __shfl(x, 0, 64);
    }
  }
}

}  // namespace

extern "C" int marl_td_lambda_returns(const float* q_next_tot, const float* r, const float* term, const float* padded,
                                      float gamma, float lambda, float* ret, int B, int T, void* stream) {
  if (B <= 0 || T <= 0) return 0;
  if (!q_next_tot || !r || !term || !padded || !ret || ret == q_next_tot || ret == r || ret == term || ret == padded)
    return (int)hipErrorInvalidValue;
  long nb = ((long)B * 64 + TL_TPB - 1) / TL_TPB;
  if (nb > TL_MAX_BLOCKS) nb = TL_MAX_BLOCKS;
  hipLaunchKernelGGL(td_lambda_kernel, dim3((unsigned)nb), dim3(TL_TPB), 0, (hipStream_t)stream, q_next_tot, r, term, padded,
                     gamma, lambda, ret, B, T);
  MARL_CHECK_LAUNCH();
  return 0;
}
