// What the per-step kernels of the device environments share (battle.hip, hunt.hip): the wave-wide write of one contiguous run of a
// record slot, and the action choice in front of a fused step.
#pragma once
#include "policy_rows.h"
#include "synth_env.h"

namespace {

// p[0 .. n) = f(0 .. n) by the 64 lanes of a wave: scalar stores up to the first 16-byte boundary and after the last, f32x4 between
template <class F>
__device__ __forceinline__ void write_run(float* p, int n, int lane, F f) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int body = (n - head) >> 2;
  if (lane < head) p[lane] = f(lane);
  for (int q = lane; q < body; q += MARL_WAVE) {
    const int k = head + 4 * q;
    f32x4 v;
    v[0] = f(k); v[1] = f(k + 1); v[2] = f(k + 2); v[3] = f(k + 3);
    *reinterpret_cast<f32x4*>(p + k) = v;
  }
  const int tail = head + 4 * body;
  if (tail + lane < n) p[tail + lane] = f(tail + lane);
}

// The choice of agent n of environment env at time index tg from its row qa of q and its availability row av (both A wide):
// select_kernel's epsilon-greedy rule and draws (rollout.hip), or with SAMPLE policy_sample's draw from the stochastic policy of the
// row, keyed by (rseed, env, tg, n)
template <bool SAMPLE>
__device__ __forceinline__ int env_choose(const float* qa, const float* av, int A, float eps, unsigned rseed, unsigned env, unsigned tg,
                                          int n) {
  int arg = -1;
  if constexpr (SAMPLE) {
    const RowPolicy p = row_policy(qa, av, A, eps);
    arg = row_sample(p, qa, av, A, u01(hkey(rseed, ST_SAMPLE, env, tg, (unsigned)n)));
  } else {
    float best = 0.f; int navail = 0;
    for (int k = 0; k < A; ++k) {
      if (av[k] == 0.f) continue;
      ++navail;
      if (arg < 0 || qa[k] > best) { best = qa[k]; arg = k; }
    }
    if (arg < 0) arg = 0;
    const bool explore = u01(hkey(rseed, ST_EXPLORE, env, tg, (unsigned)n)) < eps;
    if (explore && navail > 0) {
      int kk;
      env_pick(u01(hkey(rseed, ST_PICK, env, tg, (unsigned)n)), navail, kk);
      int cnt = 0;
      for (int k = 0; k < A; ++k) {
        if (av[k] == 0.f) continue;
        if (cnt == kk) { arg = k; break; }
        ++cnt;
      }
    }
  }
  return arg;
}

}  // namespace
