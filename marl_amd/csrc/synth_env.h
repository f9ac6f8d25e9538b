// The synthetic SMAC-shaped environment of every rollout kernel (rollout.hip, rollout_fused.hip, rollout_x6.hip, rollout_x6_v1.hip):
// its counter hash and its rules; numpy restatement: oracle/rollout.py - bit for bit.  The kernels keep their own work split, lane
// mapping and LDS layout.  Some rules stay written out at their sites, because a function for them compiles to other machine code
// there: the episode length (below), the step's record (r = the agent-order sum / N, 0 once over | terminated | padded), the
// agent-order wave sum in rollout_fused.hip and rollout_x6_v1.hip, and rollout.hip's short-circuit availability test.  Helpers
// return results through a reference where a returned value would carry attributes that change the kernels' code.
#pragma once
#include "common.h"

// (ST_SAMPLE: the draws of the stochastic policy, policy.hip.  Its number is also the MAIC latent noise's, maic_head.hip: the two
// never meet, a policy controller has no head.  ST_GUMBEL: the logistic noise of G2ANet's hard attention, g2anet.hip.  Streams
// other files declare: 16 .. 19 the battle starts, battle_env.h; 24 MAVEN's noise index, maven.hip; 32 .. 36 the hunt environment's
// starts HT_PX, HT_PY, HT_QX, HT_QY and its prey walk HT_MOVE, hunt_env.h)
enum { ST_OBS = 0, ST_STATE, ST_AVAIL, ST_REWARD, ST_LEN, ST_WON, ST_EXPLORE, ST_PICK, ST_SAMPLE, ST_GUMBEL };

__host__ __device__ inline unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
// prefix over (seed, stream, env, t); hfin() adds the element index
__host__ __device__ inline unsigned hprefix(unsigned seed, unsigned stream, unsigned env, unsigned t) {
  unsigned h = mix32(seed + stream * 0x9E3779B1u);
  h = mix32(h + env * 0x85EBCA77u + 1u);
  h = mix32(h + t * 0xC2B2AE3Du + 2u);
  return h;
}
__host__ __device__ inline unsigned hfin(unsigned prefix, unsigned idx) { return mix32(prefix + idx * 0x27D4EB2Fu + 3u); }
__host__ __device__ inline unsigned hkey(unsigned seed, unsigned stream, unsigned env, unsigned t, unsigned idx) {
  return hfin(hprefix(seed, stream, env, t), idx);
}
__host__ __device__ inline float u01(unsigned h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// time index of slot (or step) t of an episode: an episode has T + 1 slots
__host__ __device__ inline unsigned env_tg(int episode, int T, int t) { return (unsigned)(episode * (T + 1) + t); }

// ---- the episode: length lmin + hash % (T - lmin + 1) with lmin = max(T / 2, 1), or T with fixed_len (written out); won = the low
// bit of a hash
__host__ __device__ inline int env_won(unsigned seed, unsigned env, int episode) {
  return (int)(hkey(seed, ST_WON, env, (unsigned)episode, 0u) & 1u);
}

// ---- slot t: live while t <= L (slot L is the final observation), zeros after
// an observation / state element: 2u - 1
__host__ __device__ inline float env_value(unsigned prefix, unsigned idx) { return 2.0f * u01(hfin(prefix, idx)) - 1.0f; }
// action k of an agent: always action 0, any other when its draw u (element n A + k) is below 0.7
__host__ __device__ inline bool env_avail(float u, int k) { return (k == 0) | (u < 0.7f); }

// ---- step t: live while t < L
// agent n's reward term for action a (element idx = n A + a): u - 0.5
__host__ __device__ inline float env_reward_term(unsigned prefix, unsigned idx) { return u01(hfin(prefix, idx)) - 0.5f; }
// the agent-order sum on every lane of an environment's N consecutive lanes l0 .. l0 + N - 1 of a wave (four shuffles in flight)
__device__ inline void env_agent_sum(float term, int l0, int N, float& acc) {
  acc = 0.f;
  for (int n0 = 0; n0 < N; n0 += 4) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __shfl(term, (l0 + n0 + k) & 63, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = n0 + k < N ? acc + v[k] : acc;
  }
}

// ---- the epsilon-greedy choice (share_params.py:66-70): explore when the ST_EXPLORE draw is below epsilon, then take the k-th
// available action, k = floor(u navail) of the ST_PICK draw u, clamped
__host__ __device__ inline void env_pick(float u, int navail, int& k) {
  k = (int)floorf(u * (float)navail);
  if (k > navail - 1) k = navail - 1;
}
// epsilon of the next lock-step without a device vector: the reference's anneal (rollout.py:100-101) in fp64
__host__ __device__ inline double eps_anneal_step(double eps, double anneal, double eps_min) { return eps > eps_min ? eps - anneal : eps; }
