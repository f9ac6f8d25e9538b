// Row helpers of the stochastic policy (policy.hip has the definition and the derivation): the scalars of a row, pi, log pi(u) and
// the entropy with their gradients by the logits, and the sampler's ordered walk.  Shared by policy.hip, coma.hip and the rollout
// kernels (rollout.hip, rollout_fused.hip); a row's A logits / availability flags may lie in LDS or in global memory.
#pragma once
#include "common.h"

namespace {

constexpr float EXP_CLAMP = 80.f;

struct RowPolicy { float mx, S, Sa, D, cw, ew; int n; };     // w_k = cw e_k + ew

// the scalars of one row; z, a: the row's A logits / availability flags (LDS or global)
__device__ __forceinline__ RowPolicy row_policy(const float* z, const float* a, int A, float eps) {
  RowPolicy p;
  p.n = 0; p.mx = 0.f;
  for (int k = 0; k < A; ++k) {
    if (a[k] == 0.f) continue;
    const float v = z[k];
    if (p.n == 0 || v > p.mx) p.mx = v;
    ++p.n;
  }
  p.S = 0.f; p.Sa = 0.f; p.D = 1.f; p.cw = 0.f; p.ew = 0.f;
  if (p.n == 0) return p;
  for (int k = 0; k < A; ++k) {
    const float e = expf(fminf(z[k] - p.mx, EXP_CLAMP));
    p.S += e;
    if (a[k] != 0.f) p.Sa += e;
  }
  p.cw = 1.f - eps;
  p.ew = eps * p.S / (float)p.n;
  p.D = p.cw * p.Sa + eps * p.S;
  return p;
}
__device__ __forceinline__ float row_e(const RowPolicy& p, float z) { return expf(fminf(z - p.mx, EXP_CLAMP)); }

// row_policy of a row whose e_k = row_e(z_k) a caller already holds (e: all A columns, computed against the row's mx): the same
// ordered fp32 sums S (all columns) and Sa (the available ones) and the same statements for n, cw, ew and D; mx is not needed again
__device__ __forceinline__ RowPolicy row_policy_e(const float* e, const float* a, int A, float eps) {
  RowPolicy p;
  p.n = 0; p.mx = 0.f;
  for (int k = 0; k < A; ++k)
    if (a[k] != 0.f) ++p.n;
  p.S = 0.f; p.Sa = 0.f; p.D = 1.f; p.cw = 0.f; p.ew = 0.f;
  if (p.n == 0) return p;
  for (int k = 0; k < A; ++k) {
    const float ek = e[k];
    p.S += ek;
    if (a[k] != 0.f) p.Sa += ek;
  }
  p.cw = 1.f - eps;
  p.ew = eps * p.S / (float)p.n;
  p.D = p.cw * p.Sa + eps * p.S;
  return p;
}

// the sampler's walk (marl_policy_sample, include/marl_hip.h): the running fp32 sum of (cw e_k + ew) / D over the available actions
// in index order; the first k whose sum exceeds the draw u, the last available action when rounding leaves none (action 0 when no
// action is available: cannot happen for a live agent).  E_ROW: z holds the row's e_k (row_policy_e) instead of its logits
template <bool E_ROW = false>
__device__ __forceinline__ int row_walk(const RowPolicy& p, const float* z, const float* av, int A, float u) {
  const float inv = 1.f / p.D;
  int arg = -1, last = 0;
  float cum = 0.f;
  for (int k = 0; k < A; ++k) {
    if (av[k] == 0.f) continue;
    last = k;
    cum += (p.cw * (E_ROW ? z[k] : row_e(p, z[k])) + p.ew) * inv;
    if (cum > u) { arg = k; break; }
  }
  return arg >= 0 ? arg : last;
}
// one draw from the policy of a row: row_policy's scalars, then the walk
__device__ __forceinline__ int row_sample(const RowPolicy& p, const float* z, const float* av, int A, float u) {
  return row_walk<false>(p, z, av, A, u);
}

// pi of one row, written over out (out may be z)
__device__ __forceinline__ void row_probs(const float* z, const float* a, float* out, int A, float eps) {
  const RowPolicy p = row_policy(z, a, A, eps);
  const float inv = 1.f / p.D;
  for (int k = 0; k < A; ++k) out[k] = (p.n > 0 && a[k] != 0.f) ? (p.cw * row_e(p, z[k]) + p.ew) * inv : 0.f;
}

// { L1, Hn } = { sum a_k e_k log pi_k, sum pi_k log pi_k } of a row with a policy; a term whose pi_k = 0 is 0
__device__ __forceinline__ float2 row_ent_sums(const RowPolicy& p, const float* z, const float* a, int A) {
  const float logD = logf(p.D), invD = 1.f / p.D;
  float L1 = 0.f, Hn = 0.f;
  for (int k = 0; k < A; ++k) {
    if (a[k] == 0.f) continue;
    const float e = row_e(p, z[k]);
    const float w = p.cw * e + p.ew;
    if (w > 0.f) {
      const float lp = logf(w) - logD;
      L1 += e * lp;
      Hn += w * invD * lp;
    }
  }
  return make_float2(L1, Hn);
}

// scale * d log pi_u / dz written over out (out may be z); returns log pi_u.  A row without a policy (n = 0, or a taken action
// that is not available) returns `false`: exact zeros and log pi = 0, whatever z holds
__device__ __forceinline__ bool row_logp_grad_of(const RowPolicy& p, const float* z, const float* a, float* out, int A, int u,
                                                 float scale, float& logp) {
  logp = 0.f;
  if (p.n == 0 || u < 0 || u >= A || a[u] == 0.f) {
    for (int k = 0; k < A; ++k) out[k] = 0.f;
    return false;
  }
  if (p.n == 1) {                      // the one available action: pi = 1 whatever the logits hold, log pi = 0, no gradient
    for (int k = 0; k < A; ++k) out[k] = 0.f;
    return true;
  }
  const float eu = row_e(p, z[u]);
  const float wu = p.cw * eu + p.ew;
  logp = logf(wu) - logf(p.D);
  const float invS = 1.f / p.S, Pa = p.Sa * invS;
  const float c1 = p.cw * eu / wu, c2 = p.cw / p.D;
  for (int k = 0; k < A; ++k) {
    const float e = row_e(p, z[k]);
    const float ak = a[k] != 0.f ? 1.f : 0.f;
    out[k] = scale * (c1 * ((k == u ? 1.f : 0.f) - e * invS) - c2 * e * (ak - Pa));
  }
  return true;
}
__device__ __forceinline__ bool row_logp_grad(const float* z, const float* a, float* out, int A, float eps, int u, float scale,
                                              float& logp) {
  return row_logp_grad_of(row_policy(z, a, A, eps), z, a, out, A, u, scale, logp);
}

// row_logp_grad with the entropy H = - sum_{a_k = 1} pi_k log pi_k of the row's policy (0 log 0 = 0: w_k underflows to 0 at
// eps = 0 once z_k sits about 104 below mx) and, for hs != 0, out = scale d log pi_u / dz - hs dH / dz.  With
// L1 = sum a_k e_k log pi_k and Hn = sum pi_k log pi_k = -H (one walk, before out - which may be z - is written):
//   dH/dz_i = -c2 (a_i e_i log pi_i - e_i L1 / S) + c2 e_i (a_i - Pa) Hn          (the second walk; -pi_i (log pi_i + H) at eps = 0).
// hs = 0 takes row_logp_grad's own walk: the same bits.  A row with n = 1 has H = 0 and no gradient.
// SPLIT (marl_ppo_loss_bwd): the last combine rounds scale * (..) and hs * dH each before they are subtracted.  That is the form the
// compiler gives the marl_policy_loss_bwd_ex instantiations of its own accord (their ISA: a packed multiply, then a subtract), while
// it fused hs * dH into the subtraction in the PPO ones - and the PPO pass without logp_old is held to the _ex pass bit for bit
// (tests/test_gpu_ppo.py).  The callers without SPLIT compile the statement they always had
// dH/dz_k of the comment above, from the row's scalars and column k's e, a and w = cw e + ew
__device__ __forceinline__ float row_dH(float e, float ak, float w, float logD, float c2, float Pa, float Hn, float L1S) {
  const float elp = (ak != 0.f && w > 0.f) ? e * (logf(w) - logD) : 0.f;
  return c2 * (e * (ak - Pa) * Hn - (elp - e * L1S));
}
template <bool SPLIT = false>
__device__ __forceinline__ bool row_logp_ent_grad_of(const RowPolicy& p, const float* z, const float* a, float* out, int A, int u,
                                                     float scale, float hs, float& logp, float& H) {
  H = 0.f;
  const bool spread = p.n > 1 && u >= 0 && u < A && a[u] != 0.f;      // a policy over more than one action
  if (!spread || hs == 0.f) {
    if (spread) H = -row_ent_sums(p, z, a, A).y;
    return row_logp_grad_of(p, z, a, out, A, u, scale, logp);
  }
  const float2 s = row_ent_sums(p, z, a, A);
  const float L1 = s.x, Hn = s.y;
  H = -Hn;
  const float eu = row_e(p, z[u]);
  const float wu = p.cw * eu + p.ew;
  const float logD = logf(p.D);
  logp = logf(wu) - logD;
  const float invS = 1.f / p.S, Pa = p.Sa * invS;
  const float c1 = p.cw * eu / wu, c2 = p.cw / p.D;
  const float L1S = L1 * invS;
  for (int k = 0; k < A; ++k) {
    const float e = row_e(p, z[k]);
    const float ak = a[k] != 0.f ? 1.f : 0.f;
    const float w = p.cw * e + p.ew;
    const float dH = row_dH(e, ak, w, logD, c2, Pa, Hn, L1S);
    if constexpr (SPLIT) {
      const float g = c1 * ((k == u ? 1.f : 0.f) - e * invS) - c2 * e * (ak - Pa);
      {
#pragma clang fp contract(off)
        out[k] = scale * g - hs * dH;
      }
    } else {
      out[k] = scale * (c1 * ((k == u ? 1.f : 0.f) - e * invS) - c2 * e * (ak - Pa)) - hs * dH;
    }
  }
  return true;
}
__device__ __forceinline__ bool row_logp_ent_grad(const float* z, const float* a, float* out, int A, float eps, int u, float scale,
                                                  float hs, float& logp, float& H) {
  return row_logp_ent_grad_of(row_policy(z, a, A, eps), z, a, out, A, u, scale, hs, logp, H);
}

// The transpose-Jacobian of pi by the logits applied to g (A values, read on available actions only), less hs dH/dz:
//   (J^T g)_i = (e_i / D) [ (1 - eps) a_i g_i + (eps / n) sum_k a_k g_k - ((1 - eps) a_i + eps) sum_k pi_k g_k ]
// (pi_i (g_i - sum_k pi_k g_k) on available actions and 0 elsewhere at eps = 0), written over out, which may be z or g: column k of
// both is read before out[k] is written, the sums before any.  H: the row's entropy (row_ent_sums).  A row without a policy
// (n = 0) returns `false`; it and a row with one available action (pi = 1 whatever the logits hold) get exact zeros and H = 0
__device__ __forceinline__ bool row_probs_bwd(const RowPolicy& p, const float* z, const float* a, const float* g, float* out, int A,
                                              float eps, float hs, float& H) {
  H = 0.f;
  if (p.n <= 1) {
    for (int k = 0; k < A; ++k) out[k] = 0.f;
    return p.n == 1;
  }
  const float invD = 1.f / p.D;
  float sag = 0.f, spg = 0.f;
  for (int k = 0; k < A; ++k) {
    if (a[k] == 0.f) continue;
    const float gk = g[k];
    sag += gk;
    spg += (p.cw * row_e(p, z[k]) + p.ew) * invD * gk;
  }
  const float2 s = row_ent_sums(p, z, a, A);
  const float Hn = s.y;
  H = -Hn;
  const float logD = logf(p.D);
  const float invS = 1.f / p.S, Pa = p.Sa * invS, c2 = p.cw / p.D, L1S = s.x * invS;
  const float us = eps / (float)p.n * sag;
  for (int k = 0; k < A; ++k) {
    const float e = row_e(p, z[k]);
    const float ak = a[k] != 0.f ? 1.f : 0.f;
    const float gk = ak != 0.f ? g[k] : 0.f;
    float v = e * invD * (p.cw * ak * gk + us - (p.cw * ak + eps) * spg);
    if (hs != 0.f) v -= hs * row_dH(e, ak, p.cw * e + p.ew, logD, c2, Pa, Hn, L1S);
    out[k] = v;
  }
  return true;
}

}  // namespace
