// THE FIRST DECOMPOSITION of the split whole-rollout kernel (round 5), kept behind marl_experiment_set("rollout_v1", 1) as the
// bitwise twin of rollout_x6.hip (same arithmetic, another division of labour: tests/test_gpu_rollout.py compares the two records).
// Whole-rollout persistent kernel with the agent step as bf16x6 split products (x6.h; args.gemm_mode = "bf16x6"): ONE launch plays all
// T lock-steps of E synthetic SMAC-shaped environments (reference rollout.py:60-101 + controller/share_params.py:37-72, vectorised).
// Same environment (synth_env.h), same epsilon-greedy choice, same episode record as rollout_fused.hip (the fp32 MFMA kernel); the
// agent's products (network/q_network.py:16-21) are six bf16 MFMA products each, fp32 accumulate.
//
// Why it is another decomposition and not a variant of rollout_fused.hip: pre-split, a hidden-unit slice's weights are 204 registers,
// so the two teams of the workgroup hold DIFFERENT weights (as in agent_x6.hip) - and a rollout cannot run its input side ahead of
// the recurrence, because step t + 1's input contains the action chosen at step t.  What can run ahead is the OBSERVATION part of fc1
// (the environment's observations do not depend on the actions): fc1 = (bias + W1[:, obs | id] in) - on the matrix cores, a step
// ahead - + W1[:, O + u], one column of fp32 weights added per row once u is known (a table in LDS).
//   team R (waves 0-3, hidden-unit slice s): W_hh and fc1 fragments (72 + 12 NK1 registers), the hidden state in fp32 registers
//   team I (waves 4-7, slice s):             W_ih and fc2 fragments (72 + 24)
// A lock-step, four LDS-only barriers:
//   P1  R: gates(t) = GI(t) + h(t-1) W_hh, gate math, h(t) -> planes          I: generate the observations of slot t+1 (record + planes)
//   P2  R: pre(t+1) = fc1 of the slot-(t+1) planes                            I: q(t) = fc2(h(t)) and the epsilon-greedy choice IN REGISTERS
//                                                                                (a wave holds a row tile's 16 actions on 16 lanes: DPP max + ballots)
//   P3  R: x(t+1) = relu(pre + W1[:, O + u(t)]) -> planes                     I: env step (reward / terminated / padded), next uniforms, hash prefixes
//   P4  R: generate state + availability of slot t+2                         I: GI(t+1) = bias + x(t+1) W_ih -> LDS
// A workgroup holds whole environments in RTC <= 3 row tiles of 16 (episode, agent) rows (~45 KB of LDS per tile); larger batches
// run in rounds of workgroups (4096 envs x 5 agents: 512 workgroups of 8 environments = two full rounds).
#include "x6.h"
#include "synth_rollout.h"

namespace {

template <int RTC, int NK1>
__global__ __launch_bounds__(RNT, 2) void synth_rollout_x6_kernel(RX6Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int team = wave >> 2, s = wave & 3;      // team 0 = R (recurrent + fc1), team 1 = I (W_ih + fc2 + choice)
  const int q = lane >> 4, m = lane & 15, u = 16 * s + m;
  constexpr int rows = 16 * RTC;
  const int T = a.T, N = a.N, O = a.O, S = a.S, A = a.A;
  const int IP = a.KI + 8;
  const int IN_E = 3 * rows * IP, XP_E = 3 * rows * HP;
  short* In0 = reinterpret_cast<short*>(smem);                             // [3][rows][IP]   input planes of the slot to come
  short* Xp0 = In0 + IN_E;                                                 // [3][rows][HP]   x(t+1)
  short* Hp0 = Xp0 + XP_E;                                                 // [2][3][rows][HP] h by step parity
  float* GI0 = reinterpret_cast<float*>(Hp0 + 2 * XP_E);                   // [RTC][4][3][64] f32x4
  float* Av0 = GI0 + RTC * 4 * 3 * 256;                                    // [2][rows][A] availability by slot parity
  float* W1a = Av0 + 2 * rows * A;                                         // [A + 1][64]: fc1 columns of the one-hot(last action) block; row A = zeros
  int* act = reinterpret_cast<int*>(W1a + (A + 1) * H);                    // [rows]
  int* rowe = act + rows;                                                  // [rows] local env of the row
  int* rown = rowe + rows;                                                 // [rows] agent
  int* elen = rown + rows;                                                 // [rows] episode length of the local env
  unsigned* pfxO = reinterpret_cast<unsigned*>(elen + rows);               // [rows] hash prefix of the observations of the slot to generate
  unsigned* pfxA = pfxO + rows;                                            // [rows] ... of its availability
  unsigned* pfxS = pfxA + rows;                                            // [rows] ... of its state (per env: entries 0 .. EPW-1); entries rows/2 .. : the reward hash prefix of the NEXT step, per env
  float* uex = reinterpret_cast<float*>(pfxS + rows);                      // [2 step parities][2][rows] explore / pick uniforms of a step's choice
  int4* rmeta = reinterpret_cast<int4*>(uex + 4 * rows);                   // [rows] {obs offset of (b,0,n,0), avail offset, episode length, n}
  int4* emeta = rmeta + rows;                                              // [rows] {state offset of (b,0,0), episode length, env in range, -}
  i32x4* W2f = reinterpret_cast<i32x4*>(emeta + rows);                     // [2 k chunks][3 planes][64 lanes]: the fc2 fragments (the same for every wave)
  auto hpp = [&](int b) { return Hp0 + b * XP_E; };

  const int nenv_wg = a.EPW;
  const int vrows = nenv_wg * N;                         // valid rows; rows vrows .. 16 RTC - 1 are padding
  // (the host sizes RTC = ceil(EPW N / 16): every row tile holds valid rows)
  const int b0 = blockIdx.x * nenv_wg;
  const long row0 = (long)b0 * N;
  for (int r = tid; r < rows; r += RNT) {
    long rho = row0 + (r < vrows ? r : vrows - 1);
    if (rho > a.R - 1) rho = a.R - 1;                    // clamp: duplicates of the last row
    rowe[r] = (int)(rho / N) - b0;
    rown[r] = (int)(rho % N);
    act[r] = -1;
  }
  const int lmin = T / 2 > 1 ? T / 2 : 1;
  for (int e = tid; e < nenv_wg; e += RNT) {
    int b = b0 + e; if (b > a.E - 1) b = a.E - 1;
    const unsigned env = (unsigned)(a.env0 + b);
    int L = lmin + (int)(hkey(a.seed, ST_LEN, env, (unsigned)a.episode, 0u) % (unsigned)(T - lmin + 1));
    if (a.fixed_len) L = T;
    elen[e] = L;
    a.length[b] = L;
    const int won_ = env_won(a.seed, env, a.episode);
    a.won[b] = won_;
    if (a.stats && b0 + e < a.E) { a.stats[a.E + b] = (float)won_; a.stats[2L * a.E + b] = (float)L; }
  }
  // planes: zero everywhere (padding rows, pad columns, the one-hot block: its contribution comes from the W1a table), h(-1) = 0
  for (int e = tid; e < (IN_E + 3 * XP_E) / 2; e += RNT) reinterpret_cast<int*>(In0)[e] = 0;
  for (int e = tid; e < (A + 1) * H; e += RNT) {
    const int aa = e / H, j = e % H;
    W1a[e] = (a.has_act && aa < A) ? a.W1[(long)j * a.I + O + aa] : 0.f;
  }
  __syncthreads();
  for (int r = tid; r < vrows; r += RNT) {
    const int el = rowe[r], n = rown[r];
    const int bn = (b0 + el) * (T + 1) * N + n;
    rmeta[r] = make_int4(bn * O, bn * A, elen[el], n);
    if (a.has_id) In0[r * IP + (a.I - N) + n] = (short)0x3F80;      // agent id: bf16 1.0 in the hi plane
  }
  for (int el = tid; el < nenv_wg; el += RNT)
    emeta[el] = make_int4((b0 + el) * (T + 1) * (int)a.SL, elen[el], b0 + el < a.E ? 1 : 0, 0);

  // ---- the environment's slot t -> record (+ input planes / availability); flattened over (row, 4-column group) items, branch-free
  // (rollout_fused.hip: gen_slot); `first` / `nthr`: the threads that share the work
  const int O4 = O >> 2, S4 = (S + 3) >> 2;
  const float invO4 = 1.0f / (float)(O4 > 0 ? O4 : 1), invA = 1.0f / (float)A;
  const float invS4 = 1.0f / (float)(S4 > 0 ? S4 : 1), invS = 1.0f / (float)S;
  const bool svec = (a.SL & 3) == 0 && a.SL >= 4 * S4 && (reinterpret_cast<uintptr_t>(a.state) & 15) == 0;
  auto bits = [](float v) { return __builtin_bit_cast(unsigned, v); };
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  auto gen_prefix_obs = [&](int t, int r) {
    const unsigned tg = env_tg(a.episode, T, t);
    pfxO[r] = hprefix(a.seed, ST_OBS, (unsigned)(a.env0 + b0 + rowe[r]), tg);
  };
  auto gen_prefix_rest = [&](int t, int r) {
    const unsigned tg = env_tg(a.episode, T, t);
    pfxA[r] = hprefix(a.seed, ST_AVAIL, (unsigned)(a.env0 + b0 + rowe[r]), tg);
    if (r < nenv_wg) pfxS[r] = hprefix(a.seed, ST_STATE, (unsigned)(a.env0 + b0 + r), tg);
  };
  // the (row, 4-column group) items of a thread are the same at every step: their metadata is resolved once (gen_obs_items) and
  // kept in registers by the team that generates the observations inside the loop - a step reads only the slot's hash prefix
  constexpr int NOI = NK1 == 3 ? 5 : 8;                    // items per thread of a 256-thread team: rows (<= 48) x O / 4 (<= 8 NK1) <= 256 NOI
  auto gen_obs = [&](int t, bool to_lds, int tl, int nthr) {
    const int tNO = t * N * O;
    for (int e = tl; e < vrows * O4; e += nthr) {
      const int r = (int)(((float)e + 0.5f) * invO4);
      const int k = 4 * (e - r * O4);
      const int4 mt = rmeta[r];
      const unsigned po = pfxO[r];
      const unsigned lm = t <= mt.z ? 0xffffffffu : 0u, fm = t < mt.z ? 0xffffffffu : 0u;
      const unsigned idx = (unsigned)(mt.w * O + k);
      u32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = bits(env_value(po, idx + (unsigned)i)) & lm;
      *reinterpret_cast<u32x4*>(a.obs + (long)mt.x + tNO + k) = v;
      if (to_lds) {                              // padded steps feed zeros (rollout.py:122-133); split once, here
        f32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = __builtin_bit_cast(float, v[i] & fm);
        const F3h f = split4(w);
        short* p = In0 + r * IP + k;
        *reinterpret_cast<i32x2*>(p) = f.h;
        *reinterpret_cast<i32x2*>(p + rows * IP) = f.m;
        *reinterpret_cast<i32x2*>(p + 2 * rows * IP) = f.l;
      }
    }
  };
  auto gen_rest = [&](int t, float* Av, int tl, int nthr) {
    const int tNA = t * N * A, tS = t * (int)a.SL;
    for (int e = tl; e < vrows * A; e += nthr) {
      const int r = (int)(((float)e + 0.5f) * invA);
      const int k = e - r * A;
      const int4 mt = rmeta[r];
      const float uu = u01(hfin(pfxA[r], (unsigned)(mt.w * A + k)));
      const bool on = (t <= mt.z) & env_avail(uu, k);
      const float v = on ? 1.f : 0.f;
      a.avail[(long)mt.y + tNA + k] = v;
      Av[r * A + k] = v;
    }
    if (svec) {
      for (int e = tl; e < nenv_wg * S4; e += nthr) {
        const int el = (int)(((float)e + 0.5f) * invS4);
        const int k = 4 * (e - el * S4);
        const int4 mt = emeta[el];
        const unsigned ps = pfxS[el];
        const unsigned lm = t <= mt.y ? 0xffffffffu : 0u;
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = bits(env_value(ps, (unsigned)(k + i))) & (k + i < S ? lm : 0u);
        if (mt.z) *reinterpret_cast<u32x4*>(a.state + (long)mt.x + tS + k) = v;
      }
    } else {
      for (int e = tl; e < nenv_wg * S; e += nthr) {
        const int el = (int)(((float)e + 0.5f) * invS);
        const int k = e - el * S;
        const int4 mt = emeta[el];
        const unsigned lm = t <= mt.y ? 0xffffffffu : 0u;
        const unsigned v = bits(env_value(pfxS[el], (unsigned)k)) & lm;
        if (mt.z) reinterpret_cast<unsigned*>(a.state)[(long)mt.x + tS + k] = v;
      }
    }
  };
  __syncthreads();
  if (tid < rows) { gen_prefix_obs(0, tid); gen_prefix_rest(0, tid); }
  __syncthreads();
  gen_obs(0, true, tid, RNT);
  gen_rest(0, Av0, tid, RNT);
  __syncthreads();
  if (tid < rows) {       // prefixes of slot 1; uniforms of the first choice
    gen_prefix_obs(1, tid); gen_prefix_rest(1, tid);
    const unsigned env = (unsigned)(a.env0 + b0 + rowe[tid]), tg0 = env_tg(a.episode, T, 0);
    uex[tid] = u01(hkey(a.rseed, ST_EXPLORE, env, tg0, (unsigned)rown[tid]));
    uex[rows + tid] = u01(hkey(a.rseed, ST_PICK, env, tg0, (unsigned)rown[tid]));
  }
  const int KC1 = a.KI >> 5;

  // ---- q = fc2(h) and the epsilon-greedy choice (share_params.py:66-70) of a row tile, in registers: lane (q, m) of the accumulator
  // tile holds rows 4q + r of action m - a row's 16 actions sit on the 16 lanes of a DPP row.  A wave computes q of the tile (12
  // products) and makes the choice of its rows 4q + s (four rows in ONE pass of ballots); the four slice waves of a team cover a
  // tile.  Both teams hold the fc2 fragments: row tiles 0 .. RTI-1 are team I's, the last of three is team R's (it waits otherwise).
  constexpr int RTI = RTC == 3 ? 2 : RTC;
  // (ready fragments in LDS, read back per use: the teams need their registers for their own weights - keeping them in team I's
  // registers was measured: 41 spilled registers in the three-tile instantiation, slower)
  if (wave < 2) {
    const F3 f = wfrag(a.W2, H, 0, A, H, wave, lane);
    W2f[(wave * 3 + 0) * 64 + lane] = f.h; W2f[(wave * 3 + 1) * 64 + lane] = f.m; W2f[(wave * 3 + 2) * 64 + lane] = f.l;
  }
  const float bias_2 = m < A ? a.b2[m] : 0.f;
  int c_rr[RTC], c_len[RTC], c_uoff[RTC], c_av[RTC];      // this lane's row of each tile: its index (clamped), episode length (-1: not a row), offsets
#pragma unroll
  for (int rt = 0; rt < RTC; ++rt) {
    const int row = rt * 16 + 4 * q + s;
    const bool valid = row < vrows;
    const int rr = valid ? row : vrows - 1;
    const int4 mt = rmeta[rr];
    c_rr[rt] = rr; c_len[rt] = valid ? mt.z : -1;
    c_uoff[rt] = (b0 + rowe[rr]) * T * N + mt.w;
    c_av[rt] = rr * A + (m < A ? m : 0);
  }
  auto choose = [&](int rt, int t, float eps) __attribute__((always_inline)) {
    const int par = t & 1;
    F3 hb[2], w2[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      hb[c] = bfrag(hpp(par ^ 1) + rt * 16 * HP, HP, rows * HP, c, lane);
      w2[c].h = W2f[(c * 3 + 0) * 64 + lane]; w2[c].m = W2f[(c * 3 + 1) * 64 + lane]; w2[c].l = W2f[(c * 3 + 2) * 64 + lane];
    }
    f32x4 ac[2] = {splat(bias_2), splat(0.f)};
#define OP(p_, q_) _Pragma("unroll") for (int c = 0; c < 2; ++c) ac[c] = mm(hb[c].p_, w2[c].q_, ac[c]);
    X6_TERMS(OP)
#undef OP
    const f32x4 qv = ac[0] + ac[1];
    const float qs = s == 0 ? qv[0] : s == 1 ? qv[1] : s == 2 ? qv[2] : qv[3];
    const int rr = c_rr[rt], sh = 16 * q;
    const bool on = m < A && Av0[par * rows * A + c_av[rt]] != 0.f;
    const float v = on ? qs : -3.0e38f;
    const float mx = group_max16(v);
    const unsigned am = (unsigned)(__ballot(on) >> sh) & 0xffffu;
    const unsigned em = (unsigned)(__ballot(on && v == mx) >> sh) & 0xffffu;
    const int navail = __popc(am);
    int arg = em ? __ffs(em) - 1 : (am ? __ffs(am) - 1 : 0);
    const bool explore = uex[par * 2 * rows + rr] < eps;
    int kk;
    env_pick(uex[par * 2 * rows + rows + rr], navail, kk);
    const bool sel = explore && on && __popc(am & ((1u << m) - 1u)) == kk;
    const unsigned sm = (unsigned)(__ballot(sel) >> sh) & 0xffffu;
    if (sm) arg = __ffs(sm) - 1;
    if (!(t < c_len[rt])) arg = -1;
    if (c_len[rt] >= 0 && m == 0) {
      act[rt * 16 + 4 * q + s] = arg;
      a.u[c_uoff[rt] + t * N] = arg;
    }
  };
  // (the reward prefixes live in the upper half of pfxS, double-buffered by step parity: EPW <= rows / 4 - always, unless N < 4)
  const bool pre_r = 4 * nenv_wg <= rows;
  // the uniforms of step t+1's choice and the hash prefixes of slot t+2, ONE hash per thread of a 256-thread team (index ti)
  auto hashes = [&](int t, int ti) __attribute__((always_inline)) {
    const unsigned tg = env_tg(a.episode, T, t);
    const int kind = ti / rows, r = ti - kind * rows;
    if (kind < 5) {
      const unsigned env = (unsigned)(a.env0 + b0 + rowe[r]), nn_ = (unsigned)rown[r];
      float* ux = uex + ((t + 1) & 1) * 2 * rows;
      if (kind == 0) ux[r] = u01(hkey(a.rseed, ST_EXPLORE, env, tg + 1u, nn_));
      else if (kind == 1) ux[rows + r] = u01(hkey(a.rseed, ST_PICK, env, tg + 1u, nn_));
      else if (kind == 2) pfxO[r] = hprefix(a.seed, ST_OBS, env, tg + 2u);
      else if (kind == 3) pfxA[r] = hprefix(a.seed, ST_AVAIL, env, tg + 2u);
      else if (r < nenv_wg) pfxS[r] = hprefix(a.seed, ST_STATE, (unsigned)(a.env0 + b0 + r), tg + 2u);
      else if (pre_r && r >= rows / 2 && r - rows / 2 < nenv_wg)      // the reward prefix of step t+1 (off the env step's dependent chain)
        pfxS[rows / 2 + ((t + 1) & 1) * (rows / 4) + (r - rows / 2)] = hprefix(a.seed, ST_REWARD, (unsigned)(a.env0 + b0 + r - rows / 2), tg + 1u);
    }
  };
  // epsilon of step t: a device vector, or the reference's per-step anneal (rollout.py:100-101) evaluated here in fp64
  float eps_next = a.eps ? a.eps[0] : (float)a.eps0;
  double eps_d = a.eps0;

  if (team == 0) {
    // =============================== team R: fc1 (observation part), the recurrence, x ===============================
    F3 wh[6], w1[NK1];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int c = 0; c < 2; ++c) wh[2 * g + c] = wfrag(a.Whh, H, g * H + 16 * s, 3 * H, H, c, lane);
#pragma unroll
    for (int c = 0; c < NK1; ++c) w1[c] = c < KC1 ? wfrag(a.W1, a.I, 16 * s, H, a.I, c, lane) : F3{};
    const float bias_1 = a.b1[u], bias_hn = a.bhh[2 * H + u];
    f32x4 hreg[RTC], pre[RTC];
#pragma unroll
    for (int rt = 0; rt < RTC; ++rt) hreg[rt] = splat(0.f);
    // pre = bias + W1[:, obs | id] in  of every row tile from the input planes (three accumulator chains, chunk c on chain c % 3)
    auto fc1 = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int rt = 0; rt < RTC; ++rt) {
        f32x4 acc[3] = {splat(bias_1), splat(0.f), splat(0.f)};
#pragma unroll
        for (int c0 = 0; c0 < NK1; c0 += 3) {
          F3 xi[3];
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (c0 + c < NK1) xi[c] = bfrag(In0 + rt * 16 * IP, IP, rows * IP, c0 + c < KC1 ? c0 + c : 0, lane);
#define OP(p_, q_) _Pragma("unroll") for (int c = 0; c < 3; ++c) if (c0 + c < NK1) acc[c] = mm(xi[c].p_, w1[c0 + c].q_, acc[c]);
          X6_TERMS(OP)
#undef OP
        }
        pre[rt] = (acc[0] + acc[1]) + acc[2];
      }
    };
    // x = relu(pre + W1[:, O + last action]) -> planes (rows whose last action is "none": the zero row of the table)
    auto xput = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int rt = 0; rt < RTC; ++rt) {
        f32x4 x;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int aa = act[rt * 16 + 4 * q + r];
          x[r] = fmaxf(__fadd_rn(pre[rt][r], W1a[(aa < 0 ? A : aa) * H + u]), 0.f);
        }
        put4(Xp0, HP, rows * HP, rt * 16 + 4 * q, u, x);
      }
    };
    WG_BARRIER();                                  // slot 0 in the planes, tables
    fc1();
    xput();                                        // x(0): no last action
    WG_BARRIER();                                  // x(0) | (team I: GI(0))
    gen_rest(1, Av0 + rows * A, tid, RNT / 2);     // state + availability of slot 1
    WG_BARRIER();
    ST_DECL(8);
    for (int t = 0; t < T; ++t) {
      const int par = t & 1;
      // ---- P1: gates(t) on top of the handed input-side sums, gate math, h(t)
#pragma unroll
      for (int rt = 0; rt < RTC; ++rt) {
        const f32x4* gp = reinterpret_cast<const f32x4*>(GI0) + (rt * 4 + s) * 192 + lane;
        f32x4 ah[3] = {gp[0], gp[64], splat(bias_hn)};
        const f32x4 an = gp[128];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const F3 hb = bfrag(hpp(par) + rt * 16 * HP, HP, rows * HP, c, lane);
#define OP(p_, q_) _Pragma("unroll") for (int g = 0; g < 3; ++g) ah[g] = mm(hb.p_, wh[2 * g + c].q_, ah[g]);
          X6_TERMS(OP)
#undef OP
        }
        f32x4 hn;
#pragma unroll
        for (int r = 0; r < 4; ++r) hn[r] = gru_h_x6(ah[0][r], ah[1][r], an[r], ah[2][r], hreg[rt][r]);
        put4(hpp(par ^ 1), HP, rows * HP, rt * 16 + 4 * q, u, hn);
        hreg[rt] = hn;
      }
      ST_MARK(0);
      WG_BARRIER();                                // B1: h(t) planes | obs planes of slot t+1
      ST_MARK(1);
      // ---- P2: pre(t+1) from the planes team I filled during P1; the hashes of the steps to come (they depend on nothing of this
      // step; the uniforms go to the other parity's buffer - team I reads this step's now); the choice of the third row tile
      const float eps = eps_next;
      if (a.eps) { if (t + 1 < T) eps_next = a.eps[t + 1]; }
      else { eps_d = eps_anneal_step(eps_d, a.eps_anneal, a.eps_min); eps_next = (float)eps_d; }
      if (RTC == 3) choose(RTC - 1, t, eps);
      if (t + 1 < T) fc1();
      hashes(t, tid);
      ST_MARK(2);
      WG_BARRIER();                                // B2: act(t)
      ST_MARK(3);
      // ---- P3: x(t+1)
      if (t + 1 < T) xput();
      ST_MARK(4);
      WG_BARRIER();                                // B3: x(t+1) planes | prefixes of slot t+2
      ST_MARK(5);
      // ---- P4: state + availability of slot t+2 (its availability buffer held slot t's, last read before B2)
      if (t + 2 <= T) gen_rest(t + 2, Av0 + par * rows * A, tid, RNT / 2);
      ST_MARK(6);
      WG_BARRIER();                                // B4: GI(t+1)
      ST_MARK(7);
    }
    ST_DUMP(8);
    if (a.h_out) {
#pragma unroll
      for (int rt = 0; rt < RTC; ++rt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + 4 * q + r;
          const long rho = row0 + row;
          if (row < vrows && rho < a.R) a.h_out[rho * H + u] = hreg[rt][r];
        }
      }
    }
  } else {
    // =============================== team I: W_ih, fc2 + the choice, the environment's bookkeeping ===============================
    const int ti = tid - RNT / 2;
    F3 wi[6];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int c = 0; c < 2; ++c) wi[2 * g + c] = wfrag(a.Wih, H, g * H + 16 * s, 3 * H, H, c, lane);
    const float bias_r = a.bih[u] + a.bhh[u], bias_z = a.bih[H + u] + a.bhh[H + u], bias_n = a.bih[2 * H + u];
    // GI = bias + x W_ih of every row tile from the x planes -> LDS (for the R wave of this slice)
    auto gih = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int rt = 0; rt < RTC; ++rt) {
        f32x4 ag[3] = {splat(bias_r), splat(bias_z), splat(bias_n)};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const F3 xb = bfrag(Xp0 + rt * 16 * HP, HP, rows * HP, c, lane);
#define OP(p_, q_) _Pragma("unroll") for (int g = 0; g < 3; ++g) ag[g] = mm(xb.p_, wi[2 * g + c].q_, ag[g]);
          X6_TERMS(OP)
#undef OP
        }
        f32x4* gp = reinterpret_cast<f32x4*>(GI0) + (rt * 4 + s) * 192 + lane;
        gp[0] = ag[0]; gp[64] = ag[1]; gp[128] = ag[2];
      }
    };
    // env step: lane -> (env, agent); the N rows of an environment sit in ONE wave, environments dealt to the four waves in turn
    const int es_epw = 64 / N, es_er = lane / N;
    const int es_n = lane - es_er * N, es_l0 = es_er * N;
    const int es_el = 4 * es_er + s;
    const bool es_has = es_er < es_epw && es_el < nenv_wg && b0 + es_el < a.E;
    // this thread's observation items (row, 4-column group): item j = ti + 256 j, the same at every step
    int oi_off[NOI], oi_len[NOI], oi_idx[NOI], oi_lds[NOI], oi_row[NOI];
#pragma unroll
    for (int j = 0; j < NOI; ++j) {
      int e = ti + (RNT / 2) * j;
      const bool has = e < vrows * O4;
      if (!has) e = 0;
      const int r = (int)(((float)e + 0.5f) * invO4);
      const int k = 4 * (e - r * O4);
      const int4 mt = rmeta[r];
      oi_off[j] = mt.x + k; oi_len[j] = has ? mt.z : -2;      // (no item: never live, nothing stored)
      oi_idx[j] = mt.w * O + k; oi_lds[j] = r * IP + k; oi_row[j] = r;
    }
    auto gen_obs_items = [&](int t, bool to_lds) __attribute__((always_inline)) {
      const int tNO = t * N * O;
#pragma unroll
      for (int j = 0; j < NOI; ++j) {
        if (oi_len[j] == -2) continue;
        const unsigned po = pfxO[oi_row[j]];
        const unsigned lm = t <= oi_len[j] ? 0xffffffffu : 0u, fm = t < oi_len[j] ? 0xffffffffu : 0u;
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = bits(env_value(po, (unsigned)(oi_idx[j] + i))) & lm;
        *reinterpret_cast<u32x4*>(a.obs + (long)oi_off[j] + tNO) = v;
        if (to_lds) {
          f32x4 w;
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = __builtin_bit_cast(float, v[i] & fm);
          const F3h f = split4(w);
          short* p = In0 + oi_lds[j];
          *reinterpret_cast<i32x2*>(p) = f.h;
          *reinterpret_cast<i32x2*>(p + rows * IP) = f.m;
          *reinterpret_cast<i32x2*>(p + 2 * rows * IP) = f.l;
        }
      }
    };
    float ep_r = 0.f;
    WG_BARRIER();                                  // (team R: slot 0 planes -> fc1, x(0))
    WG_BARRIER();                                  // x(0)
    gih();                                         // GI(0)
    WG_BARRIER();
    ST_DECL(8);
    for (int t = 0; t < T; ++t) {
      const int par = t & 1;
      const float eps = eps_next;
      if (a.eps) { if (t + 1 < T) eps_next = a.eps[t + 1]; }
      else { eps_d = eps_anneal_step(eps_d, a.eps_anneal, a.eps_min); eps_next = (float)eps_d; }
      const unsigned tg = env_tg(a.episode, T, t);
      // ---- P1: the observations of slot t+1 -> record, and (steps that feed the network) -> input planes
      gen_obs_items(t + 1, t + 1 < T);
      ST_MARK(0);
      WG_BARRIER();                                // B1
      ST_MARK(1);
      // ---- P2: q(t) and the choice of this team's row tiles
#pragma unroll
      for (int rt = 0; rt < RTI; ++rt) choose(rt, t, eps);
      ST_MARK(2);
      WG_BARRIER();                                // B2: act(t)
      ST_MARK(3);
      // ---- P3: env step (reward / terminated / padded; fixed-order fp32 sum over agents)
      if (es_has) {
        const int L = elen[es_el];
        const bool live = t < L;
        float term = 0.f;
        if (live) {
          const unsigned pre_ = (pre_r && t > 0) ? pfxS[rows / 2 + (t & 1) * (rows / 4) + es_el]
                                                 : hprefix(a.seed, ST_REWARD, (unsigned)(a.env0 + b0 + es_el), tg);
          term = env_reward_term(pre_, (unsigned)(es_n * A + act[es_el * N + es_n]));
        }
        float acc = 0.f;
        for (int n0 = 0; n0 < N; n0 += 4) {          // four shuffles in flight; the sum stays in agent order
          float v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = __shfl(term, (es_l0 + n0 + k) & 63, 64);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = n0 + k < N ? acc + v[k] : acc;
        }
        if (es_n == 0) {
          const long o = (long)(b0 + es_el) * T + t;
          const float rew = live ? acc * (1.0f / (float)N) : 0.f;
          ep_r = ep_r + rew;
          a.r[o] = rew;
          a.term[o] = live ? (t + 1 >= L ? 1.f : 0.f) : 1.f;
          a.padded[o] = live ? 0.f : 1.f;
        }
      }
      ST_MARK(4);
      WG_BARRIER();                                // B3: x(t+1)
      ST_MARK(5);
      // ---- P4: GI(t+1)
      if (t + 1 < T) gih();
      ST_MARK(6);
      WG_BARRIER();                                // B4
      ST_MARK(7);
    }
    ST_DUMP(8);
    if (a.stats && es_has && es_n == 0) a.stats[b0 + es_el] = ep_r;
  }
}

// LDS bytes of a workgroup of RTC row tiles
static size_t rx6_lds(int rtc, int KI, int A) {
  const size_t rows = 16 * (size_t)rtc, IP = KI + 8;
  return 3 * rows * IP * 2 + 3 * 3 * rows * HP * 2 + (size_t)rtc * 4 * 3 * 1024 + 2 * rows * A * 4 + (size_t)(A + 1) * H * 4 +
         rows * (4 * 4 + 3 * 4 + 4 * 4) + 2 * rows * 16 + 6 * 64 * 16;
}

}  // namespace

ST_DEFINE_SETTER(marl_debug_stamps_rollout_x6_v1)

// shapes the split rollout covers: H = 64, <= 16 actions, observation width a multiple of 4, input width <= 160 (three / five fc1
// chunks: 2s3z- and 3s5z-sized agents), whole environments in at most three row tiles (N <= 48; an environment's agents in one wave)
__attribute__((visibility("hidden"))) int marl_rollout_x6_v1_supported(int N, int O, int A) {
  if (A < 1 || A > 16 || N < 1 || O < 4 || (O & 3)) return 0;
  const int I = O + A + N;
  if (I > 160) return 0;
  const int KI = (I + 31) / 32 * 32;
  if (N > (KI > 96 ? 32 : 48)) return 0;                   // whole environments in at most three (wide inputs: two) row tiles
  return rx6_lds(KI > 96 ? 2 : 3, KI, A) <= 160 * 1024 ? 1 : 0;
}

// environments per workgroup: even rounds of workgroups of up to three row tiles (five fc1 chunks: two - registers)
__attribute__((visibility("hidden"))) int marl_rollout_x6_v1_epw(int E, int N, int KI) {
  const int epw_max = (KI > 96 ? 32 : 48) / N;
  return epw_max < 1 ? 0 : even_rounds_epw(E, epw_max);
}

__attribute__((visibility("hidden"))) int marl_rollout_x6_v1(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed,
                                     unsigned rseed, int env0, int episode, int fixed_len, const float* eps, float* h_out,
                                     float* stats, double eps0, double eps_anneal, double eps_min, int last_action,
                                     int reuse_network, void* stream) {
  if (!rec) return (int)hipErrorInvalidValue;
  const int E = rec->E, N = rec->N, A = rec->A;
  if (E <= 0 || rec->T <= 0) return 0;
  if (!marl_rollout_x6_v1_supported(N, rec->O, A) || (reinterpret_cast<uintptr_t>(rec->obs) & 15)) return (int)hipErrorInvalidValue;
  RX6Args a;
  if (const int e = rollout_args(a, w, rec, seed, rseed, env0, episode, fixed_len, eps, h_out, stats, eps0, eps_anneal, eps_min,
                                 last_action, reuse_network))
    return e;
  a.KI = (a.I + 31) / 32 * 32;
  const int nk1 = a.KI > 96 ? 5 : 3;
  const int epw = marl_rollout_x6_v1_epw(E, N, a.KI);
  if (epw < 1) return (int)hipErrorInvalidValue;
  a.EPW = epw;
  const int rtc = (epw * N + 15) / 16;
  const size_t lds = rx6_lds(rtc, a.KI, A);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  const void* fn;
  if (nk1 == 3) fn = rtc == 1 ? (const void*)synth_rollout_x6_kernel<1, 3> : rtc == 2 ? (const void*)synth_rollout_x6_kernel<2, 3> : (const void*)synth_rollout_x6_kernel<3, 3>;
  else fn = rtc == 1 ? (const void*)synth_rollout_x6_kernel<1, 5> : (const void*)synth_rollout_x6_kernel<2, 5>;
  return launch_rollout(fn, (E + epw - 1) / epw, lds, a, stream);
}
