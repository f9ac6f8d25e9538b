// Whole-rollout persistent kernel for the battle environment: ONE launch plays the reset and all T lock-steps of E environments.
//
// The shape is synth_rollout_kernel's (rollout_fused.hip): a workgroup of RNT threads owns EPW whole environments - EPW N (episode,
// agent) rows in 16 RT tile rows - for the entire episode; agent weights stay in registers / LDS, the hidden state never leaves LDS.
// Phases 1 - 3 (fc1, GRU, fc2) issue the MFMA sequences of synth_rollout_kernel / agent_fwd_kernel in the same order and apply
// agent_fwd_kernel's gate math, so q is bit for bit the T = 1 unroll's, and the choice block is that kernel's (epsilon-greedy lane groups, or the SAMPLE two-phase draw).
// They are carried here and not shared through a header: rollout_fused.hip is the kernel bench.py times and stays byte for byte
// what it was.
//
// What differs is the environment.  The unit state (x, y, hp, shield, cooldown of 2 N units per environment) lives in LDS as
// integers; a lock-step is: decisions from the pre-step state (one thread per unit; damage by integer LDS atomics), then movement,
// landing damage, cooldowns and points (the same thread), then the endings (one thread per environment) - all through battle_env.h's
// functions.  The next observation depends on the actions, so slot t + 1 cannot be generated under the gate MFMAs as the synthetic
// slot is: it sits on the critical path, and all RNT threads generate it, flattened over (environment, 16-byte store) items of the
// three runs of a slot, writing each feature to the record and to the LDS input / availability tile that step t + 1 reads.
#include "synth_rollout.h"
#include "battle_env.h"
#include "policy_rows.h"

namespace {

constexpr int HS = H + MARL_PAD_H;
constexpr int BR_MAX_RT = 8;

struct BattleRollArgs {
  const float *W1, *b1, *Wih, *Whh, *bih, *bhh, *W2, *b2;
  const float* eps;       // unused (always null): the schedule below
  double eps0, eps_anneal, eps_min;   // eps(0) = eps0, eps(t+1) = eps(t) > eps_min ? eps(t) - eps_anneal : eps(t), in fp64, rounded per step
  float* stats;           // [3][E] or null: per episode  sum_t r (fp32, in step order) | won | length
  float *obs, *state, *avail;   // (E,T+1,N,O) (E,T+1,SL >= S) (E,T+1,N,A)
  long SL;
  int* u;                 // (E,T,N)
  float *r, *term, *padded;     // (E,T)
  int *length, *won;      // (E)
  float* h_out;           // (E*N,64) final hidden state or null
  unsigned seed, rseed;
  int env0, episode, fixed_len;
  int E, T, N, O, S, A, I, KC, RT;
  int EPW;                // whole environments per workgroup: EPW*N valid rows in 16*RT tile rows
  int has_act, has_id;
  long R;
  BattleCfg c;
  float scale;            // reward per point
  int* units;             // (E, 2N, BT_F): receives the final unit state
};

template <int AC, bool SAMPLE>
__global__ __launch_bounds__(RNT, 2) void battle_rollout_kernel(BattleRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int team = wave >> 2, ws = wave & 3;
  const int q = lane >> 4, m = lane & 15;
  const int rows = a.RT * 16;
  const int KP = a.KC * 16, KS = KP + MARL_PAD_K;
  const int AS = a.A + 1;
  float* W1s = smem;                                  // [4][KC][64] f32x4
  float* In = W1s + 4 * a.KC * 64 * 4;                // [rows][KS]
  float* Xt = In + rows * KS;                         // [rows][HS]
  float* Ha = Xt + rows * HS;                         // [rows][HS] x2
  float* Hb = Ha + rows * HS;
  float* Qs = Hb + rows * HS;                         // [rows][AS]  q of the current step
  float* Av = Qs + rows * AS;                         // [rows][A]   availability of the current slot
  float* uex = Av + rows * a.A;                       // [2][rows]: explore / pick uniforms of the coming choice
  int* act = reinterpret_cast<int*>(uex + 2 * rows);  // [rows]
  int* rowe = act + rows;                             // [rows]: local env index
  int* rown = rowe + rows;                            // [rows]: n
  int* elen = rown + rows;                            // [rows / N ..]: episode length of the local env so far (T while it runs)
  int* pts = elen + rows;                             // [rows / N ..]: points of the step
  int* upm = pts + rows;                              // [rows / N ..]: bit 0 an ally stands, bit 1 an enemy stands
  int* dmg = upm + rows;                              // [2 rows]: damage landing on each unit this step
  int* un = dmg + 2 * rows;                           // [2 rows][BT_F]: the unit state

  const BattleCfg& c = a.c;
  const int T = a.T, N = a.N, O = a.O, S = a.S, A = a.A, NU = c.N + c.M;
  const int b0 = blockIdx.x * a.EPW;
  const int nenv = a.E - b0 < a.EPW ? a.E - b0 : a.EPW;    // the last workgroup may hold fewer
  const int vrows = nenv * N;                          // valid rows; rows vrows .. 16 RT - 1 are padding (zero input)
  const long row0 = (long)b0 * N;
  for (int r = tid; r < rows; r += RNT) {
    const int rr = r < vrows ? r : vrows - 1;
    rowe[r] = rr / N;
    rown[r] = rr % N;
  }
  for (int e = tid; e < rows * H; e += RNT) Ha[(e / H) * HS + (e % H)] = 0.f;     // init_hidden: zeros
  // the input tile: zeros (observation and one-hot(last action) columns, padding rows and columns), the agent id
  for (int e = tid; e < rows * KS; e += RNT) {
    const int r = e / KS, k = e - r * KS;
    float v = 0.f;
    if (a.has_id && r < vrows && k >= a.I - N && k < a.I) v = (r % N == k - (a.I - N)) ? 1.f : 0.f;
    In[e] = v;
  }
  // reset: the start positions, full hp / shield
  for (int k = tid; k < nenv * NU; k += RNT) {
    const int el = k / NU;
    bt_start(c, a.seed, (unsigned)(a.env0 + b0 + el), a.episode, k - el * NU, un + k * BT_F);
    dmg[k] = 0;
  }
  for (int el = tid; el < nenv; el += RNT) { elen[el] = T; pts[el] = 0; upm[el] = 0; }
  __syncthreads();

  // ---- slot `slot` of every environment from the unit state -> the record and the LDS tiles of the step that reads it.
  // A slot is three contiguous runs per environment (N O observation floats, S state floats, N A availability floats) that start
  // on any 4-byte boundary; a run is [scalars up to the first 16-byte boundary | f32x4 body | scalars after], at most n / 4 + 2
  // items, and the threads take (environment, item) pairs.  A slot after the episode's end is zeros; slot `length` is the final
  // observation.  actp: the step's recorded actions (the state's last columns), or null at the reset
  const int Qo = ((N * O) >> 2) + 2, Qst = (S >> 2) + 2, Qa = ((N * A) >> 2) + 2, Qt = Qo + Qst + Qa;
  auto gen_slot = [&](int slot, const int* actp) {
    for (int e = tid; e < nenv * Qt; e += RNT) {
      const int el = e / Qt;
      int j = e - el * Qt;
      const bool live = slot <= elen[el];              // (the step's ending may be landing in elen now: either value says the same)
      const long row = (long)(b0 + el) * (T + 1) + slot;
      const int* une = un + el * NU * BT_F;
      const int* ae = actp ? actp + el * N : nullptr;
      int kind = 0, n = N * O;
      float* p = a.obs + row * N * O;
      if (j >= Qo + Qst) { j -= Qo + Qst; kind = 2; n = N * A; p = a.avail + row * N * A; }
      else if (j >= Qo) { j -= Qo; kind = 1; n = S; p = a.state + row * a.SL; }
      int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
      if (head > n) head = n;
      const int body = (n - head) >> 2;
      int k0, cnt;
      if (j == 0) { k0 = 0; cnt = head; }
      else if (j - 1 < body) { k0 = head + 4 * (j - 1); cnt = 4; }
      else if (j - 1 == body) { k0 = head + 4 * body; cnt = n - k0; }
      else continue;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= cnt) continue;
        const int k = k0 + i;
        float x;
        if (kind == 0) {
          const int ag = k / O, col = k - ag * O;
          x = live ? bt_obs(c, une, ag, col) : 0.f;
          In[(el * N + ag) * KS + col] = x;
        } else if (kind == 1) {
          x = live ? bt_state(c, une, ae, k) : 0.f;
        } else {
          const int ag = k / A, col = k - ag * A;
          x = live && bt_avail(c, une, ag, col) ? 1.f : 0.f;
          Av[(el * N + ag) * A + col] = x;
        }
        v[i] = x;
      }
      if (cnt == 4) {
        *reinterpret_cast<f32x4*>(p + k0) = v;
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (i < cnt) p[k0 + i] = v[i];
      }
    }
  };
  gen_slot(0, nullptr);
  if (tid < rows) {       // uniforms of the first choice
    const unsigned env = (unsigned)(a.env0 + b0 + rowe[tid]), tg0 = env_tg(a.episode, T, 0);
    if constexpr (SAMPLE) {      // one uniform per (env, agent, step): the policy's draw; uex[rows + r] stays unused
      uex[tid] = u01(hkey(a.rseed, ST_SAMPLE, env, tg0, (unsigned)rown[tid]));
    } else {
      uex[tid] = u01(hkey(a.rseed, ST_EXPLORE, env, tg0, (unsigned)rown[tid]));
      uex[rows + tid] = u01(hkey(a.rseed, ST_PICK, env, tg0, (unsigned)rown[tid]));
    }
  }

  // ---- weights (as in agent_fwd_kernel)
  f32x4 wih[3][4], whh[3][4], w2[AC][4];
  float bias_r, bias_z, bias_in, bias_hn, bias1, bias2[AC];
  const int j = 16 * ws + m;
  {
    if (team == 0) {
      for (int cc = 0; cc < a.KC; ++cc) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int k = 16 * cc + 4 * q + i;
          v[i] = k < a.I ? a.W1[(long)j * a.I + k] : 0.f;
        }
        *reinterpret_cast<f32x4*>(W1s + ((ws * a.KC + cc) * 64 + lane) * 4) = v;
      }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        wih[g][cc] = *reinterpret_cast<const f32x4*>(a.Wih + (long)(g * H + j) * H + 16 * cc + 4 * q);
        whh[g][cc] = *reinterpret_cast<const f32x4*>(a.Whh + (long)(g * H + j) * H + 16 * cc + 4 * q);
      }
#pragma unroll
    for (int ac = 0; ac < AC; ++ac) {
      int arow = 16 * ac + m; if (arow >= A) arow = A - 1;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
        w2[ac][cc] = *reinterpret_cast<const f32x4*>(a.W2 + (long)arow * H + 16 * cc + 4 * q);
      bias2[ac] = a.b2[arow];
    }
    bias1 = a.b1[j];
    bias_r = a.bih[j] + a.bhh[j];
    bias_z = a.bih[H + j] + a.bhh[H + j];
    bias_in = a.bih[2 * H + j];
    bias_hn = a.bhh[2 * H + j];
    // the gate math is agent_fwd_kernel's, by AC as there (pre-scaled accumulators with two action tiles, the plain form with one):
    // h and q are then the T = 1 unroll's bit for bit.  (synth_rollout_kernel pre-scales always; its record only has to agree with
    // the per-step path's in the argmax.  Here the next observation depends on the action, so q is held equal itself.)
    if (AC == 2) gru_prescale(wih, whh, bias_r, bias_z, bias_in, bias_hn);
  }
  WG_BARRIER();

  float* Hp = Ha;
  float* Hn = Hb;
  // this thread's unit (threads 0 .. nenv NU - 1) and environment (threads 0 .. nenv - 1)
  const bool has_unit = tid < nenv * NU;
  const int un_el = has_unit ? tid / NU : 0, un_j = has_unit ? tid - un_el * NU : 0;
  const int un_type = bt_type(c, un_j);
  float ep_r = 0.f;                                // episode reward of this thread's environment
  int ep_won = 0;
  float eps_next = (float)a.eps0;
  double eps_d = a.eps0;
  ST_DECL(14);
  for (int t = 0; t < T; ++t) {
    const float eps = eps_next;
    eps_d = eps_anneal_step(eps_d, a.eps_anneal, a.eps_min);
    eps_next = (float)eps_d;
    // ---------------- phase 1: x = relu(fc1(in))
    for (int rt = team; rt < a.RT; rt += 4) {
      const bool two = rt + 2 < a.RT;
      f32x4 acc0 = {bias1, bias1, bias1, bias1}, acc1 = acc0;
      const float* in0 = In + (rt * 16 + m) * KS + 4 * q;
      const float* in1 = in0 + 32 * KS;
      const float* wf = W1s + (ws * a.KC * 64 + lane) * 4;
#define FC1_LD(B_, A0_, A1_, c_)                                                  \
      B_ = *reinterpret_cast<const f32x4*>(wf + (c_) * 256);                      \
      A0_ = *reinterpret_cast<const f32x4*>(in0 + 16 * (c_));                     \
      if (two) A1_ = *reinterpret_cast<const f32x4*>(in1 + 16 * (c_));
      f32x4 bA, aA, a1A = acc0, bB, aB, a1B = acc0;
      FC1_LD(bA, aA, a1A, 0)
      for (int cc = 0; cc < a.KC; cc += 2) {
        const bool odd = cc + 1 < a.KC;
        const int cB = odd ? cc + 1 : cc, cA = cc + 2 < a.KC ? cc + 2 : cc;
        FC1_LD(bB, aB, a1B, cB)
        if (two) mfma16x4_il2(aA, bA, acc0, a1A, bA, acc1);
        else acc0 = mfma16x4(aA, bA, acc0);
        FC1_LD(bA, aA, a1A, cA)
        if (odd) {
          if (two) mfma16x4_il2(aB, bB, acc0, a1B, bB, acc1);
          else acc0 = mfma16x4(aB, bB, acc0);
        }
      }
#undef FC1_LD
      const int r0 = rt * 16 + 4 * q;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Xt[(r0 + i) * HS + j] = fmaxf(acc0[i], 0.f);
        if (two) Xt[(r0 + 32 + i) * HS + j] = fmaxf(acc1[i], 0.f);
      }
    }
    ST_MARK(0);
    WG_BARRIER();
    ST_MARK(1);
    // ---------------- phase 2: GRU; the two waves of a hidden-unit slice (one per team) take alternate row tiles
    for (int rt = team; rt < a.RT; rt += 2) {
      f32x4 ar = {bias_r, bias_r, bias_r, bias_r};
      f32x4 az = {bias_z, bias_z, bias_z, bias_z};
      f32x4 ain = {bias_in, bias_in, bias_in, bias_in};
      f32x4 ahn = {bias_hn, bias_hn, bias_hn, bias_hn};
      const float* xr = Xt + (rt * 16 + m) * HS + 4 * q;
      const float* hr = Hp + (rt * 16 + m) * HS + 4 * q;
      // input-side products first, hidden-side products after them (the SAME order in every GRU kernel)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        f32x4 ax = *reinterpret_cast<const f32x4*>(xr + 16 * cc);
        mfma16x4_il3(ax, wih[0][cc], ar, ax, wih[1][cc], az, ax, wih[2][cc], ain);
      }
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        f32x4 ah = *reinterpret_cast<const f32x4*>(hr + 16 * cc);
        mfma16x4_il3(ah, whh[2][cc], ahn, ah, whh[0][cc], ar, ah, whh[1][cc], az);
      }
      const int r0 = rt * 16 + 4 * q;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hp = Hp[(r0 + i) * HS + j];
        float rg, zg, ng, hv;
        if (AC == 2) gru_point(ar[i], az[i], ain[i], ahn[i], hp, rg, zg, ng, hv);
        else gru_point_plain(ar[i], az[i], ain[i], ahn[i], hp, rg, zg, ng, hv);
        Hn[(r0 + i) * HS + j] = hv;
      }
    }
    ST_MARK(2);
    WG_BARRIER();
    ST_MARK(3);
    // ---------------- phase 3: q = fc2(h') -> LDS
    for (int rt = wave; rt < a.RT; rt += 8) {
      f32x4 acc[AC];
#pragma unroll
      for (int ac = 0; ac < AC; ++ac) acc[ac] = (f32x4){bias2[ac], bias2[ac], bias2[ac], bias2[ac]};
      const float* hr = Hn + (rt * 16 + m) * HS + 4 * q;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        f32x4 ah = *reinterpret_cast<const f32x4*>(hr + 16 * cc);
#pragma unroll
        for (int ac = 0; ac < AC; ++ac) acc[ac] = mfma16x4(ah, w2[ac][cc], acc[ac]);
      }
#pragma unroll
      for (int ac = 0; ac < AC; ++ac) {
        const int col = 16 * ac + m;
        if (col < A) {
#pragma unroll
          for (int i = 0; i < 4; ++i) Qs[(rt * 16 + 4 * q + i) * AS + col] = acc[ac][i];
        }
      }
    }
    ST_MARK(4);
    WG_BARRIER();
    ST_MARK(5);
    // ---------------- the choice (rollout_fused.hip's block): 16 AC lanes per (env, agent) row, lane = action; first-index argmax
    // over the available actions by a lane-group max + ballot, the explored action is the kk-th set bit of the availability mask.
    // SAMPLE: a draw from the row's stochastic policy in two phases
    const unsigned tg = env_tg(a.episode, T, t);
    {
      constexpr int LG = 16 * AC;
      constexpr unsigned GM = LG == 32 ? 0xffffffffu : ((1u << LG) - 1u);
      const int gl = lane & (LG - 1), sh = lane & ~(LG - 1);
      if constexpr (SAMPLE) {
        constexpr int G = 64 / LG;                      // rows of one pass of a wave
        // phase A: the row's max over the available actions (order-free) and each lane's e_k = exp(min(z_k - mx, 80)), written
        // over the row in Qs, which nothing reads after the choice
        for (int base = wave * G; base < vrows; base += (RNT / 64) * G) {
          const int r = base + lane / LG;
          const bool valid = r < vrows;
          const int rr = valid ? r : vrows - 1;
          const int gk = gl < A ? gl : 0;
          const float z = Qs[rr * AS + gk];
          const bool on = gl < A && Av[rr * A + gk] != 0.f;
          float mx = group_max16(on ? z : -3.0e38f);
          if (LG == 32) mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
          const float ek = expf(fminf(z - mx, EXP_CLAMP));
          if (valid && gl < A) Qs[r * AS + gl] = ek;       // (a padding group would write over the row it duplicates)
        }
        __builtin_amdgcn_wave_barrier();
        // phase B, one lane per row, once for all rows this wave handled in phase A (lane l: row l % G of pass l / G; a wave's LDS
        // accesses complete in order, so no workgroup barrier): the sums and the walk keep index order, as row_policy and
        // row_sample do
        {
          const int r = (wave + (RNT / 64) * (lane / G)) * G + lane % G;
          if (r < vrows) {
            const int el = rowe[r], n = rown[r];
            const RowPolicy p = row_policy_e(Qs + r * AS, Av + r * A, A, eps);
            int arg = row_walk<true>(p, Qs + r * AS, Av + r * A, A, uex[r]);
            if (!(t < elen[el])) arg = -1;
            act[r] = arg;
            a.u[((long)(b0 + el) * T + t) * N + n] = arg;
          }
        }
        __builtin_amdgcn_wave_barrier();
        if (a.has_act) {                                   // one-hot fed to step t+1, phase A's mapping again
          for (int base = wave * G; base < vrows; base += (RNT / 64) * G) {
            const int r = base + lane / LG;
            if (r < vrows && gl < A) In[r * KS + O + gl] = (gl == act[r]) ? 1.f : 0.f;
          }
        }
      } else {
        for (int base = wave * (64 / LG); base < vrows; base += (RNT / 64) * (64 / LG)) {
          const int r = base + lane / LG;
          const bool valid = r < vrows;
          const int rr = valid ? r : vrows - 1;
          const int el = rowe[rr], n = rown[rr];
          const bool on = gl < A && Av[rr * A + (gl < A ? gl : 0)] != 0.f;
          const float v = on ? Qs[rr * AS + gl] : -3.0e38f;
          float mx = group_max16(v);
          if (LG == 32) mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
          const unsigned am = (unsigned)(__ballot(on) >> sh) & GM;
          const unsigned em = (unsigned)(__ballot(on && v == mx) >> sh) & GM;
          const int navail = __popc(am);
          int arg = em ? __ffs(em) - 1 : (am ? __ffs(am) - 1 : 0);
          const bool explore = uex[rr] < eps;
          int kk;
          env_pick(uex[rows + rr], navail, kk);
          const bool sel = explore && on && __popc(am & ((1u << gl) - 1u)) == kk;
          const unsigned sm = (unsigned)(__ballot(sel) >> sh) & GM;
          if (sm) arg = __ffs(sm) - 1;
          if (!(t < elen[el])) arg = -1;
          if (valid) {
            if (gl == 0) {
              act[r] = arg;
              a.u[((long)(b0 + el) * T + t) * N + n] = arg;
            }
            if (a.has_act && gl < A) In[r * KS + O + gl] = (gl == arg) ? 1.f : 0.f;      // one-hot fed to step t+1
          }
        }
      }
    }
    ST_MARK(6);
    WG_BARRIER();
    ST_MARK(7);
    // ---------------- the battle step.  1. every unit's action, from the pre-step state; the two last waves (a unit never sits
    // there: 2 EPW N <= 256) hash the uniforms of the NEXT step's choice
    if (tid >= RNT - 128 && tid - (RNT - 128) < rows) {
      const int r = tid - (RNT - 128);
      const unsigned env = (unsigned)(a.env0 + b0 + rowe[r]), nn_ = (unsigned)rown[r];
      if constexpr (SAMPLE) {
        uex[r] = u01(hkey(a.rseed, ST_SAMPLE, env, tg + 1u, nn_));
      } else {
        uex[r] = u01(hkey(a.rseed, ST_EXPLORE, env, tg + 1u, nn_));
        uex[rows + r] = u01(hkey(a.rseed, ST_PICK, env, tg + 1u, nn_));
      }
    }
    int dx = 0, dy = 0, target = -1;
    const bool un_live = has_unit && t < elen[un_el];
    int* une = un + un_el * NU * BT_F;
    if (un_live) {
      if (un_j < N) bt_ally_decide(c, une, un_j, act[un_el * N + un_j], dx, dy, target);
      else bt_enemy_decide(c, une, un_j - N, dx, dy, target);
      if (target >= 0) atomicAdd(&dmg[un_el * NU + target], bt_damage(un_type));
    }
    ST_MARK(8);
    WG_BARRIER();
    ST_MARK(9);
    // 2. - 4. movers move, damage lands (a unit killed this step has dealt its own), cooldowns
    if (un_live) {
      int* me = une + un_j * BT_F;
      int hp = me[BT_HP], shd = me[BT_SH];
      const int hp0 = hp, cd = me[BT_CD];
      me[BT_X] += dx; me[BT_Y] += dy;
      const int removed = bt_hit(dmg[tid], hp, shd);
      dmg[tid] = 0;
      me[BT_HP] = hp; me[BT_SH] = shd;
      me[BT_CD] = target >= 0 ? bt_cooldown(un_type) : (cd > 0 ? cd - 1 : 0);
      if (un_j >= N && removed > 0) atomicAdd(&pts[un_el], removed + (hp0 > 0 && hp <= 0 ? BT_KILL : 0));
      if (hp > 0) atomicOr(&upm[un_el], un_j < N ? 1 : 2);
    }
    ST_MARK(10);
    WG_BARRIER();
    ST_MARK(11);
    // the endings, one thread per environment, beside slot t + 1: the final observation at the terminating step, zeros after
    if (tid < nenv) {
      const bool live = t < elen[tid];
      const bool allies = (upm[tid] & 1) != 0, enemies = (upm[tid] & 2) != 0;
      const bool win = live && !enemies && allies;
      const bool over = !live || !enemies || !allies || t + 1 == T;
      const long o = (long)(b0 + tid) * T + t;
      const float rew = live ? (float)(pts[tid] + (win ? BT_WIN : 0)) * a.scale : 0.f;
      ep_r = ep_r + rew;
      a.r[o] = rew;
      a.term[o] = over ? 1.f : 0.f;
      a.padded[o] = live ? 0.f : 1.f;
      if (live && over) { elen[tid] = t + 1; ep_won = win ? 1 : 0; }
      pts[tid] = 0; upm[tid] = 0;
    }
    gen_slot(t + 1, act);
    float* tmp = Hp; Hp = Hn; Hn = tmp;
    ST_MARK(12);
    WG_BARRIER();
    ST_MARK(13);
  }
  ST_DUMP(14);
  if (tid < nenv) {
    const int b = b0 + tid;
    a.length[b] = elen[tid];
    a.won[b] = ep_won;
    if (a.stats) { a.stats[b] = ep_r; a.stats[a.E + b] = (float)ep_won; a.stats[2L * a.E + b] = (float)elen[tid]; }
  }
  for (int k = tid; k < nenv * NU * BT_F; k += RNT) a.units[(long)b0 * NU * BT_F + k] = un[k];
  if (a.h_out) {
    for (int e = tid; e < vrows * H; e += RNT) {
      const int r = e / H, k = e % H;
      a.h_out[(row0 + r) * H + k] = Hp[r * HS + k];
    }
  }
}

}  // namespace

ST_DEFINE_SETTER(marl_debug_stamps_battle)

// LDS bytes of a workgroup of rt row tiles of width-I inputs: the fc1 slice + the row state + the unit state of the rows' environments
static size_t battle_lds(int I, int A, int rt) {
  const int KC = (I + 15) / 16, KS = KC * 16 + MARL_PAD_K;
  const size_t fixed = (size_t)4 * KC * 64 * 16;
  const size_t per_row = (size_t)(KS + 3 * HS + (A + 1) + A + 2) * 4 + 6 * 4 + 2 * 4 + 2 * BT_F * 4;
  return fixed + per_row * 16 * rt;
}
static int battle_max_rt(int I, int A) {
  int rt = 0;
  for (int c = 1; c <= BR_MAX_RT; ++c) if (battle_lds(I, A, c) <= 160 * 1024) rt = c;
  return rt;
}
// workgroups | environments per workgroup | row tiles | LDS bytes; false: no plan places the shape
static bool battle_plan(int E, int N, int O, int A, int last_action, int reuse_network, int plan[4]) {
  if (!bt_supported(N, N, A) || O < 1 || E < 1) return false;
  const int I = O + (last_action ? A : 0) + (reuse_network ? N : 0);
  const int rt_max = battle_max_rt(I, A);
  if (16 * rt_max < N) return false;
  // one workgroup per CU while the batch allows it (a lock-step is latency bound), capped by the row tiles the LDS holds
  int epw = (E + 255) / 256;
  if (epw * N > 16 * rt_max) epw = (16 * rt_max) / N;
  plan[0] = (E + epw - 1) / epw;
  plan[1] = epw;
  plan[2] = (epw * N + 15) / 16;
  plan[3] = (int)battle_lds(I, A, plan[2]);
  return true;
}

extern "C" int marl_battle_rollout_supported(int N, int O, int A) {
  int plan[4];
  return battle_plan(1, N, O, A, 1, 1, plan) ? 1 : 0;      // the widest input: last action and agent id appended
}

extern "C" int marl_battle_rollout_plan(int E, int N, int O, int A, int last_action, int reuse_network, int* plan) {
  return battle_plan(E, N, O, A, last_action, reuse_network, plan) ? 0 : (int)hipErrorInvalidValue;
}

template <bool SAMPLE>
static int battle_rollout(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0, int episode,
                          unsigned types, int shield, int type_bits, float scale, int* units, float* h_out, float* stats,
                          double eps0, double eps_anneal, double eps_min, int M, int last_action, int reuse_network, void* stream) {
  if (!rec) return (int)hipErrorInvalidValue;
  BattleRollArgs a;
  const int bad = battle_cfg(rec->N, M, rec->A, shield, type_bits, types, rec->state_ld, rec->T, a.c);
  if (bad) return bad;
  if (rec->O != a.c.O || rec->S != a.c.S) return (int)hipErrorInvalidValue;      // the widths the map derives
  if (rec->E <= 0) return 0;
  int plan[4];
  if (!battle_plan(rec->E, rec->N, rec->O, rec->A, last_action, reuse_network, plan)) return (int)hipErrorInvalidValue;
  if (const int e = rollout_args(a, w, rec, seed, rseed, env0, episode, 0, nullptr, h_out, stats, eps0, eps_anneal, eps_min, last_action,
                                 reuse_network))
    return e;
  a.KC = (a.I + 15) / 16;
  a.EPW = plan[1];
  a.RT = plan[2];
  a.scale = scale;
  a.units = units;
  return launch_rollout(rec->A <= 16 ? (const void*)battle_rollout_kernel<1, SAMPLE> : (const void*)battle_rollout_kernel<2, SAMPLE>,
                        plan[0], (size_t)plan[3], a, stream);
}

extern "C" int marl_battle_rollout(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                                   int episode, unsigned types, int shield, int type_bits, float scale, int* units, float* h_out,
                                   float* stats, double eps0, double eps_anneal, double eps_min, int M, int last_action,
                                   int reuse_network, void* stream) {
  return battle_rollout<false>(w, rec, seed, rseed, env0, episode, types, shield, type_bits, scale, units, h_out, stats, eps0,
                               eps_anneal, eps_min, M, last_action, reuse_network, stream);
}

extern "C" int marl_battle_rollout_sample(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed,
                                          int env0, int episode, unsigned types, int shield, int type_bits, float scale, int* units,
                                          float* h_out, float* stats, double eps0, double eps_anneal, double eps_min, int M,
                                          int last_action, int reuse_network, void* stream) {
  return battle_rollout<true>(w, rec, seed, rseed, env0, episode, types, shield, type_bits, scale, units, h_out, stats, eps0,
                              eps_anneal, eps_min, M, last_action, reuse_network, stream);
}
