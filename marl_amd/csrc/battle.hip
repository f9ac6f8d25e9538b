// The battle environment's per-step kernels (rules: battle_env.h): reset, one launch per lock-step that applies the step and writes
// slot t + 1 of the record, and the same launch with the action choice in front (the whole rollout in one launch: battle_rollout.hip).  A wave per environment, BT_WPB environments per workgroup; the units sit on lanes 0 .. N + M - 1 for the
// dynamics (the unit state of the workgroup's environments lives in LDS), damage and points are integer LDS atomics (any order gives
// the same sum), then all 64 lanes write the slot's N O + S + N A floats as three contiguous runs, 16 bytes a lane where a run's
// address allows (a run starts on any 4-byte boundary: N O is 90 floats on 3m).
#include "battle_env.h"
#include "env_slot.h"
#include "../../include/marl_hip.h"

namespace {
constexpr int BT_WPB = 4;                       // environments (waves) per workgroup
constexpr int BT_UNITS = 2 * BT_MAX_SIDE;

// slot `slot` of environment e from the unit state un (LDS); act: the step's recorded actions (LDS) or NULL; !live: zeros
__device__ __forceinline__ void write_slot(const BattleCfg& c, const int* un, const int* act, bool live, float* obs, float* state,
                                           long SL, float* avail, long e, int T, int slot, int lane) {
  const long row = e * (T + 1) + slot;
  const int O = c.O, A = c.A;
  write_run(obs + row * c.N * O, c.N * O, lane, [&](int k) { const int i = k / O; return live ? bt_obs(c, un, i, k - i * O) : 0.f; });
  write_run(state + row * SL, c.S, lane, [&](int k) { return live ? bt_state(c, un, act, k) : 0.f; });
  write_run(avail + row * c.N * A, c.N * A, lane,
            [&](int k) { const int i = k / A; return live && bt_avail(c, un, i, k - i * A) ? 1.f : 0.f; });
}

__global__ __launch_bounds__(BT_WPB * MARL_WAVE) void battle_reset_kernel(BattleCfg c, unsigned seed, int env0, int episode, int* units,
                                                                         int* length, int* won, float* obs, float* state, long SL,
                                                                         float* avail, int E, int T) {
  __shared__ int s_un[BT_WPB][BT_UNITS * BT_F];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * BT_WPB + w;
  const bool valid = e < E;
  const int NU = c.N + c.M;
  if (valid && lane < NU) {
    int* un = s_un[w] + lane * BT_F;
    bt_start(c, seed, (unsigned)(env0 + (int)e), episode, lane, un);
    for (int f = 0; f < BT_F; ++f) units[(e * NU + lane) * BT_F + f] = un[f];
  }
  if (valid && lane == 0) { length[e] = T; won[e] = 0; }
  __syncthreads();
  if (valid) write_slot(c, s_un[w], nullptr, true, obs, state, SL, avail, e, T, 0, lane);
}

// The shared memory of a step: the unit state of the workgroup's environments (pre-step, then post-step), the damage and points
// accumulators and the step's recorded actions
struct BattleStepLds {
  int un[BT_WPB][BT_UNITS * BT_F];
  int dmg[BT_WPB][BT_UNITS];
  int act[BT_WPB][BT_MAX_SIDE];
  int pts[BT_WPB];
};

// Lock-step t of environment e by its wave (every thread of the workgroup calls this: it holds workgroup barriers).  a: the action of
// ally `lane` as given (lanes < N of a live environment; anything elsewhere); live: t < length[e] as read before the step
__device__ __forceinline__ void battle_step_body(const BattleCfg& c, BattleStepLds& s, float scale, int t, int a, bool valid, bool live,
                                                 long e, int w, int lane, int* units, int* u, float* r, float* term, float* padded,
                                                 int* length, int* won, int* alive_next, float* obs, float* state, long SL,
                                                 float* avail, int T) {
  const int N = c.N, NU = c.N + c.M;
  const bool unit = valid && lane < NU;
  int me[BT_F] = {0, 0, 0, 0, 0};
  if (unit) {
    for (int f = 0; f < BT_F; ++f) s.un[w][lane * BT_F + f] = me[f] = units[(e * NU + lane) * BT_F + f];
    s.dmg[w][lane] = 0;
  }
  if (valid && lane < N) {
    a = live ? a : -1;                                // the record keeps the action as given
    s.act[w][lane] = a;
    u[(e * T + t) * N + lane] = a;
  }
  if (lane == 0) s.pts[w] = 0;
  __syncthreads();
  // 1. every unit's action, from the pre-step state
  int dx = 0, dy = 0, target = -1;
  const int type = unit ? bt_type(c, lane) : 0;
  if (live && unit) {
    if (lane < N) bt_ally_decide(c, s.un[w], lane, s.act[w][lane], dx, dy, target);
    else bt_enemy_decide(c, s.un[w], lane - N, dx, dy, target);
    if (target >= 0) atomicAdd(&s.dmg[w][target], bt_damage(type));
  }
  __syncthreads();
  // 2. - 4. movers move, damage lands (a unit killed this step has dealt its own), cooldowns
  if (live && unit) {
    const int hp0 = me[BT_HP];
    me[BT_X] += dx; me[BT_Y] += dy;
    const int removed = bt_hit(s.dmg[w][lane], me[BT_HP], me[BT_SH]);
    me[BT_CD] = target >= 0 ? bt_cooldown(type) : (me[BT_CD] > 0 ? me[BT_CD] - 1 : 0);
    if (lane >= N && removed > 0) atomicAdd(&s.pts[w], removed + (hp0 > 0 && me[BT_HP] <= 0 ? BT_KILL : 0));
    for (int f = 0; f < BT_F; ++f) {
      s.un[w][lane * BT_F + f] = me[f];
      units[(e * NU + lane) * BT_F + f] = me[f];
    }
  }
  const unsigned long long up = __ballot(unit && me[BT_HP] > 0);
  const bool allies = (up & ((1ull << N) - 1ull)) != 0ull, enemies = (up >> N) != 0ull;
  __syncthreads();
  if (valid && lane == 0) {
    const bool win = live && !enemies && allies;
    const bool over = !live || !enemies || !allies || t + 1 == T;
    r[e * T + t] = live ? (float)(s.pts[w] + (win ? BT_WIN : 0)) * scale : 0.f;
    term[e * T + t] = over ? 1.f : 0.f;
    padded[e * T + t] = live ? 0.f : 1.f;
    if (live && over) { length[e] = t + 1; won[e] = win ? 1 : 0; }
    if (alive_next) alive_next[e] = over ? 0 : 1;
  }
  // slot t + 1: the final observation at the terminating step, zeros after
  if (valid) write_slot(c, s.un[w], s.act[w], live, obs, state, SL, avail, e, T, t + 1, lane);
}

__global__ __launch_bounds__(BT_WPB * MARL_WAVE) void battle_step_kernel(BattleCfg c, float scale, int t, const int* act, int* units,
                                                                        int* u, float* r, float* term, float* padded, int* length,
                                                                        int* won, int* alive_next, float* obs, float* state, long SL,
                                                                        float* avail, int E, int T) {
  __shared__ BattleStepLds s;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * BT_WPB + w;
  const bool valid = e < E;
  const bool live = valid && t < length[e];          // an episode that ended at step t' has length t' + 1 <= t
  const int a = live && lane < c.N ? act[e * c.N + lane] : -1;
  battle_step_body(c, s, scale, t, a, valid, live, e, w, lane, units, u, r, term, padded, length, won, alive_next, obs, state, SL,
                   avail, T);
}

// The action choice and the step in one launch: ally lane n of a live environment chooses from its row of q (E,1,N,A) and slot t's
// availability in the record - select_kernel's epsilon-greedy rule and draws (rollout.hip), or with SAMPLE policy_sample's draw from
// the stochastic policy of the row (policy_rows.h) - keyed by (rseed, env0 + e, env_tg(episode, T, t), n); then battle_step_body
template <bool SAMPLE>
__global__ __launch_bounds__(BT_WPB * MARL_WAVE) void battle_fused_step_kernel(BattleCfg c, float scale, unsigned rseed, int env0,
                                                                              int episode, int t, float eps, const float* q,
                                                                              int* units, int* u, float* r, float* term, float* padded,
                                                                              int* length, int* won, float* obs, float* state, long SL,
                                                                              float* avail, int E, int T) {
  __shared__ BattleStepLds s;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * BT_WPB + w;
  const bool valid = e < E;
  const bool live = valid && t < length[e];
  const int N = c.N, A = c.A;
  int arg = -1;
  if (live && lane < N)
    arg = env_choose<SAMPLE>(q + (e * N + lane) * A, avail + ((e * (T + 1) + t) * N + lane) * A, A, eps, rseed,
                             (unsigned)(env0 + (int)e), env_tg(episode, T, t), lane);
  battle_step_body(c, s, scale, t, arg, valid, live, e, w, lane, units, u, r, term, padded, length, won, nullptr, obs, state, SL,
                   avail, T);
}

}  // namespace

extern "C" int marl_battle_supported(int n_allies, int n_enemies, int A) { return bt_supported(n_allies, n_enemies, A) ? 1 : 0; }

// every launcher's checks, in this order: a record, battle_cfg's refusals, the widths the record states against the ones the map
// derives, lock-step t (reset: 0) inside the episode
static int battle_record_cfg(const marl_record_t* rec, int M, unsigned types, int shield, int type_bits, int t, BattleCfg& cfg) {
  if (!rec) return (int)hipErrorInvalidValue;
  const int bad = battle_cfg(rec->N, M, rec->A, shield, type_bits, types, rec->state_ld, rec->T, cfg);
  if (bad) return bad;
  return rec->O != cfg.O || rec->S != cfg.S || t < 0 || t >= rec->T ? (int)hipErrorInvalidValue : 0;
}

extern "C" int marl_battle_reset(unsigned seed, int env0, int episode, unsigned types, int shield, int type_bits, int* units,
                                 const marl_record_t* rec, int M, void* stream) {
  BattleCfg cfg;
  const int bad = battle_record_cfg(rec, M, types, shield, type_bits, 0, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(battle_reset_kernel, dim3((rec->E + BT_WPB - 1) / BT_WPB), dim3(BT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, seed,
                     env0, episode, units, rec->length, rec->won, rec->obs, rec->state, rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_battle_step(unsigned types, int shield, int type_bits, float scale, int t, const int* act, int* units,
                                const marl_record_t* rec, int* alive_next, int M, void* stream) {
  BattleCfg cfg;
  const int bad = battle_record_cfg(rec, M, types, shield, type_bits, t, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(battle_step_kernel, dim3((rec->E + BT_WPB - 1) / BT_WPB), dim3(BT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, scale,
                     t, act, units, rec->u, rec->r, rec->term, rec->padded, rec->length, rec->won, alive_next, rec->obs, rec->state,
                     rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

template <bool SAMPLE>
static int battle_fused_step(unsigned types, int shield, int type_bits, float scale, unsigned rseed, int env0, int episode, int t,
                             float eps, const float* q, int* units, const marl_record_t* rec, int M, void* stream) {
  BattleCfg cfg;
  const int bad = battle_record_cfg(rec, M, types, shield, type_bits, t, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(battle_fused_step_kernel<SAMPLE>, dim3((rec->E + BT_WPB - 1) / BT_WPB), dim3(BT_WPB * MARL_WAVE), 0,
                     (hipStream_t)stream, cfg, scale, rseed, env0, episode, t, eps, q, units, rec->u, rec->r, rec->term, rec->padded,
                     rec->length, rec->won, rec->obs, rec->state, rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_battle_fused_step(unsigned types, int shield, int type_bits, float scale, unsigned rseed, int env0, int episode,
                                      int t, float eps, const float* q, int* units, const marl_record_t* rec, int M, void* stream) {
  return battle_fused_step<false>(types, shield, type_bits, scale, rseed, env0, episode, t, eps, q, units, rec, M, stream);
}

extern "C" int marl_battle_fused_step_sample(unsigned types, int shield, int type_bits, float scale, unsigned rseed, int env0,
                                             int episode, int t, float eps, const float* q, int* units, const marl_record_t* rec,
                                             int M, void* stream) {
  return battle_fused_step<true>(types, shield, type_bits, scale, rseed, env0, episode, t, eps, q, units, rec, M, stream);
}
