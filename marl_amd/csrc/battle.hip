// The battle environment's two kernels (rules: battle_env.h): reset, and one launch per lock-step that applies the step and writes
// slot t + 1 of the record.  A wave per environment, BT_WPB environments per workgroup; the units sit on lanes 0 .. N + M - 1 for the
// dynamics (the unit state of the workgroup's environments lives in LDS), damage and points are integer LDS atomics (any order gives
// the same sum), then all 64 lanes write the slot's N O + S + N A floats as three contiguous runs, 16 bytes a lane where a run's
// address allows (a run starts on any 4-byte boundary: N O is 90 floats on 3m).
#include "battle_env.h"
#include "../../include/marl_hip.h"

namespace {
constexpr int BT_WPB = 4;                       // environments (waves) per workgroup
constexpr int BT_UNITS = 2 * BT_MAX_SIDE;

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

__global__ __launch_bounds__(BT_WPB * MARL_WAVE) void battle_step_kernel(BattleCfg c, float scale, int t, const int* act, int* units,
                                                                        int* u, float* r, float* term, float* padded, int* length,
                                                                        int* won, int* alive_next, float* obs, float* state, long SL,
                                                                        float* avail, int E, int T) {
  __shared__ int s_un[BT_WPB][BT_UNITS * BT_F];      // the pre-step state, then the post-step state
  __shared__ int s_dmg[BT_WPB][BT_UNITS];
  __shared__ int s_act[BT_WPB][BT_MAX_SIDE];
  __shared__ int s_pts[BT_WPB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * BT_WPB + w;
  const bool valid = e < E;
  const bool live = valid && t < length[e];          // an episode that ended at step t' has length t' + 1 <= t
  const int N = c.N, NU = c.N + c.M;
  const bool unit = valid && lane < NU;
  int me[BT_F] = {0, 0, 0, 0, 0};
  if (unit) {
    for (int f = 0; f < BT_F; ++f) s_un[w][lane * BT_F + f] = me[f] = units[(e * NU + lane) * BT_F + f];
    s_dmg[w][lane] = 0;
  }
  if (valid && lane < N) {
    const int a = live ? act[e * N + lane] : -1;     // the record keeps the action as given
    s_act[w][lane] = a;
    u[(e * T + t) * N + lane] = a;
  }
  if (lane == 0) s_pts[w] = 0;
  __syncthreads();
  // 1. every unit's action, from the pre-step state
  int dx = 0, dy = 0, target = -1;
  const int type = unit ? bt_type(c, lane) : 0;
  if (live && unit) {
    if (lane < N) bt_ally_decide(c, s_un[w], lane, s_act[w][lane], dx, dy, target);
    else bt_enemy_decide(c, s_un[w], lane - N, dx, dy, target);
    if (target >= 0) atomicAdd(&s_dmg[w][target], bt_damage(type));
  }
  __syncthreads();
  // 2. - 4. movers move, damage lands (a unit killed this step has dealt its own), cooldowns
  if (live && unit) {
    const int hp0 = me[BT_HP];
    me[BT_X] += dx; me[BT_Y] += dy;
    const int removed = bt_hit(s_dmg[w][lane], me[BT_HP], me[BT_SH]);
    me[BT_CD] = target >= 0 ? bt_cooldown(type) : (me[BT_CD] > 0 ? me[BT_CD] - 1 : 0);
    if (lane >= N && removed > 0) atomicAdd(&s_pts[w], removed + (hp0 > 0 && me[BT_HP] <= 0 ? BT_KILL : 0));
    for (int f = 0; f < BT_F; ++f) {
      s_un[w][lane * BT_F + f] = me[f];
      units[(e * NU + lane) * BT_F + f] = me[f];
    }
  }
  const unsigned long long up = __ballot(unit && me[BT_HP] > 0);
  const bool allies = (up & ((1ull << N) - 1ull)) != 0ull, enemies = (up >> N) != 0ull;
  __syncthreads();
  if (valid && lane == 0) {
    const bool win = live && !enemies && allies;
    const bool over = !live || !enemies || !allies || t + 1 == T;
    r[e * T + t] = live ? (float)(s_pts[w] + (win ? BT_WIN : 0)) * scale : 0.f;
    term[e * T + t] = over ? 1.f : 0.f;
    padded[e * T + t] = live ? 0.f : 1.f;
    if (live && over) { length[e] = t + 1; won[e] = win ? 1 : 0; }
    if (alive_next) alive_next[e] = over ? 0 : 1;
  }
  // slot t + 1: the final observation at the terminating step, zeros after
  if (valid) write_slot(c, s_un[w], s_act[w], live, obs, state, SL, avail, e, T, t + 1, lane);
}

// hipErrorInvalidValue unless the shape is one the kernels cover; cfg: the feature widths
int battle_cfg(int N, int M, int A, int shield, int type_bits, unsigned types, long state_ld, int T, BattleCfg& cfg) {
  if (!bt_supported(N, M, A) || (shield != 0 && shield != 1) || type_bits < 0 || type_bits > BT_TYPES - 1 || T < 1)
    return (int)hipErrorInvalidValue;
  cfg = bt_cfg(N, M, A, shield, type_bits, types);
  for (int i = 0; i < N; ++i) {
    const int type = bt_type(cfg, i);
    if (type >= BT_TYPES || type > type_bits) return (int)hipErrorInvalidValue;     // a type the one-hot has no bit for
  }
  return state_ld < cfg.S ? (int)hipErrorInvalidValue : 0;
}
}  // namespace

extern "C" int marl_battle_supported(int n_allies, int n_enemies, int A) { return bt_supported(n_allies, n_enemies, A) ? 1 : 0; }

extern "C" int marl_battle_reset(unsigned seed, int env0, int episode, unsigned types, int shield, int type_bits, int* units,
                                 int* length, int* won, float* obs, float* state, long state_ld, float* avail, int E, int T, int N,
                                 int M, int A, void* stream) {
  BattleCfg cfg;
  const int bad = battle_cfg(N, M, A, shield, type_bits, types, state_ld, T, cfg);
  if (bad) return bad;
  if (E <= 0) return 0;
  hipLaunchKernelGGL(battle_reset_kernel, dim3((E + BT_WPB - 1) / BT_WPB), dim3(BT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, seed,
                     env0, episode, units, length, won, obs, state, state_ld, avail, E, T);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_battle_step(unsigned types, int shield, int type_bits, float scale, int t, const int* act, int* units, int* u,
                                float* r, float* term, float* padded, int* length, int* won, int* alive_next, float* obs,
                                float* state, long state_ld, float* avail, int E, int T, int N, int M, int A, void* stream) {
  BattleCfg cfg;
  const int bad = battle_cfg(N, M, A, shield, type_bits, types, state_ld, T, cfg);
  if (bad) return bad;
  if (t < 0 || t >= T) return (int)hipErrorInvalidValue;
  if (E <= 0) return 0;
  hipLaunchKernelGGL(battle_step_kernel, dim3((E + BT_WPB - 1) / BT_WPB), dim3(BT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, scale,
                     t, act, units, u, r, term, padded, length, won, alive_next, obs, state, state_ld, avail, E, T);
  MARL_CHECK_LAUNCH();
  return 0;
}
