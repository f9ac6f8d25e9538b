// The hunt environment's kernels (rules: hunt_env.h): reset, one launch per lock-step that applies the step and writes slot t + 1 of
// the record, and the same launch with the action choice in front.  The shape is battle.hip's: a wave per environment, HT_WPB
// environments per workgroup; the units sit on lanes 0 .. N + M - 1 for the dynamics (the unit state of the workgroup's environments
// lives in LDS), catcher counts per prey, captures and lone attempts are integer LDS atomics (any order gives the same sum), then all
// 64 lanes write the slot's N O + S + N A floats as three contiguous runs, 16 bytes a lane where a run's address allows.  A slot is
// N x 77 window features: the unit lanes first count themselves into two G x G tiles in LDS (predators per cell, live prey per
// cell), and an element of the window is one lookup there, not a walk over the units.
#include "hunt_env.h"
#include "env_slot.h"
#include "../../include/marl_hip.h"

namespace {
constexpr int HT_WPB = 4;                       // environments (waves) per workgroup
constexpr int HT_UNITS = 2 * HT_MAX_SIDE;
constexpr int HT_CELLS = HT_MAX_G * HT_MAX_G;

// The shared memory of a launch: the unit state of the workgroup's environments (pre-step, then post-step), the slot's two count
// tiles (pitch G), the catchers per prey and the step's captures and lone attempts
struct HuntLds {
  int un[HT_WPB][HT_UNITS * HT_F];
  int pc[HT_WPB][HT_CELLS];
  int qc[HT_WPB][HT_CELLS];
  int cnt[HT_WPB][HT_MAX_SIDE];
  int cap[HT_WPB], lone[HT_WPB];
};

__device__ __forceinline__ void clear_tiles(const HuntCfg& c, HuntLds& s, int w, int lane) {
  for (int k = lane; k < c.G * c.G; k += MARL_WAVE) s.pc[w][k] = s.qc[w][k] = 0;
}
// unit `lane` (me: its state) counts itself into its tile; a barrier after clear_tiles before, one before the first lookup after
// (a unit state that never saw a reset may hold anything: a position off the grid is not counted)
__device__ __forceinline__ void count_unit(const HuntCfg& c, HuntLds& s, int w, int lane, const int* me) {
  if (me[HT_LIVE] && ht_on_grid(c.G, me[HT_X], me[HT_Y])) atomicAdd(&(lane < c.N ? s.pc : s.qc)[w][ht_cell(c.G, me[HT_X], me[HT_Y])], 1);
}

// slot `slot` of environment e from the unit state and the count tiles of wave w (LDS); !live: zeros
__device__ __forceinline__ void write_slot(const HuntCfg& c, const HuntLds& s, int w, bool live, float* obs, float* state, long SL,
                                           float* avail, long e, int T, int slot, int lane) {
  const long row = e * (T + 1) + slot;
  const int* un = s.un[w];
  const int *pc = s.pc[w], *qc = s.qc[w];
  write_run(obs + row * c.N * HT_O, c.N * HT_O, lane,
            [&](int k) { const int i = k / HT_O; return live ? ht_obs(c, un, pc, qc, i, k - i * HT_O) : 0.f; });
  write_run(state + row * SL, c.S, lane, [&](int k) { return live ? ht_state(c, un, k) : 0.f; });
  write_run(avail + row * c.N * HT_A, c.N * HT_A, lane,
            [&](int k) { const int i = k / HT_A; return live && ht_avail(c, un, qc, i, k - i * HT_A) ? 1.f : 0.f; });
}

__global__ __launch_bounds__(HT_WPB * MARL_WAVE) void hunt_reset_kernel(HuntCfg c, unsigned seed, int env0, int episode, int* units,
                                                                       int* length, int* won, float* obs, float* state, long SL,
                                                                       float* avail, int E, int T) {
  __shared__ HuntLds s;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * HT_WPB + w;
  const bool valid = e < E;
  const int NU = c.N + c.M;
  clear_tiles(c, s, w, lane);
  __syncthreads();
  if (valid && lane < NU) {
    int* un = s.un[w] + lane * HT_F;
    ht_start(c, seed, (unsigned)(env0 + (int)e), episode, lane, un);
    for (int f = 0; f < HT_F; ++f) units[(e * NU + lane) * HT_F + f] = un[f];
    count_unit(c, s, w, lane, un);
  }
  if (valid && lane == 0) { length[e] = T; won[e] = 0; }
  __syncthreads();
  if (valid) write_slot(c, s, w, true, obs, state, SL, avail, e, T, 0, lane);
}

// Lock-step t of environment e by its wave (every thread of the workgroup calls this: it holds workgroup barriers).  a: the action of
// predator `lane` as given (lanes < N of a live environment; anything elsewhere); live: t < length[e] as read before the step
__device__ __forceinline__ void hunt_step_body(const HuntCfg& c, HuntLds& s, unsigned seed, int env0, int episode, int t, int a,
                                               bool valid, bool live, long e, int w, int lane, int* units, int* u, float* r,
                                               float* term, float* padded, int* length, int* won, int* alive_next, float* obs,
                                               float* state, long SL, float* avail, int T) {
  const int N = c.N, NU = c.N + c.M;
  const bool unit = valid && lane < NU;
  int me[HT_F] = {0, 0, 0};
  if (unit)
    for (int f = 0; f < HT_F; ++f) s.un[w][lane * HT_F + f] = me[f] = units[(e * NU + lane) * HT_F + f];
  if (lane < HT_MAX_SIDE) s.cnt[w][lane] = 0;
  if (valid && lane < N) {
    a = live ? a : -1;                                // the record keeps the action as given
    u[(e * T + t) * N + lane] = a;
  }
  if (lane == 0) s.cap[w] = s.lone[w] = 0;
  clear_tiles(c, s, w, lane);
  __syncthreads();
  // 1. every predator's decision, from the pre-step state: its move, or the prey it catches at
  int dx = 0, dy = 0;
  if (live && unit && lane < N) {
    int target;
    ht_decide(c, s.un[w], lane, a, dx, dy, target);
    if (target >= 0) atomicAdd(&s.cnt[w][target], 1);
  }
  __syncthreads();
  // 2. - 7. captures and lone attempts, predators move, captured prey leave, the other live prey walk
  if (live && unit) {
    if (lane >= N && me[HT_LIVE]) {
      const int catchers = s.cnt[w][lane - N];
      if (catchers >= 2) {
        me[HT_LIVE] = 0;
        atomicAdd(&s.cap[w], 1);
      } else {
        if (catchers == 1) atomicAdd(&s.lone[w], 1);
        ht_prey_move(c, me, seed, (unsigned)(env0 + (int)e), env_tg(episode, T, t), lane - N, dx, dy);
      }
    }
    me[HT_X] += dx; me[HT_Y] += dy;
    for (int f = 0; f < HT_F; ++f) {
      s.un[w][lane * HT_F + f] = me[f];
      units[(e * NU + lane) * HT_F + f] = me[f];
    }
  }
  if (unit) count_unit(c, s, w, lane, me);
  const bool prey_left = __ballot(unit && lane >= N && me[HT_LIVE]) != 0ull;
  __syncthreads();
  if (valid && lane == 0) {
    const bool win = live && !prey_left;
    const bool over = !live || !prey_left || t + 1 == T;
    r[e * T + t] = live ? ht_reward(c, s.cap[w], s.lone[w]) : 0.f;
    term[e * T + t] = over ? 1.f : 0.f;
    padded[e * T + t] = live ? 0.f : 1.f;
    if (live && over) { length[e] = t + 1; won[e] = win ? 1 : 0; }
    if (alive_next) alive_next[e] = over ? 0 : 1;
  }
  // slot t + 1: the final observation at the terminating step, zeros after
  if (valid) write_slot(c, s, w, live, obs, state, SL, avail, e, T, t + 1, lane);
}

__global__ __launch_bounds__(HT_WPB * MARL_WAVE) void hunt_step_kernel(HuntCfg c, unsigned seed, int env0, int episode, int t,
                                                                      const int* act, int* units, int* u, float* r, float* term,
                                                                      float* padded, int* length, int* won, int* alive_next,
                                                                      float* obs, float* state, long SL, float* avail, int E, int T) {
  __shared__ HuntLds s;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * HT_WPB + w;
  const bool valid = e < E;
  const bool live = valid && t < length[e];          // an episode that ended at step t' has length t' + 1 <= t
  const int a = live && lane < c.N ? act[e * c.N + lane] : -1;
  hunt_step_body(c, s, seed, env0, episode, t, a, valid, live, e, w, lane, units, u, r, term, padded, length, won, alive_next, obs,
                 state, SL, avail, T);
}

// The action choice and the step in one launch: predator lane n of a live environment chooses from its row of q (E,1,N,A) and slot
// t's availability in the record (env_slot.h: env_choose), keyed by (rseed, env0 + e, env_tg(episode, T, t), n); then hunt_step_body
template <bool SAMPLE>
__global__ __launch_bounds__(HT_WPB * MARL_WAVE) void hunt_fused_step_kernel(HuntCfg c, unsigned seed, unsigned rseed, int env0,
                                                                            int episode, int t, float eps, const float* q, int* units,
                                                                            int* u, float* r, float* term, float* padded, int* length,
                                                                            int* won, float* obs, float* state, long SL, float* avail,
                                                                            int E, int T) {
  __shared__ HuntLds s;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * HT_WPB + w;
  const bool valid = e < E;
  const bool live = valid && t < length[e];
  const int N = c.N;
  int arg = -1;
  if (live && lane < N)
    arg = env_choose<SAMPLE>(q + (e * N + lane) * HT_A, avail + ((e * (T + 1) + t) * N + lane) * HT_A, HT_A, eps, rseed,
                             (unsigned)(env0 + (int)e), env_tg(episode, T, t), lane);
  hunt_step_body(c, s, seed, env0, episode, t, arg, valid, live, e, w, lane, units, u, r, term, padded, length, won, nullptr, obs,
                 state, SL, avail, T);
}

}  // namespace

extern "C" int marl_hunt_supported(int N, int M, int G, int A) { return ht_supported(N, M, G, A) ? 1 : 0; }

// every launcher's checks, in this order: a record, hunt_cfg's refusals, the widths the record states against the derived ones,
// lock-step t (reset: 0) inside the episode
static int hunt_record_cfg(const marl_record_t* rec, int M, int G, int pen4, int t, HuntCfg& cfg) {
  if (!rec) return (int)hipErrorInvalidValue;
  const int bad = hunt_cfg(rec->N, M, rec->A, G, pen4, rec->state_ld, rec->T, cfg);
  if (bad) return bad;
  return rec->O != cfg.O || rec->S != cfg.S || t < 0 || t >= rec->T ? (int)hipErrorInvalidValue : 0;
}

static dim3 hunt_grid(int E) { return dim3((E + HT_WPB - 1) / HT_WPB); }

extern "C" int marl_hunt_reset(unsigned seed, int env0, int episode, int G, int M, int* units, const marl_record_t* rec,
                               void* stream) {
  HuntCfg cfg;
  const int bad = hunt_record_cfg(rec, M, G, 0, 0, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(hunt_reset_kernel, hunt_grid(rec->E), dim3(HT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, seed, env0, episode,
                     units, rec->length, rec->won, rec->obs, rec->state, rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_hunt_step(unsigned seed, int env0, int episode, int G, int pen4, int t, const int* act, int* units,
                              const marl_record_t* rec, int* alive_next, int M, void* stream) {
  HuntCfg cfg;
  const int bad = hunt_record_cfg(rec, M, G, pen4, t, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(hunt_step_kernel, hunt_grid(rec->E), dim3(HT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, seed, env0, episode,
                     t, act, units, rec->u, rec->r, rec->term, rec->padded, rec->length, rec->won, alive_next, rec->obs, rec->state,
                     rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

template <bool SAMPLE>
static int hunt_fused_step(unsigned seed, unsigned rseed, int env0, int episode, int G, int pen4, int t, float eps, const float* q,
                           int* units, const marl_record_t* rec, int M, void* stream) {
  HuntCfg cfg;
  const int bad = hunt_record_cfg(rec, M, G, pen4, t, cfg);
  if (bad) return bad;
  if (rec->E <= 0) return 0;
  hipLaunchKernelGGL(hunt_fused_step_kernel<SAMPLE>, hunt_grid(rec->E), dim3(HT_WPB * MARL_WAVE), 0, (hipStream_t)stream, cfg, seed,
                     rseed, env0, episode, t, eps, q, units, rec->u, rec->r, rec->term, rec->padded, rec->length, rec->won, rec->obs,
                     rec->state, rec->state_ld, rec->avail, rec->E, rec->T);
  MARL_CHECK_LAUNCH();
  return 0;
}

extern "C" int marl_hunt_fused_step(unsigned seed, unsigned rseed, int env0, int episode, int G, int pen4, int t, float eps,
                                    const float* q, int* units, const marl_record_t* rec, int M, void* stream) {
  return hunt_fused_step<false>(seed, rseed, env0, episode, G, pen4, t, eps, q, units, rec, M, stream);
}

extern "C" int marl_hunt_fused_step_sample(unsigned seed, unsigned rseed, int env0, int episode, int G, int pen4, int t, float eps,
                                           const float* q, int* units, const marl_record_t* rec, int M, void* stream) {
  return hunt_fused_step<true>(seed, rseed, env0, episode, G, pen4, t, eps, q, units, rec, M, stream);
}
