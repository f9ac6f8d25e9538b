// The "battle" environment: a deterministic micro-combat simulator in SMAC's observation / state / action layout.
// Its rules as __host__ __device__ functions, for the per-step kernels (battle.hip) and the whole-rollout kernel (battle_rollout.hip); numpy restatement:
// tests/battle_oracle.py - integer fields equal, float fields bit for bit (every feature is one correctly rounded fp32 operation on
// integers: sqrtf of an integer, then one division).  The start positions are the only random part: hkey() draws on streams from 16 up.
//
// A 32 x 32 integer grid; sight 9 (d2 <= 81), shoot 6 (d2 <= 36), a move is 2 cells; no armour, regeneration or collision.
// Unit state: (x, y, hp, shield, cooldown) per unit, allies 0 .. N - 1 then enemies N .. N + M - 1, as BT_F ints each.
#pragma once
#include "synth_env.h"

enum { BT_AX = 16, BT_AY, BT_EX, BT_EY };                         // hash streams (synth_env.h holds 0 .. 9)
enum { BT_X = 0, BT_Y, BT_HP, BT_SH, BT_CD, BT_F };               // the fields of a unit
enum { BT_MARINE = 0, BT_STALKER, BT_ZEALOT, BT_TYPES };          // type one-hot: stalker = bit 0, zealot = bit 1
enum { BT_GRID = 32, BT_SIGHT2 = 81, BT_SHOOT2 = 36, BT_STEP = 2, BT_MAX_SIDE = 16, BT_KILL = 10, BT_WIN = 200 };

__host__ __device__ inline int bt_max_hp(int type) { return type == BT_MARINE ? 45 : type == BT_STALKER ? 80 : 100; }
__host__ __device__ inline int bt_max_sh(int type) { return type == BT_MARINE ? 0 : type == BT_STALKER ? 80 : 50; }
__host__ __device__ inline int bt_damage(int type) { return type == BT_MARINE ? 6 : type == BT_STALKER ? 13 : 16; }
__host__ __device__ inline int bt_cooldown(int type) { return type == BT_STALKER ? 2 : 1; }

// A map: N allies against M = N enemies of the same types (two bits per unit of a side, unit 0 lowest); the feature widths follow
// SMAC's: per enemy [attackable, dist, dx, dy, hp, (shield), type bits], per other ally [visible, ...], own [hp, (shield), type bits];
// state per ally [hp, cd, x, y, (shield), type bits], per enemy [hp, x, y, (shield), type bits], then the (N, A) last actions
struct BattleCfg {
  int N, M, A, shield, tbits;
  unsigned types;
  int nf, own, na, ne, O, S;
};
__host__ __device__ inline bool bt_supported(int N, int M, int A) { return N >= 1 && N <= BT_MAX_SIDE && M == N && A == 6 + M; }
__host__ __device__ inline BattleCfg bt_cfg(int N, int M, int A, int shield, int tbits, unsigned types) {
  BattleCfg c;
  c.N = N; c.M = M; c.A = A; c.shield = shield; c.tbits = tbits; c.types = types;
  c.nf = 5 + shield + tbits; c.own = 1 + shield + tbits; c.na = 4 + shield + tbits; c.ne = 3 + shield + tbits;
  c.O = 4 + (M + N - 1) * c.nf + c.own;
  c.S = N * c.na + M * c.ne + N * A;
  return c;
}
// type of unit k of either side's list (k < N: ally k; else enemy k - N)
__host__ __device__ inline int bt_type(const BattleCfg& c, int k) { return (int)(c.types >> (2 * (k < c.N ? k : k - c.N))) & 3; }

// ---- reset: ally i at x = 8 + h % 3, y = 16 + 2 i - N + h' % 2; enemy j at x = 23 - h % 3, the same y rule; full hp / shield, cd 0
__host__ __device__ inline void bt_start(const BattleCfg& c, unsigned seed, unsigned env, int episode, int k, int* un) {
  const bool ally = k < c.N;
  const int i = ally ? k : k - c.N, n = ally ? c.N : c.M;
  const unsigned hx = hkey(seed, ally ? BT_AX : BT_EX, env, (unsigned)episode, (unsigned)i);
  const unsigned hy = hkey(seed, ally ? BT_AY : BT_EY, env, (unsigned)episode, (unsigned)i);
  un[BT_X] = ally ? 8 + (int)(hx % 3u) : 23 - (int)(hx % 3u);
  un[BT_Y] = 16 + 2 * i - n + (int)(hy % 2u);
  un[BT_HP] = bt_max_hp(bt_type(c, k));
  un[BT_SH] = c.shield ? bt_max_sh(bt_type(c, k)) : 0;
  un[BT_CD] = 0;
}

__host__ __device__ inline int bt_d2(const int* a, const int* b) {
  const int dx = b[BT_X] - a[BT_X], dy = b[BT_Y] - a[BT_Y];
  return dx * dx + dy * dy;
}
// the displacement of move action k (2 .. 5): (0,+2) (0,-2) (+2,0) (-2,0); available iff the destination stays on the grid
__host__ __device__ inline void bt_move(int k, int& dx, int& dy) {
  dx = k == 4 ? BT_STEP : k == 5 ? -BT_STEP : 0;
  dy = k == 2 ? BT_STEP : k == 3 ? -BT_STEP : 0;
}
__host__ __device__ inline bool bt_move_ok(const int* a, int k) {
  int dx, dy;
  bt_move(k, dx, dy);
  const int x = a[BT_X] + dx, y = a[BT_Y] + dy;
  return x >= 0 && x < BT_GRID && y >= 0 && y < BT_GRID;
}
// availability of action k to agent i (un: every unit's state): a dead agent has the no-op alone; a live one stop, the moves that
// stay on the grid and the attacks on live enemies within shoot range
__host__ __device__ inline bool bt_avail(const BattleCfg& c, const int* un, int i, int k) {
  const int* a = un + i * BT_F;
  if (a[BT_HP] <= 0) return k == 0;
  if (k < 2) return k == 1;
  if (k < 6) return bt_move_ok(a, k);
  const int* e = un + (c.N + k - 6) * BT_F;
  return e[BT_HP] > 0 && bt_d2(a, e) <= BT_SHOOT2;
}

// ---- decisions, from the pre-step state.  (dx, dy): the unit's move; target: the unit it fires at, or -1
// a live agent's action that is unavailable (out of range included), or an attack on cooldown, counts as stop
__host__ __device__ inline void bt_ally_decide(const BattleCfg& c, const int* un, int i, int act, int& dx, int& dy, int& target) {
  dx = dy = 0; target = -1;
  const int* a = un + i * BT_F;
  if (a[BT_HP] <= 0 || act < 2 || act >= c.A || !bt_avail(c, un, i, act)) return;
  if (act < 6) bt_move(act, dx, dy);
  else if (a[BT_CD] == 0) target = c.N + act - 6;
}
// a live enemy takes the live ally with the smallest d2 (ties: the lowest index): fires at it within shoot range when its cooldown is
// 0, waits there otherwise, else walks min(2, |delta|) cells towards it along the axis of the larger |delta| (ties: x)
__host__ __device__ inline void bt_enemy_decide(const BattleCfg& c, const int* un, int j, int& dx, int& dy, int& target) {
  dx = dy = 0; target = -1;
  const int* e = un + (c.N + j) * BT_F;
  if (e[BT_HP] <= 0) return;
  int best = -1, bd = 0;
  for (int i = 0; i < c.N; ++i) {
    const int* a = un + i * BT_F;
    if (a[BT_HP] <= 0) continue;
    const int d = bt_d2(e, a);
    if (best < 0 || d < bd) { best = i; bd = d; }
  }
  if (best < 0) return;
  if (bd <= BT_SHOOT2) {
    if (e[BT_CD] == 0) target = best;
    return;
  }
  const int ddx = un[best * BT_F + BT_X] - e[BT_X], ddy = un[best * BT_F + BT_Y] - e[BT_Y];
  const int ax = ddx < 0 ? -ddx : ddx, ay = ddy < 0 ? -ddy : ddy;
  if (ax >= ay) dx = (ddx < 0 ? -1 : 1) * (ax < BT_STEP ? ax : BT_STEP);
  else dy = (ddy < 0 ? -1 : 1) * (ay < BT_STEP ? ay : BT_STEP);
}
// damage d on (hp, shield): the shield first, then hp, floored at 0; returns what was actually removed
__host__ __device__ inline int bt_hit(int d, int& hp, int& sh) {
  const int ds = d < sh ? d : sh;
  sh -= ds;
  const int dh = d - ds < hp ? d - ds : hp;
  hp -= dh;
  return ds + dh;
}

// ---- features of a slot, from the unit state un
__host__ __device__ inline float bt_ratio(int v, int max) { return max > 0 ? (float)v / (float)max : 0.f; }
// fields 4 .. of an entity block of the observation / fields of the own block from 0: hp, (shield), type bits
__host__ __device__ inline float bt_health(const BattleCfg& c, const int* u, int type, int f) {
  if (f == 0) return bt_ratio(u[BT_HP], bt_max_hp(type));
  if (c.shield && f == 1) return bt_ratio(u[BT_SH], bt_max_sh(type));
  return type == f - c.shield ? 1.f : 0.f;          // type bit b = f - 1 - shield: stalker (1) bit 0, zealot (2) bit 1
}
// element k of agent i's observation (zeros if dead): the four moves' availability, the enemies, the other allies, itself
__host__ __device__ inline float bt_obs(const BattleCfg& c, const int* un, int i, int k) {
  const int* a = un + i * BT_F;
  if (a[BT_HP] <= 0) return 0.f;
  if (k < 4) return bt_move_ok(a, k + 2) ? 1.f : 0.f;
  k -= 4;
  const int ents = (c.M + c.N - 1) * c.nf;
  if (k >= ents) return bt_health(c, a, bt_type(c, i), k - ents);
  const int b = k / c.nf, f = k - b * c.nf;
  const bool enemy = b < c.M;
  const int o = enemy ? c.N + b : (b - c.M) + (b - c.M >= i ? 1 : 0);
  const int* u = un + o * BT_F;
  const int d2 = bt_d2(a, u);
  if (u[BT_HP] <= 0 || d2 > BT_SIGHT2) return 0.f;
  if (f == 0) return !enemy || d2 <= BT_SHOOT2 ? 1.f : 0.f;
  if (f == 1) return sqrtf((float)d2) / 9.0f;
  if (f == 2) return (float)(u[BT_X] - a[BT_X]) / 9.0f;
  if (f == 3) return (float)(u[BT_Y] - a[BT_Y]) / 9.0f;
  return bt_health(c, u, bt_type(c, o), f - 4);
}
// element k of the state: allies, enemies (dead units are zero rows), then the one-hot of the last recorded actions (act == NULL or an
// action outside 0 .. A - 1: a zero row)
__host__ __device__ inline float bt_state(const BattleCfg& c, const int* un, const int* act, int k) {
  const int na = c.N * c.na, ne = c.M * c.ne;
  if (k < na + ne) {
    const bool ally = k < na;
    const int w = ally ? c.na : c.ne, r = ally ? k : k - na;
    const int b = r / w;
    int f = r - b * w;
    const int o = ally ? b : c.N + b, type = bt_type(c, o);
    const int* u = un + o * BT_F;
    if (u[BT_HP] <= 0) return 0.f;
    if (f == 0) return bt_ratio(u[BT_HP], bt_max_hp(type));
    if (ally) {
      if (f == 1) return (float)u[BT_CD] / (float)bt_cooldown(type);
      --f;
    }
    if (f == 1) return (float)(u[BT_X] - 16) / 32.0f;
    if (f == 2) return (float)(u[BT_Y] - 16) / 32.0f;
    return bt_health(c, u, type, f - 2);
  }
  k -= na + ne;
  const int n = k / c.A;
  return act && act[n] == k - n * c.A ? 1.f : 0.f;
}

// ---- the host side of every launcher (battle.hip, battle_rollout.hip)
// hipErrorInvalidValue unless the shape is one the kernels cover; cfg: the feature widths
inline int battle_cfg(int N, int M, int A, int shield, int type_bits, unsigned types, long state_ld, int T, BattleCfg& cfg) {
  if (!bt_supported(N, M, A) || (shield != 0 && shield != 1) || type_bits < 0 || type_bits > BT_TYPES - 1 || T < 1)
    return (int)hipErrorInvalidValue;
  cfg = bt_cfg(N, M, A, shield, type_bits, types);
  for (int i = 0; i < N; ++i) {
    const int type = bt_type(cfg, i);
    if (type >= BT_TYPES || type > type_bits) return (int)hipErrorInvalidValue;     // a type the one-hot has no bit for
  }
  return state_ld < cfg.S ? (int)hipErrorInvalidValue : 0;
}
