// The "hunt" environment: predator-prey with a lone-catch penalty.  Its rules as __host__ __device__ functions, for
// the per-step kernels (hunt.hip); numpy restatement: tests/hunt_oracle.py - integer fields equal, float fields bit for bit (every
// feature is 0, 1 or one correctly rounded fp32 division of two integers).  The start positions and the prey's walk are the random
// part: hkey() draws on streams 32 .. 36.
//
// A G x G integer grid; N predators (the agents) and M prey share cells freely.  Unit state: (x, y, live) per unit, predators
// 0 .. N - 1 (always live) then prey N .. N + M - 1, as HT_F ints each.  Actions: 0 stay, 1 .. 4 one cell (0,+1) (0,-1) (+1,0)
// (-1,0), 5 catch.  A prey with two or more catchers in a step is captured (10 points each); a prey with exactly one costs the team
// the penalty; pen4 = 4 x penalty, so that points4 = 40 captures - pen4 lone attempts is an integer and r = points4 / 4 exact.
#pragma once
#include "synth_env.h"

enum { HT_PX = 32, HT_PY, HT_QX, HT_QY, HT_MOVE };                // hash streams (synth_env.h lists every file's)
enum { HT_X = 0, HT_Y, HT_LIVE, HT_F };                           // the fields of a unit
enum { HT_A = 6, HT_CATCH = 5, HT_WIN = 5, HT_O = 3 * HT_WIN * HT_WIN + 2, HT_MAX_SIDE = 16, HT_MAX_G = 32, HT_MIN_G = 3,
       HT_MAX_PEN4 = 64, HT_CAPTURE4 = 40 };

struct HuntCfg { int N, M, G, pen4, O, S; };
__host__ __device__ inline bool ht_supported(int N, int M, int G, int A) {
  return N >= 2 && N <= HT_MAX_SIDE && M >= 1 && M <= HT_MAX_SIDE && G >= HT_MIN_G && G <= HT_MAX_G && A == HT_A;
}
__host__ __device__ inline HuntCfg ht_cfg(int N, int M, int G, int pen4) {
  HuntCfg c;
  c.N = N; c.M = M; c.G = G; c.pen4 = pen4;
  c.O = HT_O;
  c.S = 2 * N + 3 * M;
  return c;
}

// ---- reset: predator i at (h % G, h' % G) of streams HT_PX / HT_PY, prey j likewise of HT_QX / HT_QY; every unit live
__host__ __device__ inline void ht_start(const HuntCfg& c, unsigned seed, unsigned env, int episode, int k, int* un) {
  const bool pred = k < c.N;
  const unsigned i = (unsigned)(pred ? k : k - c.N);
  un[HT_X] = (int)(hkey(seed, pred ? HT_PX : HT_QX, env, (unsigned)episode, i) % (unsigned)c.G);
  un[HT_Y] = (int)(hkey(seed, pred ? HT_PY : HT_QY, env, (unsigned)episode, i) % (unsigned)c.G);
  un[HT_LIVE] = 1;
}

__host__ __device__ inline bool ht_on_grid(int G, int x, int y) { return x >= 0 && x < G && y >= 0 && y < G; }
// the displacement of move k (1 .. 4): (0,+1) (0,-1) (+1,0) (-1,0); anything else: none
__host__ __device__ inline void ht_move(int k, int& dx, int& dy) {
  dx = k == 3 ? 1 : k == 4 ? -1 : 0;
  dy = k == 1 ? 1 : k == 2 ? -1 : 0;
}
__host__ __device__ inline int ht_dist(const int* a, const int* b) {
  const int dx = b[HT_X] - a[HT_X], dy = b[HT_Y] - a[HT_Y];
  return (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
}
// the live prey at the smallest Manhattan distance from predator i (ties: the lowest index), or -1; dist: that distance
__host__ __device__ inline int ht_target(const HuntCfg& c, const int* un, int i, int& dist) {
  int best = -1;
  dist = 0;
  for (int j = 0; j < c.M; ++j) {
    const int* q = un + (c.N + j) * HT_F;
    if (!q[HT_LIVE]) continue;
    const int d = ht_dist(un + i * HT_F, q);
    if (best < 0 || d < dist) { best = j; dist = d; }
  }
  return best;
}

// ---- the two count tiles of a slot, G x G ints each with pitch G: predators per cell (pc), live prey per cell (qc).  The kernels
// fill them with one LDS atomic per unit lane, and the features below look cells up in them instead of walking the units
__host__ __device__ inline int ht_cell(int G, int x, int y) { return y * G + x; }
__host__ __device__ inline int ht_count(const int* tile, int G, int x, int y) { return ht_on_grid(G, x, y) ? tile[ht_cell(G, x, y)] : 0; }

// availability of action k to predator i: stay always, a move iff its destination is on the grid, catch iff a live prey is at
// Manhattan distance <= 1 (its own cell included)
__host__ __device__ inline bool ht_avail(const HuntCfg& c, const int* un, const int* qc, int i, int k) {
  const int x = un[i * HT_F + HT_X], y = un[i * HT_F + HT_Y];
  if (k == 0) return true;
  if (k < HT_CATCH) {
    int dx, dy;
    ht_move(k, dx, dy);
    return ht_on_grid(c.G, x + dx, y + dy);
  }
  return ht_count(qc, c.G, x, y) + ht_count(qc, c.G, x, y + 1) + ht_count(qc, c.G, x, y - 1) + ht_count(qc, c.G, x + 1, y) +
         ht_count(qc, c.G, x - 1, y) > 0;
}

// ---- decisions, from the pre-step state.  (dx, dy): the predator's move; target: the prey it catches at, or -1.  An action that
// is unavailable or outside 0 .. A - 1 counts as stay
__host__ __device__ inline void ht_decide(const HuntCfg& c, const int* un, int i, int act, int& dx, int& dy, int& target) {
  dx = dy = 0; target = -1;
  if (act < 1 || act >= HT_A) return;
  if (act < HT_CATCH) {
    ht_move(act, dx, dy);
    if (!ht_on_grid(c.G, un[i * HT_F + HT_X] + dx, un[i * HT_F + HT_Y] + dy)) dx = dy = 0;
    return;
  }
  int dist;
  const int j = ht_target(c, un, i, dist);
  if (j >= 0 && dist <= 1) target = j;
}
// the move of live, not captured prey j at time index tg: draw % 5 - 0 stays, 1 .. 4 the moves above, off the grid stays
__host__ __device__ inline void ht_prey_move(const HuntCfg& c, const int* q, unsigned seed, unsigned env, unsigned tg, int j, int& dx,
                                             int& dy) {
  ht_move((int)(hkey(seed, HT_MOVE, env, tg, (unsigned)j) % 5u), dx, dy);
  if (!ht_on_grid(c.G, q[HT_X] + dx, q[HT_Y] + dy)) dx = dy = 0;
}
// the reward of a step with these captures and lone attempts: exact in fp32
__host__ __device__ inline float ht_reward(const HuntCfg& c, int captures, int lone) {
  return (float)(HT_CAPTURE4 * captures - c.pen4 * lone) * 0.25f;
}

// ---- features of a slot, from the unit state un and its count tiles
__host__ __device__ inline float ht_ratio(int v, int G) { return (float)v / (float)(G - 1); }
// element k of predator i's observation: the 5 x 5 window centred on it, cell (dy + 2) 5 + (dx + 2), per cell [another predator
// there, a live prey there, off the grid]; then its own x and y ratios
__host__ __device__ inline float ht_obs(const HuntCfg& c, const int* un, const int* pc, const int* qc, int i, int k) {
  const int px = un[i * HT_F + HT_X], py = un[i * HT_F + HT_Y];
  if (k >= HT_O - 2) return ht_ratio(k == HT_O - 2 ? px : py, c.G);
  const int cell = k / 3, f = k - 3 * cell;
  const int row = cell / HT_WIN, dx = cell - HT_WIN * row - HT_WIN / 2, dy = row - HT_WIN / 2;
  const int x = px + dx, y = py + dy;
  if (!ht_on_grid(c.G, x, y)) return f == 2 ? 1.f : 0.f;
  if (f == 0) return pc[ht_cell(c.G, x, y)] - (dx == 0 && dy == 0 ? 1 : 0) > 0 ? 1.f : 0.f;
  if (f == 1) return qc[ht_cell(c.G, x, y)] > 0 ? 1.f : 0.f;
  return 0.f;
}
// element k of the state: per predator its x and y ratios, per prey [live, x ratio, y ratio] (a captured prey: a zero row)
__host__ __device__ inline float ht_state(const HuntCfg& c, const int* un, int k) {
  if (k < 2 * c.N) return ht_ratio(un[(k >> 1) * HT_F + (k & 1 ? HT_Y : HT_X)], c.G);
  k -= 2 * c.N;
  const int j = k / 3, f = k - 3 * j;
  const int* q = un + (c.N + j) * HT_F;
  if (!q[HT_LIVE]) return 0.f;
  return f == 0 ? 1.f : ht_ratio(q[f == 1 ? HT_X : HT_Y], c.G);
}

// ---- the host side of every launcher (hunt.hip)
// hipErrorInvalidValue unless the shape is one the kernels cover; cfg: the feature widths
inline int hunt_cfg(int N, int M, int A, int G, int pen4, long state_ld, int T, HuntCfg& cfg) {
  if (!ht_supported(N, M, G, A) || pen4 < 0 || pen4 > HT_MAX_PEN4 || T < 1) return (int)hipErrorInvalidValue;
  cfg = ht_cfg(N, M, G, pen4);
  return state_ld < cfg.S ? (int)hipErrorInvalidValue : 0;
}
