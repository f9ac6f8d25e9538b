// What the three whole-rollout files share (rollout_fused.hip, rollout_x6.hip, rollout_x6_v1.hip): the agent's hidden width, the
// workgroup, the split kernels' argument struct and plane pitch, and the host side of a launch - the argument fields and checks of
// every launcher, the launch itself, the even-rounds tiling - plus the hidden entry points of the round-5 split kernel
// (rollout_x6_v1.hip) that rollout_x6.hip dispatches to and plans with.
#pragma once
#include "synth_env.h"
#include "../../include/marl_hip.h"

namespace {

constexpr int H = 64;
constexpr int RNT = 512;          // threads per workgroup
constexpr int HP = 72;            // pitch (bf16) of the split kernels' 64-wide planes

// arguments of the split kernels (rollout_x6.hip, rollout_x6_v1.hip); RollArgs (rollout_fused.hip) shares every field but KI
struct RX6Args {
  const float *W1, *b1, *Wih, *Whh, *bih, *bhh, *W2, *b2;
  const float* eps;       // [T] epsilon of each lock-step (device), or null: the schedule below
  double eps0, eps_anneal, eps_min;
  float* stats;           // [3][E] or null: per episode  sum_t r | won | length
  float *obs, *state, *avail;   // (E,T+1,N,O) (E,T+1,SL >= S) (E,T+1,N,A)
  long SL;
  int* u;                 // (E,T,N)
  float *r, *term, *padded;     // (E,T)
  int *length, *won;      // (E)
  float* h_out;           // (E*N,64) final hidden state or null
  unsigned seed, rseed;
  int env0, episode, fixed_len;
  int E, T, N, O, S, A, I, KI;
  int EPW;                // whole environments per workgroup
  int has_act, has_id;
  long R;
};

}  // namespace

// The fields RollArgs and RX6Args share, and the checks every whole-rollout launcher makes (a null record is refused and a batch
// with E or T <= 0 launches nothing: the launchers return before).  0, or hipErrorInvalidValue
template <class Args>
int rollout_args(Args& a, const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0, int episode,
                 int fixed_len, const float* eps, float* h_out, float* stats, double eps0, double eps_anneal, double eps_min,
                 int last_action, int reuse_network) {
  a.E = rec->E; a.T = rec->T; a.N = rec->N; a.O = rec->O; a.S = rec->S; a.A = rec->A; a.SL = rec->state_ld;
  if (w->H != H || a.SL < a.S) return (int)hipErrorInvalidValue;
  // record offsets are 32-bit element offsets inside the kernels
  if ((double)a.E * (a.T + 1) * a.N * (a.O > a.A ? a.O : a.A) >= 2147483648.0 || (double)a.E * (a.T + 1) * a.SL >= 2147483648.0)
    return (int)hipErrorInvalidValue;
  a.W1 = w->fc1_w; a.b1 = w->fc1_b; a.Wih = w->w_ih; a.Whh = w->w_hh; a.bih = w->b_ih; a.bhh = w->b_hh;
  a.W2 = w->fc2_w; a.b2 = w->fc2_b;
  a.eps = eps; a.eps0 = eps0; a.eps_anneal = eps_anneal; a.eps_min = eps_min; a.h_out = h_out; a.stats = stats;
  a.obs = rec->obs; a.state = rec->state; a.avail = rec->avail; a.u = rec->u; a.r = rec->r; a.term = rec->term; a.padded = rec->padded;
  a.length = rec->length; a.won = rec->won;
  a.seed = seed; a.rseed = rseed; a.env0 = env0; a.episode = episode; a.fixed_len = fixed_len;
  a.has_act = last_action ? 1 : 0; a.has_id = reuse_network ? 1 : 0;
  a.I = a.O + (last_action ? a.A : 0) + (reuse_network ? a.N : 0);
  a.R = (long)a.E * a.N;
  return 0;
}

// launch of a whole-rollout kernel: its dynamic LDS, `grid` workgroups of RNT threads, the argument struct; checked
template <class Args>
int launch_rollout(const void* fn, int grid, size_t lds, Args& a, void* stream) {
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {(void*)&a};
  e = hipLaunchKernel(fn, dim3((unsigned)grid), dim3(RNT), kargs, lds, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  MARL_CHECK_LAUNCH();
  return 0;
}

// environments per workgroup of the split kernels: one workgroup per CU while the batch fits one round of 256 workgroups (small
// batches spread over all CUs with partly filled tiles); beyond that as few FULL rounds as epw_max environments per workgroup allow,
// evenly filled
inline int even_rounds_epw(int E, int epw_max) {
  int epw = (E + 255) / 256;
  if (epw > epw_max) {
    const int rounds = (E + 256 * epw_max - 1) / (256 * epw_max);
    epw = (E + 256 * rounds - 1) / (256 * rounds);
    if (epw > epw_max) epw = epw_max;
  }
  return epw;
}

// the round-5 kernel (rollout_x6_v1.hip): the shapes it covers, the environments per workgroup it runs a batch with (KI: input
// width rounded up to 32; 0: none fits), the launch
int marl_rollout_x6_v1_supported(int N, int O, int A);
int marl_rollout_x6_v1_epw(int E, int N, int KI);
int marl_rollout_x6_v1(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0, int episode,
                       int fixed_len, const float* eps, float* h_out, float* stats, double eps0, double eps_anneal, double eps_min,
                       int last_action, int reuse_network, void* stream);
