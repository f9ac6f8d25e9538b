/* marl_hip.h - C ABI of the MI355X (gfx950) hot path for Skylarking/MARL.
 *
 * The reference has no FFI layer (it is pure Python/PyTorch); the functions below are what a
 * binding for its hot path would call, one per fused torch-op sequence.
 * Each entry cites the reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless typed otherwise; row-major; sizes in elements
 *   - `stream` is a hipStream_t passed as void*; nothing synchronises, allocates or frees
 *   - return value: 0 on success, otherwise a hipError_t
 *   - workspaces are caller-provided; *_workspace() gives the byte count
 *   - (B,T,N,*) arrays are episode-major: row = (b*T + t)*N + n
 */
#ifndef MARL_HIP_H
#define MARL_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Virtual row-major matrix [M,K] = [dense0 | dense1 | nhot one-hot blocks | agent-id block].
 * Replaces the th.cat([...]) input builders: controller/share_params.py:84-112,
 * network/mixer.py:151-153 (QPLEX [s|actions]), :380,:386 (QTRAN [h|u], [s|enc]), :416.
 * Row remap (rpe != 0): source row = (row / rpe) * bs + (row % rpe) + off, and a row whose
 * (row % rpe) + off < 0 reads as zero / "no action" (used for (T+1)-slot episode storage and
 * for the one-step-shifted last action). */
typedef struct {
  const float* p0; long ld0; int k0;        /* dense segment 0, k0 columns */
  const float* p1; long ld1; int k1;        /* dense segment 1 */
  const int* idx; int nhot; int hot_w;      /* column j*hot_w + idx[row*nhot + j] = 1 (idx < 0: none) */
  int nid;                                  /* column (row % nid) = 1 */
  const float* m0; long ldm0;               /* optional relu gate on segment 0: v * (m0 > 0) */
  long rpe0, bs0, off0;                     /* row remap for p0 (and m0) */
  long rpei, bsi, offi;                     /* row remap for idx */
  const int* emap0;                         /* optional episode map of the p0 remap (needs rpe0 > 0): episode
                                               e = row / rpe0 reads storage episode emap0[e] - replay samples are
                                               read in place from the ring (common/replaybuffer.py:54-60) */
} marl_src_t;

/* Batched ("grouped") launches over equally shaped problems whose operands sit at a constant
 * element stride (QPLEX's 10 attention heads, network/mixer.py:117-145). 0 = shared operand. */
typedef struct {
  int groups;
  long gs_x0, gs_x1, gs_w, gs_b, gs_y, gs_m0;
} marl_group_t;

/* RNNQNet parameters (network/q_network.py:12-14), torch layouts. */
typedef struct {
  const float *fc1_w, *fc1_b;   /* (H,I), (H)   */
  const float *w_ih, *w_hh;     /* (3H,H) gate order r,z,n */
  const float *b_ih, *b_hh;     /* (3H) */
  const float *fc2_w, *fc2_b;   /* (A,H), (A) */
  int H;                        /* must be 64 */
} marl_agent_weights_t;

/* ---- dense layers on the fp32 matrix cores (gemm.hip) ---------------------------------------
 * Y = act(X W^T + b) [+ beta*Y].  Replaces every nn.Linear(+ReLU) on the path
 * (network/mixer.py:37-55,117-145,200-206,365-375,399-409).  w_kmajor=1 reads W as [K][N]
 * so the same kernel computes dX = dY W (autograd of nn.Linear wrt input). act: 0 none, 1 relu;
 * | 0x100 = round both operands to bf16 and use the bf16 matrix cores (fp32 accumulate) - opt-in for the
 * MIXER layers only (BASELINE config 5 "bf16 mixer with MFMA"; tolerance ~1e-2 instead of 1e-4). */
int marl_linear(const marl_src_t* x, const float* W, long ldw, int w_kmajor, const float* bias,
                float* Y, long ldy, int M, int N, int K, int act, float beta,
                const marl_group_t* grp, void* stream);
/* dW += G^T X, db += colsum(G) with G = dY * (Yact > 0 if Yact). Fixed-order slab reduction.
 * In grp: gs_y = dY stride, gs_m0 = Yact stride, gs_w / gs_b = dW / db strides.  flags: 1 = bf16 operands
 * (as act | 0x100 above). */
int marl_linear_wgrad(const float* dY, long lddy, const float* Yact, long ldya, const marl_src_t* x,
                      float* dW, long lddw, float* db, int M, int N, int K, int flags,
                      const marl_group_t* grp, float* ws, size_t ws_bytes, void* stream);
size_t marl_linear_wgrad_workspace(int M, int N, int K, int groups);
int marl_wgrad_slabs(int M);
/* Launch plans of the two functions above, from the host code the launches themselves decide with.  Host only: no GPU, no device
 * memory touched - only sizes, strides, group strides and the alignment of the pointer VALUES are read (any integer of the right
 * alignment stands for a pointer).  Return 0, or the hipError_t the entry point itself returns for these arguments (then plan is
 * undefined); sizes <= 0 launch nothing and give an all-zero plan (family -1).  Both honour marl_experiment_set.
 * marl_linear_plan, plan[9]:
 *   [0] operand path of the whole 16-column chunks of dense segment 0: 0 element-wise (k0 < 16 or no segment 0), 1 16-byte
 *       vectors, 2 dwords (a row stride, base or group stride of x.p0 - or of the gate x.m0 - off the 16-byte grid)
 *   [1] column tiles per workgroup: 5 for 64 < N <= 80 in fp32, else 4     [2] gate (x.m0 != NULL)     [3] W read k-major
 *   [4] bf16 operands     [5] W read in 16-byte vectors by those chunks in every group (row-major, ldw % 4 == 0, base and group
 *       stride aligned)     [6..8] grid x (128-row blocks), y (column blocks), z (groups)
 * marl_linear_wgrad_plan, plan[8] (ws_bytes as passed to marl_linear_wgrad: it decides the tall kernel's slab count):
 *   [0] family: 0 generic 64 x 64-block kernel, 1 one-pass full-width kernel, 2 direct kernel, 3 direct kernel in column passes,
 *       4 LDS-staged tall kernel, 5 thin one-column kernel
 *   [1], [2] instantiation: direct <KP, NTP> (column passes: 1 and the NTP of the last, plain pass <0, NTP>; every pass before it
 *       is <1, 0>); tall <KTT, NX>; full-width: gate, 0; generic: bf16, 0; thin: 0, 0
 *   [3] passes (kernel + slab-reduce pairs)     [4] slabs of each pass as launched (= grid x, = what the reduce adds up)
 *   [5] gvec, [6] xvec: dY (and Yact) / x.p0 may be read in 16-byte vectors
 *   [7] column passes: the columns the permuted passes cover (64 or 128); else 0 */
int marl_linear_plan(const marl_src_t* x, const float* W, long ldw, int w_kmajor, const float* bias, long ldy,
                     int M, int N, int K, int act, const marl_group_t* grp, int* plan);
int marl_linear_wgrad_plan(const float* dY, long lddy, const float* Yact, long ldya, const marl_src_t* x, int M, int N, int K,
                           int flags, const marl_group_t* grp, size_t ws_bytes, int* plan);

/* ---- agent (agent.hip) ----------------------------------------------------------------------
 * T-step unroll of RNNQNet over B*N rows in ONE launch.  Replaces SharedMAC.get_current_q_values /
 * get_next_q_values (controller/share_params.py:125-168) incl. _build_inputs (:84-112), and with
 * T=1 the network call of SharedMAC.choose_action (:37-63).
 *   obs   : row (b,t,n) at obs + ((b*obs_bs) + (t+obs_t0)*N + n)*O        (obs_bs = rows/episode)
 *   ufed  : int32 action fed back at step t: ufed[b*u_bs + (t+u_t0)*N + n]; none if t+u_t0 < 0,
 *           value < 0 or ufed == NULL (one-hot of zeros, share_params.py:96-100)
 *   ep_len: per-episode int32 length or NULL; observations of steps t >= ep_len[b] read as zeros
 *           (the zero padding rollout.py:122-133 writes, needed when obs is (T+1)-slot storage)
 *   ep_map: per-episode int32 storage index or NULL: batch episode b reads obs of storage episode
 *           ep_map[b] (replay samples read in place, common/replaybuffer.py:54-60); ufed / ep_len / outputs
 *           stay indexed by b
 *   h0    : (B*N,64) or NULL = zeros (init_hidden, :74-76); h_last may alias h0
 *   q (B,T,N,A); hs (B,T,N,64) hidden AFTER each step or NULL; saved = (T+1) * R16 * 6 * 64 floats (R16 = B*N rounded up to
 *   16) or NULL: per row-step the 6 vectors hprev,x,r,z,n,hn for the backward pass, in a tile layout private to the two
 *   kernels ([T][16-row tile][plane][16-column tile][lane][4]: one 16-byte access per lane and plane on both sides)
 *   cu_budget: CUs (= workgroups) a T > 1 launch spreads its rows over, 1..256; 0 = 256 = the whole chip.  With 128
 *           the two independent unrolls of an update - eval current-Q and target next-Q (q_learner.py:97,104) - fit
 *           on the chip together and can be launched on two HIP streams; results do not depend on it (rows are
 *           independent).  A per-call argument: the library keeps no process-wide state.
 *   gi_out: NULL, or T * R16 * 3 * 64 floats (same tile layout): with `saved`, the input-side gate sums bias + x W_ih (r | z | n blocks) of every
 *           row-step are stored as well.
 *   gi_in : NULL, or the gi_out buffer an EARLIER unroll of the same weights wrote for the same rows whose step t+1 input
 *           equals this unroll's step t input for t < T-1 (the double-Q pass after the eval pass, q_learner.py:97-110:
 *           observations shifted by one step, same last actions): fc1 and the input-side gate products of those steps - 288
 *           of a row tile's 496 multiplies per step - are not recomputed; every GRU kernel here accumulates the input-side
 *           products before the hidden-side ones, so the result is bit-identical.  Ragged episodes stay exact: a step t at
 *           which a row of the workgroup has ep_len - 1 == t (the earlier unroll saw the zero padding there, this one sees
 *           the final observation) and the last step are computed in full.  Both pointers are ignored where the kernel
 *           chosen for the shape has no such variant (marl_agent_unroll_reuse_supported). */
int marl_agent_unroll_fwd(const marl_agent_weights_t* w, const float* obs, long obs_bs, int obs_t0,
                          const int* ufed, long u_bs, int u_t0, const int* ep_len, const int* ep_map,
                          const float* h0, float* q, float* hs, float* h_last, float* saved, int B, int T,
                          int N, int O, int A, int last_action, int reuse_network, int cu_budget,
                          float* gi_out, const float* gi_in, void* stream);
int marl_agent_unroll_reuse_supported(int B, int T, int N, int O, int A, int cu_budget);

/* Gradient destinations of the recurrent / output layers (accumulated into, torch layouts). */
typedef struct {
  float *w_ih, *w_hh;           /* (3H,H) */
  float *b_ih, *b_hh;           /* (3H)   */
  float *fc2_w, *fc2_b;         /* (A,H), (A) */
} marl_agent_grads_t;

/* BPTT (autograd of the unroll above; q_learner.py:171 loss.backward()), fused: per step the delta
 * pass AND the weight-gradient reductions of W_ih, W_hh, W_2 and their biases (in-register
 * accumulators, one partial slab per workgroup in `ws`, fixed-order reduce => reproducible).
 *   dq (B,T,N,A) gradient on q, OR (dq_idx != NULL) its sparse form: row (b,t,n) has the single non-zero
 *   dq_val[b,t,n] in column dq_idx[b,t,n] (the TD loss reaches q only through th.gather, q_learner.py:100;
 *   the dense tile is then never materialised); dq_idx2 / dq_val2: optional SECOND pair per row (QTRAN reaches q through the
 *   taken and the greedy action, qtran_learner.py:139,145; equal columns add); dq_gdiv > 1: the values are indexed by
 *   row / dq_gdiv (N: one value per (episode, step), shared by its agents - autograd of .sum(dim=-1));
 *   dhs (B,T,N,64) extra gradient on hs or NULL (QTRAN heads)
 *   saved: output of the forward pass (it holds h(t) as well; `hs` is not read any more and may be NULL);
 *   dxp (B,T,N,64) = gradient at the fc1 pre-activation
 * The fc1 gradient follows as ONE marl_linear_wgrad over dxp and the virtual input [obs|u|id]. */
size_t marl_agent_bwd_workspace(int B, int N, int A);
int marl_agent_unroll_bwd(const marl_agent_weights_t* w, const float* dq, const int* dq_idx,
                          const float* dq_val, const int* dq_idx2, const float* dq_val2, int dq_gdiv, const float* dhs,
                          const float* saved, const float* hs, float* dxp, float* dh0,
                          const marl_agent_grads_t* g, float* ws, size_t ws_bytes,
                          int B, int T, int N, int A, void* stream);

/* ---- per-row kernels (mixers.hip) -----------------------------------------------------------*/
/* out[row] = q[row,idx[row]] (th.gather, q_learner.py:100,114); idx < 0 -> 0.  With avail != NULL the
 * value read is the masked one: avail[row,idx]==0 ? mask_val : q (q_learner.py:105 then :114). */
int marl_q_gather(const float* q, const int* idx, const float* avail, float mask_val, float* out,
                  long rows, int A, void* stream);
/* q[avail==0] = mask_val; max / first-index argmax over actions (q_learner.py:105,112-117,125-127;
 * qtran_learner.py:104-113). avail may be NULL. out_max / out_arg may be NULL. */
int marl_q_masked_max(const float* q, const float* avail, float mask_val, float* out_max, int* out_arg,
                      long rows, int A, void* stream);
/* Double-Q selection in one pass (q_learner.py:104-117): arg[row] = first-index argmax of q_sel masked with
 * avail (mask_val where avail == 0), out_val[row] = q_val[row, arg] masked the same way; out_arg may be NULL; avail may be NULL
 * (everything available).  Serves every action count: up to A = 21 a wave stages 64 rows of the three operands through LDS, from
 * A = 22 on (the tiles of four waves would exceed 64 KiB) one thread scans a row - same comparisons, same results bit for bit. */
int marl_q_double_select(const float* q_sel, const float* q_val, const float* avail, float mask_val,
                         float* out_val, int* out_arg, long rows, int A, void* stream);
/* dq = 0; dq[row,idx1[row]] += g1[row/gdiv]; dq[row,idx2[row]] += g2[row/gdiv] (idx2/g2 may be
 * NULL): autograd of gather / max (+ of the sum over agents when gdiv = N). */
int marl_q_scatter(float* dq, const int* idx1, const float* g1, const int* idx2, const float* g2,
                   long rows, int A, int gdiv, void* stream);
/* out = a + b (q_tot = v_tot + a_tot, q_learner.py:135,154) */
int marl_vec_add(const float* a, const float* b, float* out, long n, void* stream);
/* out[r,d] = sum_n in[r,n,d]   (VDNMixer, mixer.py:15-16 with D=1; QTRAN .sum(dim=-2), :384,:414); ld_in / ld_out =
 * row strides (>= D) of the (rows*N, D) input and the (rows, D) output */
int marl_agent_sum(const float* in, long ld_in, float* out, long ld_out, long rows, int N, int D, void* stream);
/* out[r,n,d] = in[r,d] (+ out if accumulate): autograd of the sum above */
int marl_agent_bcast(const float* in, long ld_in, float* out, long ld_out, long rows, int N, int D, int accumulate,
                     void* stream);

/* QMixMixer.forward after the hypernet layers (mixer.py:64-80).  hy row = [w1raw (N*E, agent-major)
 * | b1 (E) | w2raw (E) | relu(hyper_b2.0) (E)].  b2 (rows) = hyper_b2.2 output, or NULL: then it is formed in the kernel from the
 * fourth block, b2 = w22 . hb + b22 (w22 (E), b22 (1): hyper_b2.2's weight and bias, mixer.py:46-47). */
int marl_qmix_mix_fwd(const float* hy, long ldh, const float* b2, const float* w22, const float* b22, const float* q,
                      float* q_tot, long rows, int N, int E, void* stream);
/* its autograd: fills dhy[w1raw|b1|w2raw], db2 (= dq_tot), dq; the 4th block of dhy is written by the caller, or here when w22 is
 * given: d hb = dq_tot w22 (hb > 0) - the backward of hyper_b2.2 and its relu */
int marl_qmix_mix_bwd(const float* hy, long ldh, const float* q, const float* dq_tot, const float* w22, float* dhy,
                      float* db2, float* dq, long rows, int N, int E, void* stream);
/* The state-conditioned bias layers of QMixMixer in one pass over s, written into hy (rows, ldhy):
 * hy[:, c_b1 : c_b1 + 32] = hyper_b1(s), hy[:, c_h : c_h + 32] = relu(hyper_b2.0(s)) (mixer.py:44-47; E = 32).  Wb1, Wh: (32, S)
 * weights with the same row stride; s as in marl_qtran_state_parts.  With marl_qmix_mix_fwd(b2 = NULL) the generic mixer path
 * (two_hyper_layers, mixer.py:36-43) launches no marl_linear. */
int marl_qmix_tail_fwd(const marl_src_t* s, long rows, int S, const float* Wb1, long ldb1, const float* bb1, const float* Wh,
                       long ldwh, const float* bh, float* hy, long ldhy, int c_b1, int c_h, void* stream);

/* Fused QMIX (qmix_fused.hip): hypernet GEMMs + mixing in one kernel; the backward recomputes the
 * hypernet tile and accumulates the hypernet weight gradients in registers.  Supported when
 * marl_qmix_fused_supported(N, S, E) (E == 32, N*E+3E <= 256, S <= 128); otherwise compose
 * marl_linear + marl_qmix_mix_*.  `s` must be a dense-segment-0 source (row remap allowed). */
typedef struct {
  const float *w1, *w1_b;       /* hyper_w1   (N*E,S), (N*E) */
  const float *b1, *b1_b;       /* hyper_b1   (E,S), (E)     */
  const float *w2, *w2_b;       /* hyper_w2   (E,S), (E)     */
  const float *h, *h_b;         /* hyper_b2.0 (E,S), (E)     */
  const float *b2_w, *b2_b;     /* hyper_b2.2 (1,E), (1)     */
} marl_qmix_weights_t;
int marl_qmix_fused_supported(int N, int S, int E);
size_t marl_qmix_fused_workspace(long rows, int N, int S);
int marl_qmix_fused_fwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, float* q_tot,
                        long rows, int N, int S, int E, void* stream);
/* grads: same struct, pointing at the gradient tensors (accumulated into) */
int marl_qmix_fused_bwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* dq_tot,
                        float* dq, const marl_qmix_weights_t* grads, float* ws, size_t ws_bytes, long rows,
                        int N, int S, int E, void* stream);
/* The same backward with the TD loss of q_learner.py:112-127 folded in (the backward pass recomputes q_tot anyway, so the eval
 * mixer's forward launch, marl_td_loss and its reduction are not needed): per row target = r + gamma q_tot_tgt (1 - term),
 * td = mask (target - q_tot), dL/dq_tot = -2 mask td with mask = 1 - padded.  loss2[0] += sum td^2, loss2[1] += sum mask
 * (un-normalised; fixed summation order); q_tot (rows) is written when not NULL. */
int marl_qmix_fused_loss_bwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* q_tot_tgt,
                             const float* r, const float* term, const float* padded, float gamma, float* q_tot,
                             float* dq, const marl_qmix_weights_t* grads, float* loss2, float* ws, size_t ws_bytes,
                             long rows, int N, int S, int E, void* stream);
/* The same three entry points with the two GEMMs of a tile - hypernet output (network/mixer.py:60-77) and the hypernet weight
 * gradient - as bf16x6 split products (args.gemm_mode = "bf16x6"; see the agent_x6 / mlp3_x6 blocks for the arithmetic: every fp32
 * operand split exactly into three bf16 terms, six bf16 MFMA products per fp32 product, fp32 accumulate).  Same arguments, same
 * workspace, same supported shapes, same epilogue arithmetic; results differ from the fp32-MFMA entry points by summation order
 * and the dropped <= 2^-24 terms only. */
int marl_qmix_fused_fwd_x6(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, float* q_tot,
                           long rows, int N, int S, int E, void* stream);
int marl_qmix_fused_bwd_x6(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* dq_tot,
                           float* dq, const marl_qmix_weights_t* grads, float* ws, size_t ws_bytes, long rows,
                           int N, int S, int E, void* stream);
int marl_qmix_fused_loss_bwd_x6(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* q_tot_tgt,
                                const float* r, const float* term, const float* padded, float gamma, float* q_tot,
                                float* dq, const marl_qmix_weights_t* grads, float* loss2, float* ws, size_t ws_bytes,
                                long rows, int N, int S, int E, void* stream);

/* Fused QMIX for WIDE states (qmix_wide.hip; MMM2: S = 322, N = 10 -> a 416 x 322 concatenated hypernet that does not fit
 * the registers-resident design above): the weights are packed per call into MFMA-fragment order (L2 resident) and
 * streamed against 64-row state tiles in LDS; same arithmetic, same gradient destinations.  `s`: dense segment 0 whose
 * rows start on 16-byte boundaries and hold S rounded up to 4 readable floats (EpisodeRecord pads the state row stride).
 * flags & 1: bf16 operands for the hypernet GEMM (v_mfma_f32_16x16x32_bf16, fp32 accumulate; BASELINE config 5 "bf16
 * mixer with MFMA") - the forward kernel is then bound by reading the states from HBM; mixing arithmetic and gradients stay
 * fp32.  flags & 2 (backward entry points, only together with flags & 1): the weight-gradient GEMM dW += dhy^T s also takes
 * bf16 operands (dhy - a gradient - and the states rounded to bf16 where a 32-row chunk is staged; fp32 accumulate; the bias
 * gradient stays an exact fp32 column sum): the four hypernet weight gradients then carry ~2e-3 relative error; without the
 * bit that GEMM is fp32 (v_mfma_f32_16x16x4_f32).  Workspace: packed weights (+ for backward: d(hypernet output) rows x (N*E+3E)
 * and the slabs).  Supported when marl_qmix_wide_supported(N, S, E) (E == 32, N <= 10, S <= 384).
 * CONTRACT on the row padding: the kernels read the columns S .. 4 ceil(S / 4) - 1 of every state row (the 16-byte loads of the
 * last chunk) and multiply them by packed weights that are exactly zero, so these pad columns must hold FINITE values (0 * NaN
 * would poison q_tot); EpisodeRecord zero-initialises them, a caller with its own buffers must do the same.
 * marl_qmix_wide_fwd_kernel(): the name prefix (rocprofv3 kernel trace) of the forward kernel a call with this shape launches -
 * "qmix_wide_kernel<false" (streaming) or "qmix_wide_res_fwd_kernel" (bf16, weights resident in LDS: preceded by the pack kernel and
 * a memset of q_tot). */
int marl_qmix_wide_supported(int N, int S, int E);
const char* marl_qmix_wide_fwd_kernel(long rows, int N, int S, int flags);
size_t marl_qmix_wide_workspace(long rows, int N, int S, int backward);
int marl_qmix_wide_fwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, float* q_tot, float* ws,
                       size_t ws_bytes, long rows, int N, int S, int E, int flags, void* stream);
int marl_qmix_wide_bwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* dq_tot, float* dq,
                       const marl_qmix_weights_t* grads, float* ws, size_t ws_bytes, long rows, int N, int S, int E,
                       int flags, void* stream);
/* marl_qmix_wide_bwd with the TD loss folded in (see marl_qmix_fused_loss_bwd): q_tot of a row is complete inside one wave of
 * the backward kernel, so dL/dq_tot is formed there; loss2[0] += sum (mask td)^2, loss2[1] += sum mask; q_tot optional. */
int marl_qmix_wide_loss_bwd(const marl_qmix_weights_t* w, const marl_src_t* s, const float* q, const float* q_tot_tgt,
                            const float* r, const float* term, const float* padded, float gamma, float* q_tot, float* dq,
                            const marl_qmix_weights_t* grads, float* loss2, float* ws, size_t ws_bytes, long rows,
                            int N, int S, int E, int flags, void* stream);

/* ---- fused three-layer heads (mlp3_fused.hip) -----------------------------------------------
 * Y[:, g*gs_y + 0..N3) = W3_g relu(W2_g relu(W1_g x + b1_g) + b2_g) + b3_g for `groups` equally shaped heads
 * with hidden width 64 whose parameters sit at constant element strides: the key / agents / action extractors
 * of DMAQ_SI_Weight (network/mixer.py:117-145, evaluated at :155-169 - 10 heads x 3 families per mixer call).
 * One kernel per family: the 64-wide hidden activations never leave the CU (composed from marl_linear they
 * cross HBM four times per update).  x: [dense0 | dense1 | one-hot blocks], shared by all heads; no gate / id
 * block.  The backward recomputes the hidden activations, keeps the weight gradients of a stripe of rows in
 * registers and accumulates them (fixed-order slab reduction) into `grads` (same struct, gradient tensors);
 * inputs get no gradient (states / actions).  Use when marl_mlp3_supported(); otherwise compose marl_linear.
 * w2 == NULL (H2 = 0 in marl_mlp3_supported): two-layer heads y = W3 relu(W1 x + b1) + b3 - the transformation nets
 * hyper_w_final / V of DMAQer (network/mixer.py:200-206), evaluated as one launch with groups = 2. */
typedef struct {
  const float *w1, *b1;         /* (64,K1), (64) of head 0 */
  const float *w2, *b2;         /* (64,64), (64)           */
  const float *w3, *b3;         /* (N3,64), (N3)           */
  long gs_w1, gs_b1, gs_w2, gs_b2, gs_w3, gs_b3;   /* element strides between consecutive heads */
} marl_mlp3_weights_t;
int marl_mlp3_supported(const marl_src_t* x, int K1, int H1, int H2, int N3, int groups);
int marl_mlp3_fwd(const marl_mlp3_weights_t* w, const marl_src_t* x, float* Y, long ldy, long gs_y,
                  long M, int K1, int N3, int groups, void* stream);
size_t marl_mlp3_bwd_workspace(long M, int K1, int N3, int groups);
int marl_mlp3_bwd(const marl_mlp3_weights_t* w, const marl_src_t* x, const float* dY, long lddy, long gs_dy,
                  const marl_mlp3_weights_t* grads, float* ws, size_t ws_bytes, long M, int K1, int N3,
                  int groups, void* stream);
/* The same pair with the hidden activations KEPT between forward and backward instead of recomputed (what autograd
 * does for these heads in the reference, network/mixer.py:149-171): the forward writes relu(h1) [and relu(h2)] of
 * every 16-row tile as the MFMA fragments the backward wants (`hsave`: marl_mlp3_save_floats(M, three, groups)
 * floats, layout private to the pair), the backward reads them back with 16-byte coalesced loads and skips layers
 * 1-2.  Same values as the recomputing pair (outputs bit-identical; the gradients are sums over another number of row
 * stripes).  hsave == NULL: exactly marl_mlp3_fwd / marl_mlp3_bwd. */
size_t marl_mlp3_save_floats(long M, int three, int groups);
/* Wide outputs: two-layer heads (w2 == NULL) take 16 < N3 <= 160 outputs, N3 a multiple of 4 (hyper_w1 / hyper_w2 of QMixMixer
 * with two_hyper_layers, network/mixer.py:36-43: state -> 64 -> n_agents * embed); a wider head is evaluated as `groups` column
 * blocks that share layer 1 (gs_w1 = gs_b1 = 0: those gradients are then summed over the groups).
 * 1 when the backward of this shape exists only as marl_mlp3_bwd_saved with hsave != NULL (N3 > 16, or K1 > 192, e.g. the heads of
 * DMAQ_SI_Weight on MMM2: state 322 [+ 10 x 18 one-hot actions], network/mixer.py:117-145): W1 no longer fits in LDS beside the
 * operand exchange, so layer 1 is not recomputed. */
int marl_mlp3_needs_kept(const marl_src_t* x, int K1, int N3);
int marl_mlp3_fwd_save(const marl_mlp3_weights_t* w, const marl_src_t* x, float* Y, long ldy, long gs_y,
                       float* hsave, size_t hsave_floats, long M, int K1, int N3, int groups, void* stream);
int marl_mlp3_bwd_saved(const marl_mlp3_weights_t* w, const marl_src_t* x, const float* dY, long lddy, long gs_dy,
                        const marl_mlp3_weights_t* grads, float* ws, size_t ws_bytes, const float* hsave,
                        size_t hsave_floats, long M, int K1, int N3, int groups, void* stream);

/* ---- agent unroll, forward, with the multiplies as an fp32-accurate split on the bf16 matrix cores (agent_x6.hip) ----------------
 * Opt-in (args.gemm_mode = "bf16x6"): the same T-step unroll as marl_agent_unroll_fwd (controller/share_params.py:147-168;
 * network/q_network.py:16-21) with every fp32 product as six bf16 MFMA products (see the mlp3_x6 block below for the arithmetic).
 * Same arguments, same meaning: `saved` (the six activation planes per row-step the fp32 BPTT kernel marl_agent_unroll_bwd reads,
 * same tile layout), `gi_out` / `gi_in` (the input-side gate sums one unroll stores and the double-Q continuation reads; these
 * hold PLAIN sums here - a pair of launches that shares them must both be this entry), `cu_budget` (two row tiles per workgroup
 * once there are more tiles than that many CUs).  marl_agent_unroll_x6_supported(), exactly: H = 64; 8 <= O <= 192 and O a multiple
 * of 8 (a row tile's observations fit three 16-byte prefetch registers per thread of one team); input width
 * I = O + (last_action ? A : 0) + (reuse_network ? N : 0) <= 224; 1 <= A <= 16, or <= 32 when I > 160 (two action tiles only in the
 * widest instantiation); T >= 4; B T N 256 < 2^32 (32-bit offsets): 2s3z-, 3s5z- and MMM2-sized agents; beyond 96 input columns one row
 * tile per workgroup.  The entry point also wants obs on a 16-byte boundary.  The caller uses marl_agent_unroll_fwd otherwise. */
int marl_agent_unroll_x6_supported(int B, int T, int N, int O, int A, int last_action, int reuse_network);
/* 1 when a NON-SAVING launch of marl_agent_unroll_fwd_x6 on this batch (saved = gi_in = hs = NULL: the target network's unroll and the
 * double-Q continuation of reference q_learner.py:104-110) runs on the round-6 decomposition (csrc/agent_x6p.hip: the recurrent team
 * multiplies x W_ih and h W_hh in one chain, five row tiles per workgroup, two barriers per step): whole-chip launches (cu_budget 0 /
 * 256) of more than 512 row tiles of 2s3z-sized agents (<= 96 input columns, <= 16 actions), given h0 and h_last on 16-byte boundaries
 * (other alignments run on csrc/agent_x6.hip).  The learner then keeps no input-side gate sums (gi_out / gi_in) for that batch. */
int marl_agent_unroll_x6_plain_r6(int B, int T, int N, int O, int A, int last_action, int reuse_network, int cu_budget);
int marl_agent_unroll_fwd_x6(const marl_agent_weights_t* w, const float* obs, long obs_bs, int obs_t0,
                             const int* ufed, long u_bs, int u_t0, const int* ep_len, const int* ep_map,
                             const float* h0, float* q, float* hs, float* h_last, float* saved, int B, int T, int N,
                             int O, int A, int last_action, int reuse_network, int cu_budget, float* gi_out,
                             const float* gi_in, void* stream);

/* ---- which kernel a forward unroll runs (host only: no GPU, no launch) ------------------------------------------------------------
 * The launch plan of marl_agent_unroll_fwd (x6 = 0) or marl_agent_unroll_fwd_x6 (x6 = 1) for these dimensions, taken from the
 * same host function the launch itself calls.  `flags` says what the caller would pass: */
#define MARL_UNROLL_SAVED 1        /* saved != NULL */
#define MARL_UNROLL_GI_OUT 2       /* gi_out != NULL */
#define MARL_UNROLL_GI_IN 4        /* gi_in != NULL */
#define MARL_UNROLL_HS 8           /* hs != NULL */
#define MARL_UNROLL_OBS_ALIGNED 16 /* obs on a 16-byte boundary */
#define MARL_UNROLL_H_ALIGNED 32   /* h0 and h_last each NULL or on a 16-byte boundary */
/* Returns 0 and fills plan[8], or non-zero where the entry point would refuse the call (and for B <= 0 or T <= 0, where it launches
 * nothing):
 *   plan[0] kernel family: */
#define MARL_UNROLL_F32_PIPE 0     /* agent.hip: agent_fwd_pipe_kernel, software-pipelined */
#define MARL_UNROLL_F32_MULTI 1    /* agent.hip: agent_fwd_kernel, the multi-tile kernel */
#define MARL_UNROLL_X6 2           /* agent_x6.hip */
#define MARL_UNROLL_X6_R6 3        /* agent_x6p.hip: the round-6 decomposition */
/*   plan[1] row tiles (16 rows) per workgroup
 *   plan[2] workgroups
 *   plan[3] workgroups that hold plan[1] whole tiles.  fp32 and round-6: tiles / plan[1], the last workgroup holds what is left.
 *           agent_x6.hip: its n_full argument - the workgroups after the first plan[3] hold ONE tile each (the last round of a
 *           launch that runs in rounds); with two tiles per workgroup and plan[3] == plan[2] an odd tile count leaves the last
 *           workgroup without a second tile
 *   plan[4] action tiles of fc2 (1: A <= 16 columns, 2)
 *   plan[5] fc1 chunks: 16-column chunks of the input for the fp32 kernels (KC), 32-column chunks for the split kernels (3, 5, 7)
 *   plan[6] how a step's observations are read: */
#define MARL_UNROLL_IN_ELEMENT 0   /* float by float (O % 4 != 0 or obs not 16-byte aligned) */
#define MARL_UNROLL_IN_VECTOR 1    /* 16-byte vectors through the prefetch registers */
#define MARL_UNROLL_IN_HALF 2      /* ... one column half of the tile at a time (wide observations) */
#define MARL_UNROLL_IN_W2L 3       /* ... six prefetch registers, fc2 fragments in LDS (saving, wide observations, two action tiles) */
/*   plan[7] 1 when the launch really reads gi_in (0: it computes every step itself) */
int marl_agent_unroll_fwd_plan(int x6, int B, int T, int N, int O, int A, int last_action, int reuse_network, int cu_budget,
                               int flags, int* plan);

/* ---- BPTT of the unroll on the same split arithmetic (agent_bwd_x6.hip) -------------------------------------------------------
 * Opt-in (args.gemm_mode = "bf16x6"): marl_agent_unroll_bwd with every fp32 product - the delta pass and the weight-gradient
 * reductions over rows - as six bf16 MFMA products; bias gradients are exact fp32 sums.  Same argument meaning (no dense dq and no
 * `hs`: the Q-learning losses reach q through one or two (column, value) pairs per row); `saved` is what either forward entry
 * stored.  marl_agent_unroll_bwd_x6_supported(): H = 64, A <= 32, sparse dq, T >= 3; the caller uses marl_agent_unroll_bwd
 * otherwise.  Workspace: marl_agent_bwd_x6_workspace() bytes (one slab per 32 rows). */
int marl_agent_unroll_bwd_x6_supported(int B, int T, int N, int A, int sparse_dq);
size_t marl_agent_bwd_x6_workspace(int B, int N, int A);
int marl_agent_unroll_bwd_x6(const marl_agent_weights_t* w, const int* dq_idx, const float* dq_val, const int* dq_idx2,
                             const float* dq_val2, int dq_gdiv, const float* dhs, const float* saved, float* dxp, float* dh0,
                             const marl_agent_grads_t* g, float* ws, size_t ws_bytes, int B, int T, int N, int A, void* stream);

/* ---- the same heads with the multiplies as an fp32-accurate SPLIT on the bf16 matrix cores (mlp3_x6.hip) -------------
 * Opt-in (args.gemm_mode = "bf16x6"; the default is the pair above on v_mfma_f32_16x16x4_f32).  Every fp32 operand is split
 * exactly into three bf16 terms (hi + mid + lo) and a product is the six bf16 products hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid
 * accumulated in fp32 by v_mfma_f32_16x16x32_bf16: the error against fp64 is that of the fp32 MFMA path (dropped terms <= 2^-24 of a
 * product), at 0.4 of its matrix-pipe time.  Same math as marl_mlp3_fwd_save / marl_mlp3_bwd_saved (network/mixer.py:117-145,
 * :149-171) for THREE-layer heads (w2 != NULL, H1 = H2 = 64) with N3 <= 16 outputs that marl_mlp3_supported() covers, whose virtual input
 * width KV = K1 + (the kernels' own padding of a dense segment 0 that is not a multiple of 4) satisfies KV < 16 KC with
 * KC = 4 ceil(KV / 64) <= 12: at most 191 columns, and the last 64-column block must leave a free column (KV = 112 is accepted, 64 /
 * 128 / 192 are not) - the first free column carries the ones that produce the layer-1 bias gradient.  `hsave`: marl_mlp3_save_floats(M, 1, groups) floats in the
 * layout of the fp32 pair (the kept fp32 activations; the backward splits them).  hsave == NULL in the forward: nothing is kept
 * (target mixer).  Workspace: marl_mlp3_bwd_workspace(). */
int marl_mlp3_x6_supported(const marl_src_t* x, int K1, int H1, int H2, int N3, int groups);
int marl_mlp3_x6_fwd_save(const marl_mlp3_weights_t* w, const marl_src_t* x, float* Y, long ldy, long gs_y,
                          float* hsave, size_t hsave_floats, long M, int K1, int N3, int groups, void* stream);
int marl_mlp3_x6_bwd_saved(const marl_mlp3_weights_t* w, const marl_src_t* x, const float* dY, long lddy, long gs_dy,
                           const marl_mlp3_weights_t* grads, float* ws, size_t ws_bytes, const float* hsave,
                           size_t hsave_floats, long M, int K1, int N3, int groups, void* stream);
/* The launch plan of one of the four calls above for these arguments - a host function: no GPU, nothing is launched, and the pointers
 * (in w, grads and x too) may be integers standing for addresses: only their alignment and whether they are NULL is read.
 * what: 0 marl_mlp3_fwd_save, 1 marl_mlp3_bwd_saved, 2 marl_mlp3_x6_fwd_save, 3 marl_mlp3_x6_bwd_saved; Y / ldy / gs_y are dY's for
 * the backwards, grads / ws_bytes are read by the backwards only; M >= 1.  These are the host functions the launches themselves
 * decide with.  Returns 0, or an error where the entry point refuses the call (plan[0] = 1).  plan[19]:
 *   [0] refused   [1] KC chunk bucket  [2] CF leading 16-byte chunks (runtime)  [3] compile-time CF variant, -1 if none
 *   [4] kpad  [5] KV = K1 + kpad  [6] three-layer  [7] WIDE  [8] n3t output tiles  [9] kept (forward: writes hsave; backward: reads it)
 *   [10] KH chunks of x^T per stage pass  [11] stage passes (forwards: KC, 1)  [12] workgroups per CU (1 / 2)
 *   [13] nst stripes per group  [14] units per stripe (forwards: 16-row tiles; backwards: 64-row iterations)  [15] grid
 *   [16] dynamic LDS bytes  [17] yvec (forwards)  [18] slabs per group the reduce sums (backwards) */
int marl_mlp3_plan(int what, const marl_mlp3_weights_t* w, const marl_src_t* x, const void* Y, long ldy, long gs_y,
                   const marl_mlp3_weights_t* grads, size_t ws_bytes, const void* hsave, size_t hsave_floats, long M, int K1,
                   int N3, int groups, int* plan);

/* ---- fused QTRAN-base heads (qtran_fused.hip) ------------------------------------------------
 * QtranQBase.forward (network/mixer.py:378-388, A = n_actions > 0, AE = 64 + A) and QtranV.forward (:411-418, A = 0,
 * AE = 64):  out[bt] = q( [s | sum_n enc([h_n | onehot(u_n)])] ).  The per-agent encoder activations never leave the
 * CU; the second encoder layer is applied AFTER the agent sum (it is linear): esum = W_enc2 (sum_n e1_n) + N b_enc2.
 *   hidden (BT*N, 64) agent rows (bt, n) at bt*N + n; u (BT*N) int32 action index (< 0: all-zero one-hot) or NULL
 *   when A = 0; sp (BT, 64) = W_q0[:, :S] s + b_q0 - the state part of the head's first layer, one marl_linear call,
 *   shared by evaluations of the same network on the same states (taken / greedy actions, qtran_learner.py:116,133).
 *   s1, e2 (BT, AEP), y1, y2 (BT, 64), AEP = AE rounded up to 16 (pad columns are written as zeros): saved
 *   activations for the backward pass (sum_n relu(e1_n), esum, the two hidden layers), all four or none (NULL).
 * Backward: given d_out (BT) writes the row-level gradients dy2, dy1 (BT, 64), de2 (BT, AEP) - the callers feed them
 * to marl_linear_wgrad for W_q4, W_q2, W_q0 and W_enc2 (reductions over BT rows) - and the gradient on hidden
 * (dhidden = or +=), and ACCUMULATES the gradients the agent-level pass owns: d_enc0_w (AE, AE), d_enc0_b (AE) and
 * d_enc2_b (AE) (= N * colsum(de2)).  Slabs + fixed-order reduce: bitwise reproducible.
 * Use when marl_qtran_supported(N, A, AE) (A <= 16, hidden widths 64); otherwise compose marl_linear. */
typedef struct {
  const float *enc0_w, *enc0_b;   /* hidden(_action)_encoding.0  (AE, AE), (AE) */
  const float *enc2_w, *enc2_b;   /* hidden(_action)_encoding.2  (AE, AE), (AE) */
  const float* q0_w; long q0_ld; int q0_s;   /* q.0 / v.0 weight (64, S + AE), its row stride, S */
  const float *q2_w, *q2_b;       /* q.2 / v.2  (64, 64), (64) */
  const float *q4_w, *q4_b;       /* q.4 / v.4  (1, 64), (1)   */
} marl_qtran_weights_t;
int marl_qtran_supported(int N, int A, int AE);
int marl_qtran_head_fwd(const marl_qtran_weights_t* w, const float* hidden, const int* u, const float* sp, float* out,
                        float* s1, float* e2, float* y1, float* y2, long BT, int N, int A, int AE, void* stream);
/* The joint-Q head on the same states and hidden states for two action sets in one launch: out <- u (activations saved as in
 * marl_qtran_head_fwd), out2 <- u2 (nothing saved): the taken and the greedy actions of the eval mixer, qtran_learner.py:116
 * and :133.  The encoder's first-layer product is computed once.  A > 0 only. */
int marl_qtran_head_fwd2(const marl_qtran_weights_t* w, const float* hidden, const int* u, const int* u2, const float* sp,
                         float* out, float* out2, float* s1, float* e2, float* y1, float* y2, long BT, int N, int A, int AE,
                         void* stream);
size_t marl_qtran_bwd_workspace(long BT, int AE);
int marl_qtran_head_bwd(const marl_qtran_weights_t* w, const float* hidden, const int* u, const float* d_out,
                        const float* y1, const float* y2, float* dy1, float* dy2, float* de2, float* dhidden,
                        int accumulate, float* d_enc0_w, float* d_enc0_b, float* d_enc2_b, float* ws, size_t ws_bytes,
                        long BT, int N, int A, int AE, void* stream);

/* State parts of the heads' first layers: sp_k (BT, 64) = W_k[:, :S] s + b_k for k < nsets (1 or 2) - the `sp` argument of
 * marl_qtran_head_fwd.  The joint-Q head and the V head of one update read the same states (qtran_learner.py:116-118):
 * nsets = 2 serves both from one pass over s.  W_k: q.0 / v.0 weight (64, ldw_k), ldw_k >= S; s: BT rows of S columns as
 * one dense segment (p0, ld0 % 4 == 0, 16-byte aligned; the row remap and the episode map of marl_src_t are honoured -
 * the learner reads s and s_next in place from the (T+1)-slot storage; S % 4 != 0 reads the row's last 16 bytes, whose pad
 * must be finite).  Use when marl_qtran_state_parts_supported(S) (S <= 384); otherwise marl_linear. */
int marl_qtran_state_parts_supported(int S);
int marl_qtran_state_parts(const marl_src_t* s, long BT, int S, int nsets, const float* W0, long ldw0, const float* b0, float* sp0,
                           const float* W1, long ldw1, const float* b1, float* sp1, void* stream);
/* Every weight gradient of one head that is a reduction over the BT rows, in one pass (network/mixer.py:381,386-387 /
 * :412,416-417; replaces five marl_linear_wgrad calls on tensors marl_qtran_head_fwd / _bwd have written):
 *   d_q0_w (64, ld_q0) += dy1^T [s | e2[:, :AE]]   d_q0_b += colsum(dy1)   d_q2_w (64,64) += dy2^T y1   d_q2_b += colsum(dy2)
 *   d_q4_w (64) += d_out^T y2   d_q4_b (1) += sum(d_out)   d_enc2_w (AE, AE) += de2[:, :AE]^T s1[:, :AE]
 * s as in marl_qtran_state_parts; s1, e2, de2 (BT, AEP); y1, y2, dy1, dy2 (BT, 64); d_out (BT).  ws: marl_qtran_wgrad_rows_workspace(S, AE)
 * bytes.  Slabs + fixed-order reduce: bitwise reproducible.  Use when marl_qtran_wgrad_rows_supported(S, AE)
 * (S % 4 == 0, S <= 384, AE = 64 + A with A <= 16). */
int marl_qtran_wgrad_rows_supported(int S, int AE);
size_t marl_qtran_wgrad_rows_workspace(int S, int AE);
int marl_qtran_wgrad_rows(const marl_src_t* s, const float* s1, const float* e2, const float* y1, const float* y2,
                          const float* d_out, const float* dy1, const float* dy2, const float* de2, float* d_q0_w, long ld_q0,
                          float* d_q0_b, float* d_q2_w, float* d_q2_b, float* d_q4_w, float* d_q4_b, float* d_enc2_w, float* ws,
                          size_t ws_bytes, long BT, int S, int AE, void* stream);
/* The launch plan of the entry points of qtran_fused.hip for these sizes, from the host functions the launches themselves decide
 * with.  Host only: no GPU, no pointer is read (alignment refusals are the entry points' own).  Arguments a query does not use are
 * ignored.  Returns 0 and fills plan[8], or the hipError_t the entry point returns for these sizes; BT <= 0 launches nothing:
 * all-zero plan.
 *   FWD / FWD2 / BWD (BT, N, A, AE): marl_qtran_head_fwd, _fwd2, _bwd
 *     plan[0] FT feature tiles of the encoder (5 <-> qtran_*_kernel<5, ..>, 4)   plan[1] HOT: one-hot table   plan[2] DUAL: two action sets
 *     plan[3] workgroups   plan[4] dynamic LDS bytes (BWD: of qtran_bwd_rows_kernel; plan[7]: of qtran_bwd_agents_kernel)
 *     plan[5] rounds: 16-row tiles the busiest wave walks   plan[6] BWD: slabs qtran_reduce_kernel sums
 *   STATE_PARTS (BT, S, nsets) / QMIX_TAIL (BT, S):
 *     plan[0] KCT: 16-column chunks of the instantiation   plan[1] nsets   plan[3] workgroups   plan[4] LDS bytes
 *     plan[5] rounds: 64-row blocks the busiest workgroup walks
 *   WGRAD_ROWS (BT, S, AE):
 *     plan[0] FT   plan[1] SMAX (224 / 384)   plan[2] 16x16 product tiles   plan[3] workgroups   plan[4] LDS bytes
 *     plan[5] rounds: 32-row blocks the busiest workgroup walks   plan[6] slabs qtran_wgrad_reduce_kernel sums */
#define MARL_QTRAN_PLAN_FWD 0
#define MARL_QTRAN_PLAN_FWD2 1
#define MARL_QTRAN_PLAN_BWD 2
#define MARL_QTRAN_PLAN_STATE_PARTS 3
#define MARL_QTRAN_PLAN_QMIX_TAIL 4
#define MARL_QTRAN_PLAN_WGRAD_ROWS 5
int marl_qtran_plan(int what, long BT, int N, int A, int AE, int S, int nsets, int* plan);

/* QPLEX (DMAQer.forward + calc_v/calc_adv, mixer.py:211-288; DMAQ_SI_Weight tail :158-169).
 *  wv row = [w_raw (N) | v (N)] (outputs of hyper_w_final.2 / V.2);
 *  heads = key (rows,K,1) | agents (rows,K,N) | action (rows,K,N) raw extractor outputs.
 *  out: v_tot, a_tot (either may be NULL).  max_q NULL => is_v only. */
int marl_qplex_mix_fwd(const float* w_raw, const float* v, const float* q, const float* max_q,
                       const float* key, const float* ag, const float* ac, float* v_tot, float* a_tot,
                       float* lam_out, long rows, int N, int K, int weighted_head, int minus_one,
                       void* stream);
/* autograd for q_tot = v_tot + a_tot given g = dL/dq_tot: dq (N), dw_raw, dv, dkey, dag, dac */
int marl_qplex_mix_bwd(const float* w_raw, const float* q, const float* max_q, const float* key,
                       const float* ag, const float* ac, const float* g, float* dq, float* dw_raw,
                       float* dv, float* dkey, float* dag, float* dac, long rows, int N, int K,
                       int weighted_head, int minus_one, void* stream);

/* QLearner.get_max_episode_len (q_learner.py:49-66; qtran_learner.py:52-69): out[0] = max over episodes of
 * (first step t with terminated[e,t] == 1) + 1, 0 when no episode terminates (the caller then uses
 * episode_limit); episodes that never terminate are ignored (quirk Q2).  term: (E, >=T) fp32, row stride ld. */
int marl_first_terminated_len(const float* term, long ld, int E, int T, int* out, void* stream);

/* ReplayBuffer.sample (common/replaybuffer.py:54-60) for a ring that lives in HBM: the per-step arrays of the B sampled
 * episodes idx[b] (int64) in one launch.  Sources are the ring's arrays: u (E,T,N) int32, r / terminated / padded (E,T)
 * fp32, length / won (E) int32, avail (E,T+1,N,A) fp32 ((T+1)-slot storage).  Outputs: o_map (B) = idx as int32 (the
 * episode map the unroll / mixer kernels read obs and state through), u and u_act = max(u, 0) (B,T,N), r / term / padded
 * (B,T), length / won (B), avail_next (B,T,N,A) = avail slots 1..T; avail_cur (B,T,N,A) or NULL = avail slots 0..T-1 with
 * zeros from each episode's end on - the availability QPLEX / QTRAN mask the current-step greedy action with
 * (q_learner.py:135-140, qtran_learner.py:103-108).  obs and state are NOT copied. */
int marl_replay_gather(const long long* idx, int B, int T, int N, int A, const int* u_src, const float* r_src,
                       const float* term_src, const float* padded_src, const int* length_src, const int* won_src,
                       const float* avail_src, int* o_map, int* u, int* u_act, float* r, float* term, float* padded,
                       int* length, int* won, float* avail_next, float* avail_cur, void* stream);

/* TD target + masked squared error (q_learner.py:165-168).  Writes the UN-normalised gradient
 * dq_tot = -2 mask^2 td and out2 = {sum (mask td)^2, sum mask}; the 1/sum(mask) factor is applied
 * in the optimizer so that data-parallel ranks can all-reduce numerators. */
int marl_td_loss(const float* q_tot, const float* q_tot_tgt, const float* r, const float* term,
                 const float* padded, float gamma, float* dq_tot, float* out2, float* ws, long rows,
                 void* stream);
/* QTRAN-base losses (qtran_learner.py:121-152). out4 = {l_td, l_opt, l_nopt numerators, sum mask};
 * gradients un-normalised: d_jq (joint_q_evals), d_v, d_qsum_opt, d_qsum_nopt. */
int marl_qtran_loss(const float* jq, const float* jq_tgt, const float* v, const float* jq_hat,
                    const float* qsum_opt, const float* qsum_nopt, const float* r, const float* term,
                    const float* padded, float gamma, float lam_opt, float lam_nopt, float* d_jq,
                    float* d_v, float* d_qsum_opt, float* d_qsum_nopt, float* out4, float* ws, long rows,
                    void* stream);
size_t marl_loss_workspace(long rows);

/* ---- Qatten mixer (qatten.hip; Yang et al. 2020 - the reference ships no Qatten: the definition is this project's own) ---------
 * Per row, with the unit features u_i = s[i U : (i + 1) U] (i < N) read in place from the state row, H heads and scale = 1/sqrt(D):
 *   l_{h,i} = scale (p_h . u_i),   lam_{h,.} = softmax_i(l_{h,.}) (maximum subtracted),   y_h = sum_i lam_{h,i} q_i,
 *   q_tot = sum_h |w_raw_h| y_h + c.
 * p_h = Wk_h^T e_h is the bias-free key layer applied to the query e_h (e_h . (Wk_h u_i) = p_h . u_i), so the kernel has no weight
 * of its own.  hy (rows, ldh): [p (H U) | w_raw (H) | c (1)] per row; q (rows, N); s: segment 0 of a marl_src_t with k0 >= N U (row
 * remap and episode map honoured; columns from N U on are never read).  Backward, g = dL/dq_tot:
 *   dq_i = g sum_h |w_raw_h| lam_{h,i},  dw_raw_h = g y_h sign(w_raw_h) (sign(0) = 0),  dp_h = scale sum_i g |w_raw_h| lam_{h,i} (q_i - y_h) u_i,
 * dc = g is the caller's.  dhy (rows, lddh): [dp (H U) | dw_raw (H)] per row, nothing else of a row is written.  lam is recomputed.
 * marl_qatten_loss_bwd: forward, the TD loss of marl_td_loss (same expressions: dq_tot = -2 mask (mask td), out2 = {sum (mask td)^2,
 *   sum mask} written through the fixed-order finish on ws = marl_loss_workspace() bytes) and the backward in one launch; q_tot is
 *   optional.  Its q_tot is marl_qatten_mix_fwd's and its dq, dhy, dq_tot are those of mix_fwd -> marl_td_loss -> mix_bwd, bit for
 *   bit.  A row with padded = 1 and finite inputs gets exact zeros in dq, dhy, dq_tot and adds nothing to either sum.
 * fp32 only, no float atomics: two calls give the same bits.  Supported: 1 <= N <= 16, 1 <= U <= 64, 1 <= H <= 8 and a source of
 * segment 0 alone (no second segment, one-hot block, agent-id block or gate); marl_qatten_supported reports it, and the entry points
 * return hipErrorInvalidValue for what it rejects, for a NULL required pointer, ldh < H U + H + 1, lddh < H U + H or rows >= 2^31,
 * and write nothing then.  rows <= 0: returns 0, no launch.
 * marl_qatten_plan (host only), plan[4]: [0] rows of a workgroup's LDS tile  [1] workgroups  [2] dynamic LDS bytes
 *   [3] tiles the busiest workgroup walks. */
int marl_qatten_supported(const marl_src_t* s, int N, int U, int H);
int marl_qatten_plan(long rows, int N, int U, int H, int* plan);
int marl_qatten_mix_fwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale, float* q_tot,
                        long rows, int N, int U, int H, void* stream);
int marl_qatten_mix_bwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale, const float* dq_tot,
                        float* dq, float* dhy, long lddh, long rows, int N, int U, int H, void* stream);
int marl_qatten_loss_bwd(const marl_src_t* s, const float* hy, long ldh, const float* q, float scale,
                         const float* q_tot_tgt, const float* r, const float* term, const float* padded, float gamma,
                         float* q_tot, float* dq, float* dhy, long lddh, float* dq_tot, float* out2, float* ws, long rows,
                         int N, int U, int H, void* stream);

/* ---- LICA's mixing critic (lica.hip; Zhou et al., NeurIPS 2020 - the reference ships no LICA: the definitions are this project's
 * own) ------------------------------------------------------------------------------------------------------------------------
 * A critic row is one step (b, t), rows = B T.  K = N A, E = mixing_embed_dim.  hy (rows, ldh), the outputs of four hypernetworks
 * of the state, holds per row [ W1 (K E, k-major: W1[k, e] at k E + e) | b1 (E) | wf (E) | b2 (1) ], ldh >= K E + 2 E + 1.  The
 * input is x (rows, K), agent-major x[i A + k] - the agents' action distributions - or the taken actions u (rows N) int32, which
 * stand for the one-hot vector with one 1 per agent block (an index outside [0, A): that block all zero).  Exactly one of x and u is
 * non-NULL; with u only the N taken rows of W1 are read and the one-hot vector is never built.
 *   pre_e = b1_e + sum_k x_k W1[k, e],   h_e = relu(pre_e),   Q = sum_e h_e wf_e + b2       (no abs(): the critic is not monotonic)
 * marl_lica_mix_fwd: q (rows) = Q.
 * marl_lica_mix_bwd: with g = dq[row] and dpre_e = g wf_e [pre_e > 0] (pre is recomputed),
 *   dhy (rows, lddh >= K E + 2 E): [ dW1[k, e] = x_k dpre_e | db1 = dpre | dwf_e = g h_e ]; db2 = g is the caller's.  All K E + 2 E
 *     columns of a row are written - with u, dpre in the blocks of the taken actions (the row's db1 bit for bit) and exact zeros in
 *     the others - and nothing beyond them;
 *   dx (rows, K): dx_k = sum_e W1[k, e] dpre_e.
 *   Either output may be NULL, not both.
 * marl_lica_loss_bwd: the forward on the taken actions, the TD loss of marl_td_loss (same expressions: dq_tot = -2 m (m td) with
 *   m = 1 - padded, td = r + gamma q_tgt (1 - term) - Q, un-normalised) and the backward to dhy in one row launch; out2 = {sum (m td)^2,
 *   sum m} comes from a pass over the q it wrote that keeps marl_td_loss's partition of the rows, then the fixed-order finish on
 *   ws = marl_loss_workspace() bytes.  q, dhy, dq_tot and out2 equal mix_fwd -> marl_td_loss -> mix_bwd bit for bit.  A row with
 *   padded = 1 gets exact zeros in dhy and dq_tot and adds nothing to either sum; its hy, u, r and q_tgt enter no computation but its
 *   own q (they may hold NaN, and q[row] is then NaN too).  q is required.
 * Sums run in a fixed order (pre over k ascending from b1, Q over e ascending then + b2, dx over e ascending); fp32, no float atomics:
 * two calls give the same bits.  Supported: 1 <= N <= 16, 1 <= A <= 32, 1 <= E <= 64 (marl_lica_supported).  An unsupported shape,
 * a NULL required pointer, both or neither of x and u, both of dhy and dx NULL, a short ldh / lddh or rows >= 2^31:
 * hipErrorInvalidValue and nothing written.  rows <= 0: returns 0, no launch.
 * marl_lica_plan (host only), plan[4]: [0] rows of a workgroup's tile  [1] workgroups  [2] dynamic LDS bytes
 *   [3] tiles the busiest workgroup walks. */
int marl_lica_supported(int N, int A, int E);
int marl_lica_plan(long rows, int N, int A, int E, int* plan);
int marl_lica_mix_fwd(const float* hy, long ldh, const float* x, const int* u, float* q, long rows, int N, int A, int E,
                      void* stream);
int marl_lica_mix_bwd(const float* hy, long ldh, const float* x, const int* u, const float* dq, float* dhy, long lddh, float* dx,
                      long rows, int N, int A, int E, void* stream);
int marl_lica_loss_bwd(const float* hy, long ldh, const int* u, const float* q_tgt, const float* r, const float* term,
                       const float* padded, float gamma, float* q, float* dhy, long lddh, float* dq_tot, float* out2, float* ws,
                       long rows, int N, int A, int E, void* stream);

/* TD(lambda) returns (td_lambda.hip; utils/rl_utils.py:4-14, build_td_lambda_targets - a function the reference ships and never
 * calls).  Per episode b over the T steps of the batch, q[t] = q_next_tot[b, t] (the target network's value at the next state of
 * step t), m = 1 - padded:
 *   done = sum_t m[t] term[t],  G[T] = q[T-1] (1 - done),
 *   G[t] = lambda gamma G[t+1] + m[t] (r[t] + (1 - lambda) gamma q[t] (1 - term[t])),  t = T-1 .. 0;   ret[b, t] = G[t].
 * That is the reference's function called with target_qs[:, t+1] = q[t] and terminated = term * m (quirk Q15: the batches here
 * carry term = 1 on padded steps).  lambda = 0: m (r + gamma q (1 - term)), the one-step target; lambda = 1: the Monte-Carlo
 * return, bootstrapped from q[T-1] only when the episode did not terminate inside the window.  A row with m = 0 contributes nothing,
 * whatever finite values r and q hold there.  All five arrays: contiguous (B, T) fp32; ret may not alias an input; nothing outside
 * ret[0 : B*T] is written.  One wave per episode, no atomics: two calls give the same bits.  B <= 0 or T <= 0: returns 0, no launch.
 * A learner hands G to the loss kernels as r with gamma = 0 (their target is then G + 0 q (1 - term) = G). */
int marl_td_lambda_returns(const float* q_next_tot, const float* r, const float* term, const float* padded,
                           float gamma, float lambda, float* ret, int B, int T, void* stream);

/* ---- independent Q-learning (iql.hip; the reference ships no IQL: the definition is this project's own) -----------------------
 * Rows r = (b T + t) N + i: agent i at step t of episode b; R = B T N; m = 1 - padded[b, t].  q (R, A) the eval unroll's Qs, u (R)
 * int32 the taken actions (>= 0; an index outside [0, A) reads 0), q_sel / q_tgt / avail_next (R, A), r / term / padded (B T):
 *   q_taken[r] = q[r, u[r]],
 *   q_next[r]  = q_tgt[r, a*] masked with avail_next (mask_val where it is 0), a* the first-index argmax of q_sel[r, :] masked the
 *                same way - marl_q_double_select's comparisons; q_sel NULL: a* is taken on q_tgt itself, which gives
 *                marl_q_masked_max's value; avail_next NULL: everything is available; a live row with nothing available: mask_val,
 *   y[r]       = r[b,t] + gamma (1 - term[b,t]) q_next[r]        (ret NULL),       y[r] = ret[b, i, t]        (ret given, (B, N, T)),
 *   td = y - q_taken,   dq_val[r] = - 2 m td (un-normalised, as marl_td_loss's dq_tot),   out2 = { sum_r m td^2, sum_r m = N sum m }.
 * A row with m = 0 contributes nothing, its dq_val, q_taken, q_next are exact zeros and its q, q_sel, q_tgt, avail_next (and ret)
 * entries never enter a computation: they may hold NaN.
 *
 * marl_iql_loss_bwd, ret NULL: gather, selection, target, loss partials and the sparse gradient (the dq_val of
 *   marl_agent_unroll_bwd with dq_idx = u) in ONE pass over the rows, then the fixed-order finish of the two sums.  q_taken and
 *   q_next (R) are optional outputs.  ret given: the target is ret; q_sel, q_tgt, avail_next, r and term are not read and q_next is
 *   not written.
 * marl_iql_select: the first half alone, for TD(lambda): q_taken (R, optional) and q_next written in (B, N, T) layout,
 *   q_next_bnt[(b N + i) T + t] - the layout marl_td_lambda_returns scans on B N sequences.  Same bits as the fused call's.
 * Up to A = 21 (three row operands; 31 with two, 63 with one) a wave stages 64 rows of each operand through LDS, beyond that a lane
 * scans its row in global memory: same comparisons, same bits.  fp32, fixed-order sums (ws: marl_loss_workspace() bytes), no float
 * atomics: two calls give the same bits.  A NULL required pointer, A < 1, N < 1, B T N >= 2^31 or an output overlapping an input or
 * another output: hipErrorInvalidValue.  B <= 0 or T <= 0: returns 0, no launch. */
int marl_iql_loss_bwd(const float* q, const int* u, const float* q_sel, const float* q_tgt, const float* avail_next,
                      const float* ret, const float* r, const float* term, const float* padded, float gamma, float mask_val,
                      float* dq_val, float* q_taken, float* q_next, float* out2, float* ws, int B, int T, int N, int A,
                      void* stream);
int marl_iql_select(const float* q, const int* u, const float* q_sel, const float* q_tgt, const float* avail_next,
                    const float* padded, float mask_val, float* q_taken, float* q_next_bnt, int B, int T, int N, int A,
                    void* stream);

/* ---- Weighted QMIX (wqmix.hip; Rashid et al., NeurIPS 2020 - the reference ships no WQMIX: the definition is this project's own) --
 * Beside QMIX's eval agent and monotonic mixer (q, the continuation q_en, Q_tot) there are a central agent (qc; its target copy on
 * the next inputs: qc_tgt) and an unconstrained central mixer Qc.  m = 1 - padded[b, t].
 *
 * marl_wqmix_select, one pass over the agent rows r = (b T + t) N + i, R = B T N.  q, qc, avail, q_en, qc_tgt, avail_next: (R, A);
 * u (R) int32; padded (B T).  Per live row (m != 0):
 *   q_taken[r] = q[r, u[r]],   qc_taken[r] = qc[r, u[r]]                       (a u outside [0, A): 0 for both)
 *   u_next[r]  = first-index argmax of q_en[r, :] masked with avail_next (mask_val where it is 0),
 *   qc_next[r] = qc_tgt[r, u_next[r]] masked the same way - marl_q_double_select's comparisons and value;
 *   u_greedy[r] = first-index argmax of q[r, :] masked with avail - marl_q_masked_max's argmax -,  qc_greedy[r] = qc[r, u_greedy[r]]
 *                 (not masked).  u_greedy and qc_greedy are optional (CW's); with both NULL q, qc and avail are read at u alone.
 * avail / avail_next NULL: everything is available.  A live row with nothing available: index 0, qc_next = mask_val.
 * A row with m = 0 gets exact zeros in the four values and -1 in the two indices; its row operands and its u enter no computation:
 * they may hold NaN or any integer.  Up to A = 21 (31 without any availability) a wave stages 64 rows of each operand through LDS,
 * beyond that a lane scans its row in global memory: same comparisons, same bits.
 * Supported: 1 <= N <= 16, 1 <= A <= 32 (marl_wqmix_supported).  An unsupported shape, a NULL required pointer, B T N >= 2^31 or an
 * output overlapping an input or another output: hipErrorInvalidValue, nothing launched.  B <= 0 or T <= 0: returns 0, no launch.
 *
 * marl_wqmix_loss, one pass over the rows (b, t), rows = B T.  q_tot, qc = Qc(qc_taken, s), qc_g = Qc(qc_greedy, s) (NULL: the OW
 * weighting), qc_next_tot = Qc_target(qc_next, s'), r, term, padded: (rows); u, u_greedy: (rows, N) int32, read only with qc_g.
 *   y = r + gamma qc_next_tot (1 - term)  (marl_td_loss's expression),   td = y - q_tot,   tdc = y - qc,
 *   OW: w = 1 if td > 0, else alpha;     CW: w = 1 if y > qc_g or u[., i] == u_greedy[., i] for every agent i, else alpha,
 *   dq_tot = - 2 w m (m td),   dqc = - 2 m (m tdc)   (un-normalised, as marl_td_loss's),   w (rows, optional),
 *   out4 = { sum w (m td)^2,  sum m,  sum (m tdc)^2,  sum m [w == 1] }.
 * The sums go through the fixed-order finish on ws = marl_loss_workspace() bytes over marl_td_loss's partition of the rows: with
 * alpha = 1, dq_tot, out4[0], out4[1] equal marl_td_loss(q_tot, qc_next_tot, ..) and dqc, out4[2] equal marl_td_loss(qc,
 * qc_next_tot, ..) bit for bit.  A row with m = 0 gets exact zeros in dq_tot, dqc and w and adds nothing to any sum, whatever its
 * inputs hold (NaN included).  fp32, no float atomics: two calls give the same bits.  N outside 1..16, alpha outside [0, 1], a NULL
 * required pointer (u / u_greedy with qc_g), rows >= 2^31 or an output overlapping an input or another output:
 * hipErrorInvalidValue, nothing launched.  rows <= 0: returns 0, no launch. */
int marl_wqmix_supported(int N, int A);
int marl_wqmix_select(const float* q, const float* qc, const int* u, const float* avail, const float* q_en, const float* qc_tgt,
                      const float* avail_next, const float* padded, float mask_val, float* q_taken, float* qc_taken,
                      int* u_greedy, float* qc_greedy, int* u_next, float* qc_next, int B, int T, int N, int A, void* stream);
int marl_wqmix_loss(const float* q_tot, const float* qc, const float* qc_g, const float* qc_next_tot, const float* r,
                    const float* term, const float* padded, float gamma, const int* u, const int* u_greedy, float alpha,
                    float* dq_tot, float* dqc, float* w, float* out4, float* ws, long rows, int N, void* stream);

/* ---- stochastic policy of the policy-gradient learners (policy.hip; central-V, REINFORCE) --------
 * A row is one agent at one step: logits z (A floats, the agent's fc2 output), availability a in {0,1}^A, exploration rate eps:
 *   p = softmax(z) over all A actions,  n = sum_k a_k,  pt_k = a_k ((1 - eps) p_k + eps / n),  pi_k = pt_k / sum_j pt_j.
 * A row with n = 0 (a padded step) has no policy: it contributes nothing to any sum, its outputs are exact zeros and its logits are
 * never looked at.  fp32 throughout; fixed-order sums, no float atomics: two calls give the same bits.
 *
 * marl_policy_probs: pi (rows, A) of logits / avail (rows, A); pi may be logits itself, not avail.
 *
 * marl_policy_loss_bwd: the actor loss of rows = B*T*N agent steps, row r belonging to (episode, step) r / N.  With m = 1 - padded
 * and Adv = G - v of that step (constants of the gradient; formed here) and u the taken action:
 *   logp[r] = log pi_r(u[r])  (0 on a row without a policy, or whose m = 0),
 *   out2 = { - sum_r m Adv logp[r],  sum_r m } = { numerator of L_actor, N * sum(m) }  (un-normalised, as marl_td_loss leaves them),
 *   dlogits (rows, A) = the gradient of out2[0] by the logits: - m Adv d log pi(u) / dz, through pt and the renormalisation
 *   (at eps = 0: - m Adv (delta_uk - pi_k)); the dense dq of marl_agent_unroll_bwd.
 * G, v, padded: (rows / N); ws: marl_loss_workspace() bytes; dlogits may be logits itself, not avail.
 *
 * marl_policy_loss_bwd_ex: the same pass without a baseline and with an entropy bonus beta >= 0 (REINFORCE; central-V with
 * --policy_entropy_coef).  v may be NULL: Adv = G.  A row "has a policy" when n > 0 and its taken action is available.  With a the
 * row's availability flags, the entropy of the policy the action was drawn from (eps mixing included, as in log pi) is
 *   H_r = - sum_{k: a_k = 1} pi_k log pi_k,  a term with pi_k = 0 being 0 (at eps = 0 the fp32 exponent underflows once a logit sits
 *   about 104 below the largest available one: 0 log 0 is 0, not NaN);  H = 0 and no entropy gradient on a row with n = 1;
 * a row without a policy, or with m = 0, contributes nothing to any sum, its dlogits are exact zeros, its logits are never looked at.
 *   L = [ - sum_r m Adv logp[r] - beta sum_r m H_r ] / (N sum m)      (REINFORCE: Adv = G, the discounted Monte-Carlo return -
 *       marl_td_lambda_returns with lambda = 1 and an all-zero q_next_tot: an episode cut at max_episode_len gets no bootstrap),
 *   out3 = { - sum m Adv logp - beta sum m H,  sum_r m,  sum_r m H }  (un-normalised),
 *   ent[r] = H_r (0 where the row has no policy or m = 0); ent may be NULL,
 *   dlogits = - m Adv d log pi(u) / dz - beta m dH / dz.  With the kernel's e_k = exp(z_k - mx), S = sum e, Sa = sum a e,
 *   D = (1 - eps) Sa + eps S, c2 = (1 - eps) / D, Pa = Sa / S, L1 = sum_k a_k e_k log pi_k and Hn = sum_k pi_k log pi_k:
 *     dH/dz_i = - c2 (a_i e_i log pi_i - e_i L1 / S) + c2 e_i (a_i - Pa) Hn    (at eps = 0: - pi_i (log pi_i + H) on available
 *     actions, exactly 0 on unavailable ones).
 * The entropy is folded into the same pass over the staged rows: no bytes moved beyond ent.  beta = 0 with v given returns
 * marl_policy_loss_bwd's dlogits, logp and first two statistics bit for bit.  ws: marl_loss_workspace() bytes (three partials
 * per workgroup); beta < 0 is an error.
 *
 * marl_policy_sample: one action per live agent of a lock-step, the argument shape of marl_select_actions.  With
 * x = u01(hash(rseed, SAMPLE, env0 + e, tg, n)) the action is the first k in index order with a_k = 1 whose running fp32 sum of
 * pi over the available actions up to k exceeds x; the last available action when rounding leaves none.  Environments with
 * alive[e] == 0 get -1. */
int marl_policy_probs(const float* logits, const float* avail, float eps, float* pi, long rows, int A, void* stream);
int marl_policy_loss_bwd(const float* logits, const float* avail, const int* u, const float* G, const float* v,
                         const float* padded, float eps, float* dlogits, float* logp, float* out2, float* ws, long rows,
                         int N, int A, void* stream);
int marl_policy_loss_bwd_ex(const float* logits, const float* avail, const int* u, const float* G, const float* v,
                            const float* padded, float eps, float beta, float* dlogits, float* logp, float* ent, float* out3,
                            float* ws, long rows, int N, int A, void* stream);
int marl_policy_sample(const float* logits, const float* avail, long avail_es, const int* alive, float eps,
                       unsigned rseed, int env0, const int* tg, int tg0, int* act_out, long act_es,
                       int E, int N, int A, void* stream);

/* ---- MAPPO: the clipped surrogate (policy.hip) and advantage standardisation (ppo.hip) -----------
 * marl_ppo_loss_bwd: marl_policy_loss_bwd_ex's pass under PPO's clipped surrogate.  Rows, m, "has a policy", pi, log pi, H and
 * their gradients (eps mixing included) are marl_policy_loss_bwd_ex's.  adv (rows / N) stands where G / v stood (a constant of the
 * gradient), logp_old (rows) is log pi(u) under the policy the batch's first pass saw (NULL: that pass itself), clip = c in (0, 1).
 * For a row with a policy and m = 1:
 *   rho = exp(min(logp - logp_old, 80))  (logp_old NULL: rho = 1 exactly),
 *   s = rho adv,  k = clamp(rho, 1 - c, 1 + c) adv,  clipped = k < s  (the minimum takes the clamped term, strictly),
 *   L_row = - min(s, k) - beta H,
 *   dlogits = - (clipped ? 0 : adv rho) d log pi(u) / dz - beta dH / dz,
 *   logp[r] = log pi_r(u_r),  ent[r] = H_r (ent may be NULL),
 *   out4 = { sum m L_row,  sum_r m = N sum m,  sum m H,  sum m [clipped] }  (un-normalised).
 * A row with m = 0 or without a policy contributes nothing, its dlogits are exact zeros, logp = ent = 0, and its logits and
 * logp_old are never looked at (nor is a padded step's adv).  A row with one available action has rho = 1 and no gradient; it
 * still contributes - adv to the numerator.  logp comes from the row's scalars before the one gradient walk, whose scale is
 * - m adv rho (0 when clipped).  With logp_old NULL, dlogits, logp and ent are marl_policy_loss_bwd_ex's with G = adv and v NULL
 * bit for bit, and out4[3] = 0.  fp32, fixed-order sums, no float atomics: two calls give the same bits.  ws: marl_loss_workspace()
 * bytes (four partials per workgroup).  dlogits may be logits itself, not avail; logp may be logp_old.  A NULL required pointer,
 * rows % N != 0, c outside (0, 1), beta < 0 or dlogits == avail: hipErrorInvalidValue.  rows <= 0: returns 0, no launch.
 *
 * marl_masked_standardize: over x (rows) and padded (rows), m = 1 - padded, M = sum m:
 *   mean = sum m x / M,  var = sum m (x - mean)^2 / M  (a pass each: never E[x^2] - mean^2),  out = m (x - mean) / (sqrt(var) + 1e-5).
 * Padded rows get exact zeros and their x is never looked at; M = 0 gives all zeros and stats3 = 0.  stats3 = { mean, var, M }.
 * out may be x itself, not padded.  ws: marl_loss_workspace() bytes.  Fixed-order sums: two calls give the same bits.
 * rows <= 0: returns 0, no launch. */
int marl_ppo_loss_bwd(const float* logits, const float* avail, const int* u, const float* adv, const float* logp_old,
                      const float* padded, float eps, float beta, float clip, float* dlogits, float* logp, float* ent,
                      float* out4, float* ws, long rows, int N, int A, void* stream);
int marl_masked_standardize(const float* x, const float* padded, float* out, float* stats3, float* ws, long rows, void* stream);

/* ---- LICA's actor pass (policy.hip): the transpose-Jacobian of the policy by its logits applied to a vector ----------------------
 * marl_policy_probs_bwd: rows = B T N agent rows, row r of step r / N; pi, m, H, dH/dz and "no policy" (n = 0) are those above.
 * gpi (rows, A) is dL/dpi, read on available actions only.  With e_k = exp(z_k - mx), S = sum e, Sa = sum a e,
 * D = (1 - eps) Sa + eps S, n = sum a:
 *   (J^T g)_i = (e_i / D) [ (1 - eps) a_i g_i + (eps / n) sum_k a_k g_k - ((1 - eps) a_i + eps) sum_k pi_k g_k ]
 *   (at eps = 0: pi_i (g_i - sum_k pi_k g_k) on available actions, exactly 0 elsewhere).
 * For an agent row with m = 1 and a policy:  dlogits = J^T gpi - beta dH/dz,  ent[r] = H_r (ent may be NULL),
 *   out3 = { - sum_r m q_pi[r / N] - beta sum_r m H_r,  sum_r m,  sum_r m H_r }  (un-normalised; q_pi (rows / N) may be NULL: that
 *   term is 0.  Every live agent row adds - q_pi of its step once, which gives a factor N).
 * A row with m = 0 or without a policy: exact zero dlogits, ent = 0, its logits and gpi never looked at; such a row still adds
 * - q_pi when m = 1.  A row with one available action: dlogits exactly 0, H = 0.  dlogits may be logits or gpi itself, not avail.
 * fp32, fixed-order sums (ws: marl_loss_workspace() bytes, three partials per workgroup), no float atomics: two calls give the same
 * bits.  A NULL required pointer, rows % N != 0, beta < 0 or dlogits == avail: hipErrorInvalidValue.  rows <= 0: returns 0, no
 * launch. */
int marl_policy_probs_bwd(const float* logits, const float* avail, const float* gpi, const float* q_pi, const float* padded,
                          float eps, float beta, float* dlogits, float* ent, float* out3, float* ws, long rows, int N, int A,
                          void* stream);

/* ---- COMA: the counterfactual critic (coma.hip; the reference ships the argument table only - the definitions are this
 * project's own, from the published algorithm) ----------------------------------------------------------------------------
 * Rows r = (b T + t) N + i: agent i at step t of episode b; R = B T N; u (R) int32 the taken actions; D = critic_dim.  The critic is
 * fc1 = Linear(K, D) - ReLU - fc2 = Linear(D, D) - ReLU - fc3 = Linear(D, A) over the per-row input
 *   x_r = [ s | o_i | one-hot(u_j) for every agent j, agent i's own block zeroed | one-hot(u_j at t-1) for all j (zero at t = 0) |
 *           one-hot(i) ],   K = S + O + 2 N A + N,
 * in this column order of fc1.weight (D, K), actions j-major.  x is never materialised: the first layer factors exactly into
 *   h1_r = relu( W_s s_bt + b  +  W_o o_r  +  sum_{j != i} Wu[j, u_j] + [t > 0] sum_j Wl[j, u_j(t-1)] + Wid[i] ).
 * An action index outside [0, A) is an all-zero one-hot.  fp32 throughout, fixed-order sums, no float atomics: two calls give the
 * same bits; every entry point returns 0 without a launch on an empty shape.  D must be a multiple of 4, at most 1024; pre_s, Wt,
 * h1, dh1, dpre, dsum 16-byte aligned.
 *
 * marl_coma_onehot_cols: Wt (C, D) = the K-major copy of columns [col0, col0 + C) of the row-major W (D, ldw): Wt[c][d] =
 *   W[d][col0 + c].  With col0 = S + O and C = 2 N A + N its rows are Wu (N A), Wl (N A), Wid (N): every gather below reads D
 *   contiguous floats.
 * marl_coma_fc1_fwd: pre_s (B T, D) = W_s s + b (marl_linear on the state block, once per step); h1 (R, D) holds W_o o on entry
 *   (marl_linear on the observation block) and relu of the sum above on return.  The step's sum over all j is formed once and
 *   agent i subtracts its own column.
 * marl_coma_fc1_bwd: dh1, h1 (R, D) -> dpre = dh1 (h1 > 0) (R, D; may be dh1), dsum (B T, D) = sum_i dpre in agent order, and the
 *   gradient of the one-hot columns ADDED into dW[d][col0 + c] (dW row stride lddw):
 *     action (j, k): sum over the steps with u_j = k of (dsum - dpre_j);  last action (j, k): sum over the steps with t > 0 and
 *     u_j(t-1) = k of dsum;  id i: sum of dpre_i  -  per slab of steps in step order, then over the slabs in slab order.
 *   The state block's gradient is marl_linear_wgrad on (dsum, s), the observation block's on (dpre, o), the bias's the column sums
 *   of dsum.  ws: marl_coma_fc1_bwd_workspace() bytes; 2 A D floats of LDS (at most 64 KiB).
 * marl_coma_q_taken: out (B, N, T), out[b, i, t] = q[b, t + shift, i, u[b, t + shift, i]] for 0 <= t + shift < T, else 0
 *   (shift = 1 on the target critic's Q: q_next, zero at the window's last step).
 * marl_coma_loss_bwd: both losses of one forward pass.  With m = 1 - padded (B T), pi the policy of marl_policy_probs (a row has
 *   a policy when n > 0 and its taken action is available), G (B, N, T) the lambda-returns (constants of the gradient):
 *     q_taken[r] = Q_r(u_r),  adv[r] = Q_r(u_r) - sum_k pi_r(k) Q_r(k)  (a constant of the gradient; exactly 0 when n = 1),
 *     logp[r] = log pi_r(u_r),  ent[r] = H_r  as in marl_policy_loss_bwd_ex,
 *     dlogits = - m Adv d log pi(u) / dz - beta m dH / dz  (beta = 0: the plain gradient walk),
 *     dq (R, A) = - 2 m (G - Q_u) at column u, exact zeros elsewhere,
 *     out_c2 = { sum m (G - Q_u)^2, sum_r m } and out_a3 = { - sum m Adv logp - beta sum m H, sum_r m, sum m H }, un-normalised
 *     (sum_r m = N sum m, the denominator of both losses).
 *   A row with m = 0 or without a policy contributes nothing to the numerators, its dlogits and dq are exact zeros, its four
 *   per-row outputs are 0 and its logits and Q are never looked at.  dlogits may be logits and dq may be q; no other aliasing.
 *   ws: marl_loss_workspace() bytes (four partials per workgroup); beta < 0 is an error. */
int marl_coma_onehot_cols(const float* W, long ldw, int col0, float* Wt, int C, int D, void* stream);
int marl_coma_fc1_fwd(const float* pre_s, const float* Wt, const int* u, float* h1, int B, int T, int N, int A, int D,
                      void* stream);
size_t marl_coma_fc1_bwd_workspace(int B, int T, int N, int A, int D);
int marl_coma_fc1_bwd(const float* dh1, const float* h1, const int* u, float* dpre, float* dsum, float* dW, long lddw,
                      int col0, float* ws, size_t ws_bytes, int B, int T, int N, int A, int D, void* stream);
int marl_coma_q_taken(const float* q, const int* u, float* out, int shift, int B, int T, int N, int A, void* stream);
int marl_coma_loss_bwd(const float* logits, const float* avail, const float* q, const int* u, const float* G,
                       const float* padded, float eps, float beta, float* dlogits, float* dq, float* logp, float* ent,
                       float* adv, float* q_taken, float* out_c2, float* out_a3, float* ws, int B, int T, int N, int A,
                       void* stream);

/* ---- optimizer (optim.hip): clip_grad_norm_ + RMSprop / Adam on ONE flat buffer -------------
 * (q_learner.py:42-47,170-173; torch defaults).  g is the un-normalised gradient; den points to
 * sum(mask) on the device (NULL = 1).  sumsq[0] receives sum g^2 (before scaling). */
int marl_grad_sumsq(const float* g, long n, float* sumsq, float* ws, void* stream);
size_t marl_sumsq_workspace(long n);
int marl_rmsprop_step(float* p, const float* g, float* sq, long n, float lr, float alpha, float eps,
                      float clip, const float* sumsq, const float* den, void* stream);
int marl_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                   float beta2, float eps, float bc1, float bc2_sqrt, float clip, const float* sumsq,
                   const float* den, void* stream);

/* ---- rollout (rollout.hip) ------------------------------------------------------------------
 * epsilon-greedy action choice of SharedMAC.choose_action (share_params.py:66-70), batched:
 * explore iff u01(hash(rseed,EXPLORE,env,tg,n)) < eps, then the floor(u01(hash(..PICK..))*n_avail)-th
 * available action, else first-index argmax of avail-masked q.  act_out[e*act_es + n]; envs with
 * alive[e]==0 get -1. tg[e] = per-env global step id (NULL: tg0). */
int marl_select_actions(const float* q, const float* avail, long avail_es, const int* alive, float eps,
                        unsigned rseed, int env0, const int* tg, int tg0, int* act_out, long act_es,
                        int E, int N, int A, void* stream);
/* The episode record every environment and rollout entry below takes: (T+1)-slot storage for what is observed, T slots for what a
 * step produces.  state_ld is the row stride of the state storage in floats: a multiple of 4 keeps every state row 16-byte aligned
 * for any S (MMM2: S = 322 -> 324), which the GEMM kernels downstream need for their vector loads; pad columns are written as zeros
 * or left untouched (allocate them zeroed).  The rules every entry that takes one holds to:
 *   - an entry reads only the fields its comment names (and the sizes); the others may be NULL;
 *   - rec == NULL is hipErrorInvalidValue; otherwise E <= 0 (for the whole rollouts also T <= 0) returns 0 and launches nothing,
 *     whatever the pointers are (the battle entries refuse a shape that is not the map's first);
 *   - every other refusal is hipErrorInvalidValue, made before anything is dereferenced or written (the shape checks before w). */
typedef struct {
  float *obs, *state, *avail;   /* (E,T+1,N,O)  (E,T+1,state_ld >= S)  (E,T+1,N,A) */
  long state_ld;
  int* u;                       /* (E,T,N) */
  float *r, *term, *padded;     /* (E,T) */
  int *length, *won;            /* (E) */
  int E, T, N, O, S, A;
} marl_record_t;

/* Synthetic SMAC-shaped environment (stands in for StarCraft II, main.py:16-20).  lengths: len / won (E) of the
 * episode.  observe: reads length, writes slot t of obs / state / avail. */
int marl_synth_lengths(unsigned seed, int env0, int episode, int* len, int* won, int E, int T, void* stream);
int marl_synth_observe(unsigned seed, int env0, int episode, int t, const marl_record_t* rec, void* stream);
/* reward / terminated / padded for step t given act (E,N) (rollout.py:86-96,122-133 for padding): reads length, writes r / term /
 * padded and u (the action, or -1 on padding) of step t; never touches obs / state / avail.  alive_next[e] = (t+1 < length[e]) */
int marl_synth_step(unsigned seed, int env0, int episode, int t, const int* act, const marl_record_t* rec, int* alive_next,
                    void* stream);

/* select + step + observe(t+1) of the synthetic env in ONE launch per lock-step (same arithmetic as the
 * three calls above; q is the (E,N,A) output of the T=1 agent unroll).  Reads length and slot t of avail; writes u / r / term /
 * padded of step t and slot t + 1 of obs / state / avail; never touches won. */
int marl_synth_fused_step(unsigned seed, unsigned rseed, int env0, int episode, int t, float eps, const float* q,
                          const marl_record_t* rec, void* stream);
/* marl_synth_fused_step with the choice drawn from the stochastic policy of the agent's row of q (logits) and its availability at
 * slot t: marl_policy_sample's definition with eps as the mixing epsilon and x = u01(hash(rseed, SAMPLE, env0 + e, tg, n)).  Same
 * arguments; everything after the choice is marl_synth_fused_step's. */
int marl_synth_fused_step_sample(unsigned seed, unsigned rseed, int env0, int episode, int t, float eps, const float* q,
                                 const marl_record_t* rec, void* stream);

/* The WHOLE rollout of the synthetic env in one persistent launch (rollout_fused.hip): agent step,
 * epsilon-greedy choice, env step and next observation for all T lock-steps; weights and hidden state
 * stay on chip.  eps[T] = epsilon per lock-step; eps == NULL: eps(0) = eps0 and the reference's per-step anneal
 * eps(t+1) = eps(t) > eps_min ? eps(t) - eps_anneal : eps(t) (rollout.py:100-101) evaluated in the kernel, in fp64.  Produces the same (T+1)-slot record as the
 * launch-per-step path.  stats (optional, [3][E] floats): per episode  sum_t r | won | length - what
 * RolloutWorker.generate_episodes returns besides the batch (rollout.py:135-140), without extra launches.  Needs whole environments per workgroup: marl_synth_rollout_supported(). */
int marl_synth_rollout_supported(int N, int O, int A);
int marl_synth_rollout(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                       int episode, int fixed_len, const float* eps, float* h_out, float* stats, double eps0,
                       double eps_anneal, double eps_min, int last_action, int reuse_network, void* stream);
/* marl_synth_rollout with every action drawn from the stochastic policy of the step's logits instead of the epsilon-greedy choice:
 * marl_synth_rollout's argument list and meaning, the same marl_synth_rollout_supported() shapes and launch plan.  eps(t) - the
 * eps vector or the fp64 schedule - is the policy's mixing epsilon of lock-step t.  With x = u01(hash(rseed, SAMPLE, env, tg, n))
 * (one draw per environment, agent and global step tg) the action is marl_policy_sample's: with row_policy's scalars of the row, the
 * first k in index order with a_k = 1 whose running fp32 sum of (cw e_k + ew) / D over the available actions up to k exceeds x; the
 * last available action when rounding leaves none.  Rows past the episode's end get -1. */
int marl_synth_rollout_sample(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                              int episode, int fixed_len, const float* eps, float* h_out, float* stats, double eps0,
                              double eps_anneal, double eps_min, int last_action, int reuse_network, void* stream);

/* The same whole rollout with the agent step (network/q_network.py:16-21) as bf16x6 split products (rollout_x6.hip; args.gemm_mode =
 * "bf16x6"): same arguments, same environment, same epsilon-greedy choice, same record - the integer fields agree with
 * marl_synth_rollout wherever no two available actions' Q values lie within fp32 rounding of each other (the choice is an argmax).
 * fc1 is evaluated as (bias + W1[:, obs | id] in) + W1[:, O + last action]: the observation part on the matrix cores a step ahead,
 * the chosen action's column added in fp32.  marl_synth_rollout_x6_supported_flags(), exactly: H = 64, O a multiple of 4, input width
 * I = O (+ A if last_action) (+ N if reuse_network) <= 224, A <= 16 while I <= 160 and A <= 32 beyond (two action tiles exist only at
 * seven fc1 chunks), N <= 64 and within the row tiles of one workgroup.  The flags are those the launch will be given.
 * marl_synth_rollout_x6_supported() is the same predicate with both flags on. */
int marl_synth_rollout_x6_supported_flags(int N, int O, int A, int last_action, int reuse_network);
int marl_synth_rollout_x6_supported(int N, int O, int A);
/* How marl_synth_rollout_x6 runs a batch of E environments (two decompositions of the same arithmetic, picked by batch size:
 * csrc/rollout_x6_v1.hip holds at most three row tiles of 16 (episode, agent) rows per workgroup, csrc/rollout_x6.hip up to five):
 * plan[0] = decomposition (1 / 2), plan[1] = workgroups, plan[2] = row tiles per workgroup, plan[3] = environments per workgroup,
 * plan[4] = fc1 chunks of 32 input columns.  What bench.py's roofline model counts the executed products by. */
int marl_synth_rollout_x6_plan(int E, int N, int O, int A, int last_action, int reuse_network, int* plan);
int marl_synth_rollout_x6(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                          int episode, int fixed_len, const float* eps, float* h_out, float* stats, double eps0,
                          double eps_anneal, double eps_min, int last_action, int reuse_network, void* stream);

/* ---- RTW reflection head (rtw_head.hip) -------------------------------------------------------
 * The parts of RTWAgent (network/RTW.py:16-57) beyond the RNNQNet agent, torch layouts, hidden_dim = attn_dim = 64:
 *   t0 (64, 64+N), t2 (A, 64)      teammate_net.0 / .2
 *   w0 (64, O+N*A), w2 (O, 64)     world_net.0 / .2
 *   wq (64, 2O), wk (64, A)        w_q, w_k
 *   v0 (64, 64+A), v2 (A, 64)      w_v.0 / .2 */
typedef struct {
  const float *t0_w, *t0_b, *t2_w, *t2_b;
  const float *w0_w, *w0_b, *w2_w, *w2_b;
  const float *wq_w, *wq_b, *wk_w, *wk_b;
  const float *v0_w, *v0_b, *v2_w, *v2_b;
} marl_rtw_weights_t;
/* 1 when the head kernels cover the shape: H = hidden_dim = attn_dim = 64, 1 <= N <= 16, 1 <= A <= 32, 1 <= O <= 256. */
int marl_rtw_supported(int N, int O, int A, int H, int hidden_dim, int attn_dim);
/* Act mode (test_mode=True, RTW.py:70-119; RTWMAC.choose_action share_params.py:641-677 for every agent of E envs at once):
 * q (E*N, A) += the reflection term of each row.  h (E*N, 64) = the GRU output of the step; o of row (e, n) at
 * obs + (e*obs_bs + obs_t0*N + n)*O and avail of agent j at avail + (e*av_bs + av_t0*N + j)*A (the (ptr, bs, t0) slot
 * convention of marl_agent_unroll_fwd).  not_self_model as args.not_self_model.  Optional outputs (NULL to skip): a_out
 * (E*N, N) int32 teammate actions a_j of each row (the self entry included), ohat_out (E*N, O) the world net's o_hat. */
int marl_rtw_head_act(const marl_rtw_weights_t* w, const float* h, const float* obs, long obs_bs, int obs_t0,
                      const float* avail, long av_bs, int av_t0, float* q, int* a_out, float* ohat_out, int E, int N,
                      int O, int A, int not_self_model, void* stream);
/* Given mode (target=False, RTW.py:121-203; RTWMAC.get_current_q_values share_params.py:730-764) over B episodes x T steps:
 * q (B,T,N,A) += the reflection term with the taken actions u and the real o_next; the value of teammate j is computed
 * from hs of row j (RTW.py:122: h_repeat[b,i,j] = h[b,j]).  hs (B,T,N,64) as marl_agent_unroll_fwd writes it; o at
 * obs + (b*obs_bs + (t+obs_t0)*N + n)*O, o_next likewise, u int32 at u[b*u_bs + (t+u_t0)*N + n] (< 0 reads as 0). */
int marl_rtw_head_given(const marl_rtw_weights_t* w, const float* hs, const float* obs, long obs_bs, int obs_t0,
                        const float* obs_next, long on_bs, int on_t0, const int* u, long u_bs, int u_t0, float* q,
                        int B, int T, int N, int O, int A, int not_self_model, void* stream);

/* ---- world-model head (world_head.hip) --------------------------------------------------------
 * The WorldModel of network/world_model.py:7-41 (the part of world_model.Agent beyond the RNNQNet agent), torch layouts,
 * rnn_hidden_dim = 64:  h0 (64,64), h2 (64,64) world.hidden_embd.0 / .2;  r (A,64) world.r_out;  o (O,64) world.o_out;
 * t (2,64) world.terminate_out.  e = relu(h2 relu(h0 h + b) + b) (:33), r = r_out(e), o_hat = o_out(e), tau = terminate_out(e). */
typedef struct {
  const float *h0_w, *h0_b, *h2_w, *h2_b;
  const float *r_w, *r_b, *o_w, *o_b, *t_w, *t_b;
} marl_world_weights_t;
/* Gradient destinations of the same layers (accumulated into; terminate_out gets none: tau never reaches a loss). */
typedef struct {
  float *h0_w, *h0_b, *h2_w, *h2_b;
  float *r_w, *r_b, *o_w, *o_b;
} marl_world_grads_t;
/* 1 when the head kernels cover the shape: H = 64, 1 <= N <= 16, 1 <= A <= 32, 1 <= O <= 256. */
int marl_world_supported(int N, int O, int A, int H);
/* Forward over R = B*T*N rows (world_model.py:44-75 after the GRU; SharedMACWithState.get_current_q_values /
 * get_next_q_values share_params.py:303-375, choose_action :214-260 with B = E environments and T = 1):
 *   h (R,64): the hs plane marl_agent_unroll_fwd writes, or the (E*N,64) state of a rollout step
 *   q (R,A) += r (world_model.py:71: q = fc2(h) + r), or NULL; optional outputs r_out (R,A), ohat_out (R,O), tau_out (R,2)
 *   Act mode: loss == NULL.  Train mode (loss != NULL): loss[0] += sum over the rows of (o_hat - o_next)^2
 *   (q_learner_state.py:175-181 before the mean; unmasked).  o_next of row (b,t,n) is read with the unroll's addressing:
 *   obs + ((m(b)*obs_bs) + (t+obs_t0)*N + n)*O with m(b) = ep_map ? ep_map[b] : b; steps t >= ep_len[b] read as zeros
 *   (ep_len may be NULL).  ws: marl_world_fwd_workspace() bytes of per-workgroup partials, summed in a fixed order. */
size_t marl_world_fwd_workspace(int B, int T, int N);
int marl_world_head_fwd(const marl_world_weights_t* w, const float* h, float* q, float* r_out, float* ohat_out,
                        float* tau_out, const float* obs, long obs_bs, int obs_t0, const int* ep_len, const int* ep_map,
                        float* loss, float* ws, size_t ws_bytes, int B, int T, int N, int O, int A, void* stream);
/* Backward of the train-mode forward (autograd of q_learner_state.py:100-181 through the head, loss.backward() :184):
 *   dr = the sparse pair (dq_idx, dq_val) per row that marl_agent_unroll_bwd also receives (dr = dq; dq_idx NULL: none)
 *   d_o_hat = dscale * den[0] * (o_hat - o_next), o_next addressed as in the forward (den NULL: 1).  With dscale = 2 / K,
 *   K = B*T*N*O and den = sum(mask) the optimizer's division by den (marl_rmsprop_step / marl_adam_step) leaves d mean / d o_hat.
 *   dhs (R,64) = the gradient on hs (written), for marl_agent_unroll_bwd's dhs input; the weight and bias gradients of
 *   h0, h2, r, o are accumulated into g by fixed-order reductions (marl_linear_wgrad).  Activations are recomputed from hs.
 *   ws: marl_world_bwd_workspace() bytes. */
size_t marl_world_bwd_workspace(int B, int T, int N, int O, int A);
int marl_world_head_bwd(const marl_world_weights_t* w, const marl_world_grads_t* g, const float* hs, const int* dq_idx,
                        const float* dq_val, const float* obs, long obs_bs, int obs_t0, const int* ep_len, const int* ep_map,
                        const float* den, float dscale, float* dhs, float* ws, size_t ws_bytes, int B, int T, int N, int O,
                        int A, void* stream);

/* ---- MAIC message head (maic_head.hip, maic_head_bwd.hip) ----------------------------------------------------------
 * The parts of MAICAgent (network/MAIC.py:19-47) that its forward evaluates beyond the RNNQNet agent, torch layouts, with
 * rnn_hidden_dim = nn_hidden_size = 64, latent_dim L = 8, attention_dim D = 32 (inference_net only feeds the MI loss):
 *   e0 (64,64), bn (64) weight / bias / running_mean / running_var / num_batches_tracked (int64), e3 (2*N*L, 64)
 *                                       embed_net.0 / .1 / .3
 *   m0 (64, 64+L), m2 (A, 64)           msg_net.0 / .2
 *   k (D, 64), q (D, L)                 w_key, w_query
 * bn_rm / bn_rv / bn_nbt are read in eval mode and UPDATED in batch-statistics mode (bn_nbt may be NULL). */
typedef struct {
  const float *e0_w, *e0_b, *bn_w, *bn_b;
  float *bn_rm, *bn_rv;
  long long* bn_nbt;
  const float *e3_w, *e3_b, *m0_w, *m0_b, *m2_w, *m2_b, *k_w, *k_b, *q_w, *q_b;
} marl_maic_weights_t;
/* 1 when the head kernels cover the shape: H = NH = 64, L = 8, D = 32, 1 <= N <= 16, 1 <= A <= 32 (O only has to be positive:
 * the head does not read observations). */
int marl_maic_supported(int N, int O, int A, int H, int NH, int L, int D);
/* Bytes of scratch the batch-statistics mode needs for bs environments of N agents (eval mode needs none). */
size_t marl_maic_workspace(int bs, int N);
/* MAICAgent.forward after fc2 (MAIC.py:58-87) over bs environments x N agents, rows b*N + agent:
 *   h (bs*N, 64) the GRU output, q (bs*N, A) = fc2(h) on entry, q[b, j] += sum_i alpha[b,i,j] msg[b,i,j] on return (:85).
 *   test_mode: latent = the means and alpha < 0.25 / N is set to 0 (:63-64, :81-82); otherwise latent = mean + sqrt(var) eps
 *   with eps (bs*N, N*L) supplied by the caller (:66-68, rsample's noise) and no gate.  var = max(exp(.), var_floor) (:59-61).
 *   bn_batch 0: BatchNorm1d in eval mode (running statistics), one launch.  bn_batch 1: training mode - statistics of the
 *   batch over all bs*N rows (biased variance), running_mean / running_var (unbiased) moved by bn_momentum and
 *   num_batches_tracked += 1; three launches, partial statistics merged in a fixed order (two calls give the same bits);
 *   needs bs*N >= 2 and ws of marl_maic_workspace() bytes.
 *   Optional outputs (NULL to skip): mean_out / var_out / lat_out (bs*N, N*L), alpha_out (bs*N, N) after the gate,
 *   msg_out (bs*N*N, A) with pair row (b*N + i)*N + j (:72). */
int marl_maic_head_fwd(const marl_maic_weights_t* w, const float* h, float* q, const float* eps, float* mean_out,
                       float* var_out, float* lat_out, float* alpha_out, float* msg_out, float* ws, size_t ws_bytes, int bs,
                       int N, int A, int test_mode, int bn_batch, float var_floor, float bn_eps, float bn_momentum,
                       void* stream);
/* Gradient destinations of the message head's layers (accumulated into).  inference_net has none: it only feeds the MI loss. */
typedef struct {
  float *e0_w, *e0_b, *bn_w, *bn_b, *e3_w, *e3_b, *m0_w, *m0_b, *m2_w, *m2_b, *k_w, *k_b, *q_w, *q_b;
} marl_maic_grads_t;
/* Bytes of scratch marl_maic_head_bwd needs for bs environments of N agents with A actions (0 for an unsupported shape). */
size_t marl_maic_bwd_workspace(int bs, int N, int A);
/* Backward of marl_maic_head_fwd (maic_head_bwd.hip) for a sparse gradient on return_q: row r receives dq_val[r] on action
 * u_act[r] (an index outside [0, A) reads as no gradient) - the pairs marl_agent_unroll_bwd takes as (dq_idx, dq_val).
 *   h, eps, test_mode, bn_batch, var_floor, bn_eps: as the forward call had them (eps NULL in test mode).  Intermediates are
 *   recomputed; in batch-statistics mode so are the statistics, and bn_rm / bn_rv / bn_nbt are NOT moved.
 *   dh (bs*N, 64) is written: the head's contribution only (the identity path q -> return_q is BPTT's own dq input).
 *   The gradients of embed_net.{0,1,3}, msg_net.{0,2}, w_key and w_query are ACCUMULATED into g by fixed-order reductions
 *   (no float atomics: two calls give the same bits).  fp32 throughout; ws: marl_maic_bwd_workspace() bytes. */
int marl_maic_head_bwd(const marl_maic_weights_t* w, const marl_maic_grads_t* g, const float* h, const float* eps,
                       const int* u_act, const float* dq_val, float* dh, float* ws, size_t ws_bytes, int bs, int N, int A,
                       int test_mode, int bn_batch, float var_floor, float bn_eps, void* stream);
/* marl_maic_head_bwd with one more input: dpar_extra (bs*N, 2*N*L) or NULL, a gradient on the post-clamp [mean | var] planes of
 * embed_net (the MI term's, from marl_maic_aux).  It is added to the head's own d mean / d var before the clamp gate, so one
 * embed_net backward serves both terms; rows without a TD pair still carry it.  NULL: marl_maic_head_bwd, bit for bit. */
int marl_maic_head_bwd_ex(const marl_maic_weights_t* w, const marl_maic_grads_t* g, const float* h, const float* eps,
                          const int* u_act, const float* dq_val, const float* dpar_extra, float* dh, float* ws,
                          size_t ws_bytes, int bs, int N, int A, int test_mode, int bn_batch, float var_floor, float bn_eps,
                          void* stream);
/* ---- MAIC auxiliary losses (maic_aux.hip): the MI and the attention-entropy loss of network/MAIC.py:88-123 ------------
 * inference_net, torch layouts: i0 (64, 64 + A), ibn (64) weight / bias / running_mean / running_var / num_batches_tracked
 * (int64, may be NULL), i3 (2*L, 64). */
typedef struct {
  const float *i0_w, *i0_b, *ibn_w, *ibn_b;
  float *ibn_rm, *ibn_rv;
  long long* ibn_nbt;
  const float *i3_w, *i3_b;
} marl_maic_infer_t;
typedef struct {
  float *i0_w, *i0_b, *ibn_w, *ibn_b, *i3_w, *i3_b;
} marl_maic_infer_grads_t;
size_t marl_maic_aux_workspace(int bs, int N, int A);
/* Both losses and their gradients in one call over bs environments x N agents (rows as marl_maic_head_fwd):
 *   h, eps, test_mode, bn_batch, var_floor, bn_eps: as the head's forward call had them; return_q (bs*N, A): its output, read
 *   for the greedy actions only (lowest index on a tie, no mask).
 *   mi_out[0]  += mi_weight * mean over the bs*N*N pairs of sum_L KL(g1 || g2)           (MAIC.py:101-118)
 *   ent_out[0] += entropy_weight * mean over the bs*N rows of -sum_j a' log2 a', a' = max(alpha, 1e-4), alpha the softmax of
 *                 the UNSCALED, UNMASKED logits w_key(h) . w_query(latent)               (MAIC.py:93-97, 120-123)
 *   Every gradient is that of mi + ent times (den ? den[0] : 1) * dscale - the pre-scale for an optimizer that divides by den.
 *   dpar (bs*N, 2*N*L) is written: the MI term's gradient on the post-clamp [mean | var] planes (-> marl_maic_head_bwd_ex);
 *   dh (bs*N, 64) is written: the part of the MI gradient on h that comes through inference_net's input.
 *   ACCUMULATED: ig (inference_net: weights, biases, BatchNorm affine) and g->k_w, k_b, q_w, q_b (the entropy term; nothing else
 *   of g is touched; h and the latent are constants of that term, so it adds nothing to dh).
 *   bn_batch 1: both BatchNorms on the statistics of this call (inference_net.1 over all bs*N*N pair rows, needs >= 2), and
 *   with mi_weight > 0 inference_net.1's running statistics move ONCE, as torch moves them (unbiased variance,
 *   num_batches_tracked += 1); embed_net.1's buffers are never written.  Fixed-order reductions, no float atomics: two calls
 *   give the same bits.  fp32 throughout; ws: marl_maic_aux_workspace() bytes. */
int marl_maic_aux(const marl_maic_weights_t* w, const marl_maic_infer_t* iw, const marl_maic_grads_t* g,
                  const marl_maic_infer_grads_t* ig, const float* h, const float* eps, const float* return_q, float mi_weight,
                  float entropy_weight, const float* den, float dscale, float* mi_out, float* ent_out, float* dpar, float* dh,
                  float* ws, size_t ws_bytes, int bs, int N, int A, int test_mode, int bn_batch, float var_floor, float bn_eps,
                  float bn_momentum, void* stream);
/* eps (E*N, N*8) of a sampled-latent rollout step (replaces the torch generator behind rsample, MAIC.py:68): element (n, c) of
 * environment env0 + e is sqrt(-2 ln(1 - u1)) cos(2 pi u2) with u1, u2 the counter-hash draws 2k, 2k + 1 (k = n*N*8 + c) of
 * stream 8 keyed by (rseed, env, tg = the global step), as marl_select_actions draws its own. */
int marl_maic_noise(unsigned rseed, int env0, unsigned tg, float* eps, int E, int N, void* stream);

/* ---- CommNet communication head (commnet.hip) ---------------------------------------------------------------------------
 * The communicating actor of the +commnet algorithms (the reference ships only their argument table; the definition is this
 * project's own, taken from the published implementation the table comes from).  CommNetAgent, H = 64, K = args.k rounds:
 *   encoding = Linear(I, H), f_obs = GRUCell(H, H), f_comm = GRUCell(H, H), decoding = Linear(H, A)   (torch's gate order r, z, n)
 * Per step t and environment, over the N agent rows (x_t the virtual input [obs | one-hot(u_{t-1}) | agent id]):
 *   e      = sigmoid(encoding(x_t))
 *   h_t    = f_obs(e, h_{t-1})                  the ONLY recurrence in time: marl_agent_unroll_fwd over an identity front layer
 *   g^(0)  = f_comm(0, h_t)                     round 0 runs with a zero input: its input side is b_ih alone (also at K = 1)
 *   g^(j)  = f_comm(c^(j), g^(j-1)),  c_i^(j) = (sum over l != i of g_l^(j-1)) / N      j = 1 .. K-1: the divisor is N, not N - 1
 *   logits = decoding(g^(K-1))
 * Dead agents and finished environments are NOT masked out of the sum.  Nothing couples two environments or two steps.
 * The head entries below take G = B*T environment-steps ("groups") of N rows each; all rows of a group are in one workgroup, a
 * workgroup's 16-row tile holds marl_commnet_groups_per_workgroup(N) = 16 / N whole groups.  fp32 MFMA products. */
typedef struct {
  const float *w_ih, *w_hh, *b_ih, *b_hh;   /* f_comm: (192,64), (192,64), (192), (192) */
  const float *dec_w, *dec_b;               /* decoding: (A,64), (A) */
} marl_commnet_weights_t;
typedef struct {
  float *w_ih, *w_hh, *b_ih, *b_hh, *dec_w, *dec_b;
} marl_commnet_grads_t;
/* 1 when the head kernels cover the shape: 1 <= N <= 16, 1 <= A <= 32, 1 <= K <= 4.  Outside it both entries return
 * hipErrorInvalidValue and launch nothing. */
int marl_commnet_supported(int N, int A, int K);
int marl_commnet_groups_per_workgroup(int N);
/* logits (G,N,A) <- hs (G,N,64).  G = 0 launches nothing and returns 0. */
int marl_commnet_head_fwd(const marl_commnet_weights_t* w, const float* hs, float* logits, long G, int N, int A, int K,
                          void* stream);
/* The backward of marl_commnet_head_fwd: dhs (G,N,64) is WRITTEN with the gradient on hs for dlogits (G,N,A); the gradients of
 * f_comm's four tensors and of decoding's two are ADDED into g.  Every intermediate is recomputed from hs (nothing is kept by the
 * forward).  Reverse over the rounds: dc_i = dgi_i W_ih, and every other agent l of the group receives (sum_{i != l} dc_i) / N.
 * Weight gradients: one partial slab per workgroup, added in slab order by a second kernel - no float atomics, two calls give the
 * same bits.  ws: marl_commnet_bwd_workspace() bytes (at most 256 slabs of 27040 floats). */
size_t marl_commnet_bwd_workspace(long G, int N, int A, int K);
int marl_commnet_head_bwd(const marl_commnet_weights_t* w, const marl_commnet_grads_t* g, const float* hs, const float* dlogits,
                          float* dhs, float* ws, size_t ws_bytes, long G, int N, int A, int K, void* stream);
/* The encoder's sigmoid, elementwise over n floats: x <- sigmoid(x) in place (on marl_linear's output), and
 * dxp = de * e * (1 - e) (dxp may be de).  float4 over the 16-byte aligned middle; any 4-byte aligned view gives the same bits. */
int marl_commnet_sigmoid_fwd(float* x, long n, void* stream);
int marl_commnet_sigmoid_bwd(const float* de, const float* e, float* dxp, long n, void* stream);

/* ---- G2ANet attention head (g2anet.hip) ---------------------------------------------------------------------------------
 * The second communicating actor of the policy learners (+g2anet; the reference ships only the argument table get_g2anet_args:
 * attention_dim = 32, hard = True; the definition is this project's own, taken from the published implementation the table comes
 * from).  G2ANetAgent, H = 64, D = attention_dim = 32, 22 tensors under the published state-dict names:
 *   encoding = Linear(I, 64), h = GRUCell(64, 64), hard_bi_GRU = GRU(128, 64, bidirectional), hard_encoding = Linear(128, 2),
 *   q, k = Linear(64, 32, bias=False), v = Linear(64, 32), decoding = Linear(96, A)                  (torch's gate order r, z, n)
 * Per step t and environment, over the N agent rows (x_t the virtual input [obs | one-hot(u_{t-1}) | agent id]):
 *   h_t = h(relu(encoding(x_t)), h_{t-1})       the ONLY recurrence in time: marl_agent_unroll_fwd with fc1 = encoding, rnn = h
 *   hard (args.hard): the partners of agent i are j_1 < .. < j_{N-1}, all j != i; x_{i,p} = [h_i | h_{j_p}];
 *     f_{i,p} = GRU_fwd(x_{i,p}, f_{i,p-1}), f_{i,0} = 0;  b_{i,p} = GRU_rev(x_{i,p}, b_{i,p+1}), b_{i,N} = 0;
 *     y_{i,p} = hard_encoding([f_{i,p} | b_{i,p}]);  w_{i,p} = softmax((y + gumbel) / tau)[1] = sigmoid((y_1 - y_0 + l_{i,p}) / tau),
 *     l = g_1 - g_0 one Logistic(0, 1) draw per pair (the published gumbel_softmax(tau = 0.01, hard=False), column 1: a soft weight
 *     that is almost always 0 or 1; the gradient goes through the sigmoid, dy_1 = - dy_0 = dw w (1 - w) / tau).  hard off: w = 1,
 *     and the hard layers receive no gradient.
 *   soft: q_i = q(h_i), k_j = k(h_j), v_j = relu(v(h_j)); a_{i,.} = softmax over p of q_i . k_{j_p} / sqrt(32);
 *     x_i = sum_p a_{i,p} w_{i,p} v_{j_p}      (no renormalisation after w)
 *   logits_i = decoding([h_i | x_i])
 * Kept as published: noise in every pass (training and evaluation), tau = 0.01, dead agents and finished environments are not
 * masked out of the partners, N = 1 has no partner and is refused.  The (N-1) x 128 input of the bidirectional GRU is never built:
 * W_ih [h_i | h_j] = W_ih[:, :64] h_i + W_ih[:, 64:] h_j, so per direction P_i (with b_ih) and Q_j are computed once per row.
 * The entries take G = B*T environment-steps ("groups") of N rows each, marl_g2anet_groups_per_workgroup(N) = 16 / N whole groups
 * in a workgroup's 16-row tile.  fp32 MFMA products. */
typedef struct {
  const float *gf_w_ih, *gf_w_hh, *gf_b_ih, *gf_b_hh;   /* hard_bi_GRU *_l0: (192,128), (192,64), (192), (192) */
  const float *gr_w_ih, *gr_w_hh, *gr_b_ih, *gr_b_hh;   /* hard_bi_GRU *_l0_reverse */
  const float *he_w, *he_b;                             /* hard_encoding: (2,128), (2) */
  const float *q_w, *k_w, *v_w, *v_b;                   /* (32,64) each, (32) */
  const float *dec_w, *dec_b;                           /* decoding: (A,96), (A) */
} marl_g2anet_weights_t;
typedef struct {
  float *gf_w_ih, *gf_w_hh, *gf_b_ih, *gf_b_hh, *gr_w_ih, *gr_w_hh, *gr_b_ih, *gr_b_hh, *he_w, *he_b, *q_w, *k_w, *v_w, *v_b, *dec_w,
      *dec_b;
} marl_g2anet_grads_t;
/* 1 when the head kernels cover the shape: 2 <= N <= 10, 1 <= A <= 32, hard 0 or 1.  Outside it every entry returns
 * hipErrorInvalidValue and launches nothing. */
int marl_g2anet_supported(int N, int A, int hard);
int marl_g2anet_groups_per_workgroup(int N);
/* logits (G,N,A) <- hs (G,N,64) and noise (G,N,N-1) (NULL: l = 0; not read with hard off).  G = 0 launches nothing, returns 0. */
int marl_g2anet_head_fwd(const marl_g2anet_weights_t* w, const float* hs, const float* noise, float* logits, long G, int N, int A,
                         int hard, float tau, void* stream);
/* The backward of marl_g2anet_head_fwd on the same hs / noise / hard / tau: dhs (G,N,64) is WRITTEN with the gradient on hs for
 * dlogits (G,N,A); the gradients of the head's sixteen tensors are ADDED into g (hard off: the ten hard tensors are not touched).
 * Every intermediate is recomputed (nothing is kept by the forward): the forward kernel leaves the plane w (G,N,N-1) in ws, a soft
 * kernel (decoding, attention, q / k / v) replaces it by d(y_1 - y_0), one hard kernel per direction walks its chain in reverse.
 * Weight gradients: one partial slab per workgroup and kernel, added in slab order by reduce kernels - no float atomics, two
 * calls give the same bits.  ws: marl_g2anet_bwd_workspace() bytes (the plane and at most 256 slabs of 37504 floats). */
size_t marl_g2anet_bwd_workspace(long G, int N, int A, int hard);
int marl_g2anet_head_bwd(const marl_g2anet_weights_t* w, const marl_g2anet_grads_t* g, const float* hs, const float* noise,
                         const float* dlogits, float* dhs, float* ws, size_t ws_bytes, long G, int N, int A, int hard, float tau,
                         void* stream);
/* noise (E,T,N,N-1) of the hard attention: element (e, t, i, p) = ln(u) - ln(1 - u), u = (k + 0.5) / 2^24 with k the upper 24 bits of
 * the counter hash of stream ST_GUMBEL keyed by (seed, env0 + e, tg0 + t, i (N-1) + p): finite, |l| <= 17.4.  A rollout step is
 * T = 1 with tg0 = the global step, so one call over T steps from an episode's first global step gives the per-step draws. */
int marl_g2anet_noise(unsigned seed, int env0, unsigned tg0, float* noise, int E, int T, int N, void* stream);

/* ---- battle environment (battle.hip; rules: csrc/battle_env.h) ----------------------------------------------
 * A deterministic micro-combat simulator in SMAC's layout: N allies against M = N enemies of the same types on a 32 x 32 grid.
 * types: two bits per unit of a side, unit 0 lowest (0 marine, 1 stalker, 2 zealot); shield (0 / 1) and type_bits (0 .. 2) say
 * which feature columns the map has, A = 6 + M; observation width O = 4 + (M + N - 1)(5 + shield + type_bits) + 1 + shield +
 * type_bits, state width S = N (4 + shield + type_bits) + M (3 + shield + type_bits) + N A.  units (E, N + M, 5) int32: x, y, hp,
 * shield, cooldown, allies first.  The record is marl_record_t, with O and S the widths above: every entry returns
 * hipErrorInvalidValue for any other O or S.  marl_battle_supported(): 1 <= n_allies = n_enemies <= 16 and A = 6 + n_enemies; the
 * entries return hipErrorInvalidValue for anything else (and for a type without a bit, state_ld < S, t outside 0 .. T - 1) and
 * launch nothing. */
int marl_battle_supported(int n_allies, int n_enemies, int A);
/* start of episode `episode`: unit state (positions from the counter hash of (seed, env0 + e, episode, unit), streams 16 .. 19),
 * length = T, won = 0, and slot 0 of obs / state / avail; never touches u / r / term / padded */
int marl_battle_reset(unsigned seed, int env0, int episode, unsigned types, int shield, int type_bits, int* units,
                      const marl_record_t* rec, int M, void* stream);
/* lock-step t in one launch: reads act (E,N); writes u / r / term / padded of step t, length = t + 1 and won where the episode
 * ends here, alive_next (E; may be NULL) = 0 from the terminating step on, the new unit state and slot t + 1 of obs / state /
 * avail (the final observation at the terminating step).  Environments whose episode is over (t >= length) get u = -1, r = 0,
 * term = 1, padded = 1 and a zero slot.  r = (float)points * scale with points = hp + shield removed from enemies + 10 per kill +
 * 200 for the win; scale = 20 / (sum of enemy hp + shield + 10 M + 200) in fp32, from the caller. */
int marl_battle_step(unsigned types, int shield, int type_bits, float scale, int t, const int* act, int* units,
                     const marl_record_t* rec, int* alive_next, int M, void* stream);
/* The action choice and marl_battle_step in one launch.  q (E,1,N,A): ally n of a live environment chooses from its row and slot t's
 * availability in the record with marl_select_actions' epsilon-greedy rule and draws, keyed by (rseed, env0 + e, tg = episode (T + 1)
 * + t, n); -1 wherever t >= length[e].  Then the step, as marl_battle_step does it (no alive_next).  _sample: the choice is
 * marl_policy_sample's draw from the stochastic policy of the row instead, eps its mixing epsilon. */
int marl_battle_fused_step(unsigned types, int shield, int type_bits, float scale, unsigned rseed, int env0, int episode, int t,
                           float eps, const float* q, int* units, const marl_record_t* rec, int M, void* stream);
int marl_battle_fused_step_sample(unsigned types, int shield, int type_bits, float scale, unsigned rseed, int env0, int episode,
                                  int t, float eps, const float* q, int* units, const marl_record_t* rec, int M, void* stream);
/* Whole battle rollout, ONE persistent launch (csrc/battle_rollout.hip): marl_battle_reset and, for t = 0 .. T - 1, the agent step
 * (fp32 MFMA, marl_synth_rollout's sequences: q bit for bit the T = 1 unroll's), the choice and marl_battle_step, with the unit state
 * and the hidden state in LDS.  Writes every element of obs / state (S columns of a row) / avail / u / r / term / padded / length /
 * won - the zeros after an episode's end included - the final unit state to units, stats ([3][E], optional): sum_t r in step order |
 * won | length, and h_out (E N, 64; optional): the final hidden state.  Epsilon follows marl_synth_rollout's fp64 schedule
 * (eps0, eps_anneal, eps_min).  _sample: marl_synth_rollout_sample's draw instead of the epsilon-greedy choice.
 * marl_battle_rollout_supported(N, O, A): marl_battle_supported(N, N, A) and N within the 16-row tiles (at most 8) that 160 KB of
 * LDS hold with last action and agent id appended; the launch returns hipErrorInvalidValue for a shape no plan places, and for what
 * marl_battle_step refuses, and writes nothing.  marl_battle_rollout_plan: plan[0] = workgroups, plan[1] = environments per
 * workgroup (ceil(E / 256) until the row tiles are full), plan[2] = row tiles, plan[3] = dynamic LDS bytes. */
int marl_battle_rollout_supported(int N, int O, int A);
int marl_battle_rollout_plan(int E, int N, int O, int A, int last_action, int reuse_network, int* plan);
int marl_battle_rollout(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                        int episode, unsigned types, int shield, int type_bits, float scale, int* units, float* h_out,
                        float* stats, double eps0, double eps_anneal, double eps_min, int M, int last_action, int reuse_network,
                        void* stream);
int marl_battle_rollout_sample(const marl_agent_weights_t* w, const marl_record_t* rec, unsigned seed, unsigned rseed, int env0,
                               int episode, unsigned types, int shield, int type_bits, float scale, int* units, float* h_out,
                               float* stats, double eps0, double eps_anneal, double eps_min, int M, int last_action,
                               int reuse_network, void* stream);

/* ---- hunt environment (hunt.hip; rules: csrc/hunt_env.h) ------------------------------------------------------
 * Predator-prey with a lone-catch penalty: N predators (the agents) and M prey on a G x G grid, A = 6 (stay, four moves, catch).  A
 * prey is captured when two or more predators next to it catch in the same step (10 points); a prey with exactly one catcher costs
 * the team the penalty, which travels as the integer pen4 = 4 x penalty (0 .. 64).  Observation width O = 77 (a 5 x 5 window of
 * [another predator, a live prey, off the grid], then the own x and y ratios), state width S = 2 N + 3 M.  units (E, N + M, 3) int32:
 * x, y, live, predators first.  The record is marl_record_t, with O and S the widths above: every entry returns hipErrorInvalidValue
 * for any other O or S.  marl_hunt_supported(): 2 <= N <= 16, 1 <= M <= 16, 3 <= G <= 32 and A = 6; the entries return
 * hipErrorInvalidValue for anything else (and for pen4 outside 0 .. 64, state_ld < S, t outside 0 .. T - 1) and launch nothing. */
int marl_hunt_supported(int N, int M, int G, int A);
/* start of episode `episode`: unit state (positions from the counter hash of (seed, env0 + e, episode, unit), streams 32 .. 35, every
 * unit live), length = T, won = 0, and slot 0 of obs / state / avail; never touches u / r / term / padded */
int marl_hunt_reset(unsigned seed, int env0, int episode, int G, int M, int* units, const marl_record_t* rec, void* stream);
/* lock-step t in one launch: reads act (E,N); writes u / r / term / padded of step t, length = t + 1 and won where the episode
 * ends here (no prey left: won = 1; or t + 1 = T), alive_next (E; may be NULL) = 0 from the terminating step on, the new unit state
 * and slot t + 1 of obs / state / avail (the final observation at the terminating step).  Environments whose episode is over
 * (t >= length) get u = -1, r = 0, term = 1, padded = 1 and a zero slot.  r = (float)(40 captures - pen4 lone attempts) * 0.25f;
 * the prey that stay walk by the counter hash of (seed, env0 + e, tg = episode (T + 1) + t, prey), stream 36. */
int marl_hunt_step(unsigned seed, int env0, int episode, int G, int pen4, int t, const int* act, int* units,
                   const marl_record_t* rec, int* alive_next, int M, void* stream);
/* The action choice and marl_hunt_step in one launch.  q (E,1,N,A): predator n of a live environment chooses from its row and slot
 * t's availability in the record with marl_select_actions' epsilon-greedy rule and draws, keyed by (rseed, env0 + e, tg, n); -1
 * wherever t >= length[e].  Then the step, as marl_hunt_step does it (no alive_next).  _sample: the choice is marl_policy_sample's
 * draw from the stochastic policy of the row instead, eps its mixing epsilon. */
int marl_hunt_fused_step(unsigned seed, unsigned rseed, int env0, int episode, int G, int pen4, int t, float eps, const float* q,
                         int* units, const marl_record_t* rec, int M, void* stream);
int marl_hunt_fused_step_sample(unsigned seed, unsigned rseed, int env0, int episode, int G, int pen4, int t, float eps,
                                const float* q, int* units, const marl_record_t* rec, int M, void* stream);

/* ---- MAVEN (maven.hip; Mahajan et al., NeurIPS 2019 - the reference ships no MAVEN: the definition is this project's own) ---------
 * Sizes: K = noise_dim (1..32), H = 64, N agents (1..16), A actions (1..32), state width S, discriminator width D = 64.
 * Noise: every episode carries one index k in [0, K): marl_maven_noise writes noise[e] = hkey(rseed, stream 24, env0 + e, tg0, 0) % K
 *   for e < E (the counter hash of synth_env.h; stream 24 is declared in maven.hip), exploring or evaluating.
 * Agent: the plain shared agent plus the tables noise_w (K, A, H), id_w (N, A, H), noise_b (K, A), id_b (N, A); for episode b with
 *   noise k_b, agent n, hidden state h:   q'(b, t, n, :) = fc2(h) + (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n]
 *   - a hyper-layer Linear(K + N -> A H) applied to [one-hot(k) | one-hot(n)], whose bias matrix is fc2.
 * marl_maven_head_fwd: q (B, T, N, A) += the term, from hs (B, T, N, 64) and noise (B); an episode with k < 0 or k >= K is skipped:
 *   its q rows are not touched and its hs rows are not read.  A rollout step is B = E, T = 1.  fp32 in either gemm_mode.
 * marl_maven_head_bwd: g = scatter of the sparse pairs (dq_idx, dq_val) (both NULL: none) + dq_dense (NULL: 0), all over (B, T, N);
 *   writes dq_out (B, T, N, A) = g and dhs (B, T, N, 64) = g (noise_w[k_b] + id_w[n]) (zeros for a skipped episode), and ADDS
 *   d noise_w[k] += sum over the rows with k_b = k of g h^T, d id_w[n] += sum over the rows of agent n, d noise_b / d id_b likewise
 *   (a skipped episode adds nothing).  Partials: one slab of ws per workgroup, episodes in order, slabs added in slab order.
 * Discriminator, for a step (b, t) with m = 1 - padded:  p_n = softmax over the available actions of q'(b, t, n, :) (unavailable: 0),
 *   x = [p_0 | .. | p_{N-1} | s_{b,t}],  logits = W2 relu(W1 x + b1) + b2  (W1 (D, N A + S), W2 (K, D)),  ce = logsumexp(logits) - logits[k_b].
 * marl_maven_mi, one row launch over the rows = B T steps, forward and backward:  stats2[0] += sum m ce,  stats2[1] += sum m [argmax
 *   logits == k_b] (first index);  the gradients of lambda_mi sum m ce are ADDED into g (W1, b1, W2, b2) and written to dq_dense
 *   (B, T, N, A) through the softmax - exact zeros at padded steps and unavailable actions; no den factor (the optimizer divides).
 *   ce (rows) receives the per-step ce (0 where padded).  avail of (b, t, n) is read at avail + e avail_bs + (t N + n) A and
 *   the state row at state + (e state_bs + t) state_ld, with e = ep_map ? ep_map[b] : b (a replay sample reads the ring in place);
 *   x exists in LDS only.  A padded step, and a step of an episode with k_b outside [0, K), reads neither q, avail nor state.
 * Two calls on the same input give the same bits (no float atomics).  Supported (marl_maven_supported): the ranges above, D = 64 and
 *   N A + S small enough for a 16-step tile of x in LDS (96 KB with the kernel's other tiles; N A + S <= 832 always fits).  An unsupported shape,
 *   a NULL required pointer, a misaligned base (hs, noise_w, id_w in both head entries and W2: 16 bytes; every other base: 4 bytes), a short workspace, B T N >= 2^31 (the MI pass: B T > 2^31 - 2^20) or lambda_mi < 0 is
 *   hipErrorInvalidValue before anything is read or written; B T = 0 launches nothing.
 * marl_maven_plan (host only), plan[8]: [0] 16-step tiles per (episode, agent) of the head  [1] head forward workgroups  [2] slabs
 *   (= workgroups) of the head backward  [3] 16-step tiles of the MI pass  [4] its workgroups = slabs  [5] its dynamic LDS bytes
 *   [6] tiles the busiest MI workgroup walks  [7] LDS pitch of x in floats. */
typedef struct {
  const float *noise_w, *id_w, *noise_b, *id_b;
} marl_maven_weights_t;
typedef struct {
  float *noise_w, *id_w, *noise_b, *id_b;
} marl_maven_grads_t;
typedef struct {
  const float *w1, *b1, *w2, *b2;
} marl_maven_disc_t;
typedef struct {
  float *w1, *b1, *w2, *b2;
} marl_maven_disc_grads_t;
int marl_maven_supported(int N, int A, int K, int S, int D);
int marl_maven_plan(int B, int T, int N, int A, int K, int S, int* plan);
size_t marl_maven_bwd_workspace(int B, int N, int A, int K);
size_t marl_maven_mi_workspace(long rows, int N, int A, int K, int S);
int marl_maven_noise(unsigned rseed, int env0, unsigned tg0, int K, int* noise, int E, void* stream);
int marl_maven_head_fwd(const marl_maven_weights_t* w, const float* hs, const int* noise, float* q, int B, int T, int N, int A,
                        int K, void* stream);
int marl_maven_head_bwd(const marl_maven_weights_t* w, const marl_maven_grads_t* g, const float* hs, const int* noise,
                        const int* dq_idx, const float* dq_val, const float* dq_dense, float* dq_out, float* dhs, float* ws,
                        size_t ws_bytes, int B, int T, int N, int A, int K, void* stream);
int marl_maven_mi(const marl_maven_disc_t* d, const marl_maven_disc_grads_t* g, const float* q, const float* avail,
                  long avail_bs, const float* state, long state_ld, long state_bs, const int* ep_map, const int* noise,
                  const float* padded, float lambda_mi, float* dq_dense, float* ce, float* stats2, float* ws, size_t ws_bytes,
                  int B, int T, int N, int A, int S, int K, void* stream);

const char* marl_hip_version(void);

/* Experiment switches (A/B measurements, variant tests): one table per process; NO entry point reads the environment.
 * Names and defaults: "fwd_xs" 1 (the double-Q unroll reads the eval unroll's input-side gate sums - replaces the work
 * q_learner.py:110 repeats), "fwd_w2l" 1 (six prefetch registers for wide observations), "bwd_pipe_max_rt" 4 (row tiles per
 * workgroup up to which the one-barrier BPTT runs), "wgrad_tall" 1 (LDS-staged tall weight-gradient kernel), "wide_res" 1
 * (resident-weights forward of the wide-state QMIX mixer, mixer.py:57-80), "rollout_v1" 0 / "unroll_r6" 1 (split rollout and
 * unroll kernel choice, common.h: MarlSwitches).
 * Results do not depend on them beyond fp32 summation order.  set: 0, or -1 for an unknown name; get: the value, or INT_MIN.
 * marl_amd/experiments.py forwards the MARL_* environment variables of the same names once, at import. */
int marl_experiment_set(const char* name, int value);
int marl_experiment_get(const char* name);

#ifdef __cplusplus
}
#endif
#endif
