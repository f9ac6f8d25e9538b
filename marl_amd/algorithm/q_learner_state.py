"""QLearnerWithState (mirror of reference algorithm/q_learner_state.py:10-262): QLearner for a SharedMACWithState.

``train`` is QLearner's schedule with the reference's changes (q_learner_state.py:94-187):
  - every Q tensor includes the world head's r (network/world_model.py:71): the three unrolls write their hidden states
    (hs) and csrc/world_head.hip adds r to the eval, double-Q continuation and target Qs before the gathers, the greedy
    selections and the mixers (QPLEX's max_q included); quirks Q1 and Q2 stay as in QLearner;
  - the eval pass's head runs in train mode and adds sum (o_hat - o_next)^2 over all B*T*N*O entries - unmasked: padded
    steps count with o_next = 0 (:175-181) - into the third slot of the loss statistics;
  - after the TD loss the head's backward turns dq (the sparse pairs BPTT receives: dr = dq) and
    d_o_hat = 2 (o_hat - o_next) den / K into the gradient on hs and the head's weight gradients; BPTT takes that dhs.
    K = B*T*N*O is a host constant per shape; den = sum(mask) stays on the device.  The optimizer divides the whole
    gradient by den (FusedOptimizer.step), which leaves the prediction term at its 1 / K - exact in one process;
  - the returned loss is TD + pred: s[0] / s[1] + s[2] / K.
terminate_out never reaches a loss: its gradient is zero and it does not move (RMSprop and Adam leave a parameter with zero
gradient and zero state unchanged), but it stays in the parameter list, the clip norm and the flat buffer.
Multi-rank training is not supported: the prediction term's scale needs the global sum(mask) before the all-reduce.
"""
from __future__ import annotations

import torch

from .. import ops
from .common import MASK_BIG, agent_backward
from .q_learner import QLearner


class QLearnerWithState(QLearner):
    def __init__(self, mac, args):
        if not getattr(mac, "world", False):
            raise TypeError("QLearnerWithState needs a SharedMACWithState controller")
        super().__init__(mac, args)
        if self.reducer.enabled:
            raise NotImplementedError("multi-rank world-model training: the prediction loss is scaled by den / K on the "
                                      "device, and the global sum(mask) is only known after the gradient all-reduce")
        self._B = 0

    def _forward_backward(self, db):
        a = self.args
        dev = self.device
        B, T, N, A, O, H = db.B, db.T, db.N, db.A, db.O, a.rnn_hidden_dim
        R, BT = B * T * N, B * T
        self._B = B
        g = lambda name, shape, dt=torch.float32: self._buf.get(name, shape, dev, dt)
        q_evals, hs, saved = g("q_evals", (B, T, N, A)), g("hs", (B, T, N, H)), g("saved", ops.saved_shape(T, B, N))
        h_last, h_scr = g("h_last", (B * N, H)), g("h_scr", (B * N, H))
        q_tgt, q_en = g("q_tgt", (B, T, N, A)), g("q_en", (B, T, N, A))
        hs_tgt, hs_en = g("hs_tgt", (B, T, N, H)), (g("hs_en", (B, T, N, H)) if a.double_q else None)
        q_chosen, q_tgt_chosen = g("q_chosen", (R,)), g("q_tgt_chosen", (R,))
        (oc, oc_bs, oc_t0), (on, on_bs, on_t0) = db.o_cur, db.o_next
        u_act = db.u_act.reshape(-1)
        emap = getattr(db, 'o_map', None)
        # the loss statistics are zeroed first: the eval head's train-mode forward adds its sum into stats[2]
        self._flat.zero_grad()

        # the three unrolls as QLearner's (quirk Q1, the pair / chain schedule), each writing hs: every unroll kernel stores
        # hs when given it, the gi_in continuation included; the bf16x6 entry runs hs-writing launches on csrc/agent_x6.hip
        # (never the non-saving agent_x6p.hip path), so the input-side gate sums pair up as in QLearner
        cont, gi = None, None
        if a.double_q:
            shifted = on is oc and on_bs == oc_bs and on_t0 == oc_t0 + 1
            split = self.pair.chain_split(B * N, T, a.obs_shape)
            from .. import experiments
            if shifted and ((self.eval_net.unroll_x6(B, T, oc) and experiments.get("fwd_xs") != 0) or
                            ops.agent_unroll_reuse_supported(B, T, N, a.obs_shape, A, split[0] if split else 256)):
                gi = g("gi", ops.saved_shape(T, B, N, planes=3))
            cont = lambda cu: self.eval_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, q_en, hs_en, h_scr, None,
                                                   h0=h_last, ep_len=db.ep_len, ep_map=emap, cu_budget=cu, gi_in=gi)
        self.pair.run_chain(B * N, T, a.obs_shape,
                            lambda cu: self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, q_evals, hs, h_last, saved,
                                                            h0=None, ep_len=db.ep_len, ep_map=emap, cu_budget=cu, gi_out=gi),
                            cont,
                            lambda cu: self.target_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, q_tgt, hs_tgt, None, None,
                                                              h0=None, ep_len=db.ep_len, ep_map=emap, cu_budget=cu))
        # world heads: q += r (q_learner_state.py:95,103,107 through world_model.py:71); the eval pass also forms o_hat and
        # adds sum (o_hat - o_next)^2 (:181, o_next = the next observations the target unroll reads, zeros past ep_len)
        w_eval, w_tgt = self.eval_net.agent.world_weights(), self.target_net.agent.world_weights()
        onext = dict(obs=on, obs_bs=on_bs, obs_t0=on_t0, ep_len=db.ep_len, ep_map=emap)
        ops.world_head_fwd(w_eval, hs, q_evals, B, T, N, O, A, loss=self._flat.stats[2:3], **onext)
        if a.double_q:
            ops.world_head_fwd(w_eval, hs_en, q_en, B, T, N, O, A)
        ops.world_head_fwd(w_tgt, hs_tgt, q_tgt, B, T, N, O, A)

        ops.q_gather(q_evals, u_act, q_chosen, R, A)
        cur_max = None
        if a.double_q:
            cur_max = g("cur_max", (R,), torch.int32)
            ops.q_double_select(q_en, q_tgt, db.avail_next, MASK_BIG, q_tgt_chosen, cur_max, R, A)
        else:
            ops.q_masked_max(q_tgt, db.avail_next, MASK_BIG, q_tgt_chosen, None, R, A)

        ctx = {}
        qc, qtc = q_chosen.view(BT, N), q_tgt_chosen.view(BT, N)
        fold = False
        if a.alg == 'qplex':
            max_q = g("max_q", (R,))
            ops.q_masked_max(q_evals, db.avail, MASK_BIG, max_q, None, R, A)
            v_tot, a_tot = self.mixer.hip_forward(qc, db.s, BT, u_idx=db.u_taken.reshape(-1), max_q=max_q.view(BT, N), ctx=ctx)
            q_tot = g("q_tot", (BT,))
            ops.vec_add(v_tot, a_tot, q_tot, BT)
            if a.double_q:
                tgt_max = g("tgt_max", (R,))
                ops.q_masked_max(q_tgt, db.avail_next, MASK_BIG, tgt_max, None, R, A)
                vt, at = self.target_mixer.hip_forward(qtc, db.s_next, BT, u_idx=cur_max, max_q=tgt_max.view(BT, N), tag="t")
                q_tot_tgt = g("q_tot_tgt", (BT,))
                ops.vec_add(vt, at, q_tot_tgt, BT)
            else:
                q_tot_tgt, _ = self.target_mixer.hip_forward(qtc, db.s_next, BT, tag="t")
        else:
            fold = a.alg == 'qmix' and getattr(self.mixer, "loss_backward_fused", None) is not None and \
                self.mixer.loss_backward_fused(db.s) and not getattr(a, "no_loss_fold", False)
            q_tot = g("q_tot", (BT,)) if fold else self.mixer.hip_forward(qc, db.s, BT, ctx=ctx)
            q_tot_tgt = self.target_mixer.hip_forward(qtc, db.s_next, BT, tag="t")

        if fold:
            dq_chosen = self.mixer.hip_loss_backward(qc, db.s, BT, q_tot_tgt, db.r, db.term, db.padded, self.gamma,
                                                     self._flat.stats[:2], q_tot=q_tot)
        else:
            dq_tot = g("dq_tot", (BT,))
            ops.td_loss(q_tot, q_tot_tgt, db.r, db.term, db.padded, self.gamma, dq_tot, self._flat.stats[:2], BT)
            dq_chosen = self.mixer.hip_backward(ctx, dq_tot, BT)
        dq_val = dq_chosen.reshape(-1).contiguous()
        # world head backward (stats[1] = sum(mask) is ready): dr = dq, d_o_hat = 2 (o_hat - o_next) den / K -> dhs + head grads
        dhs = g("dhs", (B, T, N, H))
        ops.world_head_bwd(w_eval, self.eval_net.agent.world_grads(), hs, u_act, dq_val, on, on_bs, on_t0,
                           self._flat.stats[1:2], 2.0 / (R * O), dhs, B, T, N, O, A, ep_len=db.ep_len, ep_map=emap)
        agent_backward(self.eval_net, db, "cur", saved, hs, None, dhs, self._buf, dq_idx=u_act, dq_val=dq_val)
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, q_tot_target=q_tot_tgt, hs=hs)

    def _finish_update(self, train_step):
        """QLearner's, with the loss TD + pred = s[0] / s[1] + s[2] / K (q_learner_state.py:183)"""
        self.reducer.allreduce_(self._flat.gradx)
        stats = self._flat.stats
        self.optimizer.step(den=stats[1:2])
        if train_step > 0 and train_step % self.args.target_update_cycle == 0:
            self._update_targets()
        self.last_stats = stats
        K = float(self._B * self.max_episode_len * self.args.n_agents * self.args.obs_shape)
        return self.loss_readback.read(stats[:3], lambda s: s[0] / s[1] + s[2] / K)
