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
``args.td_lambda`` reaches this learner through QLearner._loss_backward (the lambda-returns of q_tot_target, r included) with no
lines of its own.
Multi-rank training is not supported: the prediction term's scale needs the global sum(mask) before the all-reduce.
"""
from __future__ import annotations

from .. import ops
from .common import agent_backward
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

    n_stats = 3               # TD numerator, sum(mask), prediction sum

    def _forward_backward(self, db):
        B, T, N, A, O, H = db.B, db.T, db.N, db.A, db.O, self.args.rnn_hidden_dim
        self._B = B
        # the loss statistics are zeroed first: the eval head's train-mode forward adds its sum into stats[2]
        self._flat.zero_grad()
        q_evals, q_en, q_tgt, saved, (hs, hs_en, hs_tgt) = self._unrolls(db, keep_hs=True)
        # world heads: q += r (q_learner_state.py:95,103,107 through world_model.py:71); the eval pass also forms o_hat and
        # adds sum (o_hat - o_next)^2 (:181, o_next = the next observations the target unroll reads, zeros past ep_len)
        w_eval, w_tgt = self.eval_net.agent.world_weights(), self.target_net.agent.world_weights()
        on, on_bs, on_t0 = db.o_next
        emap = getattr(db, 'o_map', None)
        ops.world_head_fwd(w_eval, hs, q_evals, B, T, N, O, A, loss=self._flat.stats[2:3],
                           obs=on, obs_bs=on_bs, obs_t0=on_t0, ep_len=db.ep_len, ep_map=emap)
        if self.args.double_q:
            ops.world_head_fwd(w_eval, hs_en, q_en, B, T, N, O, A)
        ops.world_head_fwd(w_tgt, hs_tgt, q_tgt, B, T, N, O, A)

        q_chosen, q_tgt_chosen, cur_max = self._select(db, q_evals, q_en, q_tgt)
        q_tot, q_tot_tgt, ctx, fold = self._mix(db, q_evals, q_tgt, q_chosen, q_tgt_chosen, cur_max)
        dq_val = self._loss_backward(db, q_chosen, q_tot, q_tot_tgt, ctx, fold).reshape(-1).contiguous()
        # world head backward (stats[1] = sum(mask) is ready): dr = dq, d_o_hat = 2 (o_hat - o_next) den / K -> dhs + head grads
        u_act = db.u_act.reshape(-1)
        dhs = self._g("dhs", (B, T, N, H))
        ops.world_head_bwd(w_eval, self.eval_net.agent.world_grads(), hs, u_act, dq_val, on, on_bs, on_t0,
                           self._flat.stats[1:2], 2.0 / (B * T * N * O), dhs, B, T, N, O, A, ep_len=db.ep_len, ep_map=emap)
        agent_backward(self.eval_net, db, "cur", saved, hs, None, dhs, self._buf, dq_idx=u_act, dq_val=dq_val)
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, q_tot_target=q_tot_tgt, hs=hs, **self._td_dbg)

    def _loss_fn(self):
        """TD + pred = s[0] / s[1] + s[2] / K (q_learner_state.py:183)"""
        K = float(self._B * self.max_episode_len * self.args.n_agents * self.args.obs_shape)
        return lambda s: s[0] / s[1] + s[2] / K
