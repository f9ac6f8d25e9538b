"""ReinforceLearner: REINFORCE on the shared RNN agent read as a stochastic policy (the reference ships its argument table,
common/arguments.py:180-199, and no code; the definitions are this project's own - DESIGN section 9, include/marl_hip.h).

With m = 1 - padded, M = sum m, G the discounted Monte-Carlo return of the episode (csrc/td_lambda.hip at lambda = 1 on an all-zero
q_next: an episode cut at max_episode_len gets no bootstrap), H_r = - sum_{a_k = 1} pi_k log pi_k the entropy of the policy a row's
action was drawn from (eps mixing included; 0 log 0 = 0; 0 on a row without a policy) and beta = args.policy_entropy_coef >= 0:

    Adv = G  (no baseline)          L = [ - sum m G log pi(u) - beta sum m H ] / (N M)

One update pass: the eval unroll with saved planes, td_lambda_returns, policy_loss_bwd_ex with v = None, the fp32 BPTT on its dense
gradient.  One flat buffer, one optimizer of ``args.optimizer``'s kind at lr_actor with grad_norm_clip and the denominator N M.  No
critic, no target network (``target_update_cycle`` is not read), no hipGraph replay, no launch ahead of max_episode_len, one rank.
Everything but the pass itself is PolicyLearner's (algorithm/policy_learner.py), taken without a critic.
"""
from __future__ import annotations

from .. import ops
from .policy_learner import PolicyLearner, entropy_coef_of      # noqa: F401  (entropy_coef_of: importable from here as before)


class ReinforceLearner(PolicyLearner):
    _no_q_table = "REINFORCE has no Q table: it has no critic"

    def _forward_backward(self, db):
        g = self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        BT, R = B * T, B * T * N
        logits, saved, hs = self._actor_unroll(db)
        # the Monte-Carlo return: lambda = 1 leaves q_next only in the bootstrap of an unterminated episode, and q_next is 0
        G, q0 = g("td_ret", (BT,)), g("q_next0", (BT,))
        q0.zero_()
        ops.td_lambda_returns(q0, db.r, db.term, db.padded, self.gamma, 1.0, G, B, T)
        self._flat.zero_grad()
        dlogits, logp, ent = g("dlogits", (B, T, N, A)), g("logp", (R,)), g("ent", (R,))
        ops.policy_loss_bwd_ex(logits, db.avail, db.u_act.reshape(-1), G, None, db.padded, self.epsilon, self.beta, dlogits, logp,
                               ent, self._flat.stats[:3], R, N, A)
        self._actor_backward(db, saved, hs, dlogits)
        self._dbg = dict(logits=logits, td_targets=G, logp=logp, ent=ent, dlogits=dlogits)
