"""CentralVLearner: central-V actor-critic (the reference ships its argument table, common/arguments.py:151-177, and no code; the
definitions are this project's own, from the published algorithm - DESIGN section 9).

The actor is the shared RNN agent read as a stochastic policy (PolicyMAC, csrc/policy.hip); the critic is a state-value MLP
V(s) = Linear(S, critic_dim) - ReLU - Linear(critic_dim, critic_dim) - ReLU - Linear(critic_dim, 1) with a target copy.  With
m = 1 - padded, M = sum m and G the lambda-returns of V_target(s_next) (csrc/td_lambda.hip; a constant of the gradient):

    L_critic = sum m (G - V(s))^2 / M          Adv = G - V(s)  (the same forward pass, a constant of the gradient)
    L_actor  = [ - sum m Adv log pi(u) - beta sum m H ] / (N M)

beta = ``args.policy_entropy_coef`` >= 0 (default 0) weighs the entropy H of the policy each action was drawn from (algorithm/
reinforce.py has the definition).  With 0 the actor pass is ops.policy_loss_bwd, exactly as before the bonus existed; a positive
value runs ops.policy_loss_bwd_ex with v and leaves the mean entropy per live agent step in ``self.entropy``.

One update pass: the eval unroll with saved planes, the critic on s, the target critic on s_next, td_lambda_returns, td_loss on
(V, G) - the ``_td_inputs`` idiom: G as r, gamma = 0 -, the critic backward, policy_loss_bwd, BPTT on its dense gradient.  Two
flat buffers, two optimizers of ``args.optimizer``'s kind (lr_actor over the agent, lr_critic over the critic), each with its own
clip and its own denominator (N M and M); the target critic follows every ``target_update_cycle`` updates; there is no target
actor.  ``args.td_lambda`` None means 0, the one-step target.  No hipGraph replay, no launch ahead of max_episode_len, one rank.
Construction, storage, the tail of an update, checkpoints and resume state are PolicyLearner's (algorithm/policy_learner.py).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..hostutil import lin_of
from .policy_learner import PolicyLearner


class VCritic(nn.Module):
    """V(s) (torch's default init); run through ops.linear / ops.linear_wgrad by the learner"""

    def __init__(self, args):
        super().__init__()
        self.fc1 = nn.Linear(args.state_shape, args.critic_dim)
        self.fc2 = nn.Linear(args.critic_dim, args.critic_dim)
        self.fc3 = nn.Linear(args.critic_dim, 1)

    def forward(self, s):
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(s)))))


class CentralVLearner(PolicyLearner):
    extra_nets = ("critic",)
    _no_q_table = "central-V has no Q table: its critic is a state value"

    def _make_critic(self, args):
        return VCritic(args)

    # ------------------------------------------------------------------ the hot path
    def _critic_forward(self, net, s, BT, tag, keep):
        """V (BT, 1) of the states s (Rows or a dense view); keep: the two hidden layers' outputs as well (the backward's ReLU gates)"""
        D, g = self.args.critic_dim, self._g
        h1, h2, v = g("c_h1" + tag, (BT, D)), g("c_h2" + tag, (BT, D)), g("c_v" + tag, (BT, 1))
        lin_of(net.fc1).fwd(ops.src(s), h1, BT, act=1)
        lin_of(net.fc2).fwd(ops.src(h1), h2, BT, act=1)
        lin_of(net.fc3).fwd(ops.src(h2), v, BT)
        return (v, h1, h2) if keep else v

    def _critic_backward(self, s, h1, h2, dv, BT):
        """autograd of _critic_forward for the gradient dv (BT, 1) on V: accumulates into the critic's .grad views"""
        D, g, c = self.args.critic_dim, self._g, self.critic
        dh2, dh1 = g("c_dh2", (BT, D)), g("c_dh1", (BT, D))
        l1, l2, l3 = lin_of(c.fc1), lin_of(c.fc2), lin_of(c.fc3)
        l3.wgrad(dv, ops.src(h2), BT)
        l3.bwd_x(dv, dh2, BT)
        l2.wgrad(dh2, ops.src(h1), BT, Yact=h2)
        l2.bwd_x(dh2, dh1, BT, Yact=h2)
        l1.wgrad(dh1, ops.src(s), BT, Yact=h1)

    def _forward_backward(self, db):
        g = self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        BT, R = B * T, B * T * N
        lam = self._lambda()
        # 1. the eval unroll keeps its activations for BPTT
        logits, saved, hs = self._actor_unroll(db)
        # 2. - 4. V(s), V_target(s_next) and its lambda-returns (padded steps carry zero states: finite on every row)
        v, h1, h2 = self._critic_forward(self.critic, db.s, BT, "", True)
        v_next = self._critic_forward(self.target_critic, db.s_next, BT, "t", False)
        G = g("td_ret", (BT,))
        ops.td_lambda_returns(v_next.view(BT), db.r, db.term, db.padded, self.gamma, lam, G, B, T)
        # 5. - 6. the critic: target G + 0 V_next (1 - term) = G
        self._flat.zero_grad()
        self._cflat.zero_grad()
        dv = g("c_dv", (BT, 1))
        ops.td_loss(v.view(BT), v_next.view(BT), G, db.term, db.padded, 0.0, dv.view(BT), self._cflat.stats[:2], BT)
        self._critic_backward(db.s, h1, h2, dv, BT)
        # 7. - 8. the actor: Adv = G - V is formed inside the loss kernel; its dense gradient on the logits goes to BPTT
        dlogits, logp = g("dlogits", (B, T, N, A)), g("logp", (R,))
        self._dbg = dict(logits=logits, v=v.view(BT), v_next=v_next.view(BT), td_targets=G, logp=logp, dlogits=dlogits)
        if self.beta == 0.0:
            ops.policy_loss_bwd(logits, db.avail, db.u_act.reshape(-1), G, v.view(BT), db.padded, self.epsilon, dlogits, logp,
                                self._flat.stats[:2], R, N, A)
        else:                                        # the entropy bonus, folded into the same pass: stats = {numerator, N M, sum m H}
            ent = self._dbg["ent"] = g("ent", (R,))
            ops.policy_loss_bwd_ex(logits, db.avail, db.u_act.reshape(-1), G, v.view(BT), db.padded, self.epsilon, self.beta,
                                   dlogits, logp, ent, self._flat.stats[:3], R, N, A)
        self._actor_backward(db, saved, hs, dlogits)
