"""COMALearner: counterfactual multi-agent policy gradients (the reference ships its argument table, common/arguments.py:56-83, and
no code; the definitions are this project's own, from the published algorithm - DESIGN section 9, include/marl_hip.h).

The actor is the shared RNN agent read as a stochastic policy (PolicyMAC, csrc/policy.hip).  The critic is the published COMA
critic, Q(s, o_i, u_-i, u(t-1), i) for all of agent i's actions at once: fc1 = Linear(K, D) - ReLU - fc2 = Linear(D, D) - ReLU -
fc3 = Linear(D, A), D = critic_dim, over the per-row input

    [ s | o_i | one-hot(u_j) for every agent j, agent i's own block zeroed | one-hot(u_j at t-1) for all j | one-hot(i) ]

of width K = S + O + 2 N A + N (the column order of fc1.weight; actions j-major; last actions all zero at t = 0; the input does not
depend on args.last_action).  The input is never built: the first layer is one state product per step, one observation product per
row and a gather-add of 2 N columns of fc1.weight (csrc/coma.hip).  With m = 1 - padded, M = sum m, pi the policy the actions were
drawn from, Q' the target critic run on the same T steps:

    q_next[b, i, t] = Q'[b, t+1, i, u[b, t+1, i]]  (t + 1 < T),   q_next[b, i, T-1] = 0
    G[b, i, .]      = the lambda-returns of q_next (csrc/td_lambda.hip on B N sequences; a constant of the gradient)
    Adv_r           = Q_r(u_r) - sum_k pi_r(k) Q_r(k)                                   (a constant of the gradient)
    L_critic        = sum m (G - Q(u))^2 / (N M)
    L_actor         = [ - sum m Adv log pi(u) - beta sum m H ] / (N M)

Quirk: the window's last step has no successor action in the batch, so q_next is 0 there and an episode cut at max_episode_len
gets no bootstrap (REINFORCE's convention here).  beta = ``args.policy_entropy_coef`` >= 0, H as in algorithm/reinforce.py.

One update pass: the eval unroll with saved planes (the split kernel in gemm_mode "bf16x6"; the critic and the BPTT are fp32), the
critic, the target critic, coma_q_taken, td_lambda_returns, coma_loss_bwd (both losses, dlogits and dQ from one pass), the critic
backward, BPTT.  Storage, the two optimizers (lr_actor, lr_critic; both denominators N M), the target sync, checkpoints and resume
state are PolicyLearner's (algorithm/policy_learner.py), as CentralVLearner's.  ``args.td_lambda`` None means 0.  No target actor,
one rank, no hipGraph replay.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..hostutil import lin_of
from .central_v import CentralVLearner


def critic_input_dim(args):
    return args.state_shape + args.obs_shape + 2 * args.n_agents * args.n_actions + args.n_agents


class QCritic(nn.Module):
    """the COMA critic as plain nn.Linears (torch's default init): a checkpoint has the published layout.  ``forward`` takes the
    concatenated (..., K) input; the learner never builds it"""

    def __init__(self, args):
        super().__init__()
        self.fc1 = nn.Linear(critic_input_dim(args), args.critic_dim)
        self.fc2 = nn.Linear(args.critic_dim, args.critic_dim)
        self.fc3 = nn.Linear(args.critic_dim, args.n_actions)

    def forward(self, x):
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x)))))


class COMALearner(CentralVLearner):
    _no_q_table = "COMA has no joint Q table: its critic is counterfactual, one agent's actions at a time"

    def _make_critic(self, args):
        return QCritic(args)

    # ------------------------------------------------------------------ the hot path
    @staticmethod
    def _obs_rows(db):
        """the current-step observations as a (R, O) row source"""
        obs, bs, t0 = db.o_cur
        T, N = db.T, db.N
        emap = getattr(db, 'o_map', None)
        remap = None if (bs == T * N and t0 == 0 and emap is None) else (T * N, bs, t0 * N)
        return ops.src(obs.reshape(-1, db.O), remap0=remap, emap0=emap)

    def _critic_forward(self, net, db, tag, keep):
        """Q (R, A) of every agent step; keep: the two hidden layers' outputs as well (the backward's ReLU gates)"""
        D, g = self.args.critic_dim, self._g
        B, T, N, A, S, O = db.B, db.T, db.N, db.A, db.S, db.O
        BT, R, C = B * T, B * T * N, 2 * N * A + N
        w, b = net.fc1.weight.data, net.fc1.bias.data
        K = w.shape[1]
        wt, pre_s = g("c_wt" + tag, (C, D)), g("c_pre_s" + tag, (BT, D))
        h1, h2, q = g("c_h1" + tag, (R, D)), g("c_h2" + tag, (R, D)), g("c_q" + tag, (R, A))
        ops.coma_onehot_cols(w, S + O, wt, C, D)                      # the one-hot columns K-major, once per update
        ops.linear(ops.src(db.s), w[:, :S], b, pre_s, BT, D, S, ldw=K)
        ops.linear(self._obs_rows(db), w[:, S:S + O], None, h1, R, D, O, ldw=K)
        ops.coma_fc1_fwd(pre_s, wt, db.u_act.reshape(-1), h1, B, T, N, A, D)
        lin_of(net.fc2).fwd(ops.src(h1), h2, R, act=1)
        lin_of(net.fc3).fwd(ops.src(h2), q, R)
        return (q, h1, h2) if keep else q

    def _critic_backward(self, db, h1, h2, dq):
        """autograd of _critic_forward for the gradient dq (R, A) on Q: accumulates into the critic's .grad views"""
        D, g, c = self.args.critic_dim, self._g, self.critic
        B, T, N, A, S, O = db.B, db.T, db.N, db.A, db.S, db.O
        BT, R = B * T, B * T * N
        dh2, dh1, dsum = g("c_dh2", (R, D)), g("c_dh1", (R, D)), g("c_dsum", (BT, D))
        l2, l3 = lin_of(c.fc2), lin_of(c.fc3)
        l3.wgrad(dq, ops.src(h2), R)
        l3.bwd_x(dq, dh2, R)
        l2.wgrad(dh2, ops.src(h1), R, Yact=h2)
        l2.bwd_x(dh2, dh1, R, Yact=h2)
        gw = c.fc1.weight.grad
        K = gw.shape[1]
        ops.coma_fc1_bwd(dh1, h1, db.u_act.reshape(-1), dh1, dsum, gw, S + O, B, T, N, A, D)       # dh1 becomes the gated dpre
        ops.linear_wgrad(dsum, ops.src(db.s), gw[:, :S], c.fc1.bias.grad, BT, D, S, lddw=K)
        ops.linear_wgrad(dh1, self._obs_rows(db), gw[:, S:S + O], None, R, D, O, lddw=K)

    def _forward_backward(self, db):
        g = self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        R = B * T * N
        lam = self._lambda()
        # 1. the eval unroll keeps its activations for BPTT
        logits, saved, hs = self._actor_unroll(db)
        # 2. - 4. Q, the target critic's Q of the next step's taken action, its lambda-returns per agent (r, term and padded are
        # expanded over the agents on the host side: plumbing)
        u = db.u_act.reshape(-1)
        q, h1, h2 = self._critic_forward(self.critic, db, "", True)
        q_tgt = self._critic_forward(self.target_critic, db, "t", False)
        q_next, G = g("q_next", (B, N, T)), g("td_ret", (B, N, T))
        ops.coma_q_taken(q_tgt, u, q_next, 1, B, T, N, A)
        per_agent = g("per_agent", (3, B, N, T))
        for k, x in enumerate((db.r, db.term, db.padded)):
            per_agent[k].copy_(x.view(B, 1, T).expand(B, N, T))
        ops.td_lambda_returns(q_next, per_agent[0], per_agent[1], per_agent[2], self.gamma, lam, G, B * N, T)
        # 5. both losses and both gradients from one pass over the rows
        self._flat.zero_grad()
        self._cflat.zero_grad()
        dlogits, dq = g("dlogits", (B, T, N, A)), g("c_dq", (R, A))
        logp, ent, adv, q_taken = g("logp", (R,)), g("ent", (R,)), g("adv", (R,)), g("q_taken", (R,))
        ops.coma_loss_bwd(logits, db.avail, q, u, G, db.padded, self.epsilon, self.beta, dlogits, dq, logp, ent, adv, q_taken,
                          self._cflat.stats[:2], self._flat.stats[:3], B, T, N, A)
        self._dbg = dict(logits=logits, q=q, q_taken=q_taken, q_next=q_next, td_targets=G, adv=adv, logp=logp, dlogits=dlogits,
                         ent=ent)
        # 6. - 7. the critic backward, and BPTT on the dense gradient of the logits (the fp32 kernel in either gemm mode)
        self._critic_backward(db, h1, h2, dq)
        self._actor_backward(db, saved, hs, dlogits)
