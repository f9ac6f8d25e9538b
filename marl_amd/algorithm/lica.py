"""LICALearner: learning implicit credit assignment (Zhou et al., NeurIPS 2020; the reference ships nothing for it - the definitions
are this project's own, DESIGN section 9, include/marl_hip.h).

The actor is the shared RNN agent read as a stochastic policy (PolicyMAC, csrc/policy.hip).  The critic is a hypernetwork mixer of
the state whose input is the agents' action distributions; the actor is trained by differentiating Q(s, pi_1, .., pi_N) straight
through the critic into the logits - a dense gradient per agent step out of the critic's backward, not Adv * dlogp.

Sizes: K = N A, E = ``args.mixing_embed_dim`` (32), HE = ``args.hypernet_embed`` (64), S = state_shape.  A critic row is one step
(b, t), rows = B T; an agent row is r = (b T + t) N + i.  ``LICACritic`` holds four hypernetworks under the published names:

    hyper_w_1     = Linear(S, HE) - ReLU - Linear(HE, K E)          hyper_b_1 = Linear(S, E)
    hyper_w_final = Linear(S, HE) - ReLU - Linear(HE, E)            hyper_b_2 = Linear(S, E) - ReLU - Linear(E, 1)

Per row, with x in R^K (agent-major, x[i A + k]) and W1[k, e] column k E + e of hyper_w_1's output:

    pre_e = b1_e + sum_k x_k W1[k, e],    h_e = relu(pre_e),    Q = sum_e h_e wf_e + b2        (no abs(): LICA's critic is not monotonic)

pi is ops.policy_probs' policy: softmax over all A, availability, the epsilon mixing of the rate the batch was drawn at,
renormalised; a row with n = 0 has no policy and an all-zero pi.  With m = 1 - padded, M = sum m, u the taken actions, onehot(u) the
K-vector with one 1 per agent block and Q' the target critic run on the same T steps:

    q_next[b, t] = Q'(s[b, t+1], onehot(u[b, t+1]))  (t + 1 < T),    q_next[b, T-1] = 0          (COMA's window quirk, kept)
    G            = the lambda-returns of q_next (csrc/td_lambda.hip on B sequences; a constant of the gradient)
    L_critic     = sum m (G - Q(s, onehot(u)))^2 / M
    L_actor      = - sum_bt m Q(s, pi) / M  -  beta sum_r m H_r / (N M)

beta = ``args.policy_entropy_coef`` >= 0, H_r the entropy of algorithm/reinforce.py.  In L_actor the critic's weights are constants;
both gradients are taken at the weights the update started from, from one pass, as CentralV / COMA.  The actor's statistics are
{ -N sum_bt m Q_pi - beta sum_r m H,  N M,  sum_r m H }, the critic's { sum (m td)^2, M }: PolicyLearner's tail takes them as they are.

One update pass: the eval unroll with saved planes (the split kernel in gemm_mode "bf16x6"; the critic is fp32 in both modes); the
four hypernetworks of the eval critic on the states into one (B T, K E + 2 E + 1) buffer - one forward, shared by the critic pass and
the actor pass - and the target critic's into a second; lica_mix_fwd on the target's with u, the shift to q_next (a slice copy:
plumbing), td_lambda_returns; lica_loss_bwd (the ``_td_inputs`` idiom: G as r, gamma = 0) and the hypernetworks' backward; then
policy_probs, lica_mix_fwd on pi, lica_mix_bwd for dQ/dpi alone with dq = -N m, policy_probs_bwd and BPTT on its dense gradient.
Scratch: hy, the target's and dhy are each B T (K E + 2 E + 1) floats (3.5 GB each at 2s3z x 4096 episodes x 120 steps, 11.4 GB at
MMM2); there is no chunking.  Out of scope: the published adaptive entropy coefficient (beta / mean H needs a pass before the
gradient), more than one rank, a fused single-launch actor pass, never materialising W1.  Storage, the two optimizers, the target
sync, checkpoints and resume state are PolicyLearner's (algorithm/policy_learner.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..hostutil import lin_of
from .policy_learner import PolicyLearner

LICA_MAX = dict(n_agents=16, n_actions=32, mixing_embed_dim=64)       # the support range of csrc/lica.hip (marl_lica_supported)


def lica_shape_of(args):
    """(N, A, E, HE, S) of the LICA critic from args, or ValueError: the row kernels cover N <= 16, A <= 32, E <= 64 and nothing
    else runs them.  The launcher calls this before anything is built, the critic at construction."""
    S = int(np.prod(args.state_shape))
    N, A, E, HE = args.n_agents, args.n_actions, args.mixing_embed_dim, args.hypernet_embed
    for name, v in (("n_agents", N), ("n_actions", A), ("mixing_embed_dim", E)):
        if not 1 <= v <= LICA_MAX[name]:
            raise ValueError("lica: %s = %d is outside the row kernels' range 1..%d" % (name, v, LICA_MAX[name]))
    if HE < 1 or S < 1:
        raise ValueError("lica: hypernet_embed = %d and state_shape = %d must be at least 1" % (HE, S))
    return N, A, E, HE, S


class LICACritic(nn.Module):
    """the LICA mixing critic as plain nn.Linears under the published names (torch's default init): a checkpoint has the published
    layout.  ``forward(x, s)`` is the plain torch form, x (..., K) and s (..., S) -> Q (..., 1); the learner runs the hypernetworks
    through ops.linear and the mix through csrc/lica.hip"""

    def __init__(self, args):
        super().__init__()
        N, A, E, HE, S = lica_shape_of(args)
        self.n_agents, self.n_actions, self.embed_dim, self.state_dim = N, A, E, S
        self.hyper_w_1 = nn.Sequential(nn.Linear(S, HE), nn.ReLU(), nn.Linear(HE, N * A * E))
        self.hyper_w_final = nn.Sequential(nn.Linear(S, HE), nn.ReLU(), nn.Linear(HE, E))
        self.hyper_b_1 = nn.Linear(S, E)
        self.hyper_b_2 = nn.Sequential(nn.Linear(S, E), nn.ReLU(), nn.Linear(E, 1))

    def forward(self, x, s):
        K, E = self.n_agents * self.n_actions, self.embed_dim
        lead = x.shape[:-1]
        x, s = x.reshape(-1, 1, K), s.reshape(-1, self.state_dim)
        w1 = self.hyper_w_1(s).view(-1, K, E)
        h = torch.relu(torch.bmm(x, w1) + self.hyper_b_1(s).view(-1, 1, E))
        q = torch.bmm(h, self.hyper_w_final(s).view(-1, E, 1)) + self.hyper_b_2(s).view(-1, 1, 1)
        return q.view(*lead, 1)


class LICALearner(PolicyLearner):
    extra_nets = ("critic",)
    has_target_critic = True
    _no_q_table = "LICA has no Q table: its critic mixes the agents' action distributions into one value"

    def _make_critic(self, args):
        return LICACritic(args)

    # ------------------------------------------------------------------ the hot path
    def _dims(self, db):
        E = self.args.mixing_embed_dim
        return db.N * db.A, E, db.N * db.A * E, self.args.hypernet_embed

    def _hyper_forward(self, net, db, tag, keep):
        """hy (B T, K E + 2 E + 1) = [W1 | b1 | wf | b2] of the states; keep: the three ReLU hiddens as well (the backward's gates)"""
        K, E, KE, HE = self._dims(db)
        BT, g = db.B * db.T, self._g
        hy = self._buf.get_rows("l_hy" + tag, BT, KE + 2 * E + 1, self.device)
        h1, hf, h2 = g("l_h1" + tag, (BT, HE)), g("l_hf" + tag, (BT, HE)), g("l_h2" + tag, (BT, E))
        xs = ops.src(db.s)
        for seq, hid, out in ((net.hyper_w_1, h1, hy[:, :KE]), (net.hyper_w_final, hf, hy[:, KE + E:KE + 2 * E]),
                              (net.hyper_b_2, h2, hy[:, KE + 2 * E:])):
            lin_of(seq[0]).fwd(xs, hid, BT, act=1)
            lin_of(seq[2]).fwd(ops.src(hid), out, BT)
        lin_of(net.hyper_b_1).fwd(xs, hy[:, KE:KE + E], BT)
        return (hy, h1, hf, h2) if keep else hy

    def _hyper_backward(self, db, h1, hf, h2, dhy, db2):
        """autograd of _hyper_forward for dhy (B T, >= K E + 2 E) = [dW1 | db1 | dwf] and db2 (B T): accumulates into the critic's
        .grad views"""
        K, E, KE, HE = self._dims(db)
        BT, g, c = db.B * db.T, self._g, self.critic
        xs = ops.src(db.s)
        for seq, hid, dout in ((c.hyper_w_1, h1, dhy[:, :KE]), (c.hyper_w_final, hf, dhy[:, KE + E:KE + 2 * E]),
                               (c.hyper_b_2, h2, db2.view(BT, 1))):
            l0, l2 = lin_of(seq[0]), lin_of(seq[2])
            dh = g("l_dh%d" % hid.shape[1], (BT, hid.shape[1]))
            l2.wgrad(dout, ops.src(hid), BT)
            l2.bwd_x(dout, dh, BT)
            l0.wgrad(dh, xs, BT, Yact=hid)
        lin_of(c.hyper_b_1).wgrad(dhy[:, KE:KE + E], xs, BT)

    def _forward_backward(self, db):
        g = self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        BT, R = B * T, B * T * N
        K, E, KE, HE = self._dims(db)
        lam = self._lambda()
        # 1. the eval unroll keeps its activations for BPTT
        logits, saved, hs = self._actor_unroll(db)
        # 2. the hypernetworks of both critics on the states: one forward of the eval critic's serves both passes below
        u = db.u_act.reshape(-1)
        hy, h1, hf, h2 = self._hyper_forward(self.critic, db, "", True)
        hy_t = self._hyper_forward(self.target_critic, db, "t", False)
        # 3. the target critic on the taken actions, shifted by one step (the window's last step has no successor), its lambda-returns
        q_tgt, q_next, G = g("q_tgt", (B, T)), g("q_next", (B, T)), g("td_ret", (B, T))
        ops.lica_mix_fwd(hy_t, None, u, q_tgt, BT, N, A, E)
        q_next[:, :T - 1].copy_(q_tgt[:, 1:])
        q_next[:, T - 1].zero_()
        ops.td_lambda_returns(q_next, db.r, db.term, db.padded, self.gamma, lam, G, B, T)
        # 4. the critic: forward on the taken actions, loss (target G + 0 q_next (1 - term) = G) and backward in one row launch
        self._flat.zero_grad()
        self._cflat.zero_grad()
        q, dq_tot = g("q", (BT,)), g("dq_tot", (BT,))
        dhy = self._buf.get_rows("l_dhy", BT, KE + 2 * E, self.device)
        ops.lica_loss_bwd(hy, u, q_next.view(BT), G.view(BT), db.term, db.padded, 0.0, q, dhy, dq_tot, self._cflat.stats[:2],
                          BT, N, A, E)
        self._hyper_backward(db, h1, hf, h2, dhy, dq_tot)
        # 5. the actor: Q(s, pi) and its gradient by pi out of the same hy, then through the policy into the logits
        pi, q_pi, dq_pi, dpi = g("pi", (B, T, N, A)), g("q_pi", (BT,)), g("dq_pi", (BT,)), g("dpi", (BT, K))
        dlogits, ent = g("dlogits", (B, T, N, A)), g("ent", (R,))
        ops.policy_probs(logits, db.avail, self.epsilon, pi, R, A)
        x = pi.view(BT, K)                           # the agent rows of one step are contiguous
        ops.lica_mix_fwd(hy, x, None, q_pi, BT, N, A, E)
        torch.mul(db.padded.reshape(BT) - 1.0, float(N), out=dq_pi)      # dq = - N m
        ops.lica_mix_bwd(hy, x, None, dq_pi, None, dpi, BT, N, A, E)
        ops.policy_probs_bwd(logits, db.avail, dpi, q_pi, db.padded, self.epsilon, self.beta, dlogits, ent, self._flat.stats[:3],
                             R, N, A)
        self._dbg = dict(logits=logits, q=q, q_tgt=q_tgt, q_next=q_next, td_targets=G, pi=pi, q_pi=q_pi, dpi=dpi, dlogits=dlogits,
                         ent=ent)
        self._actor_backward(db, saved, hs, dlogits)
