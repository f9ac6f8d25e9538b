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
"""
from __future__ import annotations

import copy
import os

import torch
import torch.nn as nn

from .. import ops
from ..hostutil import flatten_module, lin_of, require_cuda
from .reinforce import entropy_coef_of
from .common import (LearnerParams, FlatView, FusedOptimizer, Learner, LossReadback, GradReducer, Scratch, policy_backward, policy_hs,
                     td_lambda_of)


class VCritic(nn.Module):
    """V(s) (torch's default init); run through ops.linear / ops.linear_wgrad by the learner"""

    def __init__(self, args):
        super().__init__()
        self.fc1 = nn.Linear(args.state_shape, args.critic_dim)
        self.fc2 = nn.Linear(args.critic_dim, args.critic_dim)
        self.fc3 = nn.Linear(args.critic_dim, 1)

    def forward(self, s):
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(s)))))


class CentralVLearner(Learner):
    launch_ahead = False
    replay_graphs = False
    extra_nets = ("critic",)
    mixer = target_mixer = None

    def __init__(self, mac, args):
        if GradReducer().enabled:
            raise NotImplementedError("CentralVLearner trains on one rank: its two gradient buffers have no all-reduce")
        self.td_lambda = td_lambda_of(args)          # raises before anything is built
        self.beta = entropy_coef_of(args)            # (so does a negative weight)
        if not getattr(mac, "stochastic", False):
            raise ValueError("CentralVLearner needs a stochastic controller (PolicyMAC)")
        self.args = args
        self.max_episode_len = args.episode_limit
        self.gamma = args.gamma
        self.model_dir = args.model_dir + '/' + args.alg + '/' + args.map
        self.device = require_cuda("CentralVLearner")
        self.epsilon = 0.0
        self.eval_net = mac
        self.eval_net.cuda()
        self.critic = self._make_critic(args)
        self.target_critic = copy.deepcopy(self.critic)
        self.cuda()
        self.optimizer = FusedOptimizer(self._flat, args.optimizer, args.lr_actor, args.grad_norm_clip)
        self.critic_optimizer = FusedOptimizer(self._cflat, args.optimizer, args.lr_critic, args.grad_norm_clip)
        self._buf = Scratch()
        self.reducer = GradReducer()
        self.loss_readback, self.actor_readback, self.entropy_readback = LossReadback(args), LossReadback(args), LossReadback(args)
        self.graphs = None
        self.needs_avail = True                      # the policy is over the current step's available actions
        self.last_stats = self.actor_stats = None
        self.actor_loss = self.entropy = float("nan")
        self._td_dbg, self._dbg = {}, {}

    def _make_critic(self, args):
        return VCritic(args)

    def sync_replicas(self):
        """one rank: nothing to broadcast"""

    # ------------------------------------------------------------------ storage
    def cuda(self):
        dev = self.device
        self.eval_net.agent.to(dev)
        self.critic.to(dev)
        self.target_critic.to(dev)
        self.params = list(self.eval_net.parameters())
        self._flat = LearnerParams(self.params, dev)                              # the actor's buffer: stats = {L_actor numerator, N M}
        self.eval_net.agent._flat = FlatView(self._flat.flat, self.eval_net.agent.parameters(), 0)
        self.eval_net._dev = dev
        self._cflat = LearnerParams(list(self.critic.parameters()), dev)          # the critic's: stats = {L_critic numerator, M}
        self.critic._flat = FlatView(self._cflat.flat, self.critic.parameters(), 0)
        flatten_module(self.target_critic, dev)

    def _update_targets(self):
        self.target_critic._flat.flat.copy_(self._cflat.flat)

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
        a, g = self.args, self._g
        B, T, N, A, H = db.B, db.T, db.N, db.A, a.rnn_hidden_dim
        BT, R = B * T, B * T * N
        lam = self.td_lambda = td_lambda_of(a)
        lam = 0.0 if lam is None else lam
        # 1. the eval unroll keeps its activations for BPTT (the split kernel in gemm_mode "bf16x6", where QLearner's takes it)
        logits, saved, h_last = g("logits", (B, T, N, A)), g("saved", ops.saved_shape(T, B, N)), g("h_last", (B * N, H))
        oc, oc_bs, oc_t0 = db.o_cur
        hs = policy_hs(self.eval_net, g, (B, T, N, H))
        self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, logits, hs, h_last, saved, h0=None,
                             ep_len=db.ep_len, ep_map=getattr(db, 'o_map', None))
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
        # 7. - 8. the actor: Adv = G - V is formed inside the loss kernel; its dense gradient on the logits goes to BPTT (the fp32
        # kernel in either gemm mode: the split BPTT takes sparse gradients only)
        dlogits, logp = g("dlogits", (B, T, N, A)), g("logp", (R,))
        self._dbg = dict(logits=logits, v=v.view(BT), v_next=v_next.view(BT), td_targets=G, logp=logp, dlogits=dlogits)
        if self.beta == 0.0:
            ops.policy_loss_bwd(logits, db.avail, db.u_act.reshape(-1), G, v.view(BT), db.padded, self.epsilon, dlogits, logp,
                                self._flat.stats[:2], R, N, A)
        else:                                        # the entropy bonus, folded into the same pass: stats = {numerator, N M, sum m H}
            ent = self._dbg["ent"] = g("ent", (R,))
            ops.policy_loss_bwd_ex(logits, db.avail, db.u_act.reshape(-1), G, v.view(BT), db.padded, self.epsilon, self.beta,
                                   dlogits, logp, ent, self._flat.stats[:3], R, N, A)
        policy_backward(self.eval_net, db, saved, hs, dlogits, self._buf)

    def train(self, batch, train_step, epsilon=0.0):
        """One update on the episodes just generated; ``epsilon``: the exploration rate their actions were drawn at.  Returns the
        critic loss; the actor loss is left in ``self.actor_loss`` (both through LossReadback)."""
        self.epsilon = float(epsilon)
        return Learner.train(self, batch, train_step)

    def _finish_update(self, train_step):
        cs, st = self._cflat.stats, self._flat.stats
        self.critic_optimizer.step(den=cs[1:2])
        self.optimizer.step(den=st[1:2])
        if train_step > 0 and train_step % self.args.target_update_cycle == 0:
            self._update_targets()
        self.last_stats, self.actor_stats = cs, st
        self.actor_loss = self.actor_readback.read(st[:2], self._loss_fn())
        if self.beta != 0.0:
            self.entropy = self.entropy_readback.read(st[:3], lambda s: s[2] / s[1])
        return self.loss_readback.read(cs[:2], self._loss_fn())

    def get_q_and_q_tot_table(self):
        raise NotImplementedError("central-V has no Q table: its critic is a state value")

    # ------------------------------------------------------------------ checkpoints
    def save_models(self, train_step):
        num = str(train_step // self.args.save_cycle)
        os.makedirs(self.model_dir, exist_ok=True)
        self.eval_net.save_models(self.model_dir + '/' + num + '_rnn_net_params.pkl')
        torch.save({k: v.detach().cpu() for k, v in self.critic.state_dict().items()},
                   self.model_dir + '/' + num + '_critic_net_params.pkl')

    def load_models(self):
        path_rnn, path_critic = self.model_dir + '/rnn_net_params.pkl', self.model_dir + '/critic_net_params.pkl'
        if not os.path.exists(path_rnn):
            raise Exception("No model!")
        self.eval_net.load_models(path_rnn)
        self.critic.load_state_dict(torch.load(path_critic, map_location='cpu'))
        print('Successfully load the model: {} and {}'.format(path_rnn, path_critic))

    def resume_state(self):
        cpu = lambda t: t.detach().cpu().clone()
        return {"alg": self.args.alg, "n_params": int(self._flat.n), "n_critic": int(self._cflat.n),
                "params": cpu(self._flat.flat), "critic": cpu(self._cflat.flat),
                "target_critic": cpu(self.target_critic._flat.flat), "optimizer": self.optimizer.state_dict(),
                "critic_optimizer": self.critic_optimizer.state_dict()}

    def load_resume_state(self, sd):
        if sd["alg"] != self.args.alg or sd["n_params"] != int(self._flat.n) or sd.get("n_critic") != int(self._cflat.n):
            raise ValueError("resume state of a different learner (%s, %d parameters)" % (sd["alg"], sd["n_params"]))
        self._flat.flat.copy_(sd["params"])
        self._cflat.flat.copy_(sd["critic"])
        self.target_critic._flat.flat.copy_(sd["target_critic"])
        self.optimizer.load_state_dict(sd["optimizer"])
        self.critic_optimizer.load_state_dict(sd["critic_optimizer"])
