"""PolicyLearner: the frame of the policy-gradient learners (ReinforceLearner, CentralVLearner, COMALearner - DESIGN section 9).

What they share: the shared RNN agent read as a stochastic policy (PolicyMAC or a subclass of it) in one flat buffer with one
optimizer of ``args.optimizer``'s kind at lr_actor, the eval unroll with saved planes at the head of an update pass and the actor's
backward on the dense gradient of the logits at its end, the entropy weight beta = ``args.policy_entropy_coef``, eager launches (no
hipGraph replay, no launch ahead of max_episode_len), one rank, no target actor.  A learner with a critic defines ``_make_critic``:
the frame then keeps the critic and its target copy in flat buffers of their own, a second optimizer at lr_critic, the target sync
every ``target_update_cycle`` updates, the critic's model file and its part of the resume state.  A learner whose critic
bootstraps from itself sets ``has_target_critic = False`` (PPOLearner): no target copy is built, synced or carried in the resume
state.  A learner provides ``_forward_backward(db)`` between ``_actor_unroll`` and ``_actor_backward``.
"""
from __future__ import annotations

import copy

from .. import ops
from ..hostutil import Scratch, flatten_module, require_cuda
from .common import LearnerParams, FlatView, FusedOptimizer, Learner, LossReadback, GradReducer, policy_backward, policy_hs, td_lambda_of


def entropy_coef_of(args):
    """args.policy_entropy_coef: absent = 0; a negative weight is an error"""
    beta = float(getattr(args, "policy_entropy_coef", 0.0))
    if not beta >= 0.0:
        raise ValueError("policy_entropy_coef must be >= 0, got %r" % (beta,))
    return beta


class PolicyLearner(Learner):
    launch_ahead = False
    replay_graphs = False
    mixer = target_mixer = None
    critic = target_critic = None
    _make_critic = None           # a learner with a critic: _make_critic(args) -> the nn.Module (and "critic" in extra_nets)
    has_target_critic = True      # False (PPOLearner): the critic has no target copy
    _no_q_table = None            # the sentence get_q_and_q_tot_table refuses with

    def __init__(self, mac, args):
        name = type(self).__name__
        if GradReducer().enabled:
            raise NotImplementedError("%s trains on one rank: its gradient buffers have no all-reduce" % name)
        if self._make_critic is not None:
            self.td_lambda = td_lambda_of(args)      # raises before anything is built (a learner without a critic does not read it)
        self.beta = entropy_coef_of(args)            # (so does a negative weight)
        if not getattr(mac, "stochastic", False):
            raise ValueError("%s needs a stochastic controller (PolicyMAC)" % name)
        self.args = args
        self.max_episode_len = args.episode_limit
        self.gamma = args.gamma
        self.model_dir = args.model_dir + '/' + args.alg + '/' + args.map
        self.device = require_cuda(name)
        self.epsilon = 0.0
        self.eval_net = mac
        self.eval_net.cuda()
        if self._make_critic is not None:
            self.critic = self._make_critic(args)
            if self.has_target_critic:
                self.target_critic = copy.deepcopy(self.critic)
        self.cuda()
        self.optimizer = FusedOptimizer(self._flat, args.optimizer, args.lr_actor, args.grad_norm_clip)
        if self.critic is not None:
            self.critic_optimizer = FusedOptimizer(self._cflat, args.optimizer, args.lr_critic, args.grad_norm_clip)
        self._buf = Scratch()
        self.reducer = GradReducer()
        self.loss_readback, self.actor_readback, self.entropy_readback = LossReadback(args), LossReadback(args), LossReadback(args)
        self.graphs = None
        self.needs_avail = True                      # the policy is over the current step's available actions
        self.last_stats = self.actor_stats = None
        self.actor_loss = self.entropy = float("nan")
        self._td_dbg, self._dbg = {}, {}

    def sync_replicas(self):
        """one rank: nothing to broadcast"""

    # ------------------------------------------------------------------ storage
    def cuda(self):
        dev = self.device
        self.eval_net.agent.to(dev)
        if self.critic is not None:
            self.critic.to(dev)
            if self.target_critic is not None:
                self.target_critic.to(dev)
        self.params = list(self.eval_net.parameters())
        self._flat = LearnerParams(self.params, dev)                              # the actor's buffer: stats = {numerator, N M, sum m H}
        self.eval_net.agent._flat = FlatView(self._flat.flat, self.eval_net.agent.parameters(), 0)
        self.eval_net._dev = dev
        if self.critic is not None:
            self._cflat = LearnerParams(list(self.critic.parameters()), dev)      # the critic's: stats = {numerator, denominator}
            self.critic._flat = FlatView(self._cflat.flat, self.critic.parameters(), 0)
            if self.target_critic is not None:
                flatten_module(self.target_critic, dev)

    def _update_targets(self):
        self.target_critic._flat.flat.copy_(self._cflat.flat)

    # ------------------------------------------------------------------ the hot path
    def _lambda(self):
        """args.td_lambda as the returns kernel takes it: None means 0, the one-step target"""
        lam = self.td_lambda = td_lambda_of(self.args)
        return 0.0 if lam is None else lam

    def _actor_unroll(self, db):
        """the eval unroll on the batch's current observations, keeping its activations for the backward (the split kernel in
        gemm_mode "bf16x6", where QLearner's takes it): (logits (B, T, N, A), saved, what ``_actor_backward`` takes as hs)"""
        g = self._g
        B, T, N, A, H = db.B, db.T, db.N, db.A, self.args.rnn_hidden_dim
        logits, saved, h_last = g("logits", (B, T, N, A)), g("saved", ops.saved_shape(T, B, N)), g("h_last", (B * N, H))
        oc, oc_bs, oc_t0 = db.o_cur
        hs = policy_hs(self.eval_net, g, (B, T, N, H))
        self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, logits, hs, h_last, saved, h0=None,
                             ep_len=db.ep_len, ep_map=getattr(db, 'o_map', None))
        return logits, saved, hs

    def _actor_backward(self, db, saved, hs, dlogits):
        """the actor's backward on the dense gradient of the logits (BPTT: the fp32 kernel in either gemm mode, the split BPTT takes
        sparse gradients only)"""
        policy_backward(self.eval_net, db, saved, hs, dlogits, self._buf)

    def train(self, batch, train_step, epsilon=0.0):
        """One update on the episodes just generated; ``epsilon``: the exploration rate their actions were drawn at.  Returns the
        critic loss and leaves the actor loss in ``self.actor_loss``; without a critic, returns the actor loss.  The mean entropy
        per live agent step is left in ``self.entropy`` where it was computed (all through LossReadback)."""
        self.epsilon = float(epsilon)
        if hasattr(self.eval_net, "set_train_step"):     # a controller that draws noise of its own in the update keys it by the step
            self.eval_net.set_train_step(train_step)
        return Learner.train(self, batch, train_step)

    def _finish_update(self, train_step):
        st, cs = self._flat.stats, None
        if self.critic is not None:
            cs = self._cflat.stats
            self.critic_optimizer.step(den=cs[1:2])
        self.optimizer.step(den=st[1:2])
        if self.target_critic is not None and train_step > 0 and train_step % self.args.target_update_cycle == 0:
            self._update_targets()
        self.last_stats, self.actor_stats = (st if cs is None else cs), st
        if cs is not None:
            self.actor_loss = self.actor_readback.read(st[:2], self._loss_fn())
        if cs is None or self.beta != 0.0:           # (with a critic and beta = 0 the actor pass may be one that computes no entropy)
            self.entropy = self.entropy_readback.read(st[:3], lambda s: s[2] / s[1])
        return self.loss_readback.read(st[:3] if cs is None else cs[:2], self._loss_fn())

    def get_q_and_q_tot_table(self):
        raise NotImplementedError(self._no_q_table)

    # ------------------------------------------------------------------ resume state (checkpoints: Learner's, no mixer file)
    def _target_flats(self):
        """ResumeMixin: there is no target actor"""
        return {} if self.target_critic is None else {"target_critic": self.target_critic._flat.flat}

    def resume_state(self):
        sd = super().resume_state()
        if self.critic is not None:
            sd.update(n_critic=int(self._cflat.n), critic=self._cflat.flat.detach().cpu().clone(),
                      critic_optimizer=self.critic_optimizer.state_dict())
        return sd

    def load_resume_state(self, sd):
        if self.critic is not None and sd.get("n_critic") != int(self._cflat.n):      # (before any tensor is copied, as super()'s check)
            raise ValueError("resume state of a different learner (%s, %d parameters)" % (sd["alg"], sd["n_params"]))
        super().load_resume_state(sd)
        if self.critic is not None:
            self._cflat.flat.copy_(sd["critic"])
            self.critic_optimizer.load_state_dict(sd["critic_optimizer"])
