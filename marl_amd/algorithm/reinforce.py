"""ReinforceLearner: REINFORCE on the shared RNN agent read as a stochastic policy (the reference ships its argument table,
common/arguments.py:180-199, and no code; the definitions are this project's own - DESIGN section 9, include/marl_hip.h).

With m = 1 - padded, M = sum m, G the discounted Monte-Carlo return of the episode (csrc/td_lambda.hip at lambda = 1 on an all-zero
q_next: an episode cut at max_episode_len gets no bootstrap), H_r = - sum_{a_k = 1} pi_k log pi_k the entropy of the policy a row's
action was drawn from (eps mixing included; 0 log 0 = 0; 0 on a row without a policy) and beta = args.policy_entropy_coef >= 0:

    Adv = G  (no baseline)          L = [ - sum m G log pi(u) - beta sum m H ] / (N M)

One update pass: the eval unroll with saved planes, td_lambda_returns, policy_loss_bwd_ex with v = None, the fp32 BPTT on its dense
gradient.  One flat buffer, one optimizer of ``args.optimizer``'s kind at lr_actor with grad_norm_clip and the denominator N M.  No
critic, no target network (``target_update_cycle`` is not read), no hipGraph replay, no launch ahead of max_episode_len, one rank.
"""
from __future__ import annotations

import os

from .. import ops
from ..hostutil import require_cuda
from .common import LearnerParams, FlatView, FusedOptimizer, Learner, LossReadback, GradReducer, Scratch, policy_backward, policy_hs


def entropy_coef_of(args):
    """args.policy_entropy_coef: absent = 0; a negative weight is an error"""
    beta = float(getattr(args, "policy_entropy_coef", 0.0))
    if not beta >= 0.0:
        raise ValueError("policy_entropy_coef must be >= 0, got %r" % (beta,))
    return beta


class ReinforceLearner(Learner):
    launch_ahead = False
    replay_graphs = False
    mixer = target_mixer = None

    def __init__(self, mac, args):
        if GradReducer().enabled:
            raise NotImplementedError("ReinforceLearner trains on one rank")
        self.beta = entropy_coef_of(args)            # raises before anything is built
        if not getattr(mac, "stochastic", False):
            raise ValueError("ReinforceLearner needs a stochastic controller (PolicyMAC)")
        self.args = args
        self.max_episode_len = args.episode_limit
        self.gamma = args.gamma
        self.model_dir = args.model_dir + '/' + args.alg + '/' + args.map
        self.device = require_cuda("ReinforceLearner")
        self.epsilon = 0.0
        self.eval_net = mac
        self.eval_net.cuda()
        self.cuda()
        self.optimizer = FusedOptimizer(self._flat, args.optimizer, args.lr_actor, args.grad_norm_clip)
        self._buf = Scratch()
        self.reducer = GradReducer()
        self.loss_readback, self.entropy_readback = LossReadback(args), LossReadback(args)
        self.graphs = None
        self.needs_avail = True                      # the policy is over the current step's available actions
        self.last_stats = None
        self.entropy = float("nan")
        self._td_dbg, self._dbg = {}, {}

    def sync_replicas(self):
        """one rank: nothing to broadcast"""

    def cuda(self):
        dev = self.device
        self.eval_net.agent.to(dev)
        self.params = list(self.eval_net.parameters())
        self._flat = LearnerParams(self.params, dev)                              # stats = {L numerator, N M, sum m H}
        self.eval_net.agent._flat = FlatView(self._flat.flat, self.eval_net.agent.parameters(), 0)
        self.eval_net._dev = dev

    # ------------------------------------------------------------------ the hot path
    def _forward_backward(self, db):
        a, g = self.args, self._g
        B, T, N, A, H = db.B, db.T, db.N, db.A, a.rnn_hidden_dim
        BT, R = B * T, B * T * N
        logits, saved, h_last = g("logits", (B, T, N, A)), g("saved", ops.saved_shape(T, B, N)), g("h_last", (B * N, H))
        oc, oc_bs, oc_t0 = db.o_cur
        hs = policy_hs(self.eval_net, g, (B, T, N, H))
        self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, logits, hs, h_last, saved, h0=None,
                             ep_len=db.ep_len, ep_map=getattr(db, 'o_map', None))
        # the Monte-Carlo return: lambda = 1 leaves q_next only in the bootstrap of an unterminated episode, and q_next is 0
        G, q0 = g("td_ret", (BT,)), g("q_next0", (BT,))
        q0.zero_()
        ops.td_lambda_returns(q0, db.r, db.term, db.padded, self.gamma, 1.0, G, B, T)
        self._flat.zero_grad()
        dlogits, logp, ent = g("dlogits", (B, T, N, A)), g("logp", (R,)), g("ent", (R,))
        ops.policy_loss_bwd_ex(logits, db.avail, db.u_act.reshape(-1), G, None, db.padded, self.epsilon, self.beta, dlogits, logp,
                               ent, self._flat.stats[:3], R, N, A)
        policy_backward(self.eval_net, db, saved, hs, dlogits, self._buf)
        self._dbg = dict(logits=logits, td_targets=G, logp=logp, ent=ent, dlogits=dlogits)

    def train(self, batch, train_step, epsilon=0.0):
        """One update on the episodes just generated; ``epsilon``: the exploration rate their actions were drawn at.  Returns the
        loss; the mean entropy per live agent step is left in ``self.entropy`` (both through LossReadback)."""
        self.epsilon = float(epsilon)
        return Learner.train(self, batch, train_step)

    def _finish_update(self, train_step):
        st = self._flat.stats
        self.optimizer.step(den=st[1:2])
        self.last_stats = st
        self.entropy = self.entropy_readback.read(st[:3], lambda s: s[2] / s[1])
        return self.loss_readback.read(st[:3], self._loss_fn())

    def get_q_and_q_tot_table(self):
        raise NotImplementedError("REINFORCE has no Q table: it has no critic")

    # ------------------------------------------------------------------ checkpoints
    def save_models(self, train_step):
        num = str(train_step // self.args.save_cycle)
        os.makedirs(self.model_dir, exist_ok=True)
        self.eval_net.save_models(self.model_dir + '/' + num + '_rnn_net_params.pkl')

    def load_models(self):
        path_rnn = self.model_dir + '/rnn_net_params.pkl'
        if not os.path.exists(path_rnn):
            raise Exception("No model!")
        self.eval_net.load_models(path_rnn)
        print('Successfully load the model: {}'.format(path_rnn))

    def _target_flats(self):
        """ResumeMixin: the alg / parameter-count check, the parameters and the optimizer state; there is no target network"""
        return {}
