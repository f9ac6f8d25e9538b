"""MAVENLearner: MAVEN (Mahajan et al., NeurIPS 2019), ``--alg maven`` (the reference ships no MAVEN; the definition is this project's
own - DESIGN section 9, include/marl_hip.h).  QMIX on a noise-conditioned agent, plus a mutual-information term that makes the
episode's noise index recoverable from what the agents do.  Every episode of the batch carries its index k_b (MAVENMAC draws it,
the record and the replay ring carry it); with rows (b, t), m = 1 - padded:

    q'   = fc2(h) + (noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n]      (eval, continuation, and - target tables - target pass)
    td   = QLearner's TD error on q' through QMixMixer on the state (double-Q, quirks Q1 / Q2, args.td_lambda: the inherited stages)
    p_n  = softmax over the available actions of q'(b, t, n, :)               x = [p_0 | .. | p_{N-1} | s_{b,t}]
    ce   = logsumexp(W2 relu(W1 x + b1) + b2) - logits[k_b]
    L    = [ sum (m td)^2 + lambda_mi sum m ce ] / sum m

One update pass: zero the gradients, the three unrolls keeping hs, the three head forwards (csrc/maven.hip), the selections, the
mixer forwards on the unfolded path, the TD loss and the mixer backward, the MI pass (one row launch: forward, loss and backward down
to a dense gradient on q'; skipped whole with lambda_mi = 0), the head backward (dq_out for BPTT, dhs, the table gradients) and BPTT.
y, the greedy selections and k_b are constants of the backward; the MI gradients come un-normalised times lambda_mi - the optimizer
divides the whole gradient by sum m.  The discriminator's parameters sit in the flat buffer after the mixer's; it has no target copy
and is saved as <n>_maven_discrim_net_params.pkl.  One rank, eager launches (no hipGraph replay, no launch-ahead) in this version."""
from __future__ import annotations

import copy

import numpy as np
import torch

from .. import ops
from ..controller.share_params import MAVENMAC
from ..network.maven import MavenDiscriminator, lambda_mi_of
from ..network.mixer import QMixMixer
from .common import LearnerParams, FlatView, GradReducer, agent_backward
from .q_learner import QLearner


class MAVENLearner(QLearner):
    n_stats, den_slot = 4, 1          # { sum (m td)^2, sum m, sum m ce, sum m [argmax logits == k_b] }
    extra_nets = ("maven_discrim",)
    replay_graphs = False
    launch_ahead = False

    def __init__(self, mac, args):
        if not isinstance(mac, MAVENMAC):
            raise TypeError("MAVENLearner needs a MAVENMAC controller")
        if GradReducer().enabled:
            raise NotImplementedError("MAVENLearner trains on one rank: its schedule has not been run data-parallel")
        self.lambda_mi = lambda_mi_of(args)
        self._begin(mac, args, "MAVENLearner")
        self.mixer = QMixMixer(args)
        self.target_mixer = copy.deepcopy(self.mixer)
        self.maven_discrim = MavenDiscriminator(args)
        self.params = list(mac.parameters()) + list(self.mixer.parameters()) + list(self.maven_discrim.parameters())
        self.cuda()
        self._ready(needs_avail=False)       # the MI pass reads the current-step availability in place

    def cuda(self):
        """QLearner's buffers: [eval agent (with its tables) | mixer | discriminator]"""
        self.maven_discrim.to(self.device)
        super().cuda()
        self.maven_discrim._flat = FlatView(self._flat.flat, self.maven_discrim.parameters(),
                                            self.eval_net.agent._flat.n + self.mixer._flat.n)

    # ------------------------------------------------------------------ the hot path
    @staticmethod
    def _mi_sources(db):
        """(avail, floats per episode, state rows, row stride, rows per episode, episode map) the MI pass reads in place"""
        if db.avail_store is not None:                 # a device record or a replay sample: the (T+1)-slot storage, through the map
            s = db.s
            return db.avail_store[0], db.avail_store[1], s.t, s.t.stride(0), s.remap[1], s.emap
        return db.avail, db.T * db.N * db.A, db.s, db.s.stride(0), db.T, None

    def _forward_backward(self, db):
        if db.noise is None:
            raise ValueError("MAVENLearner needs the episodes' noise indices: the batch carries none (a record of another controller?)")
        a, g = self.args, self._g
        B, T, N, A, H, K = db.B, db.T, db.N, db.A, a.rnn_hidden_dim, self.eval_net.noise_dim
        lam = self.lambda_mi = lambda_mi_of(a)
        noise = db.noise
        self._flat.zero_grad()                # the MI pass adds into the statistics and the discriminator's gradients
        q_evals, q_en, q_tgt, saved, (hs, hs_en, hs_tgt) = self._unrolls(db, keep_hs=True)
        ag = self.eval_net.agent
        w_eval, w_tgt = ag.maven_weights(), self.target_net.agent.maven_weights()
        ops.maven_head_fwd(w_eval, hs, noise, q_evals, B, T, N, A, K)
        if a.double_q:
            ops.maven_head_fwd(w_eval, hs_en, noise, q_en, B, T, N, A, K)
        ops.maven_head_fwd(w_tgt, hs_tgt, noise, q_tgt, B, T, N, A, K)

        q_chosen, q_tgt_chosen, cur_max = self._select(db, q_evals, q_en, q_tgt)
        q_tot, q_tot_tgt, ctx, fold = self._mix(db, q_evals, q_tgt, q_chosen, q_tgt_chosen, cur_max)       # (maven: never folded)
        dq_val = self._loss_backward(db, q_chosen, q_tot, q_tot_tgt, ctx, fold).reshape(-1).contiguous()
        dq_dense = ce = None
        if lam > 0:
            dq_dense, ce = g("mi_dq", (B, T, N, A)), g("mi_ce", (B * T,))
            avail, avail_bs, state, state_ld, state_bs, emap = self._mi_sources(db)
            d = self.maven_discrim
            ops.maven_mi(d.weights(), d.grads(), q_evals, avail, avail_bs, state, state_ld, state_bs, emap, noise, db.padded, lam,
                         dq_dense, ce, self._flat.stats[2:4], B, T, N, A, db.S, K)
        dq_out, dhs = g("dq_out", (B, T, N, A)), g("dhs", (B, T, N, H))
        ops.maven_head_bwd(w_eval, ag.maven_grads(), hs, noise, db.u_act.reshape(-1), dq_val, dq_dense, dq_out, dhs, B, T, N, A, K)
        agent_backward(self.eval_net, db, "cur", saved, hs, dq_out, dhs, self._buf)
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, q_tot_target=q_tot_tgt, hs=hs, ce=ce, dq_dense=dq_dense,
                         **self._td_dbg)

    def _loss_fn(self):
        lam = self.lambda_mi
        return lambda s: s[0] / s[1] + lam * s[2] / s[1]

    def get_q_and_q_tot_table(self, noise=0):
        """QLearner's matrix-game diagnostic for ONE noise index (the agents' Q rows and so the table depend on it): 3x3 q_tot table +
        per-agent Q rows with obs = state = 1 and zero last action (quirk Q9).  ``noise`` outside [0, noise_dim) is a ValueError."""
        K = self.eval_net.noise_dim
        if isinstance(noise, bool) or not isinstance(noise, (int, np.integer)) or not 0 <= noise < K:
            raise ValueError("noise must be an index in [0, %d), got %r" % (K, noise))
        one = {'o': np.ones((1, 1, 2, 1)), 's': np.ones((1, 1, 1)), 'o_next': np.ones((1, 1, 2, 1)),
               'u_onehot': np.zeros((1, 1, 2, 3)), 'avail_u': np.ones((1, 1, 2, 3)), 'noise': np.array([int(noise)], dtype=np.int32)}
        self.eval_net.init_hidden(1)
        qv = self.eval_net.get_current_q_values(one, 1)[0].cpu()      # (1,1,2,3)
        q_tot_table = np.zeros((3, 3))
        s = torch.ones(1, 1, 1)
        for i in range(3):
            for j in range(3):
                chosen = torch.stack((qv[:, :, 0, i], qv[:, :, 1, j]), dim=1).view(1, 1, 2)
                q_tot_table[i, j] = self.mixer(chosen, s).item()
        return q_tot_table, qv[0, 0, 0].numpy(), qv[0, 0, 1].numpy()
