"""QLearner for VDN / QMIX / QPLEX and Qatten (mirror of reference algorithm/q_learner.py:10-262).

``train(batch, train_step)`` keeps the reference contract (returns the float loss, syncs targets
every ``target_update_cycle``), but is an explicit forward/backward schedule of HIP kernels:
three agent unrolls, mixer forward (+target), TD loss, mixer backward, BPTT, fused clip+optimizer.
Reference quirks Q1 (double-Q pass continues from the eval net's final hidden state), Q2
(get_max_episode_len ignores unterminated episodes), Q4/Q5 (mask constant, first-index argmax) and
Q6 (target sync rule) are reproduced.  With ``args.td_lambda`` set the TD target is the lambda-return of q_tot_target
(Learner._td_inputs; quirk Q15) instead of the one-step bootstrap; unset, not one call differs.
``args.alg == 'qatten'`` (this project's own; the reference ships no Qatten) mixes with QattenMixer on the same schedule, its
eval forward, the TD loss and the attention backward folded into one launch as QMIX's are (``args.no_loss_fold`` unfolds both).
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from .. import ops, experiments
from ..hostutil import flatten_module
from ..network.mixer import VDNMixer, QMixMixer, DMAQer, QattenMixer
from .common import MASK_BIG, LearnerParams, FlatView, Learner, agent_backward


class QLearner(Learner):
    def __init__(self, mac, args):
        self._begin(mac, args, "QLearner")
        if args.alg == 'vdn':
            self.mixer = VDNMixer(args)
        elif args.alg == 'qmix':
            self.mixer = QMixMixer(args)
        elif args.alg == 'qplex':
            self.mixer = DMAQer(args)
        elif args.alg == 'qatten':
            self.mixer = QattenMixer(args)
        else:
            raise ValueError("Mixer {} not recognised.".format(args.alg))
        self.target_mixer = copy.deepcopy(self.mixer)
        self.params = list(mac.parameters()) + list(self.mixer.parameters())
        self.cuda()
        self._ready(needs_avail=args.alg == 'qplex')     # the current-step availability masks the greedy action (:135-140)

    def sync_replicas(self):
        """Data-parallel replicas start from rank 0's parameters, targets and optimizer state (called after
        construction and after load_models; a no-op without a process group)."""
        o = self.optimizer
        self.reducer.broadcast_(self._flat.flat, self.target_net.agent._flat.flat,
                                self.target_mixer._flat.flat if self.target_mixer._flat.n else None, o.s1, o.s2)

    # ------------------------------------------------------------------ storage
    def cuda(self):
        """Move everything to the MI355X and (re)build the flat buffers."""
        dev = self.device
        self.mixer.to(dev)
        self.target_mixer.to(dev)
        self.eval_net.agent.to(dev)
        self._flat = LearnerParams(self.params, dev)
        self.eval_net.agent._flat = FlatView(self._flat.flat, self.eval_net.agent.parameters(), 0)
        self.mixer._flat = FlatView(self._flat.flat, self.mixer.parameters(), self.eval_net.agent._flat.n)
        self.eval_net._dev = dev
        self.target_net._dev = dev
        self.target_net.agent.to(dev)
        flatten_module(self.target_net.agent, dev)
        flatten_module(self.target_mixer, dev)

    # ------------------------------------------------------------------ the hot path: the stages of one update pass
    def _unrolls(self, db, keep_hs=False):
        """The three agent unrolls: eval current-Q (keeps activations), its double-Q continuation, target next-Q.
        keep_hs: each also writes its per-step hidden states (B,T,N,H).  Without it none does: the Q-learning losses do
        not read them and BPTT finds h(t) in `saved`.  Returns q_evals, q_en, q_tgt, saved, (hs, hs_en, hs_tgt)."""
        a, g = self.args, self._g
        B, T, N, A, H = db.B, db.T, db.N, db.A, a.rnn_hidden_dim
        q_evals, saved = g("q_evals", (B, T, N, A)), g("saved", ops.saved_shape(T, B, N))
        h_last, h_scr = g("h_last", (B * N, H)), g("h_scr", (B * N, H))
        q_tgt, q_en = g("q_tgt", (B, T, N, A)), g("q_en", (B, T, N, A))
        hs = hs_en = hs_tgt = None
        if keep_hs:
            hs, hs_tgt = g("hs", (B, T, N, H)), g("hs_tgt", (B, T, N, H))
            hs_en = g("hs_en", (B, T, N, H)) if a.double_q else None
        (oc, oc_bs, oc_t0), (on, on_bs, on_t0) = db.o_cur, db.o_next

        # the eval and the target unroll are independent of each other: on small shards they run side by side on two
        # streams, a share of the CUs each
        emap = getattr(db, 'o_map', None)
        # quirk Q1: no init_hidden between the two eval passes (reference :96-110) - the double-Q pass continues the eval chain.
        # Its inputs at steps 0..T-2 are the eval pass's inputs at steps 1..T-1 (same observations, same last actions, same
        # weights): fc1 and the input-side gate sums stored there are reused (gi), where the kernels of this shape can.
        # Every unroll kernel stores hs when given it, the gi_in continuation included; the bf16x6 entry then runs hs-writing
        # launches on csrc/agent_x6.hip (never the non-saving agent_x6p.hip path), so the gate sums pair up either way
        cont, gi = None, None
        if a.double_q:
            shifted = on is oc and on_bs == oc_bs and on_t0 == oc_t0 + 1
            split = self.pair.chain_split(B * N, T, a.obs_shape)
            # (the continuation keeps reading the eval pass's input-side gate sums at every batch size: 0.55 ms at 4096 envs against
            # 0.97 ms for a plain unroll in the round-6 decomposition, csrc/agent_x6p.hip - which the TARGET unroll below runs on)
            if shifted and ((self.eval_net.unroll_x6(B, T, oc) and experiments.get("fwd_xs") != 0) or
                            ops.agent_unroll_reuse_supported(B, T, N, a.obs_shape, A, split[0] if split else 256)):
                gi = g("gi", ops.saved_shape(T, B, N, planes=3))
            cont = lambda cu: self.eval_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, q_en, hs_en, h_scr, None, h0=h_last,
                                                   ep_len=db.ep_len, ep_map=emap, cu_budget=cu, gi_in=gi)
        self.pair.run_chain(B * N, T, a.obs_shape,
                            lambda cu: self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, q_evals, hs, h_last, saved,
                                                            h0=None, ep_len=db.ep_len, ep_map=emap, cu_budget=cu, gi_out=gi),
                            cont,
                            lambda cu: self.target_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, q_tgt, hs_tgt, None, None,
                                                              h0=None, ep_len=db.ep_len, ep_map=emap, cu_budget=cu))
        return q_evals, q_en, q_tgt, saved, (hs, hs_en, hs_tgt)

    def _select(self, db, q_evals, q_en, q_tgt):
        """Q of the taken actions and the target Q of the greedy next actions (double-Q: greedy by the continuation's Qs).
        Returns q_chosen, q_tgt_chosen (R,) and cur_max, the double-Q greedy actions (else None)."""
        R, A, g = db.B * db.T * db.N, db.A, self._g
        q_chosen, q_tgt_chosen = g("q_chosen", (R,)), g("q_tgt_chosen", (R,))
        ops.q_gather(q_evals, db.u_act.reshape(-1), q_chosen, R, A)
        cur_max = None
        if self.args.double_q:
            cur_max = g("cur_max", (R,), torch.int32)
            ops.q_double_select(q_en, q_tgt, db.avail_next, MASK_BIG, q_tgt_chosen, cur_max, R, A)
        else:
            ops.q_masked_max(q_tgt, db.avail_next, MASK_BIG, q_tgt_chosen, None, R, A)
        return q_chosen, q_tgt_chosen, cur_max

    def _mix(self, db, q_evals, q_tgt, q_chosen, q_tgt_chosen, cur_max):
        """Eval and target mixer forwards.  Returns q_tot, q_tot_tgt, the eval mixer's ctx and `fold`: QMIX's and Qatten's eval forward
        is left to the loss stage, where it is one launch with the TD loss and the mixer backward."""
        a, g = self.args, self._g
        N, BT, A = db.N, db.B * db.T, db.A
        R = BT * N
        ctx, fold = {}, False
        qc, qtc = q_chosen.view(BT, N), q_tgt_chosen.view(BT, N)
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
            fold = a.alg in ('qmix', 'qatten') and getattr(self.mixer, "loss_backward_fused", None) is not None and \
                self.mixer.loss_backward_fused(db.s) and not getattr(a, "no_loss_fold", False)
            q_tot = g("q_tot", (BT,)) if fold else self.mixer.hip_forward(qc, db.s, BT, ctx=ctx)
            q_tot_tgt = self.target_mixer.hip_forward(qtc, db.s_next, BT, tag="t")
        return q_tot, q_tot_tgt, ctx, fold

    def _loss_backward(self, db, q_chosen, q_tot, q_tot_tgt, ctx, fold):
        """TD loss (un-normalised numerator + sum(mask) land in the tail of the gradient buffer, zeroed before) and the
        mixer backward.  Returns dq_chosen, the gradient on the taken actions' Qs."""
        BT = db.B * db.T
        r, gamma = self._td_inputs(db, q_tot_tgt)        # args.td_lambda set: the lambda-returns as r, and gamma = 0
        if fold:
            # fused QMIX / Qatten: eval-mixer forward, TD loss and mixer backward are ONE launch (the backward recomputes q_tot anyway)
            return self.mixer.hip_loss_backward(q_chosen.view(BT, db.N), db.s, BT, q_tot_tgt, r, db.term, db.padded, gamma,
                                                self._flat.stats[:2], q_tot=q_tot)
        dq_tot = self._g("dq_tot", (BT,))
        ops.td_loss(q_tot, q_tot_tgt, r, db.term, db.padded, gamma, dq_tot, self._flat.stats[:2], BT)
        return self.mixer.hip_backward(ctx, dq_tot, BT)

    def _forward_backward(self, db):
        q_evals, q_en, q_tgt, saved, _ = self._unrolls(db)
        q_chosen, q_tgt_chosen, cur_max = self._select(db, q_evals, q_en, q_tgt)
        q_tot, q_tot_tgt, ctx, fold = self._mix(db, q_evals, q_tgt, q_chosen, q_tgt_chosen, cur_max)
        self._flat.zero_grad()
        dq_chosen = self._loss_backward(db, q_chosen, q_tot, q_tot_tgt, ctx, fold)
        # the loss reaches q_evals only through the gather above: hand BPTT the sparse (action, gradient) pairs
        # instead of scattering them into a dense (B,T,N,A) tensor
        agent_backward(self.eval_net, db, "cur", saved, None, None, None, self._buf,
                       dq_idx=db.u_act.reshape(-1), dq_val=dq_chosen.reshape(-1).contiguous())
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, q_tot_target=q_tot_tgt, **self._td_dbg)

    def get_q_and_q_tot_table(self):
        """Matrix-game diagnostic (reference :211-262): 3x3 q_tot table + per-agent Q rows with
        obs = state = 1 and zero last action (quirk Q9)."""
        one = {'o': np.ones((1, 1, 2, 1)), 's': np.ones((1, 1, 1)), 'o_next': np.ones((1, 1, 2, 1)),
               'u_onehot': np.zeros((1, 1, 2, 3)), 'avail_u': np.ones((1, 1, 2, 3))}
        self.eval_net.init_hidden(1)
        q_values, _ = self.eval_net.get_current_q_values(one, 1)     # (1,1,2,3)
        qv = q_values.cpu()
        q_table_i, q_table_j = qv[0, 0, 0].numpy(), qv[0, 0, 1].numpy()
        q_tot_table = np.zeros((3, 3))
        s = torch.ones(1, 1, 1)
        for i in range(3):
            for j in range(3):
                chosen = torch.stack((qv[:, :, 0, i], qv[:, :, 1, j]), dim=1).view(1, 1, 2)
                if self.args.alg == 'qplex':
                    v_tot = self.mixer(chosen, s, is_v=True)
                    onehot = torch.zeros(1, 1, 2, 3)
                    onehot[0, 0, 0, i] = 1
                    onehot[0, 0, 1, j] = 1
                    a_tot = self.mixer(chosen, s, actions=onehot, max_q_i=qv.max(dim=3)[0], is_v=False)
                    q_tot_table[i, j] = float(v_tot.item() + a_tot.item())
                else:
                    q_tot_table[i, j] = self.mixer(chosen, s).item()
        return q_tot_table, q_table_i, q_table_j
