"""WQMIXLearner: Weighted QMIX (Rashid et al., NeurIPS 2020), ``--alg ow_qmix`` / ``cw_qmix`` (the reference ships no WQMIX; the
definition is this project's own - DESIGN section 9, include/marl_hip.h).  Beside QMIX's eval agent and monotonic mixer there are a
central agent - a second SharedMAC agent, same architecture, same inputs, parameters of its own - and an unconstrained central
mixer Qc (network/mixer.py: CentralFFMixer), with target copies of both.  With rows (b, t), m = 1 - padded, u the taken actions:

    u^  = argmax_a masked q_evals (avail)          u^' = argmax_a masked q_en (avail_next; q_en the continuation, quirk Q1)
    Q_tot = Mixer(q_evals[u], s)      Q^ = Qc(qc[u], s)      Q^_g = Qc(qc[u^], s)  (CW)      Q^' = Qc_target(qc_tgt_next[u^'], s')
    y   = r + gamma (1 - term) Q^'                 or, with args.td_lambda, the lambda-return of Q^' (Learner._td_inputs)
    w   = 1 if y - Q_tot > 0 else alpha  (OW)      w = 1 if u == u^ for every agent or y > Q^_g, else alpha  (CW)
    L   = [ sum w (m (y - Q_tot))^2 + sum (m (y - Q^))^2 ] / sum m

y, w, u^, u^' and Q^_g are constants of the backward.  One update pass: the eval unroll (kept) and its continuation, the central
unroll on the current inputs (kept), the target central unroll on the next inputs, ONE selection pass over the agent rows
(csrc/wqmix.hip: marl_wqmix_select), the three (CW: four) mixer forwards, ONE loss pass over the steps (marl_wqmix_loss), the two
mixer backwards and two BPTTs on sparse (action, gradient) pairs.  The monotonic mixer takes the unfolded path (hip_forward ->
loss -> hip_backward).  The target copies of the eval agent and of the monotonic mixer enter no computation; they are kept and
synced because the frame and the resume code expect them.  All trained parameters sit in the one flat buffer: one fused
optimizer, one gradient-norm clip.  One rank, no hipGraph replay in this version."""
from __future__ import annotations

import copy

import torch

from .. import ops
from ..common.arguments import WQMIX_ALGS, wqmix_alpha_of      # (the validator lives beside get_wqmix_args)
from ..controller.share_params import SharedMAC
from ..hostutil import flatten_module
from ..network.mixer import QMixMixer, CentralFFMixer
from .common import MASK_BIG, LearnerParams, FlatView, GradReducer, agent_backward
from .q_learner import QLearner


class _Dbg(dict):
    """the update's intermediates; ``y`` is formed from its ingredients when somebody asks (nothing is launched for it in an update)"""

    def __missing__(self, key):
        if key != "y":
            raise KeyError(key)
        return self["_r"].reshape(-1) + self["_gamma"] * self["q_central_next"] * (1.0 - self["_term"].reshape(-1))


class WQMIXLearner(QLearner):
    n_stats, den_slot = 4, 1          # { sum w (m td)^2, sum m, sum (m tdc)^2, sum m [w == 1] }
    extra_nets = ("central_rnn", "central_mixer")
    replay_graphs = False

    def __init__(self, mac, args):
        if args.alg not in WQMIX_ALGS:
            raise ValueError("Mixer {} not recognised.".format(args.alg))
        if not args.double_q:
            raise ValueError("%s needs double_q: its target action is the eval agent's greedy one" % args.alg)
        if GradReducer().enabled:
            raise NotImplementedError("WQMIXLearner trains on one rank: its schedule has not been run data-parallel")
        self.alpha = wqmix_alpha_of(args)
        self._begin(mac, args, "WQMIXLearner")
        self.mixer = QMixMixer(args)
        self.target_mixer = copy.deepcopy(self.mixer)
        self.central_net = SharedMAC(args)
        self.target_central_net = copy.deepcopy(self.central_net)
        self.central_mixer = CentralFFMixer(args)
        self.target_central_mixer = copy.deepcopy(self.central_mixer)
        self.params = list(mac.parameters()) + list(self.mixer.parameters()) + list(self.central_net.parameters()) + \
            list(self.central_mixer.parameters())
        self.cuda()
        self._ready(needs_avail=args.alg == 'cw_qmix')       # the current-step availability masks the greedy action u^

    @property
    def central_rnn(self):
        """the central agent's network, under the name of its checkpoint file"""
        return self.central_net.agent

    def sync_replicas(self):
        o = self.optimizer
        self.reducer.broadcast_(self._flat.flat, self.target_net.agent._flat.flat, self.target_mixer._flat.flat,
                                self.target_central_net.agent._flat.flat, self.target_central_mixer._flat.flat, o.s1, o.s2)

    # ------------------------------------------------------------------ storage
    def cuda(self):
        """Move everything to the MI355X and (re)build the flat buffers: [eval agent | mixer | central agent | central mixer]."""
        dev = self.device
        for m in (self.mixer, self.target_mixer, self.central_mixer, self.target_central_mixer, self.eval_net.agent,
                  self.central_net.agent, self.target_net.agent, self.target_central_net.agent):
            m.to(dev)
        self._flat = LearnerParams(self.params, dev)
        start = 0
        for m in (self.eval_net.agent, self.mixer, self.central_net.agent, self.central_mixer):
            m._flat = FlatView(self._flat.flat, m.parameters(), start)
            start += m._flat.n
        for mac in (self.eval_net, self.target_net, self.central_net, self.target_central_net):
            mac._dev = dev
        for m in (self.target_net.agent, self.target_mixer, self.target_central_net.agent, self.target_central_mixer):
            flatten_module(m, dev)

    def _update_targets(self):
        super()._update_targets()
        self.target_central_net.agent._flat.flat.copy_(self.central_net.agent._flat.flat)
        self.target_central_mixer._flat.flat.copy_(self.central_mixer._flat.flat)

    def _target_flats(self):
        return dict(super()._target_flats(), target_central_agent=self.target_central_net.agent._flat.flat,
                    target_central_mixer=self.target_central_mixer._flat.flat)

    # ------------------------------------------------------------------ the hot path
    def _unrolls(self, db, keep_hs=False):
        """The four agent unrolls, one after another: eval current-Q (kept), its continuation over the next inputs (quirk Q1: from
        the eval pass's final hidden state), central current-Q (kept), target central next-Q.
        Returns q_evals, q_en, qc, qc_tgt, saved, saved_c."""
        a, g = self.args, self._g
        B, T, N, A, H = db.B, db.T, db.N, db.A, a.rnn_hidden_dim
        q_evals, saved = g("q_evals", (B, T, N, A)), g("saved", ops.saved_shape(T, B, N))
        qc, saved_c = g("qc_evals", (B, T, N, A)), g("saved_c", ops.saved_shape(T, B, N))
        q_en, qc_tgt = g("q_en", (B, T, N, A)), g("qc_tgt", (B, T, N, A))
        h_last, h_scr, h_c = g("h_last", (B * N, H)), g("h_scr", (B * N, H)), g("h_last_c", (B * N, H))
        (oc, oc_bs, oc_t0), (on, on_bs, on_t0) = db.o_cur, db.o_next
        kw = dict(ep_len=db.ep_len, ep_map=getattr(db, 'o_map', None))
        self.eval_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, q_evals, None, h_last, saved, h0=None, **kw)
        self.eval_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, q_en, None, h_scr, None, h0=h_last, **kw)
        self.central_net.unroll(oc, oc_bs, oc_t0, db.u_fed, db.u_bs, -1, B, T, qc, None, h_c, saved_c, h0=None, **kw)
        self.target_central_net.unroll(on, on_bs, on_t0, db.u_fed, db.u_bs, 0, B, T, qc_tgt, None, None, None, h0=None, **kw)
        return q_evals, q_en, qc, qc_tgt, saved, saved_c

    def _forward_backward(self, db):
        a, g = self.args, self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        BT = B * T
        R = BT * N
        cw = a.alg == 'cw_qmix'
        q_evals, q_en, qc, qc_tgt, saved, saved_c = self._unrolls(db)
        u = db.u_act.reshape(-1)
        q_taken, qc_taken, qc_next = g("q_taken", (R,)), g("qc_taken", (R,)), g("qc_next", (R,))
        u_next = g("u_next", (R,), torch.int32)
        u_greedy, qc_greedy = (g("u_greedy", (R,), torch.int32), g("qc_greedy", (R,))) if cw else (None, None)
        ops.wqmix_select(q_evals, qc, u, db.avail if cw else None, q_en, qc_tgt, db.avail_next, db.padded, MASK_BIG,
                         q_taken, qc_taken, u_next, qc_next, B, T, N, A, u_greedy=u_greedy, qc_greedy=qc_greedy)
        ctx, ctx_c = {}, {}
        q_tot = self.mixer.hip_forward(q_taken.view(BT, N), db.s, BT, ctx=ctx)
        q_cen = self.central_mixer.hip_forward(qc_taken.view(BT, N), db.s, BT, ctx=ctx_c)
        q_cen_g = self.central_mixer.hip_forward(qc_greedy.view(BT, N), db.s, BT, tag="g") if cw else None
        q_cen_next = self.target_central_mixer.hip_forward(qc_next.view(BT, N), db.s_next, BT, tag="t")
        self._flat.zero_grad()
        r, gamma = self._td_inputs(db, q_cen_next)        # args.td_lambda set: the lambda-returns as r, and gamma = 0
        dq_tot, dq_cen, w = g("dq_tot", (BT,)), g("dq_cen", (BT,)), g("w", (BT,))
        ops.wqmix_loss(q_tot, q_cen, q_cen_g, q_cen_next, r, db.term, db.padded, gamma, u if cw else None, u_greedy, self.alpha,
                       dq_tot, dq_cen, self._flat.stats[:4], BT, N, w=w)
        dq = self.mixer.hip_backward(ctx, dq_tot, BT)
        dqc = self.central_mixer.hip_backward(ctx_c, dq_cen, BT)
        # the loss reaches either agent's Qs only through the gather: BPTT takes the sparse (action, gradient) pairs
        agent_backward(self.eval_net, db, "cur", saved, None, None, None, self._buf, dq_idx=u, dq_val=dq.reshape(-1).contiguous())
        agent_backward(self.central_net, db, "cur", saved_c, None, None, None, self._buf, dq_idx=u,
                       dq_val=dqc.reshape(-1).contiguous())
        self._dbg = _Dbg(q_evals=q_evals, q_targets=qc_tgt, q_tot=q_tot, q_tot_target=q_cen_next, q_central=q_cen,
                         q_central_greedy=q_cen_g, q_central_next=q_cen_next, w=w, u_next=u_next.view(B, T, N),
                         u_greedy=None if u_greedy is None else u_greedy.view(B, T, N), _r=r, _gamma=gamma, _term=db.term,
                         **self._td_dbg)

    def _loss_fn(self):
        return lambda s: (s[0] + s[2]) / s[1]
