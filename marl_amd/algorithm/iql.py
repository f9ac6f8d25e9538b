"""IQLLearner: independent Q-learning, the value-side baseline without a mixer (the reference ships no IQL; the definition is this
project's own - DESIGN section 9, include/marl_hip.h).  Every agent regresses its own Q of the taken action onto its own target:
with rows r = (b, t, i), m = 1 - padded[b, t], q the eval unroll's Qs, q_sel its continuation over the next observations (quirk
Q1) and q_tgt the target unroll's,

    q_taken[r] = q[r, u[r]]
    q_next[r]  = q_tgt[r, argmax_a masked q_sel[r, a]]   (double_q; otherwise max_a of the masked q_tgt; masked with avail_next)
    y[r]       = r[b,t] + gamma (1 - term[b,t]) q_next[r]         or, with args.td_lambda, the lambda-return G[b, i, t] of agent i's
                 own sequence (csrc/td_lambda.hip on B N sequences; r, term and padded expanded over the agents on the host side)
    L          = sum m (y - q_taken)^2 / (N sum m)

One update pass: QLearner's three unrolls (the method itself), then ONE row pass (csrc/iql.hip) that gathers, selects, forms the
target, the loss statistics and the sparse (action, gradient) pairs BPTT takes - marl_q_gather, marl_q_double_select, the mixer
forward, marl_td_loss and the mixer backward of a VDN update in one launch (+ the fixed-order finish of the two sums).  With
td_lambda: marl_iql_select (q_next straight in (B, N, T) layout), marl_td_lambda_returns, marl_iql_loss_bwd on the returns.
Storage, optimizer, target sync, checkpoints (no mixer file), resume state, hipGraph replay, launch-ahead and the data-parallel
statistics tail are the frame's (algorithm/common.py)."""
from __future__ import annotations

from .. import ops
from ..hostutil import flatten_module
from .common import MASK_BIG, LearnerParams, FlatView, Learner, agent_backward, td_lambda_of
from .q_learner import QLearner


class IQLLearner(Learner):
    def __init__(self, mac, args):
        self._begin(mac, args, "IQLLearner")
        self.mixer = self.target_mixer = None
        self.params = list(mac.parameters())
        self.cuda()
        self._ready(needs_avail=False)

    def sync_replicas(self):
        o = self.optimizer
        self.reducer.broadcast_(self._flat.flat, self.target_net.agent._flat.flat, None, o.s1, o.s2)

    def cuda(self):
        """Move everything to the MI355X and (re)build the flat buffers."""
        dev = self.device
        self.eval_net.agent.to(dev)
        self._flat = LearnerParams(self.params, dev)
        self.eval_net.agent._flat = FlatView(self._flat.flat, self.eval_net.agent.parameters(), 0)
        self.eval_net._dev = dev
        self.target_net._dev = dev
        self.target_net.agent.to(dev)
        flatten_module(self.target_net.agent, dev)

    # ------------------------------------------------------------------ the hot path
    _unrolls = QLearner._unrolls      # eval current-Q (keeps activations), its double-Q continuation, target next-Q

    def _forward_backward(self, db):
        a, g = self.args, self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        R = B * T * N
        q_evals, q_en, q_tgt, saved, _ = self._unrolls(db)
        u = db.u_act.reshape(-1)
        q_sel = q_en if a.double_q else None
        lam = self.td_lambda = td_lambda_of(a)
        dq_val, q_taken = g("dq_val", (R,)), g("q_taken", (R,))
        stats = self._flat.stats[:2]
        self._flat.zero_grad()
        if lam is None:
            q_next = g("q_next", (R,))
            ops.iql_loss_bwd(q_evals, u, q_sel, q_tgt, db.avail_next, None, db.r, db.term, db.padded, self.gamma, MASK_BIG,
                             dq_val, stats, B, T, N, A, q_taken=q_taken, q_next=q_next)
            dbg = dict(q_next=q_next.view(B, T, N))
        else:
            q_next, G = g("q_next_bnt", (B, N, T)), g("td_ret", (B, N, T))
            ops.iql_select(q_evals, u, q_sel, q_tgt, db.avail_next, db.padded, MASK_BIG, q_taken, q_next, B, T, N, A)
            per_agent = g("per_agent", (3, B, N, T))        # r, term and padded per agent sequence: plumbing, as COMA's
            for k, x in enumerate((db.r, db.term, db.padded)):
                per_agent[k].copy_(x.reshape(B, 1, T).expand(B, N, T))
            ops.td_lambda_returns(q_next, per_agent[0], per_agent[1], per_agent[2], self.gamma, lam, G, B * N, T)
            ops.iql_loss_bwd(q_evals, u, None, None, None, G, None, None, db.padded, self.gamma, MASK_BIG, dq_val, stats,
                             B, T, N, A)
            dbg = dict(q_next=q_next.permute(0, 2, 1), td_targets=G)
        # the loss reaches q_evals only through the gather: BPTT takes the sparse (action, gradient) pairs
        agent_backward(self.eval_net, db, "cur", saved, None, None, None, self._buf, dq_idx=u, dq_val=dq_val)
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_taken=q_taken.view(B, T, N), **dbg)

    def get_q_and_q_tot_table(self):
        raise NotImplementedError("IQL has no joint value: there is no q_tot table")
