"""MAICTDLearner: trains a MAICMAC (``--MAIC True --MAIC_train True``).  The reference's algorithm/MAIC_q_learner.py is
QLearner line for line: its loss has no MI or entropy term although its agent computes them (network/MAIC.py:88-123).  This
learner trains on the TD loss and, with ``args.mi_loss_weight`` / ``args.entropy_loss_weight`` positive, on those two as well -
the MI loss is the only thing that gives inference_net a gradient.  The schedule of the two is this project's own.

``train`` is QLearner's schedule with the message head in it, shaped like QLearnerWithState:
  - the three unrolls keep their hidden states, and csrc/maic_head.hip adds the gated messages to the eval, double-Q
    continuation and target Qs before the gathers, the greedy selections and the mixers (QPLEX's max_q included);
  - the head runs with sampled latents (test_mode False) in each network's own BatchNorm mode.  In training mode (a freshly built
    agent; the reference never leaves it) that is one head call per transition index, and every call moves the running
    statistics of its network; ``agent.eval()`` takes one call over all B*T*N rows;
  - after the TD loss, csrc/maic_head_bwd.hip turns the sparse pairs BPTT receives (u_act, dq) into the gradient on hs and
    the head's weight gradients, over the same rows per call as the forward; BPTT takes that dhs;
  - with a positive weight, csrc/maic_aux.hip runs in front of each of those backward calls, over the same rows and on the
    eval network's current pass alone (the double-Q continuation and the target pass carry no term):
    loss = TD + (1/T) sum_t (mi_t + ent_t), T = max_episode_len, one (mi_t, ent_t) per transition index over its B
    environments, padded steps included (as the world-model prediction term's).  It runs AFTER the loss kernel because its
    gradients are pre-scaled on the device by den / T, den = sum(mask) - the optimizer divides the whole gradient by den
    (FusedOptimizer.step) - and den is that kernel's output; what it needs of the forward (hs, eps, the returned Qs) is kept
    anyway, the rest is recomputed as the head's backward recomputes it.  The two sums land in slots 2 and 3 of the loss
    statistics (``last_stats``), the returned loss is s[0] / s[1] + (s[2] + s[3]) / T.  Exact in one process only.
    With both weights zero not one call differs from the TD-only learner.
``args.td_lambda`` reaches this learner through QLearner._loss_backward with no lines of its own.
The latents' noise is an optional argument of ``train`` (a dict of three (B,T,N,N*latent_dim) tensors: cur, next_eval,
next_target); absent, it is drawn from a generator this learner owns, seeded from args.seed.
Target copies carry the BatchNorm buffers (inference_net.1's too).  The update is never launched before max_episode_len is known
and never replayed from a hipGraph: a redone or replayed pass would move the running statistics and the generator on its own.
Multi-rank training is not supported: batch statistics are per rank, and so is den.
"""
from __future__ import annotations

import torch

from .common import agent_backward
from .q_learner import QLearner

NOISE_KEYS = ("cur", "next_eval", "next_target")


class MAICTDLearner(QLearner):
    # a pass redone at another length, or replayed from a graph, would move the running statistics and the generator on its own
    launch_ahead = False
    replay_graphs = False

    def __init__(self, mac, args):
        if getattr(mac, "head_name", None) != "MAIC":
            raise TypeError("MAICTDLearner needs a MAICMAC controller")
        super().__init__(mac, args)
        if self.reducer.enabled:
            raise NotImplementedError("multi-rank MAIC training: BatchNorm's batch statistics are per rank")
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(getattr(args, "seed", 0)))
        self._eps = None
        self.aux = getattr(args, "mi_loss_weight", 0) > 0 or getattr(args, "entropy_loss_weight", 0) > 0
        if self.aux:
            self.n_stats = 4      # TD numerator, sum(mask), sum_t mi_t, sum_t ent_t

    def _loss_fn(self):
        if not self.aux:
            return super()._loss_fn()
        T = float(self.max_episode_len)
        return lambda s: s[0] / s[1] + (s[2] + s[3]) / T

    def train(self, batch, train_step, eps=None):
        self._eps = eps
        try:
            return super().train(batch, train_step)
        finally:
            self._eps = None

    def _noise(self, B, T, N):
        """the three passes' noise as (B,T,N,N*latent_dim) device tensors: the caller's, cut to T, or this learner's draws"""
        NL = N * self.args.latent_dim
        keys = NOISE_KEYS if self.args.double_q else (NOISE_KEYS[0], NOISE_KEYS[2])
        if self._eps is None:
            return {k: torch.randn(B, T, N, NL, device=self.device, generator=self._gen) for k in keys}
        out = {}
        for k in keys:
            e = torch.as_tensor(self._eps[k]).to(device=self.device, dtype=torch.float32)
            if e.dim() != 4 or e.shape[0] != B or e.shape[1] < T or tuple(e.shape[2:]) != (N, NL):
                raise ValueError("eps[%r] has shape %s, expected (%d, >=%d, %d, %d)" % (k, tuple(e.shape), B, T, N, NL))
            out[k] = e[:, :T].contiguous()
        return out

    def _forward_backward(self, db):
        B, T, N, H = db.B, db.T, db.N, self.args.rnn_hidden_dim
        eps = self._noise(B, T, N)
        q_evals, q_en, q_tgt, saved, (hs, hs_en, hs_tgt) = self._unrolls(db, keep_hs=True)
        self.eval_net.head_over(hs, q_evals, B, T, False, eps["cur"])
        if self.args.double_q:
            self.eval_net.head_over(hs_en, q_en, B, T, False, eps["next_eval"])
        self.target_net.head_over(hs_tgt, q_tgt, B, T, False, eps["next_target"])

        q_chosen, q_tgt_chosen, cur_max = self._select(db, q_evals, q_en, q_tgt)
        q_tot, q_tot_tgt, ctx, fold = self._mix(db, q_evals, q_tgt, q_chosen, q_tgt_chosen, cur_max)
        self._flat.zero_grad()
        dq_val = self._loss_backward(db, q_chosen, q_tot, q_tot_tgt, ctx, fold).reshape(-1).contiguous()
        # the loss reaches q_evals only through the gather: the same sparse pairs go through the head (-> dhs, head gradients)
        # and, for the identity path, into BPTT
        u_act = db.u_act.reshape(-1)
        dhs = self._g("dhs", (B, T, N, H))
        if self.aux:          # stats[1] = sum(mask) is ready; the two sums go to stats[2], stats[3] (zeroed with the gradient)
            st = self._flat.stats
            self.eval_net.head_backward(hs, u_act, dq_val, B, T, False, eps["cur"], dhs, self._buf, q=q_evals,
                                        aux=(st[2:3], st[3:4], st[1:2]))
        else:
            self.eval_net.head_backward(hs, u_act, dq_val, B, T, False, eps["cur"], dhs, self._buf)
        agent_backward(self.eval_net, db, "cur", saved, hs, None, dhs, self._buf, dq_idx=u_act, dq_val=dq_val)
        self._dbg = dict(q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, q_tot_target=q_tot_tgt, hs=hs, **self._td_dbg)

    def _update_targets(self):
        super()._update_targets()
        src = dict(self.eval_net.agent.named_buffers())
        for k, b in self.target_net.agent.named_buffers():
            b.copy_(src[k])

    # ------------------------------------------------------------------ full resume: the buffers and the generator as well
    def resume_state(self):
        sd = super().resume_state()
        for name, net in (("eval", self.eval_net), ("target", self.target_net)):
            sd["maic_buffers_" + name] = {k: b.detach().cpu().clone() for k, b in net.agent.named_buffers()}
        sd["maic_noise"] = self._gen.get_state().cpu()
        return sd

    def load_resume_state(self, sd):
        super().load_resume_state(sd)
        for name, net in (("eval", self.eval_net), ("target", self.target_net)):
            for k, b in net.agent.named_buffers():
                b.copy_(sd["maic_buffers_" + name][k])
        self._gen.set_state(sd["maic_noise"])

    def get_q_and_q_tot_table(self):
        raise NotImplementedError("get_q_and_q_tot_table is not defined for the MAIC agent")
