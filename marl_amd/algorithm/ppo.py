"""PPOLearner: PPO with a centralised value function (MAPPO; the reference ships neither code nor a table for it - the definitions
are this project's own, from the published algorithm - DESIGN section 9, include/marl_hip.h).

The actor and the critic are central-V's (PolicyMAC, VCritic); what differs is that one rollout is used for K = ``args.ppo_epochs``
gradient steps, made safe by the clipped surrogate.  Once per batch, on the weights as they stand (there is no target network: the
same critic bootstraps), with m = 1 - padded and M = sum m:

    G   = the lambda-returns of V(s_next) (csrc/td_lambda.hip)            adv = G - V(s): GAE(lambda)
    adv = m (adv - mean) / (sqrt(var) + 1e-5) over the live steps         (``args.ppo_norm_adv``; csrc/ppo.hip)

both constants of every pass.  Pass k = 0 .. K-1, on the weights pass k-1 left:

    L_critic = sum m (G - V(s))^2 / M                                      (exactly central-V's, against the fixed G)
    rho      = pi(u) / pi_0(u), pi_0 the policy of pass 0 (rho = 1 exactly there)
    L_actor  = [ - sum m min(rho adv, clamp(rho, 1 - c, 1 + c) adv) - beta sum m H ] / (N M),     c = ``args.ppo_clip``

(ops.ppo_loss_bwd, csrc/policy.hip).  Pass 0 writes its log pi(u) into the buffer the later passes read as logp_old.  After every
pass but the last both optimizers step with their own denominators (M and N M); the last pass's step is the frame's
``_finish_update``, which also reads back the last pass's losses, entropy and ``clip_frac`` = the clipped share of the live agent
steps.  ``on_epoch`` (default None) is called as ``on_epoch(k, self._dbg)`` after each pass's backward and before its optimizer
step.  Mini-batches, early stopping on KL, value clipping and value normalisation are not built.  ``args.td_lambda`` None means 0.
Storage, checkpoints and resume state are PolicyLearner's with ``has_target_critic = False``; one rank, eager launches.
"""
from __future__ import annotations

import numbers

import torch

from .. import ops
from .central_v import CentralVLearner
from .common import LossReadback


def ppo_settings_of(args):
    """(ppo_clip, ppo_epochs, ppo_norm_adv) of args; absent or None = 0.2, 5, True.  A clip outside (0, 1) or fewer than one pass
    is an error"""
    clip, epochs, norm = (getattr(args, k, None) for k in ("ppo_clip", "ppo_epochs", "ppo_norm_adv"))
    clip, epochs, norm = 0.2 if clip is None else clip, 5 if epochs is None else epochs, True if norm is None else norm
    if isinstance(clip, bool) or not isinstance(clip, numbers.Real) or not 0.0 < clip < 1.0:
        raise ValueError("ppo_clip must lie in (0, 1), got %r" % (clip,))
    if isinstance(epochs, bool) or not isinstance(epochs, numbers.Integral) or epochs < 1:
        raise ValueError("ppo_epochs must be an integer >= 1, got %r" % (epochs,))
    return float(clip), int(epochs), bool(norm)


class PPOLearner(CentralVLearner):
    has_target_critic = False
    _no_q_table = "MAPPO has no Q table: its critic is a state value"
    on_epoch = None
    clip_frac = float("nan")

    def __init__(self, mac, args):
        self.clip, self.epochs, self.norm_adv = ppo_settings_of(args)      # raises before anything is built
        super().__init__(mac, args)
        self.clip_readback = LossReadback(args)

    # ------------------------------------------------------------------ the hot path
    def _forward_backward(self, db):
        g = self._g
        B, T, N, A = db.B, db.T, db.N, db.A
        BT, R = B * T, B * T * N
        lam = self._lambda()
        self.clip, self.epochs, self.norm_adv = ppo_settings_of(self.args)
        # once per batch: V(s), V(s_next) of the same critic, the lambda-returns and the advantage - buffers no pass writes
        v0 = self._critic_forward(self.critic, db.s, BT, "0", False).view(BT)
        v_next = self._critic_forward(self.critic, db.s_next, BT, "n", False).view(BT)
        G, adv = g("td_ret", (BT,)), g("ppo_adv", (BT,))
        ops.td_lambda_returns(v_next, db.r, db.term, db.padded, self.gamma, lam, G, B, T)
        torch.sub(G, v0, out=adv)                        # (the subtraction the central-V loss kernel makes per row: plumbing here)
        if self.norm_adv:
            ops.masked_standardize(adv, db.padded, adv, g("ppo_adv_stats", (3,)), BT)
        u = db.u_act.reshape(-1)
        dlogits, dv, ent = g("dlogits", (B, T, N, A)), g("c_dv", (BT, 1)), g("ent", (R,))
        logp_old, logp_new = g("logp_old", (R,)), g("logp", (R,))
        for k in range(self.epochs):
            self._flat.zero_grad()
            self._cflat.zero_grad()
            logits, saved, hs = self._actor_unroll(db)
            # the critic against the fixed G: target G + 0 V_next (1 - term) = G
            v, h1, h2 = self._critic_forward(self.critic, db.s, BT, "", True)
            ops.td_loss(v.view(BT), v_next, G, db.term, db.padded, 0.0, dv.view(BT), self._cflat.stats[:2], BT)
            self._critic_backward(db.s, h1, h2, dv, BT)
            # the actor: pass 0 is the policy the later passes' ratios are taken against
            logp = logp_old if k == 0 else logp_new
            ops.ppo_loss_bwd(logits, db.avail, u, adv, None if k == 0 else logp_old, db.padded, self.epsilon, self.beta, self.clip,
                             dlogits, logp, ent, self._flat.stats[:4], R, N, A)
            self._actor_backward(db, saved, hs, dlogits)
            self._dbg = dict(logits=logits, v=v.view(BT), v0=v0, v_next=v_next, td_targets=G, adv=adv, logp=logp, logp_old=logp_old,
                             dlogits=dlogits, ent=ent)
            if self.on_epoch is not None:
                self.on_epoch(k, self._dbg)
            if k + 1 < self.epochs:                      # (the last pass's step is _finish_update's)
                self.critic_optimizer.step(den=self._cflat.stats[1:2])
                self.optimizer.step(den=self._flat.stats[1:2])

    def _finish_update(self, train_step):
        loss = super()._finish_update(train_step)
        st = self._flat.stats
        if self.beta == 0.0:                             # (the frame reads the entropy only where every actor pass computes it: this one does)
            self.entropy = self.entropy_readback.read(st[:3], lambda s: s[2] / s[1])
        self.clip_frac = self.clip_readback.read(st[:4], lambda s: s[3] / s[1])
        return loss
