"""Float64 restatement of the policy-gradient loss with an entropy bonus, of REINFORCE and of central-V with the bonus (TEST
INFRASTRUCTURE, written for this project: the reference ships REINFORCE as an argument table only).  torch autograd over
tests/policy_oracle.py's policy, agent unroll and seeded learner cases, tests/td_lambda_oracle.returns and
oracle.learners.clip_and_step.

* ``has_policy``   n > 0 and the taken action available
* ``log_prob`` / ``entropy``   log pi(u) and H = - sum_{a_k = 1} pi_k log pi_k of the eps-mixed, masked policy; 0 log 0 = 0; both 0
                   on a row without a policy
* ``numerator``    - sum m Adv log pi(u) - beta sum m H with Adv = G - v, or G where v is None; rows with m = 0 or without a policy
                   contribute nothing and their logits are never looked at (they may hold NaN)
* ``State`` / ``forward`` / ``train``   what ReinforceLearner owns and one ``train`` call
* ``central_v_train``   policy_oracle.train with the bonus in the actor loss
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import learners, nets, seeded
import policy_oracle as po
import td_lambda_oracle as tl

EPS = po.EPS
BETAS = (0.0, 0.01)


# ------------------------------------------------------------------------------------------------ a row
def has_policy(avail, u):
    a_u = torch.gather(avail, -1, u.unsqueeze(-1)).squeeze(-1)
    return (avail.sum(dim=-1) > 0) & (a_u > 0)


def log_prob(z, avail, u, eps):
    """log pi(u) (...); 0 on rows without a policy (no available action, or a taken action that is not available)"""
    pi_u = torch.gather(po.policy(z, avail, eps), -1, u.unsqueeze(-1)).squeeze(-1)
    has = has_policy(avail, u)
    return torch.where(has, torch.log(torch.where(has, pi_u, torch.ones_like(pi_u))), torch.zeros_like(pi_u))


def entropy(z, avail, eps):
    """H (...) = - sum over the available actions of pi log pi; a term with pi = 0 is 0 (not 0 * -inf); n = 1: pi = 1, H = 0"""
    pi = po.policy(z, avail, eps)
    pos = (pi > 0) & (avail > 0)
    term = torch.where(pos, pi * torch.log(torch.where(pos, pi, torch.ones_like(pi))), torch.zeros_like(pi))
    return -term.sum(dim=-1)


def numerator(z, avail, u, G, v, padded, eps, beta):
    """z, avail (BT, N, A); u (BT, N); G, padded (BT); v (BT) or None.  Returns (- sum m Adv log pi(u) - beta sum m H,
    log pi(u) (BT, N), H (BT, N), N sum m, sum m H): log pi and H are 0 on rows with m = 0 or without a policy"""
    m = 1.0 - padded
    live = (m[:, None] > 0) & has_policy(avail, u)
    z = torch.where(live[..., None], z, torch.zeros_like(z))             # a dead row's logits are never looked at
    adv = torch.where(m > 0, G if v is None else G - v, torch.zeros_like(G)).detach()
    zero = torch.zeros(live.shape, dtype=z.dtype)
    logp = torch.where(live, log_prob(z, avail, u, eps), zero)
    H = torch.where(live, entropy(z, avail, eps), zero)
    num = -(m[:, None] * adv[:, None] * logp).sum() - beta * (m[:, None] * H).sum()
    return num, logp, H, z.shape[1] * m.sum(), (m[:, None] * H).sum()


def kernel_reference(rows, N, eps, beta, with_v=True):
    """float64 of the float32 kernel inputs as they are: logp, ent (R), dlogits (autograd of the numerator), the three statistics"""
    t = lambda k: torch.tensor(rows[k].astype(np.float64))
    R, A = rows["logits"].shape
    z = t("logits").requires_grad_(True)
    a, u = t("avail"), torch.tensor(rows["u"].astype(np.int64))
    num, logp, H, den, hsum = numerator(z.view(R // N, N, A), a.view(R // N, N, A), u.view(R // N, N), t("G"),
                                        t("v") if with_v else None, t("padded"), eps, beta)
    (dz,) = torch.autograd.grad(num, z)
    return dict(logp=logp.detach().reshape(R).numpy(), ent=H.detach().reshape(R).numpy(), dlogits=dz.numpy(),
                stats=np.array([float(num.detach()), float(den), float(hsum.detach())]))


def special_rows(rows, N):
    """kernel_rows content with three special rows written in (all on real steps): a row whose taken action is unavailable, a row
    with a logit 200 below the largest available one (available itself: pi underflows there at eps = 0), a row whose unavailable
    logit towers 100 over the available ones.  Returns the row indices"""
    real = np.nonzero(~rows["pad_rows"])[0]
    many = [r for r in real if rows["avail"][r].sum() >= 2 and rows["avail"][r].sum() < rows["avail"].shape[1]]
    assert len(many) >= 3
    bad_u, deep, tower = many[0], many[1], many[2]
    rows["u"][bad_u] = int(np.nonzero(rows["avail"][bad_u] == 0)[0][0])
    k = [int(i) for i in np.nonzero(rows["avail"][deep])[0] if i != rows["u"][deep]][0]
    rows["logits"][deep, k] = rows["logits"][deep][rows["avail"][deep] > 0].max() - 200.0
    k = int(np.nonzero(rows["avail"][tower] == 0)[0][0])
    rows["logits"][tower, k] = rows["logits"][tower][rows["avail"][tower] > 0].max() + 100.0
    return dict(bad_u=bad_u, deep=deep, tower=tower)


# ------------------------------------------------------------------------------------------------ REINFORCE
def make_args(shape, T, **over):
    kw = dict(lr_actor=1e-4, grad_norm_clip=10, policy_entropy_coef=0.0)
    kw.update(over)
    return seeded.make_args(shape, "reinforce", episode_limit=T, **kw)


class State:
    def __init__(self, args, agent, dtype=torch.float64):
        self.args, self.dtype = args, dtype
        self.agent = {k: torch.tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True) for k, x in agent.items()}
        self.actor_half = po._Half(args, "agent.", self.agent, args.lr_actor)


def _cut(batch, T, dt):
    return {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}


def forward(state, batch, eps, beta):
    """the loss and every intermediate the GPU tests compare"""
    args, dt = state.args, state.dtype
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = _cut(batch, T, dt)
    B, N, H = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim
    fed = nets.shifted_onehot(bt["u_onehot"])
    logits, _, _ = nets.agent_unroll(state.agent, bt["o"], fed, torch.zeros(B * N, H, dtype=dt), args.last_action, args.reuse_network)
    r, term, padded = (bt[k].reshape(B, T) for k in ("r", "terminated", "padded"))
    npdt = np.float64 if dt == torch.float64 else np.float32
    # the discounted Monte-Carlo return: lambda = 1 on an all-zero q (an episode cut at T gets no bootstrap)
    G = torch.tensor(tl.returns(np.zeros((B, T)), r.numpy(), term.numpy(), padded.numpy(), args.gamma, 1.0, dtype=npdt), dtype=dt)
    num, logp, ent, den, hsum = numerator(logits.reshape(B * T, N, -1), bt["avail_u"].reshape(B * T, N, -1), bt["u"].reshape(B * T, N),
                                          G.reshape(-1), None, padded.reshape(-1), eps, beta)
    loss = num / den
    m = 1.0 - padded
    with torch.no_grad():
        fc1_pre = torch.stack([nets.lin(state.agent, "fc1", nets.build_inputs(bt["o"][:, t], fed[:, t], N, args.last_action,
                                                                            args.reuse_network)).view(B, N, H) for t in range(T)], 1)
    inter = dict(T=T, logits=logits, td_targets=G, logp=logp.reshape(B, T, N), ent=ent.reshape(B, T, N), loss=loss,
                 entropy=hsum / den, den=den, M=m.sum(), mask=m, fc1_pre=fc1_pre, critic_pre=[])
    return loss, inter


def _step(half, loss, inter, grads):
    named = half.named_params()
    gs = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    g = {n: (x if x is not None else torch.zeros_like(p)) for (n, p), x in zip(named, gs)}
    norm, coef = learners.clip_and_step(half, g)
    inter[half.prefix + "grad_norm"], inter[half.prefix + "clip_coef"] = norm, coef
    grads.update(g)


def train(state, batch, train_step, eps, beta):
    """one ReinforceLearner.train call: (loss, gradients before the clip, intermediates)"""
    loss, inter = forward(state, batch, eps, beta)
    grads = {}
    _step(state.actor_half, loss, inter, grads)
    return float(loss.detach()), grads, inter


# weight seeds and data seeds of update 0 and 1 (policy_oracle's cases and batches): no ReLU pre-activation that carries a gradient
# lies within 1e-5 of zero in either update at either beta (tests/test_pg_oracle_cpu.py asserts the count)
BATCH_SEEDS = {"2s3z": (100, 106), "MMM2": (100, 101)}


def learner_case(name, dtype=torch.float64, **over):
    """(args, State, batch(i)) of REINFORCE on policy_oracle's learner case ``name``"""
    _, shape, B, T, lengths, seed = next(c for c in po.LEARNER_CASES if c[0] == name)
    args = make_args(shape, T, **over)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed)
    if shape == "matrix":
        batch = lambda i: po.matrix_batch()
    else:
        batch = lambda i: seeded.make_batch(args, B, seed=BATCH_SEEDS[name][i], lengths=lengths)
    return args, State(args, agent, dtype), batch


# ------------------------------------------------------------------------------------------------ central-V with the bonus
def central_v_train(state, batch, train_step, eps, lam, beta):
    """policy_oracle.train with L_actor = [- sum m Adv log pi(u) - beta sum m H] / (N M)"""
    l_critic, _, inter = po.forward(state, batch, eps, lam)
    T, dt, N = inter["T"], state.dtype, state.args.n_agents
    bt = _cut({k: batch[k] for k in ("avail_u", "u", "padded")}, T, dt)
    B = bt["u"].shape[0]
    num, logp, ent, den, hsum = numerator(inter["logits"].reshape(B * T, N, -1), bt["avail_u"].reshape(B * T, N, -1),
                                          bt["u"].reshape(B * T, N), inter["td_targets"].reshape(-1), inter["v"].reshape(-1),
                                          bt["padded"].reshape(-1), eps, beta)
    l_actor = num / den
    inter.update(l_actor=l_actor, logp=logp.reshape(B, T, N), ent=ent.reshape(B, T, N), entropy=hsum / den)
    grads = {}
    _step(state.critic_half, l_critic, inter, grads)
    _step(state.actor_half, l_actor, inter, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    return float(l_critic.detach()), float(l_actor.detach()), grads, inter


# float32-oracle errors (max abs) of the tensors that do not stay under a quarter of 1e-4 * max|ref| (the GPU
# tests bound these alone by 4x the figure).  keys: (alg, case, beta, tensor)
F32_EXCEPTIONS = {}
# (alg, case, beta) runs the GPU file makes two updates of
YARDSTICK_RUNS = tuple(("reinforce", n, b) for n in ("2s3z", "MMM2", "matrix") for b in BETAS) + (("central_v", "2s3z", 0.01),)
