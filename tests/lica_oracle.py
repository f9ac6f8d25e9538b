"""Float64 restatement of LICA (TEST INFRASTRUCTURE, written for this project from the definitions of include/marl_hip.h and
algorithm/lica.py's docstring, not from the kernels: the reference ships no LICA).  torch autograd over tests/policy_oracle.py's
policy, agent unroll and seeded learner cases, tests/td_lambda_oracle.returns and oracle.learners.clip_and_step.

* ``critic``               Q of the textbook form: four hypernetworks of the state, x W1 + b1, ReLU, . wf + b2, under autograd
* ``hyper``                the per-row [W1 | b1 | wf | b2] image of the hypernetworks' outputs (the kernels' ``hy``)
* ``rows``                 the kernels' analytic contract in numpy float64: q, dhy, dx, the TD loss folded in
* ``twin32``               the same arithmetic, sequentially, in numpy float32: the yardstick of the kernel-level bounds
* ``jt_formula`` / ``probs_bwd_reference``   the closed form of J^T g, and autograd through ``policy_oracle.policy`` (the oracle)
* ``State`` / ``forward`` / ``train``        what LICALearner owns and one ``train`` call, in ``dtype``
* ``CASES``, ``WEIGHT_SEEDS``, ``F32_EXCEPTIONS``
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import learners, nets, seeded
import coma_oracle as co
import pg_oracle as pg
import policy_oracle as po
import td_lambda_oracle as tl

EPS = po.EPS
BETAS = pg.BETAS
GAMMA = 0.99
State = po.State
onehot = co.onehot


# ------------------------------------------------------------------------------------------------ the critic
def critic_param_shapes(args):
    """the published state-dict layout, in LICACritic's order"""
    S, HE, E, K = args.state_shape, args.hypernet_embed, args.mixing_embed_dim, args.n_agents * args.n_actions
    two = lambda name, mid, out: [(name + ".0.weight", (mid, S)), (name + ".0.bias", (mid,)),
                                  (name + ".2.weight", (out, mid)), (name + ".2.bias", (out,))]
    return two("hyper_w_1", HE, K * E) + two("hyper_w_final", HE, E) + [("hyper_b_1.weight", (E, S)), ("hyper_b_1.bias", (E,))] + \
        two("hyper_b_2", E, 1)


def _two(p, name, s, pre):
    a = nets.lin(p, name + ".0", s)
    if pre is not None:
        pre.append(a)
    return nets.lin(p, name + ".2", torch.relu(a))


def hyper(p, s, pre=None):
    """(W1 (..., K E), b1 (..., E), wf (..., E), b2 (..., 1)) of the states s (..., S)"""
    return _two(p, "hyper_w_1", s, pre), nets.lin(p, "hyper_b_1", s), _two(p, "hyper_w_final", s, pre), _two(p, "hyper_b_2", s, pre)


def critic(p, x, s, pre=None):
    """Q (...) of x (..., K) and s (..., S); pre: a list that receives the ReLU pre-activations (three hypernetwork hiddens, the mix)"""
    w1, b1, wf, b2 = hyper(p, s, pre)
    K = x.shape[-1]
    a = b1 + torch.einsum("...k,...ke->...e", x, w1.reshape(*w1.shape[:-1], K, -1))
    if pre is not None:
        pre.append(a)
    return (torch.relu(a) * wf).sum(dim=-1) + b2[..., 0]


# ------------------------------------------------------------------------------------------------ the kernels' contract
def _split(hy, K, E):
    KE = K * E
    return hy[:, :KE].reshape(-1, K, E), hy[:, KE:KE + E], hy[:, KE + E:KE + 2 * E], hy[:, KE + 2 * E]


def onehot_rows(u, N, A, dtype=np.float64):
    """u (rows, N) -> (rows, N A); an index outside [0, A) gives an all-zero block"""
    u = np.asarray(u).reshape(-1, N)
    x = np.zeros((u.shape[0], N, A), dtype=dtype)
    ok = (u >= 0) & (u < A)
    r, i = np.nonzero(ok)
    x[r, i, u[r, i]] = 1.0
    return x.reshape(-1, N * A)


def rows(hy, N, A, E, x=None, u=None, dq=None, loss=None):
    """numpy float64.  hy (rows, K E + 2 E + 1); x (rows, K) or u (rows, N).  q always; with dq (rows): dhy (rows, K E + 2 E) and dx
    (rows, K); with loss = dict(q_tgt, r, term, padded, gamma): dq_tot = -2 m (m td), out2 = {sum (m td)^2, sum m} and the backward
    for dq = dq_tot - a padded row's hy, u, r and q_tgt are never looked at: exact zeros, nothing added"""
    hy = np.asarray(hy, dtype=np.float64)
    K = N * A
    x = onehot_rows(u, N, A) if x is None else np.asarray(x, dtype=np.float64)
    out = {}
    live = np.ones(hy.shape[0], dtype=bool)
    if loss is not None:
        m = 1.0 - np.asarray(loss["padded"], dtype=np.float64)
        live = m != 0
        hy = np.where(live[:, None], hy, 0.0)
        x = np.where(live[:, None], x, 0.0)
    W1, b1, wf, b2 = _split(hy, K, E)
    pre = b1 + np.einsum("rk,rke->re", x, W1)
    h = np.maximum(pre, 0.0)
    q = (h * wf).sum(axis=1) + b2
    out.update(q=q, pre=pre)
    if loss is not None:
        f = lambda k: np.where(live, np.asarray(loss[k], dtype=np.float64), 0.0)
        td = f("r") + loss["gamma"] * f("q_tgt") * (1.0 - f("term")) - q
        mtd = np.where(live, m * td, 0.0)
        dq = -2.0 * m * mtd
        out.update(dq_tot=dq, out2=np.array([(mtd * mtd).sum(), m.sum()]))
    if dq is not None:
        dq = np.asarray(dq, dtype=np.float64)
        dpre = dq[:, None] * wf * (pre > 0)
        out["dhy"] = np.concatenate([(x[:, :, None] * dpre[:, None, :]).reshape(len(q), -1), dpre, dq[:, None] * h], axis=1)
        out["dx"] = np.einsum("rke,re->rk", W1, dpre)
    return out


def twin32(hy, N, A, E, x=None, u=None, dq=None):
    """``rows`` in numpy float32, every sum taken sequentially in the order the header states (pre over k from b1, Q over e then
    + b2, dx over e): what float32 alone costs"""
    f = np.float32
    hy = np.asarray(hy, dtype=f)
    K = N * A
    x = onehot_rows(u, N, A, f) if x is None else np.asarray(x, dtype=f)
    W1, b1, wf, b2 = _split(hy, K, E)
    pre = b1.copy()
    for k in range(K):
        pre = (pre + (x[:, k, None] * W1[:, k, :]).astype(f)).astype(f)
    h = np.maximum(pre, f(0))
    q = np.zeros(len(hy), dtype=f)
    for e in range(E):
        q = (q + (h[:, e] * wf[:, e]).astype(f)).astype(f)
    q = (q + b2).astype(f)
    out = dict(q=q)
    if dq is not None:
        dq = np.asarray(dq, dtype=f)
        dpre = ((dq[:, None] * wf).astype(f) * (pre > 0)).astype(f)
        out["dhy"] = np.concatenate([(x[:, :, None] * dpre[:, None, :]).astype(f).reshape(len(q), -1), dpre,
                                     (dq[:, None] * h).astype(f)], axis=1)
        dx = np.zeros((len(q), K), dtype=f)
        for e in range(E):
            dx = (dx + (W1[:, :, e] * dpre[:, None, e]).astype(f)).astype(f)
        out["dx"] = dx
    return out


# (rows, N, A, E) of the kernel tests: one row; a full tile of 32 rows twice less one and plus one; two agents' worth of MMM2; the
# support corner (K = 512); an odd E without a 16-byte row pitch.  TILES: tiny rows, enough of them that the busiest workgroup walks
# two tiles (asserted from marl_lica_plan)
CASES = ((1, 1, 1, 1), (63, 5, 11, 32), (65, 5, 11, 32), (130, 10, 18, 32), (67, 16, 32, 64), (5, 3, 30, 7))
TILES_CASE = (64 * 1024 + 65, 2, 2, 4)
KINK = 1e-5


def kernel_case(R, N, A, E, seed):
    """float32 content of a mix test: hy of hypernetwork-like magnitudes (W1 ~ U(+-1/sqrt(K))), pi-like x with exact zeros on
    unavailable actions, taken actions u, an upstream gradient dq, TD operands.  Where a pre-activation of either input lies within
    1e-4 of the ReLU kink, that row's b1_e is moved by 1e-3 until none does (both inputs see the same b1), so every case is clear
    of KINK = 1e-5 with room for the float32 rounding"""
    K = N * A
    KE = K * E
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    hy = f(np.concatenate([rng.uniform(-1, 1, (R, KE)) / np.sqrt(K), rng.uniform(-0.5, 0.5, (R, E)),
                           rng.uniform(-1, 1, (R, E)), rng.uniform(-1, 1, (R, 1))], axis=1))
    avail = rng.random((R, N, A)) < 0.6
    avail[np.arange(R)[:, None], np.arange(N)[None], rng.integers(0, A, (R, N))] = True
    pt = avail * rng.random((R, N, A))
    x = f((pt / pt.sum(-1, keepdims=True)).reshape(R, K))
    u = np.argmax(avail * (0.5 + rng.random((R, N, A))), axis=-1).astype(np.int32)
    c = dict(hy=hy, x=x, u=u, dq=f(rng.standard_normal(R)), q_tgt=f(rng.standard_normal(R)), r=f(rng.standard_normal(R)),
             term=f(rng.random(R) < 0.2), padded=f(np.arange(R) % 3 == 1))
    for _ in range(50):
        near = (np.abs(rows(hy, N, A, E, x=x)["pre"]) < 10 * KINK) | (np.abs(rows(hy, N, A, E, u=u)["pre"]) < 10 * KINK)
        if not near.any():
            return c
        hy[:, KE:KE + E][near] += np.float32(1e-3)
    raise AssertionError("kernel_case: pre-activations stay near the kink")


# ------------------------------------------------------------------------------------------------ the policy's transpose-Jacobian
def jt_formula(z, a, g, eps):
    """the closed form of include/marl_hip.h, numpy float64: z, a, g (rows, A); rows with n = 0 give zeros"""
    z, a, g = (np.asarray(t, dtype=np.float64) for t in (z, a, g))
    n = a.sum(-1, keepdims=True)
    has = n > 0
    mx = np.where(a > 0, z, -np.inf).max(-1, keepdims=True)
    e = np.exp(np.minimum(z - np.where(has, mx, 0.0), 80.0))
    S, Sa = e.sum(-1, keepdims=True), (a * e).sum(-1, keepdims=True)
    D = (1.0 - eps) * Sa + eps * S
    nn = np.where(has, n, 1.0)
    pi = a * ((1.0 - eps) * e + eps * S / nn) / np.where(has, D, 1.0)
    ga = np.where(a > 0, g, 0.0)
    out = e / np.where(has, D, 1.0) * ((1.0 - eps) * a * ga + eps / nn * ga.sum(-1, keepdims=True)
                                     - ((1.0 - eps) * a + eps) * (pi * ga).sum(-1, keepdims=True))
    return np.where(has, out, 0.0)


def probs_bwd_case(B, T, N, A, seed):
    """coma_oracle.kernel_case's rows (every action available / exactly one / shifted by +1e4 / random availability; padded steps
    with logits of magnitude 1e6) with a gradient gpi (R, A) - magnitude 1e6 on padded steps - and q_pi (BT)"""
    c = po.kernel_rows(B, T, N, A, seed)
    rng = np.random.default_rng(seed + 2000)
    g = rng.standard_normal((B * T * N, A)) * 3.0
    pad = c["pad_rows"]
    g[pad] = 1.0e6 * np.where(rng.random((int(pad.sum()), A)) < 0.5, -1.0, 1.0)
    c["gpi"] = np.ascontiguousarray(g, dtype=np.float32)
    c["q_pi"] = np.ascontiguousarray(rng.standard_normal(B * T), dtype=np.float32)
    return c


def probs_bwd_reference(c, N, eps, beta, with_q=True):
    """float64 autograd through policy_oracle.policy of the float32 inputs as they are: dlogits = d/dz [ sum_live pi . gpi -
    beta sum m H ], ent, out3 = {- sum_r m q_pi - beta sum m H, sum_r m, sum m H}"""
    t = lambda k: torch.tensor(c[k].astype(np.float64))
    R, A = c["logits"].shape
    z = t("logits").requires_grad_(True)
    a, g = t("avail"), t("gpi")
    m = (1.0 - t("padded")).repeat_interleave(N)
    live = ((m > 0) & (a.sum(-1) > 0))[:, None]
    zs = torch.where(live, z, torch.zeros_like(z))                      # a dead row's logits and gpi are never looked at
    gs = torch.where(live & (a > 0), g, torch.zeros_like(g))
    pi = po.policy(zs, a, eps)
    H = torch.where(live[:, 0], pg.entropy(zs, a, eps), torch.zeros_like(m))
    hsum = (m * H).sum()
    (dz,) = torch.autograd.grad((pi * gs).sum() - beta * hsum, z)
    num = -beta * hsum.detach()
    if with_q:
        num = num - (m * t("q_pi").repeat_interleave(N)).sum()
    return dict(dlogits=dz.numpy(), ent=H.detach().numpy(), out3=np.array([float(num), float(m.sum()), float(hsum.detach())]))


# ------------------------------------------------------------------------------------------------ the learner
def make_args(shape, T, **over):
    kw = dict(lr_actor=1e-4, lr_critic=1e-3, critic_dim=128, td_lambda=0.8, grad_norm_clip=10, policy_entropy_coef=0.0)
    kw.update(over)
    return seeded.make_args(shape, "lica", episode_limit=T, **kw)


def forward(state, batch, eps, lam, beta=0.0):
    """Both losses and every intermediate the GPU tests compare"""
    args, dt = state.args, state.dtype
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}
    B, N, A, Hd = bt["o"].shape[0], args.n_agents, args.n_actions, args.rnn_hidden_dim
    K = N * A
    fed = nets.shifted_onehot(bt["u_onehot"])
    logits, _, _ = nets.agent_unroll(state.agent, bt["o"], fed, torch.zeros(B * N, Hd, dtype=dt), args.last_action, args.reuse_network)
    logits = logits.reshape(B, T, N, A)
    s = bt["s"].reshape(B, T, -1)
    u = bt["u"].reshape(B, T, N)
    xu = onehot(u, A, dt).reshape(B, T, K)
    pre = []
    q = critic(state.critic, xu, s, pre)                                               # (B, T)
    with torch.no_grad():
        q_tgt = critic(state.target_critic, xu, s)
        q_next = torch.cat([q_tgt[:, 1:], torch.zeros_like(q_tgt[:, :1])], dim=1)
    r, term, padded = (bt[k].reshape(B, T) for k in ("r", "terminated", "padded"))
    npdt = np.float64 if dt == torch.float64 else np.float32
    lam = 0.0 if lam is None else lam
    G = torch.tensor(tl.returns(q_next.numpy(), r.numpy(), term.numpy(), padded.numpy(), args.gamma, lam, dtype=npdt), dtype=dt)
    m = 1.0 - padded
    M = m.sum()
    l_critic = (m * (G - q) ** 2).sum() / M
    # the actor: Q(s, pi) through the critic at constant weights
    avail = bt["avail_u"].reshape(B, T, N, A)
    live = (m > 0)[:, :, None] & (avail.sum(-1) > 0)
    zs = torch.where(live[..., None], logits, torch.zeros_like(logits))
    pi = po.policy(zs, avail, eps)
    const = {k: v.detach() for k, v in state.critic.items()}
    pre_pi = []
    q_pi = critic(const, pi.reshape(B, T, K), s, pre_pi)
    H = torch.where(live, pg.entropy(zs, avail, eps), torch.zeros_like(zs[..., 0]))
    hsum = (m[:, :, None] * H).sum()
    den = N * M
    num_actor = -N * (m * q_pi).sum() - beta * hsum
    l_actor = num_actor / den
    dpi, dlogits = torch.autograd.grad(num_actor, [pi, logits], retain_graph=True)
    with torch.no_grad():
        fc1_pre = torch.stack([nets.lin(state.agent, "fc1", nets.build_inputs(bt["o"][:, t], fed[:, t], N, args.last_action,
                                                                            args.reuse_network)).view(B, N, Hd) for t in range(T)], 1)
    inter = dict(T=T, logits=logits, q=q, q_tgt=q_tgt, q_next=q_next, td_targets=G, pi=pi, q_pi=q_pi, dpi=dpi.reshape(B, T, K),
                 dlogits=dlogits, ent=H, l_critic=l_critic, l_actor=l_actor, den=den, M=M, entropy=hsum / den, mask=m,
                 fc1_pre=fc1_pre, critic_pre=[a.detach().reshape(B, T, -1) for a in pre + pre_pi[-1:]])
    return l_critic, l_actor, inter


relu_near_zero = po.relu_near_zero      # the agent's fc1; inter["critic_pre"]: the three hypernetwork hiddens, the mix on u and on pi


def train(state, batch, train_step, eps, lam, beta=0.0):
    """one LICALearner.train call: (critic loss, actor loss, gradients before the clips, intermediates)"""
    l_critic, l_actor, inter = forward(state, batch, eps, lam, beta)
    grads = {}
    pg._step(state.critic_half, l_critic, inter, grads)
    pg._step(state.actor_half, l_actor, inter, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    return float(l_critic.detach()), float(l_actor.detach()), grads, inter


# policy_oracle.LEARNER_CASES' shapes: 2s3z B = 4, lengths [1, -1, 4, 5]; MMM2 B = 3; matrix: nine one-step episodes.  (agent weight
# seed, critic weight seed): chosen on the CPU so that no ReLU pre-activation that carries a gradient lies within 1e-5 of zero in any
# run of YARDSTICK_RUNS (tests/test_lica_oracle_cpu.py asserts it)
WEIGHT_SEEDS = {"2s3z": (22, 31), "MMM2": (42, 45), "matrix": (14, 17)}
BATCH_SEEDS = {"2s3z": (100, 106), "MMM2": (100, 101)}


def learner_case(name, dtype=torch.float64, **over):
    """(args, State, batch(i)): batch(i) is the case's batch of update i.  target_update_cycle = 1: the second update crosses a sync"""
    _, shape, B, T, lengths, _ = next(c for c in po.LEARNER_CASES if c[0] == name)
    over.setdefault("target_update_cycle", 1)
    args = make_args(shape, T, **over)
    sa, sc = WEIGHT_SEEDS[name]
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), sa)
    critic_w = seeded.seeded_state(critic_param_shapes(args), sc)
    if shape == "matrix":
        batch = lambda i: po.matrix_batch()
    else:
        batch = lambda i: seeded.make_batch(args, B, seed=BATCH_SEEDS[name][i], lengths=lengths)
    return args, State(args, agent, critic_w, dtype), batch


# float32-oracle errors (max abs) of the tensors that do not stay under a quarter of 1e-4 * max|ref| (the GPU
# tests bound these alone by 4x the figure), measured by running the float64 and the float32 oracle on the CPU
# (tests/test_lica_oracle_cpu.py prints them); tensors from 0.6 of the quarter on are listed too, because the figure depends on the
# host's summation order: each entry is the largest seen on the two hosts the table was made on.  Nearly all are the critic's
# parameters: RMSprop's first steps are about 10 lr g / (|g| + 1e-7), so where a gradient is that small its rounding decides the
# step, and the second update's values follow the parameters the first one left.  keys: (case, td_lambda, beta, tensor)
F32_EXCEPTIONS = {
    ('2s3z', 0.8, 0.0, 'step0/param critic.hyper_w_1.0.weight'): 6.16e-05,
    ('2s3z', 0.8, 0.0, 'step0/param critic.hyper_w_1.2.weight'): 4.04e-06,
    ('2s3z', 0.8, 0.0, 'step0/param critic.hyper_b_2.0.weight'): 3.21e-06,
    ('2s3z', 0.8, 0.0, 'step1/q'): 2.45e-05,
    ('2s3z', 0.8, 0.0, 'step1/grad critic.hyper_w_1.2.weight'): 6.11e-06,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_w_1.0.weight'): 6.16e-05,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_w_1.2.weight'): 3.27e-06,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_w_final.0.weight'): 2.05e-06,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_w_final.2.weight'): 3.24e-06,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_b_1.weight'): 3.17e-06,
    ('2s3z', 0.8, 0.0, 'step1/param critic.hyper_b_2.0.weight'): 5.38e-06,
    ('2s3z', 0.0, 0.0, 'step0/param critic.hyper_w_1.0.weight'): 2.21e-06,
    ('2s3z', 0.0, 0.0, 'step0/param critic.hyper_w_final.2.weight'): 7.23e-06,
    ('2s3z', 0.0, 0.0, 'step0/param critic.hyper_b_2.0.bias'): 3.41e-05,
    ('2s3z', 0.0, 0.0, 'step1/grad critic.hyper_b_2.2.bias'): 4.65e-06,
    ('2s3z', 0.0, 0.0, 'step1/param critic.hyper_w_1.0.weight'): 2.67e-06,
    ('2s3z', 0.0, 0.0, 'step1/param critic.hyper_w_1.2.weight'): 4.10e-04,
    ('2s3z', 0.0, 0.0, 'step1/param critic.hyper_w_final.2.weight'): 7.23e-06,
    ('2s3z', 0.0, 0.0, 'step1/param critic.hyper_b_2.0.bias'): 3.40e-05,
    ('2s3z', 1.0, 0.0, 'step0/param critic.hyper_w_1.2.weight'): 1.10e-05,
    ('2s3z', 1.0, 0.0, 'step0/param critic.hyper_w_final.0.weight'): 1.64e-05,
    ('2s3z', 1.0, 0.0, 'step1/param critic.hyper_w_1.0.weight'): 1.84e-06,
    ('2s3z', 1.0, 0.0, 'step1/param critic.hyper_w_1.2.weight'): 1.10e-05,
    ('2s3z', 1.0, 0.0, 'step1/param critic.hyper_w_final.0.weight'): 1.64e-05,
    ('2s3z', 1.0, 0.0, 'step1/param critic.hyper_b_1.weight'): 5.87e-06,
    ('2s3z', 0.8, 0.01, 'step0/param critic.hyper_w_1.0.weight'): 6.16e-05,
    ('2s3z', 0.8, 0.01, 'step0/param critic.hyper_w_1.2.weight'): 4.04e-06,
    ('2s3z', 0.8, 0.01, 'step0/param critic.hyper_b_2.0.weight'): 3.21e-06,
    ('2s3z', 0.8, 0.01, 'step1/q'): 2.45e-05,
    ('2s3z', 0.8, 0.01, 'step1/grad critic.hyper_w_1.2.weight'): 6.11e-06,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_w_1.0.weight'): 6.16e-05,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_w_1.2.weight'): 3.27e-06,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_w_final.0.weight'): 2.05e-06,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_w_final.2.weight'): 3.24e-06,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_b_1.weight'): 3.17e-06,
    ('2s3z', 0.8, 0.01, 'step1/param critic.hyper_b_2.0.weight'): 5.38e-06,
    ('MMM2', 0.8, 0.0, 'step0/param agent.fc1.weight'): 2.57e-06,
    ('MMM2', 0.8, 0.0, 'step0/param critic.hyper_w_1.2.weight'): 1.24e-05,
    ('MMM2', 0.8, 0.0, 'step0/param critic.hyper_w_final.0.weight'): 1.37e-05,
    ('MMM2', 0.8, 0.0, 'step0/param critic.hyper_b_1.weight'): 1.49e-04,
    ('MMM2', 0.8, 0.0, 'step0/param critic.hyper_b_2.0.weight'): 2.00e-06,
    ('MMM2', 0.8, 0.0, 'step1/l_critic'): 4.45e-04,
    ('MMM2', 0.8, 0.0, 'step1/l_actor'): 3.50e-05,
    ('MMM2', 0.8, 0.0, 'step1/q'): 2.90e-04,
    ('MMM2', 0.8, 0.0, 'step1/q_pi'): 2.89e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_1.0.weight'): 1.15e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_1.0.bias'): 4.09e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_1.2.weight'): 7.79e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_1.2.bias'): 5.09e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_final.0.weight'): 3.73e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_final.0.bias'): 1.38e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_final.2.weight'): 1.31e-03,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_w_final.2.bias'): 8.47e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_1.weight'): 1.44e-04,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_1.bias'): 5.09e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_2.0.weight'): 3.18e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_2.0.bias'): 1.15e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_2.2.weight'): 6.40e-05,
    ('MMM2', 0.8, 0.0, 'step1/grad critic.hyper_b_2.2.bias'): 7.25e-05,
    ('MMM2', 0.8, 0.0, 'step1/critic.grad_norm'): 3.91e-03,
    ('MMM2', 0.8, 0.0, 'step1/critic.clip_coef'): 2.42e-06,
    ('MMM2', 0.8, 0.0, 'step1/param agent.fc1.weight'): 2.57e-06,
    ('MMM2', 0.8, 0.0, 'step1/param agent.rnn.weight_ih'): 2.10e-06,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_w_1.0.weight'): 1.17e-05,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_w_1.2.weight'): 1.24e-05,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_w_final.0.weight'): 3.04e-05,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_w_final.0.bias'): 1.95e-06,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_w_final.2.weight'): 2.44e-06,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_b_1.weight'): 1.49e-04,
    ('MMM2', 0.8, 0.0, 'step1/param critic.hyper_b_2.0.weight'): 3.27e-06,
}
# (case, td_lambda, beta) runs the GPU file makes two updates of
YARDSTICK_RUNS = (("2s3z", 0.8, 0.0), ("2s3z", 0.0, 0.0), ("2s3z", 1.0, 0.0), ("2s3z", 0.8, 0.01), ("MMM2", 0.8, 0.0),
                  ("matrix", 0.8, 0.0))
