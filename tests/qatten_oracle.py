"""The Qatten mixer in float64 (TEST INFRASTRUCTURE, CPU), written from the definition in include/marl_hip.h and the QattenMixer
docstring, not from the kernel.

* ``mix`` / ``attend``   the UNFOLDED textbook form under torch autograd: keys built per agent, torch.softmax.  The truth for everything
* ``rows``               the row kernel's contract, folded (p_h = Wk_h^T e_h) and analytic, float64: q_tot, dq, dp, dw_raw, dq_tot, the
                         two loss sums, and the magnitudes the bounds are made of
* ``twin32``             the same arithmetic, sequentially, in numpy float32
* ``State`` / ``forward`` / ``train``   what QLearner(alg='qatten') owns and one ``train`` call over oracle.nets' agent unroll in ``dtype``
                         (oracle.learners.q_forward does not know the name): quirks Q1, Q2, Q6 as q_forward has them
* ``kernel_case`` / ``CASES``   seeded fp32 inputs of the kernel tests

Bounds.  An output of the fp32 kernel is held to  K * u * (1 + L) * mag  of ``rows``: u = 2^-24; L the row's largest
scale * sum_k |p_{h,k} u_{i,k}| (a logit's absolute error becomes a relative error of lam); mag the float64 sum of the absolute values of
the output's terms.  The constants are FOUR TIMES the worst ratio err / (u (1 + L) mag) of ``twin32`` against ``rows`` over CASES,
rounded up to a power of two - the factor covers a device exp of a few ulp where libm's has one, tree-ordered sums and free
contraction.  Measured twin ratios (tests/test_qatten_oracle_cpu.py prints and bounds them by K / 4):
    q_tot 1.763   dq 2.295   dw_raw 2.063   dp 98247.2   dp against the wide magnitude 2.560
dp's terms are  scale |g| |w_h| lam_{h,i} |q_i - y_h| |u_{i,k}|:  that magnitude takes q_i - y_h for one exact term, but y_h carries an
absolute error of u (1 + L) sum_j lam_j |q_j|, and on a row whose softmax saturates (lam_i -> 1, y_h -> q_i) the difference cancels to
nothing while the error stays - hence the ratio of 1e5 and K_DP = 2^19, which holds the saturated rows and little else.  So dp is ALSO
held to K_DP_WIDE u (1 + L) mag_dp_wide, the same sum with |q_i - y_h| taken apart into |q_i| + sum_j lam_j |q_j|: the bound that bites.
"""
import types

import numpy as np
import torch

from oracle import learners, nets, seeded
import td_lambda_oracle as tl

NS = types.SimpleNamespace
f32 = np.float32
U32 = 2.0 ** -24
GAMMA = float(f32(0.99))
K_QTOT, K_DQ, K_DW, K_DP, K_DP_WIDE = 8.0, 16.0, 16.0, 2.0 ** 19, 16.0


def dims(args):
    """(N, U, H, D, S): unset qatten_* fields take the table's 4, 32, S // N"""
    S, N = args.state_shape, args.n_agents
    g = lambda k, d: d if getattr(args, k, None) is None else getattr(args, k)
    return N, g("qatten_unit_dim", S // N), g("qatten_heads", 4), g("qatten_embed_dim", 32), S


def param_shapes(args):
    """QattenMixer's state_dict, in order"""
    N, U, H, D, S = dims(args)
    HE = args.hypernet_embed
    lin = lambda p, o, i: [(p + ".weight", (o, i)), (p + ".bias", (o,))]
    out = []
    for h in range(H):
        out += lin("query.%d.0" % h, HE, S) + lin("query.%d.2" % h, D, HE)
    out += [("key.%d.weight" % h, (D, U)) for h in range(H)]
    return out + lin("head_weight.0", HE, S) + lin("head_weight.2", H, HE) + lin("const.0", D, S) + lin("const.2", 1, D)


def _mlp(P, name, x):
    h = torch.relu(x @ P[name + ".0.weight"].T + P[name + ".0.bias"])
    return h @ P[name + ".2.weight"].T + P[name + ".2.bias"]


def attend(e, Wk, w_raw, c, q, s, N, U, D):
    """unfolded: e, Wk lists over the heads ((R, D), (D, U)); w_raw (R, H); c (R); q (R, N); s (R, >= N U) -> q_tot (R)"""
    R = q.shape[0]
    u = s[:, :N * U].reshape(R, N, U)
    ys = []
    for e_h, W in zip(e, Wk):
        keys = u @ W.T                                              # (R, N, D): the key of every agent
        lam = torch.softmax((keys * e_h[:, None, :]).sum(-1) / np.sqrt(D), dim=1)
        ys.append((lam * q).sum(1))
    return (w_raw.abs() * torch.stack(ys, 1)).sum(1) + c


def mix(P, q, s, args):
    """q_tot (R) of the mixer with parameters P (name -> tensor) on q (R, N), s (R, S)"""
    N, U, H, D, S = dims(args)
    e = [_mlp(P, "query.%d" % h, s) for h in range(H)]
    Wk = [P["key.%d.weight" % h] for h in range(H)]
    return attend(e, Wk, _mlp(P, "head_weight", s), _mlp(P, "const", s).squeeze(1), q, s, N, U, D)


# ------------------------------------------------------------------------------------------------ the kernel's contract
def _contract(dt, s, p, w_raw, c, q, scale, N, U, H, g=None, loss=None):
    """folded and analytic, every sum sequential, in dtype dt"""
    a = lambda x: np.asarray(x, dtype=dt)
    s, p, w_raw, c, q = a(s), a(p), a(w_raw), a(c), a(q)
    scale = dt(scale)
    R = q.shape[0]
    u = s[:, :N * U].reshape(R, N, U)
    ph = p.reshape(R, H, U)
    lam = np.zeros((R, H, N), dt)
    y = np.zeros((R, H), dt)
    for h in range(H):
        l = np.zeros((R, N), dt)
        for i in range(N):
            d = np.zeros(R, dt)
            for k in range(U):
                d = d + ph[:, h, k] * u[:, i, k]
            l[:, i] = scale * d
        ex = np.exp(l - l.max(axis=1, keepdims=True))
        sm = np.zeros(R, dt)
        for i in range(N):
            sm = sm + ex[:, i]
        lam[:, h] = ex / sm[:, None]
        for i in range(N):
            y[:, h] = y[:, h] + lam[:, h, i] * q[:, i]
    aw = np.abs(w_raw)
    q_tot = np.zeros(R, dt)
    for h in range(H):
        q_tot = q_tot + aw[:, h] * y[:, h]
    q_tot = q_tot + c
    o = NS(q_tot=q_tot, lam=lam, y=y)
    if loss is not None:
        q_tgt, r, term, padded = (a(x) for x in loss[:4])
        gamma = dt(loss[4])
        m = dt(1) - padded
        td = r + gamma * q_tgt * (dt(1) - term) - q_tot
        mtd = m * td
        g = dt(-2) * m * mtd
        o.num, o.den = float(np.sum((mtd * mtd).astype(np.float64))), float(np.sum(m.astype(np.float64)))
        o.mtd = mtd
        o.mag_td = np.abs(r) + np.abs(gamma * q_tgt * (dt(1) - term)) + np.abs(q_tot)
    if g is None:
        return o
    g = a(g)
    o.dq_tot = g
    ai = np.zeros((R, N), dt)
    for h in range(H):
        ai = ai + aw[:, h, None] * lam[:, h]
    o.a, o.dq = ai, g[:, None] * ai
    o.dw_raw = g[:, None] * y * np.sign(w_raw)
    dl = (g[:, None] * aw)[:, :, None] * lam * (q[:, None, :] - y[:, :, None])
    dp = np.zeros((R, H, U), dt)
    for i in range(N):
        dp = dp + dl[:, :, i, None] * u[:, None, i, :]
    o.dp = (scale * dp).reshape(R, H * U)
    return o


def rows(s, p, w_raw, c, q, scale, N, U, H, g=None, loss=None):
    """The contract in float64.  g (R) = dL/dq_tot, or loss = (q_tot_tgt, r, term, padded, gamma): then g = -2 m (m td).  Returns
    q_tot, dq, dp (R, H U), dw_raw, dq_tot, num, den and L (R), mag_qtot (R), mag_dq (R, N), mag_dw (R, H), mag_dp (R, H U), mag_num"""
    f = lambda x: np.asarray(x, dtype=np.float64)
    o = _contract(np.float64, s, p, w_raw, c, q, scale, N, U, H, g, loss)
    s, p, w_raw, c, q = f(s), f(p), f(w_raw), f(c), f(q)
    R = q.shape[0]
    u, ph = s[:, :N * U].reshape(R, N, U), p.reshape(R, H, U)
    o.L = float(scale) * np.einsum("rhk,rik->rhi", np.abs(ph), np.abs(u)).reshape(R, -1).max(axis=1)
    lq = np.einsum("rhi,ri->rh", o.lam, np.abs(q))                        # sum_i lam |q_i|
    aw = np.abs(w_raw)
    o.mag_qtot = (aw * lq).sum(1) + np.abs(c)
    if hasattr(o, "dq"):
        ag = np.abs(o.dq_tot)
        o.mag_dq = ag[:, None] * o.a
        o.mag_dw = ag[:, None] * lq
        dev = o.lam * np.abs(q[:, None, :] - o.y[:, :, None])             # lam |q_i - y_h|
        o.mag_dp = (float(scale) * (ag[:, None] * aw)[:, :, None] * np.einsum("rhi,rik->rhk", dev, np.abs(u))).reshape(R, H * U)
        wide = o.lam * (np.abs(q[:, None, :]) + lq[:, :, None])           # lam (|q_i| + sum_j lam_j |q_j|): q_i - y_h taken apart
        o.mag_dp_wide = (float(scale) * (ag[:, None] * aw)[:, :, None] * np.einsum("rhi,rik->rhk", wide, np.abs(u))).reshape(R, H * U)
    if loss is not None:
        o.mag_num = float(np.sum((1.0 - f(loss[3])) * o.mag_td ** 2))
    return o


def twin32(s, p, w_raw, c, q, scale, N, U, H, g=None, loss=None):
    return _contract(np.float32, s, p, w_raw, c, q, scale, N, U, H, g, loss)


def bounds(o):
    """absolute bounds of the fp32 kernel's q_tot, dq, dw_raw, dp against ``o`` = rows(..)"""
    e = U32 * (1.0 + o.L)
    return NS(q_tot=K_QTOT * e * o.mag_qtot, dq=K_DQ * e[:, None] * o.mag_dq, dw_raw=K_DW * e[:, None] * o.mag_dw,
              dp=K_DP * e[:, None] * o.mag_dp, dp_wide=K_DP_WIDE * e[:, None] * o.mag_dp_wide)


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
MAPS = {"2s3z": (5, 24, 4, 120), "3s5z": (8, 27, 4, 216), "MMM2": (10, 32, 4, 322)}        # N, U, H, S
SCALE = float(f32(1.0 / np.sqrt(32.0)))
# (rows, N, U, H, S), each the smallest shape at which something can go wrong; the tile-edge and grid-stride cases depend on the
# kernel's plan and are made by the GPU test
CASES = [(1, 1, 1, 1, 1), (33, 2, 1, 1, 3), (63, 5, 24, 4, 120), (64, 5, 24, 4, 120), (65, 5, 24, 4, 120), (129, 10, 32, 4, 322),
         (257, 8, 27, 4, 216), (64, 16, 64, 8, 1024)]
PLANTED = dict(w_zero=1, p_zero=2, saturated=3)          # rows of a case with U >= 2 and at least four rows


def kernel_case(R, N, U, H, S, seed=0):
    """float32 inputs.  State columns from N U on hold NaN (never read).  By row: 1 has w_raw_0 = 0 exactly and the other heads'
    w_raw negative, 2 has p_0 = 0 (uniform lam), 3 has p_0 = 40 u_0 - head 0's logits spread beyond 100 -; rows % 5 == 4 are padded,
    rows % 7 == 6 terminated."""
    g = np.random.default_rng(9000 + seed)
    s = g.standard_normal((R, S)).astype(f32)
    s[:, N * U:] = np.nan
    p = g.standard_normal((R, H * U)).astype(f32)
    w_raw = g.standard_normal((R, H)).astype(f32)
    c, q_tgt, r, gin = (g.standard_normal(R).astype(f32) for _ in range(4))
    q = g.standard_normal((R, N)).astype(f32)
    rr = np.arange(R)
    if R > 3 and U >= 2:
        w_raw[1] = -np.abs(w_raw[1])
        w_raw[1, 0] = 0.0
        p[2, :U] = 0.0
        p[3, :U] = 40.0 * s[3, :U]
    padded, term = (rr % 5 == 4).astype(f32), (rr % 7 == 6).astype(f32)
    return NS(R=R, N=N, U=U, H=H, S=S, s=s, p=p, w_raw=w_raw, c=c, q=q, g=gin, q_tgt=q_tgt, r=r, term=term, padded=padded,
              scale=SCALE, loss=(q_tgt, r, term, padded, GAMMA))


def oracle_of(c, loss=False):
    return rows(c.s, c.p, c.w_raw, c.c, c.q, c.scale, c.N, c.U, c.H, g=None if loss else c.g, loss=c.loss if loss else None)


# ------------------------------------------------------------------------------------------------ the learner
class State:
    """what QLearner(alg='qatten') owns: agent and mixer, their target copies, the optimizer state (clip_and_step's interface)"""

    def __init__(self, args, agent, mixer, dtype=torch.float64):
        self.args, self.dtype = args, dtype
        f = lambda d: {k: torch.tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True) for k, x in d.items()}
        self.agent, self.mixer = f(agent), f(mixer)
        self.opt, self.opt_step = {}, 0
        self.sync_targets()

    def named_params(self):
        return [("agent." + k, x) for k, x in self.agent.items()] + [("mixer." + k, x) for k, x in self.mixer.items()]

    def sync_targets(self):
        self.target_agent = {k: x.detach().clone() for k, x in self.agent.items()}
        self.target_mixer = {k: x.detach().clone() for k, x in self.mixer.items()}


def forward(state, batch, lam=None):
    """QLearner's loss with the Qatten mixer: oracle.learners.q_forward's schedule (Q1: the double-Q pass continues from the eval
    net's final hidden state; Q2: max_episode_len) in state.dtype.  lam: TD(lambda) returns of q_tot_target as the targets"""
    args, dt = state.args, state.dtype
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}
    B, N, H, S = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim, args.state_shape
    la, ru = args.last_action, args.reuse_network
    avail_next, u_onehot = bt["avail_u_next"], bt["u_onehot"]
    h0 = torch.zeros(B * N, H, dtype=dt)
    q_evals, _, h_last = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(u_onehot), h0, la, ru)
    q_chosen = torch.gather(q_evals, 3, bt["u"]).squeeze(3)
    with torch.no_grad():
        q_tgt = nets.agent_unroll(state.target_agent, bt["o_next"], u_onehot, h0, la, ru)[0].clone()
        q_tgt[avail_next == 0.0] = learners.MASK_BIG
        if args.double_q:
            q_en = nets.agent_unroll(state.agent, bt["o_next"], u_onehot, h_last.detach(), la, ru)[0].clone()
            q_en[avail_next == 0] = learners.MASK_BIG
            q_tgt_chosen = torch.gather(q_tgt, 3, q_en.argmax(dim=3, keepdim=True)).squeeze(3)
        else:
            q_tgt_chosen = q_tgt.max(dim=3)[0]
        q_tot_tgt = mix(state.target_mixer, q_tgt_chosen.reshape(B * T, N), bt["s_next"].reshape(B * T, S), args).reshape(B, T)
    q_tot = mix(state.mixer, q_chosen.reshape(B * T, N), bt["s"].reshape(B * T, S), args).reshape(B, T)
    r, term, padded = (bt[k].reshape(B, T) for k in ("r", "terminated", "padded"))
    m = 1.0 - padded
    if lam is None:
        targets = r + args.gamma * q_tot_tgt * (1 - term)
    else:
        targets = torch.tensor(tl.returns(q_tot_tgt.double().numpy(), r.double().numpy(), term.double().numpy(),
                                          padded.double().numpy(), args.gamma, lam), dtype=dt)
    mtd = m * (targets.detach() - q_tot)
    loss = (mtd ** 2).sum() / m.sum()
    return loss, dict(T=T, q_evals=q_evals, q_tot=q_tot, q_tot_target=q_tot_tgt, loss=loss, num=(mtd ** 2).sum(), den=m.sum())


def train(state, batch, train_step, lam=None):
    """one QLearner.train call: (loss float, gradients before the clip, intermediates); Q6: the target sync rule"""
    loss, inter = forward(state, batch, lam)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter


# 2s3z-shaped, the batch shape of the IQL learner test: B = 4; episode 0 ends at the window's last step, episode 2 never terminates
LEARNER_B, LEARNER_T, LEARNER_LENGTHS, AGENT_SEED, MIXER_SEED = 4, 6, [6, 3, -1, 4], 11, 12
LEARNER_TOL = (1e-4, 1e-3, 1e-3)      # tests/test_gpu_learners.py's
# name -> (args overrides, td_lambda, seed of update 0's batch; update i draws seed + i).  RMSprop's first step moves a parameter by
# lr g / (0.1 |g| + 1e-8): where |g| is near 1e-7 the rounding of g decides the step, and whether a batch has such entries is a
# property of the batch, not of the arithmetic under test.  A seed is acceptable only if this oracle run in float32 passes LEARNER_TOL
# against its float64 self; the seeds here are chosen ON THE CPU as the best of 100, 110, .. 490 under float32_fraction's three
# rounding draws (0.283, 0.352, 0.304 of the bound; tests/test_qatten_oracle_cpu.py asserts at most a half)
LEARNER_CASES = {"double_q": ({}, None, 120), "max": (dict(double_q=False), None, 220), "lam0.8": ({}, 0.8, 130)}


def learner_case(name, dtype=torch.float64, **more):
    """(args, State, batch(i), td_lambda) of a learner case"""
    over, lam, seed0 = LEARNER_CASES[name]
    kw = dict(over, **more)
    if lam is not None:
        kw["td_lambda"] = lam
    args = seeded.make_args("2s3z", "qatten", episode_limit=LEARNER_T, **kw)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=AGENT_SEED)
    mixer = seeded.seeded_state(param_shapes(args), seed=MIXER_SEED)
    batch = lambda i: seeded.make_batch(args, LEARNER_B, seed=seed0 + i, lengths=LEARNER_LENGTHS)
    return args, State(args, agent, mixer, dtype), batch, lam


def float32_fraction(name, draws=3):
    """the worst |float32 oracle - float64 oracle| of a parameter over the case's three updates, as a fraction of LEARNER_TOL's bound.
    Over ``draws`` float32 runs: run k starts from the parameters nudged by k ulp (p (1 + k 2^-23)) - another draw of the roundings,
    as another summation order is, so that one lucky float32 run does not pass a batch whose RMSprop steps hang on them"""
    worst = 0.0
    for k in range(draws):
        _, a, batch, lam = learner_case(name, torch.float64)
        _, b, _, _ = learner_case(name, torch.float32)
        with torch.no_grad():
            for _, x in b.named_params():
                x.mul_(1.0 + k * 2.0 ** -23)
        b.sync_targets()
        for i, tol in enumerate(LEARNER_TOL):
            train(a, learners.clone_batch(batch(i)), i, lam=lam)
            train(b, learners.clone_batch(batch(i)), i, lam=lam)
            for (_, x), (_, y) in zip(a.named_params(), b.named_params()):
                ref = x.detach().numpy()
                worst = max(worst, float(np.abs(y.detach().double().numpy() - ref).max() / (tol * np.abs(ref).max() + 1e-7)))
    return worst
