"""MAVEN in float64 (TEST INFRASTRUCTURE, CPU), written from the definition in DESIGN section 9 / include/marl_hip.h, not from the
kernels.

* ``noise_draw``          the episode noise index, the counter hash restated on Python integers
* ``head_term`` / ``hyper_layer_q``   the head as a sum of two table rows, and the literal Linear(K + N -> A H) formulation it equals
* ``mi_rows``             the MI pass under torch autograd: p, ce, the hit, lambda sum m ce
* ``head_case`` / ``mi_case``   seeded fp32 inputs of the kernel tests (tests/test_gpu_maven.py) and their float64 results
* ``State`` / ``forward`` / ``train``   what MAVENLearner owns and one ``train`` call over oracle.nets' agent unroll and QMIX mixer in
                          ``dtype`` (float64, or float32 for the yardstick): quirks Q1, Q2, Q6 as oracle.learners.q_forward has them
* ``learner_case``        the learner cases; ``conditioning`` what makes a case usable at all (below)

The discontinuities.  The double-Q action hangs on an argmax, the diagnostic hit on another, and the discriminator's ReLU on the sign
of its pre-activations: a float32 result that lands on the other side picks another action or switches a unit's gradient, and no
parity bound survives that.  So a learner case is acceptable only if, at every update of it, every argmax on a live row is decided by
at least MARGIN = 1e-3 times the largest |value| compared, no ReLU pre-activation of a live step is within RELU_EPS = 1e-5 of 0, every
noise index occurs in the batch where K <= B, and the float32 oracle makes the same selections as the float64 one.  The seeds in
LEARNER_CASES were searched ON THE CPU (tests/test_maven_oracle_cpu.py asserts all of this on the oracle alone)."""
import types

import numpy as np
import torch

from oracle import learners, nets, seeded
import td_lambda_oracle as tl

NS = types.SimpleNamespace
f32 = np.float32
MASK_BIG = learners.MASK_BIG
MARGIN = 1e-3
RELU_EPS = 1e-5
H = 64
D = 64
ST_MAVEN = 24
TABLES = ("noise_w", "id_w", "noise_b", "id_b")


# ------------------------------------------------------------------------------------------------ the noise draw
def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hkey(seed, stream, env, t, idx):
    """csrc/synth_env.h: hkey, on Python integers (every sum wraps at 32 bits)"""
    h = _mix32(seed + stream * 0x9E3779B1)
    h = _mix32(h + env * 0x85EBCA77 + 1)
    h = _mix32(h + t * 0xC2B2AE3D + 2)
    return _mix32(h + idx * 0x27D4EB2F + 3)


def noise_draw(rseed, env0, tg0, K, E):
    """noise (E,) int32: hkey(rseed, stream 24, env0 + e, tg0, 0) % K"""
    return np.array([hkey(rseed & 0xFFFFFFFF, ST_MAVEN, (env0 + e) & 0xFFFFFFFF, tg0 & 0xFFFFFFFF, 0) % K for e in range(E)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the head
def table_shapes(K, N, A):
    return [("noise_w", (K, A, H)), ("id_w", (N, A, H)), ("noise_b", (K, A)), ("id_b", (N, A))]


def seeded_tables(K, N, A, seed, scale=1.0):
    """U(+-1/sqrt(K + N)), the range nn.Linear(K + N, .) gives its columns, from a numpy stream"""
    g = np.random.default_rng(seed)
    b = scale / np.sqrt(K + N)
    return {k: g.uniform(-b, b, size=s).astype(f32) for k, s in table_shapes(K, N, A)}


def head_term(P, hs, noise, prefix=""):
    """(noise_w[k_b] + id_w[n]) h + noise_b[k_b] + id_b[n] over hs (B,T,N,H) for noise (B,) integers; an episode whose index is
    outside [0, K) gets zeros (and its hs rows are not looked at)"""
    nw, iw, nb, ib = (P[prefix + k] for k in TABLES)
    K = nw.shape[0]
    noise = torch.as_tensor(np.asarray(noise), dtype=torch.long)
    ok = (noise >= 0) & (noise < K)
    k = torch.where(ok, noise, torch.zeros_like(noise))
    hs = torch.where(ok[:, None, None, None], hs, torch.zeros((), dtype=hs.dtype))
    W = nw[k][:, None] + iw[None]                          # (B, N, A, H)
    b = nb[k][:, None] + ib[None]                          # (B, N, A)
    term = torch.einsum("bnah,btnh->btna", W, hs) + b[:, None]
    return term * ok[:, None, None, None].to(hs.dtype)


def hyper_layer_q(Wl, bl, fc2_w, fc2_b, hs, noise, K):
    """The literal formulation: z = [one-hot(k_b) | one-hot(n)], M = (Wl z).view(A, H) + fc2_w, c = bl z + fc2_b, q' = M h + c.  Wl
    (A H, K + N) and bl (A, K + N) are the weights of the hyper-layers Linear(K + N -> A H) and Linear(K + N -> A), whose biases are
    fc2's weight and bias"""
    B, T, N, _ = hs.shape
    A = fc2_w.shape[0]
    z = torch.zeros(B, N, K + N, dtype=hs.dtype)
    z[torch.arange(B)[:, None], torch.arange(N)[None], torch.as_tensor(np.asarray(noise), dtype=torch.long)[:, None].expand(B, N)] = 1.0
    z[:, torch.arange(N), K + torch.arange(N)] = 1.0
    M = (z @ Wl.T).view(B, N, A, H) + fc2_w
    c = z @ bl.T + fc2_b
    return torch.einsum("bnah,btnh->btna", M, hs) + c[:, None]


def tables_of_hyper_layer(Wl, bl, K, N, A):
    """the four tables as the columns of the two layers"""
    cols = lambda w, lo, hi, *shape: w[:, lo:hi].T.reshape(hi - lo, *shape)
    return {"noise_w": cols(Wl, 0, K, A, H), "id_w": cols(Wl, K, K + N, A, H), "noise_b": cols(bl, 0, K, A), "id_b": cols(bl, K, K + N, A)}


# (B, T, N, A, K): the issue's six
HEAD_SHAPES = [(1, 1, 1, 1, 1), (1, 15, 2, 3, 3), (3, 17, 5, 11, 16), (2, 33, 10, 18, 16), (1, 2, 16, 32, 32), (64, 1, 5, 11, 16)]


def head_case(B, T, N, A, K, seed=0):
    """float32 inputs of the head kernels.  With B >= 2 the last episode's noise is out of range (K, or -1 in odd cases) and its hs rows
    hold NaN; episode 0's value occurs nowhere else (K >= 2 and B >= 2).  The sparse pairs hold a few -1 (no entry)."""
    g = np.random.default_rng(9000 + 10 * seed + B + T + N + A + K)
    hs = g.standard_normal((B, T, N, H)).astype(f32)
    q = g.standard_normal((B, T, N, A)).astype(f32)
    noise = g.integers(0, K, size=B).astype(np.int32)
    if B >= 2 and K >= 2:
        noise[0] = K - 1
        noise[1:] = g.integers(0, K - 1, size=B - 1)
    skipped = np.zeros(B, bool)
    if B >= 2:
        noise[-1] = K if (B + T) % 2 == 0 else -1
        skipped[-1] = True
        hs[-1] = np.nan
    tables = seeded_tables(K, N, A, seed=31 + seed, scale=3.0)
    dq_idx = g.integers(0, A, size=(B, T, N)).astype(np.int32)
    dq_idx[g.random((B, T, N)) < 0.1] = -1
    dq_val = g.standard_normal((B, T, N)).astype(f32)
    dq_dense = g.standard_normal((B, T, N, A)).astype(f32)
    base = {k: g.standard_normal(s).astype(f32) for k, s in table_shapes(K, N, A)}
    return NS(B=B, T=T, N=N, A=A, K=K, hs=hs, q=q, noise=noise, skipped=skipped, tables=tables, dq_idx=dq_idx, dq_val=dq_val,
              dq_dense=dq_dense, base=base)


def head_oracle(c, dense=True):
    """float64: q_out, g, dhs and the table gradients (without the base)"""
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c.tables.items()}
    hs = torch.tensor(np.nan_to_num(c.hs), dtype=torch.float64, requires_grad=True)
    term = head_term(P, hs, c.noise)
    g = np.zeros((c.B, c.T, c.N, c.A))
    if dense:
        g += c.dq_dense.astype(np.float64)
    b, t, n = np.nonzero(c.dq_idx >= 0)
    g[b, t, n, c.dq_idx[b, t, n]] += c.dq_val[b, t, n].astype(np.float64)
    grads = torch.autograd.grad((term * torch.tensor(g)).sum(), [hs] + [P[k] for k in TABLES])
    return NS(q_out=c.q.astype(np.float64) + term.detach().numpy(), g=g, dhs=grads[0].numpy(),
              grads={k: x.numpy() for k, x in zip(TABLES, grads[1:])})


# ------------------------------------------------------------------------------------------------ the MI pass
def disc_shapes(N, A, S, K):
    return [("l1.weight", (D, N * A + S)), ("l1.bias", (D,)), ("l2.weight", (K, D)), ("l2.bias", (K,))]


def mi_rows(Dp, q, avail, state, noise, padded, lam, prefix=""):
    """The MI pass in q's dtype under autograd.  q, avail (B,T,N,A), state (B,T,S), noise (B,), padded (B,T); the inputs of a padded step
    are never looked at (they may hold NaN).  Returns ce (B,T; 0 where padded), p, the pre-activations, the logits, the hit (B,T bool),
    the live mask and ``loss`` = lam sum m ce"""
    B, T, N, A = q.shape
    dt = q.dtype
    m = 1.0 - padded
    live = m != 0
    z = torch.zeros((), dtype=dt)
    qc = torch.where(live[..., None, None], q, z)
    av = torch.where(live[..., None, None], avail, torch.ones((), dtype=dt)) != 0
    sc = torch.where(live[..., None], state, z)
    any_av = av.any(dim=3, keepdim=True)
    masked = torch.where(av, qc, torch.full((), -float("inf"), dtype=dt))
    masked = torch.where(any_av, masked, z)
    p = torch.softmax(masked, dim=3)
    p = torch.where(av & any_av, p, z)
    x = torch.cat([p.reshape(B, T, N * A), sc], dim=2)
    pre = x @ Dp[prefix + "l1.weight"].T + Dp[prefix + "l1.bias"]
    logits = torch.relu(pre) @ Dp[prefix + "l2.weight"].T + Dp[prefix + "l2.bias"]
    kb = torch.as_tensor(np.asarray(noise), dtype=torch.long)[:, None].expand(B, T)
    ce = (torch.logsumexp(logits, dim=2) - logits.gather(2, kb[..., None]).squeeze(2)) * live
    hit = (logits.argmax(dim=2) == kb) & live
    return NS(ce=ce, p=p, pre=pre, logits=logits, hit=hit, live=live, m=m, loss=lam * (m * ce).sum(), kb=kb)


# (B, T, N, A, S, K): the issue's five
MI_SHAPES = [(1, 1, 1, 1, 1, 1), (2, 7, 2, 3, 5, 3), (3, 17, 5, 11, 120, 16), (2, 9, 10, 18, 322, 16), (1, 3, 16, 32, 40, 32)]


def mi_case(B, T, N, A, S, K, seed=0):
    """float32 inputs of marl_maven_mi as a replay sample would hand them: availability and state lie in a store of B + 2 episodes of
    T + 1 slots (state rows of S + 3 floats: state_ld > S) and are read through a permuted episode map.  Lengths: episode 0 full, the
    others shorter (padded tails), the last one of B >= 2 all padded; q, avail and state of padded steps hold NaN, and so does
    everything of the store the batch does not map.  Live row (0, 0, 0) has one available action"""
    g = np.random.default_rng(9500 + 10 * seed + B + T + N + A + S + K)
    E, Ts, ld = B + 2, T + 1, S + 3
    q = (2.0 * g.standard_normal((B, T, N, A))).astype(f32)
    avail = (g.random((B, T, N, A)) < 0.7).astype(f32)
    avail[..., 0] = 1.0
    avail[0, 0, 0] = 0.0
    avail[0, 0, 0, A - 1] = 1.0
    state = g.standard_normal((B, T, S)).astype(f32)
    lengths = [T] + [int(x) for x in g.integers(1, T + 1, size=B - 1)]
    if B >= 2:
        lengths[-1] = 0
    padded = np.array([[0.0 if t < L else 1.0 for t in range(T)] for L in lengths], dtype=f32)
    dead = padded == 1
    noise = (g.permutation(B) % K).astype(np.int32)
    ep_map = np.arange(E - 1, E - 1 - B, -1).astype(np.int32)          # never the identity, never ascending
    q[dead], avail[dead], state[dead] = np.nan, np.nan, np.nan
    avail_store = np.full((E, Ts, N, A), np.nan, f32)
    state_store = np.full((E, Ts, ld), np.nan, f32)
    avail_store[ep_map, :T] = avail
    state_store[ep_map, :T, :S] = state
    disc = seeded.seeded_state(disc_shapes(N, A, S, K), seed=77 + seed)
    base = {k: g.standard_normal(s).astype(f32) for k, s in disc_shapes(N, A, S, K)}
    return NS(B=B, T=T, N=N, A=A, S=S, K=K, q=q, avail=avail, state=state, padded=padded, noise=noise, ep_map=ep_map,
              avail_store=avail_store, state_store=state_store, ld=ld, Ts=Ts, disc=disc, base=base, lengths=lengths,
              stats_base=np.array([3.0, 5.0], f32))


def mi_oracle(c, lam):
    """float64: ce, the two sums, dq_dense and the discriminator's gradients (without the bases)"""
    t = lambda x: torch.tensor(np.nan_to_num(x), dtype=torch.float64)
    Dp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c.disc.items()}
    q = t(c.q).requires_grad_(True)
    r = mi_rows(Dp, q, t(c.avail), t(c.state), c.noise, torch.tensor(c.padded, dtype=torch.float64), lam)
    names = list(Dp)
    grads = torch.autograd.grad(r.loss, [q] + [Dp[k] for k in names])
    return NS(ce=r.ce.detach().numpy(), stats=np.array([float((r.m * r.ce).sum().detach()), float((r.m * r.hit).sum())]),
              dq_dense=grads[0].numpy(), grads={k: x.numpy() for k, x in zip(names, grads[1:])}, p=r.p.detach().numpy(),
              pre=r.pre.detach().numpy(), logits=r.logits.detach().numpy(), live=r.live.numpy())


# ------------------------------------------------------------------------------------------------ the learner
def agent_shapes(args):
    """MavenAgent's state_dict, in order: RNNQNet's, then the four tables"""
    return seeded.agent_param_shapes(args) + [("maven." + k, s) for k, s in table_shapes(args.noise_dim, args.n_agents, args.n_actions)]


class State:
    """what MAVENLearner owns: the agent (with its tables), the monotonic mixer and the discriminator, target copies of the first two,
    the optimizer state (clip_and_step's interface).  The parameter order is the learner's flat buffer's"""
    NETS = ("agent", "mixer", "discrim")

    def __init__(self, args, agent, mixer, discrim, dtype=torch.float64):
        self.args, self.dtype = args, dtype
        f = lambda d: {k: torch.tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True) for k, x in d.items()}
        self.agent, self.mixer, self.discrim = f(agent), f(mixer), f(discrim)
        self.opt, self.opt_step = {}, 0
        self.sync_targets()

    def named_params(self):
        return [(n + "." + k, x) for n in self.NETS for k, x in getattr(self, n).items()]

    def sync_targets(self):
        for n in ("agent", "mixer"):
            setattr(self, "target_" + n, {k: x.detach().clone() for k, x in getattr(self, n).items()})


def _gap(qm, live_rows):
    """(smallest top-two gap over the rows ``live_rows`` selects, the largest finite |value| compared there)"""
    sel = qm[live_rows]
    if sel.numel() == 0:
        return float("inf"), 0.0
    real = sel > MASK_BIG / 2
    scale = float((sel.abs() * real).max())
    if sel.shape[-1] < 2:
        return float("inf"), scale
    top = sel.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min()), scale


def forward(state, batch, noise, lam=None):
    """MAVENLearner's loss in state.dtype.  ``noise`` (B,) integers.  Returns (loss, intermediates): T, the Qs with the head's term, hs,
    q_tot, q_tot_target, ce, dq_dense (the gradient of lambda_mi sum m ce on q'), the four statistics, the double-Q actions, the hit
    flags, ``margins``: name -> (smallest gap, largest |value| compared) of every argmax, and ``relu``: the smallest |pre-activation|
    of the discriminator on a live step"""
    args, dt = state.args, state.dtype
    lam_mi = float(args.lambda_mi)
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}
    B, N, S = bt["o"].shape[0], args.n_agents, args.state_shape
    la, ru = args.last_action, args.reuse_network
    u, u_onehot, avail, avail_next = bt["u"], bt["u_onehot"], bt["avail_u"], bt["avail_u_next"]
    r, term, padded = (bt[k].reshape(B, T) for k in ("r", "terminated", "padded"))
    m = 1.0 - padded
    live = m != 0
    h0 = torch.zeros(B * N, H, dtype=dt)
    q0, hs, h_last = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(u_onehot), h0, la, ru)
    q_evals = q0 + head_term(state.agent, hs, noise, "maven.")
    q_chosen = torch.gather(q_evals, 3, u).squeeze(3)
    margins = {}
    with torch.no_grad():
        q_t0, hs_t, _ = nets.agent_unroll(state.target_agent, bt["o_next"], u_onehot, h0, la, ru)
        q_targets = q_t0 + head_term(state.target_agent, hs_t, noise, "maven.")
        q_tgt = q_targets.clone()
        q_tgt[avail_next == 0] = MASK_BIG
        rows = live[:, :, None].expand(B, T, N)
        if args.double_q:
            q_e0, hs_e, _ = nets.agent_unroll(state.agent, bt["o_next"], u_onehot, h_last.detach(), la, ru)      # quirk Q1
            q_en = q_e0 + head_term(state.agent, hs_e, noise, "maven.")
            q_en[avail_next == 0] = MASK_BIG
            cur_max = q_en.argmax(dim=3, keepdim=True)
            margins["cur_max"] = _gap(q_en, rows)
            q_tgt_chosen = torch.gather(q_tgt, 3, cur_max).squeeze(3)
        else:
            cur_max = q_tgt.argmax(dim=3, keepdim=True)
            margins["cur_max"] = _gap(q_tgt, rows)
            q_tgt_chosen = q_tgt.max(dim=3)[0]
        q_tot_tgt = nets.qmix(state.target_mixer, q_tgt_chosen, bt["s_next"], args).reshape(B, T)
    q_tot = nets.qmix(state.mixer, q_chosen, bt["s"], args).reshape(B, T)
    if lam is None:
        y = r + args.gamma * q_tot_tgt * (1 - term)
    else:
        npdt = np.float64 if dt == torch.float64 else np.float32
        y = torch.tensor(tl.returns(q_tot_tgt.numpy(), r.numpy(), term.numpy(), padded.numpy(), args.gamma, lam, dtype=npdt), dtype=dt)
    mtd = m * (y.detach() - q_tot)
    num, den = (mtd ** 2).sum(), m.sum()
    mi = mi_rows(state.discrim, q_evals, avail, bt["s"], noise, padded, lam_mi)
    ce_sum, hits = (m * mi.ce).sum(), (m * mi.hit).sum()
    loss = (num + lam_mi * ce_sum) / den
    dq_dense = torch.autograd.grad(mi.loss, q_evals, retain_graph=True)[0] if lam_mi > 0 else torch.zeros_like(q_evals)
    margins["hit"] = _gap(mi.logits.detach(), live)
    relu = float(mi.pre.detach().abs()[live].min()) if bool(live.any()) else float("inf")
    return loss, dict(T=T, q_evals=q_evals, q_targets=q_targets, hs=hs, q_tot=q_tot, q_tot_target=q_tot_tgt, ce=mi.ce, dq_dense=dq_dense,
                      loss=loss, num=num, den=den, ce_sum=ce_sum, hits=hits, cur_max=cur_max.squeeze(3), hit=mi.hit, live=live,
                      margins=margins, relu=relu)


def train(state, batch, noise, train_step, lam=None):
    """one MAVENLearner.train call: (loss float, gradients before the clip, intermediates); Q6: the target sync rule"""
    loss, inter = forward(state, batch, noise, lam)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter


AGENT_SEED, MIXER_SEED, DISC_SEED, TABLE_SEED = 11, 12, 15, 16
LEARNER_TOL = (1e-4, 1e-3)            # tests/test_gpu_learners.py's, for the two updates
# name -> (shape, B, T, lengths, noise_dim, lambda_mi, td_lambda, seed of update 0's batch; update i draws seed + i).  Episode 0 ends at
# the window's last step; a length of -1 never terminates.  Seeds searched on the CPU for ``conditioning``
LEARNER_CASES = {
    "2s3z": ("2s3z", 4, 6, [6, 3, -1, 4], 16, 0.001, None, 122),
    "MMM2_lam0.8": ("MMM2", 5, 5, [5, 2, -1, 3, 4], 16, 0.001, 0.8, 100),
    "matrix_mi0": ("matrix", 6, 1, [1, 1, 1, 1, 1, 1], 3, 0.0, None, 100),
}
# (case, update, tensor) -> the float32 oracle's worst absolute error over ``conditioning``'s twelve draws where it passes a quarter of
# LEARNER_TOL's bound, from the CPU run alone (tests/wqmix_oracle.py: F32_EXCEPTIONS has the reasoning: RMSprop's first step moves a
# parameter by lr g / (0.1 |g| + 1e-8), so where |g| is near 1e-7 the rounding of g decides the step).  The GPU test holds these tensors
# to four times the figure; every gradient of the first update, and every tensor not listed, stays on LEARNER_TOL
F32_EXCEPTIONS = {
    ("2s3z", 0, "param agent.rnn.weight_ih"): 1.51e-05,      # 1.16 of the bound
    ("2s3z", 0, "param agent.rnn.weight_hh"): 1.36e-05,      # 1.04 of the bound
    ("2s3z", 0, "param mixer.hyper_w1.weight"): 5.11e-06,      # 0.53 of the bound
    ("2s3z", 0, "param mixer.hyper_w2.weight"): 4.62e-06,      # 0.48 of the bound
    ("MMM2_lam0.8", 0, "param agent.fc1.weight"): 2.87e-05,      # 3.77 of the bound
    ("MMM2_lam0.8", 0, "param agent.rnn.weight_ih"): 2.34e-05,      # 1.78 of the bound
    ("MMM2_lam0.8", 0, "param agent.rnn.weight_hh"): 7.80e-05,      # 5.95 of the bound
    ("MMM2_lam0.8", 0, "param agent.maven.noise_w"): 6.12e-06,      # 0.30 of the bound
    ("MMM2_lam0.8", 0, "param mixer.hyper_w1.weight"): 4.26e-04,      # 69.04 of the bound
    ("MMM2_lam0.8", 0, "param mixer.hyper_b2.0.weight"): 8.33e-06,      # 1.35 of the bound
    ("MMM2_lam0.8", 1, "param agent.fc1.weight"): 2.87e-05,      # 0.36 of the bound
    ("MMM2_lam0.8", 1, "param agent.rnn.weight_hh"): 7.80e-05,      # 0.58 of the bound
    ("MMM2_lam0.8", 1, "param mixer.hyper_w1.weight"): 4.26e-04,      # 6.48 of the bound
    ("MMM2_lam0.8", 1, "param mixer.hyper_w2.weight"): 2.24e-04,      # 3.42 of the bound
}


def case_noise(name, i):
    """update i's noise indices: a permutation of b % K (every index occurs where K <= B), seeded"""
    shape, B, T, lengths, K, lam_mi, lam, seed0 = LEARNER_CASES[name]
    return (np.random.default_rng(5000 + seed0 + i).permutation(B) % K).astype(np.int32)


def learner_case(name, dtype=torch.float64, zero_tables=False, **more):
    """(args, State, batch(i), noise(i), td_lambda) of a learner case"""
    shape, B, T, lengths, K, lam_mi, lam, seed0 = LEARNER_CASES[name]
    kw = dict(noise_dim=K, lambda_mi=lam_mi, maven_discrim_dim=D)
    kw.update(more)
    if lam is not None:
        kw["td_lambda"] = lam
    args = seeded.make_args(shape, "maven", episode_limit=T, **kw)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=AGENT_SEED)
    tables = seeded_tables(K, args.n_agents, args.n_actions, seed=TABLE_SEED)
    agent.update({"maven." + k: (np.zeros_like(v) if zero_tables else v) for k, v in tables.items()})
    qargs = seeded.make_args(shape, "qmix", episode_limit=T)
    mixer = seeded.seeded_state(seeded.qmix_param_shapes(qargs), seed=MIXER_SEED)
    discrim = seeded.seeded_state(disc_shapes(args.n_agents, args.n_actions, args.state_shape, K), seed=DISC_SEED)
    batch = lambda i: seeded.make_batch(args, B, seed=seed0 + i, lengths=lengths)
    return args, State(args, agent, mixer, discrim, dtype), batch, (lambda i: case_noise(name, i)), lam


def conditioning(name, draws=12):
    """Runs the case's two updates in float64 and in float32 side by side.  Returns per update: the margins as fractions
    gap / (MARGIN * scale) (>= 1 wanted), the smallest live |ReLU pre-activation| (>= RELU_EPS wanted), whether every noise index occurs
    (where K <= B), whether float32 took the same double-Q actions and hits on every live row, and per tensor the float32 oracle's worst
    error, also as a fraction of LEARNER_TOL's bound (<= 0.25 wanted).  Over ``draws`` float32 runs: run k starts from the parameters
    nudged by k ulp (p (1 + k 2^-23)) - another draw of the roundings (tests/wqmix_oracle.py: conditioning)"""
    _, a, batch, noise, lam = learner_case(name, torch.float64)
    bs = [learner_case(name, torch.float32)[1] for _ in range(draws)]
    for k, b in enumerate(bs):
        with torch.no_grad():
            for _, x in b.named_params():
                x.mul_(1.0 + k * 2.0 ** -23)
        b.sync_targets()
    K = a.args.noise_dim
    out = []
    for i, tol in enumerate(LEARNER_TOL):
        bt, nz = batch(i), noise(i)
        la, ga, ia = train(a, learners.clone_batch(bt), nz, i, lam=lam)
        live = ia["live"]
        same, frac, err = True, {}, {}

        def worst(key, got, ref, scale):
            e = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
            err[key] = max(err.get(key, 0.0), e)
            frac[key] = err[key] / (tol * scale + 1e-7)
        for b in bs:
            lb, gb, ib = train(b, learners.clone_batch(bt), nz, i, lam=lam)
            same = same and bool((ia["cur_max"][live] == ib["cur_max"][live]).all()) and bool((ia["hit"] == ib["hit"]).all())
            worst("loss", lb, la, abs(la))
            for k2 in ("q_evals", "q_targets", "hs", "q_tot", "q_tot_target", "ce", "dq_dense"):
                ref = ia[k2].detach().numpy()
                worst(k2, ib[k2].detach().numpy(), ref, np.abs(ref).max())
            for (n, x), (_, y) in zip(a.named_params(), b.named_params()):
                ref = x.detach().numpy()
                worst("param " + n, y.detach().numpy(), ref, np.abs(ref).max())
                if i == 0:
                    ref = np.zeros(x.shape) if ga[n] is None else ga[n].numpy()
                    worst("grad " + n, np.zeros(x.shape) if gb[n] is None else gb[n].numpy(), ref, np.abs(ref).max())
        out.append(NS(margins={k: g / (MARGIN * sc) if sc > 0 else float("inf") for k, (g, sc) in ia["margins"].items()},
                      relu=ia["relu"], all_noise=(K > len(nz)) or (set(nz.tolist()) == set(range(K))), same=same, frac=frac, err=err))
    return out
