"""Independent Q-learning in float64 torch (TEST INFRASTRUCTURE, CPU): a restatement of the definition in include/marl_hip.h
(csrc/iql.hip) and algorithm/iql.py, written from the definition, not from the kernel.

* ``select`` / ``rows``      the selection, the targets, the loss and the gradient over the R = B T N agent rows; the gradient comes
                             from autograd through ``gather`` and, beside it, in closed form
* ``State`` / ``forward`` / ``train``   what IQLLearner owns and one ``train`` call over oracle.nets' agent unroll, in ``dtype``
* ``kernel_case``            the float32 inputs of the kernel tests, with the edges the cases are named for

Rows r = (b T + t) N + i, m = 1 - padded[b, t].  A row with m = 0 contributes nothing, its per-row outputs are exact zeros and its row
operands are never looked at (they may hold NaN)."""
import types

import numpy as np
import torch

from oracle import learners, nets, seeded
import td_lambda_oracle as tl

NS = types.SimpleNamespace
MASK_BIG = -9999999.0           # exact in fp32
f32 = np.float32
GAMMA = float(f32(0.99))        # scalars reach the kernels as C floats: both sides get the rounded value
U = 2.0 ** -24


def _t(x, dtype=torch.float64):
    return x.to(dtype) if torch.is_tensor(x) else torch.tensor(np.asarray(x), dtype=dtype)


def select(q_sel, q_tgt, avail_next, mask_val=MASK_BIG):
    """q_next (R) and a* (R): the first-index argmax of the masked q_sel (q_sel None: of the masked q_tgt itself - its masked max),
    and the masked q_tgt there.  avail_next None: everything is available."""
    q_tgt = _t(q_tgt)
    mask = (lambda x: x) if avail_next is None else (lambda x: torch.where(_t(avail_next) == 0, torch.full_like(x, mask_val), x))
    tgt = mask(q_tgt)
    sel = tgt if q_sel is None else mask(_t(q_sel))
    arg = torch.tensor(np.argmax(sel.numpy(), axis=1))          # numpy's argmax returns the first maximum
    return tgt.gather(1, arg[:, None]).squeeze(1), arg


def rows(q, u, q_sel, q_tgt, avail_next, r, term, padded, gamma, N, ret=None, mask_val=MASK_BIG):
    """The definition over the rows.  q, q_sel, q_tgt, avail_next (R, A); u (R) integers; r, term, padded (B T); ret None or (R) in
    ROW order (the caller transposes a (B, N, T) array).  Returns q_taken, q_next, y, td (R; zeros where m = 0), num = sum m td^2,
    den = N sum m, loss, dq (R, A) = autograd of num by q, dq_val (R) = - 2 m td (closed form) and the magnitude of td's terms."""
    q = _t(q).clone()
    R, A = q.shape
    u = torch.as_tensor(np.asarray(u), dtype=torch.long).reshape(R)
    m = (1.0 - _t(padded)).reshape(-1).repeat_interleave(N)
    live = m != 0
    clean = lambda x: None if x is None else torch.where(live[:, None], _t(x), torch.zeros(R, A, dtype=torch.float64))
    zero = torch.zeros(R, dtype=torch.float64)
    qz = clean(q).requires_grad_(True)
    q_taken = qz.gather(1, u[:, None]).squeeze(1)
    per = lambda x: _t(x).reshape(-1).repeat_interleave(N)
    if ret is None:
        q_next, _ = select(clean(q_sel), clean(q_tgt), clean(avail_next) if avail_next is not None else None, mask_val)
        q_next = torch.where(live, q_next, zero)
        boot = gamma * (1.0 - per(term)) * q_next
        y = torch.where(live, per(r) + boot, zero)
        mag = torch.where(live, per(r).abs() + boot.abs() + q_taken.detach().abs(), zero)
    else:
        q_next = zero
        y = torch.where(live, _t(ret).reshape(R), zero)
        mag = torch.where(live, y.abs() + q_taken.detach().abs(), zero)
    td = torch.where(live, y.detach() - q_taken, zero)
    num = (m * td ** 2).sum()
    den = m.sum()                                      # over the rows: N sum over the steps
    dq, = torch.autograd.grad(num, qz)
    return NS(q_taken=torch.where(live, q_taken.detach(), zero), q_next=q_next, y=y, td=td.detach(), num=num.detach(), den=den,
              loss=(num / den).detach() if float(den) > 0 else None, dq=dq, dq_val=-2.0 * m * td.detach(), mag=mag, m=m, live=live,
              mag_num=(m * mag ** 2).sum())


def lambda_returns(q_next_rows, r, term, padded, gamma, lam, B, T, N):
    """G in ROW order (R): the lambda-returns of every agent's own sequence (td_lambda_oracle.returns on B N sequences, r / term /
    padded expanded over the agents); also returned in (B, N, T) layout"""
    qn = _t(q_next_rows).reshape(B, T, N).permute(0, 2, 1).reshape(B * N, T).numpy()
    per = lambda a: np.repeat(np.asarray(_t(a).reshape(B, T).numpy())[:, None, :], N, axis=1).reshape(B * N, T)
    G = torch.tensor(tl.returns(qn, per(r), per(term), per(padded), gamma, lam)).reshape(B, N, T)
    return G.permute(0, 2, 1).reshape(-1), G


# ------------------------------------------------------------------------------------------------ the learner
class State:
    """what IQLLearner owns: the agent, its target copy and the optimizer state (oracle.learners.clip_and_step's interface)"""

    def __init__(self, args, agent, dtype=torch.float64):
        self.args, self.dtype = args, dtype
        self.agent = {k: torch.tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True) for k, x in agent.items()}
        self.opt, self.opt_step = {}, 0
        self.sync_targets()

    def named_params(self):
        return [("agent." + k, x) for k, x in self.agent.items()]

    def sync_targets(self):
        self.target_agent = {k: x.detach().clone() for k, x in self.agent.items()}


def forward(state, batch, lam=None):
    """IQLLearner's loss on a batch (the 11-key episode dict): (loss, intermediates).  Quirks Q1 / Q2 as oracle.learners.q_forward"""
    args, dt = state.args, state.dtype
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}
    B, N, A, H = bt["o"].shape[0], args.n_agents, args.n_actions, args.rnn_hidden_dim
    la, ru = args.last_action, args.reuse_network
    h0 = torch.zeros(B * N, H, dtype=dt)
    q_evals, _, h_last = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(bt["u_onehot"]), h0, la, ru)
    with torch.no_grad():
        q_tgt, _, _ = nets.agent_unroll(state.target_agent, bt["o_next"], bt["u_onehot"], h0, la, ru)
        q_en = nets.agent_unroll(state.agent, bt["o_next"], bt["u_onehot"], h_last.detach(), la, ru)[0] if args.double_q else None
    R = B * T * N
    flat = lambda x: None if x is None else x.reshape(R, A).double()
    u = bt["u"].reshape(R)
    r, term, padded = (bt[k].reshape(B * T).double() for k in ("r", "terminated", "padded"))
    o = rows(flat(q_evals.detach()), u, flat(q_en), flat(q_tgt), flat(bt["avail_u_next"]), r, term, padded, args.gamma, N)
    y, G = o.y, None
    if lam is not None:
        y, G = lambda_returns(o.q_next, r, term, padded, args.gamma, lam, B, T, N)
    m = o.m.to(dt)
    q_taken = torch.gather(q_evals, 3, bt["u"].reshape(B, T, N, 1)).reshape(R)
    td = torch.where(o.live, y.to(dt) - q_taken, torch.zeros(R, dtype=dt))
    num = (m * td ** 2).sum()
    loss = num / m.sum()
    inter = dict(T=T, q_evals=q_evals, q_targets=q_tgt, q_taken=o.q_taken.reshape(B, T, N), q_next=o.q_next.reshape(B, T, N),
                 td_targets=G, loss=loss, num=num, den=m.sum())
    return loss, inter


def train(state, batch, train_step, lam=None):
    """one IQLLearner.train call: (loss float, gradients before the clip, intermediates)"""
    loss, inter = forward(state, batch, lam)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter


# ------------------------------------------------------------------------------------------------ the learner cases
# 2s3z-shaped, B = 4; episode 0 ends at the window's last step, episode 2 never terminates (quirk Q2), the others are shorter.
LEARNER_B, LEARNER_T, LEARNER_LENGTHS, AGENT_SEED = 4, 6, [6, 3, -1, 4], 11
LEARNER_TOL = (1e-4, 1e-3, 1e-3)      # tests/test_gpu_learners.py's: 1e-4 of max|ref| for the first update, 1e-3 for the later ones
# name -> (args overrides, td_lambda, seed of update 0's batch; update i draws seed + i).  RMSprop's first step moves a parameter by
# lr g / (0.1 |g| + 1e-8): where |g| is near 1e-7 the rounding of g decides the step, and whether a batch has such entries is a
# property of the batch, not of the arithmetic under test.  The seeds are chosen ON THE CPU so that this oracle run in float32 stays
# under a quarter of LEARNER_TOL of its float64 self in every parameter at all three updates (tests/test_iql_oracle_cpu.py asserts
# it; seed 100 of the other cases puts the float32 oracle of "max" at 0.63 of the bound by itself).
LEARNER_CASES = {"double_q": ({}, None, 100), "max": (dict(double_q=False), None, 160), "lam0": ({}, 0.0, 100),
                 "lam0.8": ({}, 0.8, 100)}


def learner_case(name, dtype=torch.float64, **more):
    """(args, State, batch(i), td_lambda) of a learner case"""
    over, lam, seed0 = LEARNER_CASES[name]
    kw = dict(over, **more)
    if lam is not None:
        kw["td_lambda"] = lam
    args = seeded.make_args("2s3z", "iql", episode_limit=LEARNER_T, **kw)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=AGENT_SEED)
    batch = lambda i: seeded.make_batch(args, LEARNER_B, seed=seed0 + i, lengths=LEARNER_LENGTHS)
    return args, State(args, agent, dtype), batch, lam


def float32_fraction(name):
    """the worst |float32 oracle - float64 oracle| of a parameter over the case's three updates, as a fraction of LEARNER_TOL's bound"""
    _, a, batch, lam = learner_case(name, torch.float64)
    _, b, _, _ = learner_case(name, torch.float32)
    worst = 0.0
    for i, tol in enumerate(LEARNER_TOL):
        train(a, learners.clone_batch(batch(i)), i, lam=lam)
        train(b, learners.clone_batch(batch(i)), i, lam=lam)
        for k in a.agent:
            ref = a.agent[k].detach().numpy()
            worst = max(worst, float(np.abs(b.agent[k].detach().double().numpy() - ref).max() / (tol * np.abs(ref).max() + 1e-7)))
    return worst


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
A_SIZES = (1, 2, 11, 16, 17, 21, 22, 32)         # 21 | 22: the staging switch with three row operands
A_TWO_OPERANDS = (31, 33)                        # 31 | 32: the switch with two (q_sel or avail_next NULL); 33 beyond both
A_ONE_OPERAND = (63, 64)                         # 63 | 64: the switch with one (both NULL); 63 is the largest staged tile, 64 512 bytes
TIE_FIRST, TIE_LAST = 1.25, -0.75                # q_tgt at the first and at the last column of a tie in q_sel
N_SIZES = (1, 3, 10)
BT_SIZES = ((1, 1), (3, 5), (5, 13))
BIG = (11, 7, 5)                                 # B, T, N with R = 385 = 64 * 6 + 1: partly filled waves, two workgroups


def kernel_case(B, T, N, A, seed=0):
    """float32 inputs.  Episode 0 runs the full length and terminates on its last step (term = 1 on a live step), episode 1 (if any)
    never terminates, the others are ragged with term = 1 on their last live step and on the padding.  By row % 7: 0 a tie of
    q_sel's maximum at the first and the last column, 1 a tie at the last two columns - both columns available, and q_tgt holds
    TIE_FIRST at the first and TIE_LAST at the last of them, so q_next shows which one was picked -, 2 nothing available, 3 exactly
    one action available.  Padded rows hold NaN in q, q_sel, q_tgt and avail_next."""
    g = np.random.default_rng(7000 + seed)
    R = B * T * N
    q, q_sel, q_tgt = (g.standard_normal((R, A)).astype(f32) for _ in range(3))
    avail = (g.random((R, A)) < 0.7).astype(f32)
    rr = np.arange(R)
    k0, k1, k2, k3 = (rr % 7 == k for k in range(4))
    q_sel[k0, 0] = q_sel[k0, A - 1] = 7.5
    q_sel[k1, A - 1] = q_sel[k1, max(A - 2, 0)] = 8.25
    for k, first, last in ((k0, 0, A - 1), (k1, max(A - 2, 0), A - 1)):      # q_tgt tells the tied columns apart: another tie order
        q_tgt[k, last] = TIE_LAST                                            # than the first index shows in q_next
        q_tgt[k, first] = TIE_FIRST
    avail[k0, 0] = avail[k0, A - 1] = 1
    avail[k1, A - 1] = avail[k1, max(A - 2, 0)] = 1
    avail[k2] = 0
    avail[k3] = 0
    avail[rr[k3], g.integers(0, A, size=int(k3.sum()))] = 1
    u = g.integers(0, A, size=R).astype(np.int32)
    r = g.standard_normal(B * T).astype(f32)
    lengths = [T, -1] + [int(x) for x in g.integers(1, T + 1, size=max(B - 2, 0))]
    term, padded = np.zeros((B, T), f32), np.zeros((B, T), f32)
    for b, L in enumerate(lengths[:B]):
        if L >= 0:
            term[b, L - 1:] = 1
            padded[b, L:] = 1
    dead = np.repeat(padded.reshape(-1) == 1, N)
    for x in (q, q_sel, q_tgt, avail):
        x[dead] = np.nan
    ret = g.standard_normal((B, N, T)).astype(f32)
    ret[np.repeat(padded[:, None, :], N, axis=1) == 1] = np.nan
    return NS(B=B, T=T, N=N, A=A, R=R, q=q, u=u, q_sel=q_sel, q_tgt=q_tgt, avail=avail, r=r, term=term.reshape(-1),
              padded=padded.reshape(-1), ret=ret, dead=dead, kinds=(k0, k1, k2, k3))
