"""TD(lambda) returns and the learners' losses on them (TEST INFRASTRUCTURE, CPU).

``returns`` is the recursion csrc/td_lambda.hip implements, in numpy; tests/golden/td_lambda.npz pins it to the reference's own
build_td_lambda_targets (utils/rl_utils.py:4-14) called with target_qs[:, t+1] = q[t] and the terminal flag masked by the
padding.  ``q_loss`` / ``qtran_loss`` put those returns in the place of the one-step target of oracle.learners' forwards;
``train`` is oracle.learners.q_train / qtran_train around them.
"""
import numpy as np
import torch

from oracle import learners

GAMMA = 0.99
SHAPES = ((7, 1), (7, 2), (7, 63), (7, 64), (7, 65), (7, 129))
LAMBDAS = (0.0, 0.8, 1.0)
JUNK = 1.0e6


def returns(q, r, term, padded, gamma, lam, dtype=np.float64):
    """G (B, T):  m = 1 - padded, done = sum_t m term, G[T] = q[T-1] (1 - done),
    G[t] = lam gamma G[t+1] + m[t] (r[t] + (1 - lam) gamma q[t] (1 - term[t])).  Serial in ``dtype``."""
    q, r, term, padded = (np.asarray(x, dtype=dtype) for x in (q, r, term, padded))
    B, T = q.shape
    gamma, lam, one = dtype(gamma), dtype(lam), dtype(1)
    m = one - padded
    done = (m * term).sum(axis=1, dtype=dtype)
    G = np.zeros((B, T + 1), dtype=dtype)
    G[:, T] = q[:, T - 1] * (one - done)
    for t in range(T - 1, -1, -1):
        G[:, t] = lam * gamma * G[:, t + 1] + m[:, t] * (r[:, t] + (one - lam) * gamma * q[:, t] * (one - term[:, t]))
    return G[:, :T]


def case_key(B, T):
    return "B%d_T%d" % (B, T)


def make_case(B, T, seed):
    """Seeded float32 inputs (q, r, term, padded) of a fixture case: episode 0 runs the full length and terminates on its last
    step, episode 1 has length 1, episode 2 never terminates, the others are ragged; padded steps carry term = 1 (as the
    batches of this code base do), a non-zero r and JUNK-sized values in q."""
    assert B >= 4
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, T)).astype(np.float32)
    r = rng.standard_normal((B, T)).astype(np.float32)
    term = np.zeros((B, T), np.float32)
    padded = np.zeros((B, T), np.float32)
    lengths = [T, 1, -1] + [int(x) for x in rng.integers(1, T + 1, size=B - 3)]
    for b, L in enumerate(lengths):
        if L < 0:
            continue
        term[b, L - 1:] = 1.0
        padded[b, L:] = 1.0
        q[b, L:] = JUNK * np.where(rng.random(T - L) < 0.5, -1.0, 1.0) * (1.0 + rng.random(T - L))
    return q, r, term, padded


def load_cases(golden_dir):
    """[(key, lam, (q, r, term, padded), G float64, G_literal float64)] of tests/golden/td_lambda.npz"""
    import os
    fix = np.load(os.path.join(golden_dir, "td_lambda.npz"))
    out = []
    for B, T in SHAPES:
        k = case_key(B, T)
        inputs = tuple(fix["%s/%s" % (k, n)] for n in ("q", "r", "term", "padded"))
        for lam in LAMBDAS:
            out.append((k, lam, inputs, fix["%s/lam%g/G" % (k, lam)], fix["%s/lam%g/G_literal" % (k, lam)]))
    return out


# ---------------------------------------------------------------------------------
# the learners' losses on lambda-returns
# ---------------------------------------------------------------------------------
def _cut(state, batch, T):
    bt = learners.to_tensors(batch, T)
    B = bt["r"].shape[0]
    f = lambda k: bt[k].reshape(B, T)
    return B, f("r"), f("terminated"), f("padded")


def _G(state, q_tgt, r, term, padded, lam):
    G = returns(q_tgt.detach().numpy(), r.numpy(), term.numpy(), padded.numpy(), state.args.gamma, lam)
    return torch.tensor(G, dtype=torch.float32)


def q_loss(state, batch, lam):
    """VDN / QMIX / QPLEX: sum((m (G - q_tot))^2) / sum(m), G the lambda-returns of q_tot_target (detached)"""
    _, inter = learners.q_forward(state, batch)
    T = inter["T"]
    B, r, term, padded = _cut(state, batch, T)
    q_tot, q_tgt = inter["q_tot"].reshape(B, T), inter["q_tot_target"].reshape(B, T)
    G = _G(state, q_tgt, r, term, padded, lam)
    m = 1.0 - padded
    loss = ((m * (G - q_tot)) ** 2).sum() / m.sum()
    inter.update(td_targets=G, loss=loss)
    return loss, inter


def qtran_loss(state, batch, lam):
    """QTRAN: the reference's loss with L_td on the lambda-returns of joint_q_targets"""
    loss, inter = learners.qtran_forward(state, batch)
    T = inter["T"]
    B, r, term, padded = _cut(state, batch, T)
    jq, jq_tgt = inter["joint_q_evals"].reshape(B, T), inter["joint_q_targets"].reshape(B, T)
    G = _G(state, jq_tgt, r, term, padded, lam)
    m = 1.0 - padded
    l_td = (((jq - G) * m) ** 2).sum() / m.sum()
    loss = loss - inter["l_td"] + l_td
    inter.update(td_targets=G, loss=loss, l_td=l_td)
    return loss, inter


def train(state, batch, train_step, lam):
    """oracle.learners.q_train / qtran_train with the loss above; returns (loss float, grads before the clip, intermediates)"""
    fwd = qtran_loss if state.args.alg.startswith("qtran") else q_loss
    loss, inter = fwd(state, batch, lam)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter
