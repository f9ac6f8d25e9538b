"""Float64 statements of the per-row, loss, replay-gather and optimizer operations of include/marl_hip.h (csrc/mixers.hip without
its QPLEX part, csrc/optim.hip), in plain numpy.  Written from the header comments and the reference lines they cite
(common/replaybuffer.py:54-60, algorithm/q_learner.py:100-117,165-173, algorithm/qtran_learner.py:121-152, network/mixer.py:64-80),
not from the kernels; nothing of marl_amd is imported.

Every computed float comes with a MAGNITUDE: the sum of the absolute values of the terms that form it.  A forward-error bound of an
fp32 evaluation is (operations on the path) * u * magnitude with u = 2^-24; tests/test_gpu_rowwise.py holds the kernels to it."""
import types

import numpy as np

U = 2.0 ** -24
f64 = lambda x: np.asarray(x, dtype=np.float64)
NS = types.SimpleNamespace


# ------------------------------------------------------------------------------------------ replay gather
def replay_sample(ring, idx):
    """ReplayBuffer.sample on (T+1)-slot storage.  ring: u (E,T,N) int, r / term / padded (E,T), length / won (E), avail
    (E,T+1,N,A).  avail_next = slots 1..T of the sampled episodes, avail_cur = slots 0..T-1 with zeros from length[e] on."""
    idx = np.asarray(idx, dtype=np.int64)
    T = ring.u.shape[1]
    u = ring.u[idx]
    avail = ring.avail[idx]
    live = (np.arange(T)[None, :] < ring.length[idx][:, None])
    cur = avail[:, :T] * live[:, :, None, None]
    return NS(o_map=idx.astype(np.int32), u=u.astype(np.int32), u_act=np.maximum(u, 0).astype(np.int32), r=ring.r[idx],
              term=ring.term[idx], padded=ring.padded[idx], length=ring.length[idx].astype(np.int32),
              won=ring.won[idx].astype(np.int32), avail_next=avail[:, 1:], avail_cur=cur)


# ------------------------------------------------------------------------------------------ selection
def _masked(q, avail, mask_val):
    q = f64(q)
    return q if avail is None else np.where(np.asarray(avail) == 0, float(mask_val), q)


def q_gather(q, idx, avail=None, mask_val=0.0):
    """out[row] = q[row, idx[row]], masked first when avail is given; idx < 0 -> 0"""
    idx = np.asarray(idx)
    rows = np.arange(idx.shape[0])
    v = _masked(q, avail, mask_val)[rows, np.maximum(idx, 0)]
    return np.where(idx < 0, 0.0, v)


def q_masked_max(q, avail, mask_val):
    """max and first-index argmax over the actions of the masked q"""
    m = _masked(q, avail, mask_val)
    return m.max(axis=1), m.argmax(axis=1).astype(np.int32)        # numpy's argmax returns the first maximum


def q_double_select(q_sel, q_val, avail, mask_val):
    arg = _masked(q_sel, avail, mask_val).argmax(axis=1)
    return _masked(q_val, avail, mask_val)[np.arange(arg.shape[0]), arg], arg.astype(np.int32)


def q_scatter(idx1, g1, idx2, g2, rows, A, gdiv=1):
    """dq = 0; dq[row, idx1[row]] += g1[row // gdiv]; the same for the optional second pair; idx < 0 adds nothing"""
    dq = np.zeros((rows, A))
    r = np.arange(rows)
    for idx, g in ((idx1, g1), (idx2, g2)):
        if idx is None or g is None:
            continue
        idx = np.asarray(idx)
        ok = idx >= 0
        np.add.at(dq, (r[ok], idx[ok]), f64(g)[r[ok] // gdiv])
    return dq


def agent_sum(x):
    """x (rows, N, D) -> sum over the agents and its magnitude"""
    x = f64(x)
    return x.sum(axis=1), np.abs(x).sum(axis=1)


def agent_bcast(x, N, base=None):
    """x (rows, D) -> (rows, N, D), added to base when given"""
    out = np.repeat(f64(x)[:, None, :], N, axis=1)
    return out if base is None else out + f64(base)


def vec_add(a, b):
    return f64(a) + f64(b)


# ------------------------------------------------------------------------------------------ QMIX mixing
def _qmix_blocks(hy, N, E):
    hy = f64(hy)
    R = hy.shape[0]
    return (hy[:, :N * E].reshape(R, N, E), hy[:, N * E:N * E + E], hy[:, N * E + E:N * E + 2 * E],
            hy[:, N * E + 2 * E:N * E + 3 * E])


def _elu(a):
    return np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))


def qmix_mix(hy, q, N, E, b2=None, w22=None, b22=None):
    """QMixMixer.forward after the hypernet layers: q_tot = elu(q |w1| + b1) . |w2| + b2, with b2 given per row or formed as
    w22 . relu-block + b22.  Returns q_tot, its magnitude and the intermediates the backward shares."""
    w1, b1, w2, hb = _qmix_blocks(hy, N, E)
    q = f64(q)
    pre = b1 + np.einsum("rn,rne->re", q, np.abs(w1))
    mag_pre = np.abs(b1) + np.einsum("rn,rne->re", np.abs(q), np.abs(w1))
    hid = _elu(pre)
    # a <= 0: exp(a) - 1 passes the error of a on scaled by exp(a) <= 1 and is itself formed from two terms of size <= 1
    # (the + 1 up to pre = 2^-10: an fp32 evaluation of a pre-activation that close to 0 may land on either side)
    mag_hid = np.where(pre > 0, mag_pre, np.exp(np.minimum(pre, 0.0)) * mag_pre) + (pre <= 2.0 ** -10)
    if b2 is not None:
        bias, mag_bias = f64(b2), np.abs(f64(b2))
    else:
        bias = hb @ f64(w22) + float(np.asarray(b22).reshape(-1)[0])
        mag_bias = np.abs(hb) @ np.abs(f64(w22)) + abs(float(np.asarray(b22).reshape(-1)[0]))
    q_tot = (hid * np.abs(w2)).sum(axis=1) + bias
    mag = (mag_hid * np.abs(w2)).sum(axis=1) + mag_bias
    return NS(q_tot=q_tot, mag=mag, pre=pre, mag_pre=mag_pre, hid=hid, mag_hid=mag_hid)


def qmix_mix_grad(hy, q, dq_tot, N, E, w22=None):
    """autograd of qmix_mix for g = dL/dq_tot: dhy blocks [w1raw | b1 | w2raw (| relu block when w22 is given)], db2 = g, dq.
    d|x|/dx = sign(x) with sign(0) = 0 and d relu(x)/dx = [x > 0], as torch gives them."""
    w1, b1, w2, hb = _qmix_blocks(hy, N, E)
    q, g = f64(q), f64(dq_tot)[:, None]
    f = qmix_mix(hy, q, N, E, b2=np.zeros(hy.shape[0]))
    delu = np.where(f.pre > 0, 1.0, np.exp(np.minimum(f.pre, 0.0)))
    d_w2 = g * f.hid * np.sign(w2)
    dpre = g * np.abs(w2) * delu
    # exp(pre) inherits the absolute error of pre as a relative one: magnitude (1 + mag_pre) |dpre|
    mag_dpre = np.abs(dpre) * (1.0 + f.mag_pre)
    d_w1 = q[:, :, None] * dpre[:, None, :] * np.sign(w1)
    dq = np.einsum("rne,re->rn", np.abs(w1), dpre)
    out = NS(d_w1=d_w1, mag_w1=np.abs(q)[:, :, None] * mag_dpre[:, None, :] * (w1 != 0), d_b1=dpre, mag_b1=mag_dpre,
             d_w2=d_w2, mag_w2=np.abs(g) * f.mag_hid * (w2 != 0), db2=g[:, 0], dq=dq,
             mag_q=np.einsum("rne,re->rn", np.abs(w1), mag_dpre), d_hb=None, mag_hb=None)
    if w22 is not None:
        out.d_hb = g * f64(w22)[None, :] * (hb > 0)
        out.mag_hb = np.abs(out.d_hb)
    return out


# ------------------------------------------------------------------------------------------ losses
def td_loss(q_tot, q_tgt, r, term, padded, gamma):
    """target = r + gamma q_tgt (1 - term); td = mask (target - q_tot), mask = 1 - padded; dq_tot = -2 mask^2 (target - q_tot);
    out2 = {sum td^2, sum mask} (un-normalised)"""
    q_tot, q_tgt, r, term, padded = map(f64, (q_tot, q_tgt, r, term, padded))
    mask = 1.0 - padded
    boot = gamma * q_tgt * (1.0 - term)
    td = mask * (r + boot - q_tot)
    mag_td = np.abs(mask) * (np.abs(r) + np.abs(boot) + np.abs(q_tot))
    return NS(dq_tot=-2.0 * mask * td, mag_dq=2.0 * np.abs(mask) * mag_td, out2=np.array([(td ** 2).sum(), mask.sum()]),
              mag_num=(mag_td ** 2).sum())


def qtran_loss(jq, jq_tgt, v, jq_hat, qs_opt, qs_nopt, r, term, padded, gamma, lam_opt, lam_nopt):
    """qtran_learner.py:121-152 with the 1 / sum(mask) left out: L = l_td + lam_opt l_opt + lam_nopt l_nopt,
    l_td = sum (mask (jq - y))^2, l_opt = sum (mask (qs_opt - jq_hat + v))^2, l_nopt = sum (mask min(qs_nopt - jq + v, 0))^2 with jq_hat
    (l_opt) and jq (l_nopt) held fixed.  out4 = {l_td, l_opt, l_nopt, sum mask}."""
    jq, jq_tgt, v, jq_hat, qs_opt, qs_nopt, r, term, padded = map(f64, (jq, jq_tgt, v, jq_hat, qs_opt, qs_nopt, r, term, padded))
    mask = 1.0 - padded
    boot = gamma * jq_tgt * (1.0 - term)
    td = mask * (jq - (r + boot))
    mag_td = np.abs(mask) * (np.abs(jq) + np.abs(r) + np.abs(boot))
    opt = mask * (qs_opt - jq_hat + v)
    mag_opt = np.abs(mask) * (np.abs(qs_opt) + np.abs(jq_hat) + np.abs(v))
    nraw = qs_nopt - jq + v
    nopt = mask * np.minimum(nraw, 0.0)
    mag_nopt = np.abs(mask) * (np.abs(qs_nopt) + np.abs(jq) + np.abs(v))
    go, gn = lam_opt * 2.0 * mask * opt, lam_nopt * 2.0 * mask * nopt
    mgo, mgn = abs(lam_opt) * 2.0 * np.abs(mask) * mag_opt, abs(lam_nopt) * 2.0 * np.abs(mask) * mag_nopt
    return NS(d_jq=2.0 * mask * td, mag_jq=2.0 * np.abs(mask) * mag_td, d_v=go + gn, mag_v=mgo + mgn, d_qs_opt=go, mag_qs_opt=mgo,
              d_qs_nopt=gn, mag_qs_nopt=mgn, nraw=nraw,
              out4=np.array([(td ** 2).sum(), (opt ** 2).sum(), (nopt ** 2).sum(), mask.sum()]),
              mag_num=np.array([(mag_td ** 2).sum(), (mag_opt ** 2).sum(), (mag_nopt ** 2).sum()]))


# ------------------------------------------------------------------------------------------ optimizer
def sumsq(g):
    """fp64 sum of squares (a sum of non-negative terms: it is its own magnitude)"""
    g = f64(g)
    return float((g * g).sum())


def grad_scale(ss, den, clip):
    """what multiplies the un-normalised gradient: 1 / den, then torch's clip_grad_norm_ coefficient clip / (norm + 1e-6) clamped to
    1, norm being that of the normalised gradient.  Returns (scale, unclamped coefficient)."""
    inv = 1.0 if den is None else 1.0 / float(den)
    coef = float(clip) / (np.sqrt(ss) * inv + 1e-6)
    return inv * min(coef, 1.0), coef


def rmsprop_step(p, g, sq, lr, alpha, eps, clip, den=None, ss=None):
    """clip_grad_norm_ + one torch.optim.RMSprop step (not centred, no momentum) on a flat buffer"""
    p, g, sq = f64(p), f64(g), f64(sq)
    sc, coef = grad_scale(sumsq(g) if ss is None else ss, den, clip)
    gi = g * sc
    s = alpha * sq + (1.0 - alpha) * gi * gi
    dp = lr * gi / (np.sqrt(s) + eps)
    return NS(p=p - dp, sq=s, dp=dp, mag_dp=np.abs(dp), coef=coef)


def adam_step(p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, clip, den=None, ss=None):
    """clip_grad_norm_ + one torch.optim.Adam step; bc1 = 1 - b1^t and bc2_sqrt = sqrt(1 - b2^t) are arguments"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    sc, coef = grad_scale(sumsq(g) if ss is None else ss, den, clip)
    gi = g * sc
    mi = b1 * m + (1.0 - b1) * gi
    mag_m = np.abs(b1 * m) + np.abs((1.0 - b1) * gi)
    vi = b2 * v + (1.0 - b2) * gi * gi
    denom = np.sqrt(vi) / bc2_sqrt + eps
    dp = (lr / bc1) * mi / denom
    return NS(p=p - dp, m=mi, mag_m=mag_m, v=vi, dp=dp, mag_dp=(lr / bc1) * mag_m / denom, coef=coef)


# ------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
# Everything is drawn in float32 (what the kernels are given); the oracle reads the same values in float64.
f32 = np.float32
MASK_VAL = -9999999.0           # q_learner.py:105; exact in fp32
GAMMA = float(f32(0.99))        # scalars reach the kernels as C floats: both sides get the rounded value
LAM_OPT, LAM_NOPT = float(f32(0.7)), float(f32(1.9))
LR, ALPHA, EPS, CLIP = float(f32(5e-4)), float(f32(0.99)), float(f32(1e-8)), 10.0
BETA1, BETA2 = float(f32(0.9)), float(f32(0.999))

REPLAY_SHAPES = [(1, 1, 1), (5, 3, 7), (16, 8, 8), (41, 5, 5), (60, 8, 14), (300, 1, 2)]
REPLAY_RING, REPLAY_IDX = 11, (10, 0, 3, 3, 9, 0, 5)


def replay_case(T, N, A, seed=0):
    """a ring of 11 episodes, every one with different data, and 7 unsorted indices with repeats, the first and the last slot"""
    g = np.random.default_rng(1000 + seed)
    E = REPLAY_RING
    length = g.integers(1, T + 1, size=E).astype(np.int32)
    length[0], length[E - 1], length[3] = 1, T, (T + 1) // 2
    u = g.integers(0, A, size=(E, T, N)).astype(np.int32)
    steps = np.arange(T)[None, :]
    u[steps >= length[:, None]] = -1
    ring = NS(u=u, r=g.standard_normal((E, T)).astype(f32), term=(steps == length[:, None] - 1).astype(f32),
              padded=(steps >= length[:, None]).astype(f32), length=length, won=g.integers(0, 2, size=E).astype(np.int32),
              avail=g.uniform(0.25, 1.0, size=(E, T + 1, N, A)).astype(f32), T=T, N=N, A=A)
    return ring, np.array(REPLAY_IDX, dtype=np.int64)


def select_case(rows, A, seed=0):
    """q_sel / q_val / avail / idx with, by row % 5: 0 a tie of the maximum at the first and the last column, 1 a tie at the last
    column and the one before, 2 nothing available; idx in [-1, A)"""
    g = np.random.default_rng(2000 + seed)
    q_sel = g.standard_normal((rows, A)).astype(f32)
    q_val = g.standard_normal((rows, A)).astype(f32)
    avail = (g.random((rows, A)) < 0.7).astype(f32)
    r = np.arange(rows)
    t0, t1, t2 = r % 5 == 0, r % 5 == 1, r % 5 == 2
    q_sel[t0, 0] = q_sel[t0, A - 1] = 7.5
    avail[t0, 0] = avail[t0, A - 1] = 1
    q_sel[t1, A - 1] = q_sel[t1, max(A - 2, 0)] = 8.25
    avail[t1, A - 1] = avail[t1, max(A - 2, 0)] = 1
    avail[t2] = 0
    idx = g.integers(-1, A, size=rows).astype(np.int32)
    return NS(q_sel=q_sel, q_val=q_val, avail=avail, idx=idx, rows=rows, A=A)


def qmix_case(R, N, E, seed=0):
    """hy rows [w1raw | b1 | w2raw | relu block] with exact zeros planted in the w1, w2 and relu blocks; by row % 4: 1 large negative
    pre-activations, 2 pre-activations within rounding of 0 (b1 cancels the weighted sum)"""
    g = np.random.default_rng(3000 + seed)
    W = N * E + 3 * E
    hy = (0.5 * g.standard_normal((R, W))).astype(f32)
    q = g.standard_normal((R, N)).astype(f32)
    hy[:, N * E + 2 * E:] = np.maximum(hy[:, N * E + 2 * E:], 0)
    zero = g.random((R, W)) < 0.05
    zero[:, N * E:N * E + E] = False
    hy[zero] = 0
    r = np.arange(R)
    hy[r % 4 == 1, N * E:N * E + E] -= f32(30.0)
    near = r % 4 == 2
    q[near] *= f32(0.125)          # small terms: the cancellation leaves the bound of these rows under the older test's ceiling
    w1 = np.abs(hy[near, :N * E].astype(np.float64)).reshape(-1, N, E)
    hy[near, N * E:N * E + E] = (-np.einsum("rn,rne->re", q[near].astype(np.float64), w1)).astype(f32)
    return NS(hy=hy, q=q, b2=g.standard_normal(R).astype(f32), w22=g.standard_normal(E).astype(f32),
              b22=g.standard_normal(1).astype(f32), dq_tot=g.standard_normal(R).astype(f32), R=R, N=N, E=E, W=W)


LOSS_KINDS = ("mixed", "all_padded", "none_padded", "all_terminated")


def loss_case(R, kind="mixed", seed=0):
    """inputs of both losses; by row % 3 == 0 the non-optimal term qs_nopt - jq + v is exactly 0 (in fp32 and fp64)"""
    g = np.random.default_rng(4000 + seed)
    c = NS(R=R, kind=kind)
    for k in ("q_tot", "q_tgt", "r", "jq", "jq_tgt", "v", "jq_hat", "qs_opt", "qs_nopt"):
        setattr(c, k, g.standard_normal(R).astype(f32))
    z = np.arange(R) % 3 == 0
    c.v[z] = 0
    c.qs_nopt[z] = c.jq[z]
    c.term = (g.random(R) < 0.1).astype(f32)
    c.padded = (g.random(R) < 0.2).astype(f32)
    if kind == "all_padded":
        c.padded[:] = 1
    elif kind == "none_padded":
        c.padded[:] = 0
    elif kind == "all_terminated":
        c.term[:] = 1
    return c


OPT_REGIMES = {"under": 0.1, "over": 5.0, "just_under": 1.0 - 5e-4, "just_over": 1.0 + 5e-4}   # norm / clip


def optim_case(n, regime, den, seed=0):
    """p, g and non-zero incoming state (sq for RMSprop; m, v for Adam); every 7th entry has g = 0 and zero state.  g is scaled so
    that the norm of g / den is OPT_REGIMES[regime] * CLIP (up to the fp32 rounding of g)"""
    g = np.random.default_rng(5000 + seed)
    grad = g.standard_normal(n)
    sq, m, v = 0.1 * g.standard_normal(n) ** 2, 0.1 * g.standard_normal(n), 0.01 * g.standard_normal(n) ** 2
    if n > 1:
        for a in (grad, sq, m, v):
            a[::7] = 0
    grad *= OPT_REGIMES[regime] * CLIP * (1.0 if den is None else den) / np.sqrt((grad * grad).sum())
    return NS(n=n, den=den, p=g.standard_normal(n).astype(f32), g=grad.astype(f32), sq=sq.astype(f32), m=m.astype(f32),
              v=v.astype(f32))


def bias_corrections(step):
    """(bc1, bc2_sqrt) of Adam step `step` as the C floats the kernel is given"""
    return float(f32(1.0 - BETA1 ** step)), float(f32(np.sqrt(1.0 - BETA2 ** step)))


# ------------------------------------------------------------------------------------------ forward-error bounds, in units of u
# Each constant counts the fp32 roundings on the path of one term of the output, from the formula in the header, plus 2 of slack;
# the bound is constant * U * magnitude.  None is tuned against a kernel's output.
SUM_TREE = 64                 # any summation tree of depth <= 64 over non-negative terms: 64 u relative
K_ELU = 4                     # exp(a) - 1, a <= 0, through the hardware base-2 exponential: the argument a * log2(e) carries two
                              # roundings (the constant and the product), each |a| u relative in the result: 2 |a| e^a u <= 0.74 u;
                              # v_exp_f32 is accurate to 1 ulp = 2 u e^a <= 2 u (AMD CDNA ISA reference); the subtraction <= 1 u


def k_qmix_pre(N):            # b1 + sum_n q_n |w1_n|: a term passes one product and at most N additions
    return N + 1


def k_qmix_fwd(N, E):         # pre, elu, the product with |w2|, the sum over E units (E / 32 per lane, doubled when the w22 . hb
    return k_qmix_pre(N) + K_ELU + 1 + (2 * max(E // 32, 1) + 5 + 1) + 2       # terms ride along), 5 shuffle levels, the bias


def k_qmix_dpre(N):           # g |w2| exp(pre): pre's error and the two argument roundings act relative to (1 + mag_pre), the
    return k_qmix_pre(N) + 2 + 2 + 2 + 2                                        # exponential 2 u, two products


def k_qmix_dw1(N):            # q_n * dpre * sign
    return k_qmix_dpre(N) + 2


def k_qmix_dw2(N):            # g * hid * sign: hid as in the forward
    return k_qmix_pre(N) + K_ELU + 2 + 2


def k_qmix_dq(N, E):          # sum_e |w1| dpre: one product, E / 32 additions per lane and 5 shuffle levels
    return k_qmix_dpre(N) + 1 + max(E // 32, 1) + 5


K_TD = 6 + 2                  # gamma * q_tgt, * (1 - term), + r, - q_tot, * mask, * mask (the factor 2 is exact)
K_TD_NUM = 2 * 6 + 1 + SUM_TREE + 2      # a squared term: twice the error of td (relative to its magnitude) and the product, then the tree
K_QTRAN_G = 4 + 3 + 2         # opt / nopt error: two additions, the mask, (the bootstrap's three for td); then * 2 mask * lambda
K_QTRAN_NUM = 2 * 6 + 1 + SUM_TREE + 2
K_SUMSQ = 1 + SUM_TREE + 2    # g^2, then the tree
# scale = (1 / den) * min(clip / (sqrt(sumsq) / den + 1e-6), 1): half of sumsq's relative error through the square root, then the
# square root, 1 / den, the product, the addition, the division, the product with 1 / den and 1 / den itself
K_SCALE = (1 + SUM_TREE) / 2.0 + 7
K_GI = K_SCALE + 1            # g * scale
K_SQ = 2 * K_GI + 1 + 1 + 1 + 2          # alpha sq + (1 - alpha) gi gi: the square, two products (the larger path), the addition
K_RMS_DP = (K_GI + 1) + (K_SQ - 2) / 2.0 + 2 + 1 + 2    # lr gi / (sqrt(s) + eps): numerator, sqrt(s), + eps, the division
K_ADAM_M = K_GI + 1 + 1 + 2   # b1 m + (1 - b1) gi relative to |b1 m| + |(1 - b1) gi|
K_ADAM_V = K_SQ
K_ADAM_DP = (K_ADAM_M - 2) + 2 + (K_ADAM_V - 2) / 2.0 + 3 + 1 + 2   # (lr / bc1) * m / (sqrt(v) / bc2s + eps)
