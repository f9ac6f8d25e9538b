"""Float64 restatement of PPO's clipped surrogate, of advantage standardisation and of PPOLearner (TEST INFRASTRUCTURE, written for
this project: the reference ships no PPO).  torch autograd over tests/policy_oracle.py's policy, critic, agent unroll and seeded
learner cases, tests/pg_oracle.py's log pi / entropy, tests/td_lambda_oracle.returns and oracle.learners.clip_and_step.

* ``numerator``         - sum m min(rho adv, clamp(rho, 1 - c, 1 + c) adv) - beta sum m H, written with torch.minimum / clamp; rows
                        with m = 0 or without a policy contribute nothing and their logits and logp_old are never looked at
* ``gate_coefficient``  the hand-written gradient gate: d numerator / d log pi(u) = - m (clipped ? 0 : adv rho)
* ``standardize``       m (x - mean) / (sqrt(var) + 1e-5) over the live entries, the variance around the mean
* ``kernel_case`` / ``kernel_reference``   content and float64 reference of the kernel test
* ``train``             one PPOLearner.train call: K passes with per-epoch intermediates, in the state's dtype
* ``RUNS`` / ``run_updates``   the learner runs of the GPU file and every tensor it compares; ``TEST_CLIP``, ``F32_EXCEPTIONS``
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import learners, nets, seeded
import pg_oracle as pg
import policy_oracle as po
import td_lambda_oracle as tl

CLASSES = ("unclipped", "clipped_high_pos", "clipped_low_neg", "past_high_neg", "below_low_pos")


# ------------------------------------------------------------------------------------------------ the loss
def numerator(z, avail, u, adv, logp_old, padded, eps, beta, clip):
    """z, avail (BT, N, A); u (BT, N); adv, padded (BT); logp_old (BT, N) or None (rho = 1: the first pass).  Returns a dict:
    num, logp, ent, rho (BT, N; 0 / 0 / 1 on dead rows), clipped (BT, N) bool, live (BT, N) bool, den = N sum m, hsum, nclip"""
    m = 1.0 - padded
    live = (m[:, None] > 0) & pg.has_policy(avail, u)
    z = torch.where(live[..., None], z, torch.zeros_like(z))                 # a dead row's logits are never looked at
    a = torch.where(m > 0, adv, torch.zeros_like(adv)).detach()[:, None].expand(live.shape)
    zero = torch.zeros(live.shape, dtype=z.dtype)
    logp = torch.where(live, pg.log_prob(z, avail, u, eps), zero)
    H = torch.where(live, pg.entropy(z, avail, eps), zero)
    old = logp.detach() if logp_old is None else torch.where(live, logp_old, zero)      # (nor its logp_old: it may hold NaN)
    old = torch.where(avail.sum(-1) == 1, logp.detach(), old)        # one available action: pi = 1 in every pass, rho = 1 exactly
    rho = torch.exp(torch.clamp(logp - old, max=80.0))
    s, k = rho * a, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * a
    w = m[:, None] * live.to(z.dtype)
    num = -(w * torch.minimum(s, k)).sum() - beta * (w * H).sum()
    clipped = live & (k.detach() < s.detach())
    return dict(num=num, logp=logp, ent=H, rho=rho.detach(), clipped=clipped, live=live, den=z.shape[1] * m.sum(),
                hsum=(w * H).sum(), nclip=(w * clipped.to(z.dtype)).sum(), adv_rows=a, s=s.detach(), k=k.detach())


def gate_coefficient(out, padded):
    """- m (clipped ? 0 : adv rho) per row: what the kernel hands its gradient walk as the scale of d log pi(u) / dz"""
    m = (1.0 - padded)[:, None] * out["live"].to(out["rho"].dtype)
    return -m * torch.where(out["clipped"], torch.zeros_like(out["rho"]), out["adv_rows"] * out["rho"])


def row_classes(out, avail, clip):
    """counts of the five classes over the live rows with a policy over more than one action"""
    many = out["live"] & (avail.sum(-1) > 1)
    rho, a, cl = out["rho"], out["adv_rows"], out["clipped"]
    hi, lo = rho > 1.0 + clip, rho < 1.0 - clip
    sets = dict(unclipped=many & ~hi & ~lo, clipped_high_pos=many & hi & (a > 0) & cl, clipped_low_neg=many & lo & (a < 0) & cl,
                past_high_neg=many & hi & (a < 0) & ~cl, below_low_pos=many & lo & (a > 0) & ~cl)
    return {k: int(v.sum()) for k, v in sets.items()}


def clip_margin(out, avail, clip):
    """the smallest |rho - (1 +- c)| over the live rows with a policy over more than one action (inf where there is none)"""
    many = out["live"] & (avail.sum(-1) > 1)
    if not bool(many.any()):
        return float("inf")
    rho = out["rho"][many]
    return float(torch.minimum((rho - (1.0 - clip)).abs(), (rho - (1.0 + clip)).abs()).min())


def standardize(x, padded):
    """(out, mean, var, M) in x's dtype; all zeros when no entry is live"""
    m = 1.0 - padded
    M = m.sum()
    if float(M) == 0.0:
        return torch.zeros_like(x), 0.0, 0.0, 0.0
    xm = torch.where(m > 0, x, torch.zeros_like(x))
    mean = (m * xm).sum() / M
    var = (m * (xm - mean) ** 2).sum() / M
    return m * (xm - mean) / (torch.sqrt(var) + 1e-5), float(mean), float(var), float(M)


# ------------------------------------------------------------------------------------------------ kernel test content
def standardize_case(rows, how, seed=0):
    """x, padded (rows) float32.  rand: about a third padded, padded entries hold NaN; allpad; one: exactly one live row; far:
    x = 100 + N(0, 1), where E[x^2] - mean^2 would lose the variance in fp32"""
    rng = np.random.default_rng(seed + rows)
    x = rng.standard_normal(rows).astype(np.float32) * 3.0 + 0.5
    padded = (rng.random(rows) < 0.33).astype(np.float32)
    if how == "far":
        x = (100.0 + rng.standard_normal(rows)).astype(np.float32)
    if how == "allpad":
        padded[:] = 1.0
    if how == "one":
        padded[:] = 1.0
        padded[rows // 2] = 0.0
    if how == "rand" and rows <= 2:
        padded[:] = 0.0
    x[padded == 1] = np.nan
    return x, padded


RHO_NEAR, RHO_AWAY = 1e-3, 1e-2      # a rho_target within RHO_NEAR of 1 - c or 1 + c is moved RHO_AWAY from it
RHO_MARGIN = 5e-4                    # ... so that every realised rho (float64 of the float32 logp_old) stays this far from both


def kernel_case(shape, eps, seed, clip=0.2):
    """po.kernel_rows' rows of shape (B, T, N, A) plus adv ~ N(0, 1) per step and logp_old = logp64 - log(rho_target), rho_target
    uniform in [0.5, 1.6] and kept away from the two clip edges: no row's branch depends on fp32 rounding.  Padded rows carry a
    NaN logp_old.  Asserts the distance on the float64 policy, and that each of the five classes is non-empty at a shape with at
    least 16 live rows; a smaller shape asserts that it holds a row with a spread policy and records which classes it has."""
    B, T, N, A = shape
    rows = po.kernel_rows(B, T, N, A, seed)
    rng = np.random.default_rng(seed + 1000)
    BT, R = B * T, B * T * N
    t = lambda k: torch.tensor(rows[k].astype(np.float64))
    z, a, u, padded = t("logits").view(BT, N, A), t("avail").view(BT, N, A), torch.tensor(rows["u"].astype(np.int64)).view(BT, N), t("padded")
    adv = rng.standard_normal(BT).astype(np.float32)
    adv[adv == 0] = 1.0
    m = 1.0 - padded
    live = (m[:, None] > 0) & pg.has_policy(a, u)
    logp64 = torch.where(live, pg.log_prob(torch.where(live[..., None], z, torch.zeros_like(z)), a, u, eps), torch.zeros(BT, N, dtype=torch.float64))
    target = rng.uniform(0.5, 1.6, size=(BT, N))
    for edge in (1.0 - clip, 1.0 + clip):
        near = np.abs(target - edge) < RHO_NEAR
        target[near] = edge + np.where(target[near] >= edge, RHO_AWAY, -RHO_AWAY)
    old = (logp64.numpy() - np.log(target)).astype(np.float32)
    old[np.repeat(rows["padded"], N).reshape(BT, N) == 1] = np.nan
    rows.update(adv=adv, logp_old=old.reshape(R), clip=clip)
    out = numerator(z, a, u, torch.tensor(adv.astype(np.float64)), torch.tensor(old.astype(np.float64)), padded, eps, 0.0, clip)
    assert clip_margin(out, a, clip) >= RHO_MARGIN, (shape, eps, seed, clip_margin(out, a, clip))
    counts = row_classes(out, a, clip)
    nlive = int(live.sum())
    if nlive >= 16:
        assert all(counts[c] > 0 for c in CLASSES), (shape, eps, seed, counts)
    else:
        assert sum(counts.values()) > 0, (shape, eps, seed, "no live row with more than one available action")
    rows["classes"] = counts                 # (a small shape holds the classes with a non-zero count here, and only those)
    return rows


# the kernel test's shapes (B, T, N, A) - tests/test_gpu_policy.py's SHAPES: the edges of the wave tile, (2, 3, 2, 30) on the
# row-per-lane form, (87500, 1, 3, 3) one row past a grid pass... -, its exploration rates and the content seed of a shape
KERNEL_SHAPES = ((3, 1, 2, 3), (4, 6, 5, 11), (2, 7, 8, 14), (37, 3, 10, 18), (2, 3, 2, 30), (87500, 1, 3, 3))
KERNEL_EPS = (0.0, 0.02, 0.5)
KERNEL_CLIP, KERNEL_BETA = 0.2, 0.01


def kernel_seed(shape):
    return 7 + sum(shape)


def kernel_reference(rows, N, eps, beta, clip, logp_old, adv):
    """float64 of the float32 kernel inputs as they are: dlogits (autograd of the numerator in its minimum / clamp form), logp, ent
    (R), the four statistics, rho (R) and the clipped mask (R).  logp_old (R) float32 or None; adv (BT) float32"""
    t = lambda x: torch.tensor(np.asarray(x).astype(np.float64))
    R, A = rows["logits"].shape
    BT = R // N
    z = t(rows["logits"]).requires_grad_(True)
    a, u = t(rows["avail"]).view(BT, N, A), torch.tensor(rows["u"].astype(np.int64)).view(BT, N)
    out = numerator(z.view(BT, N, A), a, u, t(adv), None if logp_old is None else t(logp_old).view(BT, N), t(rows["padded"]), eps, beta, clip)
    (dz,) = torch.autograd.grad(out["num"], z)
    return dict(dlogits=dz.numpy(), logp=out["logp"].detach().reshape(R).numpy(), ent=out["ent"].detach().reshape(R).numpy(),
                stats=np.array([float(out["num"].detach()), float(out["den"]), float(out["hsum"].detach()), float(out["nclip"])]),
                rho=out["rho"].reshape(R).numpy(), clipped=out["clipped"].reshape(R).numpy())


# ------------------------------------------------------------------------------------------------ the learner
def train(state, batch, train_step, eps, lam, clip, epochs, norm_adv, beta):
    """one PPOLearner.train call on a policy_oracle.State (its target critic is not used): returns the list of the K passes'
    intermediates.  Each holds v, td_targets, adv (B, T), logp, rho (B, T, N), dlogits, l_critic, l_actor, clip_frac, entropy, grads
    (before the clips, of the mean losses), agent. / critic. grad_norm and clip_coef, M, den_actor, mask, T, classes, clip_margin,
    relu_near_zero.  Both optimizers step after every pass, the last one included"""
    args, dt = state.args, state.dtype
    T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dt) for k, v in batch.items()}
    B, N, H = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim
    fed = nets.shifted_onehot(bt["u_onehot"])
    r, term, padded = (bt[k].reshape(B, T) for k in ("r", "terminated", "padded"))
    npdt = np.float64 if dt == torch.float64 else np.float32
    lam = 0.0 if lam is None else lam
    m = 1.0 - padded
    M = m.sum()
    avail, u = bt["avail_u"].reshape(B * T, N, -1), bt["u"].reshape(B * T, N)
    # once per batch, on the weights as they stand
    with torch.no_grad():
        v0 = po.critic(state.critic, bt["s"]).reshape(B, T)
        v_next = po.critic(state.critic, bt["s_next"]).reshape(B, T)
    G = torch.tensor(tl.returns(v_next.numpy(), r.numpy(), term.numpy(), padded.numpy(), args.gamma, lam, dtype=npdt), dtype=dt)
    adv = G - v0
    if norm_adv:
        adv = standardize(adv.reshape(-1), padded.reshape(-1))[0].reshape(B, T)
    with torch.no_grad():        # fc1's inputs do not depend on the weights: built once
        xin = [nets.build_inputs(bt["o"][:, t], fed[:, t], N, args.last_action, args.reuse_network) for t in range(T)]
    logp_old, passes = None, []
    for k in range(epochs):
        logits, _, _ = nets.agent_unroll(state.agent, bt["o"], fed, torch.zeros(B * N, H, dtype=dt), args.last_action, args.reuse_network)
        pre = []
        v = po.critic(state.critic, bt["s"], pre).reshape(B, T)
        l_critic = (m * (G - v) ** 2).sum() / M
        out = numerator(logits.reshape(B * T, N, -1), avail, u, adv.reshape(-1), logp_old, padded.reshape(-1), eps, beta, clip)
        l_actor = out["num"] / out["den"]
        (dlogits,) = torch.autograd.grad(out["num"], logits, retain_graph=True)
        with torch.no_grad():
            fc1_pre = torch.stack([nets.lin(state.agent, "fc1", x).view(B, N, H) for x in xin], 1)
        inter = dict(T=T, v=v.detach(), td_targets=G, adv=adv, logp=out["logp"].detach().reshape(B, T, N), rho=out["rho"].reshape(B, T, N),
                     dlogits=dlogits.reshape(B, T, N, -1), l_critic=float(l_critic.detach()), l_actor=float(l_actor.detach()),
                     clip_frac=float(out["nclip"] / out["den"]), entropy=float(out["hsum"].detach() / out["den"]), M=M,
                     den_actor=out["den"], mask=m, fc1_pre=fc1_pre, critic_pre=[x.detach().reshape(B, T, -1) for x in pre],
                     classes=row_classes(out, avail, clip), clip_margin=clip_margin(out, avail, clip))
        inter["relu_near_zero"] = po.relu_near_zero(inter)
        if k == 0:
            logp_old = out["logp"].detach()
        grads = {}
        pg._step(state.critic_half, l_critic, inter, grads)
        pg._step(state.actor_half, l_actor, inter, grads)
        inter["grads"] = grads
        passes.append(inter)
    return passes


# ------------------------------------------------------------------------------------------------ the learner runs
# The clip of the learner runs that must meet clipped rows.  With lr_actor = 1e-4 the ratio moves by a few percent in three passes
# (|rho - 1| up to 0.06 on 2s3z and 0.1 on MMM2, 0.02 on the matrix game), so c = 0.2 clips nothing there.  Found on the CPU from
# this oracle (tests/test_ppo_oracle_cpu.py asserts the classes and the margins):
#   2s3z, MMM2  c = 0.02: last pass of update 0 holds (unclipped, clipped-high adv > 0, clipped-low adv < 0) = (52, 11, 11) and (49, 25, 25)
#               rows, at td_lambda 0 and 1 (2s3z) (54, 10, 8) and (59, 9, 7);
#   matrix      c = 0.0095: the SECOND pass of update 0 holds (6, 4, 4).  Its last pass cannot hold a clipped row at any c: the 18
#               rows share one state, so they are six policy entries; once some are clipped the gradient comes from the rows that
#               pull the ratio back only, and the third pass finds every ratio inside the clip again (scanned c = 0.001 .. 0.03 in
#               steps of 0.00025 at beta 0, 0.01 and 0.05: no c with the three classes in the last pass).
TEST_CLIP = {"2s3z": 0.02, "MMM2": 0.02, "matrix": 0.0095}
CLIPPED_PASS = {"2s3z": 2, "MMM2": 2, "matrix": 1}        # the pass of update 0 (of 3) that holds the three classes
BETA = 0.01

# key -> (case, td_lambda, clip, epochs, norm_adv, beta, data seeds - one per update).  The seeds leave no ReLU pre-activation that
# carries a gradient within 1e-5 of zero and no ratio within 1e-4 of 1 - c or 1 + c, in any pass (the CPU file asserts both).
# The GPU learner file makes exactly these runs ("2s3z" in both gemm modes)
RUNS = {"2s3z": ("2s3z", 0.95, TEST_CLIP["2s3z"], 3, True, BETA, (101, 102)),
        "MMM2": ("MMM2", 0.95, TEST_CLIP["MMM2"], 3, True, BETA, (101, 100)),
        "matrix": ("matrix", 0.95, TEST_CLIP["matrix"], 3, True, BETA, (0, 0)),
        "2s3z/k1": ("2s3z", 0.95, 0.2, 1, False, 0.0, (100,)),
        "2s3z/norm": ("2s3z", 0.95, 0.2, 3, True, BETA, (101,)),
        "2s3z/nonorm": ("2s3z", 0.95, 0.2, 3, False, BETA, (101,)),
        "2s3z/lam0": ("2s3z", 0.0, TEST_CLIP["2s3z"], 3, True, BETA, (105,)),
        "2s3z/lam1": ("2s3z", 1.0, TEST_CLIP["2s3z"], 3, True, BETA, (106,))}
CLIPPED_RUNS = ("2s3z", "MMM2", "matrix", "2s3z/lam0", "2s3z/lam1")

# float32-oracle errors (max abs) of the tensors that do not stay under a quarter of 1e-4 * max|ref| (the GPU
# tests bound these alone by 4x the figure; derived from the two oracles on the CPU, never from GPU output).  Tensors from 0.6 of
# the quarter on are listed too: where RMSprop's step hangs on the rounding of a gradient near zero the float32 error depends on the
# host's summation order.  keys: (run, tensor)
F32_EXCEPTIONS = {
    ("2s3z", "step0/param critic.fc1.weight"): 9.25e-05, ("2s3z", "step0/param critic.fc2.weight"): 3.16e-06,
    ("2s3z", "step1/pass0/grad critic.fc2.weight"): 6.56e-06, ("2s3z", "step1/pass1/grad critic.fc2.weight"): 2.22e-06,
    ("2s3z", "step1/param critic.fc1.weight"): 9.24e-05, ("2s3z", "step1/param critic.fc2.weight"): 2.98e-06,
    ("MMM2", "step0/param critic.fc1.weight"): 1.78e-05, ("MMM2", "step1/param critic.fc1.weight"): 1.78e-05,
    ("2s3z/k1", "step0/param critic.fc1.weight"): 2.51e-05, ("2s3z/k1", "step0/param critic.fc2.weight"): 1.01e-05,
    ("2s3z/norm", "step0/param critic.fc1.weight"): 9.25e-05, ("2s3z/norm", "step0/param critic.fc2.weight"): 3.16e-06,
    ("2s3z/nonorm", "step0/param critic.fc1.weight"): 9.25e-05, ("2s3z/nonorm", "step0/param critic.fc2.weight"): 3.16e-06,
    ("2s3z/lam0", "step0/param critic.fc1.weight"): 1.53e-05}


def run_case(key, dtype=torch.float64):
    """(args, State, batch(i)) of a RUNS entry: policy_oracle.learner_case (its shapes, lengths and weight seeds) with MAPPO's fields
    in the arguments and the run's data seeds"""
    name, lam, clip, epochs, norm_adv, beta, seeds = RUNS[key]
    args, state, batch = po.learner_case(name, dtype, td_lambda=lam, ppo_clip=clip, ppo_epochs=epochs, ppo_norm_adv=norm_adv,
                                         policy_entropy_coef=beta)
    args.alg = "mappo"
    if name != "matrix":
        _, shape, B, T, lengths, _ = next(c for c in po.LEARNER_CASES if c[0] == name)
        batch = lambda i: seeded.make_batch(args, B, seed=seeds[i], lengths=lengths)
    return args, state, batch


def param_dict(state):
    return dict([("agent." + k, x) for k, x in state.agent.items()] + [("critic." + k, x) for k, x in state.critic.items()])


PASS_TENSORS = ("v", "td_targets", "adv", "logp", "rho", "dlogits")
PASS_SCALARS = ("l_critic", "l_actor", "clip_frac", "entropy")


def run_updates(key, dtype=torch.float64):
    """every tensor the GPU learner file compares, of all updates of a RUNS entry, as a flat dict "step<i>/pass<k>/<name>" ->
    array or float ("step<i>/param <name>" after each update); plus "near_zero" and "clip_margin" over all passes and
    "classes" = the class counts of update 0's passes"""
    name, lam, clip, epochs, norm_adv, beta, seeds = RUNS[key]
    args, state, batch = run_case(key, dtype)
    out = {"near_zero": 0, "clip_margin": float("inf"), "classes": None}
    for i in range(len(seeds)):
        passes = train(state, batch(i), i, po.EPS, lam, clip, epochs, norm_adv, beta)
        if i == 0:
            out["classes"] = [p["classes"] for p in passes]
        for k, p in enumerate(passes):
            s = "step%d/pass%d/" % (i, k)
            mask = p["mask"].numpy()
            for n in PASS_TENSORS:
                x = p[n].detach().numpy()
                out[s + n] = x * mask.reshape(mask.shape + (1,) * (x.ndim - 2))      # (a padded step's values are part of no loss)
            for n in PASS_SCALARS:
                out[s + n] = p[n]
            for n, g in p["grads"].items():
                out[s + "grad " + n] = g.detach().numpy()
            out[s + "clip actor"], out[s + "clip critic"] = p["agent.clip_coef"], p["critic.clip_coef"]
            out["near_zero"] += p["relu_near_zero"]
            out["clip_margin"] = min(out["clip_margin"], p["clip_margin"])
        for n, x in param_dict(state).items():
            out["step%d/param %s" % (i, n)] = x.detach().numpy().copy()
    return out
