"""Float64 restatement of MAIC training on the TD loss (TEST INFRASTRUCTURE, written for this project): torch autograd over
tests/maic_oracle.py's ``head`` / the oracle's agent unroll, mixers, loss and optimizer (oracle/), the way tests/world_oracle.py
restates the world-model learner.

* ``head_grads``   gradients of sum_r return_q[r, u_act[r]] * dq_val[r] with respect to h and every head parameter
* ``State``        what MAICTDLearner owns: parameters (agent in MAICAgent's order, mixer), BatchNorm buffers of the eval and the
                   target network, optimizer state - all in ``dtype`` (float64; float32 for the precision yardstick)
* ``train``        one MAICTDLearner.train call: loss, every gradient, the grad norm; the state holds the parameters and buffers
                   after the step
* ``*_margins``    how far a case is from its discontinuities: greedy / double-Q selections, the variance clamp, the LeakyReLUs
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import learners, nets, seeded
import maic_oracle as mo

BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
HEAD_PREFIXES = ("embed_net.", "msg_net.", "w_key.", "w_query.")


def is_buffer(k):
    return k.rsplit(".", 1)[-1] in BUFFERS


def is_head_param(k):
    return k.startswith(HEAD_PREFIXES) and not is_buffer(k)


def _leaky_margin(pre, used):
    """min |pre| over the entries in ``used`` / max |pre| over the whole tensor (inf when none is used)"""
    sel = pre.abs()[used]
    return float(sel.min() / pre.abs().max()) if sel.numel() else float("inf")


def head_margins(p, h, out, bs, N, bn_train, val=None, var_floor=mo.VAR_FLOOR):
    """(clamp margin, LeakyReLU margin) of one head call whose outputs are ``out``.  The LeakyReLU margin is taken over the
    pre-activations whose DERIVATIVE reaches a gradient (the forward value is continuous at the kink: only the backward decides
    there): with ``val`` (bs*N) the gradient value at each receiver row - None: every row receives one - the pair (i, j) of
    msg_net counts when alpha[i][j] val_j != 0, and a row of embed_net when any row of its environment receives a gradient
    (its latents reach only that environment's receivers).  Always relative to the max over the whole tensor."""
    with torch.no_grad():
        y = F.linear(h, p["embed_net.0.weight"], p["embed_net.0.bias"])
        mean, var = (y.mean(0), y.var(0, unbiased=False)) if bn_train else (p[mo.BN + "running_mean"], p[mo.BN + "running_var"])
        bn = (y - mean) / torch.sqrt(var + mo.BN_EPS) * p[mo.BN + "weight"] + p[mo.BN + "bias"]
        par = F.linear(F.leaky_relu(bn, 0.01), p["embed_net.3.weight"], p["embed_net.3.bias"])
        ex = torch.exp(par[:, N * mo.L:])
        clamp = float(((ex - var_floor).abs() / var_floor).min())
        live = torch.ones(bs, N, dtype=torch.bool) if val is None else torch.as_tensor(np.asarray(val)).reshape(bs, N) != 0
        hj = h.view(bs, 1, N, -1).expand(bs, N, N, h.shape[-1])
        pre = F.linear(torch.cat([hj, out["latent"].reshape(bs, N, N, mo.L)], -1), p["msg_net.0.weight"], p["msg_net.0.bias"])
        pair = (out["alpha"] != 0) & live[:, None, :]
        row = live.any(1, keepdim=True).expand(bs, N).reshape(-1)
        return clamp, min(_leaky_margin(bn, row), _leaky_margin(pre, pair))


def head_grads(state, h, q, eps, u_act, dq_val, bs, N, test_mode, bn_train, dtype=torch.float64, G=None):
    """Gradients of sum(return_q * G), G given or built from the sparse pairs (G[r, u_act[r]] = dq_val[r]).  state: numpy state
    dict (maic_oracle.maic_state).  Returns dict(dh = the head's part (q is an input here, not fc2(h)), grads{head parameter:
    array}, out = the head's outputs, clamp / leaky margins)."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in state.items()}
    names = [k for k in p if is_head_param(k)]
    for k in names:
        p[k].requires_grad_(True)
    h = torch.tensor(np.asarray(h), dtype=dtype, requires_grad=True)
    q = torch.tensor(np.asarray(q), dtype=dtype)
    e = None if eps is None else torch.tensor(np.asarray(eps), dtype=dtype)
    out = mo.head(p, h, q, bs, N, test_mode, bn_train, e)
    if G is None:
        G = np.zeros(tuple(q.shape))
        G[np.arange(q.shape[0]), np.asarray(u_act)] = np.asarray(dq_val)
    obj = (out["return_q"] * torch.tensor(np.asarray(G), dtype=dtype)).sum()
    gs = torch.autograd.grad(obj, [h] + [p[k] for k in names], allow_unused=True)
    grads = {k: (g.numpy() if g is not None else np.zeros(tuple(p[k].shape))) for k, g in zip(names, gs[1:])}
    val = None if u_act is None else dq_val
    clamp, leaky = head_margins({k: v.detach() for k, v in p.items()}, h.detach(), out, bs, N, bn_train, val)
    return dict(dh=gs[0].numpy(), grads=grads, out={k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()},
                clamp_margin=clamp, leaky_margin=leaky)


class State(learners.LearnerState):
    """LearnerState in ``dtype`` with the BatchNorm buffers beside the parameters (they are not trained, the optimizer and
    the clip norm do not see them; the target copy carries them)"""

    def __init__(self, args, agent, mixer, dtype=torch.float64):
        f = lambda d: {k: torch.tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True) for k, x in d.items()}
        self.args, self.dtype = args, dtype
        self.agent = f({k: v for k, v in agent.items() if not is_buffer(k)})
        self.bn = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in agent.items() if is_buffer(k)}
        self.mixer = f(mixer)
        self.v = self.extra = None
        self.opt, self.opt_step = {}, 0
        self.sync_targets()

    def sync_targets(self):
        self.target_agent = {k: x.detach().clone() for k, x in self.agent.items()}
        self.target_mixer = {k: x.detach().clone() for k, x in self.mixer.items()}
        self.target_bn = {k: x.clone() for k, x in self.bn.items()}


def _head_over(p, bn, hs, q, eps, bn_train, margins, val=None):
    """q (B,T,N,A) + the gated messages, sampled latents.  bn_train: one head call per transition index, the buffers in ``bn``
    move with every call; otherwise one call over all rows.  val (B,T,N): where the differentiated pass receives a gradient -
    None for a pass without one, whose LeakyReLU margin is then infinite (nothing is differentiated there)."""
    B, T, N, A = q.shape

    def track(pp, h, out, bs, v):
        v = torch.zeros(bs * N) if v is None else v.reshape(-1)
        margins.append(head_margins({k: x.detach() for k, x in pp.items()}, h.detach(), out, bs, N, bn_train, v))
    if not bn_train:
        pp = {**p, **bn}
        out = mo.head(pp, hs.reshape(B * T * N, -1), q.reshape(B * T * N, A), B * T, N, False, False, eps.reshape(B * T * N, -1))
        track(pp, hs.reshape(B * T * N, -1), out, B * T, val)
        return out["return_q"].view(B, T, N, A)
    res = []
    for t in range(T):
        pp = {**p, **bn}
        h = hs[:, t].reshape(B * N, -1)
        out = mo.head(pp, h, q[:, t].reshape(B * N, A), B, N, False, True, eps[:, t].reshape(B * N, -1))
        track(pp, h, out, B, None if val is None else val[:, t])
        bn[mo.BN + "running_mean"], bn[mo.BN + "running_var"] = out["running_mean"].detach(), out["running_var"].detach()
        bn[mo.BN + "num_batches_tracked"] = bn[mo.BN + "num_batches_tracked"] + 1
        res.append(out["return_q"].view(B, N, A))
    return torch.stack(res, 1)


def _top2_gap(q, avail):
    """min over rows of (best - second best) / max |q| among available actions (rows with one available action: none)"""
    qq = q.detach().clone()
    scale = float(qq.abs().max())
    qq[avail == 0] = -float("inf")
    srt = torch.sort(qq, -1, descending=True)[0]
    gap = srt[..., 0] - srt[..., 1]
    gap = gap[torch.isfinite(gap)]
    return float(gap.min()) / scale if gap.numel() else float("inf")


def q_forward(state, batch, eps, bn_train=True, T=None):
    """learners.q_forward with the message head on every Q tensor (MAICTDLearner._forward_backward).  eps: dict of
    (B,T,N,N*L) arrays cur / next_eval / next_target.  Returns (loss, intermediates incl. the decision margins)."""
    args, dt = state.args, state.dtype
    if T is None:
        T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = {k: (v if k == "u" else v.to(dt)) for k, v in learners.to_tensors(batch, T).items()}
    B, N, H = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim
    s, u, r, s_next = bt["s"], bt["u"], bt["r"], bt["s_next"]
    avail_u, avail_next, term, u_onehot = bt["avail_u"], bt["avail_u_next"], bt["terminated"], bt["u_onehot"]
    mask = 1.0 - bt["padded"]
    la, ru = args.last_action, args.reuse_network
    e = {k: torch.tensor(np.asarray(v), dtype=dt)[:, :T] for k, v in eps.items()}
    margins, sel = [], []
    h0 = torch.zeros(B * N, H, dtype=dt)
    q_evals, hs_eval, h_last = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(u_onehot), h0, la, ru)
    q_evals = _head_over(state.agent, state.bn, hs_eval, q_evals, e["cur"], bn_train, margins, val=mask.expand(-1, -1, N))
    q_chosen = torch.gather(q_evals, 3, u).squeeze(3)
    with torch.no_grad():
        if args.double_q:
            q_en, hs_en, _ = nets.agent_unroll(state.agent, bt["o_next"], u_onehot, h_last.detach(), la, ru)
            q_en = _head_over(state.agent, state.bn, hs_en, q_en, e["next_eval"], bn_train, margins).clone()
        q_tgt, hs_tgt, _ = nets.agent_unroll(state.target_agent, bt["o_next"], u_onehot, h0, la, ru)
        q_tgt = _head_over(state.target_agent, state.target_bn, hs_tgt, q_tgt, e["next_target"], bn_train, margins).clone()
        live = (mask > 0).expand(-1, -1, N) if mask.dim() == 3 else mask > 0
        pick = lambda q, av: _top2_gap(q[live], av[live])
        if args.double_q:
            sel.append(pick(q_en, avail_next))
        else:
            sel.append(pick(q_tgt, avail_next))
        q_tgt[avail_next == 0.0] = learners.MASK_BIG
        if args.double_q:
            q_en[avail_next == 0] = learners.MASK_BIG
            cur_max = q_en.argmax(dim=3, keepdim=True)
            q_tgt_chosen = torch.gather(q_tgt, 3, cur_max).squeeze(3)
        else:
            cur_max = None
            q_tgt_chosen = q_tgt.max(dim=3)[0]
    if args.alg == "qplex":
        v_tot = nets.qplex(state.mixer, q_chosen, s, args, is_v=True)
        qd = q_evals.detach().clone()
        qd[avail_u == 0] = learners.MASK_BIG
        a_tot = nets.qplex(state.mixer, q_chosen, s, args, actions=u_onehot, max_q_i=qd.max(dim=3)[0], is_v=False)
        q_tot = v_tot + a_tot
        with torch.no_grad():
            if args.double_q:
                onehot = torch.zeros_like(u_onehot).scatter_(3, cur_max, 1)
                vt = nets.qplex(state.target_mixer, q_tgt_chosen, s_next, args, is_v=True)
                at = nets.qplex(state.target_mixer, q_tgt_chosen, s_next, args, actions=onehot, max_q_i=q_tgt.max(dim=3)[0],
                                is_v=False)
                q_tot_tgt = vt + at
            else:
                q_tot_tgt = nets.qplex(state.target_mixer, q_tgt_chosen, s_next, args, is_v=True)
    elif args.alg == "qmix":
        q_tot = nets.qmix(state.mixer, q_chosen, s, args)
        with torch.no_grad():
            q_tot_tgt = nets.qmix(state.target_mixer, q_tgt_chosen, s_next, args)
    elif args.alg == "vdn":
        q_tot = nets.vdn(q_chosen)
        q_tot_tgt = nets.vdn(q_tgt_chosen)
    else:
        raise ValueError("Mixer {} not recognised.".format(args.alg))
    td = (r + args.gamma * q_tot_tgt * (1 - term)).detach() - q_tot
    loss = ((mask * td) ** 2).sum() / mask.sum()
    return loss, dict(T=T, q_evals=q_evals, q_targets=q_tgt, q_tot=q_tot, den=mask.sum(), selection_margin=min(sel),
                      clamp_margin=min(m[0] for m in margins), leaky_margin=min(m[1] for m in margins))


def train(state, batch, train_step, eps, bn_train=True):
    """one MAICTDLearner.train call: (loss float, grads before the clip {agent.* / mixer.*: tensor or None}, intermediates)"""
    loss, inter = q_forward(state, batch, eps, bn_train)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter


# ---------------------------------------------------------------------------------------------------- the cases of the tests
# head backward: (shape, bs, test_mode, batch statistics)
HEAD_CASES = [(shape, bs, tm, bn) for shape in ("matrix", "2s3z", "MMM2")
              for bs, tm, bn in ((37, False, False), (37, False, True), (1, False, False), (2, False, True), (37, True, False))]
# the partial merge has 16 slices (csrc/maic_head_bwd.hip: MB_SLICES) and goes through them only above 16 tiles: MMM2 at bs 37 has
# 37 tiles (slices of 3 and of 2 tiles), 2s3z at bs 70 has 24 (slices of 2 and of 1).  2s3z at bs 8 (3 tiles, the last one partly
# filled) is the case in which EVERY row receives a gradient: no tile's partials or row planes are zero there.
HEAD_CASES += [("2s3z", 70, False, False), ("2s3z", 70, False, True), ("2s3z", 8, False, False), ("2s3z", 8, False, True)]
DENSE_BS = 8              # up to this many environments every row of a head case receives a gradient
# (shape, bs, test_mode, bn) -> seed: the first seed from 1 on at which the case clears the clamp margin (1e-3) and the LeakyReLU
# margin (1e-5) by a factor of 1.3
HEAD_SEED = {("matrix", 37, False, False): 1, ("matrix", 37, False, True): 1, ("matrix", 1, False, False): 1,
             ("matrix", 2, False, True): 1, ("matrix", 37, True, False): 1,
             ("2s3z", 37, False, False): 10, ("2s3z", 37, False, True): 12, ("2s3z", 1, False, False): 1,
             ("2s3z", 2, False, True): 2, ("2s3z", 37, True, False): 1,
             ("2s3z", 70, False, False): 3, ("2s3z", 70, False, True): 9, ("2s3z", 8, False, False): 3, ("2s3z", 8, False, True): 1,
             ("MMM2", 37, False, False): 73, ("MMM2", 37, False, True): 36, ("MMM2", 1, False, False): 1,
             ("MMM2", 2, False, True): 2, ("MMM2", 37, True, False): 2}
HEAD_SEED0 = 5


def head_case_id(c):
    return "%s_bs%d_%s_%s" % (c[0], c[1], "test" if c[2] else "samp", "batch" if c[3] else "eval")


def head_case_inputs(case, scale=3.0):
    """(args, state, h, q, eps, u_act, dq_val) of a head-backward case"""
    shape, bs, test_mode, bn = case
    seed = HEAD_SEED.get(case, HEAD_SEED0)
    args = mo.maic_args(shape)
    N, A = args.n_agents, args.n_actions
    state = mo.maic_state(args, seed=seed, scale=scale)
    rng = np.random.default_rng(100 + seed)
    R = bs * N
    h = (0.5 * rng.standard_normal((R, 64))).astype(np.float32)
    q = rng.standard_normal((R, A)).astype(np.float32)
    eps = rng.standard_normal((R, N * mo.L)).astype(np.float32)
    u_act = rng.integers(0, A, R).astype(np.int32)
    dq_val = rng.standard_normal(R).astype(np.float32)
    if bs > DENSE_BS:     # as under the TD loss's mask, most environments carry no gradient (their rows still count in the statistics)
        dq_val = dq_val * np.repeat(rng.random(bs) < 0.3, N)
    return args, state, h, q, eps, u_act, dq_val


# one update: (name, shape, alg, B, T, lengths, agent in training mode, weight scale, seed).  Seeds: the first from 1 on that clears
# all three margins by a factor of 1.3.  MMM2 holds 6400 msg_net pre-activations per live step, so its episodes are short: the
# padded steps still run through every kernel and count in the batch statistics, they only carry no gradient.
UPDATE_CASES = [
    ("maic_qmix_2s3z", "2s3z", "qmix", 6, 8, [8, 3, 1, 4, 2, 5], True, 1.0, 5),
    ("maic_qmix_MMM2", "MMM2", "qmix", 6, 8, [8, 1, 2, 1, 1, 1], True, 1.0, 22),
    ("maic_vdn_matrix", "matrix", "vdn", 6, 8, [8, 3, 1, 4, 2, 5], True, 1.0, 2),
    ("maic_qplex_2s3z", "2s3z", "qplex", 6, 8, [8, 3, 1, 4, 2, 5], True, 1.0, 5),
    ("maic_qmix_2s3z_eval", "2s3z", "qmix", 6, 8, [8, 3, 1, 4, 2, 5], False, 1.0, 1),
]


def update_case_states(case):
    """seeded numpy weights: (args, MAICAgent state dict, mixer state dict)"""
    name, shape, alg, B, T, lengths, bn_train, scale, seed = case
    args = mo.maic_args(shape, episode_limit=T)
    args.alg = alg
    agent = mo.maic_state(args, seed=seed, scale=scale)
    mshapes = seeded.mixer_param_shapes(args)
    mixer = seeded.seeded_state(mshapes, seed=seed + 1) if mshapes else {}
    return args, agent, mixer


def update_case_data(case, batch_seed=100):
    """(batch, eps dict) of an update case"""
    name, shape, alg, B, T, lengths, bn_train, scale, seed = case
    args, _, _ = update_case_states(case)
    batch = seeded.make_batch(args, B, seed=batch_seed, lengths=lengths)
    rng = np.random.default_rng(batch_seed + 7)
    N = args.n_agents
    eps = {k: rng.standard_normal((B, T, N, N * mo.L)).astype(np.float32) for k in ("cur", "next_eval", "next_target")}
    return batch, eps


# ---------------------------------------------------------------------------------------------------- bounds
TOL = 1e-4                # the project's bound: max |got - ref| <= TOL * max |ref|
TINY_GRAD = 1e-5          # see step_is_decided


def is_zero_gradient(name, bn_batch):
    """the gradients that are zero analytically, so that max |ref| is the float64 rounding and bounds nothing: w_query.bias (the d
    logits of a softmax sum to zero) and, under batch statistics, embed_net.0.bias (BatchNorm subtracts the column mean).
    name: a parameter's name, with or without the ``agent.`` prefix of an update's gradients."""
    n = name[len("agent."):] if name.startswith("agent.") else name
    return n == "w_query.bias" or (bn_batch and n == "embed_net.0.bias")


def bound_scale(name, bn_batch, ref64, ref32):
    """the ``scale`` to hand tests/parity.close (tol 1e-4) for a tensor: max |ref| - and for the analytically zero gradients
    (is_zero_gradient) alone 4 x the float32 oracle's own error on that tensor, where that is more"""
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    base = float(np.abs(ref64).max()) if ref64.size else 0.0
    if not is_zero_gradient(name, bn_batch):
        return base
    err32 = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    return max(base, 4.0 * err32 / TOL)


def layer_of(name):
    return name.rsplit(".", 1)[0]


def step_is_decided(name, grads64):
    """Mask of the entries of parameter ``name`` whose first optimizer step is decided by the gradient rather than by its
    rounding: RMSprop's first step is lr g / (0.1 |g| + 1e-8), a sign function of g, so an entry whose gradient is below
    TINY_GRAD of the largest gradient of its layer (weight and bias: sums of the same rows) - the analytically zero ones, such as
    w_query.bias, among them - moves by up to 10 lr in a direction float32 cannot know.  The same holds below |g| = 1e-6, where
    0.1 |g| is within an order of the 1e-8 beside it and the step follows |g| itself (d step / d g = lr 1e-8 / (0.1 |g| + 1e-8)^2).
    Those entries are checked through their gradients only."""
    top = max(float(np.abs(g).max()) for n, g in grads64.items() if layer_of(n) == layer_of(name))
    return np.abs(grads64[name]) >= max(TINY_GRAD * top, 1e-6)


def reference_update(case):
    """the first update of an update case in float64 and in float32: two dicts with loss, T, grads {agent.* / mixer.*: array
    (zeros where no gradient arrives)}, grad_norm, params after the step, bn_eval / bn_target buffers and the margins"""
    name, shape, alg, B, T, lengths, bn_train, scale, seed = case
    args, agent, mixer = update_case_states(case)
    batch, eps = update_case_data(case)
    out = []
    for dt in (torch.float64, torch.float32):
        st = State(args, agent, mixer, dtype=dt)
        loss, grads, inter = train(st, learners.clone_batch(batch), 0, eps, bn_train=bn_train)
        named = dict(st.named_params())
        g = {n: (grads[n].numpy() if grads[n] is not None else np.zeros(tuple(named[n].shape))) for n in grads}
        out.append(dict(loss=loss, T=inter["T"], grads=g, grad_norm=inter["grad_norm"],
                        params={n: p.detach().numpy() for n, p in named.items()},
                        bn_eval={k: v.numpy() for k, v in st.bn.items()}, bn_target={k: v.numpy() for k, v in st.target_bn.items()},
                        selection_margin=inter["selection_margin"], clamp_margin=inter["clamp_margin"],
                        leaky_margin=inter["leaky_margin"]))
    return out[0], out[1]
