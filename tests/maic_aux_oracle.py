"""Float64 restatement of the MAIC agent's two auxiliary losses and of MAICTDLearner with them (TEST INFRASTRUCTURE, written for
this project from the formulas of reference network/MAIC.py:88-123), on top of tests/maic_oracle.py / tests/maic_train_oracle.py.

* ``aux``              both losses of one head call as differentiable tensors, inference_net.1's buffers after the call, margins
* ``kernel_reference`` what csrc/maic_aux.hip returns for one call: the losses, the gradient on the post-clamp (mean, var) planes,
                       the part of dh through inference_net's input, every weight gradient, the buffers
* ``full_grads``       d (mi + ent) with respect to h (both paths) and every parameter - what the reference's autograd gives
* ``train``            one MAICTDLearner.train call with the two weights: loss = TD + (1/T) sum_t (mi_t + ent_t)
* the cases of tests/test_maic_aux_cpu.py and tests/test_gpu_maic_aux.py, and their bounds
"""
from __future__ import annotations

import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import learners, nets, seeded
import maic_oracle as mo
import maic_train_oracle as mt

IBN = "inference_net.1."
ALPHA_FLOOR = 1e-4
MI_W, ENT_W = 0.001, 0.01                  # the weights of the fixtures and of the update cases
KMI_W, KENT_W = 1.0, 1.0                   # of the kernel cases: gradients of order one, far above parity's absolute floor
AUX_PREFIXES = ("inference_net.", "w_key.", "w_query.")


def _bn(x, p, prefix, bn_train):
    """BatchNorm1d: (normalised x, batch mean, biased batch variance) - the batch values are None on the running statistics"""
    if bn_train:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = p[prefix + "running_mean"], p[prefix + "running_var"]
    out = (x - mean) / torch.sqrt(var + mo.BN_EPS) * p[prefix + "weight"] + p[prefix + "bias"]
    return out, (mean if bn_train else None), (var if bn_train else None)


def aux(p, h, return_q, bs, N, test_mode, bn_train, eps, mi_w, ent_w, var_floor=mo.VAR_FLOOR, h_infer=None):
    """p: tensors with MAICAgent's keys (buffers included); h (bs*N, 64), return_q (bs*N, A) the Q values after the messages.
    ``h_infer``: the tensor inference_net reads instead of h (the same values; lets a caller separate that path's gradient).
    Returns a dict: mi, ent (weighted, differentiable), mean / var (bs*N, N*L, post-clamp, in the graph), inference_net.1's
    running_mean / running_var / num_batches_tracked after the call, and the margins of the call."""
    L, D = mo.L, mo.D
    lk = lambda t: F.leaky_relu(t, 0.01)
    A = return_q.shape[1]
    NL, P = N * L, bs * N * N
    y = F.linear(h, p["embed_net.0.weight"], p["embed_net.0.bias"])
    z = lk(_bn(y, p, mo.BN, bn_train)[0])
    par = F.linear(z, p["embed_net.3.weight"], p["embed_net.3.bias"])
    mu, ex1 = par[:, :NL], torch.exp(par[:, NL:])
    v1 = torch.clamp(ex1, min=var_floor)
    latent = mu if test_mode else mu + torch.sqrt(v1) * eps
    out = dict(mean=mu, var=v1, clamp1_margin=float(((ex1.detach() - var_floor).abs() / var_floor).min()))
    rq = return_q.detach()
    srt = torch.sort(rq, -1, descending=True)[0]
    out["top2_margin"] = float((srt[:, 0] - srt[:, 1]).min() / rq.abs().max())
    rm, rv = p[IBN + "running_mean"].clone(), p[IBN + "running_var"].clone()
    nbt = int(p[IBN + "num_batches_tracked"])
    zero = (h * 0).sum()
    out.update(mi=zero, ent=zero, leaky_margin=float("inf"), clamp2_margin=float("inf"), alpha_margin=float("inf"))
    if mi_w > 0:
        a = rq.argmax(1)                                                    # the lowest index wins a tie
        hi = (h if h_infer is None else h_infer).view(bs, N, 1, -1).expand(bs, N, N, h.shape[-1]).reshape(P, -1)
        oh = F.one_hot(a, A).to(h.dtype).view(bs, 1, N, A).expand(bs, N, N, A).reshape(P, A)
        u = F.linear(torch.cat([hi, oh], -1), p["inference_net.0.weight"], p["inference_net.0.bias"])
        pre, bm, bv = _bn(u, p, IBN, bn_train)
        if bn_train:
            rm = (1 - mo.BN_MOM) * rm + mo.BN_MOM * bm.detach()
            rv = (1 - mo.BN_MOM) * rv + mo.BN_MOM * bv.detach() * P / (P - 1)
            nbt += 1
        o = F.linear(lk(pre), p["inference_net.3.weight"], p["inference_net.3.bias"])
        m2, ex2 = o[:, :L], torch.exp(o[:, L:])
        v2 = torch.clamp(ex2, min=var_floor)
        m1, s1 = mu.reshape(P, L), v1.reshape(P, L)
        kl = 0.5 * (torch.log(v2) - torch.log(s1)) + (s1 + (m1 - m2) ** 2) / (2 * v2) - 0.5
        out.update(mi=mi_w * kl.sum(-1).mean(), leaky_margin=float(pre.detach().abs().min() / pre.detach().abs().max()),
                   clamp2_margin=float(((ex2.detach() - var_floor).abs() / var_floor).min()),
                   below2=float((ex2.detach() < var_floor).double().mean()))
    if ent_w > 0:
        key = F.linear(h.detach(), p["w_key.weight"], p["w_key.bias"]).view(bs, N, 1, D)
        query = F.linear(latent.detach().reshape(bs, N, N, L), p["w_query.weight"], p["w_query.bias"])
        alpha = torch.softmax((key * query).sum(-1), -1)                    # no 1/sqrt(D), no diagonal mask
        ac = torch.clamp(alpha, min=ALPHA_FLOOR)
        out.update(ent=ent_w * (-(ac * torch.log2(ac)).sum(-1).mean()), alpha_margin=float((alpha.detach() - ALPHA_FLOOR).abs().min()),
                   below_alpha=float((alpha.detach() < ALPHA_FLOOR).double().mean()))
    out.update({"running_mean": rm, "running_var": rv, "num_batches_tracked": nbt})
    return out


MARGINS = ("top2_margin", "clamp1_margin", "clamp2_margin", "alpha_margin", "leaky_margin")


def _tensors(state, dtype, grad_prefixes):
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in state.items()}
    names = [k for k in p if k.startswith(grad_prefixes) and not mt.is_buffer(k)]
    for k in names:
        p[k].requires_grad_(True)
    return p, names


def kernel_reference(state, h, return_q, eps, bs, N, test_mode, bn_train, mi_w=KMI_W, ent_w=KENT_W, dtype=torch.float64):
    """one csrc/maic_aux.hip call: dict(mi, ent, dpar (bs*N, 2*N*L) = d mi / d [mean | var], dh = d mi / d h through
    inference_net's input alone, grads {inference_net.*, w_key.*, w_query.*}, buffers {inference_net.1.*}, margins)"""
    p, names = _tensors(state, dtype, AUX_PREFIXES)
    ht = torch.tensor(np.asarray(h), dtype=dtype, requires_grad=True)        # puts mean / var into the graph
    hin = ht.detach().clone().requires_grad_(True)
    e = None if eps is None else torch.tensor(np.asarray(eps), dtype=dtype)
    o = aux(p, ht, torch.tensor(np.asarray(return_q), dtype=dtype), bs, N, test_mode, bn_train, e, mi_w, ent_w, h_infer=hin)
    gs = torch.autograd.grad(o["mi"] + o["ent"], [o["mean"], o["var"], hin] + [p[k] for k in names], allow_unused=True)
    z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()
    res = dict(mi=float(o["mi"].detach()), ent=float(o["ent"].detach()), dh=z(gs[2], hin),
               dpar=np.concatenate([z(gs[0], o["mean"]), z(gs[1], o["var"])], 1),
               grads={k: z(g, p[k]) for k, g in zip(names, gs[3:])},
               buffers={IBN + "running_mean": o["running_mean"].numpy(), IBN + "running_var": o["running_var"].numpy(),
                        IBN + "num_batches_tracked": o["num_batches_tracked"]})
    res.update({k: o[k] for k in MARGINS + ("below2", "below_alpha") if k in o})
    return res


def full_grads(state, h, return_q, eps, bs, N, test_mode, bn_train, mi_w=MI_W, ent_w=ENT_W, dtype=torch.float64):
    """d (mi + ent) / d h (through inference_net's input AND through embed_net) and / d every parameter that receives one"""
    p, names = _tensors(state, dtype, AUX_PREFIXES + ("embed_net.",))
    ht = torch.tensor(np.asarray(h), dtype=dtype, requires_grad=True)
    e = None if eps is None else torch.tensor(np.asarray(eps), dtype=dtype)
    o = aux(p, ht, torch.tensor(np.asarray(return_q), dtype=dtype), bs, N, test_mode, bn_train, e, mi_w, ent_w)
    gs = torch.autograd.grad(o["mi"] + o["ent"], [ht] + [p[k] for k in names], allow_unused=True)
    return dict(mi=float(o["mi"].detach()), ent=float(o["ent"].detach()), dh=gs[0].numpy(),
                grads={k: (np.zeros(tuple(p[k].shape)) if g is None else g.numpy()) for k, g in zip(names, gs[1:])},
                buffers={IBN + "running_mean": o["running_mean"].numpy(), IBN + "running_var": o["running_var"].numpy(),
                         IBN + "num_batches_tracked": o["num_batches_tracked"]})


# ---------------------------------------------------------------------------------------------------- the learner
def train(state, batch, train_step, eps, bn_train=True, mi_w=MI_W, ent_w=ENT_W):
    """one MAICTDLearner.train call with the two weights on a maic_train_oracle.State: (loss float, grads before the clip,
    intermediates with mi_sum / ent_sum = the sums over the transition indices and the margins)"""
    args, dt = state.args, state.dtype
    loss, inter = mt.q_forward(state, batch, eps, bn_train)
    T = inter["T"]
    bt = {k: (v if k == "u" else v.to(dt)) for k, v in learners.to_tensors(batch, T).items()}
    B, N, H = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim
    h0 = torch.zeros(B * N, H, dtype=dt)
    _, hs, _ = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(bt["u_onehot"]), h0, args.last_action, args.reuse_network)
    q = inter["q_evals"].detach()
    e = torch.tensor(np.asarray(eps["cur"]), dtype=dt)[:, :T]
    margins = {k: float("inf") for k in MARGINS}
    mi_sum = ent_sum = 0.0

    def call(h, rq, ee, bs):
        nonlocal mi_sum, ent_sum
        o = aux({**state.agent, **state.bn}, h, rq, bs, N, False, bn_train, ee, mi_w, ent_w, var_floor=args.var_floor)
        for k in ("running_mean", "running_var"):
            state.bn[IBN + k] = o[k].detach()
        state.bn[IBN + "num_batches_tracked"] = torch.tensor(float(o["num_batches_tracked"]), dtype=dt)
        for k in MARGINS:
            margins[k] = min(margins[k], o[k])
        return o["mi"], o["ent"]
    if bn_train:
        for t in range(T):
            mi, ent = call(hs[:, t].reshape(B * N, -1), q[:, t].reshape(B * N, -1), e[:, t].reshape(B * N, -1), B)
            mi_sum, ent_sum = mi_sum + mi, ent_sum + ent
    else:                     # one call over all B*T environments: T times its losses is the sum over the indices
        mi, ent = call(hs.reshape(B * T * N, -1), q.reshape(B * T * N, -1), e.reshape(B * T * N, -1), B * T)
        mi_sum, ent_sum = T * mi, T * ent
    total = loss + (mi_sum + ent_sum) / T
    grads = learners._grads(state, total)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef, mi_sum=float(mi_sum.detach()), ent_sum=float(ent_sum.detach()), td=float(loss.detach()),
                 aux_margins=margins)
    return float(total.detach()), grads, inter


# ---------------------------------------------------------------------------------------------------- the kernel cases
SHAPES = {"2s3z": (5, 11), "MMM2": (10, 18), "n2a3": (2, 3), "n16a32": (16, 32)}
# (name, shape, bs, clamped).  2s3z bs 8: three environments per tile, ragged last tile; MMM2 bs 37 (37 tiles) and 2s3z bs 70 (24)
# go through the 16-slice merge; n2a3 bs 9: eight environments per tile, the smallest pair count per environment; n16a32 bs 2: the
# shape limits, one environment per tile; clamped: both clamps of the two losses populated on both sides
KERNEL_SHAPES = [("2s3z_bs8", "2s3z", 8, False), ("MMM2_bs37", "MMM2", 37, False), ("2s3z_bs70", "2s3z", 70, False),
                 ("n2a3_bs9", "n2a3", 9, False), ("n16a32_bs2", "n16a32", 2, False), ("clamped", "2s3z", 8, True)]
KERNEL_CASES = [c + (bn,) for c in KERNEL_SHAPES for bn in (False, True)]
# (name, batch statistics) -> data seed: the first from 1 on at which every margin of the case clears 1e-5 by a factor of 1.3.
# MMM2 at bs 37 holds 236 800 inference_net pre-activations (LEAKY_BUDGET below): its seeds are far out.
KERNEL_SEED = {("2s3z_bs8", False): 2, ("2s3z_bs8", True): 2, ("MMM2_bs37", False): 7045, ("MMM2_bs37", True): 1193,
               ("2s3z_bs70", False): 911, ("2s3z_bs70", True): 267, ("n2a3_bs9", False): 1, ("n2a3_bs9", True): 1,
               ("n16a32_bs2", False): 7, ("n16a32_bs2", True): 3, ("clamped", False): 12, ("clamped", True): 3}
WEIGHT_SEED = 1
KEY_SCALE, KEY_SCALE_CLAMPED = 0.03, 1.0
LEAKY_BUDGET = 200000        # inference_net pre-activations (pairs x 64) above which a case favours a few greedy actions


def kernel_case_id(c):
    return "%s_%s" % (c[0], "batch" if c[4] else "eval")


def shape_args(shape):
    N, A = SHAPES[shape]
    a = mo.maic_args("2s3z")
    a.n_agents, a.n_actions = N, A
    a.mi_loss_weight, a.entropy_loss_weight = MI_W, ENT_W
    return a


def kernel_case_inputs(case, seed=None):
    """(args, state, h, return_q, eps) of a kernel case"""
    name, shape, bs, clamped, bn = case
    seed = KERNEL_SEED.get((name, bn), 1) if seed is None else seed
    args = shape_args(shape)
    N, A = args.n_agents, args.n_actions
    state = mo.maic_state(args, seed=WEIGHT_SEED, scale=3.0)
    # the entropy term's logits carry no 1 / sqrt(D): at the weight scale of the other layers more than half of the alphas lie
    # under 1e-4 and, over a few thousand rows, some within 1e-5 of it.  The clamped case wants exactly that; the others damp w_key
    for k in ("w_key.weight", "w_key.bias"):
        state[k] = state[k] * (KEY_SCALE_CLAMPED if clamped else KEY_SCALE)
    if clamped:               # inference_net's variance outputs pushed under log(var_floor) for half of the latents
        state["inference_net.3.bias"][mo.L:mo.L + mo.L // 2] -= 6.0
    rng = np.random.default_rng(500 + seed)
    R = bs * N
    h = (0.5 * rng.standard_normal((R, 64))).astype(np.float32)
    q = rng.standard_normal((R, A)).astype(np.float32)
    eps = rng.standard_normal((R, N * mo.L)).astype(np.float32)
    if bs * N * N * mo.NH > LEAKY_BUDGET:
        # a pair's pre-activation is decided by (sender, greedy action of the receiver): with the greedy actions spread over all A
        # the case holds bs * N * A * 64 distinct ones, too many for a smooth density to leave none under 1e-5 of the maximum at any
        # seed within reach.  Four favoured actions cut that to a quarter; the other cases keep the spread
        q[:, :4] += 1.5
    return args, state, h, q, eps


# ---------------------------------------------------------------------------------------------------- the combined backward
# marl_maic_head_bwd_ex: the TD pairs and the MI term's plane through ONE embed_net backward.  (kernel case, seed of the data and of
# the pairs: the first from 1 on that clears the margins of both parts by a factor of 1.3)
COMBINED_CASES = [(KERNEL_SHAPES[0] + (False,), 3), (KERNEL_SHAPES[0] + (True,), 3)]
COMBINED_DQ = 2.0


def combined_inputs(ccase):
    """(u_act, dq_val) of a combined case: a third of the rows carries no TD pair - an action index out of range or a zero value"""
    case, seed = ccase
    args = shape_args(case[1])
    R = case[2] * args.n_agents
    rng = np.random.default_rng(900 + seed)
    u_act = rng.integers(0, args.n_actions, R).astype(np.int32)
    dq_val = (COMBINED_DQ * rng.standard_normal(R)).astype(np.float32)     # the TD part no larger than the MI part
    u_act[0::6] = -1
    dq_val[3::6] = 0.0
    return u_act, dq_val


def combined_reference(ccase, dtype=torch.float64):
    """dict(dh = d (TD pairs + mi + ent) / d h without the part through inference_net's input (the aux kernel's own output),
    grads {embed_net.*, msg_net.*}: what head_bwd_ex must produce given the aux kernel's plane; leaky / clamp margins of the TD part)"""
    case, _ = ccase
    args, state, h, q, eps = kernel_case_inputs(case, seed=ccase[1])
    N, bs, bn = args.n_agents, case[2], case[4]
    u_act, dq_val = combined_inputs(ccase)
    G = np.zeros(q.shape)
    ok = u_act >= 0
    G[np.arange(len(u_act))[ok], u_act[ok]] = dq_val[ok]
    q0 = np.zeros_like(q)     # the head's backward does not read q
    td = mt.head_grads(state, h, q0, eps, None, None, bs, N, False, bn, dtype=dtype, G=G)
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in state.items()}
    with torch.no_grad():
        val = torch.tensor(dq_val * ok, dtype=dtype)
        clamp, leaky = mt.head_margins(p, torch.tensor(h, dtype=dtype), {k: torch.tensor(v) if isinstance(v, np.ndarray) else v
                                                                           for k, v in td["out"].items()}, bs, N, bn, val)
    full = full_grads(state, h, q, eps, bs, N, False, bn, mi_w=KMI_W, ent_w=KENT_W, dtype=dtype)
    ker = kernel_reference(state, h, q, eps, bs, N, False, bn, dtype=dtype)
    grads = {k: td["grads"][k] + full["grads"].get(k, 0.0) for k in td["grads"] if k.startswith(("embed_net.", "msg_net."))}
    return dict(dh=td["dh"] + full["dh"] - ker["dh"], grads=grads, dpar=ker["dpar"], clamp_margin=clamp, leaky_margin=leaky,
                aux_margins={k: ker[k] for k in MARGINS}, aux_share=float(np.abs(full["dh"] - ker["dh"]).max() / np.abs(td["dh"]).max()))


# ---------------------------------------------------------------------------------------------------- the update cases
# (name, alg, agent in training mode): 2s3z, B = 4, T = 4, one episode ending early (its padded steps count), double_q on
UPDATE_CASES = [("aux_qmix", "qmix", True), ("aux_vdn", "vdn", True), ("aux_qmix_eval", "qmix", False)]
UPDATE_SEED = {"aux_qmix": 2, "aux_vdn": 5, "aux_qmix_eval": 8}    # the first seeds that clear every margin by 1.3
UB, UT, ULEN = 4, 4, [4, 2, 4, 4]


def update_case_states(case):
    name, alg, bn_train = case
    args = mo.maic_args("2s3z", episode_limit=UT)
    args.alg, args.double_q = alg, True
    args.mi_loss_weight, args.entropy_loss_weight = MI_W, ENT_W
    seed = UPDATE_SEED[name]
    agent = mo.maic_state(args, seed=seed, scale=1.0)
    mshapes = seeded.mixer_param_shapes(args)
    mixer = seeded.seeded_state(mshapes, seed=seed + 1) if mshapes else {}
    return args, agent, mixer


def update_case_data(case, batch_seed=100):
    args, _, _ = update_case_states(case)
    batch = seeded.make_batch(args, UB, seed=batch_seed, lengths=ULEN)
    rng = np.random.default_rng(batch_seed + 7)
    N = args.n_agents
    eps = {k: rng.standard_normal((UB, UT, N, N * mo.L)).astype(np.float32) for k in ("cur", "next_eval", "next_target")}
    return batch, eps


def reference_updates(case, steps=2, weights=(MI_W, ENT_W)):
    """``steps`` consecutive updates of a case (train_step 0, 1, ..) in float64 and in float32: two lists of dicts with loss, td,
    mi_sum, ent_sum, T, grads, grad_norm, params after the step, bn_eval / bn_target and the margins"""
    args, agent, mixer = update_case_states(case)
    batch, eps = update_case_data(case)
    out = []
    for dt in (torch.float64, torch.float32):
        st = mt.State(args, agent, mixer, dtype=dt)
        res = []
        for ts in range(steps):
            loss, grads, inter = train(st, learners.clone_batch(batch), ts, eps, bn_train=case[2], mi_w=weights[0], ent_w=weights[1])
            named = dict(st.named_params())
            g = {n: (grads[n].numpy() if grads[n] is not None else np.zeros(tuple(named[n].shape))) for n in grads}
            res.append(dict(loss=loss, td=inter["td"], mi_sum=inter["mi_sum"], ent_sum=inter["ent_sum"], T=inter["T"], grads=g,
                            grad_norm=inter["grad_norm"], params={n: p.detach().numpy().copy() for n, p in named.items()},
                            bn_eval={k: v.numpy().copy() for k, v in st.bn.items()},
                            bn_target={k: v.numpy().copy() for k, v in st.target_bn.items()},
                            selection_margin=inter["selection_margin"], clamp_margin=inter["clamp_margin"],
                            leaky_margin=inter["leaky_margin"], aux_margins=inter["aux_margins"]))
        out.append(res)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------- bounds
TOL = mt.TOL
MARGIN = 1e-5


def is_zero_gradient(name, bn_batch):
    """maic_train_oracle.is_zero_gradient, and under batch statistics inference_net.0.bias as well: BatchNorm subtracts the
    column mean of the pair rows, so the bias in front of it has no effect"""
    n = name[len("agent."):] if name.startswith("agent.") else name
    return mt.is_zero_gradient(name, bn_batch) or (bn_batch and n == "inference_net.0.bias")


def bound_scale(name, bn_batch, ref64, ref32):
    """maic_train_oracle.bound_scale with this module's list of analytically zero gradients"""
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    base = float(np.abs(ref64).max()) if ref64.size else 0.0
    if not is_zero_gradient(name, bn_batch):
        return base
    err32 = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    return max(base, 4.0 * err32 / TOL)


def follows_a_free_bias(name, bn_batch, step):
    """Under batch statistics embed_net.0.bias and inference_net.0.bias have no effect and an analytically zero gradient, so the
    optimizer moves them by the rounding of that gradient: a walk of up to 10 lr per step that float32 and float64 take differently
    (maic_train_oracle.step_is_decided).  Nothing the networks compute sees it - except the running_mean behind each bias, which
    from the second update on (step >= 1) carries the difference."""
    return bool(bn_batch) and step >= 1 and name in (mo.BN + "running_mean", IBN + "running_mean")


def buffer_scale(name, bn_batch, step, ref64, ref32):
    """the ``scale`` of a BatchNorm buffer's bound: max |ref|, and for the running means that follow a free bias 4 x the float32
    oracle's own error where that is more"""
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    base = float(np.abs(ref64).max())
    if not follows_a_free_bias(name, bn_batch, step):
        return base
    return max(base, 4.0 * float(np.abs(ref32 - ref64).max()) / TOL)
