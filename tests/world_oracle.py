"""CPU restatement of the world-model agent's head and prediction loss (TEST INFRASTRUCTURE; reference
network/world_model.py:7-75, algorithm/q_learner_state.py:94-187).

``head`` is the WorldModel forward in the dtype of its arguments (float64 wherever a kernel is judged; ``params_t`` converts
the weights, ``pre_activations`` returns the two ReLU inputs); ``head_backward`` its gradients by autograd, in float64 unless
told otherwise, for a given gradient on r (the TD loss reaching q = fc2(h) + r) and on o_hat (the prediction loss).  ``train`` restates QLearnerWithState.train on the
oracle's LearnerState (oracle/learners.py) with the agent's world.* tensors in ``state.agent``: the q_forward schedule with
r added to every Q tensor, plus mean((o_next - o_hat)^2) from the eval pass."""
from __future__ import annotations

import numpy as np
import torch

from oracle import learners, nets

WORLD = ("world.hidden_embd.0", "world.hidden_embd.2", "world.r_out", "world.o_out", "world.terminate_out")


def world_param_shapes(args):
    """WorldModel (world_model.py:12-19) parameter shapes, in registration order"""
    H, A, O = args.rnn_hidden_dim, args.n_actions, args.obs_shape
    out = []
    for name, n_out in zip(WORLD, (H, H, A, O, 2)):
        out += [(name + ".weight", (n_out, H)), (name + ".bias", (n_out,))]
    return out


def head(p, h):
    """(r, o_hat, tau) of hidden states h (..., 64): e = relu(W2 relu(W1 h + b1) + b2) (world_model.py:33)"""
    lin = lambda x, n: x @ p[n + ".weight"].T + p[n + ".bias"]
    e = torch.relu(lin(torch.relu(lin(h, WORLD[0])), WORLD[1]))
    return lin(e, WORLD[2]), lin(e, WORLD[3]), lin(e, WORLD[4])


def params_t(p, dtype=torch.float64):
    """the world.* tensors of a numpy state dict in `dtype` (float64: the reference; float32: the yardstick)"""
    return {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in p.items() if k.startswith("world.")}


def pre_activations(p, h):
    """the two ReLU inputs of `head`, (W1 h + b1, W2 z + b2): where a caller counts values near the kink at 0"""
    lin = lambda x, n: x @ p[n + ".weight"].T + p[n + ".bias"]
    zp = lin(h, WORLD[0])
    return zp, lin(torch.relu(zp), WORLD[1])


def head_backward(p, h, dr, dohat, dtype=torch.float64):
    """gradients of sum(r * dr) + sum(o_hat * dohat), computed in `dtype` (float64 unless told): (dh, {param name: grad})"""
    p64 = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in p.items()
           if k.startswith("world.")}
    h64 = torch.tensor(np.asarray(h), dtype=dtype, requires_grad=True)
    r, ohat, _ = head(p64, h64)
    obj = (r * torch.as_tensor(np.asarray(dr), dtype=dtype)).sum() + \
        (ohat * torch.as_tensor(np.asarray(dohat), dtype=dtype)).sum()
    names = list(p64)
    gs = torch.autograd.grad(obj, [h64] + [p64[n] for n in names], allow_unused=True)
    return gs[0].numpy(), {n: (g.numpy() if g is not None else np.zeros(p64[n].shape)) for n, g in zip(names, gs[1:])}


def q_forward(state, batch, T=None):
    """learners.q_forward with q + r everywhere and the prediction loss (q_learner_state.py:94-183)"""
    args = state.args
    if T is None:
        T = learners.max_episode_len(batch["terminated"], args.episode_limit)
    bt = learners.to_tensors(batch, T)
    B, N, H = bt["o"].shape[0], args.n_agents, args.rnn_hidden_dim
    s, u, r, s_next = bt["s"], bt["u"], bt["r"], bt["s_next"]
    avail_u, avail_next, term, u_onehot = bt["avail_u"], bt["avail_u_next"], bt["terminated"], bt["u_onehot"]
    mask = 1.0 - bt["padded"]
    la, ru = args.last_action, args.reuse_network
    h0 = torch.zeros(B * N, H)
    q_evals, hs_eval, h_last = nets.agent_unroll(state.agent, bt["o"], nets.shifted_onehot(u_onehot), h0, la, ru)
    r_e, ohat, tau = head(state.agent, hs_eval)
    q_evals = q_evals + r_e
    q_chosen = torch.gather(q_evals, 3, u).squeeze(3)
    with torch.no_grad():
        q_tgt, hs_tgt, _ = nets.agent_unroll(state.target_agent, bt["o_next"], u_onehot, h0, la, ru)
        q_tgt = (q_tgt + head(state.target_agent, hs_tgt)[0]).clone()
        q_tgt[avail_next == 0.0] = learners.MASK_BIG
        if args.double_q:
            q_en, hs_en, _ = nets.agent_unroll(state.agent, bt["o_next"], u_onehot, h_last.detach(), la, ru)
            q_en = (q_en + head(state.agent, hs_en)[0]).clone()
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
                at = nets.qplex(state.target_mixer, q_tgt_chosen, s_next, args, actions=onehot,
                                max_q_i=q_tgt.max(dim=3)[0], is_v=False)
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
    loss_td = ((mask * td) ** 2).sum() / mask.sum()
    loss_pred = ((bt["o_next"] - ohat) ** 2).mean()
    loss = loss_td + loss_pred
    return loss, dict(T=T, q_evals=q_evals, hs_eval=hs_eval, ohat=ohat, tau=tau, loss_td=loss_td, loss_pred=loss_pred,
                      den=mask.sum())


def train(state, batch, train_step):
    """one QLearnerWithState.train call: (loss float, grads before the clip, intermediates)"""
    loss, inter = q_forward(state, batch)
    grads = learners._grads(state, loss)
    norm, coef = learners.clip_and_step(state, grads)
    if train_step > 0 and train_step % state.args.target_update_cycle == 0:
        state.sync_targets()
    inter.update(grad_norm=norm, clip_coef=coef)
    return float(loss.detach()), grads, inter


# (name, shape, alg, B, T, lengths, overrides): ragged lengths with an unterminated episode (-1) so padded steps carry weight
CASES = [
    ("world_qmix_2s3z", "2s3z", "qmix", 4, 6, [5, 3, -1, 4], {}),
    ("world_qplex_2s3z", "2s3z", "qplex", 4, 6, [6, 3, -1, 4], {}),
    ("world_vdn_2s3z_nodq", "2s3z", "vdn", 3, 5, [3, -1, 4], {"double_q": False}),
    ("world_qmix_MMM2", "MMM2", "qmix", 3, 5, [5, -1, 4], {}),
    ("world_qmix_2s3z_nolast", "2s3z", "qmix", 3, 5, [5, -1, 3], {"last_action": False}),
    ("world_qmix_2s3z_noreuse", "2s3z", "qmix", 3, 5, [-1, 4, 2], {"reuse_network": False}),
]
TRAIN_STEPS = [0, 1, 200, 201]   # 200 crosses the target-sync boundary (world.* included)
WORLD_SEED = 15


def serial_agent_state(args):
    """the weights of the serial-rollout fixture: seeded agent and world.* at scale 3 (decisive greedy choices)"""
    from oracle import seeded
    sd = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11, scale=3.0)
    sd.update(seeded.seeded_state(world_param_shapes(args), seed=WORLD_SEED, scale=3.0))
    return sd


def case_states(case):
    """seeded numpy weights: (args, agent incl. world.*, mixer)"""
    from oracle import seeded
    name, shape, alg, B, T, lengths, over = case
    args = seeded.make_args(shape, alg, episode_limit=T, **over)
    agent = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11)
    agent.update(seeded.seeded_state(world_param_shapes(args), seed=WORLD_SEED))
    mshapes = seeded.mixer_param_shapes(args)
    mixer = seeded.seeded_state(mshapes, seed=12) if mshapes else {}
    return args, agent, mixer


def build_oracle_state(case):
    args, agent, mixer = case_states(case)
    return args, learners.LearnerState(args, agent, mixer)
