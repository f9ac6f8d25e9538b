"""Torch-CPU restatement of the RTW reflection head (reference network/RTW.py:70-203), TEST INFRASTRUCTURE.

Written from the formulas, not from the reference's code: a row is agent i of one environment (act mode) or of one
(episode, t) (given mode); j runs over the N agents of that environment.
  act   : t_j = T2 relu(T0 [h_i ; e_j] + b) + b (self input zeroed), a_j = first argmax with unavailable at -1e9,
          m_j = onehot(a_j) (self zeroed), o_hat = W2 relu(W0 [o_i ; m_0..m_{N-1}] + b) + b, query = Wq [o_i ; o_hat] + bq,
          s_j = (query / 8) . (Wk m_j + bk) (self at -1e9), p = softmax(s), v_j = V2 relu(V0 [h_i ; m_j] + b) + b,
          q_i += sum_j p_j v_j
  given : m_j = onehot(u_j) (self zeroed), o_hat -> the real o_next, and v_j from h_j (RTW.py:122 h_repeat[b,i,j] = h[b,j])
The parameters are dicts name -> tensor with RTWAgent's state_dict keys; act_head, given_head and _reflect compute in the dtype
of their inputs (params_t(sd, torch.float64) and float64 inputs give the float64 statement the kernel tests compare against).  Also: the batched lock-step RTW rollout, a copy
of oracle.rollout.batched_rollout with the head between the agent step and the selection.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets
from oracle.rollout import key, u01, ST_EXPLORE, ST_PICK


def _lin(p, name, x):
    return F.linear(x, p[name + ".weight"], p[name + ".bias"])


def _mlp(p, name, x):
    return _lin(p, name + ".2", torch.relu(_lin(p, name + ".0", x)))


def params_t(sd, dtype=torch.float32):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in sd.items()}


def _reflect(p, h_val, o, o2, m, N, not_self):
    """h_val (G,N,N,H): h feeding v_j of row i; o, o2 (G,N,O); m (G,N,N,A) one-hot blocks (self already zeroed)."""
    G = o.shape[0]
    query = _lin(p, "w_q", torch.cat([o, o2], -1)) / 8.0                  # (G,N,64)
    keyv = _lin(p, "w_k", m)                                              # (G,N,N,64)
    s = (query.unsqueeze(2) * keyv).sum(-1)                               # (G,N,N)
    if not_self:
        s = s.clone()
        idx = torch.arange(N)
        s[:, idx, idx] = -1e9
    pr = torch.softmax(s, -1)
    v = _mlp(p, "w_v", torch.cat([h_val, m], -1))                         # (G,N,N,A)
    return (pr.unsqueeze(-1) * v).sum(2)                                  # (G,N,A)


def act_head(p, h, o, avail, N, not_self=True):
    """h (G*N,H), o (G*N,O), avail (G,N,A) -> q_r (G*N,A), o_hat (G*N,O), a (G*N,N), gap (G*N,N): gap = top-2 margin of
    the masked teammate logits (how robust each a_j is to rounding)."""
    G = h.shape[0] // N
    H, O, A = h.shape[1], o.shape[1], avail.shape[-1]
    hr = h.view(G, N, 1, H).expand(G, N, N, H)
    e = torch.eye(N, dtype=h.dtype).view(1, 1, N, N).expand(G, N, N, N)
    x = torch.cat([hr, e], -1).clone()
    if not_self:
        idx = torch.arange(N)
        x[:, idx, idx] = 0.0
    t = _mlp(p, "teammate_net", x)                                        # (G,N,N,A)
    av = avail.view(G, 1, N, A).expand(G, N, N, A)
    tm = torch.where(av == 0.0, torch.full_like(t, -1e9), t)
    a = tm.argmax(-1)                                                     # first index of the maximum
    top2 = tm.topk(min(2, A), -1).values
    gap = (top2[..., 0] - top2[..., 1]) if A > 1 else torch.full_like(top2[..., 0], float("inf"))
    m = F.one_hot(a, A).to(h.dtype)
    if not_self:
        idx = torch.arange(N)
        m[:, idx, idx] = 0.0
    og = o.view(G, N, O)
    ohat = _mlp(p, "world_net", torch.cat([og, m.reshape(G, N, N * A)], -1))
    qr = _reflect(p, hr, og, ohat, m, N, not_self)
    return qr.reshape(G * N, A), ohat.reshape(G * N, O), a.reshape(G * N, N), gap.reshape(G * N, N)


def given_head(p, hs, o, on, u, N, not_self=True):
    """hs (G*N,H), o / on (G*N,O), u (G*N,) taken actions -> q_r (G*N,A)."""
    G = hs.shape[0] // N
    H, O = hs.shape[1], o.shape[1]
    A = p["w_k.weight"].shape[1]
    hr = hs.view(G, 1, N, H).expand(G, N, N, H)                           # row i, teammate j: h_j
    uj = u.view(G, 1, N).expand(G, N, N).clamp(min=0).long()
    m = F.one_hot(uj, A).to(hs.dtype)
    if not_self:
        idx = torch.arange(N)
        m[:, idx, idx] = 0.0
    return _reflect(p, hr, o.view(G, N, O), on.view(G, N, O), m, N, not_self).reshape(G * N, A)


def current_q_values(p, batch, T, args):
    """RTWMAC.get_current_q_values: (q, hs) over the (B,T,...) batch dict (numpy or torch)."""
    tb = {k: torch.as_tensor(np.asarray(batch[k]), dtype=torch.float32) for k in ("o", "o_next", "u_onehot")}
    u = torch.as_tensor(np.asarray(batch["u"])).long()[:, :T]
    o, on, uo = tb["o"][:, :T], tb["o_next"][:, :T], tb["u_onehot"][:, :T]
    B, _, N, O = o.shape
    with torch.no_grad():
        q, hs, _ = nets.agent_unroll(p, o, nets.shifted_onehot(uo), torch.zeros(B * N, 64), args.last_action, args.reuse_network)
        qr = given_head(p, hs.reshape(-1, 64), o.reshape(-1, O), on.reshape(-1, O), u.reshape(-1), N,
                        getattr(args, "not_self_model", True))
    return q + qr.view(q.shape), hs


def batched_rtw_rollout(agent, args, synth, n_envs, epsilon, evaluate=False, rseed=0, env0=0, episode=0):
    """oracle.rollout.batched_rollout with the act-mode head added to q before the selection (same key / u01 streams)."""
    p = params_t(agent)
    not_self = getattr(args, "not_self_model", True)
    N, A, O, S, T, H = args.n_agents, args.n_actions, args.obs_shape, args.state_shape, args.episode_limit, args.rnn_hidden_dim
    E = n_envs
    env = np.arange(env0, env0 + E)
    ep = np.full(E, episode)
    L = synth.length(env, ep)
    obs = np.zeros((E, T + 1, N, O), np.float32); st = np.zeros((E, T + 1, S), np.float32)
    av = np.zeros((E, T + 1, N, A), np.float32)
    u = np.zeros((E, T, N, 1), np.int64); uo = np.zeros((E, T, N, A), np.float32)
    r = np.zeros((E, T, 1), np.float32); term = np.ones((E, T, 1), np.float32); pad = np.ones((E, T, 1), np.float32)
    h = torch.zeros(E * N, H)
    last = np.zeros((E, N, A), np.float32)
    eps = 0.0 if evaluate else epsilon
    if args.epsilon_anneal_scale == "episode":
        eps = eps - args.anneal_epsilon if eps > args.min_epsilon else eps
    eye = np.eye(N, dtype=np.float32)
    with torch.no_grad():
        for t in range(T):
            alive = t < L
            if not alive.any():
                break
            o_t, s_t, a_t = synth.obs(env, ep, t), synth.state(env, ep, t), synth.avail(env, ep, t)
            parts = [o_t] + ([last] if args.last_action else []) + ([np.broadcast_to(eye, (E, N, N))] if args.reuse_network else [])
            inp = np.concatenate(parts, axis=-1).reshape(E * N, -1)
            q, h = nets.agent_step(p, torch.tensor(inp), h)
            qr = act_head(p, h, torch.tensor(o_t).reshape(E * N, O), torch.tensor(a_t), N, not_self)[0]
            q = (q + qr).numpy().reshape(E, N, A).copy()
            q[a_t == 0] = -np.inf
            greedy = q.argmax(-1)
            tg = synth.tg(ep, t)[:, None]
            explore = u01(key(rseed, ST_EXPLORE, env[:, None], tg, np.arange(N)[None])) < np.float32(eps)
            navail = a_t.sum(-1).astype(np.int64)
            k = np.floor(u01(key(rseed, ST_PICK, env[:, None], tg, np.arange(N)[None])) * navail.astype(np.float32)).astype(np.int64)
            k = np.minimum(k, navail - 1)
            csum = np.cumsum(a_t, -1)
            pick = (csum <= k[..., None]).sum(-1)
            act = np.where(explore, pick, greedy)
            rew = synth.reward(env, ep, t, act)
            oh = np.eye(A, dtype=np.float32)[act]
            m = alive
            obs[m, t], st[m, t], av[m, t] = o_t[m], s_t[m], a_t[m]
            u[m, t, :, 0] = act[m]; uo[m, t] = oh[m]; r[m, t, 0] = rew[m]
            pad[m, t, 0] = 0.0
            term[m, t, 0] = (t + 1 >= L[m]).astype(np.float32)
            last = oh
            fin = (t + 1 == L)
            if fin.any():
                obs[fin, t + 1] = synth.obs(env, ep, t + 1)[fin]
                st[fin, t + 1] = synth.state(env, ep, t + 1)[fin]
                av[fin, t + 1] = synth.avail(env, ep, t + 1)[fin]
            if args.epsilon_anneal_scale == "step":
                eps = eps - args.anneal_epsilon if eps > args.min_epsilon else eps
    o, o_n = obs[:, :-1].copy(), obs[:, 1:].copy()
    s, s_n = st[:, :-1].copy(), st[:, 1:].copy()
    a, a_n = av[:, :-1].copy(), av[:, 1:].copy()
    for e in range(E):
        o_n[e, L[e]:] = 0; s_n[e, L[e]:] = 0; a_n[e, L[e]:] = 0
        o[e, L[e]:] = 0; s[e, L[e]:] = 0; a[e, L[e]:] = 0
    episodes = dict(o=o, s=s, u=u, r=r, avail_u=a, o_next=o_n, s_next=s_n, avail_u_next=a_n,
                    u_onehot=uo, padded=pad, terminated=term)
    rewards = [float(r[e, :, 0].sum()) for e in range(E)]
    wins = list(synth.won(env, ep))
    return episodes, rewards, wins, int(L.sum()), (epsilon if evaluate else eps)


def random_rtw_params(args, seed):
    """Seeded RTWAgent state dict (torch default-init scale: U(-1/sqrt(fan_in), 1/sqrt(fan_in)))."""
    rng = np.random.default_rng(seed)
    N, A, O, H = args.n_agents, args.n_actions, args.obs_shape, args.rnn_hidden_dim
    I = O + (A if args.last_action else 0) + (N if args.reuse_network else 0)
    shapes = [("fc1", H, I), ("rnn.weight_ih", 3 * H, H), ("rnn.weight_hh", 3 * H, H), ("fc2", A, H),
              ("teammate_net.0", 64, H + N), ("teammate_net.2", A, 64), ("world_net.0", 64, O + N * A),
              ("world_net.2", O, 64), ("w_q", 64, 2 * O), ("w_k", 64, A), ("w_v.0", 64, H + A), ("w_v.2", A, 64)]
    sd = {}
    for name, n_out, n_in in shapes:
        bnd = 1.0 / np.sqrt(n_in)
        if name.startswith("rnn."):
            bnd = 1.0 / np.sqrt(H)
            sd[name] = rng.uniform(-bnd, bnd, (n_out, n_in)).astype(np.float32)
            sd[name.replace("weight", "bias")] = rng.uniform(-bnd, bnd, (n_out,)).astype(np.float32)
        else:
            sd[name + ".weight"] = rng.uniform(-bnd, bnd, (n_out, n_in)).astype(np.float32)
            sd[name + ".bias"] = rng.uniform(-bnd, bnd, (n_out,)).astype(np.float32)
    order = ["fc1.weight", "fc1.bias", "rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh", "fc2.weight", "fc2.bias"]
    rest = [k for k in sd if k not in order]
    return {k: sd[k] for k in order + rest}
