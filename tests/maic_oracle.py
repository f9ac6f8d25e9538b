"""Float64 restatement of the MAIC agent for the tests (TEST INFRASTRUCTURE, written for this project):

* ``maic_state``      seeded weights with MAICAgent's state-dict keys (reference network/MAIC.py:19-47)
* ``head``            MAICAgent.forward after fc2 (:58-87), every intermediate returned, BatchNorm in either mode
* ``forward``         the whole forward (agent step + head)
* ``hash_noise``      the standard-normal draws of a sampled-latent rollout step (csrc/maic_head.hip: marl_maic_noise)
* ``serial_rollout``  a reference-style serial loop over SerialSynthEnv that calls ``forward`` once per step (bs = 1)
* ``batched_rollout`` the lock-step rollout of E environments with the head, epsilon-greedy draws as oracle/rollout.py
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import seeded, nets
from oracle import rollout as orl

L, NH, D, VAR_FLOOR = 8, 64, 32, 0.002
BN_EPS, BN_MOM = 1e-5, 0.1
ST_MAIC_EPS = 8
SHAPES = {"2s3z": (5, 80, 11), "3s5z": (8, 128, 14), "MMM2": (10, 176, 18), "matrix": (2, 1, 3)}
MAIC_SEED = 0
BN = "embed_net.1."


def maic_args(shape, **over):
    if shape == "matrix":
        a = seeded.make_args("2s3z", "qmix", **over)
        a.n_agents, a.obs_shape, a.n_actions, a.state_shape, a.map = 2, 1, 3, 1, "MatrixGame"
    else:
        a = seeded.make_args(shape, "qmix", **over)
    a.latent_dim, a.nn_hidden_size, a.var_floor, a.attention_dim = L, NH, VAR_FLOOR, D
    a.MAIC = True
    return a


def key_shapes(args):
    """state-dict keys and shapes of MAICAgent, in the reference's order"""
    H, N, A = args.rnn_hidden_dim, args.n_agents, args.n_actions
    I = args.obs_shape + (A if args.last_action else 0) + (N if args.reuse_network else 0)
    bn = lambda p: [(p + ".weight", (NH,)), (p + ".bias", (NH,)), (p + ".running_mean", (NH,)), (p + ".running_var", (NH,)),
                    (p + ".num_batches_tracked", ())]
    lin = lambda p, o, i: [(p + ".weight", (o, i)), (p + ".bias", (o,))]
    return (lin("embed_net.0", NH, H) + bn("embed_net.1") + lin("embed_net.3", N * L * 2, NH)
            + lin("inference_net.0", NH, H + A) + bn("inference_net.1") + lin("inference_net.3", L * 2, NH)
            + lin("fc1", H, I) + [("rnn.weight_ih", (3 * H, H)), ("rnn.weight_hh", (3 * H, H)), ("rnn.bias_ih", (3 * H,)),
                                  ("rnn.bias_hh", (3 * H,))]
            + lin("fc2", A, H) + lin("msg_net.0", NH, H + L) + lin("msg_net.2", A, NH) + lin("w_key", D, H) + lin("w_query", D, L))


def maic_state(args, seed=MAIC_SEED, scale=3.0):
    """float32 numpy state dict: Linear / GRU tensors torch-default-like times ``scale`` (oracle.seeded), BatchNorm tensors
    away from their defaults so both modes are exercised"""
    shapes = key_shapes(args)
    dense = [(k, s) for k, s in shapes if ".1." not in k or not k.split(".")[0].endswith("_net")]
    out = seeded.seeded_state(dense, seed=seed, scale=scale)
    rng = np.random.default_rng(seed + 1000)
    for p in ("embed_net.1", "inference_net.1"):
        out[p + ".weight"] = rng.uniform(0.5, 1.5, NH).astype(np.float32)
        out[p + ".bias"] = rng.uniform(-0.5, 0.5, NH).astype(np.float32)
        out[p + ".running_mean"] = (0.5 * rng.standard_normal(NH)).astype(np.float32)
        out[p + ".running_var"] = rng.uniform(0.5, 2.0, NH).astype(np.float32)
        out[p + ".num_batches_tracked"] = np.array(3, dtype=np.int64)
    return {k: out[k] for k, _ in shapes}


def p64(state):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in state.items()}


def head(p, h, q, bs, N, test_mode, bn_train, eps=None, var_floor=VAR_FLOOR):
    """p: float64 tensors; h (bs*N, 64), q (bs*N, A) = fc2(h).  Returns a dict: return_q, mean, var, latent (bs*N, N*L),
    alpha (bs, N, N) after the gate, msg (bs, N, N, A) and running_mean / running_var / num_batches_tracked after the call."""
    lk = lambda t: F.leaky_relu(t, 0.01)
    y = F.linear(h, p["embed_net.0.weight"], p["embed_net.0.bias"])
    rm, rv, nbt = p[BN + "running_mean"].clone(), p[BN + "running_var"].clone(), int(p[BN + "num_batches_tracked"])
    if bn_train:
        R = y.shape[0]
        mean, var = y.mean(0), y.var(0, unbiased=False)
        rm = (1 - BN_MOM) * rm + BN_MOM * mean
        rv = (1 - BN_MOM) * rv + BN_MOM * var * R / (R - 1)
        nbt += 1
    else:
        mean, var = rm, rv
    z = lk((y - mean) / torch.sqrt(var + BN_EPS) * p[BN + "weight"] + p[BN + "bias"])
    par = F.linear(z, p["embed_net.3.weight"], p["embed_net.3.bias"])
    NL = N * L
    mu, v = par[:, :NL], torch.clamp(torch.exp(par[:, NL:]), min=var_floor)
    latent = mu if test_mode else mu + torch.sqrt(v) * eps
    lat = latent.reshape(bs, N, N, L)                                         # [b, i, j]
    hj = h.view(bs, 1, N, -1).expand(bs, N, N, h.shape[-1])                   # [b, i, j] = h of agent j
    hid = lk(F.linear(torch.cat([hj, lat], -1), p["msg_net.0.weight"], p["msg_net.0.bias"]))
    msg = F.linear(hid, p["msg_net.2.weight"], p["msg_net.2.bias"])           # (bs, N, N, A)
    key = F.linear(h, p["w_key.weight"], p["w_key.bias"]).view(bs, N, 1, -1) / np.sqrt(D)
    query = F.linear(lat, p["w_query.weight"], p["w_query.bias"])             # (bs, N, N, D)
    logits = (key * query).sum(-1)
    logits = torch.where(torch.eye(N, dtype=torch.bool)[None], torch.full_like(logits, -1e9), logits)
    alpha = torch.softmax(logits, -1)
    if test_mode:
        alpha = torch.where(alpha < 0.25 / N, torch.zeros_like(alpha), alpha)
    rq = q + (alpha[..., None] * msg).sum(1).reshape(bs * N, -1)
    return dict(return_q=rq, mean=mu, var=v, latent=latent, alpha=alpha, msg=msg, running_mean=rm, running_var=rv,
                num_batches_tracked=nbt)


def forward(p, inputs, h0, bs, N, test_mode, bn_train, eps=None):
    q, h = nets.agent_step(p, inputs, h0)
    out = head(p, h, q, bs, N, test_mode, bn_train, eps)
    out["h"], out["q"] = h, q
    return out


def hash_noise(rseed, env, tg, N):
    """(len(env), N, N*L) float32: Box-Muller over draws 2k, 2k+1 (k = n*N*L + c) of stream ST_MAIC_EPS"""
    env = np.asarray(env).reshape(-1, 1)
    tg = np.asarray(tg).reshape(-1, 1)
    k = np.arange(N * N * L)[None]
    u1 = orl.u01(orl.key(rseed, ST_MAIC_EPS, env, tg, 2 * k))
    u2 = orl.u01(orl.key(rseed, ST_MAIC_EPS, env, tg, 2 * k + 1))
    z = np.sqrt(np.float32(-2.0) * np.log(np.float32(1.0) - u1)) * np.cos(np.float32(6.283185307179586) * u2)
    return z.astype(np.float32).reshape(-1, N, N * L)


def step_inputs(args, obs, last):
    """obs (E, N, O), last (E, N, A) one-hot -> (E*N, I)"""
    E, N = obs.shape[0], args.n_agents
    parts = [obs] + ([last] if args.last_action else []) + ([np.broadcast_to(np.eye(N), (E, N, N))] if args.reuse_network else [])
    return np.concatenate(parts, -1).reshape(E * N, -1)


def serial_rollout(forward_fn, args, env, n_episodes):
    """greedy serial episodes: per step ONE forward over the N agents of the environment (bs = 1, test mode) through
    ``forward_fn(inputs (N, I) float64 tensor, h (N, 64)) -> (q (N, A), h)``; the record keys of RolloutWorker"""
    N, A, T = args.n_agents, args.n_actions, args.episode_limit
    out = {k: [] for k in ("o", "u", "r", "avail_u", "padded", "terminated", "qmax_gap")}
    rewards, wins, steps = [], [], 0
    for _ in range(n_episodes):
        env.reset()
        h = torch.zeros(N, args.rnn_hidden_dim, dtype=torch.float64)
        last = np.zeros((1, N, A))
        o, u, r, av, pad, te, gaps = [], [], [], [], [], [], []
        term, step, ep_r, win = False, 0, 0.0, False
        while not term and step < T:
            obs, avail = np.array(env.get_obs(), dtype=np.float64), np.array(env.get_avail_actions())
            q, h = forward_fn(torch.tensor(step_inputs(args, obs[None], last)), h)
            q = q.detach().numpy().astype(np.float64).copy()
            scale = np.abs(q).max()
            q[avail == 0] = -np.inf
            acts = q.argmax(-1)
            srt = np.sort(q, -1)
            gaps.append(np.min(np.where(np.isfinite(srt[:, -2]), srt[:, -1] - srt[:, -2], np.inf)) / scale)
            last = np.eye(A)[acts][None]
            rew, term, info = env.step(list(acts))
            win = bool(term and info.get("battle_won", False))
            o.append(obs); u.append(acts.reshape(N, 1)); r.append([rew]); av.append(avail); pad.append([0.0]); te.append([float(term)])
            ep_r += rew
            step += 1
        for _i in range(step, T):
            o.append(np.zeros((N, args.obs_shape))); u.append(np.zeros((N, 1))); r.append([0.0]); av.append(np.zeros((N, A)))
            pad.append([1.0]); te.append([1.0])
        for k, v in zip(("o", "u", "r", "avail_u", "padded", "terminated"), (o, u, r, av, pad, te)):
            out[k].append(np.array(v, dtype=np.float64))
        out["qmax_gap"].append(min(gaps))
        rewards.append(ep_r); wins.append(win); steps += step
    ep = {k: np.stack(v, 0) for k, v in out.items()}
    return ep, rewards, wins, steps


def batched_rollout(state, args, synth, n_envs, epsilon, evaluate, rseed=0, bn_train=False):
    """lock-step rollout of oracle.rollout.batched_rollout with the MAIC head: test mode = evaluate, sampled latents from
    ``hash_noise``; epsilon fixed over the rollout (anneal_epsilon = 0 in the tests).  Returns u (E, T, N) and padded (E, T)."""
    p = p64(state)
    N, A, T = args.n_agents, args.n_actions, args.episode_limit
    E = n_envs
    env, ep = np.arange(E), np.zeros(E, dtype=np.int64)
    Ls = synth.length(env, ep)
    u = np.zeros((E, T, N), np.int64)
    pad = np.ones((E, T), np.float64)
    h = torch.zeros(E * N, args.rnn_hidden_dim, dtype=torch.float64)
    last = np.zeros((E, N, A))
    eps_g = 0.0 if evaluate else epsilon
    with torch.no_grad():
        for t in range(T):
            alive = t < Ls
            if not alive.any():
                break
            o_t, a_t = synth.obs(env, ep, t).astype(np.float64), synth.avail(env, ep, t)
            tg = synth.tg(ep, t)
            noise = None if evaluate else torch.tensor(hash_noise(rseed, env, tg, N).reshape(E * N, -1), dtype=torch.float64)
            # finished environments keep stepping (their rows count in the batch statistics): slot L still holds the final
            # observation, later slots are zeros, and the last action of a padded step reads as "none"
            o_in = np.where((t <= Ls)[:, None, None], o_t, 0.0)
            out = forward(p, torch.tensor(step_inputs(args, o_in, last)), h, E, N, evaluate, bn_train, noise)
            h = out["h"]
            q = out["return_q"].numpy().reshape(E, N, A).copy()
            q[a_t == 0] = -np.inf
            greedy = q.argmax(-1)
            explore = orl.u01(orl.key(rseed, orl.ST_EXPLORE, env[:, None], tg[:, None], np.arange(N)[None])) < np.float32(eps_g)
            navail = a_t.sum(-1).astype(np.int64)
            k = np.floor(orl.u01(orl.key(rseed, orl.ST_PICK, env[:, None], tg[:, None], np.arange(N)[None]))
                         * navail.astype(np.float32)).astype(np.int64)
            k = np.minimum(k, navail - 1)
            pick = (np.cumsum(a_t, -1) <= k[..., None]).sum(-1)
            act = np.where(explore, pick, greedy)
            u[alive, t] = act[alive]
            pad[alive, t] = 0.0
            last = np.where(alive[:, None, None], np.eye(A)[act], 0.0)
    return u, pad
