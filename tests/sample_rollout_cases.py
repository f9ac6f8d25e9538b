"""Cases and float64 checks of the sampled rollouts (TEST INFRASTRUCTURE; tests/test_sample_rollout_cpu.py and
tests/test_gpu_sample_rollout.py): the whole-rollout kernel and the fused step drawing their actions from the stochastic policy.

* ``CASES``         the smallest shapes at which each mechanism of the sampling choice block can go wrong
* ``step_check``    the per-step float64 check of a record: its observations and previous actions through the float64 agent,
                    then policy_oracle.sample (the float64 CDF) - the synthetic observations do not depend on the actions, so
                    every step is checked on its own
* ``prefix_clean``  cells whose row made no near-boundary draw so far
* ``rollout64``     a float64 sampled rollout from oracle.rollout.SynthSMAC, oracle.nets and policy_oracle.sample
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import nets, seeded
from oracle import rollout as orl
import policy_oracle as po

SHAPES = {"2s3z": (5, 80, 120, 11), "MMM2": (10, 176, 322, 18), "a16": (16, 64, 100, 16), "a32": (4, 180, 50, 32),
          "n49": (49, 40, 60, 5), "n1": (1, 8, 10, 3)}
ENV_SEED, ENV0, RSEED, AGENT_SEED = 5, 2, 77, 11


def _case(name, shape, E, T, eps=0.3, scale="episode", anneal=0.01, last_action=True, wscale=1.0, why=""):
    return dict(name=name, shape=shape, E=E, T=T, eps=eps, scale=scale, anneal=anneal, last_action=last_action, wscale=wscale, why=why)


# (N, O, S, A), E, T: what the case exercises.  The epsilon variants of 2s3z E = 37 anneal per step (0.03 a step: the kernel's
# fp64 schedule runs); "sharp" scales the agent's weights until logit gaps pass 80 (the exponent clamp, w_k underflow at eps = 0)
CASES = (
    _case("2s3z-e0", "2s3z", 37, 8, eps=0.0, scale="step", anneal=0.03, why="EPW = 1, 5 valid rows in a 16-row tile; eps = 0"),
    _case("2s3z-e03", "2s3z", 37, 8, eps=0.3, scale="step", anneal=0.03, why="the fp64 schedule"),
    _case("2s3z-e1", "2s3z", 37, 8, eps=1.0, scale="step", anneal=0.03, why="eps = 1: the uniform policy over the available actions"),
    _case("2s3z-sharp", "2s3z", 37, 8, eps=0.0, scale="step", anneal=0.03, wscale=40.0, why="logit gaps past 80: clamp, underflow"),
    _case("2s3z-700", "2s3z", 700, 5, why="EPW = 3, 15 of 16 rows; the last workgroup holds one env"),
    _case("2s3z-noact", "2s3z", 37, 8, last_action=False, why="no one-hot feed"),
    _case("a16", "a16", 300, 5, why="a full 16-lane action group"),
    _case("MMM2", "MMM2", 37, 6, why="AC = 2, 18 of 32 lanes"),
    _case("a32", "a32", 300, 5, why="AC = 2, all 32 lanes"),
    _case("n49", "n49", 23, 6, why="one env across four row tiles"),
    _case("n1", "n1", 700, 5, why="one-agent envs; rows with one available action"),
)
CASE_IDS = [c["name"] for c in CASES]


def make_args(c, **over):
    N, O, S, A = SHAPES[c["shape"]]
    kw = dict(n_agents=N, obs_shape=O, state_shape=S, n_actions=A, seed=RSEED, epsilon=c["eps"], anneal_epsilon=c["anneal"],
              min_epsilon=0.02, epsilon_anneal_scale=c["scale"], last_action=c["last_action"], map=c["shape"])
    kw.update(over)
    return po.make_args("2s3z", c["T"], **kw)


def agent_weights(c, args):
    return seeded.seeded_state(seeded.agent_param_shapes(args), seed=AGENT_SEED, scale=c["wscale"])


def eps_schedule(args, eps, T):
    """(epsilon of each lock-step of one training rollout that starts from ``eps``, epsilon after it): the host loop of
    RolloutWorker, in Python floats"""
    if args.epsilon_anneal_scale == "episode":
        eps = eps - args.anneal_epsilon if eps > args.min_epsilon else eps
        return [eps] * T, eps
    out = []
    for _ in range(T):
        out.append(eps)
        eps = eps - args.anneal_epsilon if eps > args.min_epsilon else eps
    return out, eps


def _fed(u, A, last_action):
    """the one-hot fed at step t: zeros at t = 0, the action of t - 1 after (zeros where it is -1)"""
    E, T, N = u.shape
    oh = np.zeros((E, T, N, A))
    np.put_along_axis(oh, np.maximum(u, 0)[..., None], (u >= 0)[..., None].astype(np.float64), axis=3)
    return nets.shifted_onehot(torch.tensor(oh))


def step_check(record, agent64, args, eps_of_t, rseed, env):
    """record: an EpisodeRecord (device or host tensors); agent64: float64 torch weights; eps_of_t: T epsilons; env: an object
    with env0 and global_step(t).  Returns (wanted actions (E, T, N) int64 with -1 on padding, float64 margins (E, T, N),
    live (E, T) bool)"""
    T, N, A, H = record.T, record.N, record.A, args.rnn_hidden_dim
    u = record.u.cpu().numpy().astype(np.int64)
    length = record.length.cpu().numpy()
    E = u.shape[0]
    obs, avail = record.obs.cpu().numpy()[:, :T], record.avail.cpu().numpy()[:, :T]
    live = np.arange(T)[None] < length[:, None]
    with torch.no_grad():
        logits, _, _ = nets.agent_unroll(agent64, torch.tensor(obs, dtype=torch.float64), _fed(u, A, args.last_action),
                                         torch.zeros(E * N, H, dtype=torch.float64), args.last_action, args.reuse_network)
    logits = logits.numpy()
    want = np.full((E, T, N), -1, np.int64)
    margin = np.full((E, T, N), np.inf)
    for t in range(T):
        w, m, _ = po.sample(logits[:, t], avail[:, t], live[:, t], eps_of_t[t], rseed, env.env0, env.global_step(t))
        want[:, t], margin[:, t] = w, m
    margin[~live] = np.inf
    return want, margin, live


def prefix_clean(margin, live):
    """(E, T, N) bool: cell (e, t, n) is clean iff every draw of row (e, n) at steps <= t has margin >= SAMPLER_EXCLUDE (draws of
    padded steps do not count: there are none)"""
    near = (np.asarray(margin) < po.SAMPLER_EXCLUDE) & np.asarray(live)[..., None]
    return np.cumsum(near, axis=1) == 0


class OracleEnv:
    """env0 / global_step of the device environment, for po.sample"""

    def __init__(self, T, env0=ENV0, episode=0):
        self.T, self.env0, self.episode = T, env0, episode

    def global_step(self, t):
        return self.episode * (self.T + 1) + t


def rollout64(c, episode=0, rseed=RSEED, env0=ENV0):
    """The sampled training rollout of case ``c`` in float64: SynthSMAC's observations and availability (fp32 values, exact),
    the float64 agent, po.sample.  Returns dict(u (E,T,N) with -1 on padding, margin (E,T,N), live (E,T), r (E,T) float32,
    gap = the largest max - min of a live row's logits)"""
    args = make_args(c)
    N, O, S, A = SHAPES[c["shape"]]
    E, T, H = c["E"], c["T"], args.rnn_hidden_dim
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in agent_weights(c, args).items()}
    sy = orl.SynthSMAC(N, O, S, A, T, seed=ENV_SEED)
    env, ep = np.arange(env0, env0 + E), np.full(E, episode)
    L = sy.length(env, ep)
    eps_of_t, _ = eps_schedule(args, args.epsilon, T)
    u = np.full((E, T, N), -1, np.int64)
    margin = np.full((E, T, N), np.inf)
    r = np.zeros((E, T), np.float32)
    live = np.arange(T)[None] < L[:, None]
    h = torch.zeros(E * N, H, dtype=torch.float64)
    last = torch.zeros(E, N, A, dtype=torch.float64)
    oe = OracleEnv(T, env0, episode)
    gap = 0.0
    with torch.no_grad():
        for t in range(T):
            o_t, a_t = sy.obs(env, ep, t), sy.avail(env, ep, t)
            lv = live[:, t]
            o_t = np.where(lv[:, None, None], o_t, 0.0)           # padded steps feed zeros
            inp = nets.build_inputs(torch.tensor(o_t, dtype=torch.float64), last, N, args.last_action, args.reuse_network)
            q, h = nets.agent_step(p, inp, h)
            act, m, _ = po.sample(q.view(E, N, A).numpy(), a_t, lv, eps_of_t[t], rseed, env0, oe.global_step(t))
            z = q.view(E, N, A).numpy()[lv]
            gap = max(gap, float((z.max(-1) - z.min(-1)).max())) if z.size else gap
            u[:, t] = act
            margin[:, t] = np.where(lv[:, None], m, np.inf)
            r[lv, t] = sy.reward(env, ep, t, np.maximum(act, 0))[lv]
            last = torch.zeros(E, N, A, dtype=torch.float64)
            last.scatter_(2, torch.tensor(np.maximum(act, 0))[..., None], torch.tensor((act >= 0)[..., None].astype(np.float64)))
    return dict(u=u, margin=margin, live=live, r=r, gap=gap)
