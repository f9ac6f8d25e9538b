"""Float64 / float32 restatement of the CommNet actor (TEST INFRASTRUCTURE, written for this project: the reference ships the three
+commnet algorithms as an argument table only; the definition is include/marl_hip.h's).  Plain torch with autograd.

* ``gru``            torch's GRUCell formula on a parameter dict
* ``head`` / ``head_published``   the K communication rounds and the decoding layer, written two ways: sum over the group minus the
                     row's own value, times 1 / N - and the published repeat / mask / mean(dim=-2) form
* ``step`` / ``unroll``   one step and the T-step unroll of the whole actor (encoder, f_obs, head)
* ``commnet_actor``  context manager under which tests/policy_oracle.py, pg_oracle.py and coma_oracle.py run their learner forwards
                     with the CommNet actor in the place of RNNQNet: ``policy``, ``log_prob``, ``actor_numerator``, ``critic``, the case
                     tables and the seeds are theirs, imported and not copied
* ``learner_case``   a learner case of one of the three oracles with the actor's parameters swapped for seeded CommNet ones
* ``head_case`` / ``head_reference``   content and float64 results of the head kernel tests
* ``F32_EXCEPTIONS`` float32-oracle errors of the tensors that miss a quarter of 1e-4 max|ref| (tests/test_commnet_cpu.py derives it)
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from oracle import nets, seeded
import policy_oracle as po
import pg_oracle as pg
import coma_oracle as co

H = 64
EPS = po.EPS
LEARNER_CASES = po.LEARNER_CASES
K_OF = {"2s3z": 3, "MMM2": 3, "matrix": 2}       # rounds of the learner cases: get_commnet_args' 3, and 2 on the small matrix game


# ------------------------------------------------------------------------------------------------ the actor
def param_shapes(args):
    """CommNetAgent's state dict in torch's order (published names)"""
    A = args.n_actions
    I = args.obs_shape + (A if args.last_action else 0) + (args.n_agents if args.reuse_network else 0)
    return [("encoding.weight", (H, I)), ("encoding.bias", (H,)),
            ("f_obs.weight_ih", (3 * H, H)), ("f_obs.weight_hh", (3 * H, H)), ("f_obs.bias_ih", (3 * H,)), ("f_obs.bias_hh", (3 * H,)),
            ("f_comm.weight_ih", (3 * H, H)), ("f_comm.weight_hh", (3 * H, H)), ("f_comm.bias_ih", (3 * H,)), ("f_comm.bias_hh", (3 * H,)),
            ("decoding.weight", (A, H)), ("decoding.bias", (A,))]


def seeded_params(args, seed):
    """torch-default-like init from a numpy stream: U(+-1/sqrt(fan_in)) for the Linear layers, U(+-1/sqrt(H)) for both GRU cells"""
    rng = np.random.default_rng(seed)
    shapes = param_shapes(args)
    fan = {"encoding": shapes[0][1][1], "f_obs": H, "f_comm": H, "decoding": H}
    return {k: rng.uniform(-1.0, 1.0, size=shp).astype(np.float32) / np.float32(np.sqrt(fan[k.split(".")[0]])) for k, shp in shapes}


def gru(p, prefix, x, h):
    gi = x @ p[prefix + ".weight_ih"].T + p[prefix + ".bias_ih"]
    gh = h @ p[prefix + ".weight_hh"].T + p[prefix + ".bias_hh"]
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1 - z) * n + z * h


def head(p, h, N, K):
    """h (G N, H) in agent order -> logits (G N, A): the sum-minus-own form"""
    g = gru(p, "f_comm", torch.zeros_like(h), h)
    for _ in range(1, K):
        gg = g.reshape(-1, N, H)
        c = ((gg.sum(dim=1, keepdim=True) - gg) / N).reshape(-1, H)
        g = gru(p, "f_comm", c, g)
    return nets.lin(p, "decoding", g)


def head_published(p, h, N, K):
    """the same in the published form: every agent's hidden state repeated for every agent, the own block zeroed by a mask, then
    mean(dim=-2) over all N blocks (hence the divisor N)"""
    for k in range(K):
        if k == 0:
            c = torch.zeros_like(h)
        else:
            h = h.reshape(-1, N, H)
            c = h.reshape(-1, 1, N * H).repeat(1, N, 1)
            mask = (1 - torch.eye(N, dtype=h.dtype)).view(-1, 1).repeat(1, H).view(N, -1)
            c = (c * mask.unsqueeze(0)).reshape(-1, N, N, H).mean(dim=-2)
            h, c = h.reshape(-1, H), c.reshape(-1, H)
        h = gru(p, "f_comm", c, h)
    return nets.lin(p, "decoding", h)


def step(p, x, h, N, K):
    """x (rows, I), h (rows, H) -> (logits, h_out)"""
    h_out = gru(p, "f_obs", torch.sigmoid(nets.lin(p, "encoding", x)), h)
    return head(p, h_out, N, K), h_out


def unroll(p, obs, fed_onehot, h0, last_action, reuse_network, K):
    """nets.agent_unroll's contract with the CommNet actor: (logits (B,T,N,A), hs (B,T,N,H), h)"""
    B, T, N = obs.shape[:3]
    h, zs, hs = h0, [], []
    for t in range(T):
        z, h = step(p, nets.build_inputs(obs[:, t], fed_onehot[:, t], N, last_action, reuse_network), h, N, K)
        zs.append(z.view(B, N, -1))
        hs.append(h.view(B, N, -1))
    return torch.stack(zs, 1), torch.stack(hs, 1), h


@contextlib.contextmanager
def commnet_actor(K):
    """the three learner oracles call nets.agent_unroll(state.agent, ...) for the actor: under this context a parameter dict with
    CommNet's names takes ``unroll`` above.  Their ReLU-margin probe reads fc1's pre-activations: the CommNet actor has no ReLU
    (sigmoid and tanh have no kink), so the probe is answered with ones - far from any kink."""
    real_unroll, real_lin = nets.agent_unroll, nets.lin

    def agent_unroll(p, obs, fed, h0, last_action=True, reuse_network=True):
        if "encoding.weight" in p:
            return unroll(p, obs, fed, h0, last_action, reuse_network, K)
        return real_unroll(p, obs, fed, h0, last_action, reuse_network)

    def lin(p, prefix, x):
        if prefix == "fc1" and "encoding.weight" in p:
            return torch.ones(x.shape[0], H, dtype=x.dtype)
        return real_lin(p, prefix, x)

    nets.agent_unroll, nets.lin = agent_unroll, lin
    try:
        yield
    finally:
        nets.agent_unroll, nets.lin = real_unroll, real_lin


def learner_case(alg, name, dtype=torch.float64, **over):
    """(args, state, batch(i)) of ``alg`` in ("reinforce", "central_v", "coma") on the shared learner case ``name``: the oracle's own
    case (its critic, its batches, its seeds) with the actor's parameters replaced, in the dict its optimizer half holds, by CommNet
    ones seeded with the case's weight seed + 7; args.k and args.alg are set"""
    mod = {"reinforce": pg, "central_v": po, "coma": co}[alg]
    args, state, batch = mod.learner_case(name, dtype=dtype, **over)
    args.k, args.alg = K_OF[name], alg + "+commnet"
    seed = next(c for c in LEARNER_CASES if c[0] == name)[5] + 7
    w = seeded_params(args, seed)
    state.agent.clear()
    state.agent.update({k: torch.tensor(x, dtype=dtype).clone().requires_grad_(True) for k, x in w.items()})
    return args, state, batch


# ------------------------------------------------------------------------------------------------ the head kernels' content
HEAD_SHAPES = ((1, 2, 3), (7, 3, 9), (37, 5, 11), (64, 8, 14), (37, 10, 18), (5, 2, 30), (601, 5, 11))
HEAD_KS = (1, 2, 3)


def head_case(G, N, A, seed):
    """float32 content of a head kernel test: hidden states in (-1, 1), f_comm and decoding weights at twice torch's init scale and a
    dense dlogits of the size that makes every gradient of order one, about a third of its rows zeroed as padded rows are"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s)
    u = lambda bound, *s: rng.uniform(-bound, bound, size=s)
    c = {"hs": np.tanh(f(G * N, H)), "f_comm.weight_ih": u(0.25, 3 * H, H), "f_comm.weight_hh": u(0.25, 3 * H, H),
         "f_comm.bias_ih": u(0.25, 3 * H), "f_comm.bias_hh": u(0.25, 3 * H), "decoding.weight": u(0.25, A, H),
         "decoding.bias": u(0.25, A)}
    dl = f(G * N, A) / np.sqrt(G * N / 16.0 + 1.0)
    dl[rng.random(G * N) < 1.0 / 3.0] = 0.0
    c["dlogits"] = dl
    return {k: v.astype(np.float32) for k, v in c.items()}


HEAD_PARAMS = ("f_comm.weight_ih", "f_comm.weight_hh", "f_comm.bias_ih", "f_comm.bias_hh", "decoding.weight", "decoding.bias")


def head_reference(c, N, K, dtype=torch.float64):
    """logits, dhs and the six parameter gradients of sum(logits * dlogits), in ``dtype`` from the float32 content as it is"""
    p = {k: torch.tensor(c[k].astype(np.float64), dtype=dtype).requires_grad_(True) for k in HEAD_PARAMS}
    hs = torch.tensor(c["hs"].astype(np.float64), dtype=dtype).requires_grad_(True)
    z = head(p, hs, N, K)
    gs = torch.autograd.grad((z * torch.tensor(c["dlogits"].astype(np.float64), dtype=dtype)).sum(), [hs] + [p[k] for k in HEAD_PARAMS])
    out = {"logits": z.detach().numpy(), "dhs": gs[0].numpy()}
    out.update({k: g.numpy() for k, g in zip(HEAD_PARAMS, gs[1:])})
    return out


# float32-oracle errors (max abs) of the tensors that do not stay under a quarter of 1e-4 * max|ref| on the runs of
# tests/test_gpu_commnet_learner.py; keys as the three oracles' own tables, with the algorithm in front:
#   ("reinforce", case, beta, tensor), ("central_v", case, td_lambda, tensor), ("coma", case, td_lambda, beta, tensor)
# tests/test_commnet_cpu.py derives the table from the two oracles and asserts that this copy holds it.
F32_EXCEPTIONS = {}
RUNS = (tuple(("reinforce", n, b) for n in ("2s3z", "MMM2", "matrix") for b in pg.BETAS)
        + (("central_v", "2s3z", 0.8), ("central_v", "2s3z", 0.0), ("central_v", "2s3z", 1.0), ("central_v", "MMM2", 0.8),
           ("central_v", "matrix", 0.8))
        + (("coma", "2s3z", 0.8, 0.0), ("coma", "MMM2", 0.8, 0.0), ("coma", "matrix", 0.8, 0.0)))
