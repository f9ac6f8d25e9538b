"""Float64 / float32 restatement of the G2ANet actor (TEST INFRASTRUCTURE, written for this project: the reference ships the three
+g2anet algorithms as an argument table only; the definition is include/marl_hip.h's).  Plain torch with autograd.

* ``gru``            torch's GRU formula on a parameter dict (cell ``h``; ``hard_bi_GRU`` with the _l0 / _l0_reverse names)
* ``head`` / ``head_published``   hard attention, soft attention and the decoding layer, written two ways: the factored form
                     W_ih [h_i | h_j] = W_ih[:, :64] h_i + W_ih[:, 64:] h_j with index gathers - and the published loop / stack / view /
                     permute form over the explicitly built (N-1, rows, 128) input
* ``step`` / ``unroll``   one step and the T-step unroll of the whole actor (encoding, h, head)
* ``logistic`` / ``noise``   the noise formula of marl_g2anet_noise on 24-bit draws / on the counter hash (oracle/rollout.py's)
* ``g2anet_actor``   context manager under which tests/policy_oracle.py, pg_oracle.py and coma_oracle.py run their learner forwards with
                     the G2ANet actor in the place of RNNQNet, fed the noise ``noise_fn(step, B, T, N)`` gives
* ``learner_case``   a learner case of one of the three oracles with the actor's parameters swapped for seeded G2ANet ones
* ``head_case`` / ``head_reference``   content and float64 results of the head kernel tests
* ``F32_EXCEPTIONS`` float32-oracle errors of the tensors that miss a quarter of 1e-4 max|ref| (tests/test_g2anet_cpu.py derives it)
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

from oracle import nets
from oracle import rollout as orr
import policy_oracle as po
import pg_oracle as pg
import coma_oracle as co

H, D = 64, 32
TAU = 0.01
EPS = po.EPS
LEARNER_CASES = po.LEARNER_CASES
ST_GUMBEL = 9                            # csrc/synth_env.h: the stream after ST_SAMPLE
UPDATE_SALT = 0x5BD1E995                 # controller/share_params.py: G2ANET_UPDATE_SALT
GRU = "hard_bi_GRU"
HEAD_PARAMS = tuple(GRU + "." + k + s for s in ("_l0", "_l0_reverse") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) + \
    ("hard_encoding.weight", "hard_encoding.bias", "q.weight", "k.weight", "v.weight", "v.bias", "decoding.weight", "decoding.bias")
HARD_PARAMS = HEAD_PARAMS[:10]


# ------------------------------------------------------------------------------------------------ the actor
def param_shapes(args):
    """G2ANetAgent's state dict in torch's order (published names): 22 tensors"""
    A = args.n_actions
    I = args.obs_shape + (A if args.last_action else 0) + (args.n_agents if args.reuse_network else 0)
    gru = [(GRU + "." + k + s, shp) for s in ("_l0", "_l0_reverse")
           for k, shp in (("weight_ih", (3 * H, 2 * H)), ("weight_hh", (3 * H, H)), ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,)))]
    return [("encoding.weight", (H, I)), ("encoding.bias", (H,)),
            ("h.weight_ih", (3 * H, H)), ("h.weight_hh", (3 * H, H)), ("h.bias_ih", (3 * H,)), ("h.bias_hh", (3 * H,))] + gru + \
           [("hard_encoding.weight", (2, 2 * H)), ("hard_encoding.bias", (2,)), ("q.weight", (D, H)), ("k.weight", (D, H)),
            ("v.weight", (D, H)), ("v.bias", (D,)), ("decoding.weight", (A, H + D)), ("decoding.bias", (A,))]


def head_param_shapes(A):
    """the sixteen tensors behind the recurrence, in state-dict order"""
    args = type("A", (), dict(n_actions=A, obs_shape=1, n_agents=2, last_action=False, reuse_network=False))
    return param_shapes(args)[6:]


def seeded_params(args, seed):
    """torch-default-like init from a numpy stream: U(+-1/sqrt(fan_in)) for the Linear layers, U(+-1/sqrt(H)) for the GRUs"""
    rng = np.random.default_rng(seed)
    shapes = param_shapes(args)
    fan = {"encoding": shapes[0][1][1], "h": H, GRU: H, "hard_encoding": 2 * H, "q": H, "k": H, "v": H, "decoding": H + D}
    return {k: rng.uniform(-1.0, 1.0, size=shp).astype(np.float32) / np.float32(np.sqrt(fan[k.split(".")[0]])) for k, shp in shapes}


def gru(p, prefix, x, h, suffix=""):
    gi = x @ p[prefix + ".weight_ih" + suffix].T + p[prefix + ".bias_ih" + suffix]
    gh = h @ p[prefix + ".weight_hh" + suffix].T + p[prefix + ".bias_hh" + suffix]
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1 - z) * n + z * h


def partners(N):
    """(N, N-1) long: row i = the agents j != i in agent order"""
    return torch.tensor([[j for j in range(N) if j != i] for i in range(N)], dtype=torch.long)


def _gate_point(gi, gh, h):
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1 - z) * n + z * h


def hard_weights(p, h, noise, N, tau):
    """w (G, N, N-1) in the factored form: per direction P = W_ih[:, :64] h + b_ih and Q = W_ih[:, 64:] h once per row"""
    hg = h.reshape(-1, N, H)
    G = hg.shape[0]
    part = partners(N)
    states = []
    for suffix, order in (("_l0", range(N - 1)), ("_l0_reverse", range(N - 2, -1, -1))):
        W = p[GRU + ".weight_ih" + suffix]
        P = hg @ W[:, :H].T + p[GRU + ".bias_ih" + suffix]
        Q = hg @ W[:, H:].T
        s = torch.zeros(G, N, H, dtype=h.dtype)
        out = [None] * (N - 1)
        for pos in order:
            gh = s @ p[GRU + ".weight_hh" + suffix].T + p[GRU + ".bias_hh" + suffix]
            s = _gate_point(P + Q[:, part[:, pos]], gh, s)
            out[pos] = s
        states.append(torch.stack(out, 2))                       # (G, N, N-1, H)
    y = torch.cat(states, -1) @ p["hard_encoding.weight"].T + p["hard_encoding.bias"]
    l = torch.zeros(G, N, N - 1, dtype=h.dtype) if noise is None else noise.reshape(G, N, N - 1)
    return torch.sigmoid((y[..., 1] - y[..., 0] + l) / tau)


def head(p, h, noise, N, hard=True, tau=TAU, with_w=False):
    """h (G N, H) in agent order, noise (G N, N-1) or None -> logits (G N, A): the factored form"""
    hg = h.reshape(-1, N, H)
    G = hg.shape[0]
    part = partners(N)
    w = hard_weights(p, h, noise, N, tau) if hard else torch.ones(G, N, N - 1, dtype=h.dtype)
    q, k, v = hg @ p["q.weight"].T, hg @ p["k.weight"].T, torch.relu(hg @ p["v.weight"].T + p["v.bias"])
    a = torch.softmax((q.unsqueeze(2) * k[:, part]).sum(-1) / math.sqrt(D), dim=-1)
    x = ((a * w).unsqueeze(-1) * v[:, part]).sum(2)
    z = nets.lin(p, "decoding", torch.cat([hg, x], -1).reshape(G * N, H + D))
    return (z, w) if with_w else z


def head_published(p, h, noise, N, hard=True, tau=TAU):
    """the same in the published form: the pair inputs built by loops, stack, view and permute, torch-style sequence GRUs over the
    explicit (N-1, rows, 128) input, column 1 of softmax((y + gumbel) / tau) written as the softmax over [y_0, y_1 + l], and the soft
    attention agent by agent"""
    size = h.shape[0]
    hh = h.reshape(-1, N, H)
    if hard:
        input_hard = []
        for i in range(N):
            h_i = hh[:, i]
            h_hard_i = [torch.cat([h_i, hh[:, j]], dim=-1) for j in range(N) if j != i]
            input_hard.append(torch.stack(h_hard_i, dim=0))
        input_hard = torch.stack(input_hard, dim=-2).view(N - 1, -1, 2 * H)
        fwd, s = [], torch.zeros(size, H, dtype=h.dtype)
        for t in range(N - 1):
            s = gru(p, GRU, input_hard[t], s, "_l0")
            fwd.append(s)
        bwd, s = [None] * (N - 1), torch.zeros(size, H, dtype=h.dtype)
        for t in range(N - 2, -1, -1):
            s = gru(p, GRU, input_hard[t], s, "_l0_reverse")
            bwd[t] = s
        h_hard = torch.cat([torch.stack(fwd, 0), torch.stack(bwd, 0)], -1).permute(1, 0, 2).reshape(-1, 2 * H)
        y = nets.lin(p, "hard_encoding", h_hard)
        l = torch.zeros(size * (N - 1), dtype=h.dtype) if noise is None else noise.reshape(-1)
        hw = torch.softmax(torch.stack([y[:, 0], y[:, 1] + l], -1) / tau, dim=-1)
        hw = hw[:, 1].view(-1, N, 1, N - 1).permute(1, 0, 2, 3)
    else:
        hw = torch.ones(N, size // N, 1, N - 1, dtype=h.dtype)
    q = (h @ p["q.weight"].T).reshape(-1, N, D)
    k = (h @ p["k.weight"].T).reshape(-1, N, D)
    v = torch.relu(nets.lin(p, "v", h)).reshape(-1, N, D)
    x = []
    for i in range(N):
        q_i = q[:, i].view(-1, 1, D)
        k_i = torch.stack([k[:, j] for j in range(N) if j != i], dim=0).permute(1, 2, 0)
        v_i = torch.stack([v[:, j] for j in range(N) if j != i], dim=0).permute(1, 2, 0)
        soft = torch.softmax(torch.matmul(q_i, k_i) / math.sqrt(D), dim=-1)
        x.append((v_i * soft * hw[i]).sum(dim=-1))
    x = torch.stack(x, dim=1).reshape(-1, D)
    return nets.lin(p, "decoding", torch.cat([h, x], dim=-1))


def step(p, x, h, noise, N, hard=True, tau=TAU):
    """x (rows, I), h (rows, H), noise (rows, N-1) -> (logits, h_out)"""
    h_out = gru(p, "h", torch.relu(nets.lin(p, "encoding", x)), h)
    return head(p, h_out, noise, N, hard, tau), h_out


def unroll(p, obs, fed_onehot, h0, noise, last_action, reuse_network, hard=True, tau=TAU):
    """nets.agent_unroll's contract with the G2ANet actor and noise (B,T,N,N-1) or None: (logits (B,T,N,A), hs (B,T,N,H), h)"""
    B, T, N = obs.shape[:3]
    h, zs, hs = h0, [], []
    for t in range(T):
        z, h = step(p, nets.build_inputs(obs[:, t], fed_onehot[:, t], N, last_action, reuse_network), h,
                    None if noise is None else noise[:, t].reshape(B * N, N - 1), N, hard, tau)
        zs.append(z.view(B, N, -1))
        hs.append(h.view(B, N, -1))
    return torch.stack(zs, 1), torch.stack(hs, 1), h


# ------------------------------------------------------------------------------------------------ the noise
def logistic(k):
    """l = ln(u) - ln(1 - u), u = (k + 0.5) / 2^24, of 24-bit draws k: float64"""
    u = (np.asarray(k, dtype=np.float64) + 0.5) / 16777216.0
    return np.log(u) - np.log(1.0 - u)


def noise(seed, env0, tg0, E, T, N):
    """marl_g2anet_noise in numpy: (E, T, N, N-1) float64"""
    e = np.arange(E, dtype=np.int64).reshape(E, 1, 1)
    t = np.arange(T, dtype=np.int64).reshape(1, T, 1)
    i = np.arange(N * (N - 1), dtype=np.int64).reshape(1, 1, -1)
    U = lambda x: (np.asarray(x, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    h = orr.key(int(seed) & 0xFFFFFFFF, ST_GUMBEL, U(env0 + e), U(tg0 + t), U(i))
    return logistic(h >> np.uint32(8)).reshape(E, T, N, N - 1)


def update_noise(args, step, B, T, N):
    """what G2ANetMAC draws for update ``step``: float32, as the device stores it"""
    return noise(getattr(args, "seed", 0) ^ UPDATE_SALT, 0, step * args.episode_limit, B, T, N).astype(np.float32)


class Actor:
    """what ``g2anet_actor`` yields: set ``step`` to the update the next forward belongs to"""

    def __init__(self, noise_fn, hard, tau):
        self.noise_fn, self.hard, self.tau, self.step = noise_fn, hard, tau, 0


@contextlib.contextmanager
def g2anet_actor(noise_fn, hard=True, tau=TAU):
    """the three learner oracles call nets.agent_unroll(state.agent, ...) for the actor: under this context a parameter dict with
    G2ANet's names takes ``unroll`` above on the noise ``noise_fn(actor.step, B, T, N)`` (B, T, N, N-1).  Their ReLU-margin probe reads
    fc1's pre-activations: here those are ``encoding``'s."""
    real_unroll, real_lin = nets.agent_unroll, nets.lin
    actor = Actor(noise_fn, hard, tau)

    def agent_unroll(p, obs, fed, h0, last_action=True, reuse_network=True):
        if "hard_encoding.weight" in p:
            B, T, N = obs.shape[:3]
            l = torch.tensor(np.asarray(actor.noise_fn(actor.step, B, T, N), dtype=np.float64), dtype=obs.dtype) if actor.hard else None
            return unroll(p, obs, fed, h0, l, last_action, reuse_network, actor.hard, actor.tau)
        return real_unroll(p, obs, fed, h0, last_action, reuse_network)

    def lin(p, prefix, x):
        if prefix == "fc1" and "hard_encoding.weight" in p:
            return real_lin(p, "encoding", x)
        return real_lin(p, prefix, x)

    nets.agent_unroll, nets.lin = agent_unroll, lin
    try:
        yield actor
    finally:
        nets.agent_unroll, nets.lin = real_unroll, real_lin


# with this shift no pre-activation of encoding's ReLU that carries a gradient lies within 1e-5 of zero in either update of any run or
# controller case (tests/test_g2anet_cpu.py asserts the count)
SEED_SHIFT = 16


def learner_case(alg, name, dtype=torch.float64, hard=True, **over):
    """(args, state, batch(i)) of ``alg`` in ("reinforce", "central_v", "coma") on the shared learner case ``name``: the oracle's own
    case (its critic, its batches, its seeds) with the actor's parameters replaced, in the dict its optimizer half holds, by G2ANet
    ones seeded with the case's weight seed + SEED_SHIFT; args.hard, args.attention_dim and args.alg are set"""
    mod = {"reinforce": pg, "central_v": po, "coma": co}[alg]
    args, state, batch = mod.learner_case(name, dtype=dtype, **over)
    args.hard, args.attention_dim, args.alg = hard, D, alg + "+g2anet"
    seed = next(c for c in LEARNER_CASES if c[0] == name)[5] + SEED_SHIFT
    w = seeded_params(args, seed)
    state.agent.clear()
    state.agent.update({k: torch.tensor(x, dtype=dtype).clone().requires_grad_(True) for k, x in w.items()})
    return args, state, batch


# ------------------------------------------------------------------------------------------------ the head kernels' content
HEAD_SHAPES = ((1, 2, 3), (64, 2, 3), (7, 3, 9), (37, 5, 11), (64, 8, 14), (37, 10, 18), (5, 2, 30), (601, 5, 11))
MANY_TILES = ((2000, 5, 11), (600, 10, 18))
EXTRA_NA = ((2, 3), (3, 9), (5, 11), (8, 14), (10, 18))
HEAD_MODES = ((True, 0.01), (True, 1.0), (False, 0.01), (False, 1.0))       # (hard, tau)
# seeds of the tiny cases at which at least two pairs have w inside (1e-3, 1 - 1e-3) at tau = 0.01 and every gradient reaches 0.02 in
# every mode (tests/test_g2anet_cpu.py asserts both for every case); every other case: 1000 + 7 G + N
HEAD_SEEDS = {(1, 2, 3): 5907, (64, 2, 3): 1, (5, 2, 30): 44, (17, 2, 3): 1, (11, 3, 9): 45}
# exactly zero at N = 2, on both sides: a single step from a zero state never reads W_hh, and a softmax over one partner has no
# gradient, so q and k receive none
ZERO_AT_N2 = (GRU + ".weight_hh_l0", GRU + ".weight_hh_l0_reverse", "q.weight", "k.weight")


def head_seed(G, N, A):
    return HEAD_SEEDS.get((G, N, A), 1000 + 7 * G + N)


def head_case(G, N, A, seed):
    """float32 content of a head kernel test (CommNet's recipe): hidden states in (-1, 1), weights uniform +-0.25, a dense dlogits of
    the size that makes every gradient of order one with about a third of its rows zeroed as padded rows are, and the noise formula on
    a seeded stream of 24-bit draws"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s)
    u = lambda *s: rng.uniform(-0.25, 0.25, size=s)
    c = {"hs": np.tanh(f(G * N, H))}
    for k, shp in head_param_shapes(A):
        c[k] = u(*shp)
    dl = f(G * N, A) / np.sqrt(G * N / 16.0 + 1.0)
    dl[rng.random(G * N) < 1.0 / 3.0] = 0.0
    c["dlogits"] = dl
    c["noise"] = logistic(rng.integers(0, 1 << 24, size=(G * N, N - 1)))
    return {k: v.astype(np.float32) for k, v in c.items()}


def head_reference(c, N, hard=True, tau=TAU, dtype=torch.float64):
    """logits, w, dhs and the sixteen parameter gradients of sum(logits * dlogits), in ``dtype`` from the float32 content as it is
    (hard off: the ten hard tensors get zeros)"""
    p = {k: torch.tensor(c[k].astype(np.float64), dtype=dtype).requires_grad_(True) for k in HEAD_PARAMS}
    hs = torch.tensor(c["hs"].astype(np.float64), dtype=dtype).requires_grad_(True)
    z, w = head(p, hs, torch.tensor(c["noise"].astype(np.float64), dtype=dtype), N, hard, tau, with_w=True)
    gs = torch.autograd.grad((z * torch.tensor(c["dlogits"].astype(np.float64), dtype=dtype)).sum(), [hs] + [p[k] for k in HEAD_PARAMS],
                             allow_unused=True)
    out = {"logits": z.detach().numpy(), "w": w.detach().numpy(), "dhs": gs[0].numpy()}
    out.update({k: (np.zeros(p[k].shape) if g is None else g.numpy()) for k, g in zip(HEAD_PARAMS, gs[1:])})
    return out


def all_head_cases():
    """every (G, N, A, hard, tau) the GPU head tests compare against float64"""
    shapes = list(HEAD_SHAPES) + list(MANY_TILES)
    return [s + m for s in shapes for m in HEAD_MODES]


# ------------------------------------------------------------------------------------------------ the controller's content
MAC_CASES = tuple((name, flags) for name in ("2s3z", "MMM2") for flags in (True, False))


def mac_reference(name, flags, noise_fn, dtype=torch.float64):
    """G2ANetMAC.unroll + .backward on batch 0 of the ragged learner case ``name`` with last_action = reuse_network = ``flags``:
    (args, state, batch, dict of logits and hs under m and the 22 gradients of sum(logits * dl)), dl a seeded normal under m.
    ``noise_fn(B, T, N)``: the update's noise (B, T, N, N-1)"""
    from oracle import learners
    args, state, batch = learner_case("reinforce", name, dtype, last_action=flags, reuse_network=flags)
    b = batch(0)
    T = learners.max_episode_len(b["terminated"], args.episode_limit)
    bt = {k: torch.tensor(np.asarray(v)[:, :T], dtype=torch.long if k == "u" else dtype) for k, v in b.items()}
    B, N = bt["o"].shape[0], args.n_agents
    fed = nets.shifted_onehot(bt["u_onehot"])
    l = torch.tensor(np.asarray(noise_fn(B, T, N), dtype=np.float64), dtype=dtype)
    z, hs, _ = unroll(state.agent, bt["o"], fed, torch.zeros(B * N, H, dtype=dtype), l, args.last_action, args.reuse_network, True, TAU)
    m = (1.0 - bt["padded"]).reshape(B, T, 1, 1)
    dl = torch.tensor(np.random.default_rng(11).standard_normal((B, T, N, args.n_actions)), dtype=dtype) * m
    names = list(state.agent)
    gs = torch.autograd.grad((z * dl).sum(), [state.agent[k] for k in names])
    out = {"logits": (z * m).detach().numpy(), "hs": (hs * m).detach().numpy()}
    out.update({"grad " + k: g.numpy() for k, g in zip(names, gs)})
    return args, state, b, dl, out


# float32-oracle errors (max abs) of the tensors that do not stay under a quarter of 1e-4 * max|ref|.  Keys:
#   ("head", G, N, A, hard, tau, tensor) for the head cases and ("mac", case, flags, tensor) for the controller cases of
#   tests/test_gpu_g2anet.py, and for the runs of
#   tests/test_gpu_g2anet_learner.py the three oracles' own, with the algorithm in front:
#   ("reinforce", case, beta, tensor), ("central_v", case, td_lambda, tensor), ("coma", case, td_lambda, beta, tensor)
# tests/test_g2anet_cpu.py derives the table from the two oracles and asserts that this copy holds it.
F32_EXCEPTIONS = {
    ('head', 37, 5, 11, True, 0.01, 'hard_bi_GRU.bias_ih_l0'): 4.16e-06,
    ('head', 37, 5, 11, True, 0.01, 'hard_bi_GRU.bias_hh_l0'): 3.56e-06,
    ('head', 37, 5, 11, True, 0.01, 'hard_bi_GRU.bias_ih_l0_reverse'): 5.61e-06,
    ('head', 37, 5, 11, True, 0.01, 'hard_bi_GRU.bias_hh_l0_reverse'): 4.07e-06,
    ('head', 37, 5, 11, True, 0.01, 'hard_encoding.bias'): 1.65e-05,
    ('head', 37, 10, 18, True, 0.01, 'dhs'): 4.33e-05,
    ('head', 37, 10, 18, True, 0.01, 'hard_bi_GRU.weight_hh_l0'): 1.62e-05,
    ('head', 37, 10, 18, True, 0.01, 'hard_bi_GRU.bias_hh_l0'): 8.95e-06,
    ('head', 37, 10, 18, True, 0.01, 'hard_bi_GRU.weight_hh_l0_reverse'): 1.63e-05,
    ('head', 37, 10, 18, True, 0.01, 'hard_bi_GRU.bias_ih_l0_reverse'): 1.85e-05,
    ('head', 37, 10, 18, True, 0.01, 'hard_bi_GRU.bias_hh_l0_reverse'): 1.36e-05,
    ('head', 37, 10, 18, True, 0.01, 'hard_encoding.bias'): 3.27e-05,
    ('head', 5, 2, 30, True, 0.01, 'hard_encoding.bias'): 8.17e-06,
    ('head', 2000, 5, 11, True, 0.01, 'hard_encoding.bias'): 8.18e-05,
    ('head', 600, 10, 18, True, 0.01, 'hard_encoding.bias'): 1.02e-05,
    ('head', 3, 10, 18, True, 0.01, 'hard_bi_GRU.weight_ih_l0_reverse'): 1.23e-06,
}
RUNS = ((("reinforce", "2s3z", 0.0), ("reinforce", "2s3z", 0.01), ("reinforce", "MMM2", 0.0), ("reinforce", "matrix", 0.0))
        + (("central_v", "2s3z", 0.8), ("central_v", "MMM2", 0.8), ("central_v", "matrix", 0.8))
        + (("coma", "2s3z", 0.8, 0.0), ("coma", "MMM2", 0.8, 0.0), ("coma", "matrix", 0.8, 0.0)))
