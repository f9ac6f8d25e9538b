"""Seeded cases of the RTW and world-model head kernels at every edge of their support (TEST INFRASTRUCTURE), shared by
tests/test_head_cases_cpu.py - which asserts the seed conditions and the float32 yardstick - and tests/test_gpu_head_edges.py.

Shapes (N, O, A) come from the kernels' launch code and support limits (csrc/rtw_head.hip, csrc/world_head.hip: one wave per
16-row tile, 16-column output tiles, N <= 16, A <= 32, O <= 256):
    (1, 1, 1)       smallest supported shape
    (1, 80, 11)     16 environments per RTW tile, ordinary O and A
    (2, 1, 3)       the matrix game
    (3, 17, 17)     15 live rows; O and A one past a 16-column tile; O % 4 != 0 (ldo = round4(O) != O)
    (5, 80, 11)     2s3z
    (7, 15, 16)     14 live rows; O one short of a tile; A exactly one tile
    (8, 128, 14)    3s5z
    (10, 176, 18)   MMM2; one environment per tile with six dead rows
    (16, 256, 32)   every maximum
    (16, 255, 32)   O one short of the maximum; O % 4 == 3
RTW row counts, with EPT = 16 // N environments per tile: G in {1, EPT - 1, EPT, EPT + 1, 3 EPT + 1} (act mode), and in given
mode B >= 3 episodes of T steps with T no multiple of EPT, so tiles straddle episodes.  World row counts R = B T N reach
1, 15, 16, 17, 4096 (256 loss partials) and the first R above 4096 the shape allows (257 partials: the reduce kernel's strided
loop takes a second trip); the N = 1 shapes use exactly those with T = 1, the controllers' form.  marl_linear_wgrad gives
the four weight-gradient calls (M = R, N = 64 / A / O, K = 64) one slab up to 512 rows and 8 or 16 slabs ("full", "thin" or
"generic" family) at the 4096-row cases, so no extra case is needed for a second plan (asserted on the CPU).

Everything the contract says is not read is NaN: the other slots of (T+1)-slot storage, stored episodes the map does not name
and - world head - steps t >= ep_len[b] of a mapped episode.  (The int32 action plane cannot hold a NaN: its unread slots hold
2^30, which the kernel's clamp would turn into action A - 1.)

Seeds are chosen for conditions, not for results: every top-two margin of the masked teammate logits of an RTW act case is at
least 1e-4 in float64 (a single available action, or none, has no runner-up and counts as satisfied), and no ReLU
pre-activation of a world case lies within 1e-5 of 0 in float64.  tests/test_head_cases_cpu.py asserts both."""
from __future__ import annotations

import types

import numpy as np
import torch

from oracle import seeded
import rtw_oracle
import world_oracle as wo

SHAPES = [(1, 1, 1), (1, 80, 11), (2, 1, 3), (3, 17, 17), (5, 80, 11), (7, 15, 16), (8, 128, 14), (10, 176, 18),
          (16, 256, 32), (16, 255, 32)]
MARGIN = 1e-4           # smallest top-two margin of an act-mode case
KINK_BAND = 1e-5        # no world pre-activation closer to 0 than this
KINK_CAP = 2            # weight rows a world case may leave out of one layer's gradient comparison (none does)
POISON_U = 1 << 30
# (head, case id, tensor) -> float32-oracle error measured on the CPU, for tensors whose float32 oracle does not stay under a
# quarter of 1e-4 x max|ref|; the GPU test bounds those alone by 4 x the figure.  None needed.
F32_EXCEPTIONS = {}


def shape_id(N, O, A):
    return "N%d_O%d_A%d" % (N, O, A)


def _f32(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ RTW head
# (N, O, A, seed): the seed draws the weights (rtw_oracle.random_rtw_params) and, with the row count, every input
RTW_CASES = [(1, 1, 1, 1), (1, 80, 11, 1), (2, 1, 3, 1), (3, 17, 17, 1), (5, 80, 11, 1), (7, 15, 16, 2), (8, 128, 14, 1),
             (10, 176, 18, 1), (16, 256, 32, 2), (16, 255, 32, 11)]
RTW_SLOTS, RTW_T0 = 4, 2          # act mode reads slot 2 of 4: neither the first nor the last


def rtw_row_counts(N):
    ept = 16 // N
    return sorted({1, ept - 1, ept, ept + 1, 3 * ept + 1} - {0})


def rtw_given_bt(N):
    """(B, T) pairs of given mode: T no multiple of EPT where EPT > 1, B >= 3"""
    ept = 16 // N
    return [(3, ept + 1), (4, 2 * ept + 1)] if ept > 1 else [(3, 2), (4, 3)]


def rtw_params(N, O, A, seed):
    args = types.SimpleNamespace(n_agents=N, n_actions=A, obs_shape=O, rnn_hidden_dim=64, last_action=True, reuse_network=True)
    return rtw_oracle.random_rtw_params(args, seed)


def make_rtw_act(N, O, A, G, seed):
    """h (G*N, 64), obs / avail in RTW_SLOTS-slot storage with everything but slot RTW_T0 NaN, q0 of the size of real Q values.
    Agent j of environment g with (g + j) % 3 == 1 may only take action 0; agent 0 of environment 0 has no action at all."""
    rng = np.random.default_rng([seed, 1, G])
    h = _f32(rng, G * N, 64)
    obs = np.full((G, RTW_SLOTS, N, O), np.nan, np.float32)
    obs[:, RTW_T0] = _f32(rng, G, N, O)
    av = (rng.random((G, N, A)) < 0.6).astype(np.float32)
    av[..., 0] = 1.0
    g, j = np.meshgrid(np.arange(G), np.arange(N), indexing="ij")
    av[(g + j) % 3 == 1, 1:] = 0.0
    av[0, 0, :] = 0.0
    avail = np.full((G, RTW_SLOTS, N, A), np.nan, np.float32)
    avail[:, RTW_T0] = av
    q0 = _f32(rng, G * N, A, scale=2.0)
    return types.SimpleNamespace(N=N, O=O, A=A, G=G, h=h, obs=obs, avail=avail, q0=q0, o=obs[:, RTW_T0].reshape(G * N, O), av=av)


def make_rtw_given(N, O, A, B, T, seed):
    """hs (B, T, N, 64) as the unroll writes it; o at slot t and o_next at slot t + 1 of one (T+1)-slot storage (every slot is
    read); u in a (T+2)-slot plane read from slot 1, values in [-1, A) with at least one -1, the two unread slots at POISON_U"""
    rng = np.random.default_rng([seed, 2, B, T])
    hs = _f32(rng, B, T, N, 64)
    obs = _f32(rng, B, T + 1, N, O)
    u = rng.integers(-1, A, (B, T, N)).astype(np.int32)
    u[B - 1, T - 1, N - 1] = -1
    plane = np.full((B, T + 2, N), POISON_U, np.int32)
    plane[:, 1:T + 1] = u
    q0 = _f32(rng, B, T, N, A, scale=2.0)
    return types.SimpleNamespace(N=N, O=O, A=A, B=B, T=T, hs=hs, obs=obs, u=u, plane=plane, q0=q0)


def _t(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype)


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rtw_act_oracle(N, O, A, G, seed, not_self, dtype=torch.float64):
    """(case, namespace of numpy q_r, o_hat, a, margin) in `dtype`, computed once; margin (G*N, N) is the top-two margin of the
    masked logits of teammate j, infinite where agent j has at most one available action"""
    def run():
        c = _cached(("rtw_act", N, O, A, G, seed), lambda: make_rtw_act(N, O, A, G, seed))
        p = rtw_oracle.params_t(rtw_params(N, O, A, seed), dtype)
        with torch.no_grad():
            qr, ohat, a, gap = rtw_oracle.act_head(p, _t(c.h, dtype), _t(c.o, dtype), _t(c.av, dtype), N, not_self)
        few = np.broadcast_to((c.av.sum(-1) <= 1.0)[:, None, :], (G, N, N)).reshape(G * N, N)
        margin = np.where(few, np.inf, gap.double().numpy())
        return c, types.SimpleNamespace(qr=qr.numpy(), ohat=ohat.numpy(), a=a.numpy(), margin=margin)
    return _cached(("rtw_act_oracle", N, O, A, G, seed, not_self, dtype), run)


def rtw_given_oracle(N, O, A, B, T, seed, not_self, dtype=torch.float64):
    """(case, q_r (B, T, N, A) numpy) in `dtype`, computed once"""
    def run():
        c = _cached(("rtw_given", N, O, A, B, T, seed), lambda: make_rtw_given(N, O, A, B, T, seed))
        p = rtw_oracle.params_t(rtw_params(N, O, A, seed), dtype)
        with torch.no_grad():
            qr = rtw_oracle.given_head(p, _t(c.hs, dtype).reshape(-1, 64), _t(c.obs[:, :T], dtype).reshape(-1, O),
                                       _t(c.obs[:, 1:], dtype).reshape(-1, O), torch.tensor(c.u).reshape(-1), N, not_self)
        return c, qr.numpy().reshape(B, T, N, A)
    return _cached(("rtw_given_oracle", N, O, A, B, T, seed, not_self, dtype), run)


# ---------------------------------------------------------------------------------------------------------- world head
# (N, O, A, B, T, seed): R = B T N.  The seed draws the weights (oracle.seeded.seeded_state) and every input.
WORLD_CASES = [
    (1, 1, 1, 1, 1, 1), (1, 1, 1, 15, 1, 1), (1, 1, 1, 16, 1, 1), (1, 1, 1, 17, 1, 1), (1, 1, 1, 4096, 1, 12), (1, 1, 1, 4097, 1, 5),
    (1, 80, 11, 1, 1, 1), (1, 80, 11, 15, 1, 1), (1, 80, 11, 16, 1, 1), (1, 80, 11, 17, 1, 1), (1, 80, 11, 4096, 1, 12),
    (1, 80, 11, 4097, 1, 5),
    (2, 1, 3, 1, 1, 1), (2, 1, 3, 1, 7, 1), (2, 1, 3, 2, 4, 1), (2, 1, 3, 3, 3, 1), (2, 1, 3, 4, 512, 4), (2, 1, 3, 3, 683, 11),
    (3, 17, 17, 1, 1, 1), (3, 17, 17, 1, 5, 1), (3, 17, 17, 2, 3, 1), (3, 17, 17, 3, 455, 1), (3, 17, 17, 2, 683, 7),
    (5, 80, 11, 1, 1, 1), (5, 80, 11, 1, 3, 1), (5, 80, 11, 2, 2, 1), (5, 80, 11, 3, 273, 19), (5, 80, 11, 4, 205, 7),
    (7, 15, 16, 1, 1, 1), (7, 15, 16, 1, 2, 1), (7, 15, 16, 3, 1, 1), (7, 15, 16, 3, 195, 1), (7, 15, 16, 2, 293, 2),
    (8, 128, 14, 1, 1, 1), (8, 128, 14, 1, 2, 1), (8, 128, 14, 3, 1, 1), (8, 128, 14, 4, 128, 4), (8, 128, 14, 3, 171, 1),
    (10, 176, 18, 1, 1, 1), (10, 176, 18, 2, 1, 1), (10, 176, 18, 1, 409, 14), (10, 176, 18, 2, 205, 1),
    (16, 256, 32, 1, 1, 1), (16, 256, 32, 2, 1, 1), (16, 256, 32, 4, 64, 6), (16, 256, 32, 1, 257, 2),
    (16, 255, 32, 1, 1, 1), (16, 255, 32, 3, 1, 1), (16, 255, 32, 4, 64, 6), (16, 255, 32, 257, 1, 7),
]
# two small cases also run the backward with dq_idx = NULL and with den = NULL
WORLD_OPTIONAL_CASES = [c for c in WORLD_CASES if c[:5] in ((3, 17, 17, 2, 3), (5, 80, 11, 2, 2))]
WORLD_MODES = ("map", "len", "plain")      # (ep_map, ep_len) both given / ep_len alone / neither; all read from obs_t0 = 1
# weights at three times the default-init scale (as world_oracle.serial_agent_state): pre-activations of order 2 and 5, so that
# a 4096-row case (2 x 64 x 4096 of them) has seeds with none inside the kink band - at scale 1 about ten fall inside per seed
WORLD_WEIGHT_SCALE = 3.0
WORLD_DEN, WORLD_GRADS = 3.0, tuple(n + s for n in wo.WORLD[:4] for s in (".weight", ".bias"))


def world_id(case):
    N, O, A, B, T, seed = case
    return "%s_B%d_T%d" % (shape_id(N, O, A), B, T)


def make_world(N, O, A, B, T, seed):
    """weights p (numpy, world.* keys), h (B, T, N, 64), q0, the o_next every row would see (B, T, N, O), a permuted map into
    B + 2 stored episodes, ragged lengths (episode 0 full, episode 1 one short), the sparse TD gradient pair, base gradients"""
    rng = np.random.default_rng([seed, 3, B, T])
    args = types.SimpleNamespace(rnn_hidden_dim=64, n_actions=A, obs_shape=O)
    p = seeded.seeded_state(wo.world_param_shapes(args), seed=seed, scale=WORLD_WEIGHT_SCALE)
    R = B * T * N
    h = _f32(rng, B, T, N, 64)
    q0 = _f32(rng, B, T, N, A, scale=2.0)
    onext = _f32(rng, B, T, N, O)
    E = B + 2
    emap = rng.permutation(E)[:B].astype(np.int32)
    if np.array_equal(emap, np.arange(B)):
        emap = ((emap + 1) % E).astype(np.int32)
    ep_len = rng.integers(0, T + 1, B).astype(np.int32)
    ep_len[0] = T
    if B > 1:
        ep_len[1] = T - 1
    dq_idx = rng.integers(0, A, R).astype(np.int32)
    dq_val = _f32(rng, R)
    base = {k: _f32(rng, *v, scale=0.1) for k, v in wo.world_param_shapes(args) if k in WORLD_GRADS}
    return types.SimpleNamespace(N=N, O=O, A=A, B=B, T=T, R=R, E=E, p=p, h=h, q0=q0, onext=onext, emap=emap, ep_len=ep_len,
                                 dq_idx=dq_idx, dq_val=dq_val, den=WORLD_DEN, dscale=2.0 / (R * O), base=base)


def world_storage(c, mode):
    """(storage (episodes, T+1, N, O) read from slot 1 with everything unread NaN, the o_next the kernel must see (B, T, N, O))"""
    eps = c.E if mode == "map" else c.B
    st = np.full((eps, c.T + 1, c.N, c.O), np.nan, np.float32)
    seen = np.zeros_like(c.onext)
    for b in range(c.B):
        n = c.T if mode == "plain" else int(c.ep_len[b])
        st[c.emap[b] if mode == "map" else b, 1:1 + n] = c.onext[b, :n]
        seen[b, :n] = c.onext[b, :n]
    return st, seen


def world_case(case):
    return _cached(("world", case), lambda: make_world(*case))


def world_forward_oracle(case, dtype=torch.float64):
    """(r, o_hat, tau) numpy (B, T, N, .) in `dtype`, computed once"""
    def run():
        c = world_case(case)
        with torch.no_grad():
            return tuple(x.numpy() for x in wo.head(wo.params_t(c.p, dtype), _t(c.h, dtype)))
    return _cached(("world_fwd", case, dtype), run)


def world_backward_oracle(case, mode, dtype=torch.float64, dq=True, den=True):
    """namespace(loss, dhs, grads) of one addressing mode in `dtype`, computed once; dq False: no gradient on r, den False: 1"""
    def run():
        c = world_case(case)
        _, seen = world_storage(c, mode)
        ohat = torch.tensor(world_forward_oracle(case, dtype)[1])
        diff = ohat - _t(seen, dtype)
        dr = np.zeros((c.R, c.A), np.float64)
        if dq:
            dr[np.arange(c.R), c.dq_idx] = c.dq_val
        scale = torch.tensor(c.dscale, dtype=dtype) * torch.tensor(c.den if den else 1.0, dtype=dtype)
        dh, g = wo.head_backward(c.p, c.h, dr.reshape(c.B, c.T, c.N, c.A), (scale * diff).numpy(), dtype=dtype)
        return types.SimpleNamespace(loss=float((diff * diff).sum()), dhs=dh, grads=g)
    return _cached(("world_bwd", case, mode, dtype, dq, den), run)


def world_kinks(case):
    """{layer name: bool (64) rows of that layer's weight with a float64 pre-activation within KINK_BAND of 0}"""
    c = world_case(case)
    with torch.no_grad():
        zp, ep = wo.pre_activations(wo.params_t(c.p), _t(c.h, torch.float64).reshape(-1, 64))
    return {wo.WORLD[0]: (zp.abs() < KINK_BAND).any(0).numpy(), wo.WORLD[1]: (ep.abs() < KINK_BAND).any(0).numpy()}


def world_wgrad_plans(case):
    """the plans marl_linear_wgrad gives the four weight-gradient calls of the backward (host query, no GPU)"""
    from marl_amd import ops, _lib
    N, O, A, B, T, seed = case
    R = B * T * N
    x = ops.MarlSrc()
    x.p0, x.ld0, x.k0 = 1 << 20, 64, 64
    lib = _lib.load()
    ws = max(lib.marl_linear_wgrad_workspace(R, n, 64, 1) for n in (64, A, O))
    r4 = lambda n: (n + 3) // 4 * 4
    calls = ((64, 64, 1 << 21), (64, 64, 1 << 21), (A, r4(A), None), (O, r4(O), None))
    return [ops.linear_wgrad_plan(1 << 22, ld, x, R, n, 64, Yact=act, ldya=64 if act else 0, ws_bytes=ws) for n, ld, act in calls]
