"""The float64 statement of backward-through-time of the agent unroll, for the kernel tests of the two BPTT implementations
(csrc/agent.hip: agent_bwd_kernel / agent_bwd_pipe_kernel; csrc/agent_bwd_x6.hip) - tests/test_gpu_bptt.py - and its own CPU
tests (tests/test_bptt_oracle_cpu.py).  TEST INFRASTRUCTURE: the product never imports it.

* `make_case`: seeded parameters, observations and fed actions exactly as tests/test_gpu_kernels.py:_agent_case draws them (weights
  at scale 2.0) plus a non-zero h0; every value is an fp32 number, so the device gets bit for bit what float64 sees.
* `make_dq`: the gradient the backward pass starts from - one sparse (action, value) pair per row, two pairs with one value per
  (episode, step) shared by its agents (dq_gdiv = N, the QTRAN form) plus an external gradient on hs, a dense dq plus that
  gradient, or the seam probe: one pair per row whose values are exactly 0 except on the rows `probe_rows` names.
* `unroll` / `backward`: the unroll with the arithmetic of oracle/nets.agent_step in any dtype; the fc1 pre-activation of every
  row-step keeps its gradient (dxp: the relu gate is part of it) and h0 is a gradient leaf (dh0).
* `kink_mask`: the elements of dxp an fp32 forward may gate the other way.
* `bx6_plan` / `f32_plan` / `seams` / `probe_rows`: a mirror of the two launch plans, used to pick and to label the cases.
* `CASES`: the row counts at which the launch code takes another path, with the plan each one was picked for."""
from __future__ import annotations

import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import seeded, nets

H = 64
PARAMS = ("fc1.weight", "fc1.bias", "rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh", "fc2.weight", "fc2.bias")
BWD_PARAMS = PARAMS[2:]                 # what the BPTT kernels accumulate themselves; fc1's come from dxp through linear_wgrad
FORMS = ("s1", "s2h", "dense", "probe")


# --------------------------------------------------------------------------------------------------------- launch plans
def tiles_of(R):
    return (R + 15) // 16


def bx6_plan(R):
    """(n2, n1) of csrc/agent_bwd_x6.hip: n2 two-tile workgroups, then a second launch of n1 one-tile workgroups."""
    tiles = tiles_of(R)
    if tiles <= 256:
        return 0, tiles
    n2 = tiles // 512 * 256
    rem = tiles - 2 * n2
    if n2 > 0 and 0 < rem <= 256:
        return n2, rem
    return (tiles + 1) // 2, 0


def f32_plan(R, A):
    """(RT, nwg) of csrc/agent.hip: RT row tiles per workgroup = ceil(tiles / 256) up to what LDS (160 KB) and the dq prefetch
    registers allow - 6 with one action tile (A <= 16), 4 with two."""
    AC = 1 if A <= 16 else 2
    HS, DGS, NQ, BNT = H + 8, 256 + 8, 4, 512
    QS = AC * 16 + 4
    per_row = (DGS + 2 * QS + HS) * 4 + 12
    cap = min(8, (NQ * BNT) // (16 * AC * 16))
    rt_max = max(1, min(cap, (160 * 1024 - 4 * 64 * 4) // (per_row * 16)))
    rt = max(1, min(rt_max, (tiles_of(R) + 255) // 256))
    return rt, (R + rt * 16 - 1) // (rt * 16)


def seams(R, A):
    """first rows of: the second row tile; the second and the last workgroup of either kernel; the split kernel's second launch"""
    out = []
    if R > 16:
        out.append(16)
    n2, n1 = bx6_plan(R)
    starts = [32 * k for k in range(n2)] + [32 * n2 + 16 * k for k in range(n1)]
    if len(starts) > 1:
        out += [starts[1], starts[-1]]
    if n2 and n1:
        out.append(32 * n2)
    rt, nwg = f32_plan(R, A)
    if nwg > 1:
        out += [rt * 16, (nwg - 1) * rt * 16]
    return sorted(set(out))


def probe_rows(R, seam_rows):
    """row 0, row R - 1 and the two rows either side of every seam"""
    rows = {0, R - 1}
    for s in seam_rows:
        rows |= {s - 1, s}
    rows = sorted(rows)
    assert rows[0] >= 0 and rows[-1] < R, (rows, R)
    return rows


# --------------------------------------------------------------------------------------------------------- cases
def _c(shape, B, T, x6, f32, la=1, rn=1, forms=FORMS, seed=3):
    N, A = seeded.SHAPES[shape]["n_agents"], seeded.SHAPES[shape]["n_actions"]
    return types.SimpleNamespace(shape=shape, B=B, T=T, N=N, A=A, R=B * N, la=la, rn=rn, x6=x6, f32=f32, forms=forms, seed=seed,
                                 key=(shape, B, T, la, rn, seed))


# x6 = (n2, n1) and f32 = (RT, nwg): the plan the row count was picked for (None: the split kernel does not cover T < 3)
CASES = [
    _c("2s3z", 818, 3, (0, 256), (1, 256)),       # 256 tiles, 10-row tail: one-tile upper edge
    _c("2s3z", 822, 3, (129, 0), (2, 129)),       # 257 tiles: the last workgroup of either kernel has no second tile
    _c("2s3z", 1641, 3, (256, 1), (3, 171)),      # 513 tiles: mixed plan, a second launch of one 13-row workgroup
    _c("2s3z", 1641, 3, (256, 1), (3, 171), la=0, rn=1, forms=("s1", "probe")),
    _c("2s3z", 1641, 3, (256, 1), (3, 171), la=1, rn=0, forms=("s1", "probe")),
    _c("2s3z", 1641, 3, (256, 1), (3, 171), la=0, rn=0, forms=("s1", "probe")),
    _c("2s3z", 2457, 3, (256, 256), (3, 256)),    # 768 tiles: mixed-plan upper edge
    _c("2s3z", 2460, 3, (385, 0), (4, 193)),      # 769 tiles: second round of two-tile workgroups; RT 4, last workgroup 12 rows
    _c("2s3z", 3277, 3, (512, 1), (5, 205)),      # 1025 tiles: the second launch holds ONE row
    _c("MMM2", 821, 3, (256, 2), (3, 172)),       # two action tiles, mixed plan
    _c("2s3z", 13, 40, (0, 5), (1, 5)),           # long horizon
    _c("2s3z", 1663, 3, (256, 8), (3, 174)),      # 520 tiles, 11-row tail: RT 3
    _c("2s3z", 1663, 2, None, (3, 174), forms=("s1", "probe")),   # the pipelined kernel's minimum T
    _c("2s3z", 4100, 3, (641, 0), (6, 214)),      # 1282 tiles: RT 6, the most LDS allows
    _c("MMM2", 832, 3, (256, 8), (3, 174)),       # two action tiles, RT 3
]


def case_id(c):
    s = "%s-R%d-T%d-tiles%d" % (c.shape, c.R, c.T, tiles_of(c.R))
    if not (c.la and c.rn):
        s += "-" + "-".join(n for n, f in (("nolast", c.la), ("noid", c.rn)) if not f)
    return s


def plan_id(c, kernel):
    return "x6[%d+%d]" % c.x6 if kernel == "x6" else "f32[RT%dx%d]" % c.f32


# --------------------------------------------------------------------------------------------------------- inputs
def make_case(c):
    """parameters / obs / ufed / h0 as numpy fp32 (ufed int64, -1 = no action fed), drawn as _agent_case(with_h0=True) draws them"""
    args = seeded.make_args(c.shape, "qmix", episode_limit=c.T, last_action=bool(c.la), reuse_network=bool(c.rn))
    p_np = seeded.seeded_state(seeded.agent_param_shapes(args), seed=11 + c.seed, scale=2.0)
    rng = np.random.default_rng(c.seed)
    N, O, A = args.n_agents, args.obs_shape, args.n_actions
    obs = rng.standard_normal((c.B, c.T, N, O)).astype(np.float32)
    ufed = rng.integers(-1, A, size=(c.B, c.T, N))
    h0 = rng.standard_normal((c.B * N, H)).astype(np.float32) * np.float32(0.5)
    return types.SimpleNamespace(args=args, p=p_np, obs=obs, ufed=ufed, h0=h0)


def make_dq(c, form):
    """fp32 tensors: idx / val (/ idx2 / val2, gdiv) of the sparse forms or `dense`, the external gradient dhs or None, and `full`:
    the dense (B, T, N, A) tensor the form stands for"""
    B, T, N, A = c.B, c.T, c.N, c.A
    g = torch.Generator().manual_seed(5)
    d = types.SimpleNamespace(form=form, idx=None, val=None, idx2=None, val2=None, gdiv=1, dense=None, dhs=None, rows=None)
    if form == "dense":
        d.dense = torch.randn(B, T, N, A, generator=g)
        d.dhs = torch.randn(B, T, N, H, generator=g) * 0.3
        d.full = d.dense
        return d
    d.idx = torch.randint(0, A, (B, T, N), generator=g)
    if form == "s2h":
        d.gdiv = N
        d.val = torch.randn(B, T, generator=g)
        d.idx2 = torch.randint(0, A, (B, T, N), generator=g)
        d.idx2[0, 0] = d.idx[0, 0]                                # coinciding columns add
        d.val2 = torch.randn(B, T, generator=g)
        d.dhs = torch.randn(B, T, N, H, generator=g) * 0.3
        d.full = torch.zeros(B, T, N, A).scatter_add_(3, d.idx[..., None], d.val[..., None, None].expand(B, T, N, 1).contiguous())
        d.full.scatter_add_(3, d.idx2[..., None], d.val2[..., None, None].expand(B, T, N, 1).contiguous())
        return d
    d.val = torch.randn(B, T, N, generator=g)
    if form == "probe":
        d.rows = probe_rows(c.R, seams(c.R, A))
        keep = torch.zeros(c.R, dtype=torch.bool)
        keep[d.rows] = True
        v = d.val + 0.5 * torch.sign(d.val)                       # |value| >= 0.5 on every step of a probe row
        d.val = torch.where(keep.view(B, 1, N), v, torch.zeros(()))
    else:
        assert form == "s1", form
    d.full = torch.zeros(B, T, N, A).scatter_(3, d.idx[..., None], d.val[..., None])
    return d


# --------------------------------------------------------------------------------------------------------- the operation
def gates(p, pre, h):
    """x, gi, gh, r, z, n of oracle/nets.agent_step from the fc1 pre-activation on (tests/unroll_oracle.py reads the vectors the
    forward kernels save from here)"""
    x = torch.relu(pre)
    gi = F.linear(x, p["rnn.weight_ih"], p["rnn.bias_ih"])
    gh = F.linear(h, p["rnn.weight_hh"], p["rnn.bias_hh"])
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return x, gi, gh, r, z, n


def _step(p, pre, h):
    """oracle/nets.agent_step from the fc1 pre-activation on"""
    x, gi, gh, r, z, n = gates(p, pre, h)
    h2 = (1.0 - z) * n + z * h
    return nets.lin(p, "fc2", h2), h2


def onehot(ufed, A, dtype):
    B, T, N = ufed.shape
    oh = np.zeros((B, T, N, A), np.float32)
    bb, tt, nn = np.nonzero(ufed >= 0)
    oh[bb, tt, nn, ufed[bb, tt, nn]] = 1
    return torch.tensor(oh, dtype=dtype)


def unroll(k, dtype=torch.float64, pre_delta=None):
    """k = make_case(c).  q (B,T,N,A), hs (B,T,N,H), h_last, with the graph; pre: list of T (R,H) pre-activations that retain
    their gradient; p / h0: the leaves.  pre_delta (T,R,H) is added to the pre-activations (finite differences)."""
    a = k.args
    p = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in k.p.items()}
    obs = torch.tensor(k.obs, dtype=dtype)
    oh = onehot(k.ufed, a.n_actions, dtype)
    h0 = torch.tensor(k.h0, dtype=dtype, requires_grad=True)
    B, T, N, _ = obs.shape
    h, qs, hs, pres = h0, [], [], []
    for t in range(T):
        inp = nets.build_inputs(obs[:, t], oh[:, t], N, a.last_action, a.reuse_network)
        pre = nets.lin(p, "fc1", inp)
        if pre_delta is not None:
            pre = pre + pre_delta[t]
        pre.retain_grad()
        q, h = _step(p, pre, h)
        pres.append(pre)
        qs.append(q.view(B, N, -1))
        hs.append(h.view(B, N, -1))
    return types.SimpleNamespace(p=p, h0=h0, pre=pres, q=torch.stack(qs, 1), hs=torch.stack(hs, 1), h_last=h, B=B, T=T, N=N)


def backward(u, dq, dhs=None):
    """gradients of sum(q dq) + sum(hs dhs): {the eight parameters, "dxp" (B,T,N,H), "dh0" (R,H)}.  May be called again on
    the same unroll."""
    for t in list(u.p.values()) + [u.h0] + u.pre:
        t.grad = None
    loss = (u.q * dq.to(u.q.dtype)).sum()
    if dhs is not None:
        loss = loss + (u.hs * dhs.to(u.q.dtype)).sum()
    loss.backward(retain_graph=True)
    out = {n: v.grad.clone() for n, v in u.p.items()}
    out["dxp"] = torch.stack([x.grad for x in u.pre], 0).view(u.T, u.B, u.N, H).permute(1, 0, 2, 3).contiguous()
    out["dh0"] = u.h0.grad.clone()
    return out


def pre_of(u):
    """(B,T,N,H) pre-activations of an unroll"""
    return torch.stack([x.detach() for x in u.pre], 0).view(u.T, u.B, u.N, H).permute(1, 0, 2, 3).contiguous()


def kink_mask(pre):
    """True where the float64 pre-activation is within 1e-5 max(1, max|pre|) of 0: an fp32 forward may gate these the other way"""
    return pre.abs() <= 1e-5 * max(1.0, float(pre.abs().max()))


def scaled_err(got, want, keep=None):
    """max|got - want| / max(1, max|want|), over `keep` when given"""
    d = (got.double() - want.double()).abs()
    if keep is not None:
        d = d[keep]
    return float(d.max()) / max(1.0, float(want.abs().max()))


class Oracle:
    """Per case: the float64 unroll, and per dq form its gradients `want` next to `ref_err`: the scaled error of fp32 torch-CPU
    autograd on the same inputs - the yardstick a kernel's error is printed beside.  Keeps the graphs of ONE case (the tests ask
    case by case)."""

    def __init__(self):
        self.key = None

    def get(self, c, form):
        if self.key != c.key:
            self.key, self.res = c.key, {}
            self.k = make_case(c)
            self.u64, self.u32 = unroll(self.k), unroll(self.k, torch.float32)
            self.pre = pre_of(self.u64)
            self.keep = ~kink_mask(self.pre)
        if form not in self.res:
            d = make_dq(c, form)
            want = backward(self.u64, d.full, d.dhs)
            want["q"] = self.u64.q.detach()
            f32 = backward(self.u32, d.full, d.dhs)
            f32["q"] = self.u32.q.detach()
            ref_err = {n: scaled_err(f32[n], want[n], self.keep if n == "dxp" else None) for n in want}
            self.res[form] = types.SimpleNamespace(k=self.k, d=d, want=want, ref_err=ref_err, keep=self.keep)
        return self.res[form]
