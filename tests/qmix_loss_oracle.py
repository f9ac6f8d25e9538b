"""float64 CPU statement of what the loss-folded QMIX backward kernels compute (TEST INFRASTRUCTURE; reference
network/mixer.py:57-80, algorithm/q_learner.py:112-127; include/marl_hip.h: marl_qmix_fused_loss_bwd / marl_qmix_wide_loss_bwd).

    q_tot  = QMixMixer.forward(q, s)                                         (E = 32, single-layer hypernets)
    mask   = 1 - padded;  target = r + gamma q_tot_tgt (1 - term);  td = mask (target - q_tot)
    loss2  = [sum td^2, sum mask]                                            (un-normalised)
    dq, d(the ten mixer tensors) = gradient of sum td^2

Everything is torch.float64 on the CPU and the gradients are torch autograd's: no derivative is written out by hand, so the
oracle shares no formula with the kernels beyond the forward pass that oracle/nets.py and the header already state."""
from __future__ import annotations

import types

import torch
import torch.nn.functional as F

E = 32
SEGMENTS = ("w1", "b1", "w2", "h")                        # the four state-conditioned layers: hyper_w1, hyper_b1, hyper_w2, hyper_b2.0
NAMES = ("w1", "w1_b", "b1", "b1_b", "w2", "w2_b", "h", "h_b", "b2_w", "b2_b")
KINKED = ("w1", "w2", "h")                                # |w1|, |w2|, relu(h): not differentiable where the layer's output is 0


def _bf16(t):
    """t rounded to bf16 (round to nearest even, as the matrix-core path rounds its operands), kept in float64"""
    return t.float().bfloat16().double()


def loss_backward(P, s, q, q_tot_tgt, r, term, padded, gamma, bf16=False, wgrad_fp32=False):
    """P: the ten QMixMixer tensors by the names of ops.qmix_weights; s (R, S), q (R, N), q_tot_tgt / r / term / padded (R).
    bf16: both operands of the four state-conditioned products are rounded to bf16 (the sums stay exact: products of bf16
    values need 16 bits); the weight gradient is then d(out)^T round(s) - the rounding is passed straight through.
    wgrad_fp32 (with bf16; flags = 1 of the wide entry points): same values, weight gradient d(out)^T s on the UNROUNDED states.
    Returns a namespace: q_tot (R), loss2 (2), dq (R, N), grads {name: tensor}, hyper {"w1" | "w2" | "h": (R, columns)} - the
    hypernet outputs BEFORE |.| / relu, where a caller looks for kinks -, td (R) and mask (R); all float64."""
    f64 = lambda t: torch.as_tensor(t).detach().to(torch.float64)
    W = {k: f64(P[k]).clone().requires_grad_() for k in NAMES}
    s, q_tot_tgt, r, term, padded = (f64(t) for t in (s, q_tot_tgt, r, term, padded))
    q = f64(q).clone().requires_grad_()
    R, N = q.shape
    assert s.shape[0] == R and W["w1"].shape == (N * E, s.shape[1]) and not (wgrad_fp32 and not bf16)

    def lin(k):
        if not bf16:
            return F.linear(s, W[k], W[k + "_b"])
        if wgrad_fp32:
            plain = F.linear(s, W[k])                                          # contributes exactly 0 and the gradient d(out)^T s
            return F.linear(_bf16(s), _bf16(W[k].detach()), W[k + "_b"]) + (plain - plain.detach())
        # W + (round(W) - W) is round(W) exactly in float64 (both fit 24 bits at neighbouring exponents); gradient: identity
        return F.linear(_bf16(s), W[k] + (_bf16(W[k].detach()) - W[k].detach()), W[k + "_b"])

    hy = {k: lin(k) for k in SEGMENTS}
    w1 = hy["w1"].abs().view(R, N, E)                                          # agent-major: column n * E + e
    hid = F.elu((q.unsqueeze(2) * w1).sum(1) + hy["b1"])
    b2 = F.linear(torch.relu(hy["h"]), W["b2_w"], W["b2_b"]).squeeze(1)
    q_tot = (hid * hy["w2"].abs()).sum(1) + b2
    mask = 1.0 - padded
    target = r + float(gamma) * q_tot_tgt * (1.0 - term)
    td = mask * (target - q_tot)
    num = (td ** 2).sum()
    names = list(NAMES)
    gs = torch.autograd.grad(num, [q] + [W[k] for k in names])
    return types.SimpleNamespace(q_tot=q_tot.detach(), loss2=torch.stack([num.detach(), mask.sum()]), dq=gs[0],
                                 grads=dict(zip(names, gs[1:])), hyper={k: hy[k].detach() for k in KINKED},
                                 td=td.detach(), mask=mask)


def kink_columns(hyper, eps=2e-6):
    """{segment: bool (columns)}: output columns of w1 / w2 / h with a row within eps of the kink at 0, where a kernel may take the
    other one-sided derivative - which changes that one row (and bias entry) of the segment's weight gradient"""
    return {k: (v.abs() < eps).any(0) for k, v in hyper.items()}


def loss0_bound(o, tol_q):
    """bound on |sum td^2 - loss2[0]| implied by |q_tot - want| <= tol_q on every row: 2 tol_q sum(mask |td|) + tol_q^2 sum(mask)"""
    return float(2.0 * tol_q * (o.mask * o.td.abs()).sum() + tol_q ** 2 * o.mask.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# seeded cases, shared by the CPU test (which counts their kinks) and the GPU kernel tests (tests/test_gpu_qmix_loss.py).
# Row counts come from the launch code: fused = one 16-row tile per workgroup up to 256 workgroups, wide = 128 rows per block
# up to 256 blocks.  (R, N, S, seed): the seed is chosen so that the float64 hypernet outputs alone stay within the kink cap.
FUSED_CASES = [(1, 1, 4, 6), (15, 2, 8, 25), (16, 5, 120, 141), (17, 3, 48, 68), (333, 5, 120, 458),
               (4099, 3, 48, 4150),              # 257 tiles: one workgroup runs two
               (8200, 5, 124, 8329),             # three tiles in workgroup 0, tail of 8 rows
               (30720, 5, 120, 2)]               # 7.5 passes of the grid
# (R, N, S, seed of flags 0, seed of the bf16 modes or None: flags 0 only)
WIDE_CASES = [(1, 10, 322, 333, None), (127, 10, 322, 459, None), (128, 10, 322, 460, None), (129, 10, 322, 461, 461),
              (333, 10, 322, 665, 665), (5000, 10, 322, 5332, 5332), (130, 4, 352, 486, 486), (100, 3, 52, 155, None),
              (32775, 10, 322, 2, 1)]            # second pass of the grid with a 7-row tail
REMAP_T, REMAP_EPISODES = 120, 36                # the learner's view: (T+1)-slot storage read through an episode map
REMAP_CASES = {"fused": (REMAP_T * REMAP_EPISODES, 5, 120, 4445), "wide": (REMAP_T * REMAP_EPISODES, 10, 322, 4652)}
KINK_CAP, KINK_CAP_32775_BF16 = 2, 4


def make_case(R, N, S, seed, episode=None):
    """Seeded inputs of one kernel call as float32 CPU tensors.  Generator order: weight and bias of w1, b1, w2, h, then b2_w,
    b2_b, then s (the kink count depends on the draws up to here only), q, q_tot_tgt, r, episode lengths, base gradients.
    Rows form pseudo-episodes of `episode` steps (default: 25, fewer where the case has under 75 rows) with a block of trailing
    padded rows each, as a learner batch has; padded rows are terminated too (rollout.py:122-133), and two episodes in three
    terminate on their last real step."""
    if episode is None:
        episode = max(2, min(25, R // 3))
    g = torch.Generator().manual_seed(seed)
    outs = {"w1": N * E, "b1": E, "w2": E, "h": E}
    P = {}
    for k in SEGMENTS:
        P[k] = torch.randn(outs[k], S, generator=g) * 0.2
        P[k + "_b"] = torch.randn(outs[k], generator=g) * 0.2
    P["b2_w"] = torch.randn(1, E, generator=g)
    P["b2_b"] = torch.randn(1, generator=g)
    s = torch.randn(R, S, generator=g)
    q = torch.randn(R, N, generator=g)
    q_tot_tgt = torch.randn(R, generator=g) * 2.0
    r = torch.randn(R, generator=g)
    n_ep = (R + episode - 1) // episode
    length = torch.randint(1, episode + 1, (n_ep,), generator=g)               # >= 1: the first row of an episode is real
    ends = torch.rand(n_ep, generator=g) < 2.0 / 3.0
    t = torch.arange(n_ep * episode) % episode
    L = length.repeat_interleave(episode)
    padded = (t >= L).float()[:R]
    term = ((t >= L) | ((t == L - 1) & ends.repeat_interleave(episode))).float()[:R]
    base = {k: torch.randn(v.shape, generator=g) for k, v in P.items()}        # the kernels accumulate into the gradients
    return types.SimpleNamespace(R=R, N=N, S=S, P=P, s=s, q=q, q_tot_tgt=q_tot_tgt, r=r, term=term, padded=padded, base=base)


def count_kinks(c, bf16=False, eps=2e-6):
    """number of hypernet output columns of a case with a float64 value within eps of 0 (forward only: no autograd graph)"""
    rnd = _bf16 if bf16 else (lambda t: t)
    n = 0
    for k in KINKED:
        out = F.linear(rnd(c.s.double()), rnd(c.P[k].double()), c.P[k + "_b"].double())
        n += int((out.abs() < eps).any(0).sum())
    return n
