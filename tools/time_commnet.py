#!/usr/bin/env python3
"""Cost of the CommNet actor on one MI355X, in alternating rounds of one process:
  1. marl_commnet_head_fwd and marl_commnet_head_bwd alone, by HIP events;
  2. the recurrence through the identity front layer (CommNetMAC's saving unroll + BPTT on a dense dhs, O = 64, a dummy fc2) beside
     the plain PolicyMAC unroll + BPTT of the same shape, by HIP events;
  3. the reinforce+commnet update beside the reinforce update built from the same tree (host clock around a device synchronise;
     fixed-length episodes, f32 mode, eager launches - the set-up of tools/time_pg.py).
Defaults: 2s3z and MMM2, T = 120, 4096 episodes, seven rounds."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def events(calls, rounds, reps):
    """median / min / max microseconds per call of every entry of ``calls``, alternating"""
    for f in calls.values():
        for _ in range(3):
            f()
    us = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in calls.items():
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: (statistics.median(x), min(x), max(x)) for k, x in us.items()}


def make(actor, shape, o):
    """(args, controller, learner, rollout worker) of reinforce on ``shape``; ``actor``: 'commnet' (k = o.k), 'g2anet' or None for the
    plain PolicyMAC - fixed-length episodes, f32 mode, eager launches"""
    from marl_amd.controller import share_params as sp
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.common.arguments import get_reinforce_args, get_g2anet_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    args = bench.make_args("reinforce", shape, o.T)
    args.gemm_mode, args.hip_graph = "f32", False
    get_reinforce_args(args)
    if actor == "commnet":
        args.alg, args.k = "reinforce+commnet", o.k
    elif actor == "g2anet":
        get_g2anet_args(args)
        args.alg = "reinforce+g2anet"
    torch.manual_seed(0)
    mac = {"commnet": sp.CommNetMAC, "g2anet": sp.G2ANetMAC, None: sp.PolicyMAC}[actor](args)
    learner = ReinforceLearner(mac, args)
    env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                           seed=1, fixed_length=True)
    w = RolloutWorker(env, mac, args)
    w.rollout_mode = "unfused"
    return args, mac, learner, w


def time_updates(shape, alg, o, learner, worker, plain_learner, plain_worker):
    """the update of ``alg`` beside the reinforce update built from the same tree, alternating: host clock around a device synchronise"""
    ep_a, ep_p = worker.generate_episodes(o.envs)[0], plain_worker.generate_episodes(o.envs)[0]
    steps = {alg: lambda i: learner.train(ep_a, i, epsilon=worker.epsilon),
             "reinforce": lambda i: plain_learner.train(ep_p, i, epsilon=plain_worker.epsilon)}
    for f in steps.values():
        for i in range(3):
            f(i)
    gc.collect()
    gc.disable()
    ms = {k: [] for k in steps}
    for _ in range(o.rounds):
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(o.updates):
                f(i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / o.updates)
    gc.enable()
    for k, x in ms.items():
        print("%-5s %-18s update  envs %d  median %.2f ms (min %.2f - max %.2f, %d rounds of %d)"
              % (shape, k, o.envs, statistics.median(x), min(x), max(x), o.rounds, o.updates))
    print("%-5s %s / reinforce  %.3f" % (shape, alg, statistics.median(ms[alg]) / statistics.median(ms["reinforce"])))


def one_shape(shape, o):
    from marl_amd import ops
    dev = torch.device("cuda")
    (ca, cmac, cl, cw), (pa, pmac, pl, pw) = make("commnet", shape, o), make(None, shape, o)
    B, T, N, A, O, H = o.envs, ca.episode_limit, ca.n_agents, ca.n_actions, ca.obs_shape, 64
    G, R = B * T, B * T * N
    # 1. the head alone
    hs, dl = torch.tanh(torch.randn(R, H, device=dev)), torch.randn(R, A, device=dev)
    logits, dhs = torch.empty(R, A, device=dev), torch.empty(R, H, device=dev)
    ag = cmac.agent
    head = events({"head fwd": lambda: ops.commnet_head_fwd(ag.head_weights(), hs, logits, G, N, A, o.k),
                   "head bwd": lambda: ops.commnet_head_bwd(ag.head_weights(), ag.head_grads(), hs, dl, dhs, G, N, A, o.k)},
                  o.rounds, o.reps)
    for k, (med, lo, hi) in head.items():
        print("%-5s %-9s G %d x N %d, A %d, K %d  median %.1f us (min %.1f - max %.1f, %d rounds of %d)"
              % (shape, k, G, N, A, o.k, med, lo, hi, o.rounds, o.reps))
    # 2. the recurrence: identity front beside the plain unroll + BPTT
    from marl_amd.network.commnet import FRONT_A
    e = torch.rand(B, T, N, H, device=dev)
    obs = torch.randn(B, T, N, O, device=dev)
    u = torch.zeros(B, T, N, dtype=torch.int32, device=dev)
    saved, h_last = torch.empty(ops.saved_shape(T, B, N), device=dev), torch.empty(B * N, H, device=dev)
    hsp, dxp = torch.empty(B, T, N, H, device=dev), torch.empty(B, T, N, H, device=dev)
    q0, qp = torch.empty(B, T, N, FRONT_A, device=dev), torch.empty(B, T, N, A, device=dev)
    zi, zv = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, device=dev)
    dhs4 = torch.randn(B, T, N, H, device=dev)
    dq = torch.randn(B, T, N, A, device=dev)
    fg = {"rnn.weight_ih": ag.f_obs.weight_ih.grad, "rnn.weight_hh": ag.f_obs.weight_hh.grad, "rnn.bias_ih": ag.f_obs.bias_ih.grad,
          "rnn.bias_hh": ag.f_obs.bias_hh.grad, "fc2.weight": torch.zeros(FRONT_A, H, device=dev), "fc2.bias": torch.zeros(FRONT_A, device=dev)}
    pg_ = pmac.agent
    gp = {"rnn.weight_ih": pg_.rnn.weight_ih.grad, "rnn.weight_hh": pg_.rnn.weight_hh.grad, "rnn.bias_ih": pg_.rnn.bias_ih.grad,
          "rnn.bias_hh": pg_.rnn.bias_hh.grad, "fc2.weight": pg_.fc2.weight.grad, "fc2.bias": pg_.fc2.bias.grad}

    def front():
        ops.agent_unroll_fwd(ag.front_weights(), e, T * N, 0, None, 0, 0, None, q0, hsp, h_last, saved, B, T, N, H, FRONT_A, False, False)
        ops.agent_unroll_bwd(ag.front_weights(), None, dhs4, saved, None, dxp, None, fg, B, T, N, FRONT_A, dq_idx=zi, dq_val=zv)

    def plain():
        ops.agent_unroll_fwd(pg_.weights(), obs, T * N, 0, u, T * N, -1, None, qp, None, h_last, saved, B, T, N, O, A,
                             pa.last_action, pa.reuse_network)
        ops.agent_unroll_bwd(pg_.weights(), dq, None, saved, None, dxp, None, gp, B, T, N, A)

    rec = events({"identity front": front, "plain unroll": plain}, o.rounds, max(1, o.reps // 5))
    for k, (med, lo, hi) in rec.items():
        print("%-5s %-15s unroll + BPTT  B %d T %d N %d  median %.2f ms (min %.2f - max %.2f)" % (shape, k, B, T, N, med / 1e3, lo / 1e3, hi / 1e3))
    print("%-5s identity front / plain  %.3f" % (shape, rec["identity front"][0] / rec["plain unroll"][0]))
    del e, obs, saved, hsp, dxp, dhs4, dq, hs, dl, logits, dhs
    # 3. the updates
    time_updates(shape, "reinforce+commnet", o, cl, cw, pl, pw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shapes", nargs="+", default=["2s3z", "MMM2"])
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--updates", type=int, default=5)
    o = ap.parse_args()
    for shape in o.shapes:
        one_shape(shape, o)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
