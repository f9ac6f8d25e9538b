#!/usr/bin/env python3
"""Cost of the G2ANet actor on one MI355X, in alternating rounds of one process:
  1. marl_g2anet_head_fwd and marl_g2anet_head_bwd alone (hard on and off) and marl_g2anet_noise, by HIP events, beside the forward's
     floor: 2 x (55.3 K + 24.6 K (N - 1)) FLOP per row at the fp32 MFMA peak (--peak_tflops, the microarchitecture guide's figure);
  2. the reinforce+g2anet update beside the reinforce update built from the same tree (host clock around a device synchronise;
     fixed-length episodes, f32 mode, eager launches - the set-up of tools/time_pg.py and tools/time_commnet.py).
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
from time_commnet import events  # noqa: E402


def one_shape(shape, o):
    from marl_amd import ops
    from marl_amd.controller.share_params import PolicyMAC, G2ANetMAC
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.common.arguments import get_reinforce_args, get_g2anet_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    dev = torch.device("cuda")

    def make(g2anet):
        args = bench.make_args("reinforce", shape, o.T)
        args.gemm_mode, args.hip_graph = "f32", False
        get_reinforce_args(args)
        if g2anet:
            get_g2anet_args(args)
            args.alg = "reinforce+g2anet"
        torch.manual_seed(0)
        mac = (G2ANetMAC if g2anet else PolicyMAC)(args)
        learner = ReinforceLearner(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return args, mac, learner, w

    (ga, gmac, gl, gw), (pa, pmac, pl, pw) = make(True), make(False)
    B, T, N, A, H = o.envs, ga.episode_limit, ga.n_agents, ga.n_actions, 64
    G, R = B * T, B * T * N
    # 1. the head alone
    hs, dl = torch.tanh(torch.randn(R, H, device=dev)), torch.randn(R, A, device=dev)
    logits, dhs = torch.empty(R, A, device=dev), torch.empty(R, H, device=dev)
    noise = torch.empty(B, T, N, N - 1, device=dev)
    ag = gmac.agent
    calls = {"noise": lambda: ops.g2anet_noise(1, 0, 0, noise, B, T, N)}
    for hard in (True, False):
        tag = "hard" if hard else "soft only"
        calls["head fwd " + tag] = lambda hard=hard: ops.g2anet_head_fwd(ag.head_weights(), hs, noise, logits, G, N, A, hard, gmac.tau)
        calls["head bwd " + tag] = lambda hard=hard: ops.g2anet_head_bwd(ag.head_weights(), ag.head_grads(), hs, noise, dl, dhs, G, N, A,
                                                                         hard, gmac.tau)
    head = events(calls, o.rounds, o.reps)
    floor_ms = 2.0 * (55.3e3 + 24.6e3 * (N - 1)) * R / (o.peak_tflops * 1e12) * 1e3
    for k, (med, lo, hi) in head.items():
        print("%-5s %-19s G %d x N %d, A %d  median %.2f ms (min %.2f - max %.2f, %d rounds of %d)"
              % (shape, k, G, N, A, med / 1e3, lo / 1e3, hi / 1e3, o.rounds, o.reps))
    print("%-5s head fwd floor at %.0f TFLOP/s fp32 MFMA: %.2f ms  (fwd hard / floor %.1f)"
          % (shape, o.peak_tflops, floor_ms, head["head fwd hard"][0] / 1e3 / floor_ms))
    del hs, dl, logits, dhs, noise
    if o.head_only:
        return
    # 2. the updates
    ep_g, ep_p = gw.generate_episodes(o.envs)[0], pw.generate_episodes(o.envs)[0]
    steps = {"reinforce+g2anet": lambda i: gl.train(ep_g, i, epsilon=gw.epsilon), "reinforce": lambda i: pl.train(ep_p, i, epsilon=pw.epsilon)}
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
    print("%-5s reinforce+g2anet / reinforce  %.3f" % (shape, statistics.median(ms["reinforce+g2anet"]) / statistics.median(ms["reinforce"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shapes", nargs="+", default=["2s3z", "MMM2"])
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--peak_tflops", type=float, default=157.3)
    ap.add_argument("--head_only", action="store_true", help="stop after the head's own timings")
    o = ap.parse_args()
    for shape in o.shapes:
        one_shape(shape, o)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
