#!/usr/bin/env python3
"""Cost of central-V on one MI355X: the CentralVLearner update beside the VDN update built from the same tree
(alternating rounds, host clock around a device synchronise, the set-up of tools/prof_learner.py: fixed-length episodes, f32 mode,
eager launches), marl_policy_loss_bwd alone by HIP events with its bytes over time, and the per-step rollout with
ops.policy_sample beside the same per-step rollout with ops.select_actions."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shape", default="2s3z")
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--rollouts", type=int, default=3)
    o = ap.parse_args()
    from marl_amd import ops
    from marl_amd.controller.share_params import SharedMAC, PolicyMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.common.arguments import get_centralv_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph = "f32", False
        if alg == "central_v":
            get_centralv_args(args)
        torch.manual_seed(0)
        mac = (PolicyMAC if alg == "central_v" else SharedMAC)(args)
        learner = (CentralVLearner if alg == "central_v" else QLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"          # both rollouts on the per-step path: select / step / observe kernels
        return args, learner, w

    (ca, cl, cw), (va, vl, vw) = make("central_v"), make("vdn")
    ep_c, ep_v = cw.generate_episodes(o.envs)[0], vw.generate_episodes(o.envs)[0]
    steps = {"central_v": lambda i: cl.train(ep_c, i, epsilon=cw.epsilon), "vdn": lambda i: vl.train(ep_v, i)}
    for f in steps.values():
        for i in range(3):
            f(i)
    gc.collect()
    gc.disable()
    rates = {k: [] for k in steps}
    for _ in range(o.rounds):
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(o.updates):
                f(i)
            torch.cuda.synchronize()
            rates[k].append(o.updates / (time.perf_counter() - t0))
    for k, r in rates.items():
        print("%-10s update  envs %d  median %.1f /s  (min %.1f - max %.1f)" % (k, o.envs, statistics.median(r), min(r), max(r)))

    # the loss kernel alone
    B, T, N, A = o.envs, ca.episode_limit, ca.n_agents, ca.n_actions
    R = B * T * N
    dev = torch.device("cuda")
    logits, avail = torch.randn(R, A, device=dev), (torch.rand(R, A, device=dev) < 0.7).float()
    avail[:, 0] = 1.0
    u = torch.zeros(R, dtype=torch.int32, device=dev)
    G, v, padded = torch.randn(B * T, device=dev), torch.randn(B * T, device=dev), torch.zeros(B * T, device=dev)
    dl, logp, st = torch.empty(R, A, device=dev), torch.empty(R, device=dev), torch.empty(2, device=dev)
    call = lambda: ops.policy_loss_bwd(logits, avail, u, G, v, padded, 0.1, dl, logp, st, R, N, A)
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = 4 * (R * (3 * A + 2) + 3 * B * T)
    print("policy_loss_bwd  rows %d x %d  %.1f us per call (with its finishing launch)  %.1f MB  %.2f TB/s" % (R, A, us, nbytes / 1e6, nbytes / us / 1e6))

    # the per-step rollouts
    for k, w in (("policy_sample", cw), ("select_actions", vw)):
        w.generate_episodes(o.envs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(o.rollouts):
            w.generate_episodes(o.envs)
        torch.cuda.synchronize()
        print("per-step rollout with %-15s envs %d  %.2f ms per rollout of %d steps" % (k, o.envs, (time.perf_counter() - t0) * 1e3 / o.rollouts, T))


if __name__ == "__main__":
    main()
