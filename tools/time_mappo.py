#!/usr/bin/env python3
"""Cost of MAPPO on one MI355X: the PPOLearner update at ppo_epochs = 5 beside the CentralVLearner update built
from the same tree (alternating rounds, host clock around a device synchronise, the set-up of tools/time_central_v.py: T = 120,
fixed-length episodes, f32 mode, eager launches), marl_ppo_loss_bwd beside marl_policy_loss_bwd_ex at the same rows by HIP events
with their bytes over time, and marl_masked_standardize alone."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def events(call, reps=50, warm=5):
    """microseconds per call by HIP events"""
    for _ in range(warm):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--shapes", default="2s3z,MMM2")
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=5)
    o = ap.parse_args()
    from marl_amd import ops
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.ppo import PPOLearner
    from marl_amd.common.arguments import get_centralv_args, get_mappo_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    dev = torch.device("cuda")

    for shape in o.shapes.split(","):
        def make(alg):
            args = bench.make_args(alg, shape, o.T)
            args.gemm_mode, args.hip_graph = "f32", False
            if alg == "mappo":
                get_mappo_args(args)
                args.ppo_epochs = o.epochs
            else:
                get_centralv_args(args)
            torch.manual_seed(0)
            mac = PolicyMAC(args)
            learner = (PPOLearner if alg == "mappo" else CentralVLearner)(mac, args)
            env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                                   seed=1, fixed_length=True)
            return args, learner, RolloutWorker(env, mac, args)

        (pa, pl, pw), (ca, cl, cw) = make("mappo"), make("central_v")
        ep_p, ep_c = pw.generate_episodes(o.envs)[0], cw.generate_episodes(o.envs)[0]
        steps = {"mappo": lambda i: pl.train(ep_p, i, epsilon=pw.epsilon), "central_v": lambda i: cl.train(ep_c, i, epsilon=cw.epsilon)}
        for f in steps.values():
            for i in range(2):
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
        for k, r in ms.items():
            print("%-5s %-10s update  envs %d  T %d  %s median %.2f ms  (min %.2f - max %.2f)" % (
                shape, k, o.envs, pa.episode_limit, "epochs %d " % o.epochs if k == "mappo" else "", statistics.median(r), min(r), max(r)))
        print("%-5s mappo / central_v  %.2f" % (shape, statistics.median(ms["mappo"]) / statistics.median(ms["central_v"])))

        # the loss kernels alone, at the same rows
        B, T, N, A = o.envs, pa.episode_limit, pa.n_agents, pa.n_actions
        R, BT = B * T * N, B * T
        logits, avail = torch.randn(R, A, device=dev), (torch.rand(R, A, device=dev) < 0.7).float()
        avail[:, 0] = 1.0
        u = torch.zeros(R, dtype=torch.int32, device=dev)
        adv, padded = torch.randn(BT, device=dev), torch.zeros(BT, device=dev)
        dl, logp, ent, st = torch.empty(R, A, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(4, device=dev)
        ops.ppo_loss_bwd(logits, avail, u, adv, None, padded, 0.1, 0.01, 0.2, dl, logp, ent, st, R, N, A)
        old = logp + 0.1 * torch.randn(R, device=dev)
        for name, call, per_row in (
                ("ppo_loss_bwd", lambda: ops.ppo_loss_bwd(logits, avail, u, adv, old, padded, 0.1, 0.01, 0.2, dl, logp, ent, st, R, N, A), 3 * A + 3),
                ("policy_loss_bwd_ex", lambda: ops.policy_loss_bwd_ex(logits, avail, u, adv, None, padded, 0.1, 0.01, dl, logp, ent, st, R, N, A), 3 * A + 2)):
            us = events(call)
            nbytes = 4 * R * per_row
            print("%-5s %-19s rows %d x %d  %.1f us per call (with its finishing launch)  %.1f MB  %.2f TB/s" % (
                shape, name, R, A, us, nbytes / 1e6, nbytes / us / 1e6))
        x, out, s3 = torch.randn(BT, device=dev), torch.empty(BT, device=dev), torch.empty(3, device=dev)
        us = events(lambda: ops.masked_standardize(x, padded, out, s3, BT))
        print("%-5s masked_standardize  rows %d  %.1f us per call (five launches)" % (shape, BT, us))
        del pl, cl, pw, cw, ep_p, ep_c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
