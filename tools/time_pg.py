#!/usr/bin/env python3
"""Cost of the entropy fold and of REINFORCE on one MI355X: marl_policy_loss_bwd_ex at beta = 0.01 (with v and
ent) beside marl_policy_loss_bwd on the same rows by HIP events, in alternating rounds of one process, with the bytes each moves
over its time; and one ReinforceLearner update beside the CentralVLearner update built from the same tree (alternating rounds,
host clock around a device synchronise, the set-up of tools/time_central_v.py: fixed-length episodes, f32 mode, eager launches)."""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--beta", type=float, default=0.01)
    o = ap.parse_args()
    from marl_amd import ops
    from marl_amd.controller.share_params import PolicyMAC
    from marl_amd.algorithm.central_v import CentralVLearner
    from marl_amd.algorithm.reinforce import ReinforceLearner
    from marl_amd.common.arguments import get_centralv_args, get_reinforce_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    # the loss kernels alone
    a0 = bench.make_args("central_v", o.shape, o.T)
    B, T, N, A = o.envs, a0.episode_limit, a0.n_agents, a0.n_actions
    R = B * T * N
    dev = torch.device("cuda")
    logits, avail = torch.randn(R, A, device=dev), (torch.rand(R, A, device=dev) < 0.7).float()
    avail[:, 0] = 1.0
    u = torch.zeros(R, dtype=torch.int32, device=dev)
    G, v, padded = torch.randn(B * T, device=dev), torch.randn(B * T, device=dev), torch.zeros(B * T, device=dev)
    dl, logp, ent, st = torch.empty(R, A, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(3, device=dev)
    calls = {"policy_loss_bwd": lambda: ops.policy_loss_bwd(logits, avail, u, G, v, padded, 0.1, dl, logp, st, R, N, A),
             "policy_loss_bwd_ex": lambda: ops.policy_loss_bwd_ex(logits, avail, u, G, v, padded, 0.1, o.beta, dl, logp, ent, st, R, N, A)}
    nbytes = {"policy_loss_bwd": 4 * (R * (3 * A + 2) + 3 * B * T), "policy_loss_bwd_ex": 4 * (R * (3 * A + 3) + 3 * B * T)}
    for f in calls.values():
        for _ in range(5):
            f()
    us = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(o.rounds):
        for k, f in calls.items():
            e0.record()
            for _ in range(o.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / o.reps)
    for k, x in us.items():
        med = statistics.median(x)
        print("%-19s rows %d x %d  median %.1f us per call with its finishing launch (min %.1f - max %.1f, %d rounds of %d)  %.1f MB  "
              "%.2f TB/s" % (k, R, A, med, min(x), max(x), o.rounds, o.reps, nbytes[k] / 1e6, nbytes[k] / med / 1e6))
    print("policy_loss_bwd_ex / policy_loss_bwd  %.3f (beta = %g)" % (statistics.median(us["policy_loss_bwd_ex"]) /
                                                                  statistics.median(us["policy_loss_bwd"]), o.beta))

    # the updates
    def make(alg):
        args = bench.make_args(alg, o.shape, o.T)
        args.gemm_mode, args.hip_graph = "f32", False
        (get_centralv_args if alg == "central_v" else get_reinforce_args)(args)
        torch.manual_seed(0)
        mac = PolicyMAC(args)
        learner = (CentralVLearner if alg == "central_v" else ReinforceLearner)(mac, args)
        env = SyntheticSMACEnv(o.envs, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                               seed=1, fixed_length=True)
        w = RolloutWorker(env, mac, args)
        w.rollout_mode = "unfused"
        return learner, w

    (rl, rw), (cl, cw) = make("reinforce"), make("central_v")
    ep_r, ep_c = rw.generate_episodes(o.envs)[0], cw.generate_episodes(o.envs)[0]
    steps = {"reinforce": lambda i: rl.train(ep_r, i, epsilon=rw.epsilon), "central_v": lambda i: cl.train(ep_c, i, epsilon=cw.epsilon)}
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


if __name__ == "__main__":
    main()
