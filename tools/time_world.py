#!/usr/bin/env python3
"""Cost of the world-model head (csrc/world_head.hip) and of a QLearnerWithState update: HIP-event ms of the head's act-mode
and train-mode forward and its backward over B episodes x T steps, and of one full update of QLearnerWithState beside a plain
QLearner on the same device batch (qmix, fixed-length episodes, no hipGraph).
    python tools/time_world.py [--shape 2s3z|3s5z|MMM2] [--envs 512 4096] [--T 120]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import seeded  # noqa: E402
from marl_amd import ops  # noqa: E402
from marl_amd.hostutil import DeviceBatch  # noqa: E402
from marl_amd.controller.share_params import SharedMAC, SharedMACWithState  # noqa: E402
from marl_amd.algorithm.q_learner import QLearner  # noqa: E402
from marl_amd.algorithm.q_learner_state import QLearnerWithState  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2s3z", choices=["2s3z", "3s5z", "MMM2"])
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--T", type=int, default=120)
    ap.add_argument("--reps", type=int, default=10)
    o = ap.parse_args()
    dev = torch.device("cuda")
    for B in o.envs:
        args = seeded.make_args(o.shape, "qmix", episode_limit=o.T, seed=1)
        args.hip_graph = False
        N, O, A, T = args.n_agents, args.obs_shape, args.n_actions, o.T
        batch = seeded.make_batch(args, B, seed=3, lengths=[T] * B, dtype=np.float32)
        db = DeviceBatch.from_dict(batch, args, dev)
        torch.manual_seed(0)
        res = {}
        for name, mac_cls, l_cls in (("plain", SharedMAC, QLearner), ("world", SharedMACWithState, QLearnerWithState)):
            mac = mac_cls(args)
            learner = l_cls(mac, args)
            res[name] = timed(lambda: learner.train(db, 1), o.reps)
        w = learner.eval_net.agent.world_weights()
        hs = torch.randn(B, T, N, 64, device=dev)
        q = torch.zeros(B, T, N, A, device=dev)
        on = torch.randn(B, T, N, O, device=dev)
        loss = torch.zeros(1, device=dev)
        act = timed(lambda: ops.world_head_fwd(w, hs, q, B, T, N, O, A), o.reps)
        train = timed(lambda: ops.world_head_fwd(w, hs, q, B, T, N, O, A, obs=on, obs_bs=T * N, obs_t0=0, loss=loss), o.reps)
        g = learner.eval_net.agent.world_grads()
        idx = torch.zeros(B * T * N, dtype=torch.int32, device=dev)
        val = torch.randn(B * T * N, device=dev)
        dhs = torch.empty(B, T, N, 64, device=dev)
        den = torch.ones(1, device=dev)
        bwd = timed(lambda: ops.world_head_bwd(w, g, hs, idx, val, on, T * N, 0, den, 1e-6, dhs, B, T, N, O, A), o.reps)
        print("%-5s envs %5d T %3d  head: act fwd %.3f ms  train fwd %.3f ms  bwd %.3f ms   update: QLearner %.3f ms  "
              "QLearnerWithState %.3f ms (x%.2f)" % (o.shape, B, T, act, train, bwd, res["plain"], res["world"],
                                                     res["world"] / res["plain"]), flush=True)


if __name__ == "__main__":
    main()
