#!/usr/bin/env python3
"""Cost of a sampled training rollout on one MI355X: the same RolloutWorker over PolicyMAC on its three paths -
"unfused" (agent step, marl_policy_sample, marl_synth_step, marl_synth_observe per lock-step), "fused_step" (agent step and the
sampling fused step) and "whole" (one launch of synth_rollout_kernel<AC, true>) - beside the greedy whole fp32 rollout of SharedMAC
over the same weights as the floor.  Fixed-length episodes of T steps, epsilon 0.3 without anneal, f32 mode; alternating rounds,
host clock around a device synchronise, `--rollouts` rollouts per reading."""
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
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--shapes", nargs="+", default=["2s3z", "MMM2"])
    ap.add_argument("--T", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rollouts", type=int, default=3)
    o = ap.parse_args()
    from marl_amd.controller.share_params import SharedMAC, PolicyMAC
    from marl_amd.common.arguments import get_centralv_args
    from marl_amd.rollout import RolloutWorker
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv

    for shape in o.shapes:
        for E in o.envs:
            args = bench.make_args("central_v", shape, o.T)
            args.gemm_mode, args.hip_graph = "f32", False
            get_centralv_args(args)
            args.epsilon, args.anneal_epsilon, args.min_epsilon = 0.3, 0.0, 0.3
            torch.manual_seed(0)
            pmac = PolicyMAC(args)
            smac = SharedMAC(args)
            smac.agent.load_state_dict(pmac.agent.state_dict())
            smac.cuda()

            def worker(mac, mode):
                env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit,
                                       seed=1, fixed_length=True)
                w = RolloutWorker(env, mac, args)
                w.rollout_mode = mode
                return w
            paths = {"unfused sampled": worker(pmac, "unfused"), "fused-step sampled": worker(pmac, "fused_step"),
                     "whole sampled": worker(pmac, "whole"), "whole greedy fp32": worker(smac, "whole")}
            for w in paths.values():
                w.generate_episodes(E)
            gc.collect()
            gc.disable()
            ms = {k: [] for k in paths}
            for _ in range(o.rounds):
                for k, w in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(o.rollouts):
                        w.generate_episodes(E)
                    torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t0) * 1e3 / o.rollouts)
            gc.enable()
            for k, r in ms.items():
                print("%-5s envs %5d T %d  %-19s median %8.3f ms per rollout  (min %.3f - max %.3f)"
                      % (shape, E, args.episode_limit, k, statistics.median(r), min(r), max(r)), flush=True)
            del paths


if __name__ == "__main__":
    main()
