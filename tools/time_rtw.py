#!/usr/bin/env python3
"""Cost of the RTW reflection head (csrc/rtw_head.hip) in the per-step rollout: HIP-event ms per lock-step of the
fused_step rollout with an RTW controller (agent step + head + env step) and with the plain controller (no head), and the
head launch alone.
    python tools/time_rtw.py [--shape 2s3z|3s5z|MMM2] [--envs 512 4096 ...]
    tools/prof_cmd.sh rtw tools/time_rtw.py        (the kernel's own time: rtw_head_kernel in the stats)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from oracle import seeded  # noqa: E402
from marl_amd import ops  # noqa: E402
from marl_amd.controller.share_params import SharedMAC, RTWMAC  # noqa: E402
from marl_amd.rollout import RolloutWorker  # noqa: E402
from marl_amd.env.synthetic_smac import SyntheticSMACEnv  # noqa: E402


def rollout_ms(mac_cls, args, E):
    torch.manual_seed(0)
    mac = mac_cls(args)
    mac.cuda()
    env = SyntheticSMACEnv(E, args.n_agents, args.obs_shape, args.state_shape, args.n_actions, args.episode_limit, seed=1,
                           fixed_length=True)
    w = RolloutWorker(env, mac, args)
    w.rollout_mode = "fused_step"
    w.epsilon = 0.3
    w.generate_episodes(E)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(3):
        w.generate_episodes(E)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 3 / args.episode_limit, mac


def head_ms(mac, args, E):
    N, O, A = args.n_agents, args.obs_shape, args.n_actions
    dev = torch.device("cuda")
    h = torch.randn(E * N, 64, device=dev)
    obs = torch.randn(E, 2, N, O, device=dev)
    avail = torch.ones(E, 2, N, A, device=dev)
    q = torch.zeros(E * N, A, device=dev)
    w = mac.agent.rtw_weights()
    for _ in range(3):
        ops.rtw_head_act(w, h, obs, 2 * N, 0, avail, 2 * N, 0, q, E, N, O, A, True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        ops.rtw_head_act(w, h, obs, 2 * N, 0, avail, 2 * N, 0, q, E, N, O, A, True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2s3z", choices=["2s3z", "3s5z", "MMM2"])
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--T", type=int, default=20, help="lock-steps per timed rollout")
    o = ap.parse_args()
    for E in o.envs:
        args = seeded.make_args(o.shape, "qmix", episode_limit=o.T, seed=1)
        args.not_self_model = True
        base, _ = rollout_ms(SharedMAC, args, E)
        rtw, mac = rollout_ms(RTWMAC, args, E)
        print("%-5s envs %5d  per lock-step: no head %.3f ms  with head %.3f ms  (+%.3f)   head launch alone %.3f ms"
              % (o.shape, E, base, rtw, rtw - base, head_ms(mac, args, E)), flush=True)


if __name__ == "__main__":
    main()
